"""The definition of the synthetic recording (gacq_simulate_dev, include/gacq.h) restated: Python integers for everything that decides
which chip, subcarrier half, symbol or noise draw a sample gets, numpy fp64 for the rest.  No GPU.

A scene's satellite is a dict with the fields of gacq_sim_sat: chips (uint8 array, 0 / 1), kind, amp, carrier_hz, carrier_phase
(turns), code_rate_hz, code_phase (chips at j = 0), and optionally symbols (+-1) with periods_per_symbol.

evaluate(..., f32=True) is the same formula with the same integer parts but the rotation, Box-Muller and the running sum in numpy
float32: its distance from the fp64 evaluation sets the bound of the device tests."""
import math

import numpy as np

M64 = (1 << 64) - 1
TMBOC_MASK = (1 << 0) | (1 << 4) | (1 << 6) | (1 << 29)
C1, C6 = 0.953463, 0.301511


def philox4x32_10(counter, key):
    """One block: counter (4 words), key (2 words) -> 4 words, Python integers."""
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & 0xffffffff, (p0 >> 32) ^ c3 ^ k1, p0 & 0xffffffff
        k0, k1 = (k0 + 0x9E3779B9) & 0xffffffff, (k1 + 0xBB67AE85) & 0xffffffff
    return c0, c1, c2, c3


def philox_words(seed, j0, n):
    """words r0, r1 of counter (j lo32, j hi32, 0, 0), key (seed lo32, seed hi32) for j = j0 .. j0 + n - 1, vectorised (uint64 arrays)"""
    j = np.arange(n, dtype=np.uint64) + np.uint64(j0)
    m32 = np.uint64(0xffffffff)
    s32 = np.uint64(32)
    c0, c1 = j & m32, j >> s32
    c2 = np.zeros(n, dtype=np.uint64)
    c3 = np.zeros(n, dtype=np.uint64)
    k0, k1 = int(seed) & 0xffffffff, (int(seed) >> 32) & 0xffffffff
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ np.uint64(k0), p1 & m32, (p0 >> s32) ^ c3 ^ np.uint64(k1), p0 & m32
        k0, k1 = (k0 + 0x9E3779B9) & 0xffffffff, (k1 + 0xBB67AE85) & 0xffffffff
    return c0, c1


def turns_fixed(v):
    """floor(frac(v) 2^64) mod 2^64, in IEEE double operations"""
    v = float(v)
    return int(math.floor(math.ldexp(v - math.floor(v), 64))) & M64


def chips_fixed(v):
    """floor(v 2^64) of v >= 0 with the whole and the fractional part split before the ldexp"""
    v = float(v)
    w = math.floor(v)
    return (int(w) << 64) + int(math.floor(math.ldexp(v - w, 64)))


def fixed(sat, fs):
    """(F, p0, Cf, c0) of a satellite"""
    return (turns_fixed(sat["carrier_hz"] / fs), turns_fixed(sat.get("carrier_phase", 0.0)), chips_fixed(sat["code_rate_hz"] / fs),
            chips_fixed(sat["code_phase"]))


def noise(seed, sigma, j0, n, f32=False):
    """(nI, nQ), fp64 (or the float32 evaluation)"""
    r0, r1 = philox_words(seed, j0, n)
    u1 = ((r0 >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    u2 = ((r1 >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    if f32:
        u1, u2 = u1.astype(np.float32), u2.astype(np.float32)
        rad = np.float32(sigma) * np.sqrt(np.float32(-2.0) * np.log(u1))
        ang = np.float32(2.0 * np.pi) * u2
        return rad * np.cos(ang), rad * np.sin(ang)
    rad = sigma * np.sqrt(-2.0 * np.log(u1))
    return rad * np.cos(2.0 * np.pi * u2), rad * np.sin(2.0 * np.pi * u2)


def satellite_parts(sat, fs, j0, n):
    """per sample: (amplitude amp w d as fp64, carrier phase as a turn fraction in fp64, chip index, period, subchip fraction (ints))"""
    F, p0, Cf, c0 = fixed(sat, fs)
    chips = np.asarray(sat["chips"])
    L = len(chips)
    kind = int(sat["kind"])
    sym = sat.get("symbols")
    pps = int(sat.get("periods_per_symbol", 1))
    a = np.empty(n, dtype=np.float64)
    turn = np.empty(n, dtype=np.float64)
    idx, per, fr = [], [], []
    for i in range(n):
        j = j0 + i
        theta = (p0 + j * F) & M64
        pos = c0 + j * Cf
        ct, frac = pos >> 64, pos & M64
        ci, period = ct % L, ct // L
        w = 1.0 - 2.0 * float(chips[ci])
        b1 = frac >> 63
        if kind == 1:
            w = -w if b1 else w
        elif kind in (2, 3):
            b6 = ((12 * frac) >> 64) & 1
            s1, s6 = (-1.0 if b1 else 1.0), (-1.0 if b6 else 1.0)
            if kind == 2:
                w = w * (C1 * s1 + C6 * s6)
            else:
                w = w * s6 if (TMBOC_MASK >> (ci % 33)) & 1 else w * s1
        elif kind in (4, 5):
            w = w if (kind == 4) == (b1 == 0) else 0.0
        d = 1.0 if sym is None or len(sym) == 0 else float(sym[(period // pps) % len(sym)])
        a[i] = float(sat["amp"]) * w * d
        turn[i] = theta / 2.0 ** 64
        idx.append(ci)
        per.append(period)
        fr.append(frac)
    return a, turn, idx, per, fr


def evaluate(sats, fs, sigma, seed, j0, n, f32=False):
    """v(j), j = j0 .. j0 + n - 1: complex128, or complex64 from the float32 evaluation"""
    nr, ni = noise(seed, sigma, j0, n, f32)
    for sat in sats:
        a, turn, _, _, _ = satellite_parts(sat, fs, j0, n)
        if f32:
            ang = np.float32(2.0 * np.pi) * turn.astype(np.float32)
            a = a.astype(np.float32)
        else:
            ang = 2.0 * np.pi * turn
        nr = nr + a * np.cos(ang)
        ni = ni + a * np.sin(ang)
    if f32:
        assert nr.dtype == np.float32 and ni.dtype == np.float32
        return (nr + 1j * ni.astype(np.complex64)).astype(np.complex64)
    return nr + 1j * ni


def to_int8(v):
    """interleaved int8 of complex values: clip(rint(.), -127, 127), ties to even"""
    out = np.empty(2 * len(v), dtype=np.int8)
    out[0::2] = np.clip(np.rint(np.real(v)), -127, 127).astype(np.int8)
    out[1::2] = np.clip(np.rint(np.imag(v)), -127, 127).astype(np.int8)
    return out


def noise_statistics(nr, ni, sigma):
    """(|mean I|, |mean Q|, |s^2/sigma^2 - 1| of I and of Q, |lag-1 autocorrelation of I|, |I Q correlation|) and their 5-sigma bounds"""
    nr, ni = np.asarray(nr, dtype=np.float64), np.asarray(ni, dtype=np.float64)
    n = len(nr)
    got = dict(mean_i=abs(nr.mean()), mean_q=abs(ni.mean()), var_i=abs(nr.var() / sigma ** 2 - 1.0), var_q=abs(ni.var() / sigma ** 2 - 1.0),
               lag1=abs(np.mean(nr[1:] * nr[:-1]) / nr.var()), iq=abs(np.mean(nr * ni) / (nr.std() * ni.std())))
    cap = dict(mean_i=5.0 * sigma / math.sqrt(n), mean_q=5.0 * sigma / math.sqrt(n), var_i=5.0 * math.sqrt(2.0 / n), var_q=5.0 * math.sqrt(2.0 / n),
               lag1=5.0 / math.sqrt(n), iq=5.0 / math.sqrt(n))
    return got, cap
