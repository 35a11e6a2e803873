"""The definition of the array-and-interference scene (gacq_scene_dev, include/gacq.h) restated: Python integers for every phase, gate
and noise counter, numpy fp64 for the rest.  No GPU.  What is unchanged from the single-antenna recording comes from
tests/simulate_oracle.py: the satellites' terms, Philox, the fixed-point conversions, to_int8 and the noise statistics.

A satellite is simulate_oracle's dict.  An emitter is a dict with the fields of gacq_scene_emitter: kind (0 tone, 1 sawtooth chirp,
2 triangle chirp, 3 broadband noise), amp, f0_hz, f1_hz, phase (turns), sweep, and gate = (on, period, first) or None.

evaluate(..., f32=True) is the same formula with the same integer parts but the rotations, Box-Muller, the gains, the products and the
running sums in numpy float32: its distance from the fp64 evaluation sets the bound of the device tests."""
import math

import numpy as np

from simulate_oracle import M64, noise_statistics, philox4x32_10, satellite_parts, to_int8, turns_fixed  # noqa: F401

TONE, SAWTOOTH, TRIANGLE, NOISE = 0, 1, 2, 3


def philox_words(seed, j0, n, c2, c3):
    """words r0, r1 of counter (j lo32, j hi32, c2, c3), key (seed lo32, seed hi32) for j = j0 .. j0 + n - 1 (uint64 arrays)"""
    j = np.arange(n, dtype=np.uint64) + np.uint64(j0)
    m32, s32 = np.uint64(0xffffffff), np.uint64(32)
    c0, c1 = j & m32, j >> s32
    c2 = np.full(n, int(c2), dtype=np.uint64)
    c3 = np.full(n, int(c3), dtype=np.uint64)
    k0, k1 = int(seed) & 0xffffffff, (int(seed) >> 32) & 0xffffffff
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ np.uint64(k0), p1 & m32, (p0 >> s32) ^ c3 ^ np.uint64(k1), p0 & m32
        k0, k1 = (k0 + 0x9E3779B9) & 0xffffffff, (k1 + 0xBB67AE85) & 0xffffffff
    return c0, c1


def gauss(seed, sigma, j0, n, c2, c3, f32=False):
    """Box-Muller of the draws of counter (j, c2, c3): (re, im), fp64 (or the float32 evaluation)"""
    r0, r1 = philox_words(seed, j0, n, c2, c3)
    u1 = ((r0 >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    u2 = ((r1 >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    if f32:
        u1, u2 = u1.astype(np.float32), u2.astype(np.float32)
        rad = np.float32(sigma) * np.sqrt(np.float32(-2.0) * np.log(u1))
        ang = np.float32(2.0 * np.pi) * u2
        return rad * np.cos(ang), rad * np.sin(ang)
    rad = sigma * np.sqrt(-2.0 * np.log(u1))
    return rad * np.cos(2.0 * np.pi * u2), rad * np.sin(2.0 * np.pi * u2)


def antenna_noise(seed, sigma, antenna, j0, n, f32=False):
    return gauss(seed, sigma, j0, n, antenna, 0, f32)


def jammer_noise(seed, sigma, index, j0, n, f32=False):
    return gauss(seed, sigma, j0, n, index, 1, f32)


def gate_on(j, gate):
    if gate is None or gate[1] == 0:
        return True
    on, period, first = gate
    return (j - first) % period < on                                 # Python's modulus is the non-negative one


def chirp_words(em, fs):
    """(p0, F0, R, P, H) of a chirp: R a signed integer mod 2^64; the sawtooth has H = P, so that its ramp never turns"""
    P = int(em["sweep"])
    H = P // 2 if em["kind"] == TRIANGLE else P
    x = (float(em["f1_hz"]) - float(em["f0_hz"])) / float(fs) / float(H)          # two fp64 divisions, in this order
    R = math.floor(math.ldexp(x, 64)) & M64                          # the scaling is exact
    return turns_fixed(em.get("phase", 0.0)), turns_fixed(float(em["f0_hz"]) / fs), R, P, H


def ramp(u, P, H):
    return u if u < H else P - 1 - u


def frequency_word(u, F0, R, P, H):
    return (F0 + R * ramp(u, P, H)) & M64


def ramp_sum(u, P, H):
    """T(u): the sum of ramp(t) over t < u"""
    tri = u * (u - 1) // 2
    return tri if u <= H else H * (H - 1) + (u - H) * (P - 1) - tri


def chirp_phase(j, p0, F0, R, P, H):
    """the closed form the kernel uses: theta = p0 + s Phi + u F0 + R T(u), s = j div P, u = j mod P, Phi = P F0 + R T(P)"""
    s, u = divmod(j, P)
    Phi = (P * F0 + R * ramp_sum(P, P, H)) & M64
    return (p0 + s * Phi + u * F0 + R * ramp_sum(u, P, H)) & M64


def chirp_phase_brute(j, p0, F0, R, P, H):
    """the definition: theta(j) = p0 + the sum of W(t mod P) over t < j"""
    th = p0
    for t in range(j):
        th += frequency_word(t % P, F0, R, P, H)
    return th & M64


def chirp_phase_by_sweeps(j, p0, F0, R, P, H):
    """the same sum without the closed form of T: whole sweeps times the brute-force sum of one sweep, then the rest of the last sweep"""
    words = [frequency_word(u, F0, R, P, H) for u in range(P)]
    s, u = divmod(j, P)
    return (p0 + s * (sum(words) & M64) + sum(words[:u])) & M64


def emitter_parts(em, fs, j0, n):
    """a tone or chirp per sample: (gated amplitude as fp64, phase as a turn fraction in fp64)"""
    a = np.empty(n, dtype=np.float64)
    turn = np.empty(n, dtype=np.float64)
    gate = em.get("gate")
    if em["kind"] == TONE:
        p0, F0 = turns_fixed(em.get("phase", 0.0)), turns_fixed(float(em["f0_hz"]) / fs)
    else:
        p0, F0, R, P, H = chirp_words(em, fs)
    for i in range(n):
        j = j0 + i
        theta = (p0 + j * F0) & M64 if em["kind"] == TONE else chirp_phase(j, p0, F0, R, P, H)
        a[i] = float(em["amp"]) if gate_on(j, gate) else 0.0
        turn[i] = theta / 2.0 ** 64
    return a, turn


def source_waveforms(sats, emitters, fs, seed, j0, n, f32=False):
    """z_e(j) of every source, satellites first: a list of (re, im) arrays, fp64 or float32"""
    out = []
    for sat in sats:
        a, turn, _, _, _ = satellite_parts(sat, fs, j0, n)
        out.append((a, turn))
    for i, em in enumerate(emitters):
        if em["kind"] == NOISE:
            re, im = jammer_noise(seed, float(em["amp"]), i, j0, n, f32)
            on = np.array([gate_on(j0 + k, em.get("gate")) for k in range(n)])
            out.append((np.where(on, re, 0).astype(re.dtype), np.where(on, im, 0).astype(im.dtype), None))
        else:
            out.append(emitter_parts(em, fs, j0, n))
    z = []
    for w in out:
        if len(w) == 3:
            z.append(w[:2])
        elif f32:
            ang = np.float32(2.0 * np.pi) * w[1].astype(np.float32)
            a = w[0].astype(np.float32)
            z.append((a * np.cos(ang), a * np.sin(ang)))
        else:
            ang = 2.0 * np.pi * w[1]
            z.append((w[0] * np.cos(ang), w[0] * np.sin(ang)))
    return z


def evaluate(sats, emitters, gains, fs, sigma, seed, first_antenna, j0, n, f32=False):
    """v_a(j) for the antennas first_antenna .. first_antenna + M - 1 (M = rows of gains [M, K + I]) and j = j0 .. j0 + n - 1:
    complex128 [M, n], or complex64 from the float32 evaluation"""
    g = np.asarray(gains, dtype=np.complex128).reshape(-1, len(sats) + len(emitters)) if len(sats) + len(emitters) else np.zeros((len(gains), 0))
    z = source_waveforms(sats, emitters, fs, seed, j0, n, f32)
    real = np.float32 if f32 else np.float64
    rows = []
    for p in range(g.shape[0]):
        vr, vi = antenna_noise(seed, sigma, first_antenna + p, j0, n, f32)
        for e, (zr, zi) in enumerate(z):
            gr, gi = real(np.float32(g[p, e].real)), real(np.float32(g[p, e].imag))          # rounded once to float
            vr, vi = vr + (gr * zr - gi * zi), vi + (gr * zi + gi * zr)
        assert vr.dtype == real and vi.dtype == real
        rows.append((vr + 1j * vi.astype(np.complex64 if f32 else np.complex128)).astype(np.complex64 if f32 else np.complex128))
    return np.stack(rows)
