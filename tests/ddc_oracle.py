"""The down-converter's definition (include/gacq.h, gacq_ddc_*) restated in numpy: exact integers (int64, the phase in uint64 that wraps
as the definition's mod 2^64 does) up to the int32 -> float32 conversion and the one float32 multiply.  Nothing here comes from the
package."""
from fractions import Fraction

import numpy as np

TABLE = 4096
AUTO_SAMPLES = 65536
UNITY = 32768


def phase_increment(f_shift, fs):
    """rint(f_shift / fs 2^64) mod 2^64, exactly from the two doubles (ties to even)"""
    v = Fraction(float(f_shift)) / Fraction(float(fs)) * (1 << 64)
    lo = v.numerator // v.denominator
    rest = v - lo
    up = rest > Fraction(1, 2) or (rest == Fraction(1, 2) and lo % 2 == 1)
    return (lo + int(up)) % (1 << 64)


def signed(dp):
    return dp - (1 << 64) if dp >= (1 << 63) else dp


def rates(f_shift, D, fs, coffset):
    """(fs_out, coffset_out): the shift applied is dP_signed / 2^64 fs"""
    f_act = float(Fraction(signed(phase_increment(f_shift, fs)), 1 << 64) * Fraction(float(fs)))
    return float(fs) / D, float(coffset) - f_act


def table():
    """int16 [4096, 2]: (rint(16384 cos), rint(16384 sin)) of 2 pi t / 4096, in double"""
    ph = 2.0 * np.pi * np.arange(TABLE, dtype=np.float64) / float(TABLE)
    return np.stack([np.rint(16384.0 * np.cos(ph)), np.rint(16384.0 * np.sin(ph))], axis=1).astype(np.int16)


_TABLE = table().astype(np.int64)


def firwin_hann(ntaps, cutoff_norm):
    """scipy.signal.firwin(ntaps, cutoff_norm, window='hann'): a windowed sinc with unity gain at 0"""
    i = np.arange(ntaps, dtype=np.float64)
    m = i - 0.5 * (ntaps - 1)
    h = cutoff_norm * np.sinc(cutoff_norm * m) * (0.5 - 0.5 * np.cos(2.0 * np.pi * i / (ntaps - 1)))
    return h / h.sum()


def design_taps(D, T=None, cutoff_norm=None):
    """default taps g[-H .. H] as int64"""
    if T is None:
        T = 1 if (D == 1 and cutoff_norm is None) else 8 * D + 1
    if T == 1:
        return np.array([UNITY], dtype=np.int64)
    g = np.rint(UNITY * firwin_hann(T, 0.8 / D if cutoff_norm is None else cutoff_norm)).astype(np.int64)
    g[T // 2] += UNITY - int(g.sum())
    return g


def out_range(D, T, in_first, in_count):
    H = T // 2
    first = 0 if in_first == 0 else -(-(in_first + H) // D)
    last = (in_first + in_count - 1 - H) // D
    return first, max(0, last - first + 1)


def needed(D, T, out_first, n_out):
    """(first, last) input sample that outputs out_first .. out_first + n_out - 1 need"""
    H = T // 2
    return max(0, out_first * D - H), (out_first + n_out - 1) * D + H


def mixed(data, dp, in_first, lo, hi):
    """z(n) for n = lo .. hi as int64 [hi - lo + 1, 2]; samples below 0 are zero, every other one must be present in `data` (int8 pairs
    of the samples from in_first on)"""
    x = np.frombuffer(bytes(data), dtype=np.int8).astype(np.int64).reshape(-1, 2)
    n = np.arange(lo, hi + 1, dtype=np.int64)
    there = n >= 0
    assert there.any() and n[there][0] >= in_first and hi < in_first + len(x), "an input that is needed is not present"
    xr, xi = np.zeros(len(n), dtype=np.int64), np.zeros(len(n), dtype=np.int64)
    xr[there], xi[there] = x[n[there] - in_first, 0], x[n[there] - in_first, 1]
    with np.errstate(over="ignore"):
        phase = np.where(there, n, 0).astype(np.uint64) * np.uint64(dp)                 # wraps mod 2^64
    t = (phase >> np.uint64(52)).astype(np.int64)
    c, s = _TABLE[t, 0], _TABLE[t, 1]
    pr, pi = xr * c + xi * s, xi * c - xr * s                                            # x conj(W)
    return np.stack([(pr + 64) >> 7, (pi + 64) >> 7], axis=1)


def accumulate(data, dp, D, taps, in_first, out_first, n_out):
    """acc(m), m = out_first .. out_first + n_out - 1, int64 [n_out, 2]"""
    g = np.asarray(taps, dtype=np.int64)
    T = len(g)
    H = T // 2
    assert T % 2 == 1 and int(np.abs(g).sum()) <= 65536
    lo, hi = out_first * D - H, (out_first + n_out - 1) * D + H
    z = mixed(data, dp, in_first, lo, hi)
    assert np.max(np.abs(z)) <= 23171
    win = np.lib.stride_tricks.sliding_window_view(z, T, axis=0)[::D]                    # [n_out, 2, T]: z(m D - H .. m D + H)
    acc = win @ g[::-1]                                                                  # g[k] meets z(m D - k)
    assert acc.shape == (n_out, 2) and np.max(np.abs(acc)) < 2 ** 31
    return acc


def scale(gain):
    return np.float32(gain) * np.float32(2.0 ** -22)


def to_int8(c64):
    v = np.ascontiguousarray(c64).view(np.float32)
    return np.clip(np.rint(v), -127, 127).astype(np.int8)


def evaluate(f_shift, fs, D, taps, data, gain, in_first=0, out_first=0, n_out=None, dtype="int8", dp=None):
    """the outputs as complex64 [n_out] or interleaved int8 [2 n_out]"""
    dp = phase_increment(f_shift, fs) if dp is None else dp
    if n_out is None:
        first, count = out_range(D, len(taps), in_first, len(bytes(data)) // 2)
        n_out = first + count - out_first
    acc = accumulate(data, dp, D, taps, in_first, out_first, n_out)
    v = acc.astype(np.float32) * scale(gain)                                            # int -> fp32 to nearest even, one multiply
    c = np.ascontiguousarray(v).view(np.complex64).reshape(-1)
    return c if dtype == "complex64" else to_int8(c)


def auto_gain(f_shift, fs, D, taps, data, target_rms=32.0):
    first, count = out_range(D, len(taps), 0, len(bytes(data)) // 2)
    u = evaluate(f_shift, fs, D, taps, data, 1.0, 0, 0, min(count, AUTO_SAMPLES), "complex64")
    power = float(np.mean(u.real.astype(np.float64) ** 2 + u.imag.astype(np.float64) ** 2))
    return float(target_rms) / float(np.sqrt(power))


def response_db(taps, D, f_over_fs_out):
    """|G(f)| / 32768 in dB at frequencies given in units of the output rate"""
    g = np.asarray(taps, dtype=np.float64)
    k = np.arange(len(g), dtype=np.float64) - len(g) // 2
    w = 2.0 * np.pi * np.asarray(f_over_fs_out, dtype=np.float64)[:, None] / D
    return 20.0 * np.log10(np.maximum(np.abs(np.exp(-1j * w * k[None, :]) @ g) / UNITY, 1e-12))
