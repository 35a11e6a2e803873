"""The definition of gacq_mitigate_dev (include/gacq.h) restated in numpy: sanitise, pulse blanking, spectral excision by overlapped
sine-window frames with a lower-median threshold, gain and int8 rounding, and the statistics.  evaluate() is the fp64 oracle;
precision="f32" evaluates the same definition with every product and sum rounded to float32 (explicit radix-2 transforms; twiddles and
window rounded from fp64): its deviation from the fp64 oracle is the yardstick of the tests' value bound."""
import types

import numpy as np

MAX_HOLD, MAX_GUARD = 64, 8
AUTO_SAMPLES = 65536


def config(blank=None, hold=2, nfft=1024, ratio=12.0, guard=2):
    return types.SimpleNamespace(blank=None if not blank else float(blank), hold=int(hold), nfft=int(nfft or 0) if ratio is not None else 0,
                                 ratio=ratio, guard=int(guard))


def window(n, dtype=np.float64):
    return np.sin(np.pi * (np.arange(n, dtype=np.float64) + 0.5) / n).astype(dtype)


def to_int8(c):
    """interleaved int8 of complex64 values: clip(rint(.), -127, 127), ties to even, NaN to 0"""
    v = np.asarray(c, dtype=np.complex64).view(np.float32)
    with np.errstate(invalid="ignore"):
        r = np.clip(np.rint(v), -127.0, 127.0)
    return np.where(np.isnan(v), np.float32(0.0), r).astype(np.int8)


def samples(data, in_complex64):
    """(complex128 samples, non-finite flags) of interleaved int8 or complex64 data (bytes or arrays)"""
    if in_complex64:
        c = np.frombuffer(data, dtype=np.complex64) if isinstance(data, (bytes, bytearray, memoryview)) else np.asarray(data, dtype=np.complex64).reshape(-1)
        bad = ~(np.isfinite(c.real) & np.isfinite(c.imag))
        return np.where(bad, 0.0, c).astype(np.complex128), bad
    v = np.frombuffer(data, dtype=np.int8) if isinstance(data, (bytes, bytearray, memoryview)) else np.asarray(data, dtype=np.int8).reshape(-1)
    v = v[:len(v) // 2 * 2].astype(np.float64)
    return v[0::2] + 1j * v[1::2], np.zeros(len(v) // 2, dtype=bool)


def out_range(cfg, in_first, in_count):
    """(first, count) of the outputs that input samples in_first .. in_first + in_count - 1 support"""
    end = in_first + in_count
    if cfg.nfft:
        h = cfg.nfft // 2
        qlo = 0 if in_first == 0 else -(-(in_first + cfg.hold) // h) + 1
        qhi = (end - cfg.hold) // h - 2
        return qlo * h, max(0, (qhi + 1 - qlo) * h)
    first = 0 if in_first == 0 else in_first + cfg.hold
    return first, max(0, end - cfg.hold - first)


def needed(cfg, out_first, n_out):
    """(lo, hi) input samples that outputs out_first .. out_first + n_out - 1 need (lo clamped at 0)"""
    last = out_first + n_out - 1
    if cfg.nfft:
        h = cfg.nfft // 2
        return max(0, (out_first // h - 1) * h - cfg.hold), (last // h + 2) * h - 1 + cfg.hold
    return max(0, out_first - cfg.hold), last + cfg.hold


def lower_median(p):
    """the (N/2)-th smallest of the last axis, 1-based"""
    n = p.shape[-1]
    return np.partition(p, n // 2 - 1, axis=-1)[..., n // 2 - 1]


def _fft32(re, im, inverse):
    """radix-2 transform of the last axis in float32: every product and sum rounded, twiddles rounded from fp64; unnormalised"""
    f, n = re.shape
    bits = n.bit_length() - 1
    rev = np.array([int(format(i, "0%db" % bits)[::-1], 2) for i in range(n)])
    re, im = re[:, rev].astype(np.float32), im[:, rev].astype(np.float32)
    m = 2
    while m <= n:
        half = m // 2
        ang = (2.0 if inverse else -2.0) * np.pi * np.arange(half, dtype=np.float64) / m
        wr, wi = np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32)
        re, im = re.reshape(f, n // m, m), im.reshape(f, n // m, m)
        ar, ai, br, bi = re[:, :, :half], im[:, :, :half], re[:, :, half:], im[:, :, half:]
        tr = br * wr - bi * wi
        ti = br * wi + bi * wr
        re = np.concatenate([ar + tr, ar - tr], axis=2).reshape(f, n)
        im = np.concatenate([ai + ti, ai - ti], axis=2).reshape(f, n)
        m *= 2
    return re, im


def blank(cfg, x, bad, in_complex64):
    """(z, forced) of sanitised samples x with their non-finite flags; samples outside x count as zero"""
    forced = bad.copy()
    if cfg.blank:
        if in_complex64:
            re, im = x.real.astype(np.float32), x.imag.astype(np.float32)
            with np.errstate(over="ignore"):
                hit = re * re + im * im > np.float32(cfg.blank) * np.float32(cfg.blank)
        else:
            hit = x.real.astype(np.int64) ** 2 + x.imag.astype(np.int64) ** 2 > float(cfg.blank) ** 2
        c = np.concatenate([[0], np.cumsum(np.concatenate([np.zeros(cfg.hold, dtype=np.int64), hit.astype(np.int64), np.zeros(cfg.hold, dtype=np.int64)]))])
        forced |= (c[2 * cfg.hold + 1:] - c[:len(x)]) > 0
    return np.where(forced, 0.0, x), forced


def evaluate(cfg, data, gain, in_complex64=False, in_first=0, out_first=None, n_out=None, precision="f64"):
    """Outputs out_first .. out_first + n_out - 1 (default: all that the data supports).  A namespace with
    y (complex128: y(j) times float32(gain), unrounded; with precision="f32" the float32 evaluation, widened), c64 (the complex64
    output), i8 (the int8 output), blanked, frames, bins, frame_bins (uint32 per owned frame), margin (min |P / (ratio med) - 1|)."""
    x, bad = samples(data, in_complex64)
    first, count = out_range(cfg, in_first, len(x))
    out_first = first if out_first is None else int(out_first)
    n_out = max(0, first + count - out_first) if n_out is None else int(n_out)
    g = np.float32(gain)
    res = types.SimpleNamespace(blanked=0, frames=0, bins=0, frame_bins=np.zeros(0, dtype=np.uint32), margin=np.inf)
    if n_out == 0:
        res.y, res.c64, res.i8 = np.zeros(0, dtype=np.complex128), np.zeros(0, dtype=np.complex64), np.zeros(0, dtype=np.int8)
        return res
    lo, hi = needed(cfg, out_first, n_out)
    if lo < in_first or hi >= in_first + len(x):
        raise ValueError("short input: outputs need %d .. %d, present %d .. %d" % (lo, hi, in_first, in_first + len(x) - 1))
    z, forced = blank(cfg, x, bad, in_complex64)
    res.blanked = int(np.count_nonzero(forced[out_first - in_first:out_first - in_first + n_out]))
    if not cfg.nfft:
        y = z[out_first - in_first:out_first - in_first + n_out]
    else:
        n = cfg.nfft
        h = n // 2
        q0, q1 = out_first // h, (out_first + n_out - 1) // h
        # absolute samples (q0 - 1) h .. (q1 + 2) h - 1; those below 0 (and any the data does not hold) are zero
        base = (q0 - 1) * h
        buf = np.zeros((q1 - q0 + 3) * h, dtype=np.complex128)
        a, b = max(base, in_first), min(base + len(buf), in_first + len(z))
        buf[a - base:b - base] = z[a - in_first:b - in_first]
        nf = q1 - q0 + 2                                              # frames q0 .. q1 + 1
        fr = np.stack([buf[i * h:i * h + n] for i in range(nf)])
        if precision == "f32":
            w = window(n, np.float32)
            fre, fim = fr.real.astype(np.float32) * w, fr.imag.astype(np.float32) * w
            xr, xi = _fft32(fre, fim, False)
            p = xr * xr + xi * xi
        else:
            w = window(n)
            xf = np.fft.fft(fr * w, axis=1)
            p = xf.real ** 2 + xf.imag ** 2
        med = lower_median(p)
        thr = (np.float32(cfg.ratio) if precision == "f32" else float(cfg.ratio)) * med
        hit = p > thr[:, None]
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = np.abs(p / thr[:, None] - 1.0)
        if np.any(thr > 0):
            res.margin = float(np.min(rel[thr > 0]))
        zero = np.zeros_like(hit)
        for d in range(-cfg.guard, cfg.guard + 1):
            zero |= np.roll(hit, d, axis=1)
        if precision == "f32":
            xr, xi = np.where(zero, np.float32(0), xr), np.where(zero, np.float32(0), xi)
            yr, yi = _fft32(xr, xi, True)
            inv = np.float32(1.0 / n)
            yf = ((yr * inv) * w).astype(np.complex128) + 1j * ((yi * inv) * w).astype(np.complex128)
            ysum = (yf[:-1, h:].real.astype(np.float32) + yf[1:, :h].real.astype(np.float32)).astype(np.float64) + 1j * (
                yf[:-1, h:].imag.astype(np.float32) + yf[1:, :h].imag.astype(np.float32)).astype(np.float64)
        else:
            yf = w * np.fft.ifft(np.where(zero, 0.0, xf), axis=1)
            ysum = yf[:-1, h:] + yf[1:, :h]
        y = ysum.reshape(-1)[out_first - q0 * h:out_first - q0 * h + n_out]
        fo = np.arange(q0, q1 + 2)
        own = (fo * h >= out_first) & (fo * h < out_first + n_out)
        res.frame_bins = np.count_nonzero(zero, axis=1)[own].astype(np.uint32)
        res.frames, res.bins = int(np.count_nonzero(own)), int(res.frame_bins.sum())
    c64 = np.empty(n_out, dtype=np.complex64)
    with np.errstate(over="ignore"):
        c64.real, c64.imag = y.real.astype(np.float32) * g, y.imag.astype(np.float32) * g
    res.y = c64.astype(np.complex128) if precision == "f32" else y * np.float64(g)
    res.c64, res.i8 = c64, to_int8(c64)
    return res


def auto_gain(cfg, data, in_complex64=False, target_rms=32.0):
    """target_rms over the rms of the first min(available, 65536) outputs at gain 1, from the fp64 oracle"""
    x, _ = samples(data, in_complex64)
    first, count = out_range(cfg, 0, len(x))
    p = min(count, AUTO_SAMPLES)
    y = evaluate(cfg, data, 1.0, in_complex64, 0, 0, p).y
    return float(target_rms) / float(np.sqrt(np.mean(y.real ** 2 + y.imag ** 2)))
