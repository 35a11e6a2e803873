"""The definition of the cancellation (gacq_cancel_dev, include/gacq.h) restated: Python integers for everything that decides which chip
and subcarrier half a sample gets and what its carrier phase is, numpy fp64 for the rest.  No GPU.

A satellite is a dict with chips (uint8 array, 0 / 1) and kind; its segments are a cancel.SEG_DTYPE array (or anything indexable by the
same field names), ascending and not overlapping.

evaluate(..., f32=True) and estimate(..., f32=True) are the same formulas with the same integer parts but the rotation, the products
and the running subtraction in numpy float32 (the sums of the estimate stay fp64): their distance from the fp64 evaluation sets the
bounds of the device tests, as simulate_oracle.evaluate(..., f32=True) does for the simulator."""
import numpy as np

from simulate_oracle import C1, C6, M64, TMBOC_MASK, chips_fixed, to_int8, turns_fixed  # noqa: F401  (to_int8 is re-exported)


def fixed(seg, fs):
    """(F, p0, Cf, c0) of a segment"""
    return (turns_fixed(float(seg["carrier_hz"]) / fs), turns_fixed(float(seg["carrier_phase"])), chips_fixed(float(seg["code_rate_hz"]) / fs),
            chips_fixed(float(seg["code_phase"])))


def replica_parts(sat, seg, fs, lo=None, hi=None):
    """per sample j = lo .. hi - 1 of the segment (default: all of it): (w as fp64, carrier phase as a turn fraction in fp64)"""
    F, p0, Cf, c0 = fixed(seg, fs)
    chips = np.asarray(sat["chips"])
    L = len(chips)
    kind = int(sat["kind"])
    s0 = int(seg["s0"])
    lo = s0 if lo is None else int(lo)
    hi = s0 + int(seg["n"]) if hi is None else int(hi)
    w = np.empty(hi - lo, dtype=np.float64)
    turn = np.empty(hi - lo, dtype=np.float64)
    for j in range(lo, hi):
        i = j - s0
        theta = (p0 + i * F) & M64
        pos = c0 + i * Cf
        ct, frac = pos >> 64, pos & M64
        ci = ct % L
        v = 1.0 - 2.0 * float(chips[ci])
        b1 = frac >> 63
        if kind == 1:
            v = -v if b1 else v
        elif kind in (2, 3):
            b6 = ((12 * frac) >> 64) & 1
            s1, s6 = (-1.0 if b1 else 1.0), (-1.0 if b6 else 1.0)
            v = v * (C1 * s1 + C6 * s6) if kind == 2 else (v * s6 if (TMBOC_MASK >> (ci % 33)) & 1 else v * s1)
        elif kind in (4, 5):
            v = v if (kind == 4) == (b1 == 0) else 0.0
        w[j - lo] = v
        turn[j - lo] = theta / 2.0 ** 64
    return w, turn


def _rotation(w, turn, f32):
    if f32:
        ang = np.float32(2.0 * np.pi) * turn.astype(np.float32)
        w = w.astype(np.float32)
    else:
        ang = 2.0 * np.pi * turn
    return w, w * np.cos(ang), w * np.sin(ang)


def estimate(sat, seg, fs, x, in_first, f32=False):
    """A = sum x conj(r) / sum w^2 over the segment (complex128; 0 when the denominator is 0).  x: the input from sample in_first on
    (complex); f32: products in float32, sums in fp64."""
    s0, n = int(seg["s0"]), int(seg["n"])
    xs = np.asarray(x)[s0 - in_first:s0 - in_first + n]
    w, turn = replica_parts(sat, seg, fs)
    w, rr, ri = _rotation(w, turn, f32)
    xr, xi = (xs.real.astype(np.float32), xs.imag.astype(np.float32)) if f32 else (xs.real.astype(np.float64), xs.imag.astype(np.float64))
    pr, pi, ww = xr * rr + xi * ri, xi * rr - xr * ri, w * w
    if f32:
        assert pr.dtype == np.float32 and pi.dtype == np.float32 and ww.dtype == np.float32
    e = float(np.sum(ww.astype(np.float64)))
    if e == 0.0:
        return 0j
    return complex(float(np.sum(pr.astype(np.float64))) / e, float(np.sum(pi.astype(np.float64))) / e)


def evaluate(sats, segs, amps, fs, x, in_first, out_first, n_out, f32=False):
    """v(j), j = out_first .. out_first + n_out - 1: complex128, or complex64 from the float32 evaluation.  segs: one segment array
    per satellite; amps: one complex array per satellite (rounded to complex64 before use, as the device does); x: the input from
    sample in_first on (complex)."""
    xs = np.asarray(x)[out_first - in_first:out_first - in_first + n_out]
    vr = xs.real.astype(np.float32 if f32 else np.float64)
    vi = xs.imag.astype(np.float32 if f32 else np.float64)
    for sat, sg, am in zip(sats, segs, amps):
        for g, a in zip(sg, am):
            lo, hi = max(int(g["s0"]), out_first), min(int(g["s0"]) + int(g["n"]), out_first + n_out)
            if lo >= hi:
                continue
            w, turn = replica_parts(sat, g, fs, lo, hi)
            _, rr, ri = _rotation(w, turn, f32)
            a = np.complex64(a)
            ar, ai = (np.float32(a.real), np.float32(a.imag)) if f32 else (float(a.real), float(a.imag))
            sl = slice(lo - out_first, hi - out_first)
            vr[sl] = vr[sl] - (ar * rr - ai * ri)
            vi[sl] = vi[sl] - (ar * ri + ai * rr)
    if f32:
        assert vr.dtype == np.float32 and vi.dtype == np.float32
        return (vr + 1j * vi.astype(np.complex64)).astype(np.complex64)
    return vr + 1j * vi


def clip_count(int8_iq):
    """the components of an int8 output at +-127"""
    return int(np.count_nonzero(np.abs(np.asarray(int8_iq).astype(np.int16)) == 127))
