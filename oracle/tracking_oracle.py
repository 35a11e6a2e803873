"""CPU ORACLE -- TEST INFRASTRUCTURE ONLY.  Sequential restatement of the reference's tracking correlators
(gnsstools/gps/ca.py:120-128 plain; gps/l1cd.py:101-112 BOC(1,1); galileo/e1b.py:45-58 CBOC; gps/l1cp.py:210-228 TMBOC;
gps/l2cm.py:81-92 and gps/l2cl.py RZ), phases advanced by repeated fp64 addition exactly like the reference.
Pinned by tests/golden/tracking_cases.json (tools/make_goldens_tracking.py ran the reference functions)."""
import math
from fractions import Fraction

import numpy as np

from . import codes_oracle

BOC11 = (1.0, -1.0)
TMBOC = (1, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0)
KIND = {"gps.l1cd": 1, "beidou.b1cd": 1, "beidou.b1cp": 1, "galileo.e1b": 2, "galileo.e1c": 2, "gps.l1cp": 3, "gps.l2cm": 4,
        "gps.l2cl": 5}


def correlate(code, x, prn, chips, frac, incr):
    c = codes_oracle.chips(code, prn)
    L = len(c)
    kind = KIND.get(code, 0)
    p = 0.0j
    cp = (chips + frac) % L
    bp = (2 * (chips + frac)) % 2
    bp6 = (12 * (chips + frac)) % 2
    for i in range(len(x)):
        w = 1.0 - 2.0 * c[int(cp)]
        if kind == 1:
            w *= BOC11[int(bp)]
        elif kind == 2:
            w *= 0.953463 * BOC11[int(bp)] + 0.301511 * BOC11[int(bp6)]
        elif kind == 3:
            w *= BOC11[int(bp6)] if TMBOC[int(cp % 33)] else BOC11[int(bp)]
        elif kind == 4:
            w *= (1.0, 0.0)[int(bp)]
        elif kind == 5:
            w *= (0.0, 1.0)[int(bp)]
        p += x[i] * w
        cp = (cp + incr) % L
        bp = (bp + 2 * incr) % 2
        bp6 = (bp6 + 12 * incr) % 2
    return p


def _start(L, chips, frac):
    """cp, bp, bp6 at sample 0, the sequential correlate()'s own expressions (Python's floored %)."""
    s = float(chips) + float(frac)
    return s % L, (2 * s) % 2, (12 * s) % 2


def _floor_single_rounded(a, c, n):
    """floor(fl(c + a*i)) for i = 0..n-1, fl() one rounding of the exact value -- the device's v_fma_f64.  numpy forms c + a*i with two
    roundings; the floors can differ only where a rounding happened and the value is within an ulp of an integer.  Those samples
    (found with the exact error terms of the product and the sum) are redone in exact rational arithmetic."""
    i = np.arange(n, dtype=np.float64)
    p = a * i
    pos = c + p
    out = np.floor(pos)
    # Dekker's product error and Knuth's sum error: both zero <=> c + a*i was formed without rounding
    split = 134217729.0
    ah = split * a - (split * a - a)
    al = a - ah
    ih = split * i - (split * i - i)
    il = i - ih
    e_mul = ((ah * ih - p) + ah * il + al * ih) + al * il
    bb = pos - c
    e_add = (c - (pos - bb)) + (p - bb)
    near = np.nonzero((np.abs(pos - np.round(pos)) < 1e-6) & ((e_mul != 0) | (e_add != 0)))[0]
    if len(near):
        fa, fc = Fraction(a), Fraction(c)
        out[near] = [math.floor(float(fa * int(j) + fc)) for j in near]        # float(Fraction) rounds correctly
    return out.astype(np.int64)


def closed_form_indices(L, chips, frac, incr, n):
    """(int(cp), int(bp), int(bp6)) of samples 0..n-1 in closed form, as gacq_tracking.hip forms them: floor(cp0 + incr*i) mod L,
    floor(bp0 + (2 incr)*i) mod 2, floor(bp60 + (12 incr)*i) mod 2, where 12 incr is rounded first and each sum-of-product is a
    single fused rounding."""
    cp0, bp0, bp60 = _start(L, chips, frac)
    incr = float(incr)
    idx = np.mod(_floor_single_rounded(incr, cp0, n), L)
    b1 = np.mod(_floor_single_rounded(2.0 * incr, bp0, n), 2)
    b6 = np.mod(_floor_single_rounded(12.0 * incr, bp60, n), 2)
    return idx, b1, b6


def sequential_indices(L, chips, frac, incr, n):
    """The same three index sequences as correlate() walks them (phases advanced by repeated fp64 addition and %), for K correlators
    at once: [K, n] int arrays.  One numpy step per sample -- for checking that closed_form_indices agrees on a given case."""
    chips, frac, incr = np.broadcast_arrays(np.atleast_1d(chips), np.atleast_1d(frac), np.atleast_1d(incr))
    start = [_start(L, c, f) for c, f in zip(chips, frac)]
    cp = np.array([s[0] for s in start])
    bp = np.array([s[1] for s in start])
    bp6 = np.array([s[2] for s in start])
    incr = incr.astype(np.float64)
    idx = np.empty((n, len(cp)), dtype=np.int32)
    b1 = np.empty((n, len(cp)), dtype=np.int8)
    b6 = np.empty((n, len(cp)), dtype=np.int8)
    for i in range(n):
        idx[i], b1[i], b6[i] = cp, bp, bp6                       # int() of a non-negative phase: the assignments truncate
        cp = np.mod(cp + incr, L)
        bp = np.mod(bp + 2 * incr, 2)
        bp6 = np.mod(bp6 + 12 * incr, 2)
    return idx.T, b1.T, b6.T


def correlate_many(code, x, prns, chips, frac, incr, chips01=None):
    """correlate() for K (prn, chips, frac, incr) correlators over one block, vectorised over the samples with the closed-form
    phases of closed_form_indices (the device kernel's); fp64 weights and sums.  complex128[K].
    chips01: a {0,1} table used instead of every correlator's own code (a deliberately corrupted one, for sensitivity checks)."""
    prns, chips, frac, incr = np.broadcast_arrays(np.atleast_1d(prns), np.atleast_1d(chips), np.atleast_1d(frac), np.atleast_1d(incr))
    kind = KIND.get(code, 0)
    x = np.asarray(x, dtype=np.complex128)
    out = np.empty(len(prns), dtype=np.complex128)
    tmboc = np.array(TMBOC, dtype=bool)
    for k in range(len(prns)):
        c = codes_oracle.chips(code, int(prns[k])) if chips01 is None else np.asarray(chips01)
        idx, b1, b6 = closed_form_indices(len(c), chips[k], frac[k], incr[k], len(x))
        s1 = 1.0 - 2.0 * b1                                      # BOC11[int(bp)]
        s6 = 1.0 - 2.0 * b6                                      # BOC11[int(bp6)]
        w = 1.0 - 2.0 * c[idx].astype(np.float64)
        if kind == 1:
            w *= s1
        elif kind == 2:
            w *= 0.953463 * s1 + 0.301511 * s6
        elif kind == 3:
            w *= np.where(tmboc[idx % 33], s6, s1)
        elif kind == 4:
            w *= (b1 == 0)
        elif kind == 5:
            w *= (b1 == 1)
        out[k] = np.dot(x.real, w) + 1j * np.dot(x.imag, w)
    return out
