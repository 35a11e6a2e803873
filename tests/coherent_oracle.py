"""numpy restatement of the coherent fold (gacq_fold_dev, csrc/gacq_cohfold.hip) and of the search chain behind it.  No GPU.

    y[d,h,i] = sum_{m<M} W[h,m] x[start[d,m] + i] exp(-2 pi i frac(f_d (j0 + start[d,m] + i) / fs))

The phase is the exact one: frac(f_d (j0 + start) / fs) in rational arithmetic on the fp64 values of f_d and fs, plus i frac-free
f_d / fs in fp64 (i < 2^17, so the product is good to 1e-14 of a cycle).  fold64 sums in complex128; fold32 evaluates the same
formula in complex64 (rotation rounded to complex64, complex64 product, complex64 running sum in the order of m) and is what the
device tolerance is measured from.  correlate / best are oracle.acq_oracle's search statements on one row at Doppler 0, B = 1."""
from fractions import Fraction

import numpy as np
import scipy.fft as _fft

from oracle import acq_oracle


def phases(f, fs, j0, starts_d, n_out):
    """fraction of a cycle, fp64 [M, n_out], in [0, 1)"""
    r = Fraction(float(f)) / Fraction(float(fs))
    base = np.array([float((r * (int(j0) + int(s))) % 1) for s in starts_d], dtype=np.float64)
    return np.mod(base[:, None] + float(r) * np.arange(n_out, dtype=np.float64)[None, :], 1.0)


def wiped(x, n_out, starts_d, f, fs, j0=0):
    """the M carrier-wiped periods of one Doppler row, complex128 [M, n_out]"""
    x = np.asarray(x)
    seg = np.stack([x[int(s):int(s) + n_out] for s in starts_d]).astype(np.complex128)
    return seg * np.exp(-2j * np.pi * phases(f, fs, j0, starts_d, n_out))


def fold64(x, n_out, starts, dopplers, fs, W, j0=0):
    W = np.asarray(W, dtype=np.float64)
    return np.stack([W @ wiped(x, n_out, st, f, fs, j0) for st, f in zip(np.asarray(starts), np.atleast_1d(dopplers))])


def fold32(x, n_out, starts, dopplers, fs, W, j0=0):
    W = np.asarray(W).astype(np.float32)
    x = np.asarray(x).astype(np.complex64)
    out = []
    for st, f in zip(np.asarray(starts), np.atleast_1d(dopplers)):
        rot = np.exp(-2j * np.pi * phases(f, fs, j0, st, n_out)).astype(np.complex64)
        acc = np.zeros((W.shape[0], n_out), dtype=np.complex64)
        for m, s in enumerate(st):
            v = x[int(s):int(s) + n_out] * rot[m]
            acc = acc + W[:, m, None] * v[None, :]
            assert acc.dtype == np.complex64
        out.append(acc)
    return np.stack(out)


def code_spectrum(sig, chips01):
    return acq_oracle.code_spectrum(chips01, sig.n, sig.pad, sig.boc)


def correlate(row, C):
    """r of acq_oracle.accumulate_row for one block at Doppler 0 (the table NCO is 1 there): ifft(C conj(fft(row)))"""
    return _fft.ifft(C * np.conj(_fft.fft(np.asarray(row, dtype=np.complex128) * acq_oracle.nco(-0.0, 0, len(row)))))


def best(sig, chips01, row):
    """(metric, idx) of acq_oracle.search on one row with doppler_search = [0.0], blocks = 1"""
    q = acq_oracle.accumulate_row(np.asarray(row, dtype=np.complex128), code_spectrum(sig, chips01), -0.0 / sig.fs, sig.n, sig.pad, 1)
    idx = int(np.argmax(q))
    return (q[idx] / np.mean(q) if sig.normalised else q[idx]), idx


def code_offset(sig, L, idx):
    c = L * (float(idx) / sig.n)
    return c % L if sig.fold else c


def chain(sig, chips01, y):
    """The coherent search on folded rows y [D, H, n_out]: (metric [D, H], idx [D, H]) and the first strictly greatest cell"""
    D, H = y.shape[:2]
    C = code_spectrum(sig, chips01)
    met = np.zeros((D, H))
    idx = np.zeros((D, H), dtype=np.int64)
    for d in range(D):
        for h in range(H):
            q = acq_oracle.accumulate_row(y[d, h], C, -0.0 / sig.fs, sig.n, sig.pad, 1)
            idx[d, h] = int(np.argmax(q))
            met[d, h] = q[idx[d, h]] / np.mean(q) if sig.normalised else q[idx[d, h]]
    d, h = np.unravel_index(int(np.argmax(met)), met.shape)
    return met, idx, int(d), int(h)
