"""numpy fp64 restatement of the correlation grid of csrc/gacq_corrgrid.hip (gacq_corr_grid_dev), vectorised per block.  No GPU.

With j = s0 + m n + i the absolute sample index,
    f_d = doppler0 + (d - (D-1)/2) df,   cf = (chip_rate + doppler0/ratio) / fs,
    C[m,d,p] = sum_{i<n} x[j] exp(-2 pi i frac((carrier_hz + f_d) j / fs)) w(code0 + off[p] + cf j)
The code position is (code0 + off[p]) + cf * j, product and sum rounded separately; the subcarrier phases are 2 pos (exact) and
12 (code0 + off[p]) + (12 cf) j, as the tracking loops' chip_weight forms them from one start phase."""
import numpy as np

TMBOC_MASK = (1 << 0) | (1 << 4) | (1 << 6) | (1 << 29)


def weight(chips, kind, cpp, cf, j):
    """w at samples j (float64 array) for the start phase cpp: plain (0), BOC(1,1) (1), CBOC (2), TMBOC (3), RZ [1,0] (4), RZ [0,1] (5)"""
    L = len(chips)
    pos = cpp + cf * j
    idx = np.mod(np.floor(pos), L).astype(np.int64)
    w = 1.0 - 2.0 * chips[idx].astype(np.float64)
    if kind == 0:
        return w
    b1 = np.mod(np.floor(2.0 * cpp + (2.0 * cf) * j), 2.0)
    if kind == 1:
        return np.where(b1 != 0, -w, w)
    if kind in (2, 3):
        b6 = np.mod(np.floor(12.0 * cpp + (12.0 * cf) * j), 2.0)
        s1 = np.where(b1 != 0, -1.0, 1.0)
        s6 = np.where(b6 != 0, -1.0, 1.0)
        if kind == 2:
            return w * (0.953463 * s1 + 0.301511 * s6)
        return np.where((TMBOC_MASK >> (idx % 33)) & 1, w * s6, w * s1)
    return np.where((kind == 4) == (b1 == 0), w, 0.0)


def grid(g, chips, iq_int8):
    """C [M, D, P] complex128 of one grid (any object with the fields of gnss_dsp_tools_amd.refine.Grid) on the interleaved int8
    recording iq_int8 (numpy)."""
    off = np.asarray(g.offsets, dtype=np.float64)
    D, P, n, M = int(g.D), len(off), int(g.n), int(g.M)
    fs = float(g.fs)
    cf = (g.chip_rate + g.doppler0 / g.ratio) / fs
    fd = g.doppler0 + (np.arange(D, dtype=np.float64) - (D - 1) / 2.0) * g.df
    iq = np.asarray(iq_int8).reshape(-1)
    out = np.zeros((M, D, P), dtype=np.complex128)
    for m in range(M):
        a = int(g.s0) + m * n
        j = np.arange(a, a + n, dtype=np.float64)
        x = iq[2 * a:2 * (a + n):2].astype(np.float64) + 1j * iq[2 * a + 1:2 * (a + n):2].astype(np.float64)
        ph = np.mod((g.carrier_hz + fd)[:, None] * j[None, :] / fs, 1.0)
        v = x[None, :] * np.exp(-2j * np.pi * ph)
        W = np.stack([weight(chips, int(g.kind), g.code0 + off[p], cf, j) for p in range(P)], axis=1)
        out[m] = v @ W
    return out
