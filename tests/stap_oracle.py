"""numpy restatement of the space-time nulling definition of include/gacq.h (gacq_stap_*): the stacked samples z_e(j) = x_p(j + t_c - t),
e = p T + t, their exact block covariances, and then tests/nulling_oracle.py with M replaced by N = M T for everything that is
unchanged -- the window sum, the loading, the elimination in the header's written-out order, the quantised weights, the output rule."""
import numpy as np

import nulling_oracle as O

WQ, WQ_MAX = O.WQ, O.WQ_MAX
MAX_WEIGHTS = 56


def centre(T):
    return (int(T) - 1) // 2


def segment(x, in_first, a, n):
    """(I, Q) int64 of absolute samples a .. a + n - 1 of an array that holds samples in_first ..; samples below 0 are zeros, any other
    absent sample is an error"""
    i, q = O.split(x)
    lo, hi = max(a, 0), a + n
    I, Q = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    if hi > lo:
        if lo < in_first or hi > in_first + len(i):
            raise ValueError("short input")
        I[lo - a:], Q[lo - a:] = i[lo - in_first:hi - in_first], q[lo - in_first:hi - in_first]
    return I, Q


def stacked_rows(xs, T, in_first, a, n):
    """the 2N real rows (I and Q of every stacked element, antenna-major) over absolute samples a .. a + n - 1: int64 [2N][n]"""
    tc = centre(T)
    rows = np.empty((2 * len(xs) * T, n), dtype=np.int64)
    for p, x in enumerate(xs):
        for t in range(T):
            rows[2 * (p * T + t)], rows[2 * (p * T + t) + 1] = segment(x, in_first, a + tc - t, n)
    return rows


def block_cov(xs, T, Lb, in_first, b0, nblk):
    """C_b of blocks b0 .. b0 + nblk - 1: (re, im), int64 [nblk][N][N], through the Gram matrix of the 2N real rows.  The products are
    formed in float64, where they are exact: every entry and every partial sum is an integer below 2^53."""
    rows = stacked_rows(xs, T, in_first, b0 * Lb, nblk * Lb)
    r = rows.reshape(rows.shape[0], nblk, Lb).transpose(1, 0, 2).astype(np.float64)
    G = np.matmul(r, r.transpose(0, 2, 1))
    assert np.max(np.abs(G)) <= float(1 << 29)
    G = G.astype(np.int64)
    re = G[:, 0::2, 0::2] + G[:, 1::2, 1::2]
    im = G[:, 1::2, 0::2] - G[:, 0::2, 1::2]
    return re, im


def constraint(M, T, c=None):
    """the N-vector: the M entries on the centre taps"""
    full = np.zeros(M * T, dtype=np.complex128)
    full[centre(T)::T] = O.default_constraint(M) if c is None else np.asarray(c, dtype=np.complex128)
    return full


def needed(Lb, W, T, out_first, n_out):
    """(first, end) of the input samples that outputs out_first .. out_first + n_out - 1 need"""
    lo, hi = O.needed(Lb, W, out_first, n_out)
    return max(lo - centre(T), 0), hi + centre(T)


def supported(Lb, W, T, in_first, in_count):
    """the end of the outputs that input samples in_first .. in_first + in_count - 1 support"""
    end = in_first + in_count
    return end - centre(T) if end >= W * Lb + centre(T) else 0


def run(xs, in_first, out_first, n_out, Lb, W, T, load_shift=10, c=None, gain=1.0, complex64=False):
    """Outputs out_first .. out_first + n_out - 1 from arrays that hold the antennas' samples from in_first on.  The dict of
    nulling_oracle.run, with N = M T in the place of M."""
    M = len(xs)
    N, tc = M * T, centre(T)
    assert 1 <= M <= 8 and T % 2 == 1 and 1 <= T <= 15 and N <= MAX_WEIGHTS
    lo, hi = needed(Lb, W, T, out_first, n_out)
    n_in = min(len(np.asarray(x).view(np.int8)) // 2 for x in xs)
    if n_out <= 0 or lo < in_first or hi > in_first + n_in:
        raise ValueError("short input")
    b0, b_hi = out_first // Lb, (out_first + n_out - 1) // Lb
    pb0 = max(b0 - W, 0)
    ncov = max(b_hi, W) - pb0
    Cre, Cim = block_cov(xs, T, Lb, in_first, pb0, ncov)
    blocks = np.arange(b0, b_hi + 1)
    Rre = np.stack([Cre[max(b - W, 0) - pb0:max(b - W, 0) - pb0 + W].sum(axis=0) for b in blocks])
    Rim = np.stack([Cim[max(b - W, 0) - pb0:max(b - W, 0) - pb0 + W].sum(axis=0) for b in blocks])
    wq, s = O.weights(Rre, Rim, load_shift, constraint(M, T, c))
    bi = np.arange(out_first, out_first + n_out) // Lb - b0
    rows = stacked_rows(xs, T, in_first, out_first, n_out)
    yr = np.zeros(n_out, dtype=np.int64)
    yi = np.zeros(n_out, dtype=np.int64)
    bound = np.zeros(n_out, dtype=np.int64)
    for e in range(N):
        wr, wi = wq[bi, e, 0], wq[bi, e, 1]
        yr += wr * rows[2 * e] + wi * rows[2 * e + 1]
        yi += wr * rows[2 * e + 1] - wi * rows[2 * e]
        bound += (np.abs(wr) + np.abs(wi)) * np.maximum(np.abs(rows[2 * e]), np.abs(rows[2 * e + 1]))
    assert bound.max() < 1 << 31 and 2 * N * WQ_MAX * 128 < 1 << 31       # no order of the int32 sum can leave the range
    sc = np.float32(gain) * np.float32(2.0 ** -14)
    v = np.empty(2 * n_out, dtype=np.float32)
    v[0::2] = yr.astype(np.float32) * sc
    v[1::2] = yi.astype(np.float32) * sc
    own = blocks * Lb >= out_first
    res = {"owned": int(own.sum()), "wq": wq[own].astype(np.int32), "cov": np.stack([Rre[own], Rim[own]], axis=3), "margin": O.tie_margin(s),
           "wq_all": wq.astype(np.int32), "blocks": blocks}
    if complex64:
        res["out"], res["clipped"] = v.view(np.complex64), 0
    else:
        r = np.rint(v)
        cl = np.clip(r, -127.0, 127.0)
        res["out"], res["clipped"] = cl.astype(np.int8), int(np.count_nonzero(cl != r))
    return res
