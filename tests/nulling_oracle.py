"""numpy restatement of the spatial nulling definition of include/gacq.h (gacq_null_*): block covariances as exact integers, the window
sum, the loading, Gaussian elimination without pivoting in the header's written-out order (every real product and sum an fp64
operation of its own: numpy fuses nothing), quantised weights, the integer apply and the output rule.  Everything is vectorised over
blocks only: the operations on one block's numbers are those of the header, one by one."""
import numpy as np

WQ = 1 << 14
WQ_MAX = 131071


def split(x):
    """interleaved int8 -> (I, Q) as int64"""
    x = np.asarray(x).view(np.int8).astype(np.int64)
    return x[0::2], x[1::2]


def block_cov(xs, Lb, first, nblk):
    """C_b of blocks 0 .. nblk - 1 of the samples that begin at sample `first` of the arrays: (re, im), int64 [nblk][M][M], through the
    Gram matrix of the 2M real rows"""
    M = len(xs)
    rows = np.empty((nblk, 2 * M, Lb), dtype=np.int64)
    for p, x in enumerate(xs):
        i, q = split(x)
        rows[:, 2 * p] = i[first:first + nblk * Lb].reshape(nblk, Lb)
        rows[:, 2 * p + 1] = q[first:first + nblk * Lb].reshape(nblk, Lb)
    G = np.einsum("buj,bvj->buv", rows, rows)
    re = G[:, 0::2, 0::2] + G[:, 1::2, 1::2]
    im = G[:, 1::2, 0::2] - G[:, 0::2, 1::2]
    return re, im


def solve(Are, Aim, c):
    """A u = c for a stack of matrices, [n][M][M] float64 real and imaginary parts, c complex [M]: u as (re, im) [n][M], by the header's
    elimination and back substitution"""
    n, M = Are.shape[0], Are.shape[1]
    ar = [[Are[:, r, q].copy() for q in range(M)] for r in range(M)]
    ai = [[Aim[:, r, q].copy() for q in range(M)] for r in range(M)]
    br = [np.full(n, float(np.real(c[r]))) for r in range(M)]
    bi = [np.full(n, float(np.imag(c[r]))) for r in range(M)]
    with np.errstate(all="ignore"):
        for k in range(M):
            piv = ar[k][k]
            for r in range(k + 1, M):
                mr, mi = ar[r][k] / piv, ai[r][k] / piv
                for q in range(k + 1, M):
                    pr = mr * ar[k][q] - mi * ai[k][q]
                    pi = mr * ai[k][q] + mi * ar[k][q]
                    ar[r][q] = ar[r][q] - pr
                    ai[r][q] = ai[r][q] - pi
                pr = mr * br[k] - mi * bi[k]
                pi = mr * bi[k] + mi * br[k]
                br[r] = br[r] - pr
                bi[r] = bi[r] - pi
        ur, ui = [None] * M, [None] * M
        for k in range(M - 1, -1, -1):
            sr, si = br[k], bi[k]
            for q in range(k + 1, M):
                pr = ar[k][q] * ur[q] - ai[k][q] * ui[q]
                pi = ar[k][q] * ui[q] + ai[k][q] * ur[q]
                sr = sr - pr
                si = si - pi
            ur[k], ui[k] = sr / ar[k][k], si / ar[k][k]
    return np.stack(ur, axis=1), np.stack(ui, axis=1)


def loaded(Rre, Rim, load_shift):
    """A = R + d I as float64, d = (trace >> load_shift) + 1"""
    M = Rre.shape[1]
    t = sum(Rre[:, p, p] for p in range(M))
    d = (t >> int(load_shift)) + 1
    A = Rre.copy()
    for p in range(M):
        A[:, p, p] += d
    return A.astype(np.float64), Rim.astype(np.float64)


def default_constraint(M):
    c = np.zeros(M, dtype=np.complex128)
    c[0] = 1.0
    return c


def weights(Rre, Rim, load_shift, c):
    """(wq int64 [n][M][2], the scaled weights w 2^14 as float64 [n][M][2]) of a stack of window sums"""
    M = Rre.shape[1]
    c = np.asarray(c, dtype=np.complex128)
    Are, Aim = loaded(Rre, Rim, load_shift)
    ur, ui = solve(Are, Aim, c)
    with np.errstate(all="ignore"):
        den = None
        for p in range(M):
            t = float(c[p].real) * ur[:, p] + float(c[p].imag) * ui[:, p]
            den = t if den is None else den + t
        s = np.stack([ur / den[:, None], ui / den[:, None]], axis=2) * float(WQ)
        q = np.where(np.isfinite(s), np.clip(np.rint(s), -WQ_MAX, WQ_MAX), 0.0).astype(np.int64)
    return q, s


def tie_margin(s):
    """the smallest distance of a scaled weight component from a half-integer, where rint would turn"""
    s = s[np.isfinite(s)]
    return float(np.min(np.abs((s - np.floor(s)) - 0.5))) if s.size else 1.0


def needed(Lb, W, out_first, n_out):
    """(first, end) of the input samples that outputs out_first .. out_first + n_out - 1 need"""
    b_lo = out_first // Lb
    return max(b_lo - W, 0) * Lb, max(out_first + n_out, W * Lb)


def supported(Lb, W, in_first, in_count):
    """the end of the outputs that input samples in_first .. in_first + in_count - 1 support: all of them once W whole blocks are there"""
    return in_first + in_count if in_first + in_count >= W * Lb else 0


def run(xs, in_first, out_first, n_out, Lb, W, load_shift=10, c=None, gain=1.0, complex64=False):
    """Outputs out_first .. out_first + n_out - 1 from arrays that hold the antennas' samples from in_first on.  A dict: out (int8
    interleaved or complex64), clipped, owned, wq [owned block][M][2] int32, cov [owned block][M][M][2] int64, margin, and wq_all /
    blocks for every block the outputs meet."""
    M = len(xs)
    c = default_constraint(M) if c is None else np.asarray(c, dtype=np.complex128)
    lo, hi = needed(Lb, W, out_first, n_out)
    n_in = min(len(np.asarray(x).view(np.int8)) // 2 for x in xs)
    if n_out <= 0 or lo < in_first or hi > in_first + n_in:
        raise ValueError("short input")
    b0, b_hi = out_first // Lb, (out_first + n_out - 1) // Lb
    pb0 = max(b0 - W, 0)
    ncov = max(b_hi, W) - pb0
    Cre, Cim = block_cov(xs, Lb, pb0 * Lb - in_first, ncov)
    blocks = np.arange(b0, b_hi + 1)
    Rre = np.stack([Cre[max(b - W, 0) - pb0:max(b - W, 0) - pb0 + W].sum(axis=0) for b in blocks])
    Rim = np.stack([Cim[max(b - W, 0) - pb0:max(b - W, 0) - pb0 + W].sum(axis=0) for b in blocks])
    wq, s = weights(Rre, Rim, load_shift, c)
    j = np.arange(out_first, out_first + n_out)
    bi = j // Lb - b0
    yr = np.zeros(n_out, dtype=np.int64)
    yi = np.zeros(n_out, dtype=np.int64)
    for p, x in enumerate(xs):
        i, q = split(x)
        xr, xi = i[out_first - in_first:out_first - in_first + n_out], q[out_first - in_first:out_first - in_first + n_out]
        wr, wi = wq[bi, p, 0], wq[bi, p, 1]
        yr += wr * xr + wi * xi
        yi += wr * xi - wi * xr
    assert max(np.abs(yr).max(), np.abs(yi).max()) < 1 << 28
    sc = np.float32(gain) * np.float32(2.0 ** -14)
    v = np.empty(2 * n_out, dtype=np.float32)
    v[0::2] = yr.astype(np.float32) * sc
    v[1::2] = yi.astype(np.float32) * sc
    own = blocks * Lb >= out_first
    res = {"owned": int(own.sum()), "wq": wq[own].astype(np.int32), "cov": np.stack([Rre[own], Rim[own]], axis=3), "margin": tie_margin(s),
           "wq_all": wq.astype(np.int32), "blocks": blocks}
    if complex64:
        res["out"], res["clipped"] = v.view(np.complex64), 0
    else:
        r = np.rint(v)
        cl = np.clip(r, -127.0, 127.0)
        res["out"], res["clipped"] = cl.astype(np.int8), int(np.count_nonzero(cl != r))
    return res
