"""numpy restatement of the bearing definition of include/gacq.h (gacq_bearing_*): the loading of nulling_oracle, the elimination of its
solve() in the same loop order with b = a_g (every real product and sum an fp64 operation of its own: numpy fuses nothing), no back
substitution, the quadratic form summed left to right, eligibility, the floor and the K peaks under the exclusion rule.  q() is
vectorised over blocks and cells only: the operations on one cell's numbers are those of the header, one by one."""
import numpy as np

import nulling_oracle as N

PEAK = np.dtype([("cell", "<i4"), ("zero", "<i4"), ("q", "<f8")])


def q(Rre, Rim, load_shift, a):
    """q_g of a stack of window sums, int64 [n][M][M] real and imaginary parts, over the cells of a, complex [G][M]: float64 [n][G]"""
    a = np.asarray(a, dtype=np.complex128)
    n, M = Rre.shape[0], Rre.shape[1]
    Are, Aim = N.loaded(Rre, Rim, load_shift)
    ar = [[Are[:, r, c].copy()[:, None] for c in range(M)] for r in range(M)]
    ai = [[Aim[:, r, c].copy()[:, None] for c in range(M)] for r in range(M)]
    br = [np.repeat(a[None, :, r].real, n, axis=0) for r in range(M)]
    bi = [np.repeat(a[None, :, r].imag, n, axis=0) for r in range(M)]
    with np.errstate(all="ignore"):
        for k in range(M):
            piv = ar[k][k]
            for r in range(k + 1, M):
                mr, mi = ar[r][k] / piv, ai[r][k] / piv
                for c in range(k + 1, M):
                    pr = mr * ar[k][c] - mi * ai[k][c]
                    pi = mr * ai[k][c] + mi * ar[k][c]
                    ar[r][c] = ar[r][c] - pr
                    ai[r][c] = ai[r][c] - pi
                pr = mr * br[k] - mi * bi[k]
                pi = mr * bi[k] + mi * br[k]
                br[r] = br[r] - pr
                bi[r] = bi[r] - pi
        out = None
        for k in range(M):
            t = (br[k] * br[k] + bi[k] * bi[k]) / ar[k][k]
            out = t if out is None else out + t
    return np.where(np.isnan(out), np.float64("nan"), out)          # the header's one NaN, 0x7FF8000000000000


def eligible(qs):
    with np.errstate(all="ignore"):
        return np.isfinite(qs) & (qs > 0.0)


def floor(qs):
    """the largest eligible q of every row, +inf where there is none"""
    ok = eligible(qs)
    return np.where(ok.any(axis=1), np.max(np.where(ok, qs, -np.inf), axis=1), np.inf)


def dots(u, g):
    """(u_c[0] u_g[0] + u_c[1] u_g[1]) + u_c[2] u_g[2] for every cell c"""
    u = np.asarray(u, dtype=np.float64)
    return (u[:, 0] * u[g, 0] + u[:, 1] * u[g, 1]) + u[:, 2] * u[g, 2]


def peaks(qs, u, K, cos_sep):
    """the records [n][K] of a stack of spectra"""
    qs = np.asarray(qs, dtype=np.float64)
    out = np.zeros((qs.shape[0], K), dtype=PEAK)
    out["cell"], out["q"] = -1, np.inf
    for i in range(qs.shape[0]):
        left = eligible(qs[i:i + 1])[0]
        for k in range(K):
            if not left.any():
                break
            g = int(np.argmin(np.where(left, qs[i], np.inf)))          # the first of equal minima
            out[i, k] = (g, 0, qs[i, g])
            left &= ~(dots(u, g) >= cos_sep)
    return out


def run(Rre, Rim, load_shift, a, u, K, cos_sep):
    """(records [n][K], floor [n], q [n][G])"""
    qs = q(Rre, Rim, load_shift, a)
    return peaks(qs, u, K, cos_sep), floor(qs), qs


def window_sums(xs, Lb, W, blocks):
    """R_b of the given absolute blocks of whole recordings (from sample 0): (re, im) int64 [len(blocks)][M][M]"""
    hi = max(max(blocks), W)
    Cre, Cim = N.block_cov(xs, Lb, 0, hi)
    Rre = np.stack([Cre[max(b - W, 0):max(b - W, 0) + W].sum(axis=0) for b in blocks])
    Rim = np.stack([Cim[max(b - W, 0):max(b - W, 0) + W].sum(axis=0) for b in blocks])
    return Rre, Rim


def evaluated(Lb, out_first, n_out, every):
    """the absolute blocks a call that owns outputs out_first .. out_first + n_out - 1 evaluates: owned, and a multiple of `every`"""
    lo, hi = -(-out_first // Lb), -(-(out_first + n_out) // Lb)
    return [b for b in range(lo, hi) if b % every == 0] if n_out > 0 else []
