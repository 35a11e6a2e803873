"""The definition of the level control and requantiser (gacq_requant_*, include/gacq.h) restated with Python integers and numpy:
unsigned 64-bit integers for the block powers, their sliding sums and the comparisons with the thresholds, numpy float32 for the one
multiply by the gain and the rounding.  No GPU, and nothing of the package: the gain and threshold tables are handed over, as they are
to the library.

A configuration is a dict: in_bits 8 | 16, container 's8' | 'u8' | 's16' | 'f32' | 'packed', bits, msb_first, enc (packed: the code of
each level index), block, window."""
import numpy as np


def cfg(container, block, window, in_bits=8, bits=0, msb_first=True, enc=None):
    return dict(in_bits=in_bits, container=container, bits=bits, msb_first=msb_first, enc=None if enc is None else list(enc), block=block, window=window)


def enc_of_lut(lut):
    """enc[q] = the code whose value is 2q - (n - 1), of a table of the n = len(lut) values of the codes"""
    n = len(lut)
    return [list(lut).index(2 * q - (n - 1)) for q in range(n)]


def unit(c):
    """samples per output byte of packed codes; 1 otherwise"""
    return 4 // c["bits"] if c["container"] == "packed" else 1


def block_powers(c, x):
    """P(b) of every whole block of the interleaved integer samples x: uint64"""
    v = np.asarray(x).astype(np.int64).reshape(-1)
    Lb = c["block"]
    nb = (len(v) // 2) // Lb
    sq = (v[:2 * nb * Lb] ** 2).reshape(nb, 2 * Lb)
    P = sq.sum(axis=1).astype(np.uint64)
    assert all(int(p) <= Lb << 31 for p in P[:64])
    return P


def levels(c, P, nblocks, first=0, p_first=0):
    """S(b), first <= b < nblocks, as Python integers behind a uint64 array: the W powers before b, or the first W during the warm-up
    (blocks below W).  P[i] is the power of block p_first + i: every block a level sums over must be among them."""
    W = c["window"]
    cum = [0]
    for p in P.tolist():                                     # Python integers: no width to think about
        cum.append(cum[-1] + p)
    S = []
    for b in range(first, nblocks):
        lo, hi = (0, W) if b < W else (b - W, b)
        assert lo >= p_first and hi - p_first <= len(P), "a block that the level of block %d sums over is not present" % b
        S.append(cum[hi - p_first] - cum[lo - p_first])
    assert all(s <= 1 << 53 for s in S)
    return np.array(S, dtype=np.uint64)


def gain_indices(T, S):
    """k(b) = the number of i with S(b) > T[i]"""
    T = np.asarray(T, dtype=np.uint64)
    S = np.asarray(S, dtype=np.uint64)
    k = np.searchsorted(T, S, side="left").astype(np.int64)                   # T ascending: the entries below S come first
    for b in range(0, len(S), max(1, len(S) // 64)):                          # ... and the definition itself, in Python integers
        assert int(k[b]) == sum(1 for t in T.tolist() if int(S[b]) > t)
    return k


def out_count(c, n_samples):
    """output samples of a recording of n_samples: all of them once W whole blocks are there, in whole bytes"""
    if n_samples // c["block"] < c["window"]:
        return 0
    return n_samples // unit(c) * unit(c)


def needed(c, out_first, n_out):
    """(first, end) of the input samples that outputs out_first .. out_first + n_out - 1 need: output j of block b needs j itself and
    blocks max(b - W, 0) .. max(b, W) - 1 whole"""
    Lb, W = c["block"], c["window"]
    return max(out_first // Lb - W, 0) * Lb, max(out_first + n_out, W * Lb)


def supported(c, in_first, in_count):
    """the end of the outputs that input samples in_first .. in_first + in_count - 1 support"""
    return out_count(c, in_first + in_count)


def evaluate(c, G, T, x, out_first=0, n_out=None, in_first=0):
    """What gacq_requant_run_dev writes for outputs out_first .. out_first + n_out - 1 of the recording whose samples in_first ..
    are x (interleaved integers; in_first, the absolute index of x[0], is a multiple of the block): (bytes as uint8, clipped
    components, owned blocks, k(b) of the owned blocks as uint8).  Blocks are j div Lb of the absolute index j, and the warm-up applies
    to the blocks below W only."""
    v = np.asarray(x).reshape(-1)
    Lb, W = c["block"], c["window"]
    assert in_first >= 0 and in_first % Lb == 0
    total = out_count(c, in_first + len(v) // 2)
    n_out = total - out_first if n_out is None else n_out
    assert out_first >= in_first and n_out >= 0 and out_first + n_out <= total and out_first % unit(c) == 0 and n_out % unit(c) == 0
    G = np.asarray(G, dtype=np.float32)
    assert len(G) >= 1 and len(T) == len(G) - 1 and all(int(T[i]) <= int(T[i + 1]) for i in range(len(T) - 1))
    if n_out == 0:
        return np.zeros(0, dtype=np.uint8), 0, 0, np.zeros(0, dtype=np.uint8)
    P = block_powers(c, v)
    b_lo, nblocks = out_first // Lb, (out_first + n_out - 1) // Lb + 1
    k = gain_indices(T, levels(c, P, nblocks, b_lo, in_first // Lb))          # k[i] is that of block b_lo + i
    j = np.arange(out_first, out_first + n_out, dtype=np.int64)
    g = np.repeat(G[k[j // Lb - b_lo]], 2)                                    # per component
    comp = v[2 * (out_first - in_first):2 * (out_first - in_first + n_out)].astype(np.float32)        # exact: |component| <= 32768
    val = comp * g                                                            # one float32 multiply
    assert val.dtype == np.float32
    kind = c["container"]
    if kind == "f32":
        out, clipped = val.astype("<f4").view(np.uint8), 0
    elif kind in ("s8", "u8", "s16"):
        lim = 32767 if kind == "s16" else 127
        r = np.rint(val)                                                      # ties to even
        q = np.clip(r, -lim, lim)
        clipped = int(np.count_nonzero(q != r))
        if kind == "s16":
            out = q.astype("<i2").view(np.uint8)
        else:
            out = (q.astype(np.int64) + (128 if kind == "u8" else 0)).astype(np.uint8 if kind == "u8" else np.int8).view(np.uint8)
    else:
        bits = c["bits"]
        nlev = 1 << bits
        f = np.floor(val * np.float32(0.5)) + np.float32(nlev // 2)
        q = np.clip(f, 0, nlev - 1)
        clipped = int(np.count_nonzero(q != f))
        codes = np.asarray(c["enc"], dtype=np.int64)[q.astype(np.int64)]
        per = 8 // bits
        i = np.arange(per)
        shift = (8 - bits * (i + 1)) if c["msb_first"] else bits * i
        out = (codes.reshape(-1, per) << shift[None, :]).sum(axis=1).astype(np.uint8)
    first_owned = -(-out_first // Lb)
    owned = k[first_owned - b_lo:]
    return np.ascontiguousarray(out), clipped, len(owned), owned.astype(np.uint8)


def levels_of_codes(c, values):
    """2q - (n - 1) per component of an output of evaluate() with a packed container, read back the way ingest reads it: int64"""
    bits = c["bits"]
    per = 8 // bits
    i = np.arange(per)
    shift = (8 - bits * (i + 1)) if c["msb_first"] else bits * i
    codes = (np.asarray(values, dtype=np.uint8)[:, None].astype(np.int64) >> shift[None, :]) & ((1 << bits) - 1)
    inv = np.zeros(1 << bits, dtype=np.int64)
    for q, code in enumerate(c["enc"]):
        inv[code] = 2 * q - ((1 << bits) - 1)
    return inv[codes.reshape(-1)]
