"""Fine search on the raw recording around acquisition results: the step between acquire and track.

Acquisition reports Doppler on a 20-200 Hz grid and code phase at one sample of its resampled, filtered copy.  ``refine`` evaluates,
for every candidate, the prompt correlation on the int8 recording itself over M blocks of 1 ms, D Doppler hypotheses and P code
offsets around the coarse point (csrc/gacq_corrgrid.hip, one launch for all candidates), and reduces that grid on the host in fp64:

1. S[d,p] = sum_m |C[m,d,p]|; one extra code offset half a code away is the noise floor and is kept apart;
2. (d*, p*) = the first argmax in row-major order; ``edge`` when it lies on the border of either axis;
3. the code offset by the three-point parabola over p when p* is interior, else the grid value;
4. a second launch with D = P = 1 at (f_d*, c) gives the prompts P_m;
5. f = f_d* + angle(sum_m (P_{m+1} conj(P_m))^2) / (4 pi n / fs): squaring removes data-bit and secondary-code flips, which leaves the
   estimate unambiguous within +-fs/(4n) ~ 250 Hz -- hence df <= 250 and M >= 2;
6. ratio = S[d*,p*] / S_floor[d*].

``estimate`` is that reduction over any grid function; ``refine`` runs it on the device grid.
"""
import ctypes
from dataclasses import dataclass

import numpy as np

from . import _native as nat
from . import acquire, codes, trackloop

MAX_HYP = 33             # D, P <= 33 (gacq_corr_grid_dev)
D_DEFAULT = 5
P_DEFAULT = 9


@dataclass
class Candidate:
    """One acquisition result to refine: the tracker's name and item (PRN, or the RF channel for GLONASS L1/L2), the recording's sample
    rate and carrier offset, the coarse Doppler and code offset, and the acquisition grid's Doppler increment (Hz) and code resolution
    (chips per sample of the acquisition's rate: chip_rate / signal.fs)."""
    name: str
    item: int
    fs: float
    coffset: float
    doppler: float
    code_offset: float
    doppler_incr: float
    code_res: float

    def __str__(self):
        return "%s %d" % (self.name, self.item)


@dataclass
class Grid:
    """The arguments of one gacq_grid_spec.  offsets: P code offsets in chips relative to code0."""
    code: str
    prn: int
    kind: int
    n: int
    M: int
    D: int
    fs: float
    carrier_hz: float
    chip_rate: float
    ratio: float
    doppler0: float
    code0: float
    df: float
    s0: int
    offsets: np.ndarray

    @property
    def P(self):
        return len(self.offsets)

    def dopplers(self):
        """f_d = doppler0 + (d - (D-1)/2) df"""
        return self.doppler0 + (np.arange(self.D, dtype=np.float64) - (self.D - 1) / 2.0) * self.df


@dataclass
class Refined:
    doppler: float
    code_offset: float       # chips, modulo the code length
    peak: float              # S[d*, p*]
    ratio: float             # peak over the noise-floor entry of the same Doppler row
    d_index: int
    p_index: int
    edge: bool


GridSpec = nat.struct("gacq_grid_spec")


def default_grid(c, M=16, D=D_DEFAULT, P=P_DEFAULT, df=None):
    """The grid refine() evaluates for candidate c: n = int(fs 0.001), blocks from the first code boundary, D Doppler hypotheses
    min(doppler_incr/2, 200 Hz) apart (or df), P code offsets a quarter of the acquisition's code resolution apart, and one more offset
    half a code away (the noise floor, last)."""
    if c.name not in trackloop.TRACKERS:
        raise KeyError("unknown tracker %r (the template family: %s)" % (c.name, ", ".join(sorted(trackloop.TRACKERS))))
    t = trackloop.TRACKERS[c.name]
    L = codes.code_length(t.code)
    chip_rate = float(codes.chip_rate(t.code))
    fs = float(c.fs)
    df = min(float(c.doppler_incr) / 2.0, 200.0) if df is None else float(df)
    if not (0.0 <= df <= 250.0):
        raise ValueError("%s: Doppler step %g Hz: the differential estimator is unambiguous only within +-250 Hz" % (c, df))
    if int(M) < 2:
        raise ValueError("%s: M = %d: the differential Doppler estimator needs at least two blocks" % (c, M))
    chan = int(c.item)
    carrier_hz = float(c.coffset) + (t.glonass[3] * chan if t.glonass else 0.0)
    code0 = float(np.mod(float(c.code_offset), L))
    dc = float(c.code_res) / 4.0
    offsets = np.concatenate([(np.arange(P, dtype=np.float64) - (P - 1) / 2.0) * dc, [L / 2.0]])
    return Grid(code=t.code, prn=0 if t.glonass else chan, kind=t.kind, n=int(fs * 0.001), M=int(M), D=int(D), fs=fs,
                carrier_hz=carrier_hz, chip_rate=chip_rate, ratio=t.scale(chan), doppler0=float(c.doppler), code0=code0, df=df,
                s0=int(fs * (L - code0) / chip_rate), offsets=offsets)


def corr_grid(grids, recordings, engine=None):
    """gacq_corr_grid_dev: one launch for all grids.  recordings: one interleaved int8 I/Q CUDA tensor per grid (grids may share one),
    or a single tensor for all.  Returns one complex128 array [M, D, P] per grid."""
    torch = nat.require_torch()
    eng = engine or acquire.default_engine()
    grids = list(grids)
    K = len(grids)
    if torch.is_tensor(recordings):
        recordings = [recordings] * K
    if len(recordings) != K:
        raise ValueError("need one recording per candidate (%d), got %d" % (K, len(recordings)))
    if K == 0:
        return []
    eng.use_torch_stream(torch.device("cuda", eng.device))
    specs = (GridSpec * K)()
    ptrs = (ctypes.c_void_p * K)()
    avail = np.zeros(K, dtype=np.int64)
    keep = []
    for k, (g, x) in enumerate(zip(grids, recordings)):
        if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.int8 and x.dim() == 1 and x.is_contiguous()):
            raise ValueError("candidate %d: samples must be a contiguous 1-D int8 CUDA tensor (interleaved I/Q)" % k)
        off = np.ascontiguousarray(g.offsets, dtype=np.float64)
        keep.append(off)
        specs[k] = GridSpec(code=g.code.encode(), prn=int(g.prn), kind=int(g.kind), n=int(g.n), M=int(g.M), D=int(g.D), P=len(off),
                            fs=float(g.fs), carrier_hz=float(g.carrier_hz), chip_rate=float(g.chip_rate), ratio=float(g.ratio),
                            doppler0=float(g.doppler0), code0=float(g.code0), df=float(g.df), s0=int(g.s0), offsets=off.ctypes.data)
        ptrs[k] = x.data_ptr()
        avail[k] = x.numel() // 2
    sizes = [max(int(g.M), 0) * max(int(g.D), 0) * len(g.offsets) for g in grids]
    out = np.zeros(max(sum(sizes), 1), dtype=np.complex128)
    nat.check(nat.lib.gacq_corr_grid_dev(eng._ctx, specs, K, ptrs, avail.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p)),
              eng._ctx)
    res, at = [], 0
    for g, sz in zip(grids, sizes):
        res.append(out[at:at + sz].reshape(g.M, g.D, len(g.offsets)).copy())
        at += sz
    return res


def pick(C):
    """Steps 1-3 and 6 on one grid C [M, D, P+1] (the last code offset is the noise floor): (d*, p*, edge, delta, peak, ratio) with delta
    the parabola's offset from p* in grid steps (0 on the border)."""
    S = np.abs(np.asarray(C, dtype=np.complex128)).sum(axis=0)
    floor, S = S[:, -1], S[:, :-1]
    D, P = S.shape
    d, p = np.unravel_index(int(np.argmax(S)), S.shape)            # first maximum in row-major order
    edge = bool((D > 1 and d in (0, D - 1)) or (P > 1 and p in (0, P - 1)))
    delta = 0.0
    if 0 < p < P - 1:
        a, b, c = S[d, p - 1], S[d, p], S[d, p + 1]
        den = a - 2.0 * b + c
        if den < 0.0:
            delta = float(0.5 * (a - c) / den)
    return int(d), int(p), edge, delta, float(S[d, p]), float(S[d, p] / floor[d]) if floor[d] > 0.0 else float("inf")


def fine_doppler(prompts, f, n, fs):
    """Step 5: f + angle(sum_m (P_{m+1} conj(P_m))^2) / (4 pi n / fs)"""
    prompts = np.asarray(prompts, dtype=np.complex128)
    z = np.sum((prompts[1:] * np.conj(prompts[:-1])) ** 2)
    return float(f + np.angle(z) / (4.0 * np.pi * n / fs))


def estimate(candidates, grid_fn, avail, M=16, df=None):
    """The estimator over any grid function: grid_fn(list of Grid) -> list of complex128 [M, D, P] arrays.  avail: samples in each
    candidate's recording.  A candidate whose recording is shorter than s0 + M n raises ValueError."""
    candidates = list(candidates)
    grids = [default_grid(c, M, df=df) for c in candidates]
    for c, g, a in zip(candidates, grids, avail):
        if g.s0 + g.M * g.n > int(a):
            raise ValueError("candidate %s: the recording has %d samples, the refinement needs %d (first code boundary at %d, %d blocks of %d)"
                             % (c, int(a), g.s0 + g.M * g.n, g.s0, g.M, g.n))
    if not candidates:
        return []
    picks = [pick(C) for C in grid_fn(grids)]
    second = []
    for g, (d, p, edge, delta, peak, ratio) in zip(grids, picks):
        dc = g.offsets[1] - g.offsets[0]
        # the prompts at (f_d*, c): a grid of one point centred there (its code rate follows f_d*: at most 2 df / ratio chips/s away)
        second.append(Grid(**{**g.__dict__, "D": 1, "df": 0.0, "doppler0": float(g.dopplers()[d]),
                              "offsets": np.array([g.offsets[p] + delta * dc])}))
    out = []
    for c, g, g2, (d, p, edge, delta, peak, ratio), C2 in zip(candidates, grids, second, picks, grid_fn(second)):
        L = codes.code_length(g.code)
        f = fine_doppler(C2[:, 0, 0], g2.doppler0, g.n, g.fs)
        out.append(Refined(doppler=f, code_offset=float(np.mod(g.code0 + g2.offsets[0], L)), peak=peak, ratio=ratio, d_index=d, p_index=p,
                           edge=edge))
    return out


def refine(candidates, recordings, M=16, engine=None, df=None):
    """Refine acquisition results on the device: candidates (Candidate) and their recordings (one int8 CUDA tensor each, or one shared
    tensor) -> list of Refined.  df: Doppler step in Hz instead of min(doppler_incr/2, 200); at most 250."""
    torch = nat.require_torch()
    candidates = list(candidates)
    if torch.is_tensor(recordings):
        recordings = [recordings] * len(candidates)
    if len(recordings) != len(candidates):
        raise ValueError("need one recording per candidate (%d), got %d" % (len(candidates), len(recordings)))
    return estimate(candidates, lambda grids: corr_grid(grids, recordings, engine), [x.numel() // 2 for x in recordings], M, df)
