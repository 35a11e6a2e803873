"""Steering vectors of tracked satellites across an antenna array (csrc/gacq_aprompt.hip, gacq_aprompt_dev): the replica of a tracked
satellite, one segment per tracking record as cancel builds it, is projected on all M antenna recordings at once.  The M complex prompts
of a segment are the satellite's steering vector times one common factor (amplitude, data bit, residual phase); a few hundred segments
give the vector to a fraction of a degree -- for a signal 20 dB under the noise, because the projection despreads it.  The vector is
what nulling and stap take as ``--constraint``; its direction on a grid is the satellite's bearing; tracked satellites that all share
one vector come from one emitter: a spoofer.

    python -m gnss_dsp_tools_amd.arrayprompt <signal> [handoff's search options] [--skip RECORDS] [--dwell RECORDS] [--ref P]
           --antenna IN0 --antenna IN1 [...] [--element E,N,U ... [--step DEG] [--el-min DEG]] [--alike X] [--trace FILE]
           TRACKFILE FS COFFSET

acquires and tracks <signal> on TRACKFILE as ``python -m gnss_dsp_tools_amd.handoff`` does (one of the antenna files, or the output of
nulling or stap on them), projects every channel's segments (leaving out the first RECORDS records: the pull-in) on the antenna files,
which are read whole, and prints one line per tracked item:

    <item> records <D> quality <q> steering RE,IM RE,IM ...

the entries repr-exact as ``--constraint`` parses them, scaled so that antenna P (--ref, default 0) is 1; with one --element per antenna
(as in bearing) the line goes on `` az <deg> el <deg> beam <value>``, the Bartlett maximum over the grid.  The last line is

    coherence min <x> max <y> pairs <n> directions alike|distinct

over all pairs of items (alike: every pair at or above --alike), or ``coherence none`` with fewer than two items.  --trace FILE gets one
line per (item, dwell of --dwell records).  Only the template trackers are covered.  The definition is in include/gacq.h."""
import ctypes
import sys
from typing import NamedTuple

import numpy as np

from . import _native as nat
from . import acquire, bearing, cancel, codes, handoff as _handoff, signals, streaming
from .mitigate import _count, _device_input

MAX_ANTENNAS = 8
ALIKE = 0.9


def _row_list(rows):
    torch = nat.require_torch()
    if torch.is_tensor(rows) or isinstance(rows, np.ndarray):
        if rows.ndim != 2:
            raise ValueError("rows must be a list of flat recordings or a 2-D array [antenna][samples]")
        rows = [rows[p] for p in range(rows.shape[0])]
    rows = list(rows)
    if not 1 <= len(rows) <= MAX_ANTENNAS:
        raise ValueError("need 1..%d antennas, got %d" % (MAX_ANTENNAS, len(rows)))
    return rows


def project(engine, sats, segs, fs, rows, in_first=0, in_complex64=False):
    """One call of gacq_aprompt_dev.  ``sats`` and ``segs`` as cancel.apply takes them (segments from cancel.segments_from_track; the
    amplitudes are not looked at); ``rows``: M flat int8 or complex64 CUDA tensors of equal length (or bytes, as cancel.apply takes
    them), or the 2-D tensor scene.recording returns: input samples in_first .. of every antenna.
    Returns ([complex128 [nseg_k, M] per satellite], [float64 [nseg_k] per satellite]): the prompts A_p and the energies sum w^2, NaN
    where a segment does not lie wholly inside the input.  Column p holds the bits cancel.apply(estimate=True) returns on row p alone."""
    arr, flat, segs = cancel._sat_structs(sats, segs)
    ds, flags = zip(*[_device_input(engine, r, in_complex64) for r in _row_list(rows)])
    M = len(ds)
    if len(set(flags)) != 1 or len({_count(d, c) for d, c in zip(ds, flags)}) != 1 or len({d.device for d in ds}) != 1:
        raise ValueError("the antennas' recordings must be of one kind, of equal length and on one device")
    in_c, in_count = flags[0], _count(ds[0], flags[0])
    prompts = np.full((len(flat), M), np.nan + 1j * np.nan, dtype=np.complex128)
    energy = np.full(len(flat), np.nan, dtype=np.float64)
    ptrs = (ctypes.c_void_p * M)(*[d.data_ptr() for d in ds])
    engine.use_torch_stream(ds[0].device)
    nat.check(nat.lib.gacq_aprompt_dev(engine._ctx, ctypes.addressof(arr), len(arr), ctypes.c_void_p(flat.ctypes.data), float(fs),
                                       ctypes.cast(ptrs, ctypes.c_void_p), M, int(in_c), int(in_first), in_count, ctypes.c_void_p(prompts.ctypes.data),
                                       ctypes.c_void_p(energy.ctypes.data)), engine._ctx)
    cuts = np.cumsum([0] + [len(g) for g in segs])
    return [prompts[cuts[k]:cuts[k + 1]] for k in range(len(segs))], [energy[cuts[k]:cuts[k + 1]] for k in range(len(segs))]


def steering_estimate(prompts, ref=0, noise_cov=None):
    """(a_hat, quality, segments used) of one satellite's prompts [segments, M], in numpy fp64.  Rows with a NaN are dropped;
    Rs = sum_g P[g] P[g]^H, which neither a data bit nor a segment's common phase changes; a_hat is the eigenvector of Rs's largest
    eigenvalue scaled to a_hat[ref] = 1, and quality = lambda_max / trace(Rs), the share of the prompts' power in that direction.
    With ``noise_cov`` (Hermitian positive definite [M, M], e.g. a window covariance of nulling) the estimate is whitened: with
    noise_cov = L L^H, u the principal eigenvector of L^-1 Rs L^-H, a_hat = L u scaled likewise, and quality is that matrix's; this is
    what keeps the estimate off a jammer, whose rank-one part survives despreading.
    The convention is that of nulling's constraint: for x_p = g_p s, a_hat[p] = g_p / g_ref.  No segment left: NaN, NaN, 0."""
    P = np.asarray(prompts, dtype=np.complex128)
    if P.ndim != 2 or P.shape[1] < 1:
        raise ValueError("prompts must be [segments, M]")
    M = P.shape[1]
    ref = int(ref)
    if not 0 <= ref < M:
        raise ValueError("ref must lie in 0..%d" % (M - 1))
    P = P[~np.isnan(P).any(axis=1)]
    if len(P) == 0:
        return np.full(M, np.nan + 1j * np.nan), float("nan"), 0
    Rs = P.T @ P.conj()
    L = None
    if noise_cov is not None:
        N = np.asarray(noise_cov, dtype=np.complex128)
        if N.shape != (M, M):
            raise ValueError("noise_cov must be [%d, %d]" % (M, M))
        L = np.linalg.cholesky(0.5 * (N + N.conj().T))
        Y = np.linalg.solve(L, Rs)                                  # L^-1 Rs
        Rs = np.linalg.solve(L, Y.conj().T).conj().T                # (L^-1 (L^-1 Rs)^H)^H = L^-1 Rs L^-H
    Rs = 0.5 * (Rs + Rs.conj().T)
    lam, V = np.linalg.eigh(Rs)
    u = V[:, -1]
    a = u if L is None else L @ u
    tr = float(np.real(np.trace(Rs)))
    quality = float(lam[-1]) / tr if tr > 0.0 else float("nan")
    a = a / a[ref]
    a[ref] = 1.0                                                    # exactly, whatever the complex division left
    return a, quality, len(P)


def direction(a_hat, elements, cells):
    """The Bartlett scan |a_g^H a_hat|^2 / (M |a_hat|^2) over bearing.tables(elements, cells): (cell index, az, el, value in 0..1) of
    the largest value, ties to the lowest index"""
    cells = np.asarray(cells, dtype=np.float64).reshape(-1, 2)
    a_hat = np.asarray(a_hat, dtype=np.complex128).reshape(-1)
    table, _ = bearing.tables(elements, cells)
    if table.shape[1] != len(a_hat):
        raise ValueError("%d elements for a vector of %d antennas" % (table.shape[1], len(a_hat)))
    v = np.abs(table.conj() @ a_hat) ** 2 / (len(a_hat) * float(np.sum(np.abs(a_hat) ** 2)))
    g = int(np.argmax(v))
    return g, float(cells[g, 0]), float(cells[g, 1]), float(v[g])


def coherence(vectors):
    """[K, K]: |a_k^H a_l| / (|a_k| |a_l|) of the K vectors"""
    V = np.asarray(vectors, dtype=np.complex128)
    V = V.reshape(len(V), -1)
    n = np.sqrt(np.sum(np.abs(V) ** 2, axis=1))
    return np.abs(V.conj() @ V.T) / np.outer(n, n)


class Estimate(NamedTuple):
    """records first .. first + count - 1 of a channel's segments: steering_estimate's three results on them"""
    first: int
    count: int
    a_hat: np.ndarray
    quality: float
    used: int


def dwell_estimates(prompts, dwell=None, ref=0, noise_cov=None):
    """[Estimate]: one over all of a channel's prompts, or one per ``dwell`` consecutive records (the last one may be shorter)"""
    n = len(prompts)
    if dwell is None:
        return [Estimate(0, n, *steering_estimate(prompts, ref, noise_cov))]
    step = int(dwell)
    if step < 1:
        raise ValueError("dwell must be at least 1")
    return [Estimate(i, min(step, n - i), *steering_estimate(prompts[i:i + step], ref, noise_cov)) for i in range(0, n, step)]


def _host_int8(x):
    torch = nat.require_torch()
    if torch.is_tensor(x):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(x).reshape(-1).view(np.int8)


def measure_tracked(name, rows_int8, fs, coffset, track=0, items=None, min_metric=None, skip=0, dwell=None, ref=0, **handoff_kw):
    """Acquire ``name`` and hand off as handoff.handoff does (its keywords pass through) on row ``track`` of the int8 antenna
    recordings -- or on the separate int8 recording given as ``track``, e.g. a nulled output --, track every channel over that
    recording, build each channel's segments from its records after the first ``skip``, project all channels on all rows in one call
    and estimate one steering vector per channel, or one per ``dwell`` consecutive records.
    Returns (channels, [prompts [nseg_k, M] per channel], [[Estimate] per channel])."""
    rows = _row_list(rows_int8)
    if not 0 <= int(ref) < len(rows):
        raise ValueError("ref must lie in 0..%d" % (len(rows) - 1))
    if dwell is not None and int(dwell) < 1:
        raise ValueError("dwell must be at least 1")
    tracked = _host_int8(rows[int(track)] if isinstance(track, (int, np.integer)) else track)
    _, _, loop, x_dev = _handoff.handoff(name, tracked, fs, coffset, items=items, min_metric=min_metric, **handoff_kw)
    if loop is None:
        return [], [], []
    try:
        state0 = [loop.state(k) for k in range(loop.K)]          # the loop has not run yet: what the first block runs with
        recs = loop.run([x_dev] * loop.K)
        chans = loop.channels
        eng = loop.eng
    finally:
        loop.close()
    sats = [cancel.sat_of(c) for c in chans]
    segs = [cancel.segments_from_track(c, s, r, skip) for c, s, r in zip(chans, state0, recs)]
    prompts, _ = project(eng, sats, segs, fs, rows)
    return chans, prompts, [dwell_estimates(p, dwell, ref) for p in prompts]


# ---- command line

def build_parser(sig):
    ap = _handoff.build_parser(sig)
    ap.prog = "arrayprompt %s" % sig.name
    ap.description = "Acquire and track %s and measure every tracked item's steering vector across the antenna recordings" % sig.name
    ap.add_argument("--skip", type=int, default=0, help="records of every channel left out: the pull-in (default %(default)s)")
    ap.add_argument("--dwell", type=int, default=None, help="records per line of --trace (default: all of a channel's)")
    ap.add_argument("--ref", type=int, default=0, help="the antenna whose entry is 1 (default %(default)s)")
    ap.add_argument("--antenna", action="append", default=[], metavar="IN", help="one int8 I/Q recording per antenna, 1..%d of them" % MAX_ANTENNAS)
    ap.add_argument("--element", type=bearing._element, action="append", default=[], metavar="E,N,U",
                    help="one per antenna: east,north,up in wavelengths; the lines then carry the bearing")
    ap.add_argument("--step", type=float, default=bearing.STEP, help="grid step in degrees (default %(default)s)")
    ap.add_argument("--el-min", type=float, default=0.0, help="lowest elevation of the grid in degrees (default %(default)s)")
    ap.add_argument("--alike", type=float, default=ALIKE, help="coherence at or above which two items share a direction (default %(default)s)")
    ap.add_argument("--trace", default=None, metavar="FILE", help="file for one line per (item, dwell)")
    return ap


def parse(name, argv):
    """(signal, argparse namespace with .items as a list, .doppler_search and .loop_dwells as floats, .cells the grid or None)"""
    _handoff.tracker_name(name)
    sig = signals.get(name)
    argv = list(argv)
    # --element values may begin with '-': hand them over in the form argparse never takes for an option
    for i in range(len(argv) - 1):
        if argv[i] == "--element":
            argv[i:i + 2] = ["--element=" + argv[i + 1], None]
    a = build_parser(sig).parse_args(_handoff._join_option_values([v for v in argv if v is not None]))
    if a.out_dir is not None or a.nav:
        raise SystemExit("arrayprompt: --out-dir and --nav belong to the handoff command")
    M = len(a.antenna)
    if not 1 <= M <= MAX_ANTENNAS:
        raise SystemExit("arrayprompt: need 1..%d --antenna files (%d given)" % (MAX_ANTENNAS, M))
    if a.element and len(a.element) != M:
        raise SystemExit("arrayprompt: need one --element per --antenna (%d files, %d elements)" % (M, len(a.element)))
    if a.skip < 0 or (a.dwell is not None and a.dwell < 1) or not 0 <= a.ref < M or not 0.0 <= a.alike <= 1.0:
        raise SystemExit("arrayprompt: --skip is not negative, --dwell is at least 1, --ref lies in 0..%d and --alike in 0..1" % (M - 1))
    a.cells = None
    if a.element:
        try:
            a.cells = bearing.grid(a.step, a.el_min)
        except ValueError as e:
            raise SystemExit("arrayprompt: %s" % e)
    a.items = acquire.parse_list_ranges(a.items, sep=sig.item_sep) if a.items else codes.prns(sig.code)
    a.doppler_search = acquire.parse_list_floats(a.doppler_search)
    a.loop_dwells = tuple(acquire.parse_list_floats(a.loop_dwells))
    return sig, a


def steering_text(a_hat):
    """the entries as --constraint parses them back to the same doubles"""
    return " ".join("%r,%r" % (float(v.real), float(v.imag)) for v in np.asarray(a_hat, dtype=np.complex128))


def item_line(item, est, elements=None, cells=None):
    text = "%d records %d quality %.4f steering %s" % (int(item), est.used, est.quality, steering_text(est.a_hat))
    if elements is not None and est.used:
        _, az, el, beam = direction(est.a_hat, elements, cells)
        text += " az %g el %g beam %.4f" % (az, el, beam)
    return text


def trace_line(item, est):
    return "%d record %d records %d quality %.4f steering %s" % (int(item), est.first, est.used, est.quality, steering_text(est.a_hat))


def coherence_line(vectors, alike=ALIKE):
    vectors = [v for v in vectors if not np.isnan(v).any()]
    if len(vectors) < 2:
        return "coherence none"
    c = coherence(vectors)[np.triu_indices(len(vectors), 1)]
    return "coherence min %.4f max %.4f pairs %d directions %s" % (c.min(), c.max(), len(c), "alike" if bool(np.all(c >= alike)) else "distinct")


def run(name, argv, out=None):
    sig, a = parse(name, argv)
    out = sys.stdout if out is None else out
    rows = [np.fromfile(f, dtype=np.int8) for f in a.antenna]
    if len({len(r) for r in rows}) != 1:
        raise SystemExit("arrayprompt: the --antenna files differ in length (%s bytes)" % ", ".join(str(len(r)) for r in rows))
    rows = [r[:len(r) // 2 * 2] for r in rows]
    tracked = np.fromfile(a.input_filename, dtype=np.int8)
    eng = acquire.Engine(a.device)
    try:
        chans, prompts, ests = measure_tracked(name, rows, a.sample_rate, a.carrier_offset, track=tracked, items=a.items, min_metric=a.min_metric,
                                               skip=a.skip, ref=a.ref, doppler_search=a.doppler_search, ms=a.time, min_ratio=a.min_ratio, M=a.blocks,
                                               loop_dwells=a.loop_dwells, engine=eng)
    finally:
        eng.close()
    elements = np.array(a.element, dtype=np.float64) if a.element else None
    lines = [item_line(c.prn, e[0], elements, a.cells) for c, e in zip(chans, ests)]
    lines.append(coherence_line([e[0].a_hat for e in ests], a.alike))
    if a.trace:
        with open(a.trace, "w") as f:
            for c, p in zip(chans, prompts):
                for e in dwell_estimates(p, a.dwell, a.ref):
                    print(trace_line(c.prn, e), file=f)
    for line in lines:
        print(line, file=out)
    return lines


def main(argv=None):
    return streaming.main(argv, __doc__, lambda argv: run(argv[0], argv[1:]))


if __name__ == "__main__":
    sys.exit(main())
