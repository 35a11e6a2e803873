"""GPU: the bearing kernels (csrc/gacq_bearing.hip) against the definition of tests/bearing_oracle.py, bit for bit: q and the floor as
uint64, the records as bytes, every output with sentinels past its end.  Shapes at every edge of the launch geometry, strides, exact
ties in every reduction stage, the exclusion rule at its ends, ineligible cells, calls of several chunks, the refusals of
gacq_bearing_run_dev, cut recordings, the command line, and a scene of two interferers whose directions come out."""
import ctypes
import io

import numpy as np
import pytest

import bearing_cases as C
import bearing_oracle as B
import nulling_cases as NC
from gnss_dsp_tools_amd import _native as nat
from gnss_dsp_tools_amd import bearing, nulling, scene

BAD_ARG = -1
FILL = 0x77


def _finder(engine, a, u, K=C.K, cos_sep=C.COS_SEP, shift=C.SHIFT):
    return bearing.Finder.from_tables(engine, a, u, shift, K, cos_sep)


def _run(engine, fd, cov, n, stride=1, spectrum=True):
    """gacq_bearing_run_dev through the raw ABI on outputs that end in sentinels: (records [n][K], floor [n], q [n][G] or None)"""
    torch = nat.require_torch()
    dev = "cuda:%d" % engine.device
    d_cov = torch.from_numpy(np.ascontiguousarray(cov, dtype=np.int64)).to(dev)
    sizes = (16 * n * fd.K, 8 * n, 8 * n * fd.G if spectrum else 0)
    pk, fl, sp = (torch.full((s + 64,), FILL, dtype=torch.uint8, device=dev) for s in sizes)
    engine.use_torch_stream(d_cov.device)
    rc = nat.lib.gacq_bearing_run_dev(fd._h, ctypes.c_void_p(d_cov.data_ptr()), n, stride, ctypes.c_void_p(pk.data_ptr()), ctypes.c_void_p(fl.data_ptr()),
                                      ctypes.c_void_p(sp.data_ptr()) if spectrum else None)
    assert rc == 0, nat.lib.gacq_last_error(engine._ctx)
    torch.cuda.synchronize()
    got = []
    for t, s in zip((pk, fl, sp), sizes):
        h = t.cpu().numpy()
        assert np.all(h[s:] == FILL)
        got.append(h[:s])
    return got[0].view(bearing.PEAK).reshape(n, fd.K), got[1].view(np.float64), got[2].view(np.float64).reshape(n, fd.G) if spectrum else None


def _same(got, want, what=None):
    rec, fl, q = got
    assert fl.tobytes() == want[1].tobytes(), (what, fl, want[1])
    if q is not None:
        bad = np.argwhere(q.view(np.uint64) != want[2].view(np.uint64))
        assert len(bad) == 0, (what, bad[:4])
    assert rec.tobytes() == want[0].tobytes(), (what, rec[:2], want[0][:2])


@pytest.mark.gpu
@pytest.mark.parametrize("M,G", C.SHAPES)
def test_spectrum_floor_and_peaks_equal_the_oracle(engine, M, G):
    """K = 4, n = 5, the whole spectrum: one cell, a wave edge, a workgroup edge, one cell past what LDS holds in doubles, the cap"""
    a, u = C.table(M, G)
    want = C.reference(M, G)
    with _finder(engine, a, u) as fd:
        _same(_run(engine, fd, C.stacked(*C.covariances(M)), C.N_BLOCKS), want, (M, G))
    assert np.all(want[0]["cell"][:, 0] >= 0) and not np.array_equal(want[2][0], want[2][1])                 # the blocks differ


@pytest.mark.gpu
@pytest.mark.parametrize("M", [3, 8])
def test_stride_and_a_single_block(engine, M):
    a, u = C.table(M, 257)
    R = C.stacked(*C.covariances(M))
    want = C.reference(M, 257)
    spread = np.full((3 * (C.N_BLOCKS - 1) + 1,) + R.shape[1:], -(1 << 40), dtype=np.int64)     # the rows between: nothing like a covariance
    spread[::3] = R
    with _finder(engine, a, u) as fd:
        _same(_run(engine, fd, spread, C.N_BLOCKS, 3), want, "stride 3")
        _same(_run(engine, fd, R, C.N_BLOCKS, 1), want, "stride 1")
        _same(_run(engine, fd, R[2:], 1, 1), tuple(w[2:3] for w in want), "one block")
        _same(_run(engine, fd, spread, 2, 6, spectrum=False), tuple(w[0:3:2] for w in want), "stride 6, no spectrum")


def _tie_table(order):
    cells = bearing.grid(5.0)
    a, u = bearing.tables(C.TIE_ELEMENTS, cells)
    return a[order], u[order]


@pytest.mark.gpu
def test_exact_ties_go_to_the_lowest_cell_in_every_reduction_stage(engine):
    """the two-element array: several cells share the smallest q of a block bit for bit.  The table as it is, reversed, shuffled, and with
    the tied cells of block 0 moved into one lane's own cells, neighbouring lanes, two waves, and the two ends of the grid"""
    R = C.tie_covariances()
    Rs = C.stacked(*R)
    G = 1368
    base = B.run(*R, C.SHIFT, *_tie_table(np.arange(G)), C.K, C.COS_SEP)
    tied = [int(g) for g in np.flatnonzero(base[2][0] == base[0]["q"][0, 0])]
    assert len(tied) >= 2
    orders = [np.arange(G), np.arange(G)[::-1].copy(), np.random.default_rng(3).permutation(G)]
    for spots in ((5, 5 + 256), (5 + 512, 5), (10, 11), (63, 64), (255, 256), (0, G - 1), (G - 1, 0), (700, 100)):
        order = np.arange(G)
        for g, spot in zip(tied[:2], spots):                      # cell g goes to position spot, what was there to g's place
            i, j = int(np.flatnonzero(order == g)[0]), spot
            order[i], order[j] = order[j], order[i]
        orders.append(order)
    for n, order in enumerate(orders):
        a, u = _tie_table(order)
        want = B.run(*R, C.SHIFT, a, u, C.K, C.COS_SEP)
        for i in range(Rs.shape[0]):
            same = np.flatnonzero(want[2][i] == want[0]["q"][i, 0])
            assert len(same) >= 2 and want[0]["cell"][i, 0] == same[0]
        with _finder(engine, a, u) as fd:
            _same(_run(engine, fd, Rs, Rs.shape[0]), want, n)


AXES = np.array([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0], [-1.0, 0, 0], [0, -1.0, 0], [0, 0, -1.0]])


@pytest.mark.gpu
def test_the_exclusion_rule_at_its_ends(engine):
    M = 5
    Rs = C.stacked(*C.covariances(M))
    a, u = C.table(M, 257)
    # cos_sep = -1: every cell lies within reach of rank 0
    want = B.run(*C.covariances(M), C.SHIFT, a, u, C.K, -1.0)
    assert np.all(want[0]["cell"][:, 1:] == -1) and np.all(np.isposinf(want[0]["q"][:, 1:])) and np.all(want[0]["cell"][:, 0] >= 0)
    with _finder(engine, a, u, cos_sep=-1.0) as fd:
        _same(_run(engine, fd, Rs, C.N_BLOCKS), want, "cos_sep -1")
    # cos_sep = 1 over a table whose rows come twice, the directions on the axes: only the cells with the very direction of a peak leave
    a2, u2 = np.concatenate([a[:120], a[:120]]), np.concatenate([AXES[np.arange(120) % 6]] * 2)
    want = B.run(*C.covariances(M), C.SHIFT, a2, u2, C.K, 1.0)
    rec = want[0]
    assert np.all(rec["cell"] >= 0)
    for i in range(C.N_BLOCKS):
        assert len(set(tuple(u2[g]) for g in rec["cell"][i])) == C.K                  # four ranks, four axes
        assert want[2][i, rec["cell"][i, 0]] == want[2][i, rec["cell"][i, 0] + 120]  # the twin of rank 0 ties with it and is gone
    with _finder(engine, a2, u2, cos_sep=1.0) as fd:
        _same(_run(engine, fd, Rs, C.N_BLOCKS), want, "cos_sep 1")
    # the boundary: cos_sep = 0 on the axes.  A perpendicular cell has the product 0 = cos_sep exactly and leaves; only the opposite
    # axis is left for rank 1, and nothing after it
    want = B.run(*C.covariances(M), C.SHIFT, a2, u2, C.K, 0.0)
    rec = want[0]
    assert np.all(rec["cell"][:, :2] >= 0) and np.all(rec["cell"][:, 2:] == -1)
    assert all(np.array_equal(u2[rec["cell"][i, 1]], -u2[rec["cell"][i, 0]]) for i in range(C.N_BLOCKS))
    with _finder(engine, a2, u2, cos_sep=0.0) as fd:
        _same(_run(engine, fd, Rs, C.N_BLOCKS), want, "cos_sep 0")
    # ... and half-length directions: 0.5 * 1 = cos_sep = 0.5 exactly
    u3 = u2.copy()
    u3[1::2] *= 0.5
    want = B.run(*C.covariances(M), C.SHIFT, a2, u3, C.K, 0.5)
    with _finder(engine, a2, u3, cos_sep=0.5) as fd:
        _same(_run(engine, fd, Rs, C.N_BLOCKS), want, "cos_sep 0.5")


@pytest.mark.gpu
def test_ineligible_cells(engine):
    a, u = C.table(3, 257)
    for what, R, shift in (("negative pivot", C.negative_pivot(), C.SHIFT), ("all nan", C.all_nan(), 0), ("zero", np.zeros((1, 3, 3, 2), dtype=np.int64), C.SHIFT)):
        want = B.run(R[..., 0], R[..., 1], shift, a, u, C.K, C.COS_SEP)
        if what == "negative pivot":
            assert np.any(want[2] <= 0) and np.any(want[2] > 0) and np.all(want[0]["q"] > 0)
        if what == "all nan":
            assert np.all(np.isnan(want[2])) and np.isposinf(want[1][0]) and np.all(want[0]["cell"] == -1) and np.all(np.isposinf(want[0]["q"]))
        with _finder(engine, a, u, shift=shift) as fd:
            _same(_run(engine, fd, R, 1), want, what)
    # every component of every antenna at -128: the largest window sum there is
    R = NC.reference("min-m8-b32768-w1")["cov"][:1]
    assert R.shape == (1, 8, 8, 2) and np.all(R[..., 0] == 1 << 30) and np.all(R[..., 1] == 0)
    a, u = C.table(8, 257)
    want = B.run(R[..., 0], R[..., 1], C.SHIFT, a, u, C.K, C.COS_SEP)
    with _finder(engine, a, u) as fd:
        _same(_run(engine, fd, R, 1), want, "min")


@pytest.mark.gpu
def test_a_call_of_several_chunks(engine):
    """G = 32768 leaves 512 blocks to a pair of launches: 1030 blocks are three chunks, the last one short.  The covariances repeat with
    period 5, so the oracle's five rows say what every block gives"""
    M, G, n = 2, 32768, 1030
    a, u = C.table(M, G)
    want = C.reference(M, G)
    R = C.stacked(*C.covariances(M))
    with _finder(engine, a, u) as fd:
        rec, fl, _ = _run(engine, fd, R[np.arange(n) % C.N_BLOCKS], n, spectrum=False)
    idx = np.arange(n) % C.N_BLOCKS
    assert fl.tobytes() == want[1][idx].tobytes() and rec.tobytes() == want[0][idx].tobytes()


@pytest.mark.gpu
def test_refusals_of_run_dev_leave_the_outputs_untouched(engine):
    torch = nat.require_torch()
    M, G = 3, 65
    a, u = C.table(M, G)
    dev = "cuda:%d" % engine.device
    cov = torch.from_numpy(C.stacked(*C.covariances(M))).to(dev)
    pk = torch.full((16 * C.K * C.N_BLOCKS + 16,), FILL, dtype=torch.uint8, device=dev)
    fl = torch.full((8 * C.N_BLOCKS + 16,), FILL, dtype=torch.uint8, device=dev)
    sp = torch.full((8 * G * C.N_BLOCKS + 16,), FILL, dtype=torch.uint8, device=dev)
    good = dict(h=None, cov=cov.data_ptr(), n=C.N_BLOCKS, stride=1, pk=pk.data_ptr(), fl=fl.data_ptr(), sp=sp.data_ptr())

    def call(**kw):
        k = dict(good, **kw)
        return nat.lib.gacq_bearing_run_dev(k["h"], ctypes.c_void_p(k["cov"]), k["n"], k["stride"], ctypes.c_void_p(k["pk"]), ctypes.c_void_p(k["fl"]),
                                            ctypes.c_void_p(k["sp"]))

    engine.use_torch_stream(cov.device)
    assert call() == BAD_ARG                                                          # no handle
    with _finder(engine, a, u) as fd:
        good["h"] = fd._h
        big = 1 << 48
        for kw in (dict(cov=None), dict(pk=None), dict(fl=None), dict(cov=cov.data_ptr() + 4), dict(pk=pk.data_ptr() + 4), dict(fl=fl.data_ptr() + 4),
                   dict(sp=sp.data_ptr() + 4), dict(pk=pk.data_ptr() + 1), dict(n=-1), dict(stride=0), dict(stride=-1), dict(n=big + 1), dict(stride=big + 1),
                   dict(n=2, stride=big), dict(n=1 << 30, stride=1 << 30)):
            assert call(**kw) == BAD_ARG, kw
        assert b"gacq_bearing" in nat.lib.gacq_last_error(engine._ctx)
        assert call(n=0) == 0 and call(n=0, stride=big) == 0                          # nothing to do
        torch.cuda.synchronize()
        for t in (pk, fl, sp):
            assert bool((t == FILL).all())
        assert call() == 0                                                            # the unchanged call is accepted and writes
        torch.cuda.synchronize()
    want = C.reference(M, G) if (M, G) in C.SHAPES else B.run(*C.covariances(M), C.SHIFT, a, u, C.K, C.COS_SEP)
    assert pk[:-16].cpu().numpy().tobytes() == want[0].tobytes() and fl[:-16].cpu().numpy().tobytes() == want[1].tobytes()
    assert sp[:-16].cpu().numpy().tobytes() == want[2].tobytes() and all(bool((t[-16:] == FILL).all()) for t in (pk, fl, sp))
    # the configuration and the tables are checked when the handle is opened
    for bad in (dict(K=0), dict(K=5), dict(cos_sep=1.5), dict(cos_sep=float("nan")), dict(shift=41)):
        with pytest.raises(nat.GacqError):
            _finder(engine, a, u, **bad)
    for i, j, v in ((0, 0, float("nan")), (G - 1, M - 1, complex(0.0, float("inf")))):
        a2 = a.copy()
        a2[i, j] = v
        with pytest.raises(nat.GacqError):
            _finder(engine, a2, u)
    u2 = u.copy()
    u2[G - 1, 2] = float("-inf")
    with pytest.raises(nat.GacqError):
        _finder(engine, a, u2)
    with pytest.raises(nat.GacqError):
        _finder(engine, a[:, :1], u)                                                  # one antenna


def _dev(engine, x):
    torch = nat.require_torch()
    return torch.from_numpy(np.ascontiguousarray(x).view(np.int8).reshape(-1).copy()).to("cuda:%d" % engine.device)


@pytest.mark.gpu
def test_a_cut_recording_gives_the_records_of_the_whole(engine):
    """Finder on the window sums of Nuller.run: one call over the recording, then two calls that meet inside a block, each given only
    the input it needs; and both equal the oracle on the oracle's window sums"""
    import nulling_oracle as O
    name = "long-m3-b128-w3"
    M, Lb, Wn = NC.CASES[name][:3]
    xs = [x[:2 * (40 * Lb + 17)] for x in NC.data(name)]
    Nn = len(xs[0]) // 2
    a, u = C.table(M, 257)
    want = B.run(*B.window_sums(xs, Lb, Wn, list(range(41))), C.SHIFT, a, u, C.K, C.COS_SEP)
    with nulling.Nuller(engine, M, Lb, Wn) as nl, _finder(engine, a, u) as fd:
        _, cov = nl.run([_dev(engine, x) for x in xs], 0, 0, Nn, 1.0, "int8", cov=True)
        assert cov.shape == (41, M, M, 2)
        pk, fl, q = fd.run(cov, spectrum=True)
        _same((bearing.records(pk), fl.cpu().numpy(), q.cpu().numpy()), want, "whole")
        parts = []
        cut = 19 * Lb + 77
        for lo, hi in ((0, cut), (cut, Nn)):
            in_lo, in_hi = O.needed(Lb, Wn, lo, hi - lo)
            _, cv = nl.run([_dev(engine, x[2 * in_lo:2 * in_hi]) for x in xs], in_lo, lo, hi - lo, 1.0, "int8", cov=True)
            p2, f2 = fd.run(cv)
            parts.append((bearing.records(p2), f2.cpu().numpy()))
        assert [len(p[1]) for p in parts] == [20, 21]
        _same((np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]), None), want, "cut")
        # every third row of the device's own tensor
        p3, f3 = fd.run(cov[1:], 3)
        _same((bearing.records(p3), f3.cpu().numpy(), None), tuple(w[1::3] for w in want), "stride 3")


@pytest.mark.gpu
def test_command_line_trace_does_not_depend_on_the_piece_size(engine, tmp_path):
    name = "long-m3-b128-w3"
    M, Lb, Wn = NC.CASES[name][:3]
    xs = NC.data(name)
    paths = []
    for p, x in enumerate(xs):
        paths.append(str(tmp_path / ("ant%d.iq" % p)))
        x.tofile(paths[-1])
    Nn = len(xs[0]) // 2
    els = []
    for e in C.ring(M):
        els += ["--element", "%r,%r,%r" % tuple(float(v) for v in e)]
    args = els + ["--block", str(Lb), "--window", str(Wn), "--peaks", "2", "--every", "3", "--step", "10", "--trace", str(tmp_path / "t.txt"),
                  "--out", str(tmp_path / "out.iq")]
    traces, lines = [], []
    for piece in (1000, 7 * 2 * Lb, None):
        text = io.StringIO()
        lines.append(bearing.run(args + paths, out=text, **({} if piece is None else dict(piece_bytes=piece))))
        assert lines[-1] == text.getvalue().strip()
        traces.append(open(str(tmp_path / "t.txt"), "rb").read())
        out = open(str(tmp_path / "out.iq"), "rb").read()
        nulling.run(["--block", str(Lb), "--window", str(Wn), "--out", str(tmp_path / "ref.iq")] + paths, out=io.StringIO(),
                    **({} if piece is None else dict(piece_bytes=piece)))
        assert out == open(str(tmp_path / "ref.iq"), "rb").read() and len(out) == 2 * Nn
    assert traces[0] == traces[1] == traces[2] and lines[0] == lines[1] == lines[2]
    # the lines are those of the oracle on the blocks 0, 3, 6, ..
    cells = bearing.grid(10.0)
    a, u = bearing.tables(C.ring(M), cells)
    blocks = B.evaluated(Lb, 0, Nn, 3)
    rec, fl, _ = B.run(*B.window_sums(xs, Lb, Wn, blocks), 10, a, u, 2, float(np.cos(np.deg2rad(20.0))))
    want = "".join(bearing.trace_line(b, Lb, t) + "\n" for b, t in zip(blocks, bearing.report(cells, rec, fl)))
    assert traces[0].decode() == want and len(blocks) == -(-(-(-Nn // Lb)) // 3)
    assert lines[0] == bearing.summary_line(M, Lb, Wn, cells, rec) and lines[0].startswith("antennas 3 block 128 window 3 cells 360 blocks %d rank 0 az " % len(blocks))


@pytest.mark.gpu
def test_end_to_end_two_interferers_come_out_at_their_bearings(engine, tmp_path):
    """bearing_cases.E2E: a noise jammer at (70, 20) and a tone at (250, 50) on eight elements, made by scene.recording; ranks 0 and 1
    are those cells in every block past the warm-up, through Finder and through the command line on eight files"""
    E = C.E2E
    ems, el, gains = C.e2e_scene()
    cells, g_jam, g_tone = C.e2e_cells()
    n = E["blocks"] * E["block"] + 100
    x = scene.recording([], ems, gains, E["fs"], 0.0, n, E["seed"], E["sigma"], engine=engine)
    with nulling.Nuller(engine, 8, E["block"], E["window"], E["load_shift"]) as nl, \
            bearing.Finder(engine, el, cells, E["load_shift"], E["peaks"], E["sep"]) as fd:
        _, cov = nl.run([x[p] for p in range(8)], 0, 0, n, 1.0, "int8", cov=True)
        pk, fl = fd.run(cov)
        rec = bearing.records(pk)
        rep = fd.report(pk, fl)
    assert rec.shape == (E["blocks"] + 1, 3)
    print(rep[E["window"] + 1:, :, :])
    assert np.all(rec["cell"][E["window"] + 1:, 0] == g_jam) and np.all(rec["cell"][E["window"] + 1:, 1] == g_tone)
    assert np.all(rep[E["window"] + 1:, 0, 2] > rep[E["window"] + 1:, 1, 2]) and np.all(rep[E["window"] + 1:, 1, 2] > 10.0)
    # the device's records are the oracle's on the device's own window sums
    R = cov.cpu().numpy()
    a, u = bearing.tables(el, cells)
    want = B.run(R[..., 0], R[..., 1], E["load_shift"], a, u, E["peaks"], float(np.cos(np.deg2rad(E["sep"]))))
    _same((rec, fl.cpu().numpy(), None), want, "e2e")
    # the command line on eight files
    paths, args = [], []
    h = x.cpu().numpy()
    for p in range(8):
        paths.append(str(tmp_path / ("el%d.iq" % p)))
        h[p].tofile(paths[-1])
        args += ["--element", "%r,%r,%r" % tuple(float(v) for v in el[p])]
    line = bearing.run(args + paths, out=io.StringIO())
    f = line.split()
    assert f[:10] == "antennas 8 block 4096 window 8 cells 1368 blocks 15".split(), line
    assert f[10:17] == "rank 0 az 70.00 el 20.00 count".split() and f[18:25] == "rank 1 az 250.00 el 50.00 count".split(), line
    assert min(int(f[17]), int(f[25])) >= E["blocks"] - E["window"], line              # every block past the warm-up at the least
