"""GPU: the beams kernels (csrc/gacq_beams.hip).  The contract is an equality: every byte of output k, its quantised weights and its clip
count are what nulling gives under constraint c_k and gain_k -- so beam k is held to tests/nulling_oracle.py under c_k (the margins of
beams_cases.check_margins() apply, asserted on the CPU) and, device against device, to Nuller(constraint=c_k), whatever K, the other
beams, their order, the output addresses and the cuts into calls are.  Then the refusals of gacq_beams_run_dev, the stream, the file
pump and the command line, and a scene of three satellites under a jammer whose beams find each its own satellite."""
import ctypes
import io

import numpy as np
import pytest

import array_chunk_cases as AC
import beams_cases as B
import nulling_oracle as O
from gnss_dsp_tools_amd import _native as nat
from gnss_dsp_tools_amd import beams, nulling

BAD_ARG, SHORT_INPUT = -1, -6
FILL = 0xA5


def _dev(engine, x, off=0):
    """the int8 array on the device between bytes of 127, its first byte `off` bytes past a 256-byte boundary"""
    torch = nat.require_torch()
    x = np.ascontiguousarray(x).view(np.int8).reshape(-1)
    buf = torch.full((len(x) + 512,), 127, dtype=torch.int8, device="cuda:%d" % engine.device)
    off += (-buf.data_ptr()) % 256
    v = buf[off:off + len(x)]
    v.copy_(torch.from_numpy(x))
    return v


def _inputs(engine, name):
    """every antenna at an odd address"""
    ds = [_dev(engine, x, 2 * p + 1) for p, x in enumerate(B.data(name))]
    if B.CASES[name][5] == "shared":
        ds[2] = ds[0]                               # two antennas on one tensor
    return ds


def _former(engine, name, ks=None):
    M, K, Lb, W = B.CASES[name][:4]
    cs = B.constraints(name)
    return beams.Beamformer(engine, M, [cs[k] for k in (range(K) if ks is None else ks)], Lb, W, B.LOAD_SHIFT)


class Outs:
    """K outputs of n samples in sentinel-filled buffers, output k at an odd byte address (complex64: on 8 bytes, off 16)"""

    def __init__(self, engine, K, n, cplx):
        torch = nat.require_torch()
        self.size = n * (8 if cplx else 2)
        self.bufs = [torch.full((self.size + 512,), FILL, dtype=torch.uint8, device="cuda:%d" % engine.device) for _ in range(K)]
        self.offs = [(-b.data_ptr()) % 256 + (8 * (2 * k + 1) if cplx else 2 * k + 1) for k, b in enumerate(self.bufs)]
        self.views = [b[o:o + self.size] for b, o in zip(self.bufs, self.offs)]

    def untouched_around(self):
        return all(bool((b[:o] == FILL).all()) and bool((b[o + self.size:] == FILL).all()) for b, o in zip(self.bufs, self.offs))

    def bytes(self, k):
        return self.views[k].cpu().numpy().tobytes()


def _raw(engine, bf, ds, in_first, in_count, out_first, n_out, gains, cplx, outs, stats, wq=None, cov=None):
    """gacq_beams_run_dev through the raw ABI on torch's stream"""
    engine.use_torch_stream(ds[0].device)
    ptrs = (ctypes.c_void_p * len(ds))(*[d.data_ptr() for d in ds])
    g = (ctypes.c_double * len(gains))(*gains)
    o = (ctypes.c_void_p * len(outs))(*[t.data_ptr() for t in outs])
    return nat.lib.gacq_beams_run_dev(bf._h, ctypes.cast(ptrs, ctypes.c_void_p), in_first, in_count, out_first, n_out, ctypes.cast(g, ctypes.c_void_p),
                                      int(cplx), ctypes.cast(o, ctypes.c_void_p), ctypes.c_void_p(stats.data_ptr()) if stats is not None else None,
                                      ctypes.c_void_p(wq.data_ptr()) if wq is not None else None, ctypes.c_void_p(cov.data_ptr()) if cov is not None else None)


@pytest.fixture(scope="module", autouse=True)
def margins():
    return B.check_margins()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["int8", "complex64"])
@pytest.mark.parametrize("name", list(B.CASES))
def test_every_beam_equals_the_nulling_oracle_under_its_constraint(engine, name, dtype):
    """bytes, clipped[k], owned, d_weights[:, k] and d_cov of every beam of every case; int8 at a clipping gain of the beam's own,
    complex64 at gain 1; every antenna and every output at an odd byte address (complex64 outputs on 8)"""
    torch = nat.require_torch()
    M, K, Lb, W = B.CASES[name][:4]
    cplx = dtype == "complex64"
    N = len(B.data(name)[0]) // 2
    nblk = -(-N // Lb)
    ds = _inputs(engine, name)
    dev = ds[0].device
    outs = Outs(engine, K, N, cplx)
    stats = torch.zeros(K + 2, dtype=torch.int64, device=dev)
    wq = torch.full((nblk, K, M, 2), 77, dtype=torch.int32, device=dev)
    cov = torch.full((nblk, M, M, 2), 77, dtype=torch.int64, device=dev)
    with _former(engine, name) as bf:
        rc = _raw(engine, bf, ds, 0, N, 0, N, [1.0] * K if cplx else B.gains(name), cplx, outs.views, stats, wq, cov)
        assert rc == 0, nat.lib.gacq_last_error(engine._ctx)
        torch.cuda.synchronize()
    wq, cov, st = wq.cpu().numpy(), cov.cpu().numpy(), stats.cpu().tolist()
    assert outs.untouched_around() and st[K + 1] == 0
    for k in range(K):
        want = B.reference(name, k, cplx)
        assert outs.bytes(k) == want["out"].tobytes(), (name, k)
        assert np.array_equal(wq[:, k], want["wq"]), (name, k, np.argwhere(wq[:, k] != want["wq"])[:4])
        assert (st[k], st[K]) == (want["clipped"], want["owned"]) and want["owned"] == nblk, (name, k, st)
        if k == 0:
            assert np.array_equal(cov, want["cov"]), name


def _against_nullers(engine, ds, M, Lb, W, cs, gains, in_first, out_first, n_out, dtype):
    """one beams call against K nulling calls on the same device inputs: bytes, weights, counts"""
    with beams.Beamformer(engine, M, cs, Lb, W, B.LOAD_SHIFT) as bf:
        got, wq = bf.run(ds, in_first, out_first, n_out, gains, dtype, weights=True)
        clipped, owned = bf.stats()
    assert len(got) == len(cs) and wq.shape[1:] == (len(cs), M, 2)
    for k, c in enumerate(cs):
        with nulling.Nuller(engine, M, Lb, W, B.LOAD_SHIFT, c) as nl:
            want, wk = nl.run(ds, in_first, out_first, n_out, gains[k], dtype, weights=True)
            st = nl.stats()
        assert bool((got[k] == want).all()) and bool((wq[:, k] == wk).all()) and (clipped[k], owned) == st, (k, st, clipped, owned)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["int8", "complex64"])
def test_the_long_case_equals_k_nulling_calls_whole_and_from_a_mid_block_start(engine, dtype):
    name = "long-m3-k9-b192-w2"
    M, K, Lb, W = B.CASES[name][:4]
    ds = _inputs(engine, name)
    N = len(B.data(name)[0]) // 2
    cs = list(B.constraints(name))
    _against_nullers(engine, ds, M, Lb, W, cs, B.gains(name), 0, 0, N, dtype)
    o = (W + 1) * Lb + 5
    _against_nullers(engine, ds, M, Lb, W, cs, B.gains(name), 0, o, N - o, dtype)


@pytest.mark.gpu
def test_a_call_of_several_launch_chunks_equals_k_nulling_calls(engine):
    """M = 2, K = 9, Lb = 64, W = 3 on the 2^14 + 5 blocks of array_chunk_cases' case B: the second chunk has pb0 > 0, shares an apply tile
    with the first and adds to the counters a second time.  test_array_chunks_gpu.py holds nulling to the oracle there."""
    tool, M, T, W, chunk, blocks, seed, _ = AC.CASES["B"]
    n = AC.outputs("B")
    assert AC.chunks_of("B", 0, n) == 2 and (M, W, AC.Lb) == (2, 3, 64)
    ds = [_dev(engine, x, 2 * p + 1) for p, x in enumerate(AC.data("B"))]
    cs = list(B.constraints("m2-k9-b64-w1"))
    assert len(cs) == 9
    gains = [2.5 + 0.25 * k for k in range(9)]
    _against_nullers(engine, ds, M, AC.Lb, W, cs, gains, 0, 0, n, "int8")
    o = AC.mid_first("B")
    _against_nullers(engine, ds, M, AC.Lb, W, cs, gains, 0, o, n - o, "int8")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["int8", "complex64"])
def test_a_beam_does_not_know_the_other_beams(engine, dtype):
    """permuting the beams permutes the outputs and nothing else; a subset of the beams gives those beams' bytes; identical beams
    give identical bytes"""
    name = "m3-k9-b128-w1"
    M, K, Lb, W = B.CASES[name][:4]
    N = len(B.data(name)[0]) // 2
    ds = _inputs(engine, name)
    g = B.gains(name)
    with _former(engine, name) as bf:
        whole, wq = bf.run(ds, 0, 0, N, g, dtype, weights=True)
        st = bf.stats()
    for ks in ([8, 7, 6, 5, 4, 3, 2, 1, 0], [3, 0, 8, 1, 7, 2, 6, 5, 4], [8, 0, 3], [4], [5, 5, 2, 5]):
        with _former(engine, name, ks) as bf:
            got, w = bf.run(ds, 0, 0, N, [g[k] for k in ks], dtype, weights=True)
            s = bf.stats()
        for i, k in enumerate(ks):
            assert bool((got[i] == whole[k]).all()) and bool((w[:, i] == wq[:, k]).all()) and s[0][i] == st[0][k], (ks, i)
        assert s[1] == st[1]
    assert dtype == "complex64" or min(st[0]) > 0
    name = "twin-m3-k3-b64-w3"
    with _former(engine, name) as bf:
        got = bf.run(_inputs(engine, name), 0, 0, len(B.data(name)[0]) // 2, [3.0, 7.0, 7.0], dtype)
        s = bf.stats()
    assert bool((got[1] == got[2]).all()) and not bool((got[0] == got[1]).all()) and s[0][1] == s[0][2]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["int8", "complex64"])
def test_cuts_do_not_matter(engine, dtype):
    """calls that end and start on a workgroup tile, on a block edge, one lane's run before and after each, at odd places, the warm-up
    included; every call is given only the input it needs, between bytes of 127, and writes between sentinels"""
    torch = nat.require_torch()
    name = "long-m3-k9-b192-w2"
    M, K, Lb, W = B.CASES[name][:4]
    xs = B.data(name)
    N = len(xs[0]) // 2
    cplx = dtype == "complex64"
    per = 8 if cplx else 2
    assert nat.lib.gacq_beams_tile(ctypes.addressof(beams.make_cfg(M, [None] * K, Lb, W))) == B.TILE and N > B.TILE + B.RUN and N % Lb
    g = [1.0] * K if cplx else B.gains(name)
    with _former(engine, name) as bf:
        whole, wq_whole = bf.run(_inputs(engine, name), 0, 0, N, g, dtype, weights=True)
        st_whole = bf.stats()
    whole = [w.view(torch.uint8) if not cplx else torch.view_as_real(w).reshape(-1).view(torch.uint8) for w in whole]
    for k in (0, 4, 8):
        assert whole[k].cpu().numpy().tobytes() == B.reference(name, k, cplx)["out"].tobytes()
    pts = [0] + B.NC.cuts(Lb, W, N) + [N]
    assert B.TILE in pts and B.TILE - B.RUN in pts and (W + 1) * Lb + B.RUN in pts and W * Lb + 3 in pts
    dev = whole[0].device
    stats = torch.zeros(K + 1, dtype=torch.int64, device=dev)
    with _former(engine, name) as bf:
        for a, b in zip(pts, pts[1:]):
            lo, hi = O.needed(Lb, W, a, b - a)
            ds = [_dev(engine, x[2 * lo:2 * hi], 2 * p + 1) for p, x in enumerate(xs)]
            outs = Outs(engine, K, b - a, cplx)
            blk = -(-a // Lb)
            nb = -(-b // Lb) - blk
            wq = torch.full((nb + 1, K, M, 2), 77, dtype=torch.int32, device=dev)
            assert _raw(engine, bf, ds, lo, hi - lo, a, b - a, g, cplx, outs.views, stats, wq) == 0, (a, b)
            torch.cuda.synchronize()
            assert outs.untouched_around(), (a, b)
            for k in range(K):
                assert bool((outs.views[k] == whole[k][per * a:per * b]).all()), (a, b, k)
            assert bool((wq[:nb] == wq_whole[blk:blk + nb]).all()) and bool((wq[nb] == 77).all()), (a, b)
    st = stats.cpu().tolist()
    assert (st[:K], st[K]) == st_whole


@pytest.mark.gpu
def test_refusals_of_run_dev_leave_the_outputs_untouched(engine):
    """every refusal through the raw ABI; the outputs, stats, weights and cov keep their bytes"""
    torch = nat.require_torch()
    name = "m3-k2-b64-w1"
    M, K, Lb, W = B.CASES[name][:4]
    N = len(B.data(name)[0]) // 2
    ds = _inputs(engine, name)
    dev = ds[0].device
    outs = Outs(engine, K, N, True)                                                          # room for either form
    stats = torch.full((K + 2,), 77, dtype=torch.int64, device=dev)
    nb = -(-N // Lb)
    wq = torch.full((2 * M * K * nb + 1,), 77, dtype=torch.int32, device=dev)
    cov = torch.full((2 * M * M * nb + 1,), 77, dtype=torch.int64, device=dev)
    ptrs = (ctypes.c_void_p * M)(*[d.data_ptr() for d in ds])
    holed = (ctypes.c_void_p * M)(ds[0].data_ptr(), None, ds[2].data_ptr())
    ops = (ctypes.c_void_p * K)(*[v.data_ptr() for v in outs.views])
    o_holed = (ctypes.c_void_p * K)(outs.views[0].data_ptr(), None)
    o_off = (ctypes.c_void_p * K)(outs.views[0].data_ptr(), outs.views[1].data_ptr() + 4)
    good = dict(h=None, d_in=ctypes.cast(ptrs, ctypes.c_void_p), in_first=0, in_count=N, out_first=0, n_out=N, gain=[1.0, 2.0], cplx=0,
                out=ctypes.cast(ops, ctypes.c_void_p), stats=stats.data_ptr(), wq=wq.data_ptr(), cov=cov.data_ptr())

    def call(**kw):
        a = dict(good, **kw)
        g = None if a["gain"] is None else ctypes.cast((ctypes.c_double * K)(*a["gain"]), ctypes.c_void_p)
        return nat.lib.gacq_beams_run_dev(a["h"], a["d_in"], a["in_first"], a["in_count"], a["out_first"], a["n_out"], g, a["cplx"], a["out"],
                                          ctypes.c_void_p(a["stats"]), ctypes.c_void_p(a["wq"]), ctypes.c_void_p(a["cov"]))

    engine.use_torch_stream(dev)
    assert call() == BAD_ARG                                                                  # no handle
    with _former(engine, name) as bf:
        good["h"] = bf._h
        big = (1 << 48) + 1
        for kw in (dict(d_in=None), dict(d_in=ctypes.cast(holed, ctypes.c_void_p)), dict(out=None), dict(out=ctypes.cast(o_holed, ctypes.c_void_p)),
                   dict(cplx=1, out=ctypes.cast(o_off, ctypes.c_void_p)), dict(stats=stats.data_ptr() + 4), dict(wq=wq.data_ptr() + 2),
                   dict(cov=cov.data_ptr() + 4), dict(gain=None), dict(gain=[0.0, 1.0]), dict(gain=[1.0, 0.0]), dict(gain=[1.0, float("nan")]),
                   dict(gain=[float("inf"), 1.0]), dict(gain=[1.0, 1e-50]), dict(gain=[1.0, -2.0]), dict(in_first=-1), dict(in_count=-1),
                   dict(out_first=-1), dict(n_out=-1), dict(n_out=big), dict(in_first=big), dict(in_count=big), dict(out_first=big)):
            assert call(**kw) == BAD_ARG, kw
        for kw in (dict(in_count=N - 1), dict(in_count=W * Lb - 1, n_out=1), dict(in_first=1), dict(out_first=3 * Lb, n_out=10, in_first=2 * Lb + 1),
                   dict(n_out=N + 1)):
            assert call(**kw) == SHORT_INPUT, kw
        assert "need input samples" in nat.lib.gacq_last_error(engine._ctx).decode()
        assert call(n_out=0) == 0 and call(n_out=0, in_count=0) == 0                          # nothing to do
        torch.cuda.synchronize()
        for t in [stats, wq, cov] + outs.bufs:
            assert bool((t == (FILL if t.dtype == torch.uint8 else 77)).all())
        assert call() == 0                                                                    # the unchanged call is accepted and writes
        torch.cuda.synchronize()
    st = stats.cpu().tolist()
    wq = wq.cpu().numpy()
    assert bool((wq[2 * M * K * nb:] == 77).all()) and st[K + 1] == 77
    for k in range(K):
        want = O.run(list(B.data(name)), 0, 0, N, Lb, W, B.LOAD_SHIFT, B.constraints(name)[k], [1.0, 2.0][k], False)
        assert outs.views[k][:2 * N].cpu().numpy().tobytes() == want["out"].tobytes() and bool((outs.views[k][2 * N:] == FILL).all())
        assert (st[k], st[K]) == (77 + want["clipped"], 77 + want["owned"])
        assert np.array_equal(wq[:2 * M * K * nb].reshape(nb, K, M, 2)[:, k], want["wq"])
    assert np.array_equal(cov[:2 * M * M * nb].cpu().numpy().reshape(nb, M, M, 2), want["cov"]) and bool((cov[2 * M * M * nb:] == 77).all())
    # the configuration is checked when the handle is opened
    h = ctypes.c_void_p()
    for bad in (dict(M=1), dict(block=100), dict(window=65), dict(load_shift=41), dict(cs=[None, [0, 0, 0]]), dict(K=0), dict(K=17)):
        d = dict(M=3, block=128, window=1, load_shift=10, cs=[None, None], K=2)
        d.update(bad)
        cfg = beams.make_cfg(d["M"], d["cs"], d["block"], d["window"], d["load_shift"])
        cfg.beams = d["K"]
        assert nat.lib.gacq_beams_open(engine._ctx, ctypes.addressof(cfg), ctypes.byref(h)) == BAD_ARG and not h.value, bad


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["int8", "complex64"])
def test_the_stream_is_the_whole_recording(engine, dtype):
    """pieces of two sizes, neither a multiple of a block: the concatenation of what feed() returns, the weights and the counts are
    convert()'s"""
    torch = nat.require_torch()
    name = "long-m3-k9-b192-w2"
    M, K, Lb, W = B.CASES[name][:4]
    xs = B.data(name)
    cs = list(B.constraints(name))
    g = B.gains(name)
    want, st, wq = beams.convert(engine, xs, cs, Lb, W, B.LOAD_SHIFT, g, dtype, weights=True)
    assert len(want) == K and st[1] == -(-(len(xs[0]) // 2) // Lb) and (dtype == "complex64" or min(st[0]) > 0)
    for piece in (1000, 2 * 5003):
        s = beams.Stream(engine, M, g, cs, Lb, W, B.LOAD_SHIFT, dtype, weights=True)
        got = [[] for _ in range(K)]
        for at in range(0, len(xs[0]), piece):
            for k, y in enumerate(s.feed([x[at:at + piece] for x in xs])):
                got[k].append(y)
        assert all(bool((torch.cat(got[k]) == want[k]).all()) for k in range(K)) and s.stats() == st, piece
        assert bool((torch.cat(s.traces) == wq).all())
        s.close()


@pytest.mark.gpu
def test_files_and_the_command_line(engine, tmp_path):
    """convert_files at two piece sizes with a shorter last antenna file, the weights trace, the automatic per-beam gains, and the
    command line end to end on temporary files"""
    name = "long-m3-k9-b192-w2"
    M, K, Lb, W = B.CASES[name][:4]
    N = B.TILE + 400
    xs = list(B.data(name))
    xs[2] = xs[2][:2 * N]                                                                     # the last antenna's file is shorter: the outputs end with it
    ks = [0, 1, 5]
    cs = [B.constraints(name)[k] for k in ks]
    paths = []
    for p, x in enumerate(xs):
        paths.append(str(tmp_path / ("ant%d.iq" % p)))
        x.tofile(paths[-1])
    cut = [x[:2 * N] for x in xs]
    g = [1.75, 3.0, 6.0]
    want, st, wq = beams.convert(engine, cut, cs, Lb, W, gains=g, weights=True)
    want, wq = [w.cpu().numpy().tobytes() for w in want], wq.cpu().numpy().tobytes()
    assert all(len(w) == 2 * N for w in want) and min(st[0]) > 0
    outs = [str(tmp_path / ("beam%d.iq" % k)) for k in range(3)]
    for piece in (1000, None):
        fins, fouts, ftrace = [open(p, "rb") for p in paths], [open(o, "wb") for o in outs], open(str(tmp_path / "w.bin"), "wb")
        got = beams.convert_files(engine, fins, fouts, cs, Lb, W, gains=g, ftrace=ftrace, **({} if piece is None else dict(piece_bytes=piece)))
        for f in fins + fouts + [ftrace]:
            f.close()
        assert got == (g, N, st[0])
        assert [open(o, "rb").read() for o in outs] == want and open(str(tmp_path / "w.bin"), "rb").read() == wq
    # the command line: the entries as arrayprompt prints them, a fixed gain for all beams
    args = ["--block", str(Lb), "--window", str(W), "--weights-trace", str(tmp_path / "w.bin")]
    for p in paths:
        args += ["--antenna", p]
    for o, c in zip(outs, cs):
        args += ["--beam", o] + ["%r,%r" % (float(z.real), float(z.imag)) for z in c]
    want2, st2 = beams.convert(engine, cut, cs, Lb, W, gains=1.75)
    for piece in (1000, None):
        text = io.StringIO()
        lines = beams.run(args + ["--gain", "1.75"], out=text, **({} if piece is None else dict(piece_bytes=piece)))
        assert lines == text.getvalue().strip().split("\n") == ["antennas 3 beams 3 block %d window %d samples %d" % (Lb, W, N)] + \
            ["beam %d gain 1.75 clipped %d" % (k, st2[0][k]) for k in range(3)]
        assert [open(o, "rb").read() for o in outs] == [w.cpu().numpy().tobytes() for w in want2] and open(str(tmp_path / "w.bin"), "rb").read() == wq
    # the automatic gains: per beam, target rms over the rms of the beam's first 65536 (here: all) outputs at gain 1, whatever the pieces
    unit = beams.convert(engine, cut, cs, Lb, W, gains=1.0, dtype="complex64")[0]
    auto = [32.0 / float(np.sqrt(np.mean(np.abs(u.cpu().numpy().astype(np.complex128)) ** 2))) for u in unit]
    assert beams.auto_gains(engine, cut, cs, Lb, W) == [float(v.split()[3]) for v in beams.run(args, out=io.StringIO())[1:]]
    runs = [beams.run(args, out=io.StringIO(), **kw) for kw in (dict(piece_bytes=3000), dict())]
    gs = [float(v.split()[3]) for v in runs[0][1:]]
    assert runs[0] == runs[1] and all(abs(a / b - 1.0) < 1e-6 for a, b in zip(gs, auto)) and len(set(gs)) == 3, (runs, auto)
    again = beams.convert(engine, cut, cs, Lb, W, gains=gs)[0]
    assert [open(o, "rb").read() for o in outs] == [w.cpu().numpy().tobytes() for w in again]
    # complex64 output to files
    beams.run(args + ["--gain", "1.75", "--complex64"], out=io.StringIO(), piece_bytes=5000)
    c64 = beams.convert(engine, cut, cs, Lb, W, gains=1.75, dtype="complex64")[0]
    assert [open(o, "rb").read() for o in outs] == [w.cpu().numpy().tobytes() for w in c64]


@pytest.mark.gpu
def test_end_to_end_every_beam_finds_its_own_satellite(engine):
    """three satellites at amplitude 0.25 under noise of sigma 6 and a jammer of 42 on four antennas (beams_cases.E2E has the CPU
    experiment that fixed the amplitude): each beam finds its PRN in the true cell, with a larger metric than the power-inversion
    output gives that PRN, which misses PRN 5.  Only what the CPU table showed with margin is asserted: the device scene's noise is
    not the fp64 oracle's bit for bit."""
    from gnss_dsp_tools_amd import cancel, scene, signals
    E = B.E2E
    sats, emitters, gains, cs, w0, n = B.e2e_scene()
    xs = scene.recording(sats, emitters, gains, E["fs"], 0.0, n, E["seed"], E["sigma"], engine=engine)
    outs, st = beams.convert(engine, [xs[p] for p in range(4)], cs, E["block"], E["window"], gains=1.0)
    assert len(outs) == 4 and all(o.numel() == 2 * n for o in outs) and st == ([0, 0, 0, 0], -(-n // E["block"]))
    sig = signals.get(E["signal"])
    ys = [o.cpu().numpy() for o in outs]
    power = [float(np.mean(y[2 * w0:].astype(np.float64) ** 2)) for y in ys]
    for k, s in enumerate(sats):
        pi = cancel.reacquire(engine, sig, ys[0], E["fs"], 0.0, w0, [s.item], E["doppler_search"], E["ms"])[0][1]
        beam = cancel.reacquire(engine, sig, ys[1 + k], E["fs"], 0.0, w0, [s.item], E["doppler_search"], E["ms"])[0][1]
        print("prn %d true cell %.2f %.0f: power inversion %.2f %.2f %.0f power %.1f   beam %.2f %.2f %.0f power %.1f"
              % ((s.item,) + B.e2e_true_cell(s, w0) + tuple(pi) + (power[0],) + tuple(beam) + (power[1 + k],)))
        assert B.e2e_hit(beam, s, w0) and beam[0] > pi[0], (s.item, pi, beam)
        if s.item in E["missed"]:
            assert not B.e2e_hit(pi, s, w0), (s.item, pi)
        assert power[1 + k] < 0.5 * power[0]
