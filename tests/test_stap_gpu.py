"""GPU: the space-time nulling kernels (csrc/gacq_stap.hip) against the definition of tests/stap_oracle.py.  The window sums of the
covariances, the output bytes and both counts are equalities of integers and bytes; the quantised weights are equal wherever no scaled
weight lies within 1e-6 of a rounding tie, which stap_cases.check_margins() asserts of every case here on the CPU.  T = 1 against a
Nuller run; device against device and against the oracle however the recording is cut into calls and wherever the inputs lie, each
call given only the input it needs; the refusals of gacq_stap_run_dev; the command line; then two scenes whose filtered output the
20 ms search finds the satellite in."""
import ctypes
import io

import numpy as np
import pytest

import nulling_cases as NC
import nulling_oracle as NO
import stap_cases as C
import stap_oracle as O
from gnss_dsp_tools_amd import _native as nat
from gnss_dsp_tools_amd import cancel, nulling, signals, simulate, stap

BAD_ARG, SHORT_INPUT = -1, -6


def _dev(engine, x, off=0, fill=None):
    """the int8 array on the device, its first byte `off` bytes past a 256-byte boundary; with fill the bytes around it hold that"""
    torch = nat.require_torch()
    x = np.ascontiguousarray(x).view(np.int8).reshape(-1)
    buf = torch.empty(len(x) + 1024, dtype=torch.int8, device="cuda:%d" % engine.device)
    if fill is not None:
        buf.fill_(fill)
    off += 256 + (-buf.data_ptr()) % 256
    v = buf[off:off + len(x)]
    v.copy_(torch.from_numpy(x))
    return v


def _inputs(engine, name, offs=None):
    xs = C.data(name)
    ds = [_dev(engine, x, 0 if offs is None else offs[p % len(offs)]) for p, x in enumerate(xs)]
    if C.CASES[name][5] == "shared":
        ds[2] = ds[0]                               # two antennas on one tensor
    return ds


def _open(engine, name):
    M, T, Lb, W = C.CASES[name][:4]
    return stap.Stap(engine, M, T, Lb, W, 10, C.constraint(name))


@pytest.fixture(scope="module", autouse=True)
def margins():
    return C.check_margins()


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in C.CASES if C.CASES[n][5] != "long"])
def test_window_sums_weights_bytes_and_counts_equal_the_oracle(engine, name):
    """every shape: one, two and seven 16-row tiles, a partial tile, taps that reach below sample 0 and across every block edge; the
    recordings are asymmetric between antennas and between I and Q, so a row / column swap, an I/Q swap, a tap counted the wrong way
    round or a sign error in Im C changes the integers"""
    M, T, Lb, W = C.CASES[name][:4]
    N, n = M * T, C.outputs(name)
    want = C.reference(name)
    with _open(engine, name) as sp:
        out, wq, cov = sp.run(_inputs(engine, name), 0, 0, n, 1.0, "int8", weights=True, cov=True)
        st = sp.stats()
    cov, wq = cov.cpu().numpy(), wq.cpu().numpy()
    assert cov.shape == want["cov"].shape == (-(-n // Lb), N, N, 2) and np.array_equal(cov, want["cov"]), (name, np.argwhere(cov != want["cov"])[:4])
    assert np.all(cov[:, np.arange(N), np.arange(N), 1] == 0)
    if C.CASES[name][5] == "min":
        assert cov[2, 0, 0, 0] == 2 * W * Lb * 16384 and np.all(cov[2, :, :, 0] == cov[2, 0, 0, 0])      # |G| = Lb 2^14 = 2^29, the largest
        assert cov[0, 0, 0, 0] == 2 * Lb * 16384 and cov[0, T - 1, T - 1, 0] == 2 * (Lb - 3) * 16384       # x(j - 3) does not exist for j < 3
    elif N > 1:
        assert np.any(cov[0, 0, 1] != cov[0, 1, 0]) and np.any(cov[..., 1] != 0)
    assert wq.dtype == np.int32 and np.array_equal(wq, want["wq"]), (name, np.argwhere(wq != want["wq"])[:4])
    if C.constraint(name) is None:
        assert np.all(wq[:, O.centre(T), 0] == 16384) and np.all(wq[:, O.centre(T), 1] == 0)
    assert np.array_equal(out.cpu().numpy(), want["out"]) and st == (want["clipped"], want["owned"]), (name, st)


@pytest.mark.gpu
@pytest.mark.parametrize("name", C.OUTPUT_CASES)
@pytest.mark.parametrize("dtype,gain", [("int8", 0.75), ("int8", 6.5), ("complex64", 0.75)])
def test_output_bytes_at_odd_input_addresses(engine, name, dtype, gain):
    """every antenna's first byte at another odd offset; a gain that clips many components, with the exact count"""
    n = C.outputs(name)
    want = C.reference(name, dtype == "complex64", gain)
    with _open(engine, name) as sp:
        out = sp.run(_inputs(engine, name, (1, 3, 5, 7, 9, 11, 13, 15)), 0, 0, n, gain, dtype)
        st = sp.stats()
    assert out.cpu().numpy().tobytes() == want["out"].tobytes() and st == (want["clipped"], want["owned"]), (name, st)
    assert want["clipped"] > 50 or name.startswith("shared") if (dtype == "int8" and gain > 1.0) else want["clipped"] <= 1


@pytest.mark.gpu
@pytest.mark.parametrize("M", C.NULLING_SHAPES)
def test_one_tap_is_nulling(engine, M):
    """T = 1 beside a Nuller on the same tensors: the same bytes, weights, window sums and counts"""
    name = "m%d-b128-w3" % M
    Lb, W = NC.CASES[name][1:3]
    xs = NC.data(name)
    n = len(xs[0]) // 2
    ds = [_dev(engine, x, 2 * p + 1) for p, x in enumerate(xs)]
    for dtype in ("int8", "complex64"):
        with nulling.Nuller(engine, M, Lb, W, 10) as nl, stap.Stap(engine, M, 1, Lb, W, 10) as sp:
            a = nl.run(ds, 0, 0, n, 2.5, dtype, weights=True, cov=True)
            b = sp.run(ds, 0, 0, n, 2.5, dtype, weights=True, cov=True)
            assert nl.stats() == sp.stats() and (sp.stats()[0] > 0) == (dtype == "int8")
        for u, v in zip(a, b):
            assert u.shape == v.shape and u.dtype == v.dtype and bool((u == v).all()), (M, dtype)
    assert np.array_equal(b[1].cpu().numpy(), NC.reference(name)["wq"])


@pytest.mark.gpu
def test_one_tap_file_pump_is_nullings(engine, tmp_path):
    """the command lines of both tools on the same two files, T = 1, in pieces of 100 bytes that cut samples' blocks and are held for the
    automatic gain's window: the same output and trace bytes, the same gain, clipped and sample counts, lines that differ by ` taps 1`
    alone, and the bytes of nulling_oracle.run -- at a fixed gain and at the automatic one"""
    Lb, W, n = 64, 2, 5 * 64 + 37
    xs = NC.recording(2, n, 90)                     # the seed was chosen on the CPU: the scaled weights keep 0.14 from a rounding tie
    assert NO.run(xs, 0, 0, n, Lb, W)["margin"] >= NC.MARGIN
    paths = [str(tmp_path / ("ant%d.iq" % p)) for p in range(2)]
    for x, path in zip(xs, paths):
        x.tofile(path)
    for fixed in (["--gain", "2.5"], []):
        got = {}
        for tool, extra in ((nulling, []), (stap, ["--taps", "1"])):
            out, trace = str(tmp_path / (tool.__name__ + ".iq")), str(tmp_path / (tool.__name__ + ".w"))
            line = tool.run(extra + ["--block", str(Lb), "--window", str(W), "--weights-trace", trace, "--out", out] + fixed + paths, out=io.StringIO(),
                            piece_bytes=100)
            got[tool] = (line, open(out, "rb").read(), open(trace, "rb").read())
        (nline, nout, ntrace), (sline, sout, strace) = got[nulling], got[stap]
        assert sout == nout and strace == ntrace and len(ntrace) == 8 * 2 * -(-n // Lb)
        assert sline.replace(" taps 1", "") == nline and sline != nline
        nw, sw = nline.split(), sline.split()
        gain, clipped, samples = float(nw[7]), int(nw[9]), int(nw[11])
        assert (float(sw[9]), int(sw[11]), int(sw[13])) == (gain, clipped, samples) and samples == n and (gain == 2.5) == bool(fixed)
        want = NO.run(xs, 0, 0, n, Lb, W, 10, None, gain)
        assert nout == want["out"].tobytes() and clipped == want["clipped"], (fixed, gain)


def _raw(sp, ds, in_first, out_first, n_out, cplx, out, stats, wq, cov, gain=2.5):
    ptrs = (ctypes.c_void_p * len(ds))(*[d.data_ptr() for d in ds])
    return nat.lib.gacq_stap_run_dev(sp._h, ctypes.cast(ptrs, ctypes.c_void_p), in_first, min(d.numel() for d in ds) // 2, out_first, n_out, gain, cplx,
                                     ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(stats.data_ptr()), ctypes.c_void_p(wq.data_ptr()),
                                     ctypes.c_void_p(cov.data_ptr()))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["long-m3-t3-b128-w3", "long-m8-t7-b4096-w1", "long-m1-t15-b192-w2"])
@pytest.mark.parametrize("dtype", ["int8", "complex64"])
def test_cuts_do_not_matter_and_every_call_gets_only_the_input_it_needs(engine, name, dtype):
    """calls that end and start on a workgroup tile, on a block edge, one lane's run before and after each, at odd places; every call
    is given exactly the input it needs -- t_c samples beyond its last output, t_c before the first block of its window -- as a slice,
    at an odd address, of a tensor whose neighbouring bytes are 127: a byte read from outside the range would change the result.  The
    first call starts at sample 0, where the taps reach below the recording.  One sample short at either end is refused and writes
    nothing."""
    torch = nat.require_torch()
    M, T, Lb, W = C.CASES[name][:4]
    xs = C.data(name)
    n = C.outputs(name)
    cfg = stap.make_cfg(M, T, Lb, W)
    assert nat.lib.gacq_stap_tile(ctypes.addressof(cfg)) == C.TILE and n > C.TILE + C.RUN and n % Lb
    want = C.reference(name, dtype == "complex64", 2.5)
    per = 1 if dtype == "complex64" else 2
    with _open(engine, name) as sp:
        whole, wq_whole = sp.run(_inputs(engine, name), 0, 0, n, 2.5, dtype, weights=True)
        st_whole = sp.stats()
    assert whole.cpu().numpy().tobytes() == want["out"].tobytes() and st_whole == (want["clipped"], want["owned"])
    pts = [0] + C.cuts(Lb, W, n) + [n]
    assert C.TILE in pts and C.TILE - C.RUN in pts and (W + 1) * Lb + C.RUN in pts
    dev = whole.device
    with _open(engine, name) as sp:
        for a, b in zip(pts, pts[1:]):
            lo, hi = O.needed(Lb, W, T, a, b - a)
            assert hi == max(b, W * Lb) + O.centre(T) and lo == max(max(a // Lb - W, 0) * Lb - O.centre(T), 0)
            ds = [_dev(engine, x[2 * lo:2 * hi], 2 * p + 1, fill=127) for p, x in enumerate(xs)]
            out, wq = sp.run(ds, lo, a, b - a, 2.5, dtype, weights=True)
            assert bool((out == whole[per * a:per * b]).all()), (name, a, b)
            blk = -(-a // Lb)
            assert bool((wq == wq_whole[blk:blk + wq.shape[0]]).all()) and wq.shape[0] == -(-b // Lb) - blk, (name, a, b)
        assert sp.stats() == st_whole
        # one sample short at either end: refused, and the sentinels stay
        sent = [torch.full((8 * Lb,), 77, dtype=torch.uint8, device=dev), torch.full((2,), 77, dtype=torch.int64, device=dev),
                torch.full((2 * M * T * 4,), 77, dtype=torch.int32, device=dev), torch.full((2 * (M * T) ** 2 * 4,), 77, dtype=torch.int64, device=dev)]
        engine.use_torch_stream(dev)
        for a, b in ((pts[0], pts[1]), (pts[3], pts[4]), (pts[-2], pts[-1])):
            b = min(b, a + Lb)
            lo, hi = O.needed(Lb, W, T, a, b - a)
            full = [_dev(engine, x[2 * lo:2 * hi], 1, fill=127) for x in xs]
            assert _raw(sp, [d[:-2] for d in full], lo, a, b - a, int(per == 1), *sent) == SHORT_INPUT, (a, b)
            assert "need input samples %d .. %d, present are %d .. %d" % (lo, hi - 1, lo, hi - 2) in nat.lib.gacq_last_error(engine._ctx).decode()
            if lo > 0:
                assert _raw(sp, [d[2:] for d in full], lo + 1, a, b - a, int(per == 1), *sent) == SHORT_INPUT, (a, b)
        torch.cuda.synchronize()
        assert all(bool((t == 77).all()) for t in sent) and sp.stats() == st_whole


@pytest.mark.gpu
def test_stream_feed_with_unequal_cuts_is_one_convert(engine):
    name = "long-m3-t3-b128-w3"
    M, T, Lb, W = C.CASES[name][:4]
    xs = C.data(name)
    want, st, wq = stap.convert(engine, xs, T, Lb, W, gain=2.5, weights=True)
    assert want.cpu().numpy().tobytes() == C.reference(name, False, 2.5)["out"].tobytes()
    s = stap.Stream(engine, M, 2.5, T, Lb, W, weights=True)
    outs, at = [], 0
    for size in (2 * 100, 2 * 283, 2 * 1, 2 * 3000, 2 * 64, 2 * 9001, 1 << 30):
        outs.append(s.feed([x[at:at + size] for x in xs]))
        at += size
    assert outs[0].numel() == 0 and outs[1].numel() == 0                                        # W blocks and t_c samples are not there yet
    torch = nat.require_torch()
    assert bool((torch.cat(outs) == want).all()) and s.stats() == st and bool((torch.cat(s.traces) == wq).all())
    s.close()


@pytest.mark.gpu
def test_far_calls_equal_the_near_call_on_the_same_bytes(engine):
    """out_first straddling 2^32 and at the last index the check accepts: the same bytes under another absolute index, a whole number of
    blocks away and past the warm-up, give the same output, weights and window sums"""
    name = "long-m3-t3-b128-w3"
    M, T, Lb, W = C.CASES[name][:4]
    tc = O.centre(T)
    xs = C.data(name)
    n_out = 2 * Lb + 11
    near = 16 * Lb                                                                              # the first output, on a block edge
    lo, hi = O.needed(Lb, W, T, near, n_out)
    ds = [_dev(engine, x[2 * lo:2 * hi], 2 * p + 1, fill=127) for p, x in enumerate(xs)]
    want = O.run([x[2 * lo:2 * hi] for x in xs], lo, near, n_out, Lb, W, T, 10, None, 2.5)
    with _open(engine, name) as sp:
        ref = sp.run(ds, lo, near, n_out, 2.5, "int8", weights=True, cov=True)
        assert ref[0].cpu().numpy().tobytes() == want["out"].tobytes() and np.array_equal(ref[1].cpu().numpy(), want["wq"])
        for far in ((1 << 32) - Lb, 1 << 48):
            got = sp.run(ds, far - (near - lo), far, n_out, 2.5, "int8", weights=True, cov=True)
            for u, v in zip(ref, got):
                assert u.shape == v.shape and bool((u == v).all()), far
        assert sp.stats() == (3 * want["clipped"], 3 * want["owned"])
        with pytest.raises(nat.GacqError):
            sp.run(ds, (1 << 48) + Lb - (near - lo), (1 << 48) + Lb, n_out, 2.5)
    assert tc == 1 and near - lo == W * Lb + tc


@pytest.mark.gpu
def test_refusals_of_run_dev_leave_the_outputs_untouched(engine):
    """every refusal through the raw ABI; out, stats, weights and cov keep their bytes"""
    torch = nat.require_torch()
    name = "m3-t3-b64-w1"
    M, T, Lb, W = C.CASES[name][:4]
    N, n = M * T, C.outputs(name)
    n_in = n + O.centre(T)
    ds = _inputs(engine, name)
    dev = ds[0].device
    out = torch.full((8 * n + 8,), 77, dtype=torch.uint8, device=dev)
    stats = torch.full((3,), 77, dtype=torch.int64, device=dev)
    wq = torch.full((2 * N * 8 + 1,), 77, dtype=torch.int32, device=dev)
    cov = torch.full((2 * N * N * 8 + 1,), 77, dtype=torch.int64, device=dev)
    ptrs = (ctypes.c_void_p * M)(*[d.data_ptr() for d in ds])
    holed = (ctypes.c_void_p * M)(ds[0].data_ptr(), None, ds[2].data_ptr())
    good = dict(h=None, d_in=ctypes.cast(ptrs, ctypes.c_void_p), in_first=0, in_count=n_in, out_first=0, n_out=n, gain=1.0, cplx=0, out=out.data_ptr(),
                stats=stats.data_ptr(), wq=wq.data_ptr(), cov=cov.data_ptr())

    def call(**kw):
        a = dict(good, **kw)
        return nat.lib.gacq_stap_run_dev(a["h"], a["d_in"], a["in_first"], a["in_count"], a["out_first"], a["n_out"], a["gain"], a["cplx"],
                                         ctypes.c_void_p(a["out"]), ctypes.c_void_p(a["stats"]), ctypes.c_void_p(a["wq"]), ctypes.c_void_p(a["cov"]))

    engine.use_torch_stream(dev)
    assert call() == BAD_ARG                                                          # no handle
    with _open(engine, name) as sp:
        good["h"] = sp._h
        big = (1 << 48) + 1
        for kw in (dict(d_in=None), dict(d_in=ctypes.cast(holed, ctypes.c_void_p)), dict(out=None), dict(cplx=1, out=out.data_ptr() + 4),
                   dict(stats=stats.data_ptr() + 4), dict(wq=wq.data_ptr() + 2), dict(cov=cov.data_ptr() + 4), dict(gain=0.0), dict(gain=float("nan")),
                   dict(gain=float("inf")), dict(gain=1e-50), dict(in_first=-1), dict(in_count=-1), dict(out_first=-1), dict(n_out=-1), dict(n_out=big),
                   dict(in_first=big), dict(in_count=big), dict(out_first=big)):
            assert call(**kw) == BAD_ARG, kw
        for kw in (dict(in_count=n_in - 1), dict(in_count=W * Lb, n_out=1), dict(in_first=1), dict(out_first=3 * Lb, n_out=10, in_first=2 * Lb),
                   dict(n_out=n + 1)):
            assert call(**kw) == SHORT_INPUT, kw
        assert "need input samples" in nat.lib.gacq_last_error(engine._ctx).decode()
        assert call(n_out=0) == 0 and call(n_out=0, in_count=0) == 0                  # nothing to do
        torch.cuda.synchronize()
        for t in (out, stats, wq, cov):
            assert bool((t == 77).all())
        assert call() == 0                                                            # the unchanged call is accepted and writes
        torch.cuda.synchronize()
    want = C.reference(name)
    assert out[:2 * n].cpu().numpy().view(np.int8).tobytes() == want["out"].tobytes() and bool((out[2 * n:] == 77).all())
    assert stats.cpu().tolist() == [77 + want["clipped"], 77 + want["owned"], 77]
    nb = want["owned"]
    assert np.array_equal(wq[:2 * N * nb].cpu().numpy().reshape(nb, N, 2), want["wq"]) and bool((wq[2 * N * nb:] == 77).all())
    assert np.array_equal(cov[:2 * N * N * nb].cpu().numpy().reshape(nb, N, N, 2), want["cov"]) and bool((cov[2 * N * N * nb:] == 77).all())
    # the configuration is checked when the handle is opened
    h = ctypes.c_void_p()
    for bad in (dict(M=0), dict(M=9), dict(taps=4), dict(taps=17), dict(M=8, taps=9), dict(block=100), dict(window=65), dict(load_shift=41),
                dict(constraint=[0, 0, 0])):
        d = dict(M=3, taps=3, block=128, window=1, load_shift=10, constraint=None)
        d.update(bad)
        cfg = stap.make_cfg(d["M"], d["taps"], d["block"], d["window"], d["load_shift"], d["constraint"] if d["M"] == 3 else None)
        assert nat.lib.gacq_stap_open(engine._ctx, ctypes.addressof(cfg), ctypes.byref(h)) == BAD_ARG and not h.value, bad


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["long-m1-t15-b192-w2", "long-m3-t3-b128-w3"])
def test_command_line(engine, tmp_path, name):
    """one file and three: the bytes of convert() at a small piece size and at the default, the printed line, the weights trace; the
    automatic gain does not depend on the piece size either"""
    M, T, Lb, W = C.CASES[name][:4]
    xs = [x[:2 * (C.TILE + 400 + 7 * p)] for p, x in enumerate(C.data(name))]                  # unequal files: the output ends with the shortest
    n_in = C.TILE + 400
    paths = []
    for p, x in enumerate(xs):
        paths.append(str(tmp_path / ("ant%d.iq" % p)))
        x.tofile(paths[-1])
    cut = [x[:2 * n_in] for x in xs]
    want, st, wq = stap.convert(engine, cut, T, Lb, W, gain=1.75, weights=True)
    want, wq = want.cpu().numpy().tobytes(), wq.cpu().numpy().tobytes()
    n = n_in - O.centre(T)
    assert len(want) == 2 * n and st[0] > 0
    args = ["--taps", str(T), "--block", str(Lb), "--window", str(W), "--weights-trace", str(tmp_path / "w.bin"), "--out", str(tmp_path / "out.iq")]
    for piece in (1000, None):
        text = io.StringIO()
        line = stap.run(args + ["--gain", "1.75"] + paths, out=text, **({} if piece is None else dict(piece_bytes=piece)))
        assert line == text.getvalue().strip() == "antennas %d taps %d block %d window %d gain 1.75 clipped %d samples %d" % (M, T, Lb, W, st[0], n)
        assert open(str(tmp_path / "out.iq"), "rb").read() == want and open(str(tmp_path / "w.bin"), "rb").read() == wq
    # the automatic gain: target rms over the rms of the first 65536 (here: all) outputs at gain 1
    unit = stap.convert(engine, cut, T, Lb, W, gain=1.0, dtype="complex64")[0].cpu().numpy()
    g = 32.0 / float(np.sqrt(np.mean(np.abs(unit.astype(np.complex128)) ** 2)))
    lines = [stap.run(args + paths, out=io.StringIO(), **kw) for kw in (dict(piece_bytes=3000), dict())]
    assert lines[0] == lines[1] and abs(float(lines[0].split()[9]) / g - 1.0) < 1e-6, (lines, g)
    auto = stap.convert(engine, cut, T, Lb, W, gain=float(lines[0].split()[9]))[0].cpu().numpy().tobytes()
    assert open(str(tmp_path / "out.iq"), "rb").read() == auto != want
    # complex64 output to a file
    stap.run(args + ["--gain", "1.75", "--complex64"] + paths, out=io.StringIO(), piece_bytes=5000)
    assert open(str(tmp_path / "out.iq"), "rb").read() == stap.convert(engine, cut, T, Lb, W, gain=1.75, dtype="complex64")[0].cpu().numpy().tobytes()


def _code_error(got, want, L=1023.0):
    return abs((got - want + L / 2.0) % L - L / 2.0)


def _scene(engine, E):
    """the antennas of a stap_cases scene as int8 CUDA tensors, built on the device from complex64 recordings"""
    torch = nat.require_torch()
    fs, W, Lb = E["fs"], E["window"], E["block"]
    w0 = (W + 1) * Lb
    n = w0 + int(fs * 0.001 * (E["ms"] + 5)) + 8 + 7
    quiet = simulate.Satellite(E["signal"], E["prn"], 0.0, 0.0, 0.0)
    jam = simulate.recording([quiet], fs, 0.0, n, E["jam_seed"], E["jam"], dtype="complex64", engine=engine) if E["jam"] else None
    j = torch.arange(n, dtype=torch.int64, device="cuda:%d" % engine.device)
    xs = []
    for p in range(E["antennas"]):
        sat = simulate.Satellite(E["signal"], E["prn"], E["amp"], E["doppler"], E["code_phase"], carrier_phase=E["sat_phase"][p])
        v = simulate.recording([sat], fs, 0.0, n, E["noise_seeds"][p], E["sigma"], dtype="complex64", engine=engine)
        if jam is not None:
            v = v + jam * complex(np.exp(2j * np.pi * E["jam_phase"][p]))
        for amp, num, den, step in E["tones"]:
            turn = ((j * num) % den).to(torch.float64) / den + step * p
            v = v + torch.polar(torch.full_like(turn, amp), 2.0 * np.pi * turn).to(torch.complex64)
        xs.append(torch.view_as_real(v).round().clamp(-127, 127).to(torch.int8).reshape(-1).contiguous())
    return xs, w0, n, sat


def _searched(engine, E, x, w0):
    return cancel.reacquire(engine, signals.get(E["signal"]), x, E["fs"], 0.0, w0, [E["prn"]], E["doppler_search"], E["ms"])[0][1]


def _end_to_end(engine, E, misses):
    """the 20 ms search on antenna 0 and on the outputs at the tap counts `misses` puts PRN 17 into a wrong cell, on the output at
    E["taps"] into the true one"""
    fs, Lb, W, T = E["fs"], E["block"], E["window"], E["taps"]
    xs, w0, n, sat = _scene(engine, E)
    true_code = (E["code_phase"] + w0 * sat.code_rate_hz() / fs) % 1023.0
    true_bin = 200.0 * round(E["doppler"] / 200.0)
    one_sample = 1.023e6 / fs
    hit = lambda r: r[2] == true_bin and _code_error(r[1], true_code) <= one_sample
    x0 = xs[0].cpu().numpy()
    pin = float(np.mean(x0[2 * w0:].astype(np.float64) ** 2))
    before = _searched(engine, E, x0, w0)
    print("true cell: code %.2f doppler %.0f;  antenna 0: metric %.2f code %.2f doppler %.0f power %.1f" % ((true_code, true_bin) + tuple(before) + (pin,)))
    assert not hit(before)
    for Tm in misses:
        y, st = stap.convert(engine, xs, Tm, Lb, W, gain=1.0)
        r = _searched(engine, E, y.cpu().numpy(), w0)
        print("T = %d: metric %.2f code %.2f doppler %.0f clipped %d" % ((Tm,) + tuple(r) + (st[0],)))
        assert not hit(r), Tm
    out, st, wq = stap.convert(engine, xs, T, Lb, W, gain=1.0, weights=True)                  # gain 1: the reference antenna's own scale
    assert out.numel() == 2 * (n - O.centre(T)) and st[1] == -(-(n - O.centre(T)) // Lb)
    wq = wq.cpu().numpy()
    assert wq.shape[1] == E["antennas"] * T and np.all(wq[:, O.centre(T), 0] == 16384) and np.all(wq[:, O.centre(T), 1] == 0)
    y = out.cpu().numpy()
    after = _searched(engine, E, y, w0)
    pout = float(np.mean(y[2 * w0:].astype(np.float64) ** 2))
    print("T = %d: metric %.2f code %.2f doppler %.0f power %.1f clipped %d" % ((T,) + tuple(after) + (pout, st[0])))
    assert hit(after) and pout < 0.5 * pin and after[0] > before[0]


@pytest.mark.gpu
def test_end_to_end_one_antenna_two_tones(engine):
    """two tones of amplitude 30 hide PRN 17 at amplitude 1 under noise of sigma 6 (stap_cases.E2E_TONES has the CPU experiment that
    fixed the level): the nine-tap adaptive notch brings it back, with no frames and no thresholds"""
    _end_to_end(engine, C.E2E_TONES, ())


@pytest.mark.gpu
def test_end_to_end_three_antennas_a_jammer_and_two_tones(engine):
    """a broadband jammer uses up the spatial degrees of freedom and the tones pass: one tap (nulling.py's computation) misses, three
    taps find the satellite (stap_cases.E2E_ARRAY)"""
    _end_to_end(engine, C.E2E_ARRAY, (1,))
