"""GPU: the nulling kernels (csrc/gacq_null.hip) against the definition of tests/nulling_oracle.py.  The window sums of the covariances
and the output bytes are equalities of integers and bytes; the quantised weights are equal wherever no scaled weight lies within 1e-6
of a rounding tie, which nulling_cases.check_margins() asserts of every case here on the CPU.  Device against device and against the
oracle however the recording is cut into calls and wherever the inputs lie; the refusals of gacq_null_run_dev; then four jammed
antennas whose nulled output the 20 ms search finds the satellite in, and the command line."""
import ctypes
import io

import numpy as np
import pytest

import nulling_cases as C
import nulling_oracle as O
from gnss_dsp_tools_amd import _native as nat
from gnss_dsp_tools_amd import cancel, nulling, signals, simulate

BAD_ARG, SHORT_INPUT = -1, -6


def _dev(engine, x, off=0):
    """the int8 array on the device, its first byte `off` bytes past a 256-byte boundary"""
    torch = nat.require_torch()
    x = np.ascontiguousarray(x).view(np.int8).reshape(-1)
    buf = torch.empty(len(x) + 512, dtype=torch.int8, device="cuda:%d" % engine.device)
    off += (-buf.data_ptr()) % 256
    v = buf[off:off + len(x)]
    v.copy_(torch.from_numpy(x))
    return v


def _inputs(engine, name, offs=None):
    xs = C.data(name)
    ds = [_dev(engine, x, 0 if offs is None else offs[p % len(offs)]) for p, x in enumerate(xs)]
    if C.CASES[name][4] == "shared":
        ds[2] = ds[0]                               # two antennas on one tensor
    return ds


def _nuller(engine, name):
    M, Lb, W = C.CASES[name][:3]
    return nulling.Nuller(engine, M, Lb, W, 10, C.constraint(name))


@pytest.fixture(scope="module", autouse=True)
def margins():
    return C.check_margins()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(C.CASES))
def test_covariances_weights_and_bytes_equal_the_oracle(engine, name):
    """tests 1 and 2 of every case, and the int8 bytes with them: the recordings are asymmetric between antennas and between I and Q, so
    a row/column swap, an I/Q swap or a sign error in Im C changes the integers"""
    M, Lb, W = C.CASES[name][:3]
    want = C.reference(name)
    N = len(C.data(name)[0]) // 2
    with _nuller(engine, name) as nl:
        out, wq, cov = nl.run(_inputs(engine, name), 0, 0, N, 1.0, "int8", weights=True, cov=True)
        st = nl.stats()
    cov, wq = cov.cpu().numpy(), wq.cpu().numpy()
    assert cov.shape == want["cov"].shape == (-(-N // Lb), M, M, 2) and np.array_equal(cov, want["cov"]), name
    assert np.all(cov[:, np.arange(M), np.arange(M), 1] == 0)
    if C.CASES[name][4] == "min":
        assert cov[0, 0, 0, 0] == 2 * W * Lb * 16384 and np.all(cov[..., 0] == cov[0, 0, 0, 0])      # |G| = Lb 2^14, the largest
    else:
        assert np.any(cov[0, 0, 1] != cov[0, 1, 0]) and np.any(cov[..., 1] != 0)
    assert wq.dtype == np.int32 and np.array_equal(wq, want["wq"]), (name, np.argwhere(wq != want["wq"])[:4])
    assert np.array_equal(out.cpu().numpy(), want["out"]) and st == (want["clipped"], want["owned"]), (name, st)


@pytest.mark.gpu
@pytest.mark.parametrize("name", C.OUTPUT_CASES)
@pytest.mark.parametrize("dtype,gain", [("int8", 0.75), ("int8", 6.5), ("complex64", 0.75)])
def test_output_bytes_at_odd_input_addresses(engine, name, dtype, gain):
    """test 3: every antenna's first byte at another odd offset; a gain that clips many components"""
    N = len(C.data(name)[0]) // 2
    want = C.reference(name, dtype == "complex64", gain)
    with _nuller(engine, name) as nl:
        out = nl.run(_inputs(engine, name, (1, 3, 5, 7, 9, 11, 13, 15)), 0, 0, N, gain, dtype)
        st = nl.stats()
    assert out.cpu().numpy().tobytes() == want["out"].tobytes() and st == (want["clipped"], want["owned"]), (name, st)
    # the cases are worth their gains: 6.5 clips (but for the shared antenna, which the weights cancel to nothing), 0.75 does not
    assert want["owned"] == -(-N // C.CASES[name][1])
    assert want["clipped"] > 50 or name.startswith("shared") if (dtype == "int8" and gain > 1.0) else want["clipped"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["long-m3-b128-w3", "long-m8-b4096-w1", "long-m2-b192-w2"])
@pytest.mark.parametrize("dtype", ["int8", "complex64"])
def test_cuts_do_not_matter(engine, name, dtype):
    """test 4: calls that end and start on a workgroup tile, on a block edge, one lane's run before and after each, at odd places, with
    a trailing partial block; every call is given only the input it needs, at an odd address"""
    M, Lb, W = C.CASES[name][:3]
    xs = C.data(name)
    N = len(xs[0]) // 2
    assert nat.lib.gacq_null_tile(ctypes.addressof(nulling.make_cfg(M, Lb, W))) == C.TILE and N > C.TILE + C.RUN and N % Lb
    want = C.reference(name, dtype == "complex64", 2.5)
    per = 1 if dtype == "complex64" else 2
    with _nuller(engine, name) as nl:
        whole, wq_whole = nl.run(_inputs(engine, name), 0, 0, N, 2.5, dtype, weights=True)
        st_whole = nl.stats()
    assert whole.cpu().numpy().tobytes() == want["out"].tobytes() and st_whole == (want["clipped"], want["owned"])
    pts = [0] + C.cuts(Lb, W, N) + [N]
    assert C.TILE in pts and C.TILE - C.RUN in pts and (W + 1) * Lb + C.RUN in pts
    with _nuller(engine, name) as nl:
        for a, b in zip(pts, pts[1:]):
            lo, hi = O.needed(Lb, W, a, b - a)
            ds = [_dev(engine, x[2 * lo:2 * hi], 2 * p + 1) for p, x in enumerate(xs)]
            out, wq = nl.run(ds, lo, a, b - a, 2.5, dtype, weights=True)
            assert bool((out == whole[per * a:per * b]).all()), (name, a, b)
            blk = -(-a // Lb)
            assert bool((wq == wq_whole[blk:blk + wq.shape[0]]).all()) and wq.shape[0] == -(-b // Lb) - blk, (name, a, b)
        assert nl.stats() == st_whole


@pytest.mark.gpu
def test_warm_up_blocks_share_one_weight_vector(engine):
    """test 5: loud in the first W blocks, quiet afterwards: blocks 0 .. W are weighted by the first W blocks' covariance, block W + 1 is
    the first whose window has moved"""
    name = "loud-m4-b256-w3"
    M, Lb, W = C.CASES[name][:3]
    N = len(C.data(name)[0]) // 2
    with _nuller(engine, name) as nl:
        out, wq, cov = nl.run(_inputs(engine, name), 0, 0, N, 1.0, "int8", weights=True, cov=True)
    wq, cov = wq.cpu().numpy(), cov.cpu().numpy()
    assert all(np.array_equal(wq[b], wq[0]) and np.array_equal(cov[b], cov[0]) for b in range(W + 1))
    assert not np.array_equal(wq[W + 1], wq[0]) and cov[W + 1, 0, 0, 0] < cov[0, 0, 0, 0]
    assert np.array_equal(wq, C.reference(name)["wq"])
    assert cov[2 * W, 0, 0, 0] * 8 < cov[0, 0, 0, 0]                                   # the quiet part, a window later


@pytest.mark.gpu
def test_refusals_of_run_dev_leave_the_outputs_untouched(engine):
    """test 6: every refusal through the raw ABI; out, stats, weights and cov keep their bytes"""
    torch = nat.require_torch()
    name = "m3-b128-w1"
    M, Lb, W = C.CASES[name][:3]
    N = len(C.data(name)[0]) // 2
    ds = _inputs(engine, name)
    dev = ds[0].device
    out = torch.full((8 * N + 8,), 77, dtype=torch.uint8, device=dev)
    stats = torch.full((3,), 77, dtype=torch.int64, device=dev)
    wq = torch.full((2 * M * 8 + 1,), 77, dtype=torch.int32, device=dev)
    cov = torch.full((2 * M * M * 8 + 1,), 77, dtype=torch.int64, device=dev)
    ptrs = (ctypes.c_void_p * M)(*[d.data_ptr() for d in ds])
    holed = (ctypes.c_void_p * M)(ds[0].data_ptr(), None, ds[2].data_ptr())
    good = dict(h=None, d_in=ctypes.cast(ptrs, ctypes.c_void_p), in_first=0, in_count=N, out_first=0, n_out=N, gain=1.0, cplx=0, out=out.data_ptr(),
                stats=stats.data_ptr(), wq=wq.data_ptr(), cov=cov.data_ptr())

    def call(**kw):
        a = dict(good, **kw)
        return nat.lib.gacq_null_run_dev(a["h"], a["d_in"], a["in_first"], a["in_count"], a["out_first"], a["n_out"], a["gain"], a["cplx"],
                                         ctypes.c_void_p(a["out"]), ctypes.c_void_p(a["stats"]), ctypes.c_void_p(a["wq"]), ctypes.c_void_p(a["cov"]))

    engine.use_torch_stream(dev)
    assert call() == BAD_ARG                                                          # no handle
    with _nuller(engine, name) as nl:
        good["h"] = nl._h
        big = (1 << 48) + 1
        for kw in (dict(d_in=None), dict(d_in=ctypes.cast(holed, ctypes.c_void_p)), dict(out=None), dict(cplx=1, out=out.data_ptr() + 4),
                   dict(stats=stats.data_ptr() + 4), dict(wq=wq.data_ptr() + 2), dict(cov=cov.data_ptr() + 4), dict(gain=0.0), dict(gain=float("nan")),
                   dict(gain=float("inf")), dict(gain=1e-50), dict(in_first=-1), dict(in_count=-1), dict(out_first=-1), dict(n_out=-1), dict(n_out=big),
                   dict(in_first=big), dict(in_count=big), dict(out_first=big)):
            assert call(**kw) == BAD_ARG, kw
        for kw in (dict(in_count=N - 1), dict(in_count=W * Lb - 1, n_out=1), dict(in_first=1), dict(out_first=3 * Lb, n_out=10, in_first=2 * Lb + 1),
                   dict(n_out=N + 1)):
            assert call(**kw) == SHORT_INPUT, kw
        assert "need input samples" in nat.lib.gacq_last_error(engine._ctx).decode()
        assert call(n_out=0) == 0 and call(n_out=0, in_count=0) == 0                  # nothing to do
        torch.cuda.synchronize()
        for t in (out, stats, wq, cov):
            assert bool((t == 77).all())
        assert call() == 0                                                            # the unchanged call is accepted and writes
        torch.cuda.synchronize()
    want = C.reference(name)
    assert out[:2 * N].cpu().numpy().view(np.int8).tobytes() == want["out"].tobytes() and bool((out[2 * N:] == 77).all())
    assert stats.cpu().tolist() == [77 + want["clipped"], 77 + want["owned"], 77]
    nb = want["owned"]
    assert np.array_equal(wq[:2 * M * nb].cpu().numpy().reshape(nb, M, 2), want["wq"]) and bool((wq[2 * M * nb:] == 77).all())
    assert np.array_equal(cov[:2 * M * M * nb].cpu().numpy().reshape(nb, M, M, 2), want["cov"]) and bool((cov[2 * M * M * nb:] == 77).all())
    # the configuration is checked when the handle is opened
    h = ctypes.c_void_p()
    for bad in (dict(M=1), dict(block=100), dict(window=65), dict(load_shift=41), dict(constraint=[0, 0, 0])):
        d = dict(M=3, block=128, window=1, load_shift=10, constraint=None)
        d.update(bad)
        cfg = nulling.make_cfg(d["M"], d["block"], d["window"], d["load_shift"], d["constraint"])
        assert nat.lib.gacq_null_open(engine._ctx, ctypes.addressof(cfg), ctypes.byref(h)) == BAD_ARG and not h.value, bad


def _code_error(got, want, L=1023.0):
    return abs((got - want + L / 2.0) % L - L / 2.0)


def _scene(engine, E=C.E2E):
    """the four antennas of nulling_cases.E2E as int8 CUDA tensors, built on the device from complex64 recordings"""
    torch = nat.require_torch()
    fs, W, Lb = E["fs"], E["window"], E["block"]
    w0 = (W + 1) * Lb
    n = w0 + int(fs * 0.001 * (E["ms"] + 5)) + 8
    quiet = simulate.Satellite(E["signal"], E["prn"], 0.0, 0.0, 0.0)
    jam = simulate.recording([quiet], fs, 0.0, n, E["jam_seed"], E["jam"], dtype="complex64", engine=engine)
    xs = []
    for p in range(4):
        sat = simulate.Satellite(E["signal"], E["prn"], E["amp"], E["doppler"], E["code_phase"], carrier_phase=E["sat_phase"][p])
        v = simulate.recording([sat], fs, 0.0, n, E["noise_seeds"][p], E["sigma"], dtype="complex64", engine=engine)
        ph = np.exp(2j * np.pi * E["jam_phase"][p])
        v = v + jam * complex(ph)
        xs.append(torch.view_as_real(v).round().clamp(-127, 127).to(torch.int8).reshape(-1).contiguous())
    return xs, w0, n, sat


@pytest.mark.gpu
def test_end_to_end_the_satellite_is_found_on_the_nulled_output(engine):
    """test 7: a broadband jammer at 42 per component hides PRN 17 at amplitude 1 under noise of sigma 6 (nulling_cases.E2E has the CPU
    experiment that fixed the level): on antenna 0 the 20 ms search puts it into a wrong cell, on the nulled output into the true one"""
    E = C.E2E
    fs, Lb, W = E["fs"], E["block"], E["window"]
    xs, w0, n, sat = _scene(engine)
    out, st, wq = nulling.convert(engine, xs, Lb, W, gain=1.0, weights=True)                  # gain 1: the reference antenna's own scale
    assert out.numel() == 2 * n and st[1] == -(-n // Lb)
    wq = wq.cpu().numpy()
    assert np.all(wq[:, 0, 0] == 16384) and np.all(wq[:, 0, 1] == 0)
    x0, y = xs[0].cpu().numpy(), out.cpu().numpy()
    sig = signals.get(E["signal"])
    before = cancel.reacquire(engine, sig, x0, fs, 0.0, w0, [E["prn"]], E["doppler_search"], E["ms"])[0][1]
    after = cancel.reacquire(engine, sig, y, fs, 0.0, w0, [E["prn"]], E["doppler_search"], E["ms"])[0][1]
    true_code = (E["code_phase"] + w0 * sat.code_rate_hz() / fs) % 1023.0
    true_bin = 200.0 * round(E["doppler"] / 200.0)
    one_sample = 1.023e6 / fs
    pin, pout = float(np.mean(x0[2 * w0:].astype(np.float64) ** 2)), float(np.mean(y[2 * w0:].astype(np.float64) ** 2))
    print("true cell: code %.2f doppler %.0f" % (true_code, true_bin))
    print("antenna 0: metric %.2f code %.2f doppler %.0f power %.1f   nulled: metric %.2f code %.2f doppler %.0f power %.1f clipped %d"
          % (tuple(before) + (pin,) + tuple(after) + (pout, st[0])))
    m, code, dop = after
    assert dop == true_bin and _code_error(code, true_code) <= one_sample
    m0, code0, dop0 = before
    assert not (dop0 == true_bin and _code_error(code0, true_code) <= one_sample)     # the miss on the jammed antenna
    assert pout < 0.5 * pin and m > m0


@pytest.mark.gpu
def test_command_line_four_files_in_one_out(engine, tmp_path):
    """test 8: the bytes of convert() at a small piece size and at the default, the printed line, the weights trace; the automatic
    gain does not depend on the piece size either"""
    name = "long-m3-b128-w3"
    M, Lb, W = C.CASES[name][:3]
    xs = list(C.data(name)) + [C.data("long-m2-b192-w2")[1][:2 * (C.TILE + 400)]]             # a fourth, shorter file: the output ends with it
    N = C.TILE + 400
    paths = []
    for p, x in enumerate(xs):
        paths.append(str(tmp_path / ("ant%d.iq" % p)))
        x.tofile(paths[-1])
    cut = [x[:2 * N] for x in xs]
    want, st, wq = nulling.convert(engine, cut, Lb, W, gain=1.75, weights=True)
    want, wq = want.cpu().numpy().tobytes(), wq.cpu().numpy().tobytes()
    assert len(want) == 2 * N and st[0] > 0
    args = ["--block", str(Lb), "--window", str(W), "--weights-trace", str(tmp_path / "w.bin"), "--out", str(tmp_path / "out.iq")]
    for piece in (1000, None):
        text = io.StringIO()
        line = nulling.run(args + ["--gain", "1.75"] + paths, out=text, **({} if piece is None else dict(piece_bytes=piece)))
        assert line == text.getvalue().strip() == "antennas 4 block %d window %d gain 1.75 clipped %d samples %d" % (Lb, W, st[0], N)
        assert open(str(tmp_path / "out.iq"), "rb").read() == want and open(str(tmp_path / "w.bin"), "rb").read() == wq
    # the automatic gain: target rms over the rms of the first 65536 (here: all) outputs at gain 1
    unit = nulling.convert(engine, cut, Lb, W, gain=1.0, dtype="complex64")[0].cpu().numpy()
    g = 32.0 / float(np.sqrt(np.mean(np.abs(unit.astype(np.complex128)) ** 2)))
    lines = [nulling.run(args + paths, out=io.StringIO(), **kw) for kw in (dict(piece_bytes=3000), dict())]
    assert lines[0] == lines[1] and abs(float(lines[0].split()[7]) / g - 1.0) < 1e-6, (lines, g)
    auto = nulling.convert(engine, cut, Lb, W, gain=float(lines[0].split()[7]))[0].cpu().numpy().tobytes()
    assert open(str(tmp_path / "out.iq"), "rb").read() == auto != want
    # complex64 output to a file
    nulling.run(args + ["--gain", "1.75", "--complex64"] + paths, out=io.StringIO(), piece_bytes=5000)
    assert open(str(tmp_path / "out.iq"), "rb").read() == nulling.convert(engine, cut, Lb, W, gain=1.75, dtype="complex64")[0].cpu().numpy().tobytes()
