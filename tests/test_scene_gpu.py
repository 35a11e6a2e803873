"""GPU: the scene kernel (csrc/gacq_scene.hip) against the fp64 oracle of tests/scene_oracle.py, the int8 form against the device's own
complex64 form, independence of how a recording is cut into calls and into groups of antennas, the point-source property of the noise
jammer, the argument checks through the raw ABI, the two pipelines of tests/scene_cases.py and the command line.

Bound of the complex64 output, per case: four times the deviation of the numpy float32 evaluation of the same formula
(scene_oracle.evaluate(f32=True)) from the fp64 one, relative to max |v|; both figures and the device's are printed before the
assertion (DESIGN 5.28 has the table)."""
import ctypes
import io

import numpy as np
import pytest

import nulling_cases as NC
import scene_cases as C
import scene_oracle as O
from gnss_dsp_tools_amd import _native as nat
from gnss_dsp_tools_amd import cancel, mitigate, nulling, scene, signals, simulate
from test_scene_cpu import bad_calls, raw_call


def _run(engine, case, dtype, **kw):
    c = dict(case)
    c.update(kw)
    return scene.recording(c["sats"], c["emitters"], c["gains"], c["fs"], c["coffset"], c["n"], c.get("seed", C.SEED), c["sigma"], c["j0"], dtype,
                           c["first_antenna"], engine)


def _bound(name):
    want, f32 = C.reference(name)
    scale = float(np.max(np.abs(want)))
    return want, scale, float(np.max(np.abs(f32 - want))) / scale


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(C.CASES))
def test_complex64_matches_the_fp64_oracle(engine, name):
    case = C.CASES[name]
    want, scale, dev32 = _bound(name)
    got = _run(engine, case, "complex64").cpu().numpy()
    assert got.shape == want.shape == (len(case["gains"]), case["n"]) and got.dtype == np.complex64
    err = float(np.max(np.abs(got - want))) / scale
    print("%-24s M %d K %d I %d  numpy float32 deviation %.3g  bound %.3g  device %.3g"
          % (name, len(case["gains"]), len(case["sats"]), len(case["emitters"]), dev32, 4 * dev32, err))
    assert err <= 4 * dev32


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(C.CASES) + ["amp 200"])
def test_int8_is_the_rounded_complex64_of_the_device(engine, name):
    torch = nat.require_torch()
    case = C.CLIP_CASE if name == "amp 200" else C.CASES[name]
    M, n = len(case["gains"]), case["n"]
    v = _run(engine, case, "complex64").cpu().numpy()
    got = _run(engine, case, "int8").cpu().numpy()
    assert got.dtype == np.int8 and got.shape == (M, 2 * n)
    want = np.stack([O.to_int8(row) for row in v])
    assert np.array_equal(got, want)
    if name == "amp 200":
        assert got.max() == 127 and got.min() == -127
    # rows at odd addresses, through the raw ABI: the same bytes, and nothing around them
    buf = torch.full((M, 2 * n + 6), 77, dtype=torch.int8, device=got_device(engine))
    pairs = [s.struct(case["coffset"]) for s in case["sats"]]
    K, I = len(pairs), len(case["emitters"])
    sarr = (simulate.SimSat * max(K, 1))(*[p[0] for p in pairs])
    earr = (scene.SceneEmitter * max(I, 1))(*[e.struct() for e in case["emitters"]])
    g = np.ascontiguousarray(case["gains"], dtype=np.complex128)
    ptrs = (ctypes.c_void_p * M)(*[buf[p].data_ptr() + 3 for p in range(M)])
    engine.use_torch_stream()
    nat.check(nat.lib.gacq_scene_dev(engine._ctx, ctypes.addressof(sarr) if K else None, K, ctypes.addressof(earr) if I else None, I, g.ctypes.data,
                                     case["fs"], case["sigma"], C.SEED, case["first_antenna"], M, case["j0"], n, 0, ctypes.cast(ptrs, ctypes.c_void_p)),
              engine._ctx)
    h = buf.cpu().numpy()
    assert np.array_equal(h[:, 3:3 + 2 * n], want) and (h[:, :3] == 77).all() and (h[:, 3 + 2 * n:] == 77).all()


def got_device(engine):
    return "cuda:%d" % engine.device


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["int8", "complex64"])
def test_cutting_the_recording_into_calls_does_not_matter(engine, dtype):
    torch = nat.require_torch()
    whole = _run(engine, C.CUT_CASE, dtype, n=C.CUT_N)
    parts, j = [], C.CUT_CASE["j0"]
    for n in C.CUT_PIECES:
        parts.append(_run(engine, C.CUT_CASE, dtype, n=n, j0=j))
        j += n
    assert sum(C.CUT_PIECES) == C.CUT_N and C.CUT_CASE["j0"] < 2 ** 33 < j and whole.shape[0] == 3
    assert whole.cpu().numpy().tobytes() == torch.cat(parts, dim=1).cpu().numpy().tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["int8", "complex64"])
def test_antennas_in_one_call_or_one_by_one(engine, dtype):
    """antennas 0..2 in one call (runs of 4 samples) against three one-antenna calls (runs of 8) with the matching gain rows; and the
    eight-antenna kernel (runs of 2) against the first three of its rows"""
    torch = nat.require_torch()
    case = dict(C.CUT_CASE, n=C.N, gains=C.full_gains(8, 5))
    eight = _run(engine, case, dtype)
    three = _run(engine, case, dtype, gains=case["gains"][:3])
    ones = [_run(engine, case, dtype, gains=case["gains"][p:p + 1], first_antenna=p) for p in range(3)]
    assert three.cpu().numpy().tobytes() == torch.cat(ones, dim=0).cpu().numpy().tobytes() == eight[:3].contiguous().cpu().numpy().tobytes()
    tail = _run(engine, case, dtype, gains=case["gains"][3:], first_antenna=3)                 # five antennas: 3..7
    assert tail.cpu().numpy().tobytes() == eight[3:].contiguous().cpu().numpy().tobytes()


@pytest.mark.gpu
def test_seed_and_sigma_decide_the_noise(engine):
    torch = nat.require_torch()
    case = C.CASES["K=2 I=3 M=3"]
    a = _run(engine, case, "int8")
    assert torch.equal(a, _run(engine, case, "int8")) and not torch.equal(a, _run(engine, case, "int8", seed=C.SEED + 1))
    # sigma 0 removes exactly the antenna noise: without a noise jammer the seed no longer matters, and without any source nothing is left
    quiet = dict(case, emitters=case["emitters"][:2], gains=case["gains"][:, :4], sigma=0.0)
    v = _run(engine, quiet, "complex64")
    assert torch.equal(v, _run(engine, quiet, "complex64", seed=C.SEED + 1)) and bool((v != 0).any())
    assert not torch.equal(_run(engine, dict(quiet, sigma=12.0), "complex64"), _run(engine, dict(quiet, sigma=12.0), "complex64", seed=C.SEED + 1))
    none = dict(case, sats=[], emitters=[], gains=np.zeros((3, 0)), sigma=0.0)
    assert bool((_run(engine, none, "complex64") == 0).all())
    # ... and the noise that sigma adds is the same draw whatever the sources: v(sigma) - v(0) against the noise-only recording
    noise = _run(engine, dict(none, sigma=12.0), "complex64").cpu().numpy()
    diff = (_run(engine, dict(quiet, sigma=12.0), "complex64") - v).cpu().numpy()
    assert np.max(np.abs(diff - noise)) <= 1e-5 * np.max(np.abs(v.cpu().numpy()))              # fp32 sums in another order
    got, cap = O.noise_statistics(noise[2].real, noise[2].imag, 12.0)
    for k in got:
        assert got[k] <= cap[k], (k, got[k], cap[k])


@pytest.mark.gpu
def test_a_noise_jammer_is_a_point_source_and_antenna_noise_is_not(engine):
    g = np.array([[0.8 - 0.3j], [-0.2 + 1.1j]])
    case = dict(C.CASES["jammer alone"], gains=g)
    v = _run(engine, case, "complex64").cpu().numpy().astype(np.complex128)
    ratio = np.complex64(g[1, 0]).astype(np.complex128) / np.complex64(g[0, 0]).astype(np.complex128)
    _, _, dev32 = _bound("jammer alone")
    err = float(np.max(np.abs(v[1] - ratio * v[0])) / np.max(np.abs(v)))
    print("row 1 against g1 / g0 times row 0: %.3g, bound %.3g" % (err, 4 * dev32))
    assert err <= 4 * dev32
    n = 1 << 16
    x = _run(engine, dict(case, emitters=[], gains=np.zeros((2, 0)), sigma=12.0, n=n), "complex64").cpu().numpy().astype(np.complex128)
    rho = abs(np.vdot(x[0], x[1])) / (np.linalg.norm(x[0]) * np.linalg.norm(x[1]))
    print("correlation of the noise of antennas 0 and 1: %.3g, bound %.3g" % (rho, 5 / np.sqrt(n)))
    assert rho < 5 / np.sqrt(n)


@pytest.mark.gpu
def test_every_argument_check_through_the_raw_abi(engine):
    torch = nat.require_torch()
    engine.use_torch_stream()
    out = torch.full((2, 4096), 77, dtype=torch.int8, device=got_device(engine))
    rows = [out[0].data_ptr(), out[1].data_ptr()]
    for label, code, change in bad_calls() + [("unknown PRN", -3, dict(sat=dict(prn=999)))]:
        rc = raw_call(engine._ctx, rows, **change)
        assert rc == code, (label, rc, nat.lib.gacq_last_error(engine._ctx))
        assert nat.lib.gacq_last_error(engine._ctx), label
    # complex64 rows at an address that is not 8-byte aligned
    assert raw_call(engine._ctx, [rows[0], rows[1] + 4], cplx=1) == -1
    torch.cuda.synchronize()
    assert bool((out == 77).all())
    assert raw_call(engine._ctx, rows) == 0                                          # the unchanged call is accepted and writes 200 bytes a row
    torch.cuda.synchronize()
    h = out.cpu().numpy()
    assert (h[:, 200:] == 77).all() and not (h[0, :200] == 77).all() and not (h[1, :200] == 77).all()


def _code_error(got, want, L=1023.0):
    return abs((got - want + L / 2.0) % L - L / 2.0)


def _found(result, true_code, doppler, fs):
    m, code, dop = result
    return dop == 200.0 * round(doppler / 200.0) and _code_error(code, true_code) <= 1.023e6 / fs


@pytest.mark.gpu
def test_pipeline_array_the_satellite_is_found_on_the_nulled_output(engine):
    """scene_cases.array_scene (the table there has the oracle chain): a noise jammer of sigma 42 hides PRN 17 on antenna 0; on the
    nulled output of the four rows the 20 ms search finds the true cell"""
    E = NC.E2E
    fs, Lb, W = E["fs"], E["block"], E["window"]
    w0 = (W + 1) * Lb
    n = w0 + int(fs * 0.001 * (E["ms"] + 5)) + 8
    sats, emitters, gains = C.array_scene()
    x = scene.recording(sats, emitters, gains, fs, 0.0, n, C.ARRAY_SEED, E["sigma"], engine=engine)
    out, st = nulling.convert(engine, [x[p] for p in range(4)], Lb, W, gain=1.0)
    x0, y = x[0].cpu().numpy(), out.cpu().numpy()
    sig = signals.get(E["signal"])
    before = cancel.reacquire(engine, sig, x0, fs, 0.0, w0, [E["prn"]], E["doppler_search"], E["ms"])[0][1]
    after = cancel.reacquire(engine, sig, y, fs, 0.0, w0, [E["prn"]], E["doppler_search"], E["ms"])[0][1]
    true_code = (E["code_phase"] + w0 * sats[0].code_rate_hz() / fs) % 1023.0
    pin, pout = float(np.mean(x0[2 * w0:].astype(np.float64) ** 2)), float(np.mean(y[2 * w0:].astype(np.float64) ** 2))
    print("true cell: code %.2f doppler 1200" % true_code)
    print("antenna 0: metric %.2f code %.2f doppler %.0f power %.1f   nulled: metric %.2f code %.2f doppler %.0f power %.1f clipped %d"
          % (tuple(before) + (pin,) + tuple(after) + (pout, st[0])))
    assert _found(after, true_code, E["doppler"], fs)
    assert not _found(before, true_code, E["doppler"], fs)                          # the miss on the jammed antenna
    assert pout < 0.5 * pin and after[0] > before[0]


@pytest.mark.gpu
def test_pipeline_swept_jammer_needs_short_excision_frames(engine):
    """scene_cases.swept_scene (the table there has the oracle chain): a chirp across 0.7 fs every 205 samples; the 20 ms search finds
    PRN 17 after excision with 64-sample frames, not on the raw recording and not after excision with 1024-sample frames"""
    s = C.SWEPT
    fs = s["fs"]
    n = int(fs * 0.001 * (s["ms"] + 5)) + 4096
    sats, emitters, gains = C.swept_scene()
    raw = scene.recording(sats, emitters, gains, fs, 0.0, n, s["seed"], s["sigma"], engine=engine)[0]
    sig = signals.get(s["signal"])
    got = {}
    for name, nfft in (("raw", 0), ("nfft=1024", 1024), ("nfft=64", 64)):
        y = raw
        if nfft:
            cfg = mitigate.Config(nfft=nfft)
            y = mitigate.apply(engine, cfg, raw, mitigate.auto_gain(engine, cfg, raw))
        got[name] = cancel.reacquire(engine, sig, y.cpu().numpy(), fs, 0.0, 0, [s["prn"]], s["doppler_search"], s["ms"])[0][1]
        print("%-10s metric %.2f code %.2f doppler %.0f" % ((name,) + tuple(got[name])))
    assert _found(got["nfft=64"], s["code_phase"], s["doppler"], fs)
    assert not _found(got["raw"], s["code_phase"], s["doppler"], fs) and not _found(got["nfft=1024"], s["code_phase"], s["doppler"], fs)


@pytest.mark.gpu
def test_command_line_writes_the_files_nulling_takes(tmp_path, engine):
    paths = [str(tmp_path / "a0.iq"), str(tmp_path / "a1.iq")]
    argv = ["--fs", "4.092e6", "--coffset", "0", "--seconds", "0.02", "--seed", "31", "--sigma", "6", "--element", "0,0,0", "--element", "0.5,0,0",
            "--sat", "gps-l1,17,1.0,1250.0,333.25@20,50", "--jammer", "42@90,10", "--tone", "9,-801234.5@200,5", "--gate", "700,1500,20"] + paths
    out = io.StringIO()
    lines = scene.run(argv, out, piece_bytes=1 << 16)                              # three pieces
    assert out.getvalue().splitlines() == lines == ["gps-l1 %s 4092000.0 0.0 17 1250.0 333.25" % paths[0]]
    a, sats, emitters, elements, gains = scene.parse(argv)
    n = int(4.092e6 * 0.02)
    whole = scene.recording(sats, emitters, gains, a.fs, a.coffset, n, 31, a.sigma, engine=engine).cpu().numpy()
    for p in range(2):
        assert np.fromfile(paths[p], dtype=np.int8).tobytes() == whole[p].tobytes()            # the files do not depend on the piece size
    line = nulling.run(["--block", "4096", "--window", "8", "--gain", "1.0", "--out", str(tmp_path / "y.iq")] + paths, out=io.StringIO())
    assert line.startswith("antennas 2 block 4096 window 8 gain 1.0 clipped ") and line.endswith("samples %d" % n)
    assert np.fromfile(str(tmp_path / "y.iq"), dtype=np.int8).size == 2 * n
