"""GPU: the recording-synthesis kernel (csrc/gacq_simulate.hip) against the fp64 oracle of tests/simulate_oracle.py, the int8 form
against the device's own complex64 form, independence of how a recording is cut into calls, the noise, the argument checks through
the raw ABI, and scene -> acquire -> hand off -> track on the device's own recording.

Bound of the complex64 output, per case: four times the deviation of the numpy float32 evaluation of the same formula
(simulate_oracle.evaluate(f32=True)) from the fp64 one, relative to max |v|; both figures and the device's are printed before the
assertion (DESIGN 5.17 has the table)."""
import io

import numpy as np
import pytest

import simulate_cases as C
import simulate_oracle as O
from gnss_dsp_tools_amd import _native as nat
from gnss_dsp_tools_amd import codes, handoff, simulate, track, trackloop
from test_simulate_cpu import bad_calls, raw_call


def _run(engine, case, dtype, **kw):
    c = dict(case)
    c.update(kw)
    return simulate.recording(c["sats"], c["fs"], c["coffset"], c["n"], c.get("seed", C.SEED), c["sigma"], c["j0"], dtype, engine)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(C.CASES))
def test_complex64_matches_the_fp64_oracle(engine, name):
    case = C.CASES[name]
    want, f32 = C.reference(name)
    got = _run(engine, case, "complex64").cpu().numpy()
    assert got.shape == want.shape == (case["n"],) and got.dtype == np.complex64
    scale = float(np.max(np.abs(want)))
    dev32 = float(np.max(np.abs(f32 - want))) / scale
    err = float(np.max(np.abs(got - want))) / scale
    print("%-28s K %d  numpy float32 deviation %.3g  bound %.3g  device %.3g" % (name, len(case["sats"]), dev32, 4 * dev32, err))
    assert err <= 4 * dev32


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(C.CASES) + ["amp 200"])
def test_int8_is_the_rounded_complex64_of_the_device(engine, name):
    case = C.CLIP_CASE if name == "amp 200" else C.CASES[name]
    v = _run(engine, case, "complex64").cpu().numpy()
    got = _run(engine, case, "int8").cpu().numpy()
    assert got.dtype == np.int8 and got.shape == (2 * case["n"],)
    assert np.array_equal(got, O.to_int8(v))
    if name == "amp 200":
        assert got.max() == 127 and got.min() == -127


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["int8", "complex64"])
def test_cutting_the_recording_into_calls_does_not_matter(engine, dtype):
    torch = nat.require_torch()
    whole = _run(engine, C.CUT_CASE, dtype, n=C.CUT_N)
    parts, j = [], C.CUT_CASE["j0"]
    for n in C.CUT_PIECES:
        parts.append(_run(engine, C.CUT_CASE, dtype, n=n, j0=j))
        j += n
    assert sum(C.CUT_PIECES) == C.CUT_N and C.CUT_CASE["j0"] < 2 ** 33 < j
    a, b = whole.cpu().numpy(), torch.cat(parts).cpu().numpy()
    assert a.tobytes() == b.tobytes()
    # ... and a piece written into the middle of a caller's buffer (an address that is not 16-byte aligned) is the same piece
    buf = torch.zeros(whole.numel() + 6, dtype=whole.dtype, device=whole.device)
    n0 = C.CUT_PIECES[0]
    per = 2 if dtype == "int8" else 1
    simulate.recording(C.CUT_CASE["sats"], C.CUT_CASE["fs"], C.CUT_CASE["coffset"], n0, C.SEED, C.CUT_CASE["sigma"], C.CUT_CASE["j0"], dtype, engine,
                       out=buf[3:3 + per * n0])
    assert buf[3:3 + per * n0].cpu().numpy().tobytes() == parts[0].cpu().numpy().tobytes()
    assert not buf[:3].cpu().numpy().any() and not buf[3 + per * n0:].cpu().numpy().any()


@pytest.mark.gpu
def test_seed_and_sigma_decide_the_noise(engine):
    torch = nat.require_torch()
    quiet = [simulate.Satellite("gps-l1", 7, 0.0, 0.0, 0.0)]                        # noise only
    base = dict(sats=quiet, fs=6.0e6, coffset=0.0, n=C.NOISE_N, sigma=12.0, j0=0)
    for seed in C.NOISE_SEEDS:
        v = _run(engine, base, "complex64", seed=seed)
        assert torch.equal(v.view(torch.int64), _run(engine, base, "complex64", seed=seed).view(torch.int64))
        x = _run(engine, base, "int8", seed=seed)
        assert torch.equal(x, _run(engine, base, "int8", seed=seed))
        assert not torch.equal(x, _run(engine, base, "int8", seed=seed + 1))
        assert not torch.equal(x, _run(engine, base, "int8", seed=seed, sigma=12.5))
        h = v.cpu().numpy()
        got, cap = O.noise_statistics(h.real, h.imag, 12.0)
        print(seed, got, cap)
        for k in got:
            assert got[k] <= cap[k], (seed, k, got[k], cap[k])


@pytest.mark.gpu
def test_every_argument_check_through_the_raw_abi(engine):
    torch = nat.require_torch()
    engine.use_torch_stream()
    out = torch.full((4096,), 77, dtype=torch.int8, device="cuda:%d" % engine.device)
    for label, code, change in bad_calls():
        rc = raw_call(engine._ctx, out.data_ptr(), **change)
        assert rc == code, (label, rc, nat.lib.gacq_last_error(engine._ctx))
    # complex64 output at an address that is not 8-byte aligned
    assert raw_call(engine._ctx, out.data_ptr() + 4, cplx=1) == -1
    torch.cuda.synchronize()
    assert bool((out == 77).all())
    assert raw_call(engine._ctx, out.data_ptr()) == 0                                # the unchanged call is accepted and writes 200 bytes
    torch.cuda.synchronize()
    h = out.cpu().numpy()
    assert (h[200:] == 77).all() and not (h[:200] == 77).all()


MS = 250
DWELLS = (20, 20)


def _code_error(got, want, L):
    return abs((got - want + L / 2.0) % L - L / 2.0)


def _pipeline(name, fs, coffset, sats, noise_item, engine, doppler_search=None):
    """test_handoff_gpu._check_channels on a recording generated on the device, with that test's caps"""
    n = int(fs * MS * 0.001)
    scene = []
    for i, s in enumerate(sats):
        t = simulate.tracker(s["tracker"])
        periods = int(MS * 0.001 * codes.chip_rate(t.code) / codes.code_length(t.code)) + 2
        sym = simulate.symbols(s["tracker"], s["item"], -(-periods // s["bit"]), s["bit"], 100 + i)
        scene.append(simulate.Satellite(s["tracker"], s["item"], s["amp"], s["doppler"], s["code0"], symbols=sym))
    x = simulate.recording(scene, fs, coffset, n, 31, 12.0, engine=engine).cpu().numpy()
    items = [s["item"] for s in sats] + [noise_item]
    results, refined, loop, x_dev = handoff.handoff(name, x, fs, coffset, items=items, loop_dwells=DWELLS, ms=80, doppler_search=doppler_search,
                                                    engine=engine)
    try:
        assert [it for it, _ in refined] == items and loop.K == len(items)
        L = codes.code_length(trackloop.TRACKERS[handoff.tracker_name(name)].code)
        for s, (it, r), res in zip(sats, refined, results):
            print("%s %d: acquired doppler %.1f code %.2f -> refined doppler error %.3f Hz, code error %.5f chip, ratio %.1f"
                  % (name, it, res[2], res[1], r.doppler - s["doppler"], _code_error(r.code_offset, s["code0"], L), r.ratio))
        for s, (it, r) in zip(sats, refined):
            assert abs(r.doppler - s["doppler"]) <= 10.0, (it, r)
            assert _code_error(r.code_offset, s["code0"], L) <= 0.03, (it, r)
        recs = loop.run([x_dev] * loop.K)
        assert list(loop.status) == [0] * loop.K
    finally:
        loop.close()
    noise = float(np.mean(recs[-1]["prompt"][:200]))
    for s, r in zip(sats, recs):
        assert len(r) >= 200
        print("  %d: carrier_f[199] error %.3f Hz, mean prompt %.1f, noise channel %.1f" % (s["item"], r["carrier_f"][199] - s["doppler"],
                                                                                          np.mean(r["prompt"][:200]), noise))
        assert abs(r["carrier_f"][199] - s["doppler"]) <= 10.0, (s, r["carrier_f"][199])
        assert np.mean(r["prompt"][:200]) > 3.0 * noise, (s, np.mean(r["prompt"][:200]), noise)


@pytest.mark.gpu
def test_pipeline_gps_l1_three_satellites(engine):
    sats = [dict(tracker="gps-l1", item=7, amp=3.0, bit=20, doppler=1234.5, code0=417.37),
            dict(tracker="gps-l1", item=19, amp=3.0, bit=20, doppler=-1840.2, code0=88.71),
            dict(tracker="gps-l1", item=30, amp=3.0, bit=20, doppler=3071.9, code0=1001.13)]
    _pipeline("gps-l1", 6.0e6, 250000.0, sats, 25, engine)


@pytest.mark.gpu
def test_pipeline_galileo_e1b(engine):
    """kind 2 (CBOC); 10 MS/s: above twice the 4 MHz cutoff of the signal's acquisition front-end"""
    sats = [dict(tracker="galileo-e1b", item=11, amp=3.0, bit=20, doppler=-1377.3, code0=2500.42)]
    _pipeline("galileo-e1b", 10.0e6, -150000.0, sats, 30, engine, doppler_search=[-3000.0, 3000.0, 50.0])


@pytest.mark.gpu
def test_command_line_writes_a_file_the_track_command_takes(tmp_path, engine):
    fs, coffset, seconds = 6.0e6, 250000.0, 0.25
    path = str(tmp_path / "scene.bin")
    argv = ["--fs", repr(fs), "--coffset", repr(coffset), "--seconds", repr(seconds), "--seed", "31", "--sat", "gps-l1,7,3.0,1234.5,417.37,20",
            "--sat", "gps-l1,19,3.0,-1840.2,88.71,20", path]
    out = io.StringIO()
    lines = simulate.run(argv, out, piece_bytes=1 << 20)                           # three pieces
    assert out.getvalue().splitlines() == lines and len(lines) == 2
    _, sats = simulate.parse(argv)
    n = int(fs * seconds)
    whole = simulate.recording(sats, fs, coffset, n, 31, engine=engine).cpu().numpy()
    assert np.fromfile(path, dtype=np.int8).tobytes() == whole.tobytes()           # the file does not depend on the piece size
    def prompt(args):
        rows = [r.split() for r in track.run(args[0], ["--loop-dwells", "20,20"] + args[1:], io.StringIO())]
        assert len(rows) >= 200
        return rows, float(np.mean([float(r[7]) for r in rows[:200]]))

    _, noise = prompt(lines[0].split()[:4] + ["25", "0.0", "0.0"])                   # a PRN that is not in the file
    for line, doppler in zip(lines, (1234.5, -1840.2)):
        rows, p = prompt(line.split())
        assert abs(float(rows[199][3]) - doppler) <= 10.0, (line, rows[199])
        assert p > 3.0 * noise, (line, p, noise)
