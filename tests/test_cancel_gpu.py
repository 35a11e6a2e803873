"""GPU: the cancellation kernels (csrc/gacq_cancel.hip) against the fp64 oracle of tests/cancel_oracle.py, the int8 form against the
device's own complex64 form, estimated amplitudes, independence of how a recording is cut into calls and of where the buffers lie,
the argument checks through the raw ABI, the segments of segments_from_track against the loop's own prompts, and the near-far scene
end to end.

Bounds, per case: four times the deviation of the numpy float32 evaluation of the same formula (cancel_oracle.evaluate(f32=True);
for amplitudes float32 products under fp64 sums) from the fp64 one, relative to max |v| (max |A|); all three figures are printed
before the assertion (DESIGN 5.24 has the table)."""
import io

import numpy as np
import pytest

import cancel_cases as C
import cancel_oracle as O
from gnss_dsp_tools_amd import _native as nat
from gnss_dsp_tools_amd import cancel, handoff, signals, simulate
from test_cancel_cpu import bad_calls, raw_call


def _run(engine, case, dtype, estimate=False, segs=None, **kw):
    return cancel.apply(engine, case["sats"], case["segs"] if segs is None else segs, case["fs"], case["x"], case["in_first"], case["out_first"],
                        case["n_out"], estimate, dtype, case["in_complex64"], **kw)


def _with_amps(segs, amps):
    out = []
    for g, a in zip(segs, amps):
        g = g.copy()
        g["amp_re"], g["amp_im"] = a.real, a.imag
        out.append(g)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(C.CASES))
def test_subtraction_matches_the_fp64_oracle(engine, name):
    case = C.CASES[name]
    want, f32 = C.reference(name)
    got, amps, clipped = _run(engine, case, "complex64")
    got = got.cpu().numpy()
    assert got.shape == want.shape == (case["n_out"],) and got.dtype == np.complex64 and clipped == 0
    for a, g in zip(amps, C.given_amps(case)):                                       # given amplitudes come back as given
        touched = ~np.isnan(a)
        assert np.array_equal(a[touched], g[touched]) and touched.any()
    scale = float(np.max(np.abs(want)))
    dev32 = float(np.max(np.abs(f32 - want))) / scale
    err = float(np.max(np.abs(got - want))) / scale
    print("%-14s K %2d  numpy float32 deviation %.3g  bound %.3g  device %.3g" % (name, len(case["sats"]), dev32, 4 * dev32, err))
    assert err <= 4 * dev32


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(C.CASES))
def test_int8_is_the_rounded_complex64_of_the_device(engine, name):
    case = C.CASES[name]
    v = _run(engine, case, "complex64")[0].cpu().numpy()
    got, _, clipped = _run(engine, case, "int8")
    got = got.cpu().numpy()
    assert got.dtype == np.int8 and got.shape == (2 * case["n_out"],)
    assert np.array_equal(got, O.to_int8(v))
    assert got.min() >= -127 and clipped == O.clip_count(got)                        # -128 goes in (cancel_cases.noise_int8), -127 comes out
    if name == "clip":
        assert got.max() == 127 and got.min() == -127 and clipped > 100
    if not case["in_complex64"]:
        assert case["x"].min() == -128


@pytest.mark.gpu
@pytest.mark.parametrize("name", C.ESTIMATE_CASES)
def test_estimated_amplitudes_match_the_oracle_and_drive_the_same_subtraction(engine, name):
    case = C.estimate_case(name)
    want, f32 = C.estimate_reference(name)
    out, amps, _ = _run(engine, case, "complex64", estimate=True)
    assert all(not np.isnan(a).any() for a in amps)
    scale = max(float(np.max(np.abs(w))) for w in want)
    dev32 = max(float(np.max(np.abs(a - w))) for a, w in zip(f32, want)) / scale
    err = max(float(np.max(np.abs(a - w))) for a, w in zip(amps, want)) / scale
    print("%-14s segments %2d  float32 products deviation %.3g  bound %.3g  device %.3g" % (name, sum(len(a) for a in amps), dev32, 4 * dev32, err))
    assert err <= 4 * dev32
    # the signals were put in at the segments' amplitudes: the projection finds them up to the noise, sigma sqrt(2 / n) for sigma = 12
    # (twelve of them: the return-to-zero kinds have half the weight, and the other satellites correlate a little)
    for a, g, sg in zip(amps, C.given_amps(case), case["segs"]):
        long = sg["n"] >= 2000
        assert np.all(np.abs(a[long] - g[long]) < 12 * 12.0 * np.sqrt(2.0 / sg["n"][long])), (name, a, g)
    # an estimate = 1 call is an estimate = 0 call fed the returned amplitudes, byte for byte
    for dtype in ("complex64", "int8"):
        a = _run(engine, case, dtype, estimate=True)[0].cpu().numpy()
        b = _run(engine, case, dtype, segs=_with_amps(case["segs"], amps))[0].cpu().numpy()
        assert a.tobytes() == b.tobytes()
    assert out.cpu().numpy().tobytes() == _run(engine, case, "complex64", segs=_with_amps(case["segs"], amps))[0].cpu().numpy().tobytes()


# unequal cuts of the estimate cases (8183, 13555 and 4183 samples); the rest is the last piece
CUTS = {"far": (1, 2047, 4093, 8), "kinds": (4129, 7, 2048, 5000), "complex64 in": (100, 4001, 30)}


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["int8", "complex64"])
@pytest.mark.parametrize("name", sorted(CUTS))
def test_cutting_the_recording_into_calls_does_not_matter(engine, name, dtype):
    torch = nat.require_torch()
    case = C.estimate_case(name)
    whole, amps, clipped = _run(engine, case, dtype, estimate=True)
    n, unit = case["n_out"], (1 if case["in_complex64"] else 2)
    assert case["out_first"] == case["in_first"] and len(case["x"]) == unit * n
    if name == "far":
        assert case["in_first"] < 2 ** 33 < case["in_first"] + n
    can = cancel.Canceller(engine, case["sats"], case["segs"], case["fs"], True, dtype, case["in_complex64"], start=case["in_first"])
    parts, at = [], 0
    assert sum(CUTS[name]) < n
    for m in CUTS[name] + (n - sum(CUTS[name]),):
        parts.append(can.feed(case["x"][unit * at:unit * (at + m)]))
        at += m
    assert at == n and can.next_out == case["in_first"] + n and sum(p.numel() > 0 for p in parts) >= 2
    assert whole.cpu().numpy().tobytes() == torch.cat(parts).cpu().numpy().tobytes()
    assert can.clipped == clipped
    for a, b in zip(amps, can.amps):                                                 # the same bits
        assert a.tobytes() == b.tobytes() and not np.isnan(a).any()
    # ... and a piece written into the middle of a caller's buffer, at an address that is not 16-byte aligned, from an input that
    # does not start on 16 bytes either: the same bytes, the guard bytes untouched
    per = 2 if dtype == "int8" else 1
    first, cnt = 1029, 3001
    buf = torch.zeros(per * cnt + 6, dtype=whole.dtype, device=whole.device)
    if dtype == "int8":
        buf += 77
    pad = 1 if case["in_complex64"] else 6
    x = np.concatenate([np.zeros(pad, dtype=case["x"].dtype), case["x"]])
    xd = torch.from_numpy(x).to(whole.device)[pad:]
    assert xd.data_ptr() % 16 != 0 and buf[3:].data_ptr() % 16 != 0
    # the segments that touch the piece must lie in the input as a whole: the piece is cut out of the output, not out of the input
    got, amps2, _ = cancel.apply(engine, case["sats"], case["segs"], case["fs"], xd, case["in_first"], case["in_first"] + first, cnt, True, dtype,
                                 case["in_complex64"], out=buf[3:3 + per * cnt])
    assert buf[3:3 + per * cnt].cpu().numpy().tobytes() == whole[per * first:per * (first + cnt)].cpu().numpy().tobytes()
    guard = 77 if dtype == "int8" else 0
    assert bool((buf[:3] == guard).all()) and bool((buf[3 + per * cnt:] == guard).all())
    for a, b in zip(amps, amps2):
        t = ~np.isnan(b)
        assert t.any() and a[t].tobytes() == b[t].tobytes()


@pytest.mark.gpu
def test_every_argument_check_through_the_raw_abi(engine):
    torch = nat.require_torch()
    engine.use_torch_stream()
    dev = "cuda:%d" % engine.device
    out = torch.full((4096,), 77, dtype=torch.int8, device=dev)
    x = torch.full((4096,), 3, dtype=torch.int8, device=dev)
    for label, code, change in bad_calls():
        rc = raw_call(engine._ctx, x.data_ptr(), out.data_ptr(), **change)
        assert rc == code, (label, rc, nat.lib.gacq_last_error(engine._ctx))
    torch.cuda.synchronize()
    assert bool((out == 77).all())
    assert raw_call(engine._ctx, x.data_ptr(), out.data_ptr(), n_out=0) == 0          # n_out = 0 does nothing
    torch.cuda.synchronize()
    assert bool((out == 77).all())
    assert raw_call(engine._ctx, x.data_ptr(), out.data_ptr()) == 0                   # the unchanged call is accepted and writes 400 bytes
    torch.cuda.synchronize()
    h = out.cpu().numpy()
    assert (h[400:] == 77).all() and not (h[:400] == 77).all()


def _scene(sats, n, engine, N=C.NEARFAR):
    scene = []
    for i, s in enumerate(sats):
        sym = None
        if "bit" in s:
            periods = int(N["ms"] * 0.001 * 1.023e6 / 1023) + 2
            sym = simulate.symbols("gps-l1", s["item"], -(-periods // s["bit"]), s["bit"], 100 + i)
        scene.append(simulate.Satellite("gps-l1", s["item"], s["amp"], s["doppler"], s["code0"], symbols=sym))
    return scene, simulate.recording(scene, N["fs"], N["coffset"], n, N["seed"], N["sigma"], engine=engine).cpu().numpy()


@pytest.mark.gpu
def test_segments_fit_the_loop(engine):
    """sum x conj(r) over a record's segment is the record's prompt: the loop's two table NCOs floor the phase to 1/1024 turn each, at
    most 2 x 2 pi / 1024 = 0.0123 rad together, and about one sample in a thousand may fall across a chip edge between the loop's fp64
    code position and the 2^-64 one: 0.015 |p|.  Measured: 0.0031 |p| at the most over 69 records; the derived bound is kept."""
    N = C.NEARFAR
    fs, st = N["fs"], N["strong"]
    n = int(fs * 0.120)
    _, x = _scene([st], n, engine)
    results, refined, loop, x_dev = handoff.handoff("gps-l1", x, fs, N["coffset"], items=[st["item"]], doppler_search=list(N["doppler_search"]),
                                                    ms=N["search_ms"], loop_dwells=N["loop_dwells"], engine=engine)
    try:
        assert loop is not None and loop.K == 1
        state0 = loop.state(0)
        recs = loop.run([x_dev])[0]
        ch = loop.channels[0]
    finally:
        loop.close()
    skip = 50                                                                        # the pull-in: 20 + 20 ms of frequency lock, and settling
    assert len(recs) >= 110
    segs = cancel.segments_from_track(ch, state0, recs, skip)
    assert len(segs) == len(recs) - skip and np.array_equal(segs["s0"][1:], segs["s0"][:-1] + segs["n"][:-1])
    assert np.array_equal(segs["s0"] + segs["n"] - int(state0["pos"]), recs["samp"][skip:])
    xc = C.as_complex(x, False)
    sat = C.oracle_sat(cancel.sat_of(ch))
    worst = 0.0
    for g, r in zip(segs, recs[skip:]):
        w, turn = O.replica_parts(sat, g, fs)
        s0, m = int(g["s0"]), int(g["n"])
        c = np.sum(xc[s0:s0 + m] * w * np.exp(-2j * np.pi * turn))
        p = complex(r["p_re"], r["p_im"])
        worst = max(worst, abs(c - p) / abs(p))
    print("%d records after pull-in: sum x conj(r) differs from the prompt by at most %.4f |p| (bound 0.015)" % (len(segs), worst))
    assert worst <= 0.015


def _code_error(got, want, L=1023.0):
    return abs((got - want + L / 2.0) % L - L / 2.0)


@pytest.mark.gpu
def test_near_far_the_weak_satellite_is_found_on_the_residual(engine):
    """PRN 5 at amplitude 12 hides PRN 9 at amplitude 1 (cancel_cases.NEARFAR has the CPU experiment that fixed the amplitude): on the
    input the 20 ms search puts PRN 9 into a wrong cell, on the residual of cancel_tracked into the true one."""
    N = C.NEARFAR
    fs, st, wk = N["fs"], N["strong"], N["weak"]
    n = int(fs * 0.001 * N["ms"])
    scene, x = _scene([st, wk], n, engine)
    res, (results, refined), recs = cancel.cancel_tracked("gps-l1", x, fs, N["coffset"], items=[st["item"]], skip=N["skip"],
                                                          doppler_search=list(N["doppler_search"]), ms=N["search_ms"], loop_dwells=N["loop_dwells"],
                                                          engine=engine)
    assert [it for it, _ in refined] == [st["item"]] and len(recs) == 1 and len(recs[0]) >= 290
    assert res.dtype == nat.require_torch().int8 and res.numel() == 2 * n
    r8 = res.cpu().numpy()
    assert np.array_equal(r8[:2 * 4092 * 50], np.clip(x[:2 * 4092 * 50], -127, 127))    # nothing is cancelled during the pull-in
    w0 = N["window"]
    assert int(recs[0]["samp"][N["skip"]]) < w0                                      # the window starts after the cancelled part begins
    sig = signals.get("gps-l1")
    items = [st["item"], wk["item"], N["absent"]]
    before = dict(cancel.reacquire(engine, sig, x, fs, N["coffset"], w0, items, N["doppler_search"], N["search_ms"]))
    after = dict(cancel.reacquire(engine, sig, r8, fs, N["coffset"], w0, items, N["doppler_search"], N["search_ms"]))
    for it in items:
        print("prn %2d  input metric %.2f code %.2f doppler %.0f   residual metric %.2f code %.2f doppler %.0f" % ((it,) + tuple(before[it]) + tuple(after[it])))
    true_code = (wk["code0"] + w0 * scene[1].code_rate_hz() / fs) % 1023.0
    true_bin = 200.0 * round(wk["doppler"] / 200.0)
    one_sample = 1.023e6 / fs
    print("true cell of prn %d: code %.2f doppler %.0f" % (wk["item"], true_code, true_bin))
    m, code, dop = after[wk["item"]]
    assert dop == true_bin and _code_error(code, true_code) <= one_sample
    assert after[st["item"]][0] < 0.5 * before[st["item"]][0]
    assert m > before[wk["item"]][0]
    m, code, dop = before[wk["item"]]
    assert not (dop == true_bin and _code_error(code, true_code) <= one_sample)       # the miss on the input
    pin = float(np.mean(x[2 * w0:].astype(np.float64) ** 2))
    pout = float(np.mean(r8[2 * w0:].astype(np.float64) ** 2))
    print("power per component %.1f -> %.1f (sigma^2 + 12^2 / 2 = 216, sigma^2 = 144)" % (pin, pout))
    assert pout < pin - 60.0


@pytest.mark.gpu
def test_command_line_writes_the_residual_and_reacquires_the_weak_satellite(tmp_path, engine):
    N = C.NEARFAR
    fs, st, wk = N["fs"], N["strong"], N["weak"]
    n = int(fs * 0.001 * N["ms"])
    scene, x = _scene([st, wk], n, engine)
    src, dst = str(tmp_path / "scene.iq"), str(tmp_path / "residual.iq")
    x.tofile(src)
    out = io.StringIO()
    lines = cancel.run("gps-l1", ["--prn", str(st["item"]), "--reacquire", "--skip", str(N["skip"]), "--loop-dwells", "20,20", "--time", str(N["search_ms"]),
                                  "--doppler-search", ",".join("%g" % v for v in N["doppler_search"]), src, repr(fs), repr(N["coffset"]), dst], out)
    assert out.getvalue().splitlines() == lines and len(lines) == 2 + 31
    f = lines[0].split()
    assert f[:4] == ["cancelled", "5", "samples", str(n)] and f[4] == "clipped" and f[6] == "power" and f[8] == "->" and f[10] == "dB"
    assert float(f[7]) - float(f[9]) > 1.0                                           # 216 -> 144 over 240 of 300 ms: 1.3 dB
    res = cancel.cancel_tracked("gps-l1", x, fs, N["coffset"], items=[st["item"]], skip=N["skip"], doppler_search=list(N["doppler_search"]),
                                ms=N["search_ms"], loop_dwells=N["loop_dwells"], engine=engine)[0]
    assert np.fromfile(dst, dtype=np.int8).tobytes() == res.cpu().numpy().tobytes()
    assert lines[1].startswith("residual searched from sample ")
    start = int(lines[1].split()[-1])
    assert 60 * 4000 < start < 62 * 4200
    rows = {int(l.split()[1]): l.split() for l in lines[2:]}
    assert sorted(rows) == [p for p in range(1, 33) if p != st["item"]]
    true_code = (wk["code0"] + start * scene[1].code_rate_hz() / fs) % 1023.0
    r = rows[wk["item"]]
    print(lines[0], "|", lines[1], "|", " ".join(r), "| true code %.2f" % true_code)
    assert float(r[3]) == 200.0 * round(wk["doppler"] / 200.0) and _code_error(float(r[7]), true_code) <= 1.023e6 / fs + 0.05      # one sample, and the printed digit
    assert float(r[5]) == max(float(v[5]) for v in rows.values())                    # no other item stands above it
