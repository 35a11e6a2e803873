"""GPU: the array-prompt kernels (csrc/gacq_aprompt.hip) bit for bit against the device's own gacq_cancel_dev estimates on every antenna
alone, against the fp64 oracle of tests/cancel_oracle.py, the segments outside the input, the independence of the antenna count, the
order of the rows, the addresses and the call, the refusals through the raw ABI, and two scenes of tests/scene end to end: three
satellites from three directions, and the same three from one (a spoofer).

Bounds.  Oracle: four times the deviation of the numpy evaluation with float32 products from the fp64 one, relative to max |A| of the
row, as tests/test_cancel_gpu.py has it.  Steering vectors: arrayprompt_cases.unit, 6 sqrt(2) sigma_c / (|s| sqrt(D)) per entry with
sigma_c = 12 / sqrt(n) for segments of n samples, |s| = 4 and D the segments used.  All figures are printed before the assertion."""
import ctypes
import functools
import io

import numpy as np
import pytest

import arrayprompt_cases as AC
import bearing_cases as BC
import cancel_cases as C
import cancel_oracle as O
from gnss_dsp_tools_amd import _native as nat
from gnss_dsp_tools_amd import arrayfilter, arrayprompt, bearing, cancel, scene, simulate
from test_arrayprompt_cpu import bad_calls, raw_args

BIT_CASES = ("kinds", "far", "complex64 in", "overlap32", "clip")
_AMPS = {}


def _project(engine, case, rows, segs=None, in_first=None):
    return arrayprompt.project(engine, case["sats"], case["segs"] if segs is None else segs, case["fs"], rows,
                               case["in_first"] if in_first is None else in_first, case["in_complex64"])


def _cancel_amps(engine, name, p):
    """gacq_cancel_dev's estimates of the case's own segments on antenna p alone: the device's reference, computed once"""
    if (name, p) not in _AMPS:
        case = AC.array_case(name)
        _AMPS[name, p] = cancel.apply(engine, case["sats"], case["base"], case["fs"], case["rows"][p], case["in_first"], estimate=True, dtype="complex64",
                                      in_complex64=case["in_complex64"])[1]
    return _AMPS[name, p]


@functools.lru_cache(maxsize=None)
def _energies(name):
    """sum w^2 of the case's own segments as include/gacq.h defines it: w of tests/cancel_oracle.py rounded to float32, the square a
    float32 product, the sum in fp64"""
    case = AC.array_case(name)
    out = []
    for s, g in zip(case["sats"], case["base"]):
        sat = C.oracle_sat(s)
        e = []
        for seg in g:
            w = O.replica_parts(sat, seg, case["fs"])[0].astype(np.float32)
            e.append(float(np.sum((w * w).astype(np.float64))))
        out.append(np.array(e))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("M", [1, 2, 3, 8])
@pytest.mark.parametrize("name", BIT_CASES)
def test_prompts_are_the_bits_of_cancel_on_every_antenna_alone(engine, name, M):
    case = AC.array_case(name)
    prompts, energy = _project(engine, case, case["rows"][:M])
    assert len(prompts) == len(energy) == len(case["sats"])
    for k, (P, E, own) in enumerate(zip(prompts, energy, case["own"])):
        assert P.shape == (len(case["segs"][k]), M) and P.dtype == np.complex128 and E.shape == (len(P),) and E.dtype == np.float64
        for p in range(M):
            want = _cancel_amps(engine, name, p)[k]
            assert not np.isnan(want).any() and len(want) == len(own)
            assert np.array_equal(AC.bits(P[own, p]), AC.bits(want)), (name, M, k, p)
        ref = _energies(name)[k]
        if case["sats"][k].kind == 2:                           # the weights' squares are not float32 numbers: another order of the fp64 sum
            assert np.all(np.abs(E[own] - ref) <= 1e-12 * ref), (name, k, E[own], ref)
        else:
            assert np.array_equal(E[own], ref), (name, k, E[own], ref)
    if name == "kinds":
        n = np.concatenate([g["n"] for g in case["base"]])
        assert (n == 1).any() and (n < 256).any() and (n % 256 != 0).any() and (n % 256 == 0).any() and sorted(s.kind for s in case["sats"]) == list(range(6))
    if name == "far":
        assert case["in_first"] < 2 ** 33 < case["in_first"] + case["n"]
    if name == "overlap32":
        assert len(case["sats"]) == 32


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["kinds", "complex64 in"])
def test_prompts_match_the_fp64_oracle(engine, name):
    case = AC.array_case(name)
    M = 3
    prompts, _ = _project(engine, case, case["rows"][:M])
    for p in range(M):
        x = C.as_complex(case["rows"][p], case["in_complex64"])
        want, f32 = [[np.array([O.estimate(C.oracle_sat(s), g, case["fs"], x, case["in_first"], f32=f) for g in sg]) for s, sg in zip(case["sats"], case["base"])]
                     for f in (False, True)]
        got = [P[own, p] for P, own in zip(prompts, case["own"])]
        scale = max(float(np.max(np.abs(w))) for w in want)
        dev32 = max(float(np.max(np.abs(a - w))) for a, w in zip(f32, want)) / scale
        err = max(float(np.max(np.abs(a - w))) for a, w in zip(got, want)) / scale
        print("%-14s antenna %d  segments %2d  float32 products deviation %.3g  bound %.3g  device %.3g" % (name, p, sum(len(a) for a in got), dev32, 4 * dev32, err))
        assert err <= 4 * dev32


@pytest.mark.gpu
@pytest.mark.parametrize("name", BIT_CASES)
def test_segments_outside_the_input_are_left_alone(engine, name):
    case = AC.array_case(name)
    where = np.concatenate(case["where"])
    assert (where == AC.OUTSIDE).sum() >= len(case["sats"])                           # one past the input for every satellite at the least
    if name in ("kinds", "far", "complex64 in"):
        assert (where == AC.STRADDLE).sum() >= 2                                      # one at either end
    if name in ("kinds", "far"):
        assert (where == AC.OUTSIDE).sum() > len(case["sats"])                        # wholly before the input, too
    prompts, energy = _project(engine, case, case["rows"][:3])
    P, E = np.concatenate(prompts), np.concatenate(energy)
    inside = where == AC.INSIDE
    assert np.isnan(P[~inside].real).all() and np.isnan(P[~inside].imag).all() and np.isnan(E[~inside]).all()
    assert np.isfinite(P[inside].real).all() and np.isfinite(P[inside].imag).all() and np.isfinite(E[inside]).all()


@pytest.mark.gpu
def test_bits_do_not_depend_on_the_rows_order_number_or_addresses(engine):
    torch = nat.require_torch()
    case = AC.array_case("kinds")
    rows = case["rows"]
    full, e_full = _project(engine, case, rows)
    perm = [5, 0, 7, 2, 2, 1, 6, 3]                                                  # an antenna twice: rows may share a buffer
    got, e_perm = _project(engine, case, [rows[p] for p in perm])
    for a, b, ea, eb in zip(full, got, e_full, e_perm):
        assert np.array_equal(AC.bits(a[:, perm]), AC.bits(b)) and np.array_equal(AC.bits(ea), AC.bits(eb))
    for m in (1, 3, 5, 7):                                                           # 3, 5 and 7 run the padded forms
        part, e_part = _project(engine, case, rows[:m])
        for a, b, ea, eb in zip(full, part, e_full, e_part):
            assert b.shape[1] == m and np.array_equal(AC.bits(a[:, :m]), AC.bits(b)) and np.array_equal(AC.bits(ea), AC.bits(eb))
    # int8 rows as slices at odd byte offsets of one larger buffer, and as the rows of a 2-D tensor
    nb = 2 * case["n"]
    buf = torch.zeros(4 * (nb + 3) + 1, dtype=torch.int8, device="cuda:%d" % engine.device)
    views = []
    for p in range(4):
        at = 1 + p * (nb + 2)
        buf[at:at + nb] = torch.from_numpy(np.array(rows[p])).to(buf.device)
        views.append(buf[at:at + nb])
    assert all(v.data_ptr() % 2 == 1 for v in views)
    odd, _ = _project(engine, case, views)
    flat, _ = _project(engine, case, torch.stack([torch.from_numpy(np.array(r)) for r in rows[:4]]).to(buf.device))
    for a, b, c in zip(full, odd, flat):
        assert np.array_equal(AC.bits(a[:, :4]), AC.bits(b)) and np.array_equal(AC.bits(a[:, :4]), AC.bits(c))


# name -> (the first call ends before this sample, the second begins at this one), counted from the case's first sample: in every case
# some segments lie in both calls, some in the first alone and some in the second alone
CALLS = {"kinds": (11521, 3388), "far": (7000, 400), "complex64 in": (4100, 50)}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CALLS))
def test_bits_do_not_depend_on_the_call(engine, name):
    """two calls over two overlapping parts of the input: the segments both contain have the bits of the whole call"""
    case = AC.array_case(name)
    n, unit = case["n"], (1 if case["in_complex64"] else 2)
    rows = case["rows"][:3]
    whole = np.concatenate(_project(engine, case, rows)[0])
    a_end, b_first = CALLS[name]
    assert b_first < a_end < n
    a = np.concatenate(_project(engine, case, [r[:unit * a_end] for r in rows])[0])
    b = np.concatenate(_project(engine, case, [r[unit * b_first:] for r in rows], in_first=case["in_first"] + b_first)[0])
    in_a, in_b, in_w = [~np.isnan(v).any(axis=1) for v in (a, b, whole)]
    both = in_a & in_b
    assert both.any() and (in_a & ~in_b).any() and (in_b & ~in_a).any() and not (~in_w & (in_a | in_b)).any()
    assert np.array_equal(AC.bits(a[in_a]), AC.bits(whole[in_a])) and np.array_equal(AC.bits(b[in_b]), AC.bits(whole[in_b]))
    assert np.array_equal(AC.bits(a[both]), AC.bits(b[both]))


@pytest.mark.gpu
def test_a_refused_call_writes_nothing(engine):
    torch = nat.require_torch()
    engine.use_torch_stream()
    dev = "cuda:%d" % engine.device
    xs = [torch.full((4096,), 3 + p, dtype=torch.int8, device=dev) for p in range(3)]
    rows = [xs[0].data_ptr(), xs[1].data_ptr(), xs[2].data_ptr() + 3]                # the third at an odd address, as in the CPU test
    prompts = np.full((3, 3), 77.0 + 77.0j, dtype=np.complex128)
    energy = np.full(3, 77.0)
    out = (ctypes.c_void_p(prompts.ctypes.data), ctypes.c_void_p(energy.ctypes.data))
    for label, code, change in bad_calls():
        keep, a = raw_args(**dict(dict(rows=rows), **change))
        rc = nat.lib.gacq_aprompt_dev(engine._ctx, *a, *out)
        assert rc == code, (label, rc, nat.lib.gacq_last_error(engine._ctx))
        assert (prompts == 77.0 + 77.0j).all() and (energy == 77.0).all(), label
    keep, a = raw_args(rows=rows)
    assert nat.lib.gacq_aprompt_dev(engine._ctx, *a, ctypes.c_void_p(0), out[1]) == -1 and (energy == 77.0).all()      # no place for the prompts
    assert nat.lib.gacq_aprompt_dev(engine._ctx, *a, *out) == 0                       # the unchanged call is accepted
    assert np.isfinite(prompts.real).all() and not (prompts == 77.0 + 77.0j).any()
    assert energy[0] == 100.0 and energy[1] == 50.0 and 0.0 < energy[2] < 2.0 * 90.0  # plain chips: one per sample; the CBOC weights are not
    keep, a = raw_args(rows=rows)
    assert nat.lib.gacq_aprompt_dev(engine._ctx, *a, out[0], ctypes.c_void_p(0)) == 0                                  # energy_out may be NULL
    with pytest.raises(nat.GacqError):
        arrayprompt.project(engine, [cancel.Sat("gps.nope", 1, 0)], [C.segs(C.seg(0, 10, 0.0, 0.0, 1.023e6, 0.0))], 4.092e6, xs[:2])
    with pytest.raises(ValueError):
        arrayprompt.project(engine, [cancel.Sat("gps.ca", 1, 0)], [C.segs(C.seg(0, 10, 0.0, 0.0, 1.023e6, 0.0))], 4.092e6, [xs[0], xs[1][:100]])
    good = arrayprompt.project(engine, [cancel.Sat("gps.ca", 1, 0)], [C.segs(C.seg(0, 10, 0.0, 0.0, 1.023e6, 0.0))], 4.092e6, xs[:2])
    assert good[0][0].shape == (1, 2) and np.isfinite(good[0][0].real).all() and good[1][0][0] == 10.0


# ---- end to end: GPS L1 at 4.092 MHz, sigma 12, 200 ms on ring(4); PRNs 5, 9 and 21 at amplitude 4
FS, SIGMA, AMP, MS, SKIP = 4.092e6, 12.0, 4.0, 200, 50
PRNS = ((5, 1510.0, 417.3, 20), (9, -2210.0, 305.6, None), (21, 640.0, 811.9, None))     # item, Doppler, code phase, periods per data bit
CELLS = bearing.grid(5.0, 5.0)
_SCENES = {}


def _scene(engine, spoofed):
    """(rows: int8 CUDA tensor [4, 2 n], gains [4, 3]) of the genuine scene (three directions) or the spoofed one (all from (160, 35))"""
    if spoofed not in _SCENES:
        el = BC.ring(4)
        dirs = [AC.DIRECTIONS[1]] * 3 if spoofed else AC.DIRECTIONS
        gains = np.stack([scene.steering(el, az, e) for az, e in dirs], axis=1)
        sats = []
        for i, (item, dop, code0, bit) in enumerate(PRNS):
            sym = simulate.symbols("gps-l1", item, -(-(MS + 2) // bit), bit, 300 + i) if bit else None
            sats.append(simulate.Satellite("gps-l1", item, AMP, dop, code0, 0.1 * i, symbols=sym))
        rows = scene.recording(sats, [], gains, FS, 0.0, int(FS * 0.001 * MS), 4321 + int(spoofed), SIGMA, engine=engine)
        _SCENES[spoofed] = (rows, gains)
    return _SCENES[spoofed]


def _measure(engine, spoofed):
    N = C.NEARFAR
    rows, gains = _scene(engine, spoofed)
    key = ("measured", spoofed)
    if key not in _SCENES:
        _SCENES[key] = arrayprompt.measure_tracked("gps-l1", rows, FS, 0.0, track=0, items=[p[0] for p in PRNS], skip=SKIP,
                                                   doppler_search=list(N["doppler_search"]), ms=N["search_ms"], loop_dwells=N["loop_dwells"], engine=engine)
    return _SCENES[key] + (gains,)


def _cell(az, el):
    return int(np.flatnonzero((CELLS[:, 0] == az) & (CELLS[:, 1] == el))[0])


def _neighbours(g, want):
    daz = abs((CELLS[g, 0] - CELLS[want, 0] + 180.0) % 360.0 - 180.0)
    return daz <= 5.0 and abs(CELLS[g, 1] - CELLS[want, 1]) <= 5.0


@pytest.mark.gpu
def test_three_satellites_from_three_directions_end_to_end(engine):
    chans, prompts, ests, gains = _measure(engine, False)
    assert [int(c.prn) for c in chans] == [p[0] for p in PRNS]                       # all three are tracked
    vecs = []
    for k, (c, P, e) in enumerate(zip(chans, prompts, ests)):
        assert len(e) == 1 and P.shape[1] == 4 and len(P) >= MS - SKIP - 5
        e = e[0]
        true = gains[:, k] / gains[0, k]
        unit = AC.unit(e.used, AMP / (SIGMA / np.sqrt(FS * 0.001)))
        worst = float(np.max(np.abs(e.a_hat - true)))
        g, az, el, beam = arrayprompt.direction(e.a_hat, BC.ring(4), CELLS)
        print("prn %2d  records %d  quality %.4f  worst entry %.4f (bound %.4f)  az %g el %g beam %.4f  true %g %g" % (c.prn, e.used, e.quality, worst, unit,
                                                                                                                  az, el, beam, *AC.DIRECTIONS[k]))
        assert e.used >= MS - SKIP - 5 and worst <= unit and e.quality > 0.95
        assert _neighbours(g, _cell(*AC.DIRECTIONS[k]))
        vecs.append(e.a_hat)
    coh = arrayprompt.coherence(vecs)[np.triu_indices(3, 1)]
    print("coherences %.4f %.4f %.4f (true values at most 0.434)" % tuple(coh))
    assert (coh < 0.6).all()
    # one vector per dwell of 50 records: three of them, each within its own bound
    for k, P in enumerate(prompts):
        for e in arrayprompt.dwell_estimates(P, 50):
            if e.used == 50:
                assert np.max(np.abs(e.a_hat - gains[:, k] / gains[0, k])) <= AC.unit(50, AMP / (SIGMA / np.sqrt(FS * 0.001)))


@pytest.mark.gpu
def test_three_satellites_from_one_direction_are_alike(engine):
    chans, prompts, ests, gains = _measure(engine, True)
    assert [int(c.prn) for c in chans] == [p[0] for p in PRNS]
    coh = arrayprompt.coherence([e[0].a_hat for e in ests])[np.triu_indices(3, 1)]
    print("spoofed scene: coherences %.5f %.5f %.5f" % tuple(coh))
    assert (coh > 0.99).all()
    assert arrayprompt.coherence_line([e[0].a_hat for e in ests]).endswith("pairs 3 directions alike")


def _run_command(engine, tmp_path, spoofed, extra=()):
    N = C.NEARFAR
    rows, _ = _scene(engine, spoofed)
    names = []
    for p in range(4):
        names.append(str(tmp_path / ("ant%d-%d.iq" % (p, spoofed))))
        rows[p].cpu().numpy().tofile(names[-1])
    argv = ["--prn", ",".join(str(p[0]) for p in PRNS), "--skip", str(SKIP), "--loop-dwells", "20,20", "--time", str(N["search_ms"]),
            "--doppler-search", ",".join("%g" % v for v in N["doppler_search"])]
    for f in names:
        argv += ["--antenna", f]
    out = io.StringIO()
    lines = arrayprompt.run("gps-l1", argv + list(extra) + [names[0], repr(FS), "0"], out)
    assert out.getvalue().splitlines() == lines
    return lines


@pytest.mark.gpu
def test_command_line_prints_vectors_bearings_and_the_verdict(tmp_path, engine):
    el = BC.ring(4)
    extra = ["--step", "5", "--el-min", "5", "--dwell", "50", "--trace", str(tmp_path / "trace.txt")]
    for p in range(4):
        extra += ["--element", ",".join(repr(float(v)) for v in el[p])]
    lines = _run_command(engine, tmp_path, False, extra)
    print("\n".join(lines))
    _, _, ests, _ = _measure(engine, False)
    assert len(lines) == 4
    for k, line in enumerate(lines[:3]):
        f = line.split()
        assert len(f) == 6 + 4 + 6 and f[0] == str(PRNS[k][0]) and (f[1], f[3], f[5], f[10], f[12], f[14]) == ("records", "quality", "steering", "az", "el", "beam")
        assert int(f[2]) == ests[k][0].used and float(f[4]) > 0.95 and 0.9 < float(f[15]) <= 1.0
        back = np.array([arrayfilter._complex(t) for t in f[6:10]])
        assert back.tobytes() == ests[k][0].a_hat.tobytes()                          # measure_tracked's doubles
        g = _cell(float(f[11]), float(f[13]))
        assert _neighbours(g, _cell(*AC.DIRECTIONS[k]))
    f = lines[3].split()
    assert f[:2] == ["coherence", "min"] and f[3] == "max" and f[5:] == ["pairs", "3", "directions", "distinct"] and float(f[4]) < 0.6
    trace = open(str(tmp_path / "trace.txt")).read().splitlines()
    assert len(trace) == sum(-(-ests[k][0].count // 50) for k in range(3)) and trace[0].split()[:4] == [str(PRNS[0][0]), "record", "0", "records"]
    # the spoofed scene: no elements, the verdict alone
    lines = _run_command(engine, tmp_path, True)
    print("\n".join(lines))
    assert len(lines) == 4 and all(len(l.split()) == 10 for l in lines[:3]) and lines[3].endswith("pairs 3 directions alike")
