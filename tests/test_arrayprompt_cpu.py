"""CPU: what of the array prompts (gnss_dsp_tools_amd/arrayprompt.py, gacq_aprompt_check) needs no device: the refusals through the raw
ABI, the steering estimate on synthetic prompts (with and without whitening), the Bartlett direction on noiseless vectors, the
coherence of known vectors, the parser and the printed lines."""
import ctypes

import numpy as np
import pytest

import arrayprompt_cases as AC
import bearing_cases as BC
import cancel_cases as C
from gnss_dsp_tools_amd import _native as nat
from gnss_dsp_tools_amd import arrayfilter, arrayprompt, bearing, cancel, scene

BAD_ARG, UNKNOWN_CODE, BAD_PRN, UNSUPPORTED = -1, -2, -3, -9


# ---- the argument checks: one base call, one change each
def base_call():
    """two satellites, three segments, three antennas of 200 samples"""
    return dict(sats=[["gps.ca", 3, 0, 2], ["galileo.e1b", 1, 2, 1]],
                segs=C.segs(C.seg(0, 100, 1000.0, 0.1, 1.023e6, 5.5), C.seg(100, 50, 1001.0, 0.2, 1.023e6, 600.0), C.seg(10, 90, -500.0, 0.0, 1.023e6, 4091.5)),
                K=None, fs=4.092e6, rows=[1 << 20, 1 << 21, (1 << 22) + 3], antennas=None, in_c=0, in_first=0, in_count=200, null=None)


def raw_args(rows=None, **change):
    c = base_call()
    if rows is not None:
        c["rows"] = list(rows)
    segs = c["segs"]
    for k, v in change.items():
        if k == "seg":
            segs[v[1]][v[0]] = v[2]
        elif k == "sat":
            c["sats"][v[0]][v[1]] = v[2]
        elif k == "row":
            c["rows"][v[0]] = v[1]
        else:
            c[k] = v
    sats = (cancel.CancelSat * len(c["sats"]))(*[cancel.CancelSat(code=None if s[0] is None else s[0].encode(), prn=s[1], kind=s[2], nseg=s[3], pad=0)
                                                 for s in c["sats"]])
    ptrs = (ctypes.c_void_p * max(len(c["rows"]), 1))(*c["rows"])
    ptr = dict(sats=ctypes.addressof(sats), segs=segs.ctypes.data, d_in=ctypes.addressof(ptrs))
    if c["null"]:
        ptr[c["null"]] = 0
    M = len(c["rows"]) if c["antennas"] is None else c["antennas"]
    return (sats, segs, ptrs), (ctypes.c_void_p(ptr["sats"]), len(c["sats"]) if c["K"] is None else c["K"], ctypes.c_void_p(ptr["segs"]), float(c["fs"]),
                                ctypes.c_void_p(ptr["d_in"]), M, c["in_c"], c["in_first"], c["in_count"])


def raw_check(**change):
    keep, a = raw_args(**change)
    return nat.lib.gacq_aprompt_check(*a)


def bad_calls():
    """(label, expected code, change)"""
    nan, inf = float("nan"), float("inf")
    return [
        ("antennas 0", BAD_ARG, dict(antennas=0)), ("antennas 9", BAD_ARG, dict(rows=[1 << 20] * 9)), ("antennas -1", BAD_ARG, dict(antennas=-1)),
        ("NULL row", BAD_ARG, dict(row=(1, 0))), ("NULL first row", BAD_ARG, dict(row=(0, 0))),
        ("complex64 row off 8 bytes", BAD_ARG, dict(in_c=1)), ("complex64 row off 4 bytes", BAD_ARG, dict(in_c=1, row=(2, (1 << 22) + 4))),
        ("fs 0", BAD_ARG, dict(fs=0.0)), ("fs nan", BAD_ARG, dict(fs=nan)), ("fs inf", BAD_ARG, dict(fs=inf)),
        ("carrier nan", BAD_ARG, dict(seg=(1, "carrier_hz", nan))), ("phase inf", BAD_ARG, dict(seg=(0, "carrier_phase", inf))),
        ("code phase nan", BAD_ARG, dict(seg=(2, "code_phase", nan))), ("code rate inf", BAD_ARG, dict(seg=(2, "code_rate_hz", inf))),
        ("code rate 0", BAD_ARG, dict(seg=(0, "code_rate_hz", 0.0))), ("code rate 16 fs", BAD_ARG, dict(seg=(2, "code_rate_hz", 16 * 4.092e6))),
        ("code phase L", BAD_ARG, dict(seg=(1, "code_phase", 1023.0))), ("kind 6", BAD_ARG, dict(sat=(1, 2, 6))),
        ("overlap", BAD_ARG, dict(seg=(1, "s0", 99))), ("unsorted", BAD_ARG, dict(seg=(0, "s0", 500))),
        ("n 0", BAD_ARG, dict(seg=(1, "n", 0))), ("n 2^24 + 1", BAD_ARG, dict(seg=(1, "n", (1 << 24) + 1))), ("s0 < 0", BAD_ARG, dict(seg=(0, "s0", -1))),
        ("K 0", BAD_ARG, dict(K=0)), ("K 33", BAD_ARG, dict(K=33)), ("nseg < 0", BAD_ARG, dict(sat=(1, 3, -1))), ("no code", BAD_ARG, dict(sat=(0, 0, None))),
        ("NULL sats", BAD_ARG, dict(null="sats")), ("NULL segs", BAD_ARG, dict(null="segs")), ("NULL d_in", BAD_ARG, dict(null="d_in")),
        ("in_first < 0", BAD_ARG, dict(in_first=-1)), ("in_count > 2^48", BAD_ARG, dict(in_count=(1 << 48) + 1)),
        ("unknown code", UNKNOWN_CODE, dict(sat=(1, 0, "gps.nope"))), ("unknown PRN", BAD_PRN, dict(sat=(0, 1, 211))),
        ("a code of 767250 chips", UNSUPPORTED, dict(sat=(1, 0, "gps.l2cl"))),
    ]


def test_aprompt_check_refuses_every_bad_argument_and_accepts_the_unchanged_call():
    for label, code, change in bad_calls():
        rc = raw_check(**change)
        assert rc == code, (label, rc, nat.lib.gacq_last_error(None))
        assert nat.lib.gacq_last_error(None).startswith(b"gacq_aprompt: "), label  # every message names its own tool
    assert raw_check() == 0
    for M in range(1, 9):
        assert raw_check(rows=[(1 << 20) + 8 * p for p in range(M)], in_c=1) == 0    # 1..8 antennas, complex64 on 8 bytes
    assert raw_check(rows=[1 << 20, 1 << 20]) == 0                                   # two antennas may share a pointer
    # the amplitudes are not looked at; a segment outside the input is no error
    assert raw_check(seg=(2, "amp_im", float("nan"))) == 0 and raw_check(seg=(0, "amp_re", float("inf"))) == 0
    assert raw_check(in_first=50, in_count=20) == 0 and raw_check(in_count=0) == 0
    assert raw_check(seg=(1, "n", 1 << 24)) == 0


# ---- steering_estimate
def _true(az=40.0, el=60.0, M=4):
    return scene.steering(BC.ring(M), az, el)


def test_steering_estimate_on_synthetic_prompts_over_fifty_seeds():
    a = _true()
    unit = AC.unit()
    worst, qmin = 0.0, 1.0
    for seed in range(50):
        P, b, phi = AC.synthetic(seed, a)
        for ref in (0, 2):
            a_hat, q, used = arrayprompt.steering_estimate(P, ref=ref)
            assert used == AC.D and a_hat.shape == (4,) and a_hat[ref] == 1.0
            worst = max(worst, float(np.max(np.abs(a_hat - a / a[ref]))) / unit)
            qmin = min(qmin, q)
    print("50 seeds, D %d, |s| / sigma_c %g: worst entry %.3f of the bound %.4f; smallest quality %.4f" % (AC.D, AC.RATIO, worst, unit, qmin))
    assert worst <= 1.0 and qmin > 0.99


def test_steering_estimate_ignores_bits_and_segment_phases_drops_nan_rows_and_rescales():
    a = _true()
    P, b, phi = AC.synthetic(7, a)
    a0, q0, _ = arrayprompt.steering_estimate(P)
    r = np.random.Generator(np.random.PCG64(99))
    for Q in (-P, P * np.exp(1j * r.uniform(0.0, 2.0 * np.pi, AC.D))[:, None], P * r.choice([-1.0, 1.0], AC.D)[:, None]):
        a1, q1, _ = arrayprompt.steering_estimate(Q)
        assert np.max(np.abs(a1 - a0)) < 1e-12 and abs(q1 - q0) < 1e-12
    holes = P.copy()
    holes[3, 1] = np.nan
    holes[50] = np.nan + 1j * np.nan
    holes[77, 0] = complex(1.0, np.nan)
    a2, q2, used = arrayprompt.steering_estimate(holes)
    a3, q3, _ = arrayprompt.steering_estimate(np.delete(P, [3, 50, 77], axis=0))
    assert used == AC.D - 3 and np.array_equal(a2, a3) and q2 == q3
    a4, _, _ = arrayprompt.steering_estimate(P, ref=2)
    assert a4[2] == 1.0 and np.max(np.abs(a4 - a0 / a0[2])) < 1e-12
    none, qn, used = arrayprompt.steering_estimate(np.full((5, 4), np.nan + 0j))
    assert used == 0 and np.isnan(none).all() and np.isnan(qn)
    for bad in (dict(ref=4), dict(ref=-1), dict(noise_cov=np.eye(3))):
        with pytest.raises(ValueError):
            arrayprompt.steering_estimate(P, **bad)
    # the vectors of several dwells
    est = arrayprompt.dwell_estimates(P, 30)
    assert [(e.first, e.count, e.used) for e in est] == [(0, 30, 30), (30, 30, 30), (60, 30, 30), (90, 10, 10)]
    assert np.array_equal(est[1].a_hat, arrayprompt.steering_estimate(P[30:60])[0])
    assert len(arrayprompt.dwell_estimates(P)) == 1 and arrayprompt.dwell_estimates(P)[0].used == AC.D


WHITE_D = 1000


def test_whitening_keeps_the_estimate_off_a_jammer():
    """A rank-one jammer term z_g j with three times the signal's power per segment.  Without noise_cov the largest eigenvalue is the
    jammer's (3 |s|^2 |j|^2 against |s|^2 |a|^2): the estimate is the jammer's vector.  With the true covariance the estimate is
    a + eps j, where eps is the mean of D terms z_g / (c_g s) of variance 3 each: E |eps|^2 = 3 / D, and for |a| = |j| the coherence
    with a is 1 - |eps|^2 (1 - rho^2) / 2 with rho the coherence of a and j.  No estimator does better: the jammer hides that
    component of a in every segment.  |eps|^2 is exponentially distributed, so at D = 100 (mean 0.03) the coherence is above 0.99 in
    one seed of two, whatever the code does; the printed D = 100 figures show that.  The assertions use D = 1000: mean 0.003, and
    |eps|^2 > 0.02 has probability exp(-6.7) = 0.0013 per seed."""
    a, j = _true(40.0, 60.0), _true(160.0, 35.0)
    coh = lambda u, v: float(arrayprompt.coherence([u, v])[0, 1])
    assert coh(a, j) < 0.5                                                           # the two directions are far apart on this array
    N = 2.0 * np.eye(4) + 3.0 * AC.RATIO ** 2 * np.outer(j, j.conj())               # the noise's true covariance: sigma_c = 1 per component
    for seed in range(100, 105):
        for D in (AC.D, WHITE_D):
            P, _, _ = AC.synthetic(seed, a, jammer=j, jam_power=3.0, D=D)
            plain, _, _ = arrayprompt.steering_estimate(P)
            white, _, _ = arrayprompt.steering_estimate(P, noise_cov=N)
            print("seed %d D %4d: plain estimate, coherence with the jammer %.4f and with a %.4f; whitened, with a %.6f"
                  % (seed, D, coh(plain, j), coh(plain, a), coh(white, a)))
        assert coh(plain, j) > 0.9 and coh(plain, a) < 0.7
        assert coh(white, a) > 0.99 and white[0] == 1.0


# ---- direction and coherence
@pytest.mark.parametrize("M", [4, 5, 8])
def test_direction_finds_the_cell_of_a_noiseless_vector(M):
    cells = bearing.grid(5.0, 5.0)
    for az, el in AC.DIRECTIONS:
        want = int(np.flatnonzero((cells[:, 0] == az) & (cells[:, 1] == el))[0])
        g, gaz, gel, v = arrayprompt.direction(scene.steering(BC.ring(M), az, el), BC.ring(M), cells)
        assert (g, gaz, gel) == (want, az, el) and abs(v - 1.0) <= 1e-12
        g2, _, _, v2 = arrayprompt.direction((0.3 - 2.0j) * scene.steering(BC.ring(M), az, el), BC.ring(M), cells)      # any scale
        assert g2 == want and abs(v2 - 1.0) <= 1e-12
    # ties go to the lowest index: a grid that names a cell twice
    twice = np.array([[280.0, 50.0], [40.0, 60.0], [40.0, 60.0], [160.0, 35.0], [40.0, 60.0]])
    assert arrayprompt.direction(scene.steering(BC.ring(M), 40.0, 60.0), BC.ring(M), twice)[:3] == (1, 40.0, 60.0)
    with pytest.raises(ValueError):
        arrayprompt.direction(np.ones(M + 1), BC.ring(M), cells)


def test_coherence_of_the_three_directions():
    vs = [scene.steering(BC.ring(4), az, el) for az, el in AC.DIRECTIONS]
    c = arrayprompt.coherence(vs)
    assert c.shape == (3, 3) and np.allclose(c, c.T) and np.max(np.abs(np.diag(c) - 1.0)) < 1e-15
    print("coherence on ring(4): %.4f %.4f %.4f" % (c[0, 1], c[0, 2], c[1, 2]))
    assert sorted(float(v) for v in (c[0, 1], c[0, 2], c[1, 2])) == pytest.approx([0.065, 0.334, 0.434], abs=1e-3)
    same = arrayprompt.coherence([vs[0], 2.0j * vs[0]])
    assert np.max(np.abs(same - 1.0)) < 1e-15


# ---- command line
def test_command_line_parsing_and_refusals():
    sig, a = arrayprompt.parse("gps-l1", ["--prn", "5,9", "--skip", "50", "--dwell", "25", "--ref", "1", "--antenna", "a0", "--antenna", "a1",
                                          "--element", "0,0,0", "--element", "-0.5,0.25,0", "--step", "10", "--el-min", "5", "--alike", "0.8", "--trace", "t.txt",
                                          "--doppler-search", "-5000,5000,200", "a0", "4092000", "-1000"])
    assert sig.name == "gps-l1" and a.items == [5, 9] and (a.skip, a.dwell, a.ref, a.alike, a.trace) == (50, 25, 1, 0.8, "t.txt")
    assert a.antenna == ["a0", "a1"] and a.element == [[0.0, 0.0, 0.0], [-0.5, 0.25, 0.0]] and np.array_equal(a.cells, bearing.grid(10.0, 5.0))
    assert (a.input_filename, a.sample_rate, a.carrier_offset) == ("a0", 4092000.0, -1000.0) and a.doppler_search == [-5000.0, 5000.0, 200.0]
    sig, a = arrayprompt.parse("gps-l1", ["--antenna", "x", "nulled.iq", "4092000", "0"])
    assert a.antenna == ["x"] and a.cells is None and (a.skip, a.dwell, a.ref, a.alike) == (0, None, 0, 0.9) and len(a.items) >= 32
    tail = ["t", "1", "0"]
    for bad in (tail, ["--antenna", "a", "--nav"] + tail, ["--antenna", "a", "--out-dir", "d"] + tail, ["--antenna", "a", "--skip", "-1"] + tail,
                ["--antenna", "a", "--dwell", "0"] + tail, ["--antenna", "a", "--ref", "1"] + tail, ["--antenna", "a", "--alike", "1.5"] + tail,
                ["--antenna", "a", "--antenna", "b", "--element", "0,0,0"] + tail, ["--antenna", "a", "--element", "0,0"] + tail,
                ["--antenna", "a", "--element", "0,0,0", "--step", "0"] + tail, ["--antenna", "a"] * 9 + tail, ["--antenna", "a", "t", "1"]):
        with pytest.raises(SystemExit):
            arrayprompt.parse("gps-l1", bad)
    with pytest.raises(ValueError):
        arrayprompt.parse("gps-l2cl", ["--antenna", "a"] + tail)                      # no template tracker: refused as handoff refuses it


def test_printed_steering_entries_parse_back_to_the_same_doubles():
    r = np.random.Generator(np.random.PCG64(5))
    a = (r.normal(size=6) + 1j * r.normal(size=6)) * 10.0 ** r.integers(-12, 12, 6)
    a[0] = 1.0
    a[1] = complex(-0.0, 1.0 / 3.0)
    est = arrayprompt.Estimate(0, 40, a, 0.98765, 38)
    line = arrayprompt.item_line(21, est)
    f = line.split()
    assert f[:6] == ["21", "records", "38", "quality", "0.9877", "steering"] and len(f) == 6 + 6
    back = np.array([arrayfilter._complex(t) for t in f[6:]])
    assert back.tobytes() == a.tobytes()                                              # the same doubles, the sign of zero included
    el = BC.ring(4)
    a4 = scene.steering(el, 160.0, 35.0)
    line = arrayprompt.item_line(9, arrayprompt.Estimate(0, 10, a4 / a4[0], 1.0, 10), el, bearing.grid(5.0, 5.0))
    assert line.split()[-6:] == ["az", "160", "el", "35", "beam", "1.0000"]
    t = arrayprompt.trace_line(9, arrayprompt.Estimate(50, 25, a4, 0.5, 24)).split()
    assert t[:8] == ["9", "record", "50", "records", "24", "quality", "0.5000", "steering"] and len(t) == 12
    vs = [scene.steering(el, az, e) for az, e in AC.DIRECTIONS]
    assert arrayprompt.coherence_line(vs) == "coherence min 0.0647 max 0.4338 pairs 3 directions distinct"
    assert arrayprompt.coherence_line([vs[0], vs[0] * 1j, vs[0]]) == "coherence min 1.0000 max 1.0000 pairs 3 directions alike"
    assert arrayprompt.coherence_line(vs, alike=0.05).endswith("directions alike")
    assert arrayprompt.coherence_line(vs[:1]) == "coherence none" and arrayprompt.coherence_line([]) == "coherence none"
