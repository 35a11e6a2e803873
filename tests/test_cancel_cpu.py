"""CPU: the numpy definition of the cancellation (tests/cancel_oracle.py) read against include/gacq.h on hand-worked samples and on a
noiseless signal of the simulator's oracle, and, of the library, what needs no device: the refusals of gacq_cancel_check, the segments
that segments_from_track builds from the records of the template loop's numpy restatement, the parser and the report."""
import ctypes

import numpy as np
import pytest

import cancel_cases as C
import cancel_oracle as O
import simulate_oracle as SO
import track_loop_cases as TC
from gnss_dsp_tools_amd import _native as nat
from gnss_dsp_tools_amd import cancel, chiptrack, codes, longtrack, trackloop

BAD_ARG, UNKNOWN_CODE, BAD_PRN, SHORT_INPUT, UNSUPPORTED = -1, -2, -3, -6, -9


def test_oracle_on_hand_worked_samples():
    """fs 4, one chip and one turn per four samples: a quarter turn and a quarter chip per sample, everything exact"""
    chips = np.array([0, 1, 1, 0], dtype=np.uint8)
    g = C.seg(10, 8, 1.0, 0.0, 1.0, 3.5)
    assert O.fixed(g, 4.0) == (1 << 62, 0, 1 << 62, (3 << 64) + (1 << 63))
    # code position 3.5, 3.75, 4.0 = chip 0, .., 5.0 = chip 1, ..: chips 3 3 0 0 0 0 1 1 -> + + + + + + - -; the rotation is i^i
    w, turn = O.replica_parts(dict(chips=chips, kind=0), g, 4.0)
    assert w.tolist() == [1, 1, 1, 1, 1, 1, -1, -1] and turn.tolist() == [0, .25, .5, .75, 0, .25, .5, .75]
    r = np.array([1, 1j, -1, -1j, 1, 1j, 1, 1j])
    # BOC(1,1): the second half of a chip is negated -> halves 1 1 0 0 1 1 0 0
    w1, _ = O.replica_parts(dict(chips=chips, kind=1), g, 4.0)
    assert w1.tolist() == [-1, -1, 1, 1, -1, -1, -1, -1]
    # return to zero: [1, 0] keeps the first half, [0, 1] the second
    assert O.replica_parts(dict(chips=chips, kind=4), g, 4.0)[0].tolist() == [0, 0, 1, 1, 0, 0, -1, -1]
    assert O.replica_parts(dict(chips=chips, kind=5), g, 4.0)[0].tolist() == [1, 1, 0, 0, 1, 1, 0, 0]
    # part of a segment: absolute sample indices
    assert O.replica_parts(dict(chips=chips, kind=0), g, 4.0, 15, 17)[0].tolist() == [1, -1]
    x = np.zeros(30, dtype=np.complex128)
    x[10:18] = (2.5 - 1j) * r
    x[3] = 7.0
    sat = dict(chips=chips, kind=0)
    for f32 in (False, True):
        assert abs(O.estimate(sat, g, 4.0, x[2:], 2, f32=f32) - (2.5 - 1j)) < 1e-6
        v = O.evaluate([sat], [C.segs(g)], [np.array([2.5 - 1j])], 4.0, x[2:], 2, 2, 28, f32=f32)
        assert v.dtype == (np.complex64 if f32 else np.complex128) and v[1] == 7.0 and np.max(np.abs(np.delete(v, 1))) < 1e-6
    # only the covered samples change, and the satellites are subtracted one after the other
    v = O.evaluate([sat, sat], [C.segs(g), C.segs(C.seg(12, 2, 0.0, 0.0, 1.0, 0.0))], [np.array([1.0]), np.array([10.0])], 4.0, np.zeros(30), 0, 0, 30)
    want = np.zeros(30, dtype=np.complex128)
    want[10:18] = -r
    want[12:14] -= 10.0
    assert np.max(np.abs(v - want)) < 1e-15
    assert O.to_int8(np.array([-128.0 + 127.5j, 126.5 - 127.5j])).tolist() == [-127, 127, 126, -127]
    assert O.clip_count(np.array([-127, 127, 126, -127, 0, 5], dtype=np.int8)) == 3


@pytest.mark.parametrize("kind,code,prn", [(0, "gps.ca", 5), (2, "galileo.e1b", 11), (3, "gps.l1cp", 4)])
def test_cancelling_a_noiseless_signal_leaves_the_rounding_of_the_input(kind, code, prn):
    fs, amp, n = 4.092e6, 12.0, 3000
    chips = codes.chips(code, prn)
    par = dict(carrier_hz=-2210.0, carrier_phase=0.37, code_rate_hz=1.023e6 - 1.4, code_phase=1001.25)
    x = SO.evaluate([dict(chips=chips, kind=kind, amp=amp, **par)], fs, 0.0, 1, 0, n).astype(np.complex64)
    assert float(np.max(np.abs(x))) > 0.6 * amp
    g = C.seg(0, n, par["carrier_hz"], par["carrier_phase"], par["code_rate_hz"], par["code_phase"])
    v = O.evaluate([dict(chips=chips, kind=kind)], [C.segs(g)], [np.array([amp])], fs, x, 0, 0, n)
    left = float(np.max(np.abs(v)))
    print("kind %d: max |x| %.3f, left %.3g, float32 rounding of the input %.3g" % (kind, np.max(np.abs(x)), left, 2.0 ** -24 * np.max(np.abs(x)) * 2))
    assert left <= 2.0 ** -24 * float(np.max(np.abs(x))) * 2         # a relative 2^-24 per component, and as much again for the fp64 arithmetic
    # ... and the projection finds the amplitude
    assert abs(O.estimate(dict(chips=chips, kind=kind), g, fs, x, 0) - amp) < 1e-6 * amp


# ---- the argument checks: one base call, one change each
def base_call():
    """two satellites, three segments, 200 samples, estimate on"""
    return dict(sats=[["gps.ca", 3, 0, 2], ["galileo.e1b", 1, 2, 1]],
                segs=C.segs(C.seg(0, 100, 1000.0, 0.1, 1.023e6, 5.5, 1.0), C.seg(100, 50, 1001.0, 0.2, 1.023e6, 600.0, 1.0j),
                            C.seg(10, 90, -500.0, 0.0, 1.023e6, 4091.5, 2.0)),
                K=None, fs=4.092e6, estimate=1, in_c=0, in_first=0, in_count=200, out_first=0, n_out=200, out_c=0, null=None, in_off=0, out_off=0)


def _args(d_in, d_out, change):
    c = base_call()
    segs = c["segs"]
    for k, v in change.items():
        if k == "seg":
            i, field, val = v
            segs[field][i] = val
        elif k == "sat":
            i, field, val = v
            c["sats"][i][field] = val
        else:
            c[k] = v
    sats = (cancel.CancelSat * len(c["sats"]))(*[cancel.CancelSat(code=None if s[0] is None else s[0].encode(), prn=s[1], kind=s[2], nseg=s[3], pad=0)
                                                 for s in c["sats"]])
    K = len(c["sats"]) if c["K"] is None else c["K"]
    ptr = dict(sats=ctypes.addressof(sats), segs=segs.ctypes.data, d_in=d_in + c["in_off"], d_out=d_out + c["out_off"])
    if c["null"]:
        ptr[c["null"]] = 0
    keep = (sats, segs)
    return keep, (ctypes.c_void_p(ptr["sats"]), K, ctypes.c_void_p(ptr["segs"]), float(c["fs"]), c["estimate"], ctypes.c_void_p(ptr["d_in"]), c["in_c"],
                  c["in_first"], c["in_count"], c["out_first"], c["n_out"], c["out_c"], ctypes.c_void_p(ptr["d_out"]))


def raw_check(d_in=1 << 20, d_out=1 << 21, **change):
    keep, a = _args(d_in, d_out, change)
    return nat.lib.gacq_cancel_check(*a)


def raw_call(ctx, d_in, d_out, **change):
    keep, a = _args(d_in, d_out, change)
    return nat.lib.gacq_cancel_dev(ctx, *a, None, None)


def bad_calls():
    """(label, expected code, change)"""
    nan, inf = float("nan"), float("inf")
    return [
        ("fs 0", BAD_ARG, dict(fs=0.0)), ("fs nan", BAD_ARG, dict(fs=nan)), ("fs inf", BAD_ARG, dict(fs=inf)), ("fs < 0", BAD_ARG, dict(fs=-1.0)),
        ("carrier nan", BAD_ARG, dict(seg=(1, "carrier_hz", nan))), ("phase inf", BAD_ARG, dict(seg=(0, "carrier_phase", inf))),
        ("amp nan", BAD_ARG, dict(seg=(2, "amp_im", nan))), ("code phase nan", BAD_ARG, dict(seg=(2, "code_phase", nan))),
        ("code rate 0", BAD_ARG, dict(seg=(0, "code_rate_hz", 0.0))), ("code rate < 0", BAD_ARG, dict(seg=(0, "code_rate_hz", -1.0))),
        ("code rate 16 fs", BAD_ARG, dict(seg=(2, "code_rate_hz", 16 * 4.092e6))), ("code rate inf", BAD_ARG, dict(seg=(2, "code_rate_hz", inf))),
        ("code phase < 0", BAD_ARG, dict(seg=(1, "code_phase", -0.5))), ("code phase L", BAD_ARG, dict(seg=(1, "code_phase", 1023.0))),
        ("code phase L of the second code", BAD_ARG, dict(seg=(2, "code_phase", 4092.0))),
        ("kind -1", BAD_ARG, dict(sat=(0, 2, -1))), ("kind 6", BAD_ARG, dict(sat=(1, 2, 6))),
        ("overlap", BAD_ARG, dict(seg=(1, "s0", 99))), ("unsorted", BAD_ARG, dict(seg=(0, "s0", 500))),
        ("n 0", BAD_ARG, dict(seg=(1, "n", 0))), ("n 2^24 + 1", BAD_ARG, dict(seg=(1, "n", (1 << 24) + 1))), ("s0 < 0", BAD_ARG, dict(seg=(0, "s0", -1))),
        ("s0 + n > 2^48", BAD_ARG, dict(seg=(1, "s0", 1 << 48))),
        ("K 0", BAD_ARG, dict(K=0)), ("K 33", BAD_ARG, dict(K=33)), ("nseg < 0", BAD_ARG, dict(sat=(1, 3, -1))),
        ("no code", BAD_ARG, dict(sat=(0, 0, None))),
        ("complex64 input off 8 bytes", BAD_ARG, dict(in_c=1, in_off=4)), ("complex64 output off 8 bytes", BAD_ARG, dict(out_c=1, out_off=4)),
        ("NULL sats", BAD_ARG, dict(null="sats")), ("NULL segs", BAD_ARG, dict(null="segs")), ("NULL d_in", BAD_ARG, dict(null="d_in")),
        ("NULL d_out", BAD_ARG, dict(null="d_out")),
        ("in_first < 0", BAD_ARG, dict(in_first=-1)), ("n_out > 2^48", BAD_ARG, dict(n_out=(1 << 48) + 1)), ("in_count < 0", BAD_ARG, dict(in_count=-1)),
        ("out_first > 2^48", BAD_ARG, dict(out_first=(1 << 48) + 1)),
        ("unknown code", UNKNOWN_CODE, dict(sat=(1, 0, "gps.nope"))), ("unknown PRN", BAD_PRN, dict(sat=(0, 1, 211))),
        ("a code of 767250 chips", UNSUPPORTED, dict(sat=(1, 0, "gps.l2cl"))),
        ("output past the input", SHORT_INPUT, dict(n_out=201)), ("output before the input", SHORT_INPUT, dict(in_first=1, in_count=199)),
        ("estimated segment past the input", SHORT_INPUT, dict(seg=(1, "n", 101))),
        ("estimated segment before the input", SHORT_INPUT, dict(in_first=5, in_count=195, out_first=5, n_out=195)),
    ]


def test_cancel_check_refuses_every_bad_argument_and_accepts_the_unchanged_call():
    for label, code, change in bad_calls():
        rc = raw_check(**change)
        assert rc == code, (label, rc, nat.lib.gacq_last_error(None))
        assert nat.lib.gacq_last_error(None)
        assert nat.lib.gacq_last_error(None).startswith(b"gacq_cancel: "), label   # every message names its own tool
    assert raw_check() == 0
    assert raw_check(n_out=0, in_count=0) == 0                                       # n_out = 0 does nothing
    # without estimate a segment may reach past the input: only the output samples are needed
    assert raw_check(estimate=0, seg=(1, "n", 101)) == 0 and raw_check(estimate=0, in_first=5, in_count=195, out_first=5, n_out=195) == 0
    # a segment that does not touch the output range is not estimated
    assert raw_check(out_first=0, n_out=100, in_count=100) == 0
    # complex64 in and out on 8 bytes, the limits themselves
    assert raw_check(in_c=1, out_c=1) == 0 and raw_check(seg=(1, "n", 1 << 24), estimate=0) == 0
    assert raw_check(seg=(2, "code_rate_hz", 15.9 * 4.092e6)) == 0


# ---- segments from tracking records
def _oracle_records(case_id, max_records=None):
    case = TC.load()["cases"][case_id]
    ch = TC.channel_of(case)
    spec = trackloop.channel_spec(ch)
    chips = codes.chips(trackloop.TRACKERS[ch.name].code, spec.prn)
    iq = TC.recording(case)
    recs, _ = TC.oracle_lines(ch.name, spec, chips, iq, max_records=max_records)
    # the state before the first block, as the loop sets it up from its arguments (track-gps-l1.py:140-150)
    L = len(chips)
    n0 = int(spec.fs * spec.period * ((L - spec.code_offset) / L))
    st = np.zeros(1, dtype=trackloop.STATE_DTYPE)[0]
    st["pos"], st["code_p"], st["code_f"] = n0, spec.code_offset + n0 * spec.rate * L / spec.fs, spec.chip_rate
    st["carrier_p"], st["carrier_f"], st["coffset_phase"] = spec.carrier_phase, spec.doppler, 0.0
    return ch, st, recs, chips, iq


def _circ(a, b, period):
    return abs((a - b + period / 2.0) % period - period / 2.0)


@pytest.mark.parametrize("case_id", ["gps_l1", "galileo_e1b", "glonass_l1"])
def test_segments_from_track_tile_the_timeline_and_fit_the_prompts(case_id):
    ch, st, recs, chips, iq = _oracle_records(case_id)
    t = trackloop.TRACKERS[ch.name]
    L = len(chips)
    segs = cancel.segments_from_track(ch, st, recs)
    assert segs.dtype == cancel.SEG_DTYPE and len(segs) == len(recs) >= 12 and len(recs) % t.subs == 0
    assert int(segs["s0"][0]) == int(st["pos"]) and np.all(segs["n"] > 0) and np.all(segs["amp_re"] == 0) and np.all(segs["amp_im"] == 0)
    assert np.array_equal(segs["s0"][1:], segs["s0"][:-1] + segs["n"][:-1])           # consecutive segments tile the timeline
    if t.cols == 14:                                                                 # the scripts that print samp: the running total
        assert np.array_equal(segs["s0"] + segs["n"] - int(st["pos"]), recs["samp"])
    assert np.all((segs["code_phase"] >= 0) & (segs["code_phase"] < L))
    worst_c = worst_p = 0.0
    for a, b in zip(segs[:-1], segs[1:]):                                            # the loop's own phases are continuous
        worst_c = max(worst_c, _circ(a["carrier_phase"] + a["n"] * a["carrier_hz"] / ch.fs, b["carrier_phase"], 1.0))
        worst_p = max(worst_p, _circ(a["code_phase"] + a["n"] * a["code_rate_hz"] / ch.fs, b["code_phase"], float(L)))
    print("%s: carrier phase steps %.3g turn, code phase steps %.3g chip" % (case_id, worst_c, worst_p))
    assert worst_c <= 1e-9 and worst_p <= 1e-9
    # the segment's replica is what the loop correlated with: sum x conj(r) is the record's prompt up to the loop's table NCOs
    # (two phases floored to 1/1024 turn: 2 x 2 pi / 1024 = 0.0123 rad) and a sample in a thousand across a chip edge
    x = C.as_complex(iq, False)
    sat = dict(chips=chips, kind=t.kind)
    worst = 0.0
    for g, r in zip(segs, recs):
        w, turn = O.replica_parts(sat, g, ch.fs)
        s0, n = int(g["s0"]), int(g["n"])
        c = np.sum(x[s0:s0 + n] * w * np.exp(-2j * np.pi * turn))
        p = complex(r["p_re"], r["p_im"])
        worst = max(worst, abs(c - p) / abs(p))
    print("%s: prompts off by at most %.4f |p| (bound 0.015)" % (case_id, worst))
    assert worst <= 0.015
    # skip leaves the first records out and changes nothing else; a partial outer block at the end is dropped
    assert np.array_equal(cancel.segments_from_track(ch, st, recs, skip=3), segs[3:])
    assert len(cancel.segments_from_track(ch, st, recs[:len(recs) - 1])) == len(recs) - t.subs
    assert len(cancel.segments_from_track(ch, st, recs, skip=len(recs) + 2)) == 0


def test_segments_from_track_refuses_the_other_loop_families():
    st = np.zeros(1, dtype=trackloop.STATE_DTYPE)[0]
    for name in (sorted(longtrack.LONG_TRACKERS)[0], sorted(chiptrack.CHIP_TRACKERS)[0], "no-such-tracker"):
        with pytest.raises(ValueError):
            cancel.segments_from_track(trackloop.Channel(name, 4.0e6, 0.0, 1, 0.0, 0.0), st, [])
    assert cancel.sat_of(trackloop.Channel("glonass-l1", 2.5e6, 0.0, -3, 0.0, 0.0)) == cancel.Sat("glonass.ca", 0, 0)
    assert cancel.sat_of(trackloop.Channel("galileo-e1b", 6.0e6, 0.0, 11, 0.0, 0.0)) == cancel.Sat("galileo.e1b", 11, 2)


def test_command_line_parsing_and_report():
    sig, a = cancel.parse("gps-l1", ["--prn", "5", "--reacquire", "--skip", "40", "--min-metric", "3.5", "--doppler-search", "-5000,5000,200", "in.iq",
                                     "4092000", "0", "out.iq"])
    assert sig.name == "gps-l1" and a.items == [5] and a.reacquire and a.skip == 40 and a.min_metric == 3.5 and a.doppler_search == [-5000.0, 5000.0, 200.0]
    assert (a.input_filename, a.sample_rate, a.carrier_offset, a.output_filename) == ("in.iq", 4092000.0, 0.0, "out.iq")
    sig, a = cancel.parse("gps-l1", ["in.iq", "4092000", "-1000", "-"])
    assert a.output_filename == "-" and not a.reacquire and a.skip == 0 and a.min_metric is None and len(a.items) >= 32 and a.carrier_offset == -1000.0
    for bad in (["--skip", "-1", "a", "1", "0", "b"], ["--nav", "a", "1", "0", "b"], ["--out-dir", "d", "a", "1", "0", "b"], ["a", "1", "0"]):
        with pytest.raises(SystemExit):
            cancel.parse("gps-l1", bad)
    with pytest.raises(ValueError):
        cancel.parse("gps-l2cl", ["a", "1", "0", "b"])                                # no template tracker: refused as handoff refuses it
    line = cancel.report_line([5, 12], 1000, 3, 2.0 * 1000 * 288.0, 2.0 * 1000 * 144.0)
    assert line == "cancelled 5,12 samples 1000 clipped 3 power 24.59 -> 21.58 dB"
    assert cancel.report_line([], 0, 0, 0.0, 0.0) == "cancelled none samples 0 clipped 0 power -inf -> -inf dB"
