"""Acquire-to-track hand-off on the GPU (gnss_dsp_tools_amd/handoff.py): recordings of 250 ms with satellites at off-grid Dopplers and
fractional code phases go through acquisition, the fine search and 200 ms of tracking with no number typed by hand.

The refined values are held to the caps of tests/test_refine_cpu.py (10 Hz, 0.03 chip).  GPS L1 runs at 6 MS/s and BeiDou B1I (a
padded search) at 10 MS/s; the GLONASS L1 recording is sampled at 12.5 MS/s, the lowest round rate above twice the 6 MHz cutoff of
that signal's acquisition front-end (the low-pass design rejects a cutoff at or beyond Nyquist).  Data bits last 20 code periods here
(20 ms, as on GPS L1 C/A): the acquisition integrates 1 ms blocks that are not aligned with the code, and a sign flip in the middle of
every other block moves its Doppler peak by several hundred Hz, which is acquisition's affair and not what these tests are about."""
import io

import numpy as np
import pytest

import handoff_cases as H
from gnss_dsp_tools_amd import acquire, cli, codes, handoff, track, trackloop

MS = 250
DWELLS = (20, 20)


def _code_error(got, want, L):
    return abs((got - want + L / 2.0) % L - L / 2.0)


def _check_channels(name, fs, coffset, sats, noise_item, ms=80, doppler_search=None):
    """handoff + 200 ms of tracking of the satellites' items plus one item that is not in the recording"""
    x = H.recording(31, fs, int(fs * MS * 0.001), coffset, sats)
    items = [s["item"] for s in sats] + [noise_item]
    eng = acquire.default_engine()
    results, refined, loop, x_dev = handoff.handoff(name, x, fs, coffset, items=items, loop_dwells=DWELLS, ms=ms, doppler_search=doppler_search,
                                                    engine=eng)
    try:
        assert [it for it, _ in refined] == items and loop.K == len(items)
        tracker = handoff.tracker_name(name)
        L = codes.code_length(trackloop.TRACKERS[tracker].code)
        for s, (it, r), res in zip(sats, refined, results):
            print("%s %d: acquired doppler %.1f code %.2f -> refined doppler error %.3f Hz, code error %.5f chip, ratio %.1f%s"
                  % (name, it, res[2], res[1], r.doppler - s["doppler"], _code_error(r.code_offset, s["code0"], L), r.ratio, " edge" if r.edge else ""))
        for s, (it, r) in zip(sats, refined):
            assert abs(r.doppler - s["doppler"]) <= 10.0, (it, r)
            assert _code_error(r.code_offset, s["code0"], L) <= 0.03, (it, r)
            assert not r.edge, (it, r)
            assert r.ratio > refined[-1][1].ratio
        recs = loop.run([x_dev] * loop.K)
        assert list(loop.status) == [0] * loop.K
    finally:
        loop.close()
    noise = float(np.mean(recs[-1]["prompt"][:200]))
    for s, r in zip(sats, recs):
        assert len(r) >= 200
        assert abs(r["carrier_f"][199] - s["doppler"]) <= 10.0, (s, r["carrier_f"][199])
        assert np.mean(r["prompt"][:200]) > 3.0 * noise, (s, np.mean(r["prompt"][:200]), noise)
    return recs


@pytest.mark.gpu
def test_gps_l1_three_satellites():
    sats = [dict(tracker="gps-l1", item=7, amp=3.0, bit=20, doppler=1234.5, code0=417.37),
            dict(tracker="gps-l1", item=19, amp=3.0, bit=20, doppler=-1840.2, code0=88.71),
            dict(tracker="gps-l1", item=30, amp=3.0, bit=20, doppler=3071.9, code0=1001.13)]
    _check_channels("gps-l1", 6.0e6, 250000.0, sats, 25)


@pytest.mark.gpu
def test_beidou_b1i_padded_search():
    sats = [dict(tracker="beidou-b1i", item=8, amp=3.0, bit=20, doppler=-1377.3, code0=1500.42),
            dict(tracker="beidou-b1i", item=21, amp=3.0, bit=20, doppler=905.6, code0=77.77)]
    _check_channels("beidou-b1i", 10.0e6, -150000.0, sats, 30)


@pytest.mark.gpu
def test_glonass_l1_channel():
    sats = [dict(tracker="glonass-l1", item=2, amp=3.0, bit=20, doppler=777.7, code0=301.81)]
    _check_channels("glonass-l1", 12.5e6, 100000.0, sats, -4)


@pytest.mark.gpu
def test_command_line(tmp_path):
    fs, coffset = 6.0e6, -250000.0
    sats = [dict(tracker="gps-l1", item=7, amp=3.0, bit=20, doppler=1234.5, code0=417.37),
            dict(tracker="gps-l1", item=19, amp=3.0, bit=20, doppler=-1840.2, code0=88.71),
            dict(tracker="gps-l1", item=30, amp=3.0, bit=20, doppler=3071.9, code0=1001.13)]
    path = str(tmp_path / "l1.bin")
    H.recording(32, fs, int(fs * MS * 0.001), coffset, sats).tofile(path)
    acq_args = ["--prn", "7,19,30", "--doppler-search", "-4000,4000,200", "--time", "40"]
    out = io.StringIO()
    lines = handoff.run("gps-l1", acq_args + ["--loop-dwells", "20,20", "--out-dir", str(tmp_path / "tracks"), path, repr(fs), repr(coffset)], out)
    assert out.getvalue().splitlines() == lines
    want = cli.run("gps-l1", acq_args + [path, repr(fs), repr(coffset)], io.StringIO())
    assert lines[:3] == want                                           # the acquisition lines, byte for byte
    assert len(lines) == 6
    for line, s in zip(lines[3:], sats):
        f = line.split()
        assert f[:3] == ["handoff", "gps-l1", str(s["item"])] and f[3] == "doppler" and f[5] == "code_offset" and f[7] == "ratio"
        assert abs(float(f[4]) - s["doppler"]) <= 10.0 and _code_error(float(f[6]), s["code0"], 1023) <= 0.03
        with open(str(tmp_path / "tracks" / ("track-gps-l1-%d.txt" % s["item"]))) as fp:
            got = fp.read().splitlines()
        alone = track.run("gps-l1", ["--loop-dwells", "20,20", path, repr(fs), repr(coffset), f[2], f[4], f[6]], io.StringIO())
        assert len(got) >= 200 and got == alone, s["item"]


@pytest.mark.gpu
def test_signals_without_a_template_tracker_are_refused(monkeypatch):
    def no_gpu(*a, **k):
        raise AssertionError("GPU work before the refusal")
    monkeypatch.setattr(acquire, "default_engine", no_gpu)
    monkeypatch.setattr(acquire, "Engine", no_gpu)
    x = np.zeros(2 * 600000, dtype=np.int8)
    with pytest.raises(handoff.HandoffError, match="chiptrack"):
        handoff.handoff("beidou-b2bi", x, 6.0e6, 0.0)
    with pytest.raises(handoff.HandoffError, match="prior"):
        handoff.handoff("gps-l2cl", x, 6.0e6, 0.0)
    with pytest.raises(handoff.HandoffError, match="prior"):
        handoff.run("gps-l2cl", ["rec.bin", "6e6", "0"])
