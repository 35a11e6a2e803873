"""Long-code tracking loops on the GPU (csrc/gacq_longtrack.hip): the command line against the reference's lines, a mixed batch at
16 MS/s against the numpy oracle over two outer blocks, bit-identity across batching and chunking, a recording that ends inside an
outer block, spec validation before any launch, and a chip window that cannot hold a sub-block."""
import ctypes
import io

import numpy as np
import pytest

import longtrack_cases as LC
import track_loop_cases as C
from gnss_dsp_tools_amd import _native as nat
from gnss_dsp_tools_amd import acquire, codes, longtrack, track, trackloop

GOLDEN = LC.load()
FS = 16.0e6
L2CL, GLOP = 767250, 5110000


@pytest.mark.gpu
@pytest.mark.parametrize("case_id", sorted(GOLDEN["cases"]))
def test_cli_reproduces_reference_lines(case_id, tmp_path):
    case = GOLDEN["cases"][case_id]
    path = str(tmp_path / "rec.iq")
    LC.recording(case).tofile(path)
    out = io.StringIO()
    got = track.run(case["tracker"], LC.argv_of(case, path), out)
    want = case["stdout_lines"]
    ok, worst, wabs = C.lines_match(got, want)
    assert ok, (case_id, len(got), len(want), worst, wabs, got[:2], want[:2])
    assert out.getvalue().splitlines() == got


# Two band recordings at 16 MS/s; satellites (code, prn, amplitude, frequency Hz, code phase at sample 0).  Code phases sit a little
# below L, so the alignment read is short and two outer blocks fit: 3 s of L2CL, 2 s of GLONASS P.
L2_OFF, L1_OFF = 150000.0, -2000000.0
BANDS = {
    "L2": (3.02, [("gps.l2cl", 3, 6.0, L2_OFF + 900.0, L2CL - 1000.25), ("gps.l2cl", 9, 5.0, L2_OFF - 1300.0, L2CL - 300.5),
                  ("glonass.p", 0, 5.0, -1000000.0 + 437500 * -5 + 500.0, GLOP - 5000.5),
                  ("glonass.p", 0, 5.0, -1000000.0 + 437500 * 2 - 800.0, GLOP - 20000.25)]),
    "L1": (2.02, [("glonass.p", 0, 5.0, L1_OFF + 562500 * -3 + 1100.0, GLOP - 8000.75),
                  ("glonass.p", 0, 5.0, L1_OFF + 562500 * 4 - 400.0, GLOP - 2500.5)]),
}
# (tracker, band, prn | chan, coffset, doppler, code_offset)
CHANNELS = [
    ("gps-l2cl", "L2", 3, L2_OFF, 900.0, L2CL - 1000.25), ("gps-l2cl", "L2", 9, L2_OFF, -1300.0, L2CL - 300.5),
    ("gps-l2cl", "L2", 20, L2_OFF, 0.0, L2CL - 700.0),                                            # noise only
    ("glonass-l2-p", "L2", -5, -1000000.0, 500.0, GLOP - 5000.5), ("glonass-l2-p", "L2", 2, -1000000.0, -800.0, GLOP - 20000.25),
    ("glonass-l1-p", "L1", -3, L1_OFF, 1100.0, GLOP - 8000.75), ("glonass-l1-p", "L1", 4, L1_OFF, -400.0, GLOP - 2500.5),
    ("glonass-l1-p", "L1", 0, L1_OFF, 0.0, GLOP - 4000.0),                                         # noise only
]
DWELLS = (700.0, 800.0)            # L2CL: FLL_WIDE then PLL; GLONASS P: FLL_WIDE then FLL_NARROW; every switch inside the first block
ORACLE = [0, 3, 4, 5]              # one channel per script, both bands, both signs of chan


@pytest.fixture(scope="module")
def batch():
    torch = nat.require_torch()
    eng = acquire.default_engine()
    host = {b: LC.synth_many(FS, sec, sats, 4000 + k) for k, (b, (sec, sats)) in enumerate(sorted(BANDS.items()))}
    dev = {b: torch.from_numpy(v).to("cuda:%d" % eng.device) for b, v in host.items()}
    chans = [trackloop.Channel(n, FS, co, prn, dop, cph, DWELLS) for n, _, prn, co, dop, cph in CHANNELS]
    tl = longtrack.LongTrackLoop(chans, eng)
    try:
        recs = tl.run([dev[b] for _, b, *_ in CHANNELS])
        status = list(tl.status)
    finally:
        tl.close()
    return dict(eng=eng, host=host, dev=dev, chans=chans, recs=recs, status=status)


@pytest.mark.gpu
def test_batch_runs_two_outer_blocks_per_channel(batch):
    assert len(CHANNELS) >= 8
    for (name, *_), r, st in zip(CHANNELS, batch["recs"], batch["status"]):
        assert st == 0, (name, st)
        subs = longtrack.LONG_TRACKERS[name].subs
        assert len(r) >= 2 * subs and len(r) % subs == 0, (name, len(r))         # whole outer blocks: 3 for GLONASS P on the L2 band
        assert np.array_equal(r["block"], np.arange(len(r)))
        assert np.all(np.isfinite(r["carrier_f"])) and np.all(np.isfinite(r["code_p"]))


# Every field of every record of two outer blocks against the oracle, relative to the field's scale over the channel: the two sides
# share every rounding step except the order of the correlator sums and atan / atan2 / hypot (device libm vs. glibc, <= 1 ulp).
ORACLE_REL = 1.0e-12


@pytest.mark.gpu
def test_batch_matches_oracle(batch):
    from concurrent.futures import ThreadPoolExecutor
    from longtrack_oracle import track as oracle_track

    def one(k):
        name, band = CHANNELS[k][:2]
        spec = longtrack.long_channel_spec(batch["chans"][k])
        t = longtrack.LONG_TRACKERS[name]
        return oracle_track(spec, codes.chips(t.code, spec.prn), batch["host"][band], max_records=2 * t.subs)

    with ThreadPoolExecutor(len(ORACLE)) as pool:           # numpy releases the GIL in the per-block work
        wants = list(pool.map(one, ORACLE))
    worst = 0.0
    for k, want in zip(ORACLE, wants):
        name = CHANNELS[k][0]
        got = batch["recs"][k][:len(want)]
        assert len(want) == 2 * longtrack.LONG_TRACKERS[name].subs and len(got) == len(want), (name, len(got), len(want))
        for f in ("block", "code_cyc", "carrier_cyc", "samp"):
            assert np.array_equal(got[f], [w[f] for w in want]), (name, f)
        for f in ("p_re", "p_im", "carrier_f", "code_f", "early", "prompt", "late", "code_p", "carrier_p"):
            w = np.array([r[f] for r in want], dtype=np.float64)
            scale = max(np.max(np.abs(w)), 1e-300)
            dev = np.max(np.abs(got[f] - w)) / scale
            worst = max(worst, dev)
            assert dev <= ORACLE_REL, (name, f, dev)
    print("max relative deviation from the oracle: %.3g" % worst)


@pytest.mark.gpu
def test_channels_bit_identical_alone_batched_and_in_chunks(batch):
    pick = [1, 4, 6]                                        # L2CL, GLONASS L2 P, GLONASS L1 P
    for k in pick:
        tl = longtrack.LongTrackLoop([batch["chans"][k]], batch["eng"])
        try:
            alone = tl.run([batch["dev"][CHANNELS[k][1]]])[0]
        finally:
            tl.close()
        assert alone.tobytes() == batch["recs"][k].tobytes(), CHANNELS[k]
    # uneven chunks that split outer blocks (and one I/Q pair), then 10 ms chunks, fed to a batch of the same channels
    chans = [batch["chans"][k] for k in pick]
    tl = longtrack.LongTrackLoop(chans, batch["eng"])
    n1 = len(batch["host"]["L1"]) // 2
    cuts = [0, 12345, 7 * 10 ** 6 + 1, 23 * 10 ** 6 + 7] + list(range(23 * 10 ** 6 + 7 + 160000, n1, 160000)) + [n1]
    got = [[] for _ in pick]
    try:
        for a, b in zip(cuts[:-1], cuts[1:]):
            parts = []
            for k in pick:
                x = batch["dev"][CHANNELS[k][1]]
                parts.append(x[2 * a:2 * b - 1] if a == 12345 else x[2 * a - (a == 7 * 10 ** 6 + 1):2 * b])
            for i, r in enumerate(tl.feed(parts)):
                got[i].append(r)
        rest = [batch["dev"][CHANNELS[k][1]][2 * n1:] for k in pick]
        for i, r in enumerate(tl.feed(rest)):
            got[i].append(r)
    finally:
        tl.close()
    for i, k in enumerate(pick):
        assert np.concatenate(got[i]).tobytes() == batch["recs"][k].tobytes(), CHANNELS[k]


@pytest.mark.gpu
def test_recording_ending_mid_block_gives_no_partial_block(batch):
    k = 0
    ch = batch["chans"][k]
    x = batch["dev"]["L2"][:2 * int(FS * 2.2)]                # 0.7 s into the second outer block
    tl = longtrack.LongTrackLoop([ch], batch["eng"])
    try:
        recs = tl.run([x])[0]
        st = tl.state(0)
    finally:
        tl.close()
    spec = longtrack.long_channel_spec(ch)
    n0 = int(spec.fs * spec.period * ((L2CL - spec.code_offset) / L2CL))
    assert len(recs) == 1500 and tl.status[0] == 0
    assert recs.tobytes() == batch["recs"][k][:1500].tobytes()
    assert int(st["pos"]) == n0 + int(recs["samp"][-1]) and int(st["pos"]) < x.numel() // 2
    assert int(st["block"]) == 1500


def _raw(ch, **fields):
    spec = longtrack.long_channel_spec(ch)
    for k, v in fields.items():
        setattr(spec, k, v(getattr(spec, k)) if callable(v) else v)
    return spec


@pytest.mark.gpu
def test_bad_specs_rejected_before_launch():
    eng = acquire.default_engine()
    good = trackloop.Channel("gps-l2cl", FS, 0.0, 3, 0.0, 10.0)
    with pytest.raises(KeyError):
        longtrack.LongTrackLoop([trackloop.Channel("gps-l1", FS, 0.0, 3, 0.0, 10.0)], eng)
    with pytest.raises(KeyError):
        trackloop.TrackLoop([good], eng)
    with pytest.raises(ValueError):
        longtrack.LongTrackLoop([], eng)
    h = ctypes.c_void_p()
    assert nat.lib.gacq_longtrack_open(eng._ctx, None, 0, ctypes.byref(h)) == -1 and not h.value
    for bad in (dict(fs=0.0), dict(fs=float("nan")), dict(fs=-FS), dict(code_offset=float(L2CL)), dict(code_offset=-0.5),
                dict(code_offset=float("nan")), dict(prn=1000)):
        ch = trackloop.Channel(**{**good.__dict__, **bad})
        with pytest.raises(nat.GacqError):
            longtrack.LongTrackLoop([good, ch], eng)
    gspec = longtrack.long_channel_spec(good)
    for fields in (dict(subs=1501), dict(subs=0), dict(kind=2), dict(spacing=-0.5), dict(code=b"no.such"), dict(fm=float("inf")),
                   dict(code=b"glonass.p", prn=0, code_offset=float(GLOP))):
        specs = (trackloop.TrackSpec * 2)(gspec, _raw(good, **fields))
        h = ctypes.c_void_p()
        assert nat.lib.gacq_longtrack_open(eng._ctx, specs, 2, ctypes.byref(h)) < 0 and not h.value, fields
    # the template's entry point keeps its limits: the long codes and 1500 calls per block stay out of it
    specs = (trackloop.TrackSpec * 1)(gspec)
    assert nat.lib.gacq_track_open(eng._ctx, specs, 1, ctypes.byref(h)) < 0 and not h.value


@pytest.mark.gpu
def test_window_overflow_stops_the_channel(batch):
    """A code rate far off (40 x the chip rate) makes a sub-block span more chips than the LDS window holds: the channel stops with
    GACQ_TRACK_BAD_WINDOW before it correlates that sub-block, and the channel beside it is untouched."""
    torch = nat.require_torch()
    eng = batch["eng"]
    for k in (0, 5):
        ch = batch["chans"][k]
        specs = (trackloop.TrackSpec * 2)(_raw(ch, chip_rate=lambda r: 40 * r), longtrack.long_channel_spec(ch))
        h = ctypes.c_void_p()
        nat.check(nat.lib.gacq_longtrack_open(eng._ctx, specs, 2, ctypes.byref(h)), eng._ctx)
        try:
            eng.use_torch_stream(torch.device("cuda", eng.device))
            x = batch["dev"][CHANNELS[k][1]]
            ptrs = (ctypes.c_void_p * 2)(x.data_ptr(), x.data_ptr())
            base = np.zeros(2, dtype=np.int64)
            avail = np.full(2, x.numel() // 2, dtype=np.int64)
            cap = 3000
            recs = np.zeros((2, cap), dtype=longtrack.RECORD_DTYPE)
            counts = np.zeros(2, dtype=np.int32)
            status = np.zeros(2, dtype=np.int32)
            for it in range(2):
                nat.check(nat.lib.gacq_longtrack_run_dev(h, ptrs, base.ctypes.data_as(ctypes.c_void_p),
                                                         avail.ctypes.data_as(ctypes.c_void_p), cap, recs.ctypes.data_as(ctypes.c_void_p),
                                                         cap, counts.ctypes.data_as(nat.c_int_p), status.ctypes.data_as(nat.c_int_p)),
                          eng._ctx)
                assert status[0] == 3 and counts[0] == 0, (CHANNELS[k], status, counts)
                if it == 0:
                    assert status[1] == 0 and recs[1, :counts[1]].tobytes() == batch["recs"][k].tobytes(), CHANNELS[k]
            st = np.zeros(1, dtype=longtrack.STATE_DTYPE)
            nat.check(nat.lib.gacq_longtrack_state(h, 0, st.ctypes.data_as(ctypes.c_void_p)), eng._ctx)
            assert int(st[0]["block"]) == 0 and int(st[0]["status"]) == 3
        finally:
            nat.lib.gacq_longtrack_close(h)
        assert longtrack.STATUS[3].startswith("code span")
