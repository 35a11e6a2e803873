"""B2b tracking with the chip accumulator on the GPU (csrc/gacq_chiptrack.hip): the command line against the reference's lines and
track-chips.dat, a mixed batch at 69.984 MS/s against the numpy oracle, bit-identity across batching and chunking, records equal to the
template kernel's, the code read back off a strong satellite, and spec validation before any launch."""
import ctypes
import io

import numpy as np
import pytest

import chiptrack_cases as CC
import longtrack_cases as LC
import track_loop_cases as C
from gnss_dsp_tools_amd import _native as nat
from gnss_dsp_tools_amd import acquire, chiptrack, codes, trackloop

GOLDEN = CC.load()
FS = 69.984e6
L = 10230


@pytest.mark.gpu
@pytest.mark.parametrize("case_id", sorted(GOLDEN["cases"]))
def test_cli_reproduces_reference_lines_and_chips(case_id, tmp_path, monkeypatch):
    case = GOLDEN["cases"][case_id]
    path = str(tmp_path / "rec.iq")
    CC.recording(case).tofile(path)
    monkeypatch.chdir(tmp_path)
    out = io.StringIO()
    got, _ = chiptrack.run(case["tracker"], CC.argv_of(case, path), out)
    want = case["stdout_lines"]
    ok, worst, wabs = C.lines_match(got, want)
    assert ok, (case_id, len(got), len(want), worst, wabs, got[:2], want[:2])
    assert out.getvalue().splitlines() == got
    assert open(tmp_path / "track-chips.dat").read().splitlines() == CC.chips_lines(case)


# One recording at 69.984 MS/s: satellites (code, prn, amplitude, frequency Hz, code phase at sample 0) over noise sigma 12
SATS = [("beidou.b2bi", 21, 4.0, 1200.0, 831.15), ("beidou.b2bi", 30, 3.0, -2300.0, 5000.5),
        ("beidou.b2bq", 19, 4.0, 700.0, 9000.25), ("beidou.b2bq", 33, 3.0, -400.0, 2222.75),
        ("beidou.b2bi", 45, 3.0, 3100.0, 7777.0)]
SECONDS = 0.045
# (tracker, prn, doppler, code_offset, carrier_phase)
CHANNELS = [("beidou-b2bi", 21, 1200.0, 831.15, None), ("beidou-b2bi", 30, -2300.0, 5000.5, None),
            ("beidou-b2bq", 19, 700.0, 9000.25, None), ("beidou-b2bq", 33, -400.0, 2222.75, None),
            ("beidou-b2bi", 45, 3100.0, 7777.0, None), ("beidou-b2bq", 33, -400.0, 2222.75, 0.1),
            ("beidou-b2bi", 46, 0.0, 4000.0, None), ("beidou-b2bq", 40, 500.0, 100.5, None)]      # the last two: noise only
DWELLS = (4.0, 6.0)
ACCUM_AFTER = [5, 5, 8, 8, 3, 5, 5, 0]
ORACLE_REL = 1.0e-12


@pytest.fixture(scope="module")
def batch():
    torch = nat.require_torch()
    eng = acquire.default_engine()
    host = LC.synth_many(FS, SECONDS, SATS, 5150, noise=12.0)
    dev = torch.from_numpy(host).to("cuda:%d" % eng.device)
    chans = [trackloop.Channel(n, FS, 0.0, prn, dop, cph, DWELLS, phase) for n, prn, dop, cph, phase in CHANNELS]
    tl = chiptrack.ChipTrackLoop(chans, eng, accum_after=ACCUM_AFTER)
    try:
        recs = tl.run([dev] * len(chans))
        chips = [tl.chips(k) for k in range(len(chans))]
        status = list(tl.status)
    finally:
        tl.close()
    return dict(eng=eng, host=host, dev=dev, chans=chans, recs=recs, chips=chips, status=status)


@pytest.mark.gpu
def test_batch_matches_oracle(batch):
    from concurrent.futures import ThreadPoolExecutor
    from chiptrack_oracle import track as oracle_track

    def one(k):
        spec = chiptrack.chip_channel_spec(batch["chans"][k])
        return oracle_track(spec, codes.chips(chiptrack.CHIP_TRACKERS[CHANNELS[k][0]].code, spec.prn), batch["host"],
                            accum_after=ACCUM_AFTER[k])

    with ThreadPoolExecutor(4) as pool:
        wants = list(pool.map(one, range(len(CHANNELS))))
    assert len(CHANNELS) >= 8
    worst = 0.0
    for k, (want, bins, signs) in enumerate(wants):
        got = batch["recs"][k]
        assert batch["status"][k] == 0 and len(got) == len(want) >= 40, (k, len(got), len(want))
        for f in ("block", "code_cyc", "carrier_cyc", "samp"):
            assert np.array_equal(got[f], [w[f] for w in want]), (k, f)
        for f in ("p_re", "p_im", "carrier_f", "code_f", "early", "prompt", "late", "code_p", "carrier_p"):
            w = np.array([r[f] for r in want], dtype=np.float64)
            dev = np.max(np.abs(got[f] - w)) / max(np.max(np.abs(w)), 1e-300)
            worst = max(worst, dev)
            assert dev <= ORACLE_REL, (k, f, dev)
        # the device took the oracle's sign branch at every accumulated frame ...
        dev_signs = {int(b): (1.0 if p > 0 else -1.0) for b, p in zip(got["block"], got["p_re"]) if b > ACCUM_AFTER[k]}
        assert dev_signs == signs, k
        # ... so every bin is the same sequential sum, bit for bit
        assert batch["chips"][k].tobytes() == bins.tobytes(), (k, np.max(np.abs(batch["chips"][k] - bins)))
    # the comparison is order-sensitive: on the last channel (accumulating from frame 1) a run summed out of order gives other bits
    k = len(CHANNELS) - 1
    spec = chiptrack.chip_channel_spec(batch["chans"][k])
    _, rev, _ = oracle_track(spec, codes.chips(chiptrack.CHIP_TRACKERS[CHANNELS[k][0]].code, spec.prn), batch["host"],
                             accum_after=ACCUM_AFTER[k], bug="runs_out_of_order")
    assert rev.tobytes() != batch["chips"][k].tobytes()
    both = [set(s.values()) for _, _, s in wants]
    assert any(s == {-1.0, 1.0} for s in both)                  # a channel whose sign changes between accumulated frames
    print("max relative deviation from the oracle: %.3g" % worst)


@pytest.mark.gpu
def test_channels_bit_identical_alone_batched_and_in_chunks(batch):
    pick = [0, 3, 6]
    for k in pick:
        tl = chiptrack.ChipTrackLoop([batch["chans"][k]], batch["eng"], accum_after=ACCUM_AFTER[k])
        try:
            alone = tl.run([batch["dev"]])[0]
            assert tl.chips(0).tobytes() == batch["chips"][k].tobytes(), k
        finally:
            tl.close()
        assert alone.tobytes() == batch["recs"][k].tobytes(), k
    chans = [batch["chans"][k] for k in pick]
    tl = chiptrack.ChipTrackLoop(chans, batch["eng"], accum_after=[ACCUM_AFTER[k] for k in pick])
    n = len(batch["host"]) // 2
    cuts = [0, 12345, 400001, 1000007] + list(range(1000007 + 333333, n, 333333)) + [n]
    got = [[] for _ in pick]
    x = batch["dev"]
    try:
        for a, b in zip(cuts[:-1], cuts[1:]):
            # one chunk ends inside an I/Q pair and the next starts with its second byte
            parts = [x[2 * a:2 * b - 1] if a == 12345 else x[2 * a - (a == 400001):2 * b] for _ in pick]
            for i, r in enumerate(tl.feed(parts)):
                got[i].append(r)
        chips = [tl.chips(i) for i in range(len(pick))]
    finally:
        tl.close()
    for i, k in enumerate(pick):
        assert np.concatenate(got[i]).tobytes() == batch["recs"][k].tobytes(), k
        assert chips[i].tobytes() == batch["chips"][k].tobytes(), k


@pytest.mark.gpu
def test_records_equal_the_template_kernel(batch):
    """The accumulator does not perturb the loop: a B2b channel's records equal, bit for bit, those of gacq_track_open with the same
    spec (the template kernel takes any plain code of up to 10240 chips)."""
    torch = nat.require_torch()
    eng = batch["eng"]
    for k in (0, 5):
        specs = (trackloop.TrackSpec * 1)(chiptrack.chip_channel_spec(batch["chans"][k]))
        h = ctypes.c_void_p()
        nat.check(nat.lib.gacq_track_open(eng._ctx, specs, 1, ctypes.byref(h)), eng._ctx)
        try:
            eng.use_torch_stream(torch.device("cuda", eng.device))
            x = batch["dev"]
            ptrs = (ctypes.c_void_p * 1)(x.data_ptr())
            base = np.zeros(1, dtype=np.int64)
            avail = np.full(1, x.numel() // 2, dtype=np.int64)
            cap = 200
            recs = np.zeros((1, cap), dtype=trackloop.RECORD_DTYPE)
            counts = np.zeros(1, dtype=np.int32)
            status = np.zeros(1, dtype=np.int32)
            nat.check(nat.lib.gacq_track_run_dev(h, ptrs, base.ctypes.data_as(ctypes.c_void_p), avail.ctypes.data_as(ctypes.c_void_p),
                                                 cap, recs.ctypes.data_as(ctypes.c_void_p), cap, counts.ctypes.data_as(nat.c_int_p),
                                                 status.ctypes.data_as(nat.c_int_p)), eng._ctx)
        finally:
            nat.lib.gacq_track_close(h)
        assert status[0] == 0 and counts[0] == len(batch["recs"][k])
        assert recs[0, :counts[0]].tobytes() == batch["recs"][k].tobytes(), k


@pytest.mark.gpu
def test_code_recovered_from_a_strong_satellite():
    """sign(real(chips)) is +-(1 - 2c) of the tracked PRN at every one of the 10230 chips."""
    torch = nat.require_torch()
    eng = acquire.default_engine()
    for code, name, prn in (("beidou.b2bi", "beidou-b2bi", 24), ("beidou.b2bq", "beidou-b2bq", 38)):
        # the 900 Hz offset goes in as the carrier offset, not as Doppler: the synthetic code carries no Doppler, and the loop's
        # carrier aiding (carrier_f/118) would otherwise walk the replica off it by 0.8 chip per 100 ms
        host = LC.synth_many(FS, 0.100, [(code, prn, 20.0, 900.0, 1234.5)], 77 + prn, noise=8.0)
        ch = trackloop.Channel(name, FS, 900.0, prn, 0.0, 1234.5, (5.0, 5.0))
        tl = chiptrack.ChipTrackLoop([ch], eng, accum_after=40)
        try:
            recs = tl.run([torch.from_numpy(host).to("cuda:%d" % eng.device)])[0]
            bins = tl.chips(0)
        finally:
            tl.close()
        assert len(recs) >= 98
        want = 1.0 - 2.0 * codes.chips(code, prn).astype(np.float64)
        s = np.sign(bins.real)
        assert np.array_equal(s, want) or np.array_equal(s, -want), (name, int(np.sum(s != want)), int(np.sum(s != -want)))


@pytest.mark.gpu
def test_bad_specs_refused_and_chips_zero_before_threshold(batch):
    eng = batch["eng"]
    good = batch["chans"][0]
    with pytest.raises(KeyError):
        chiptrack.ChipTrackLoop([trackloop.Channel("gps-l1", FS, 0.0, 3, 0.0, 10.0)], eng)
    with pytest.raises(ValueError):
        chiptrack.ChipTrackLoop([], eng)
    h = ctypes.c_void_p()
    thr = np.zeros(2, dtype=np.int64)
    assert nat.lib.gacq_chiptrack_open(eng._ctx, None, 0, thr.ctypes.data_as(ctypes.c_void_p), ctypes.byref(h)) < 0 and not h.value
    gspec = chiptrack.chip_channel_spec(good)
    specs = (trackloop.TrackSpec * 1)(gspec)
    assert nat.lib.gacq_chiptrack_open(eng._ctx, specs, 1, None, ctypes.byref(h)) < 0 and not h.value
    for fields in (dict(kind=1), dict(kind=3), dict(code=b"galileo.e1b", kind=2), dict(code=b"gps.l2cl", kind=5, code_offset=10.0),
                   dict(code=b"glonass.p", glonass=1, prn=0), dict(fs=0.0), dict(fs=float("nan")), dict(code_offset=float(L)),
                   dict(prn=1000), dict(code=b"no.such")):
        bad = chiptrack.chip_channel_spec(good)
        for f, v in fields.items():
            setattr(bad, f, v)
        specs = (trackloop.TrackSpec * 2)(gspec, bad)
        assert nat.lib.gacq_chiptrack_open(eng._ctx, specs, 2, thr.ctypes.data_as(ctypes.c_void_p), ctypes.byref(h)) < 0, fields
        assert not h.value, fields
    # chips(k) stays zero through frame accum_after, and the first accumulated frame makes it non-zero: one frame per launch
    tl = chiptrack.ChipTrackLoop([good], eng, max_records=1, accum_after=12)
    try:
        for frame in range(15):
            got = tl._launch([batch["dev"]], [0])[0]
            assert len(got) == 1 and int(got["block"][0]) == frame
            assert (np.count_nonzero(tl.chips(0)) == 0) == (frame <= 12), frame
    finally:
        tl.close()
