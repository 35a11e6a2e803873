"""Tracking loops on the GPU (csrc/gacq_trackloop.hip): the command line against the reference's lines, a mixed batch of channels at
69.984 MS/s against the numpy oracle, bit-identity across batching and chunking, and spec validation before any launch."""
import ctypes
import io

import numpy as np
import pytest

import track_loop_cases as C
from gnss_dsp_tools_amd import _native as nat
from gnss_dsp_tools_amd import acquire, codes, track, trackloop

GOLDEN = C.load()
FS = 69.984e6


@pytest.mark.gpu
@pytest.mark.parametrize("case_id", sorted(GOLDEN["cases"]))
def test_cli_reproduces_reference_lines(case_id):
    case = GOLDEN["cases"][case_id]
    argv = list(case["argv"]) + [C.os.path.join(C.GOLD, case["file"]), repr(case["fs"]), repr(case["coffset"]), str(case["prn"]),
                                 repr(case["doppler"]), repr(case["code_offset"])]
    out = io.StringIO()
    got = track.run(case["tracker"], argv, out)
    want = case["stdout_lines"]
    ok, worst, wabs = C.lines_match(got, want)
    assert ok, (case_id, len(got), len(want), worst, wabs, got[:2], want[:2])
    assert out.getvalue().splitlines() == got


def _recording(seed, nsamp, sats):
    """int8 I/Q: noise (sigma ~12) + plain-code satellites (code, prn, amplitude, frequency Hz, code phase at sample 0)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    i = np.arange(nsamp, dtype=np.float64)
    x = rng.normal(0.0, 12.0, size=(nsamp, 2)).astype(np.float32)
    for code, prn, amp, f, ph0 in sats:
        c = codes.chips(code, prn)
        idx = np.mod(np.floor(ph0 + codes.chip_rate(code) / FS * i).astype(np.int64), len(c))
        ang = np.mod(f / FS * i, 1.0) * (2 * np.pi)
        s = amp * (1.0 - 2.0 * c[idx])
        x[:, 0] += (s * np.cos(ang)).astype(np.float32)
        x[:, 1] += (s * np.sin(ang)).astype(np.float32)
    return np.clip(np.round(x), -127, 127).astype(np.int8).ravel()


SECONDS = 0.305
DWELLS = (4.0, 8.0)
NSAMP = int(FS * SECONDS)
# three band recordings; (tracker, recording, prn | chan, coffset, doppler, code_offset)
BANDS = {
    "L1": [("gps.ca", 3, 6.0, 200000.0 + 1200.0, 100.25), ("gps.ca", 17, 5.0, 200000.0 - 2500.0, 700.5),
           ("galileo.e1b", 11, 5.0, 200000.0 + 800.0, 2000.75), ("glonass.ca", 0, 6.0, -3000000.0 + 562500 * -2 + 500.0, 50.5),
           ("glonass.ca", 0, 6.0, -3000000.0 + 562500 * 4 - 1500.0, 300.25)],
    "L2": [("gps.l2cm", 5, 6.0, 100000.0 + 900.0, 4000.5), ("glonass.ca", 0, 6.0, -2000000.0 + 437500 * 1 + 700.0, 100.5)],
    "L5": [("gps.l5i", 12, 5.0, -300000.0 - 1700.0, 5000.25), ("galileo.e5ai", 19, 5.0, -300000.0 + 2100.0, 9000.5)],
}
CHANNELS = [
    ("gps-l1", "L1", 3, 200000.0, 1200.0, 100.25), ("gps-l1", "L1", 17, 200000.0, -2500.0, 700.5),
    ("galileo-e1b", "L1", 11, 200000.0, 800.0, 2000.75), ("glonass-l1", "L1", -2, -3000000.0, 500.0, 50.5),
    ("glonass-l1", "L1", 4, -3000000.0, -1500.0, 300.25), ("gps-l1", "L1", 25, 200000.0, 300.0, 512.0),         # noise only
    ("gps-l1cp", "L1", 3, 200000.0, 1200.0, 1000.5), ("xona-x1d", "L1", 0, 200000.0, 0.0, 10.5),
    ("gps-l2cm", "L2", 5, 100000.0, 900.0, 4000.5), ("glonass-l2", "L2", 1, -2000000.0, 700.0, 100.5),
    ("gps-l5i", "L5", 12, -300000.0, -1700.0, 5000.25), ("galileo-e5ai", "L5", 19, -300000.0, 2100.0, 9000.5),
    ("gps-l5q", "L5", 12, -300000.0, -1700.0, 5000.25),
]


@pytest.fixture(scope="module")
def batch():
    torch = nat.require_torch()
    eng = acquire.default_engine()
    host = {b: _recording(1000 + k, NSAMP, s) for k, (b, s) in enumerate(sorted(BANDS.items()))}
    dev = {b: torch.from_numpy(v).to("cuda:%d" % eng.device) for b, v in host.items()}
    chans = [trackloop.Channel(n, FS, co, prn, dop, cph, DWELLS) for n, _, prn, co, dop, cph in CHANNELS]
    tl = trackloop.TrackLoop(chans, eng)
    try:
        recs = tl.run([dev[b] for _, b, *_ in CHANNELS])
        status = list(tl.status)
    finally:
        tl.close()
    return dict(eng=eng, host=host, dev=dev, chans=chans, recs=recs, status=status)


@pytest.mark.gpu
def test_batch_runs_every_channel_over_300_ms(batch):
    assert len(batch["chans"]) >= 12
    for (name, *_), r, st in zip(CHANNELS, batch["recs"], batch["status"]):
        t = trackloop.TRACKERS[name]
        assert st == 0, (name, st)
        assert len(r) >= int(0.29 / t.period) * t.subs, (name, len(r))
        assert np.array_equal(r["block"], np.arange(len(r)))
        assert np.all(np.isfinite(r["carrier_f"])) and np.all(np.isfinite(r["code_p"]))


# Each record field against the oracle, relative to the field's scale over the channel's checked records.  The two sides share
# every rounding step except the order of the correlator sums (a tree on the device, a dot product in numpy) and atan / atan2 /
# hypot (device libm vs. glibc, <= 1 ulp); the loops carry those ~1e-16 differences forward.  The first 40 records of all 13 channels
# cover FLL_WIDE, FLL_NARROW and PLL (dwells 4, 8; the 10- and 20-record trackers switch at their outer-block boundaries).
ORACLE_RECORDS = 40
ORACLE_REL = 1.0e-12


@pytest.mark.gpu
def test_batch_matches_oracle(batch):
    from concurrent.futures import ThreadPoolExecutor
    from track_loop_oracle import track as oracle_track

    def one(k):
        name, band = CHANNELS[k][:2]
        spec = trackloop.channel_spec(batch["chans"][k])
        t = trackloop.TRACKERS[name]
        return oracle_track(spec, codes.chips(t.code, spec.prn), batch["host"][band][:2 * int(FS * t.period * (ORACLE_RECORDS / t.subs + 2))],
                            max_records=ORACLE_RECORDS)

    with ThreadPoolExecutor(8) as pool:                    # numpy releases the GIL in the per-block work
        wants = list(pool.map(one, range(len(CHANNELS))))
    worst = 0.0
    for k, (name, *_) in enumerate(CHANNELS):
        want = wants[k]
        got = batch["recs"][k][:len(want)]
        nrec = ORACLE_RECORDS
        assert len(want) == nrec and len(got) == len(want), (name, len(got), len(want))
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
def test_channels_bit_identical_alone_and_in_chunks(batch):
    torch = nat.require_torch()
    pick = [3, 5, 6, 8]                                     # GLONASS, noise only, L1CP (10 sub-blocks), L2CM (20)
    for k in pick:
        band = CHANNELS[k][1]
        tl = trackloop.TrackLoop([batch["chans"][k]], batch["eng"])
        try:
            alone = tl.run([batch["dev"][band]])[0]
        finally:
            tl.close()
        assert alone.tobytes() == batch["recs"][k].tobytes(), CHANNELS[k]
    # uneven chunks, fed to a batch of the same channels
    chans = [batch["chans"][k] for k in pick]
    tl = trackloop.TrackLoop(chans, batch["eng"])
    cuts = [0, 12345, 1000001, 4 * 10 ** 6 + 7, 9 * 10 ** 6 + 1, NSAMP]
    got = [[] for _ in pick]
    try:
        for a, b in zip(cuts[:-1], cuts[1:]):
            parts = [batch["dev"][CHANNELS[k][1]][2 * a:2 * b] for k in pick]
            for i, r in enumerate(tl.feed(parts)):
                got[i].append(r)
    finally:
        tl.close()
    for i, k in enumerate(pick):
        assert np.concatenate(got[i]).tobytes() == batch["recs"][k].tobytes(), CHANNELS[k]
    del torch


@pytest.mark.gpu
def test_bad_specs_rejected_before_launch():
    eng = acquire.default_engine()
    good = trackloop.Channel("gps-l1", FS, 0.0, 3, 0.0, 10.0)
    with pytest.raises(KeyError):
        trackloop.TrackLoop([trackloop.Channel("gps-l2cl", FS, 0.0, 3, 0.0, 10.0)], eng)
    with pytest.raises(ValueError):
        trackloop.TrackLoop([], eng)
    h = ctypes.c_void_p()
    assert nat.lib.gacq_track_open(eng._ctx, None, 0, ctypes.byref(h)) == -1 and not h.value
    for bad in (dict(fs=0.0), dict(fs=float("nan")), dict(fs=-FS), dict(code_offset=1023.0), dict(code_offset=-0.5),
                dict(code_offset=float("nan")), dict(prn=1000)):
        ch = trackloop.Channel(**{**good.__dict__, **bad})
        with pytest.raises(nat.GacqError):
            trackloop.TrackLoop([good, ch], eng)


@pytest.mark.gpu
def test_wipe_off_bit_exact_against_unfused_numpy():
    """The loop's two wipe-offs (gacq_track_debug_mix runs its device helpers) equal the oracle's: separate fp64 products and sums of
    the complex128 table, rounded to complex64 after each mix -- bit for bit, over phases and rates of both signs."""
    from track_loop_oracle import mix
    torch = nat.require_torch()
    eng = acquire.default_engine()
    n = 1 << 20
    iq = np.random.Generator(np.random.PCG64(5)).integers(-128, 128, size=2 * n, dtype=np.int8)
    d_x = torch.from_numpy(iq).to("cuda:%d" % eng.device)
    d_out = torch.empty(n, dtype=torch.complex64, device=d_x.device)
    for fo, po, fc, pc in ((-0.1334, 0.0, -1200.0 / 69.984e6, 0.214), (0.2571234, 0.7731, 3300.5 / 4.0e6, -0.6),
                           (-0.4999, 0.999999, -0.0123456789, 2.5)):
        eng.use_torch_stream(d_x.device)
        nat.check(nat.lib.gacq_track_debug_mix(eng._ctx, ctypes.c_void_p(d_x.data_ptr()), n, fo, po, fc, pc,
                                               ctypes.c_void_p(d_out.data_ptr())), eng._ctx)
        got = d_out.cpu().numpy()
        r, i = mix(iq[0::2].astype(np.float32), iq[1::2].astype(np.float32), fo, po)
        r, i = mix(r, i, fc, pc)
        assert np.array_equal(got.real.view(np.uint32), r.view(np.uint32)) and np.array_equal(got.imag.view(np.uint32), i.view(np.uint32)), \
            (fo, po, fc, pc, int(np.sum(got.real != r) + np.sum(got.imag != i)))
