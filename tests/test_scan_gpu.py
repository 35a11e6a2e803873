"""GPU: the batched front-end (csrc/gacq_scan.hip) bit for bit against Engine.frontend_dev on slices of the recording -- going down
and up in rate, the generic filter kernels, several chunks, one window, refusals -- and the scan of a simulated recording against
Engine.acquire_int8 at every file position, against the scene, and through the command line: whole, in pieces of 1.5 windows, and
from a pipe.

Parity of a scan epoch with the single-position path: locations (code phase, Doppler) equal -- they are tie-safe across kernel forms
-- and the metric within 1e-5 relative, the fp32 engines' bar, because a batch may take another kernel form than one epoch."""
import ctypes
import io
import os
import subprocess
import sys

import numpy as np
import pytest

import scan_cases as S
from gnss_dsp_tools_amd import _native as nat
from gnss_dsp_tools_amd import acquire, scan, signals, simulate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MS_PAD = 6
COFFSET = 37500.0


def _recording(n, seed):
    return np.random.default_rng(seed).integers(-128, 128, size=2 * n, dtype=np.int8)


def _single(engine, rec_dev, starts, n_in, fs, ntaps=161):
    """Engine.frontend_dev on every slice, as bytes"""
    return [engine.frontend_dev("gps-l1", rec_dev[2 * s:2 * (s + n_in)], fs, COFFSET, MS_PAD, ntaps).cpu().numpy().tobytes() for s in starts]


def _batch(engine, rec_dev, starts, n_in, fs, ntaps=161):
    out = engine.frontend_batch_dev("gps-l1", rec_dev, starts, n_in, fs, COFFSET, MS_PAD, ntaps).cpu().numpy()
    assert out.shape == (len(starts), MS_PAD * 4096) and out.dtype == np.complex64
    return [row.tobytes() for row in out]


# going down in rate: 10 MS/s -> 4.096 MS/s, seven windows; 0 and 1 share all but one sample, 30001 overlaps 4999, the last one ends
# with the buffer
DOWN_FS, DOWN_N_IN, DOWN_TOTAL = 10.0e6, 60000, 160001
DOWN_STARTS = [0, 1, 4999, 30001, 61111, 90000, DOWN_TOTAL - DOWN_N_IN]


@pytest.fixture(scope="module")
def down(engine):
    torch = nat.require_torch()
    rec = torch.from_numpy(_recording(DOWN_TOTAL, 11)).to("cuda:%d" % engine.device)
    return rec, _single(engine, rec, DOWN_STARTS, DOWN_N_IN, DOWN_FS)


@pytest.mark.gpu
def test_front_end_going_down_in_rate_equals_the_single_call_on_every_slice(engine, down):
    rec, want = down
    assert DOWN_N_IN == int(DOWN_FS * 0.001 * MS_PAD) and DOWN_STARTS[-1] + DOWN_N_IN == rec.numel() // 2
    got = _batch(engine, rec, DOWN_STARTS, DOWN_N_IN, DOWN_FS)
    assert [g == w for g, w in zip(got, want)] == [True] * len(DOWN_STARTS)
    assert len(set(want)) == len(want)                          # the windows differ: a row cannot pass for another


@pytest.mark.gpu
def test_front_end_going_up_in_rate_takes_the_clamp_branch(engine):
    torch = nat.require_torch()
    fs, n_in = 4.0e6, 24000
    step = 1.0 / (4096000.0 / fs)
    t = step * np.arange(MS_PAD * 4096)
    assert n_in == int(fs * 0.001 * MS_PAD) and (t >= n_in - 1).sum() >= 1 and (np.diff(np.floor(t)) == 0).any()      # clamped outputs; outputs that share a pair
    starts = [0, 3, 12001, 40007 - n_in]
    rec = torch.from_numpy(_recording(40007, 12)).to("cuda:%d" % engine.device)
    assert _batch(engine, rec, starts, n_in, fs) == _single(engine, rec, starts, n_in, fs)


@pytest.mark.gpu
@pytest.mark.parametrize("ntaps", [33, 512])
def test_generic_filter_path_equals_the_single_call(engine, down, ntaps):
    rec, _ = down
    starts = [1, 4999, DOWN_TOTAL - DOWN_N_IN]
    engine.set_option("fe_generic", 1)
    try:
        assert _batch(engine, rec, starts, DOWN_N_IN, DOWN_FS, ntaps) == _single(engine, rec, starts, DOWN_N_IN, DOWN_FS, ntaps)
    finally:
        engine.set_option("fe_generic", 0)


@pytest.mark.gpu
def test_generic_kernels_on_the_161_tap_filter_equal_the_fused_form(engine, down):
    rec, want = down
    engine.set_option("fe_generic", 1)
    try:
        assert _batch(engine, rec, DOWN_STARTS[:3], DOWN_N_IN, DOWN_FS) == want[:3]
    finally:
        engine.set_option("fe_generic", 0)


@pytest.mark.gpu
@pytest.mark.parametrize("generic", [0, 1])
def test_result_does_not_depend_on_the_chunking(down, generic):
    """1 MiB of workspace: two windows of y1 (487728 bytes each) fit a chunk of the fused form, one window of the generic form"""
    rec, want = down
    assert 2 * 8 * (DOWN_N_IN + 6 * 161) <= (1 << 20) < 3 * 8 * (DOWN_N_IN + 6 * 161)
    eng = acquire.Engine(rec.device.index, workspace_bytes=1 << 20)
    try:
        eng.set_option("fe_generic", generic)
        assert _batch(eng, rec, DOWN_STARTS, DOWN_N_IN, DOWN_FS) == want
    finally:
        eng.close()


@pytest.mark.gpu
def test_one_window_is_the_single_call(engine, down):
    rec, want = down
    assert _batch(engine, rec, [DOWN_STARTS[3]], DOWN_N_IN, DOWN_FS) == [want[3]]


@pytest.mark.gpu
def test_refusals_with_a_live_context_leave_the_output_untouched(engine, down):
    torch = nat.require_torch()
    rec, _ = down
    n_out = MS_PAD * 4096
    out = torch.full((2, n_out), 7.0 - 3.0j, dtype=torch.complex64, device=rec.device)
    taps = acquire.firwin_hann(161, 1.5e6 / (DOWN_FS / 2))
    good = dict(ctx=engine._ctx, iq=ctypes.c_void_p(rec.data_ptr()), avail=DOWN_TOTAL, starts=np.array([0, 5], dtype=np.int64), nwin=2, n_in=DOWN_N_IN,
                fs=DOWN_FS, off=COFFSET, taps=taps, ntaps=161, fs_out=4096000.0, n_out=n_out, out=ctypes.c_void_p(out.data_ptr()))

    def call(**kw):
        a = dict(good)
        a.update(kw)
        return nat.lib.gacq_frontend_batch_dev(a["ctx"], a["iq"], a["avail"], a["starts"].ctypes.data if a["starts"] is not None else None, a["nwin"],
                                               a["n_in"], a["fs"], a["off"], a["taps"].ctypes.data_as(nat.c_double_p) if a["taps"] is not None else None,
                                               a["ntaps"], a["fs_out"], a["n_out"], a["out"])

    bad_arg = [dict(iq=None), dict(starts=None), dict(taps=None), dict(out=None), dict(nwin=0), dict(nwin=-1), dict(ntaps=0), dict(ntaps=513),
               dict(fs=0.0), dict(fs=-1.0), dict(fs_out=0.0), dict(off=float("nan")), dict(off=float("inf")), dict(n_out=0)]
    short = [dict(n_in=483), dict(starts=np.array([0, -1], dtype=np.int64)), dict(starts=np.array([0, DOWN_TOTAL - DOWN_N_IN + 1], dtype=np.int64)),
             dict(avail=DOWN_N_IN + 4), dict(starts=np.array([0, 2 ** 62], dtype=np.int64))]
    assert [call(**kw) for kw in bad_arg] == [-1] * len(bad_arg)
    assert [call(**kw) for kw in short] == [-6] * len(short)
    assert b"window 1" in nat.lib.gacq_last_error(engine._ctx)
    torch.cuda.synchronize()
    assert bool((out == 7.0 - 3.0j).all())
    assert call(n_in=484, avail=DOWN_TOTAL) == 0                # one sample more than the padding: accepted
    # the scan entry point refuses what the search and the front-end refuse, before it launches anything
    s, idx, _ = engine._plan(signals.get("gps-l1"), [1, 2])
    dop = np.array([0.0, 200.0])
    peaks = torch.full((2, 2, 2), -5.0, dtype=torch.float64, device=rec.device)

    def scan_call(starts=good["starts"], n_out=n_out, blocks=1, items=idx, nd=2):
        return nat.lib.gacq_scan_int8_dev(s._h, good["iq"], DOWN_TOTAL, starts.ctypes.data, 2, DOWN_N_IN, DOWN_FS, COFFSET, taps.ctypes.data_as(nat.c_double_p),
                                          161, n_out, items.ctypes.data_as(nat.c_int_p), 2, dop.ctypes.data_as(nat.c_double_p), nd, None, blocks,
                                          ctypes.c_void_p(peaks.data_ptr()))

    assert scan_call(starts=np.array([0, DOWN_TOTAL], dtype=np.int64)) == -6
    assert scan_call(n_out=4095) == -6                          # fewer samples than one block
    assert scan_call(items=np.array([0, 99], dtype=np.int32)) == -3
    assert scan_call(blocks=-1) == -1
    torch.cuda.synchronize()
    assert bool((peaks == -5.0).all())


# ---- the scan against the single-position path ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def scene(engine):
    rec = simulate.recording(S.SATS, S.FS, S.COFFSET, S.N, S.SEED, S.SIGMA, engine=engine)
    starts, results = scan.scan("gps-l1", rec, S.FS, S.COFFSET, S.MS, S.EVERY, S.ITEMS, S.DOPPLER_SEARCH, engine=engine)
    return rec.cpu().numpy(), starts, results


def _single_records(engine, sig, iq, fs, coffset, ms, items, dop):
    """gacq_acquire_int8 on one slice through the raw ABI: its gacq_result records, idx and d_index included"""
    s, idx, bias = engine._plan(sig, items)
    taps = acquire.firwin_hann(161, sig.fir_cutoff / (fs / 2))
    res = (nat.Result * len(idx))()
    iq = np.ascontiguousarray(iq, dtype=np.int8)
    nat.check_search(nat.lib.gacq_acquire_int8(
        s._h, iq.ctypes.data_as(ctypes.c_void_p), iq.size // 2, float(fs), float(coffset), taps.ctypes.data_as(nat.c_double_p), len(taps),
        (ms + 5) * int(round(sig.fs * 0.001)), idx.ctypes.data_as(nat.c_int_p), len(idx), dop.ctypes.data_as(nat.c_double_p), len(dop),
        bias.ctypes.data_as(nat.c_double_p) if bias is not None else None, max(sig.blocks(ms), 0), res), engine._ctx)
    return np.frombuffer(res, dtype=acquire.RESULT_DTYPE).copy()


def _compare_with_single(engine, name, rec, fs, coffset, ms, items, doppler_search, starts, results):
    sig = signals.get(name)
    dop = np.ascontiguousarray(acquire.doppler_grid(doppler_search), dtype=np.float64)
    n_in = int(fs * 0.001 * (ms + 5))
    assert results.dtype == acquire.RESULT_DTYPE and results.shape == (len(starts), len(items))
    worst = 0.0
    for e, s in enumerate(starts):
        single = _single_records(engine, sig, rec[2 * s:2 * (s + n_in)], fs, coffset, ms, items, dop)
        assert (single["d_index"] >= 0).all() and (single["idx"] >= 0).all()
        assert results[e]["idx"].tolist() == single["idx"].tolist() and results[e]["d_index"].tolist() == single["d_index"].tolist(), (e, results[e], single)
        assert results[e]["code_chips"].tolist() == single["code_chips"].tolist() and results[e]["doppler_hz"].tolist() == single["doppler_hz"].tolist()
        worst = max(worst, float(np.max(np.abs(results[e]["metric"] - single["metric"]) / single["metric"])))
    print("%s: %d epochs x %d items, worst relative metric difference %.3g" % (name, len(starts), len(items), worst))
    assert worst <= 1e-5


@pytest.mark.gpu
def test_scan_equals_acquire_at_every_file_position(engine, scene):
    rec, starts, results = scene
    assert starts.tolist() == scan.window_starts(S.FS, S.EVERY, S.N, S.N_IN).tolist() and len(starts) == S.EPOCHS >= 5
    _compare_with_single(engine, "gps-l1", rec, S.FS, S.COFFSET, S.MS, S.ITEMS, S.DOPPLER_SEARCH, starts, results)


@pytest.mark.gpu
def test_scan_in_several_chunks_gives_the_records_of_one_chunk(engine, scene):
    """1 MiB of workspace holds the front-end output of four windows (7 x 4096 complex64 each): the six epochs go in chunks of 4 and 2"""
    torch = nat.require_torch()
    rec, starts, results = scene
    assert 4 * 8 * (S.MS + 5) * 4096 <= (1 << 20) < 5 * 8 * (S.MS + 5) * 4096 and len(starts) == 6
    eng = acquire.Engine(engine.device, workspace_bytes=1 << 20)
    try:
        s2, r2 = scan.scan("gps-l1", torch.from_numpy(rec).to("cuda:%d" % engine.device), S.FS, S.COFFSET, S.MS, S.EVERY, S.ITEMS,
                           S.DOPPLER_SEARCH, engine=eng)
    finally:
        eng.close()
    assert s2.tolist() == starts.tolist()
    assert r2["idx"].tolist() == results["idx"].tolist() and r2["d_index"].tolist() == results["d_index"].tolist()
    assert float(np.max(np.abs(r2["metric"] - results["metric"]) / results["metric"])) <= 1e-5


@pytest.mark.gpu
def test_scan_of_a_padded_signal_equals_acquire(engine):
    """beidou-b1i: N = 16384, windows of 2n; two overlapping epochs at 10 MS/s"""
    fs, coffset, ms, every = 10.0e6, -250000.0, 1, 2.5
    sats = [simulate.Satellite("beidou-b1i", 8, 3.0, 1210.0, 1500.4, 0.2), simulate.Satellite("beidou-b1i", 21, 2.5, -1890.0, 77.7, 0.6)]
    n_in = int(fs * 0.001 * (ms + 5))
    rec = simulate.recording(sats, fs, coffset, n_in + 25000, S.SEED + 1, S.SIGMA, engine=engine)
    starts, results = scan.scan("beidou-b1i", rec, fs, coffset, ms, every, [8, 13, 21], [-3000.0, 3000.0, 200.0], engine=engine)
    assert starts.tolist() == [0, 25000]
    _compare_with_single(engine, "beidou-b1i", rec.cpu().numpy(), fs, coffset, ms, [8, 13, 21], [-3000.0, 3000.0, 200.0], starts, results)


@pytest.mark.gpu
def test_every_satellite_of_the_scene_is_found_at_every_epoch(scene):
    _, starts, results = scene
    for e, s in enumerate(starts):
        for sat in S.SATS:
            r = results[e, S.ITEMS.index(sat.item)]
            bins, samples = S.found("gps-l1", sat, int(s), (r["metric"], r["code_chips"], r["doppler_hz"]))
            print("epoch %d prn %2d: metric %.2f, Doppler %.2f bins off, code %.2f samples off" % (e, sat.item, r["metric"], bins, samples))
            assert bins <= 1.0 and samples <= 1.0, (e, sat, r)
    noise = results[:, S.ITEMS.index(S.NOISE_PRN)]["metric"]
    assert noise.max() < results[:, [S.ITEMS.index(s.item) for s in S.SATS]]["metric"].min()


def _argv(path, extra=()):
    return ["--prn", ",".join(str(i) for i in S.ITEMS), "--doppler-search", ",".join("%g" % v for v in S.DOPPLER_SEARCH), "--time", str(S.MS),
            "--every", "%g" % S.EVERY] + list(extra) + [str(path), repr(S.FS), repr(S.COFFSET)]


@pytest.mark.gpu
def test_file_pieces_and_pipe_print_the_lines_of_the_whole_scan(engine, scene, tmp_path):
    rec, starts, results = scene
    sig = signals.get("gps-l1")
    want = scan.format_lines(sig, S.ITEMS, starts, results)
    assert len(want) == S.EPOCHS * len(S.ITEMS) and want[len(S.ITEMS)].startswith("epoch 1 start %d prn   5 doppler " % S.N_IN)
    path = tmp_path / "scene.iq"
    path.write_bytes(rec.tobytes())
    with open(path, "rb") as fp:                                 # the file object form of scan(), one piece
        s2, r2 = scan.scan("gps-l1", fp, S.FS, S.COFFSET, S.MS, S.EVERY, S.ITEMS, S.DOPPLER_SEARCH, engine=engine)
    assert scan.format_lines(sig, S.ITEMS, s2, r2) == want
    out = io.StringIO()
    lines = scan.run("gps-l1", _argv(path), out=out, piece_bytes=3 * S.N_IN)      # 1.5 windows: every piece is one window
    assert lines == want and out.getvalue().splitlines() == want
    # ... and a threshold removes exactly the lines below it
    metrics = np.sort(results["metric"].ravel())
    x = float(metrics[len(metrics) // 2])
    kept = scan.run("gps-l1", _argv(path, ["--min-metric", repr(x)]), out=io.StringIO(), piece_bytes=3 * S.N_IN)
    assert kept == [ln for ln, m in zip(want, results["metric"].ravel()) if m >= x] and 0 < len(kept) < len(want)
    # a pipe: the command reads /dev/stdin
    p = subprocess.run([sys.executable, "-m", "gnss_dsp_tools_amd.scan", "gps-l1"] + _argv("/dev/stdin"), input=rec.tobytes(), cwd=ROOT,
                       capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    assert p.stdout.decode().splitlines() == want
