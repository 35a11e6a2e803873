"""GPU: the mitigation kernels (csrc/gacq_mitigate.hip) against the fp64 definition of tests/mitigate_oracle.py.  Values of the
excision path are held to four times the deviation of a float32 evaluation of the same definition, relative to max |y| of the case;
every decision -- the per-frame zeroed-bin counts and the three totals -- and the whole blank-only path are compared exactly; the
int8 output is the rounding of the device's own complex64 output; device against device, the output does not depend on how the
recording is cut into calls or chunks.  Then the interference scene through the engine's search, a 250 ms recording through
mitigation, hand-off and tracking, and the command line in pieces and in a pipe into scan."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest

import mitigate_cases as C
import mitigate_oracle as O
from gnss_dsp_tools_amd import _native as nat
from gnss_dsp_tools_amd import codes, handoff, mitigate, scan, signals, simulate, trackloop
from oracle import codes_oracle
from test_mitigate_cpu import bad_calls, raw_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _mcfg(o):
    return mitigate.Config(blank=o.blank, hold=o.hold, nfft=o.nfft, ratio=o.ratio if o.nfft else None, guard=o.guard)


def _run_both(engine, ocfg, data, gain, in_c64, in_first, out_first, n_out):
    cfg = _mcfg(ocfg)
    c, sc = mitigate.apply(engine, cfg, data, gain, in_first, out_first, n_out, "complex64", True, in_c64)
    i, si = mitigate.apply(engine, cfg, data, gain, in_first, out_first, n_out, "int8", True, in_c64)
    c, i = c.cpu().numpy(), i.cpu().numpy()
    assert (sc.blanked, sc.frames, sc.bins) == (si.blanked, si.frames, si.bins) and np.array_equal(sc.frame_bins, si.frame_bins)
    assert c.dtype == np.complex64 and i.dtype == np.int8 and c.shape == (n_out,) and i.shape == (2 * n_out,)
    return c, i, sc


def _hold_to_the_oracle(label, c, i, st, ref, bound, top):
    """decisions exactly, values within bound * top, int8 by the two rules"""
    assert (st.blanked, st.frames, st.bins) == (ref.blanked, ref.frames, ref.bins), (label, vars(st))
    assert np.array_equal(st.frame_bins, ref.frame_bins), label
    dev = float(np.max(np.abs(c.astype(np.complex128) - ref.y))) / top if top > 0 else float(np.max(np.abs(c)))
    print("%s: device deviation %.3g of max |y| = %.3g, bound %.3g (float32 evaluation %.3g)" % (label, dev, top, bound, bound / 4.0))
    assert dev <= bound, (label, dev, bound)
    assert np.array_equal(i, O.to_int8(c)), label
    d = i.astype(np.int32) - ref.i8.astype(np.int32)
    assert np.max(np.abs(d)) <= 1, label
    v = ref.y.view(np.float64)[d != 0]                                   # the oracle's scaled values where a byte differs
    assert np.all(np.abs(np.abs(v - np.floor(v)) - 0.5) <= bound * top), label


@pytest.mark.gpu
def test_the_tile_of_the_cases_is_the_kernels():
    assert [nat.lib.gacq_mitigate_tile(n) for n in (64, 128, 256, 512, 1024, 2048, 4096)] == [C.TILE] * 7


@pytest.mark.gpu
@pytest.mark.parametrize("c", C.EXCISE_CASES, ids=lambda c: c.name)
def test_excision_alone_matches_the_oracle(engine, c):
    data, in_first, out_first, n_out = C.case_input(c)
    ref, bound, top = C.case_reference(c)
    got_c, got_i, st = _run_both(engine, C.cfg_of(c), data, C.GAIN, c.in_complex64, in_first, out_first, n_out)
    assert ref.bins > 0 and ref.blanked == 0
    _hold_to_the_oracle(c.name, got_c, got_i, st, ref, bound, top)


@pytest.mark.gpu
@pytest.mark.parametrize("nfft,in_c64", [(64, False), (128, True), (1024, False), (4096, True)])
def test_identity_and_silence(engine, nfft, in_c64):
    h = nfft // 2
    ocfg = O.config(nfft=nfft, ratio=1e30, guard=2)
    n_out = (C.TILE + 2) * h
    data = C.tones(O.needed(ocfg, 0, n_out)[1] + 1, nfft, C.SEED + 5, in_c64)
    ref = O.evaluate(ocfg, data, C.GAIN, in_c64, 0, 0, n_out)
    f32 = O.evaluate(ocfg, data, C.GAIN, in_c64, 0, 0, n_out, precision="f32")
    x, _ = O.samples(data, in_c64)
    top = float(np.max(np.abs(ref.y)))
    bound = 4.0 * float(np.max(np.abs(f32.y - ref.y))) / top
    assert np.max(np.abs(ref.y - x[:n_out] * np.float64(np.float32(C.GAIN)))) <= 1e-12 * top       # the oracle is the identity here
    got_c, got_i, st = _run_both(engine, ocfg, data, C.GAIN, in_c64, 0, 0, n_out)
    assert (st.blanked, st.bins, st.frames) == (0, 0, n_out // h) and not st.frame_bins.any()
    _hold_to_the_oracle("identity N=%d" % nfft, got_c, got_i, st, ref, bound, top)
    zeros = np.zeros_like(data)
    got_c, got_i, st = _run_both(engine, O.config(nfft=nfft, ratio=1.5, guard=2), zeros, C.GAIN, in_c64, 0, 0, n_out)
    assert not got_c.any() and not got_i.any() and (st.blanked, st.bins, st.frames) == (0, 0, n_out // h)


@pytest.mark.gpu
@pytest.mark.parametrize("in_c64", [False, True])
def test_blanking_alone_is_the_oracle_bit_for_bit(engine, in_c64):
    for n in C.BLANK_SIZES:
        for hold in C.BLANK_HOLDS:
            ocfg = O.config(blank=C.BLANK_THR, hold=hold, nfft=0)
            n_in = n + hold
            data = C.pulses(n_in, C.SEED + hold, in_c64, extra=(n - 1, n // 2))
            if in_c64 and n >= 9:
                data[3], data[n - 2] = complex(np.nan, 1.0), complex(5.0, -np.inf)
            ref = O.evaluate(ocfg, data, C.GAIN, in_c64, 0, 0, n)
            got_c, got_i, st = _run_both(engine, ocfg, data, C.GAIN, in_c64, 0, 0, n)
            label = ("blank", in_c64, n, hold)
            assert ref.blanked > 0 and (st.blanked, st.frames, st.bins) == (ref.blanked, 0, 0), label
            assert np.array_equal(got_c, ref.c64) and np.array_equal(got_i, ref.i8) and np.array_equal(got_i, O.to_int8(got_c)), label
    # outputs that start inside the data: the hold reaches back over samples before out_first
    data = C.pulses(5000, C.SEED + 9, in_c64, extra=(99, 100, 2147, 2148))
    ocfg = O.config(blank=C.BLANK_THR, hold=64, nfft=0)
    ref = O.evaluate(ocfg, data, C.GAIN, in_c64, 0, 101, 4099)
    got_c, got_i, st = _run_both(engine, ocfg, data, C.GAIN, in_c64, 0, 101, 4099)
    assert st.blanked == ref.blanked and np.array_equal(got_c, ref.c64) and np.array_equal(got_i, ref.i8)


@pytest.mark.gpu
@pytest.mark.parametrize("in_c64", [False, True])
def test_blanking_with_misaligned_buffers(engine, in_c64):
    """the int8 input and output one byte into an allocation, the complex64 ones one element in (8 but not 16 bytes)"""
    torch = nat.require_torch()
    dev = "cuda:%d" % engine.device
    n, hold = 4099, 2
    ocfg = O.config(blank=C.BLANK_THR, hold=hold, nfft=0)
    data = C.pulses(n + hold, C.SEED + 11, in_c64)
    ref = O.evaluate(ocfg, data, C.GAIN, in_c64, 0, 0, n)
    unit = 8 if in_c64 else 1
    raw = np.frombuffer(data.tobytes(), dtype=np.uint8)
    buf = torch.zeros(len(raw) + unit, dtype=torch.uint8, device=dev)
    buf[unit:] = torch.from_numpy(raw.copy()).to(dev)
    engine.use_torch_stream()
    out8 = torch.full((2 * n + 34,), 77, dtype=torch.int8, device=dev)
    st = torch.zeros(3, dtype=torch.int64, device=dev)
    args = dict(ctx=engine._ctx, dev=True, src=buf.data_ptr() + unit, blank=C.BLANK_THR, hold=hold, nfft=0, in_c=int(in_c64), in_count=n + hold, n_out=n,
                gain=C.GAIN)
    assert raw_check(dst=out8.data_ptr() + 17, stats=st.data_ptr(), **args) == 0
    hst = out8.cpu().numpy()
    assert np.array_equal(hst[17:17 + 2 * n], ref.i8) and (hst[:17] == 77).all() and (hst[17 + 2 * n:] == 77).all()
    outc = torch.zeros(n + 2, dtype=torch.complex64, device=dev)
    assert raw_check(dst=outc.data_ptr() + 8, cplx=1, stats=st.data_ptr(), **args) == 0
    hst = outc.cpu().numpy()
    assert np.array_equal(hst[1:1 + n], ref.c64) and hst[0] == 0 and hst[n + 1] == 0
    assert st.cpu().numpy().tolist() == [2 * ref.blanked, 0, 0]


def _both_input(nfft, n, marks, in_c64=False):
    """the tones of the excision cases with pulses (magnitude 141) at the sample indices `marks`"""
    data = C.tones(n, nfft, C.SEED + 21, in_c64)
    for m in marks:
        if in_c64:
            data[m] = complex(-100.0, 100.0)
        else:
            data[2 * m], data[2 * m + 1] = -100, 100
    return data


@pytest.mark.gpu
@pytest.mark.parametrize("nfft,in_c64", [(64, False), (128, True)])
def test_both_stages_with_holds_across_a_block_edge_and_a_tile_edge(engine, nfft, in_c64):
    h = nfft // 2
    ocfg = O.config(blank=100.0, hold=3, nfft=nfft, ratio=12.0, guard=1)
    n_out = (2 * C.TILE + 1) * h
    marks = (0, 3 * h - 1, C.TILE * h - 1, C.TILE * h + 2, 2 * C.TILE * h)      # the last ones' holds cross the tile edges
    data = _both_input(nfft, O.needed(ocfg, 0, n_out)[1] + 1, marks, in_c64)
    ref = O.evaluate(ocfg, data, C.GAIN, in_c64, 0, 0, n_out)
    f32 = O.evaluate(ocfg, data, C.GAIN, in_c64, 0, 0, n_out, precision="f32")
    top = float(np.max(np.abs(ref.y)))
    bound = 4.0 * float(np.max(np.abs(f32.y - ref.y))) / top
    assert ref.margin >= 1e-4 and ref.blanked == 4 + 7 + 10 + 7 and ref.bins > 0, (ref.margin, ref.blanked)
    got_c, got_i, st = _run_both(engine, ocfg, data, C.GAIN, in_c64, 0, 0, n_out)
    _hold_to_the_oracle("both N=%d" % nfft, got_c, got_i, st, ref, bound, top)


CUT_N, CUT_PIECES = 20000, (4099, 1, 15900)
FEED_CHUNKS = (1, 3, 4097)


@pytest.mark.gpu
@pytest.mark.parametrize("nfft,in_c64,dtype", [(1024, False, "int8"), (128, True, "complex64"), (0, False, "int8")])
def test_cutting_into_calls_and_chunks_does_not_matter(engine, nfft, in_c64, dtype):
    torch = nat.require_torch()
    ocfg = O.config(blank=100.0, hold=5, nfft=nfft, ratio=12.0, guard=2)
    cfg = _mcfg(ocfg)
    unit = 8 if in_c64 else 2
    n_in = O.needed(ocfg, 0, CUT_N)[1] + 1
    data = _both_input(nfft or 1024, n_in, (0, 4098, 4099, 4100, 9000, 19999), in_c64)
    raw = data.tobytes()
    whole, sw = mitigate.apply(engine, cfg, raw, C.GAIN, 0, 0, CUT_N, dtype, True, in_c64)
    assert sw.blanked >= 6 and (sw.bins > 0) == bool(nfft)
    parts, m, tot = [], 0, [0, 0, 0]
    for n in CUT_PIECES:
        lo, hi = O.needed(ocfg, m, n)
        out, st = mitigate.apply(engine, cfg, raw[lo * unit:(hi + 1) * unit], C.GAIN, lo, m, n, dtype, True, in_c64)
        parts.append(out)
        tot = [tot[0] + st.blanked, tot[1] + st.frames, tot[2] + st.bins]
        m += n
    assert m == CUT_N and tot == [sw.blanked, sw.frames, sw.bins]
    assert torch.cat(parts).cpu().numpy().tobytes() == whole.cpu().numpy().tobytes()
    # fed in chunks that cut samples; the whole-buffer result of the same bytes
    every = mitigate.apply(engine, cfg, raw, C.GAIN, dtype=dtype, stats=True, in_complex64=in_c64)
    mit = mitigate.Mitigate(engine, cfg, C.GAIN, dtype, in_c64)
    got, at = [], 0
    for n in FEED_CHUNKS + (len(raw) - sum(FEED_CHUNKS),):
        got.append(mit.feed(raw[at:at + n]))
        at += n
    assert at == len(raw)
    assert torch.cat(got).cpu().numpy().tobytes() == every[0].cpu().numpy().tobytes()
    assert (mit.blanked, mit.frames, mit.bins) == (every[1].blanked, every[1].frames, every[1].bins)
    assert mit.next_out == every[0].numel() // (2 if dtype == "int8" else 1) == O.out_range(ocfg, 0, n_in)[1] >= CUT_N


@pytest.mark.gpu
def test_every_refusal_with_a_live_context_leaves_output_and_statistics_untouched(engine):
    torch = nat.require_torch()
    engine.use_torch_stream()
    dev = "cuda:%d" % engine.device
    src = torch.ones(4096, dtype=torch.int8, device=dev)
    out = torch.full((4096,), 77, dtype=torch.int8, device=dev)
    st = torch.full((3,), 5, dtype=torch.int64, device=dev)
    fb = torch.full((64,), 9, dtype=torch.int32, device=dev)
    for label, code, change in bad_calls():
        kw = dict(ctx=engine._ctx, dev=True, src=src.data_ptr(), dst=out.data_ptr(), stats=st.data_ptr(), frame_bins=fb.data_ptr())
        kw.update(change)
        assert raw_check(**kw) == code, (label, nat.lib.gacq_last_error(engine._ctx))
    assert b"need input samples" in nat.lib.gacq_last_error(engine._ctx) or b"2^48" in nat.lib.gacq_last_error(engine._ctx)
    assert raw_check(ctx=engine._ctx, dev=True, src=src.data_ptr(), dst=out.data_ptr(), stats=st.data_ptr() + 4) == -1      # statistics off 8 bytes
    assert raw_check(ctx=engine._ctx, dev=True, src=src.data_ptr(), dst=out.data_ptr(), stats=st.data_ptr(), n_out=0) == 0    # nothing to do
    torch.cuda.synchronize()
    assert bool((out == 77).all()) and bool((st == 5).all()) and bool((fb == 9).all())
    # the unchanged call: 100 outputs of an all-ones recording, four owned frames, nothing blanked; the statistics are added to
    assert raw_check(ctx=engine._ctx, dev=True, src=src.data_ptr(), dst=out.data_ptr(), stats=st.data_ptr(), frame_bins=fb.data_ptr()) == 0
    assert raw_check(ctx=engine._ctx, dev=True, src=src.data_ptr(), dst=out.data_ptr() + 1024, stats=0, frame_bins=0, in_count=5 * 32 + 2) == 0
    torch.cuda.synchronize()
    hst = out.cpu().numpy()
    assert (hst[200:1024] == 77).all() and (hst[1224:] == 77).all() and not (hst[:200] == 77).any() and np.array_equal(hst[:200], hst[1024:1224])
    assert st.cpu().numpy().tolist()[:2] == [5, 5 + 4] and (fb.cpu().numpy()[4:] == 9).all()


def _chips():
    return codes_oracle.chips("gps.ca", C.SCENE["prn"])


@pytest.mark.gpu
def test_automatic_gain_is_the_oracles(engine):
    raw = C.scene_int8(_chips())
    cfg = C.scene_cfg()
    g, want = mitigate.auto_gain(engine, _mcfg(cfg), raw), O.auto_gain(cfg, raw)
    print("automatic gain %.6f, oracle %.6f" % (g, want))
    assert abs(g - want) <= 1e-5 * want
    assert abs(mitigate.auto_gain(engine, _mcfg(cfg), raw, 20.0) - want * 20.0 / 32.0) <= 1e-5 * want
    with pytest.raises(ValueError):
        mitigate.auto_gain(engine, _mcfg(cfg), bytes(8192))                # no power
    with pytest.raises(ValueError):
        mitigate.auto_gain(engine, _mcfg(cfg), raw[:2000])                 # no whole output block


def _found(result):
    metric, code, doppler = (float(v) for v in result)
    return doppler == 1200.0 and abs(code - C.SCENE["code0"]) <= 1023.0 / 4096.0, metric


@pytest.mark.gpu
def test_the_scene_is_found_by_the_engines_search_only_after_mitigation(engine):
    raw = C.scene_int8(_chips())
    prn = C.SCENE["prn"]

    def search(i8):
        v = i8.astype(np.float32)
        return engine.search("gps-l1", (v[0::2] + 1j * v[1::2]).astype(np.complex64), prn, C.SCENE_DOPPLERS, 3)

    r = search(raw)
    print("raw:", r)
    assert not _found(r)[0]
    cfg = _mcfg(C.scene_cfg())
    y, st = mitigate.apply(engine, cfg, raw, mitigate.auto_gain(engine, cfg, raw), stats=True)
    r = search(y.cpu().numpy())
    print("mitigated:", r, "blanked %.4f, %.1f bins a frame" % (st.blanked / (y.numel() / 2.0), st.bins / float(st.frames)))
    ok, metric = _found(r)
    assert ok and metric >= 5.0


MS = 250


def _code_error(got, want, L):
    return abs((got - want + L / 2.0) % L - L / 2.0)


@pytest.mark.gpu
def test_pipeline_simulated_recording_under_interference_to_tracking(engine):
    """simulate -> CW and pulses with torch -> int8 -> mitigate with the automatic gain -> handoff -> tracking, held to the caps of the
    ingest pipeline test (refined Doppler within 10 Hz, mean prompt at least 3 times an absent PRN's); without mitigation the hand-off does
    not find the satellite.  Measured on an MI355X: acquired at 1200 Hz / 417.34 chips with metric 8.09, refined to 0.084 Hz and 0.007 chip,
    mean prompt 7.7 times the absent PRN's; unmitigated 600 Hz / 248 chips, metric 1.16."""
    torch = nat.require_torch()
    s = C.SCENE
    n = int(s["fs"] * MS * 0.001)
    sym = simulate.symbols("gps-l1", s["prn"], -(-(MS + 2) // 20), 20, 100)
    sats = [simulate.Satellite("gps-l1", s["prn"], s["amp"], s["doppler"], s["code0"], symbols=sym)]
    x = simulate.recording(sats, s["fs"], 0.0, n, 31, s["sigma"], dtype="complex64", engine=engine)
    j = torch.arange(n, dtype=torch.float64, device=x.device)
    t = j / s["fs"]
    ph = 2.0 * np.pi * (s["cw_hz"] * t + 0.5 * s["cw_rate"] * t * t)
    cw = s["cw_amp"] * torch.complex(torch.cos(ph), torch.sin(ph))
    pp = 2.0 * np.pi * s["pulse_hz"] * t + 0.7
    on = ((j.to(torch.int64) + 400) % s["pulse_period"]) < s["pulse_len"]
    pulse = torch.where(on, s["pulse_amp"], 0.0) * torch.complex(torch.cos(pp), torch.sin(pp))
    v = torch.view_as_real((x.to(torch.complex128) + cw + pulse)).reshape(-1)
    raw = torch.clamp(torch.round(v), -127, 127).to(torch.int8)
    cfg = _mcfg(C.scene_cfg())
    gain = mitigate.auto_gain(engine, cfg, raw[:2 * 80000])
    y, st = mitigate.apply(engine, cfg, raw, gain, stats=True)
    items = [s["prn"], s["noise_prn"]]
    L = codes.code_length(trackloop.TRACKERS["gps-l1"].code)
    results, refined, loop, x_dev = handoff.handoff("gps-l1", y.cpu().numpy(), s["fs"], 0.0, items=items, engine=engine)
    try:
        assert [it for it, _ in refined] == items and loop.K == 2
        r = refined[0][1]
        print("gain %.4f, blanked %.4f, %.1f bins a frame: acquired doppler %.1f code %.2f metric %.2f -> refined doppler error %.3f Hz, code error "
              "%.5f chip" % (gain, st.blanked / (y.numel() / 2.0), st.bins / float(st.frames), results[0][2], results[0][1], results[0][0],
                             r.doppler - s["doppler"], _code_error(r.code_offset, s["code0"], L)))
        assert abs(r.doppler - s["doppler"]) <= 10.0, r
        recs = loop.run([x_dev] * loop.K)
        assert list(loop.status) == [0, 0]
    finally:
        loop.close()
    k = min(200, len(recs[0]))
    noise = float(np.mean(recs[1]["prompt"][:k]))
    print("%d records: mean prompt %.1f, absent PRN %.1f" % (len(recs[0]), np.mean(recs[0]["prompt"][:k]), noise))
    assert k >= 150 and np.mean(recs[0]["prompt"][:k]) > 3.0 * noise
    results, refined, loop, _ = handoff.handoff("gps-l1", raw.cpu().numpy(), s["fs"], 0.0, items=items[:1], engine=engine)
    if loop is not None:
        loop.close()
    r = refined[0][1]
    print("unmitigated: acquired doppler %.1f code %.2f metric %.2f, refined doppler %.2f code %.3f" % (results[0][2], results[0][1], results[0][0],
                                                                                                    r.doppler, r.code_offset))
    assert not (abs(r.doppler - s["doppler"]) <= 10.0 and _code_error(r.code_offset, s["code0"], L) <= 0.5)


@pytest.mark.gpu
def test_command_line_in_pieces_and_in_a_pipe_into_scan(tmp_path, engine):
    s = C.SCENE
    raw = C.scene_int8(_chips(), ms=72)                                         # every one of four pieces holds the automatic gain's window
    src, dst = str(tmp_path / "raw.iq"), str(tmp_path / "clean.iq")
    raw.tofile(src)
    argv = ["--blank", repr(s["blank"]), "--hold", str(s["hold"]), "--nfft", str(s["nfft"]), "--ratio", repr(s["ratio"]), "--guard", str(s["guard"])]
    out = io.StringIO()
    line = mitigate.run(argv + [src, dst], out, piece_bytes=160000)                # four pieces
    assert out.getvalue().splitlines() == [line]
    whole = io.BytesIO()
    cfg = _mcfg(C.scene_cfg())
    with open(src, "rb") as f:
        gain, n, mit = mitigate.mitigate_file(engine, cfg, f, whole)              # one piece
    got = np.fromfile(dst, dtype=np.int8)
    assert got.tobytes() == whole.getvalue() and len(got) == 2 * n == 2 * O.out_range(C.scene_cfg(), 0, len(raw) // 2)[1]
    assert line == mitigate.report_line(cfg, gain, n, mit.blanked, mit.frames, mit.bins) and mit.blanked > 0 and mit.bins > 0
    assert line.split()[0::2] == ["gain", "samples", "blanked", "excised"] and line.split()[3] == str(n)
    # the scan of the converted file finds the satellite ...
    scan_args = ["--prn", str(s["prn"]), "--doppler-search", "-2000,2000,200", "--time", "1"]
    starts, results = scan.scan("gps-l1", got, s["fs"], 0.0, 1, 6.0, [s["prn"]], C.SCENE_DOPPLERS, engine=engine)
    assert len(starts) >= 10
    r = results[0, 0]
    print("scan of the mitigated file:", r)
    assert abs(r["doppler_hz"] - s["doppler"]) <= 200.0 and _code_error(float(r["code_chips"]), s["code0"], 1023.0) <= 0.5 and r["metric"] >= 5.0
    want = scan.format_lines(signals.get("gps-l1"), [s["prn"]], starts, results)
    # ... and so does the pipe: - to - into scan, the report line on stderr
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = "%s -m gnss_dsp_tools_amd.mitigate %s - - | %s -m gnss_dsp_tools_amd.scan gps-l1 %s /dev/stdin %r 0.0" % (
        sys.executable, " ".join(argv), sys.executable, " ".join(scan_args), s["fs"])
    p = subprocess.run(cmd, shell=True, input=raw.tobytes(), cwd=ROOT, env=env, capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    assert p.stdout.decode().splitlines() == want
    assert line in p.stderr.decode().splitlines()
