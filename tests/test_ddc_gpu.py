"""GPU: the down-converter kernel (csrc/gacq_ddc.hip) against the integer definition of tests/ddc_oracle.py.  Every comparison of
samples is an equality: both output forms against the oracle, the int8 as the rounding of the device's own complex64, device against
device however the recording is cut into calls, chunks, pieces and bands.  Then a 250 ms recording with the satellite 4.092 MHz off
centre through the down-converter, hand-off and tracking."""
import ctypes
import io

import numpy as np
import pytest

import ddc_cases as C
import ddc_oracle as O
from gnss_dsp_tools_amd import _native as nat
from gnss_dsp_tools_amd import codes, ddc, handoff, simulate, trackloop
from test_ddc_cpu import BAD_ARG, bad_config_calls, bad_run_calls, raw_check


def _band(ts, f_shift):
    return ddc.Band(f_shift, ts.D, taps=ts.taps)


@pytest.mark.gpu
def test_the_tile_of_the_cases_is_the_kernels():
    assert [nat.lib.gacq_ddc_tile(D) for D in range(1, 65)] == [C.tile(D) for D in range(1, 65)]


@pytest.mark.gpu
@pytest.mark.parametrize("ts", C.TAP_SETS, ids=lambda ts: ts.name)
def test_both_output_forms_equal_the_oracle(engine, ts):
    """sizes 1, 7, tile - 1, tile, tile + 1, 2 tile + 3; the starts and the shifts in turn (ddc_cases.case)"""
    for i in range(len(C.sizes(ts.D))):
        data, in_first, out_first, n_out, f_shift = C.case(ts, i)
        want_c, want_i = C.case_reference(ts, i)
        band = _band(ts, f_shift)
        assert band.dphase(C.FS) == O.phase_increment(f_shift, C.FS)
        with ddc.Converter(engine, band, C.FS) as conv:
            d = ddc._device_iq(engine, data)
            got_c = conv.run(d, in_first, out_first, n_out, C.GAIN, "complex64").cpu().numpy()
            got_i = conv.run(d, in_first, out_first, n_out, C.GAIN, "int8").cpu().numpy()
        label = (ts.name, n_out, in_first, out_first, f_shift)
        assert got_c.dtype == np.complex64 and got_i.dtype == np.int8 and got_c.shape == (n_out,) and got_i.shape == (2 * n_out,)
        assert np.array_equal(got_c.view(np.float32), want_c.view(np.float32)), label
        assert np.array_equal(got_i, want_i) and np.array_equal(got_i, O.to_int8(got_c)), label
        assert np.any(want_i != 0), label


@pytest.mark.gpu
@pytest.mark.parametrize("ts", [C.TAP_SETS[3], C.TAP_SETS[5]], ids=lambda ts: ts.name)
def test_misaligned_buffers_give_the_same_output(engine, ts):
    """the input one byte and six bytes into an allocation, the int8 output 17 bytes in, the complex64 output one element (8 but not
    16 bytes) in"""
    torch = nat.require_torch()
    dev = "cuda:%d" % engine.device
    data, in_first, out_first, n_out, f_shift = C.case(ts, 4)
    want_c, want_i = C.case_reference(ts, 4)
    raw = np.frombuffer(data.tobytes(), dtype=np.uint8)
    with ddc.Converter(engine, _band(ts, f_shift), C.FS) as conv:
        engine.use_torch_stream()
        for off in (1, 6):
            buf = torch.zeros(len(raw) + 16, dtype=torch.uint8, device=dev)
            buf[off:off + len(raw)] = torch.from_numpy(raw.copy()).to(dev)
            out8 = torch.full((2 * n_out + 40,), 77, dtype=torch.int8, device=dev)
            args = (buf.data_ptr() + off, in_first, len(raw) // 2, out_first, n_out, C.GAIN)
            assert nat.lib.gacq_ddc_run_dev(conv._h, *args, 0, ctypes.c_void_p(out8.data_ptr() + 17)) == 0
            hst = out8.cpu().numpy()
            assert np.array_equal(hst[17:17 + 2 * n_out], want_i) and (hst[:17] == 77).all() and (hst[17 + 2 * n_out:] == 77).all(), off
            outc = torch.zeros(n_out + 2, dtype=torch.complex64, device=dev)
            assert nat.lib.gacq_ddc_run_dev(conv._h, *args, 1, ctypes.c_void_p(outc.data_ptr() + 8)) == 0
            hst = outc.cpu().numpy()
            assert np.array_equal(hst[1:1 + n_out].view(np.float32), want_c.view(np.float32)) and hst[0] == 0 and hst[n_out + 1] == 0, off


@pytest.mark.gpu
def test_rounding_ties_and_clipping(engine):
    """the pure shift with dP = 0 hands x 2^14 2^-7 2^15 2^-22 gain = x gain through: gains that put values on .5 and past 127"""
    x = np.arange(-128, 128, dtype=np.int8)
    data = np.stack([x, x[::-1]], axis=1).reshape(-1)
    band = ddc.Band(0.0, 1)
    for gain in (0.5, 1.5, 0.25, 1.0, 127.5 / 127.0):
        c = ddc.convert(engine, band, C.FS, data, gain, dtype="complex64").cpu().numpy()
        i = ddc.convert(engine, band, C.FS, data, gain).cpu().numpy()
        want = x.astype(np.float32) * np.float32(gain)
        assert np.array_equal(c.real, want) and np.array_equal(c.imag, want[::-1])
        assert np.array_equal(i, O.to_int8(c)) and np.array_equal(i, O.evaluate(0.0, C.FS, 1, [32768], data, gain))
        v = np.clip(np.rint(want.astype(np.float64)), -127, 127)                    # ties to even: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2
        assert np.array_equal(i[0::2], v.astype(np.int8)) and i.min() >= -127
    i = ddc.convert(engine, band, C.FS, data, 0.5).cpu().numpy()[0::2]
    assert i[128 + 1] == 0 and i[128 + 3] == 2 and i[128 + 5] == 2 and i[128 - 1] == 0 and i[128 - 3] == -2
    i = ddc.convert(engine, band, C.FS, data, 1.5).cpu().numpy()[0::2]
    assert i[0] == -127 and i[255] == 127 and i[128 + 84] == 126 and i[128 + 85] == 127 and i[128 + 86] == 127 and i[128 - 85] == -127


CUT_PIECES = (1027, 1, 2072)
FEED_CHUNKS = (1, 3, 4097, 20001)


@pytest.mark.gpu
@pytest.mark.parametrize("ts,dtype", [(C.TAP_SETS[4], "int8"), (C.TAP_SETS[6], "complex64"), (C.TAP_SETS[7], "int8")], ids=lambda v: getattr(v, "name", v))
def test_cutting_into_calls_and_chunks_does_not_matter(engine, ts, dtype):
    torch = nat.require_torch()
    T = len(ts.taps)
    n_total = sum(CUT_PIECES) if ts.D < 64 else 300
    pieces = CUT_PIECES if ts.D < 64 else (127, 1, 172)
    n_in = O.needed(ts.D, T, 0, n_total)[1] + 1 + min(5, ts.D - 1)        # a few samples more than the last output needs
    raw = C.random_int8(n_in, 900 + ts.D).tobytes()
    band = _band(ts, C.SHIFTS[2])
    whole = ddc.convert(engine, band, C.FS, raw, C.GAIN, dtype=dtype)
    per = 2 if dtype == "int8" else 1
    assert whole.numel() // per == n_total == O.out_range(ts.D, T, 0, n_in)[1]
    want = O.evaluate(C.SHIFTS[2], C.FS, ts.D, ts.taps, raw, C.GAIN, dtype=dtype)
    assert whole.cpu().numpy().tobytes() == want.tobytes()
    parts, m = [], 0
    for n in pieces:
        lo, hi = O.needed(ts.D, T, m, n)
        parts.append(ddc.convert(engine, band, C.FS, raw[2 * lo:2 * (hi + 1)], C.GAIN, lo, m, n, dtype))
        m += n
    assert m == n_total and torch.cat(parts).cpu().numpy().tobytes() == want.tobytes()
    # fed in chunks that cut samples
    dc = ddc.Downconverter(engine, band, C.FS, C.GAIN, dtype)
    got, at = [], 0
    chunks = [c for c in FEED_CHUNKS if c < len(raw) // 2]
    for n in chunks + [len(raw) - sum(chunks)]:
        got.append(dc.feed(raw[at:at + n]))
        at += n
    dc.close()
    assert at == len(raw) and dc.next_out == n_total
    assert torch.cat(got).cpu().numpy().tobytes() == want.tobytes()


@pytest.mark.gpu
def test_every_refusal_through_the_raw_abi_leaves_the_output_untouched(engine):
    torch = nat.require_torch()
    engine.use_torch_stream()
    dev = "cuda:%d" % engine.device
    src = torch.ones(4096, dtype=torch.int8, device=dev)
    out = torch.full((4096,), 77, dtype=torch.int8, device=dev)
    g = np.ascontiguousarray(O.design_taps(4, 33), dtype=np.int32)
    # what the configuration decides is refused when the handle is opened
    for label, code, change in bad_config_calls():
        taps = np.ascontiguousarray(change.get("taps", g), dtype=np.int32)
        st = ddc.DdcCfg(dphase=12345, decim=change.get("D", 4))
        h = ctypes.c_void_p()
        rc = nat.lib.gacq_ddc_open(engine._ctx, ctypes.addressof(st) if change.get("cfg", True) else None,
                                   None if change.get("null_taps") else ctypes.c_void_p(taps.ctypes.data), change.get("T", len(taps)), ctypes.byref(h))
        assert rc == code and not h.value, (label, rc)
    st = ddc.DdcCfg(dphase=12345, decim=4)
    assert nat.lib.gacq_ddc_open(engine._ctx, ctypes.addressof(st), ctypes.c_void_p(g.ctypes.data), 33, None) == BAD_ARG
    h = ctypes.c_void_p()
    assert nat.lib.gacq_ddc_open(engine._ctx, ctypes.addressof(st), ctypes.c_void_p(g.ctypes.data), 33, ctypes.byref(h)) == 0 and h.value
    try:
        kw = dict(handle=h, src=src.data_ptr(), dst=out.data_ptr())
        for label, code, change in bad_run_calls():
            assert raw_check(**dict(kw, **change)) == code, (label, nat.lib.gacq_last_error(engine._ctx))
        assert b"need input samples" in nat.lib.gacq_last_error(engine._ctx)
        assert raw_check(**dict(kw, src=0)) == BAD_ARG and raw_check(**dict(kw, dst=0)) == BAD_ARG                  # NULL pointers
        assert raw_check(**dict(kw, cplx=1, dst=out.data_ptr() + 4)) == BAD_ARG                                     # complex64 output off 8 bytes
        assert raw_check(**dict(kw, n_out=0)) == 0                                                                  # nothing to do
        torch.cuda.synchronize()
        assert bool((out == 77).all())
        assert raw_check(**kw) == 0                                                                                 # the unchanged call writes 200 bytes
        assert raw_check(**dict(kw, dst=out.data_ptr() + 1024, in_count=99 * 4 + 17)) == 0                          # just long enough
        torch.cuda.synchronize()
        hst = out.cpu().numpy()
        want = O.evaluate(0.0, 1.0, 4, g, np.ones(2000, dtype=np.int8), 1.0, 0, 0, 100, dp=12345)
        assert np.array_equal(hst[:200], want) and np.array_equal(hst[1024:1224], want) and (hst[200:1024] == 77).all() and (hst[1224:] == 77).all()
    finally:
        nat.lib.gacq_ddc_close(h)


def _scene_chunk(n, seed):
    return C.random_int8(n, seed).tobytes()


@pytest.mark.gpu
def test_two_bands_from_one_file_equal_two_single_band_runs(engine):
    raw = _scene_chunk(300000, 31)
    bands = [ddc.Band(-562500.0, 16), ddc.Band(5.0625e6, 16, cutoff_hz=1.0e6)]
    fs = 65.472e6
    outs = [io.BytesIO(), io.BytesIO()]
    gains, n = ddc.split_file(engine, bands, fs, io.BytesIO(raw), outs, piece_bytes=1 << 17)           # five pieces, automatic gains
    for k, b in enumerate(bands):
        one = io.BytesIO()
        g1, n1 = ddc.split_file(engine, [b], fs, io.BytesIO(raw), [one])                              # one piece
        assert g1 == [gains[k]] and n1 == [n[k]] and one.getvalue() == outs[k].getvalue() and n[k] == (300000 - 1 - 64) // 16 + 1
        want = O.evaluate(b.f_shift, fs, 16, b.taps_for(fs), raw, gains[k])
        assert outs[k].getvalue() == want.tobytes()
        assert abs(gains[k] - O.auto_gain(b.f_shift, fs, 16, b.taps_for(fs), raw)) <= 1e-6 * gains[k]
    assert outs[0].getvalue() != outs[1].getvalue()


@pytest.mark.gpu
def test_command_line_file_in_file_out(tmp_path, engine):
    raw = _scene_chunk(200000, 32)
    src, a, b = str(tmp_path / "wide.iq"), str(tmp_path / "a.iq"), str(tmp_path / "b.iq")
    with open(src, "wb") as f:
        f.write(raw)
    argv = ["--decim", "8", "--band", "4.092e6", a, "--band", "-1.0e6", b, src, "32.736e6", "4.092e6"]
    out = io.StringIO()
    lines = ddc.run(argv, out, piece_bytes=1 << 16)                                                   # seven pieces
    assert out.getvalue().splitlines() == lines and len(lines) == 2
    outs = [io.BytesIO(), io.BytesIO()]
    bands = [ddc.Band(4.092e6, 8), ddc.Band(-1.0e6, 8)]
    gains, n = ddc.split_file(engine, bands, 32.736e6, io.BytesIO(raw), outs)                          # one piece
    for k, name in enumerate((a, b)):
        got = np.fromfile(name, dtype=np.int8)
        assert got.tobytes() == outs[k].getvalue() and len(got) == 2 * n[k]                            # the files do not depend on the piece size
        assert lines[k] == ddc.report_line(bands[k], 32.736e6, 4.092e6, gains[k], n[k])
    word = lines[0].split()
    assert word[0::2] == ["band", "fs", "coffset", "gain", "samples"] and word[1::2] == [repr(4.092e6), repr(4.092e6), repr(0.0), repr(gains[0]), str(n[0])]
    # complex64, one gain for both
    lines = ddc.run(["--decim", "8", "--gain", "2", "--complex64", "--band", "4.092e6", a, src, "32.736e6", "4.092e6"], io.StringIO(), piece_bytes=1 << 16)
    want = O.evaluate(4.092e6, 32.736e6, 8, O.design_taps(8), raw, 2.0, dtype="complex64")
    assert np.fromfile(a, dtype=np.complex64).tobytes() == want.tobytes() and lines[0].split()[7] == "2.0"


MS = 250
DWELLS = (20, 20)


def _code_error(got, want, L):
    return abs((got - want + L / 2.0) % L - L / 2.0)


@pytest.mark.gpu
def test_pipeline_wide_recording_to_tracking(engine):
    """simulate at 32.736 MS/s with the satellite 4.092 MHz off centre -> ddc at D = 8 with the automatic gain -> handoff -> 200 ms of
    tracking, held to the caps of the ingest pipeline test.  Measured on an MI355X: gain 5.49, acquired at 1200 Hz / 417.34 chips, refined
    to 0.198 Hz and 0.0173 chip, carrier_f[199] 1.1 Hz off, mean prompt 12.8 times the absent PRN's."""
    s = C.SCENE
    n = int(s["fs"] * MS * 0.001)
    sym = simulate.symbols("gps-l1", s["prn"], -(-(MS + 2) // 20), 20, 100)
    sats = [simulate.Satellite("gps-l1", s["prn"], s["amp"], s["doppler"], s["code0"], symbols=sym)]
    raw = simulate.recording(sats, s["fs"], s["coffset"], n, 31, s["sigma"], dtype="int8", engine=engine)
    band = ddc.Band(s["coffset"], s["D"])
    fs, coffset = band.rates(s["fs"], s["coffset"])
    assert (fs, coffset) == (4.092e6, 0.0)
    gain = ddc.auto_gain(engine, band, s["fs"], raw[:2 * ddc.auto_window(band)])
    y = ddc.convert(engine, band, s["fs"], raw, gain)
    assert y.numel() == 2 * ((n - 1 - band.H) // s["D"] + 1)
    items = [s["prn"], s["noise_prn"]]
    results, refined, loop, x_dev = handoff.handoff("gps-l1", y.cpu().numpy(), fs, coffset, items=items, loop_dwells=DWELLS, ms=80, engine=engine)
    try:
        assert [it for it, _ in refined] == items and loop.K == 2
        L = codes.code_length(trackloop.TRACKERS["gps-l1"].code)
        r = refined[0][1]
        print("gain %.4f: acquired doppler %.1f code %.2f -> refined doppler error %.3f Hz, code error %.5f chip, ratio %.1f"
              % (gain, results[0][2], results[0][1], r.doppler - s["doppler"], _code_error(r.code_offset, s["code0"], L), r.ratio))
        assert abs(r.doppler - s["doppler"]) <= 10.0, r
        assert _code_error(r.code_offset, s["code0"], L) <= 0.03, r
        recs = loop.run([x_dev] * loop.K)
        assert list(loop.status) == [0, 0]
    finally:
        loop.close()
    noise = float(np.mean(recs[1]["prompt"][:200]))
    assert len(recs[0]) >= 200
    print("carrier_f[199] error %.3f Hz, mean prompt %.1f, noise channel %.1f" % (recs[0]["carrier_f"][199] - s["doppler"],
                                                                                np.mean(recs[0]["prompt"][:200]), noise))
    assert abs(recs[0]["carrier_f"][199] - s["doppler"]) <= 10.0
    assert np.mean(recs[0]["prompt"][:200]) > 3.0 * noise
