"""GPU: the ingest kernels (csrc/gacq_ingest.hip) bit for bit against the numpy definition of tests/ingest_oracle.py -- every comparison
is an equality -- in both modes and both output forms: sizes around a lane's run and a workgroup's tile, inputs that start mid-byte,
misaligned buffers, rounding and clipping, independence of how a recording is cut into calls and chunks, the simulator's two output
forms through the f32 container, the automatic gain, every refusal through the raw ABI, and a real 2-bit recording through ingest,
hand-off and tracking."""
import ctypes
import io

import numpy as np
import pytest

import ingest_cases as C
import ingest_oracle as O
import simulate_cases as SC
from gnss_dsp_tools_amd import _native as nat
from gnss_dsp_tools_amd import codes, handoff, ingest, simulate, track, trackloop
from test_ingest_cpu import bad_calls, raw_call

PACKED = ("1ob", "2sm", "2ob", "4tc", "1sm")


def _both(engine, name, data, gain, ref_key, kw=None, **call):
    """complex64 and int8 output of one conversion, each equal to the oracle's, and the int8 the rounding of the device's complex64"""
    kw = kw or {}
    f = O.fmt(name, **kw)
    c = ingest.convert(engine, ingest.Format(name, **kw), data, gain, dtype="complex64", **call).cpu().numpy()
    i = ingest.convert(engine, ingest.Format(name, **kw), data, gain, dtype="int8", **call).cpu().numpy()
    want = C.reference(ref_key, lambda: O.evaluate(f, data, gain, call.get("in_first", 0), call.get("out_first"), call.get("n_out"), "complex64"))
    assert c.dtype == np.complex64 and i.dtype == np.int8 and c.shape == want.shape and i.shape == (2 * len(want),)
    assert np.array_equal(c, want), (ref_key, int(np.argmax(c != want)))
    assert np.array_equal(i, O.to_int8(want)), ref_key
    assert np.array_equal(i, O.to_int8(c)), ref_key
    return c, i


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(C.IQ_GAIN))
def test_iq_formats_match_the_oracle(engine, name):
    gain = C.IQ_GAIN[name]
    variants = [dict(), dict(conj=True)]
    if name in PACKED:
        variants += [dict(msb_first=False), dict(lut=C.PACKED_LUT[int(name[0])]), dict(msb_first=False, conj=True, lut=C.PACKED_LUT[int(name[0])])]
    for n in C.IQ_SIZES:
        for v, kw in enumerate(variants if n in (9, 4099) else variants[:1]):
            data = C.raw(name, C.iq_bytes(O.fmt(name), n))
            _, i = _both(engine, name, data, gain, ("iq", name, n, v), kw, n_out=n)
            if n == 4099 and v == 0:
                assert len(np.unique(i)) > (1 if name == "1ob" else 3)              # the case is not a trivial one
    # the data starts at input sample 16 and the output 5 samples later: mid-byte for the packed formats, off every wide load's alignment
    in_first, out_first = C.IQ_FIRST
    data = C.raw(name, C.iq_bytes(O.fmt(name), 4099), C.SEED + 1)
    _both(engine, name, data, gain, ("iq offset", name), in_first=in_first, out_first=out_first, n_out=4099 - (out_first - in_first))
    _both(engine, name, data, gain, ("iq offset 8", name), in_first=in_first, out_first=in_first + 8, n_out=300)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(C.REAL_GAIN))
def test_real_formats_match_the_oracle(engine, name):
    gain = C.REAL_GAIN[name]
    f = O.fmt(name, real=True)
    for out_first in C.REAL_OUT_FIRST:
        in_first = C.REAL_IN_FIRST_1001 if out_first == 1001 else 0
        for n_out in C.REAL_N_OUT:
            data = C.raw(name, C.real_bytes(f, in_first, out_first, n_out), C.SEED + out_first)
            _both(engine, name, data, gain, ("real", name, out_first, n_out), dict(real=True), in_first=in_first, out_first=out_first, n_out=n_out)
    data = C.raw(name, C.real_bytes(f, 0, 0, 5000))
    kw = dict(real=True, conj=True)
    if name in PACKED:
        kw.update(msb_first=False, lut=C.PACKED_LUT[int(name[0])])
    c, _ = _both(engine, name, data, gain, ("real conj", name), kw)                     # every output the data supports
    assert len(c) == O.out_range(f, 0, len(O.values(f, data)))[1] >= 5000
    plain = ingest.convert(engine, ingest.Format(name, **dict(kw, conj=False)), data, gain, dtype="complex64").cpu().numpy()
    assert np.array_equal(c, np.conj(plain)) and np.any(plain.imag != 0)


def _raw(engine, fmt, d_in, in_first, in_count, out_first, n_out, gain, out):
    torch = nat.require_torch()
    engine.use_torch_stream()
    st = fmt.struct()
    rc = nat.lib.gacq_ingest_dev(engine._ctx, ctypes.addressof(st), ctypes.c_void_p(d_in.data_ptr()), in_first, in_count, out_first, n_out, gain,
                                 int(out.dtype == torch.complex64), ctypes.c_void_p(out.data_ptr()))
    torch.cuda.synchronize()
    return rc


@pytest.mark.gpu
@pytest.mark.parametrize("name,real", [("s8", False), ("u8", False), ("s16", False), ("f32", False), ("2sm", False), ("4tc", False), ("s8", True),
                                       ("2sm", True)])
def test_misaligned_buffers(engine, name, real):
    """the input one byte into an allocation, the int8 output one byte in, the complex64 output one element in (8 but not 16 bytes)"""
    torch = nat.require_torch()
    dev = "cuda:%d" % engine.device
    f, fmt = O.fmt(name, real=real), ingest.Format(name, real=real)
    n = 4099
    data = C.raw(name, C.real_bytes(f, 0, 0, n) if real else C.iq_bytes(f, n), C.SEED + 2)
    gain = (C.REAL_GAIN if real else C.IQ_GAIN)[name]
    want = O.evaluate(f, data, gain, 0, 0, n, "complex64")
    buf = torch.zeros(len(data) + 1, dtype=torch.uint8, device=dev)
    buf[1:] = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to(dev)
    in_count = fmt.samples(len(data))
    out8 = torch.full((2 * n + 34,), 77, dtype=torch.int8, device=dev)
    assert _raw(engine, fmt, buf[1:], 0, in_count, 0, n, gain, out8[17:17 + 2 * n]) == 0
    h = out8.cpu().numpy()
    assert np.array_equal(h[17:17 + 2 * n], O.to_int8(want)) and (h[:17] == 77).all() and (h[17 + 2 * n:] == 77).all()
    outc = torch.zeros(n + 2, dtype=torch.complex64, device=dev)
    assert _raw(engine, fmt, buf[1:], 0, in_count, 0, n, gain, outc[1:1 + n]) == 0
    h = outc.cpu().numpy()
    assert np.array_equal(h[1:1 + n], want) and h[0] == 0 and h[n + 1] == 0


@pytest.mark.gpu
def test_rounding_and_clipping(engine):
    v = np.array([32767, -32767, -32768, 127, 128, -128, 1, 0], dtype="<i2")
    i = ingest.convert(engine, "s16", v.tobytes(), 1.0).cpu().numpy()
    assert i.tolist() == [127, -127, -127, 127, 127, -127, 1, 0]
    odd = np.array([1, 3, 5, 7, -1, -3, -5, -7, 253, 255, -253, -255, 257, -257, 9, 11, 13, -9], dtype="<i2")    # halves: ties go to even
    i = ingest.convert(engine, "s16", odd.tobytes(), 0.5).cpu().numpy()
    assert i.tolist() == [0, 2, 2, 4, 0, -2, -2, -4, 126, 127, -126, -127, 127, -127, 4, 6, 6, -4]
    assert np.array_equal(i, O.evaluate(O.fmt("s16"), odd.tobytes(), 0.5))
    inf, nan = np.float32("inf"), np.float32("nan")
    f = np.array([nan, 1.0, inf, -inf, -nan, 2.5, 3.5, -2.5, 126.5, 127.5, 1e30, -1e30, 0.49999997, -0.0, nan, nan, 1.5, nan], dtype="<f4")
    c = ingest.convert(engine, "f32", f.tobytes(), 1.0, dtype="complex64").cpu().numpy()
    i = ingest.convert(engine, "f32", f.tobytes(), 1.0).cpu().numpy()
    assert np.array_equal(c.view(np.float32), f, equal_nan=True)                        # gain 1: the floats themselves
    assert i.tolist() == [0, 1, 127, -127, 0, 2, 4, -2, 126, 127, 127, -127, 0, 0, 0, 0, 2, 0]
    assert np.array_equal(i, O.to_int8(c)) and np.array_equal(i, O.evaluate(O.fmt("f32"), f.tobytes(), 1.0))


def _pieces_equal_whole(engine, name, real, dtype):
    """one call of CUT_N outputs against calls of CUT_PIECES, each piece handed only the bytes it needs (from a multiple of 16 samples)"""
    torch = nat.require_torch()
    f, fmt = O.fmt(name, real=real), ingest.Format(name, real=real)
    gain = (C.REAL_GAIN if real else C.IQ_GAIN)[name]
    data = C.raw(name, C.real_bytes(f, 0, 0, C.CUT_N) if real else C.iq_bytes(f, C.CUT_N), C.SEED + 3)
    whole = ingest.convert(engine, fmt, data, gain, 0, 0, C.CUT_N, dtype)
    parts, m = [], 0
    for n in C.CUT_PIECES:
        lo = max(0, 2 * m - O.HALF) // 16 * 16 if real else m // 16 * 16
        hi = 2 * (m + n - 1) + O.HALF + 1 if real else m + n                          # one past the last input sample needed
        a, b = lo * fmt.sample_bits // 8, -(-hi * fmt.sample_bits // 8)
        parts.append(ingest.convert(engine, fmt, data[a:b], gain, lo, m, n, dtype))
        m += n
    assert m == C.CUT_N
    assert torch.cat(parts).cpu().numpy().tobytes() == whole.cpu().numpy().tobytes()
    assert np.array_equal(whole.cpu().numpy(), O.evaluate(f, data, gain, 0, 0, C.CUT_N, dtype))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["int8", "complex64"])
@pytest.mark.parametrize("name,real", [("s16", False), ("1ob", False), ("u8", True), ("2sm", True)])
def test_cutting_into_calls_does_not_matter(engine, name, real, dtype):
    _pieces_equal_whole(engine, name, real, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("name,real", [("s16", False), ("f32", False), ("2sm", False), ("s8", True), ("2sm", True), ("1sm", True)])
def test_feeding_chunks_gives_the_whole_buffer_result(engine, name, real):
    torch = nat.require_torch()
    f, fmt = O.fmt(name, real=real), ingest.Format(name, real=real)
    gain = (C.REAL_GAIN if real else C.IQ_GAIN)[name]
    data = C.raw(name, 20001, C.SEED + 4)                       # an odd byte count: the last s16 / f32 sample stays incomplete
    for dtype in ("int8", "complex64"):
        whole = ingest.convert(engine, fmt, data, gain, dtype=dtype)
        ing = ingest.Ingest(engine, fmt, gain, dtype)
        got, at = [], 0
        for n in C.FEED_CHUNKS + (len(data) - sum(C.FEED_CHUNKS),):
            got.append(ing.feed(data[at:at + n]))
            at += n
        assert at == len(data)
        assert torch.cat(got).cpu().numpy().tobytes() == whole.cpu().numpy().tobytes()
        assert ing.next_out == len(O.evaluate(f, data, gain, dtype="complex64")) == whole.numel() // (2 if dtype == "int8" else 1)
        if real:                                                 # the kept tail starts on a byte boundary, at a multiple of 16 samples
            assert ing.in_first % 16 == 0 and ing.in_first <= 2 * ing.next_out - O.HALF
    assert np.array_equal(whole.cpu().numpy(), O.evaluate(f, data, gain, dtype="complex64"))


@pytest.mark.gpu
def test_simulated_complex64_ingested_as_f32_is_the_simulated_int8(engine):
    torch = nat.require_torch()
    c = SC.CASES["seven kinds sigma=12"]
    args = (c["sats"], c["fs"], c["coffset"], c["n"], SC.SEED, c["sigma"], c["j0"])
    v = simulate.recording(*args, "complex64", engine)
    x = simulate.recording(*args, "int8", engine)
    got = ingest.convert(engine, "f32", torch.view_as_real(v).reshape(-1).view(torch.uint8), 1.0)
    assert got.dtype == torch.int8 and torch.equal(got, x)
    back = ingest.convert(engine, "f32", torch.view_as_real(v).reshape(-1).view(torch.uint8), 1.0, dtype="complex64")
    assert torch.equal(torch.view_as_real(back), torch.view_as_real(v))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["s16", "2sm real"])
def test_automatic_gain_is_the_oracles_float64(engine, name):
    f, data = C.gaussian_recordings()[name]
    fmt = ingest.Format("2sm", real=True) if f["real"] else ingest.Format("s16")
    g = ingest.auto_gain(engine, fmt, data)
    assert g == O.auto_gain(f, data)
    assert ingest.auto_gain(engine, fmt, data, 20.0) == O.auto_gain(f, data, 20.0)
    x = ingest.convert(engine, fmt, data, g, 0, 0, O.AUTO_SAMPLES).cpu().numpy().astype(np.float64)
    rms = float(np.sqrt(np.mean(x[0::2] ** 2 + x[1::2] ** 2)))
    print(name, "gain %.6g rms %.3f" % (g, rms))
    assert abs(rms - 32.0) <= 0.05 * 32.0
    with pytest.raises(ValueError):
        ingest.auto_gain(engine, "s8", bytes(4096))              # no power


@pytest.mark.gpu
def test_every_refusal_through_the_raw_abi_leaves_the_output_untouched(engine):
    torch = nat.require_torch()
    engine.use_torch_stream()
    dev = "cuda:%d" % engine.device
    src = torch.ones(4096, dtype=torch.uint8, device=dev)
    out = torch.full((4096,), 77, dtype=torch.int8, device=dev)
    for label, code, change in bad_calls():
        rc = raw_call(engine._ctx, src.data_ptr(), out.data_ptr(), **change)
        assert rc == code, (label, rc, nat.lib.gacq_last_error(engine._ctx))
    assert raw_call(engine._ctx, src.data_ptr(), out.data_ptr() + 4, cplx=1) == -1                # complex64 output off its alignment
    assert raw_call(engine._ctx, src.data_ptr(), out.data_ptr(), n_out=0) == 0                    # nothing to do
    torch.cuda.synchronize()
    assert bool((out == 77).all())
    assert raw_call(engine._ctx, src.data_ptr(), out.data_ptr()) == 0                              # the unchanged call writes 200 bytes
    # real mode just long enough: outputs 0 .. 9 need inputs up to 2 * 9 + 21
    assert raw_call(engine._ctx, src.data_ptr(), out.data_ptr() + 1024, real=1, in_count=2 * 9 + 22, n_out=10) == 0
    torch.cuda.synchronize()
    h = out.cpu().numpy()
    assert (h[:200] == 1).all() and (h[200:1024] == 77).all() and not (h[1024:1044] == 77).all() and (h[1044:] == 77).all()


MS = 250
DWELLS = (20, 20)
_SCENE = {}


def _scene(engine):
    """250 ms of the scene of ingest_cases.SCENE from the simulator's complex64 output on the device: real part, two bits (sign,
    magnitude above sigma), four codes per byte with torch -> (packed uint8 tensor, symbols); made once"""
    if not _SCENE:
        torch = nat.require_torch()
        s = C.SCENE
        n = int(s["fs"] * MS * 0.001)
        sym = simulate.symbols("gps-l1", s["prn"], -(-(MS + 2) // 20), 20, 100)
        sats = [simulate.Satellite("gps-l1", s["prn"], s["amp"], s["doppler"], s["code0"], symbols=sym)]
        x = simulate.recording(sats, s["fs"], s["if_hz"], n, 31, s["sigma"], dtype="complex64", engine=engine).real
        code = (((x < 0).to(torch.uint8) << 1) | (x.abs() > s["sigma"]).to(torch.uint8))[:n // 4 * 4].view(-1, 4)
        _SCENE["packed"] = ((code[:, 0] << 6) | (code[:, 1] << 4) | (code[:, 2] << 2) | code[:, 3]).contiguous()
    return _SCENE["packed"]


def _code_error(got, want, L):
    return abs((got - want + L / 2.0) % L - L / 2.0)


@pytest.mark.gpu
def test_pipeline_real_two_bit_recording_to_tracking(engine):
    """ingest with the automatic gain -> handoff -> 200 ms of tracking, held to the caps of test_handoff_gpu.py"""
    s = C.SCENE
    packed = _scene(engine)
    fmt = ingest.Format("2sm", real=True)
    gain = ingest.auto_gain(engine, fmt, packed)
    y = ingest.convert(engine, fmt, packed, gain)
    fs, coffset = fmt.rates(s["fs"], s["if_hz"])
    assert (fs, coffset) == (4.092e6, 0.0) and y.numel() == 2 * ((4 * packed.numel() - 1 - O.HALF) // 2 + 1)
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


@pytest.mark.gpu
def test_command_line_file_in_file_out(tmp_path, engine):
    s = C.SCENE
    packed = _scene(engine).cpu().numpy()
    src, dst = str(tmp_path / "if.bin"), str(tmp_path / "iq.bin")
    packed.tofile(src)
    out = io.StringIO()
    line = ingest.run(["--format", "2sm", "--real", src, repr(s["fs"]), repr(s["if_hz"]), dst], out, piece_bytes=1 << 17)       # four pieces
    assert out.getvalue().splitlines() == [line]
    whole = io.BytesIO()
    with open(src, "rb") as f:
        gain, n = ingest.convert_file(engine, ingest.Format("2sm", real=True), f, whole)                  # one piece
    got = np.fromfile(dst, dtype=np.int8)
    assert got.tobytes() == whole.getvalue() and len(got) == 2 * n                   # the file does not depend on the piece size
    word = line.split()
    assert word[0::2] == ["fs", "coffset", "gain", "samples"] and word[1::2] == [repr(4.092e6), repr(0.0), repr(gain), str(n)]
    rows = track.run("gps-l1", ["--loop-dwells", "20,20", dst, word[1], word[3], str(s["prn"]), repr(s["doppler"]), repr(s["code0"])], io.StringIO())
    assert len(rows) >= 200
