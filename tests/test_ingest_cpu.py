"""CPU: the definition of the recording ingest (tests/ingest_oracle.py) against the formula of its filter, a tone at a real front-end's
frequency plan and its own closed form; the format names of gnss_dsp_tools_amd.ingest; every refusal of gacq_ingest_dev that needs no
device; the command line; and the condition of the GPU pipeline test, established on the oracles alone."""
import ctypes

import numpy as np
import pytest

import ingest_cases as C
import ingest_oracle as O
from gnss_dsp_tools_amd import _native as nat
from gnss_dsp_tools_amd import acquire, ingest
from oracle import acq_oracle, codes_oracle


def test_tap_table_is_the_rounded_hann_windowed_sinc():
    g = O.taps()
    want = O.taps_from_formula()                                   # k = -23 .. 23
    assert np.array_equal(want[2:-2], g) and not want[:2].any() and not want[-2:].any()
    h = acquire.firwin_hann(47, 0.5)                                # the same shape from the package's own window design
    assert np.array_equal(np.rint(h / h[23] * 16384.0).astype(np.int64), want)
    assert int(g.sum()) == 32768 and g[O.HALF] == 16384 and np.array_equal(g, g[::-1])
    k = np.arange(-O.HALF, O.HALF + 1)
    assert not g[(k % 2 == 0) & (k != 0)].any()                    # even offsets other than 0
    assert [int(v) for v in g[O.HALF + 1::2]] == list(O.G_ODD)
    assert 128 * int(np.abs(g).sum()) == 128 * 53736 < 2 ** 23


def test_real_mode_of_the_oracle_on_a_tone_at_the_sige_plan():
    fs, f_if, n = 16.3676e6, 4.1304e6, 1 << 16
    x = np.rint(100.0 * np.cos(2.0 * np.pi * f_if / fs * np.arange(n) + 0.3)).astype(np.int8)
    u = O.evaluate(O.fmt("s8", real=True), x.tobytes(), 1.0, dtype="complex64")
    assert len(u) == (n - 1 - O.HALF) // 2 + 1
    nfft = 1 << 14
    s = np.abs(np.fft.fft(u[100:100 + nfft] * np.hanning(nfft))) ** 2
    f = np.fft.fftfreq(nfft, 2.0 / fs)
    k = int(np.argmax(s))
    assert abs(f[k] - (f_if - fs / 4.0)) <= fs / 2.0 / nfft         # within one bin of IF - fs/4
    ki = int(np.argmin(np.abs(f + (f_if - fs / 4.0))))              # the image: -IF - fs/4 folded by the decimation
    image_db = 10.0 * np.log10(s[k] / s[ki - 3:ki + 4].max())
    print("peak at %.1f Hz, image %.1f dB down" % (f[k], image_db))
    assert image_db >= 60.0


def test_closed_form_of_the_real_mode_equals_the_plain_complex_form():
    rng = np.random.Generator(np.random.PCG64(C.SEED))
    x = rng.integers(-128, 128, size=600)

    def x_at(n):
        return np.where((n < 0) | (n >= len(x)), 0, x[np.clip(n, 0, len(x) - 1)])

    for out_first in range(8):
        a, b = O.accumulate_real(x_at, out_first, 200), O.closed_form_real(x_at, out_first, 200)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), out_first


LUTS = {"1sm": [1, -1], "1ob": [-1, 1], "2sm": [1, 3, -1, -3], "2ob": [-3, -1, 1, 3], "2tc": [1, 3, -3, -1],
        "4sm": [1, 3, 5, 7, 9, 11, 13, 15, -1, -3, -5, -7, -9, -11, -13, -15],
        "4ob": [-15, -13, -11, -9, -7, -5, -3, -1, 1, 3, 5, 7, 9, 11, 13, 15],
        "4tc": [1, 3, 5, 7, 9, 11, 13, 15, -15, -13, -11, -9, -7, -5, -3, -1]}


def test_format_names():
    assert sorted(ingest.NAMES) == sorted(["s8", "u8", "s16", "f32"] + list(LUTS))
    for name, lut in LUTS.items():
        f = ingest.Format(name)
        assert f.lut == lut == O.fmt(name)["lut"] and f.container == ingest.PACKED and f.bits == int(name[0]) and f.msb_first and not f.real
        st = f.struct()
        assert list(st.lut)[:len(lut)] == lut and (st.container, st.bits, st.msb_first, st.real, st.conj) == (4, f.bits, 1, 0, 0)
        assert f.sample_bits == 2 * f.bits and ingest.Format(name, real=True).sample_bits == f.bits
    for name, code, bits in (("s8", 0, 8), ("u8", 1, 8), ("s16", 2, 16), ("f32", 3, 32)):
        f = ingest.Format(name, conj=True)
        assert (f.container, f.sample_bits, f.struct().conj) == (code, 2 * bits, 1)
    f = ingest.Format("2OB", msb_first=False, lut=[5, 6, 7, -8], real=True)
    assert f.lut == [5, 6, 7, -8] and f.struct().msb_first == 0 and f.struct().real == 1
    for bad in ("s32", "3sm", "1tc", "2xx", "", "u16"):
        with pytest.raises(ValueError):
            ingest.Format(bad)
    for kw in (dict(name="s16", real=True), dict(name="f32", real=True), dict(name="2sm", lut=[1, 2, 3]), dict(name="2sm", lut=[1, 2, 3, 200]),
               dict(name="s8", lut=[1, 2])):
        with pytest.raises(ValueError):
            ingest.Format(**kw)
    assert ctypes.sizeof(ingest.IngestFmt) == 48
    # the output samples a stretch of input supports, as the oracle has them
    for f, o in ((ingest.Format("s8", real=True), O.fmt("s8", real=True)), (ingest.Format("s16"), O.fmt("s16"))):
        for in_first, in_count in ((0, 0), (0, 21), (0, 22), (0, 23), (0, 24), (16, 100), (17, 100), (1976, 43), (1976, 47), (1976, 48)):
            assert f.out_range(in_first, in_count) == O.out_range(o, in_first, in_count)
    assert ingest.Format("s8", real=True).out_range(0, 22) == (0, 1) and ingest.Format("s8", real=True).out_range(16, 100) == (19, 29)


def _fmt(name="s8", **kw):
    return ingest.Format(name, **{k: v for k, v in kw.items() if k in ("real", "conj", "msb_first", "lut")}).struct()


def bad_calls():
    """(label, expected code, keyword changes of raw_call) of every refusal of gacq_ingest_dev; shared with the GPU test"""
    nan, inf = float("nan"), float("inf")
    out = [("container -1", -1, dict(container=-1)), ("container 5", -1, dict(container=5)),
           ("bits 0", -1, dict(name="2sm", bits=0)), ("bits 3", -1, dict(name="2sm", bits=3)), ("bits 8", -1, dict(name="2sm", bits=8)),
           ("real s16", -1, dict(container=2, real=1, in_count=400)), ("real f32", -1, dict(container=3, real=1, in_count=400)),
           ("gain nan", -1, dict(gain=nan)), ("gain inf", -1, dict(gain=inf)), ("gain 0", -1, dict(gain=0.0)), ("gain < 0", -1, dict(gain=-1.0)),
           ("gain 0 in fp32", -1, dict(gain=1e-60)), ("gain inf in fp32", -1, dict(gain=1e60)),
           ("in_first < 0", -1, dict(in_first=-1)), ("in_count < 0", -1, dict(in_count=-1)), ("out_first < 0", -1, dict(out_first=-1)),
           ("n_out < 0", -1, dict(n_out=-1)), ("in_first > 2^48", -1, dict(in_first=2 ** 48 + 1)), ("in_count > 2^48", -1, dict(in_count=2 ** 48 + 1)),
           ("out_first > 2^48", -1, dict(out_first=2 ** 48 + 1)), ("n_out > 2^48", -1, dict(n_out=2 ** 48 + 1)),
           ("2-bit I/Q from sample 1", -1, dict(name="2sm", in_first=1, out_first=1, n_out=50)),
           ("1-bit real from sample 4", -1, dict(name="1ob", real=1, in_first=4, out_first=20, n_out=10)),
           ("fmt NULL", -1, dict(fmt=None)), ("in NULL", -1, dict(inp=None)), ("out NULL", -1, dict(out=None)),
           # an input that is needed and not present
           ("I/Q one short at the end", -6, dict(n_out=101)), ("I/Q one before in_first", -6, dict(in_first=8, out_first=7, n_out=50)),
           ("I/Q nothing present", -6, dict(in_count=0)),
           ("real one short at the end", -6, dict(real=1, in_count=2 * 9 + 21, n_out=10)),
           ("real 21 short at the end", -6, dict(real=1, in_count=2 * 9 + 1, n_out=10)),
           ("real one before in_first", -6, dict(real=1, in_first=16, in_count=184, out_first=18, n_out=10)),
           ("real below 0 is zero, but 0 must be there", -6, dict(real=1, in_first=16, in_count=184, out_first=5, n_out=10))]
    return out


def raw_call(ctx, in_ptr, out_ptr, name="s8", container=None, bits=None, real=0, in_first=0, in_count=100, out_first=0, n_out=100, gain=1.0, cplx=0,
             fmt="default", inp="default", out="default"):
    """gacq_ingest_dev on 200 bytes of input: by default 100 s8 I/Q samples to 100 outputs (real=1: give in_count and n_out)"""
    st = _fmt(name, real=bool(real))
    if container is not None:
        st.container = container
        st.real = real
    if bits is not None:
        st.bits = bits
    return nat.lib.gacq_ingest_dev(ctx, None if fmt is None else ctypes.addressof(st), ctypes.c_void_p(None if inp is None else in_ptr), in_first, in_count,
                                   out_first, n_out, gain, cplx, ctypes.c_void_p(None if out is None else out_ptr))


def test_every_refusal_without_a_device():
    """a NULL context: nothing may be touched, every call comes back with an error"""
    src = np.ones(256, dtype=np.int8)
    buf = np.zeros(1024, dtype=np.int8)
    assert raw_call(None, src.ctypes.data, buf.ctypes.data) < 0
    for label, code, change in bad_calls():
        assert raw_call(None, src.ctypes.data, buf.ctypes.data, **change) < 0, label
    assert not buf.any()


def test_command_line_parsing_and_the_printed_rates():
    a, f = ingest.parse(["--format", "2sm", "--real", "in.bin", "8.184e6", "2.046e6", "out.bin"])
    assert (a.input_filename, a.fs, a.coffset, a.output_filename, a.gain, a.target_rms, a.complex64) == ("in.bin", 8.184e6, 2.046e6, "out.bin", None, 32.0, False)
    assert f.real and not f.conj and f.msb_first and f.lut == [1, 3, -1, -3]
    assert ingest.report_line(f, a.fs, a.coffset, 2.5, 1000) == "fs 4092000.0 coffset 0.0 gain 2.5 samples 1000"
    assert f.rates(16.3676e6, 4.1304e6) == (16.3676e6 / 2, 4.1304e6 - 16.3676e6 / 4)
    a, f = ingest.parse(["--format", "2ob", "--lsb-first", "--lut", "-3,-1,1,3", "--conj", "--gain", "4", "--complex64", "-", "6e6", "-250000", "-"])
    assert not f.msb_first and f.conj and f.lut == [-3, -1, 1, 3] and a.gain == 4.0 and a.complex64 and a.coffset == -250000.0
    assert f.rates(a.fs, a.coffset) == (6.0e6, 250000.0)                                    # --conj negates the offset
    assert ingest.Format("s8", real=True, conj=True).rates(8.0e6, 2.5e6) == (4.0e6, -500000.0)
    a, f = ingest.parse(["--format", "s16", "--target-rms", "20", "x", "4e6", "0", "y"])
    assert a.target_rms == 20.0 and a.gain is None and f.container == ingest.S16
    for bad in (["--format", "s24", "x", "4e6", "0", "y"], ["--format", "s16", "--real", "x", "4e6", "0", "y"], ["--format", "s8", "x", "0", "0", "y"],
                ["--format", "s8", "--gain", "0", "x", "4e6", "0", "y"], ["--format", "s8", "--gain", "2", "--target-rms", "3", "x", "4e6", "0", "y"],
                ["--format", "2sm", "--lut", "1,2", "x", "4e6", "0", "y"], ["x", "4e6", "0", "y"]):
        with pytest.raises(SystemExit):
            ingest.parse(bad)


def test_automatic_gain_of_the_oracle_brings_gaussian_input_to_the_target():
    for f, data in C.gaussian_recordings().values():
        g = O.auto_gain(f, data)
        x = O.evaluate(f, data, g, 0, 0, O.AUTO_SAMPLES).astype(np.float64)
        rms = np.sqrt(np.mean(x[0::2] ** 2 + x[1::2] ** 2))
        print(f["container"], "gain %.6g rms %.3f" % (g, rms))
        assert abs(rms - 32.0) <= 0.05 * 32.0


def test_scene_of_the_pipeline_test_is_found_by_the_acquisition_oracle():
    """4 ms of the real 2-bit GPS L1 scene through the ingest oracle, then the reference's search at the output rate: the true
    Doppler bin and the code phase within one output sample"""
    s = C.SCENE
    chips = codes_oracle.chips("gps.ca", s["prn"])
    ms, per_ms = 4, 4092
    x = C.scene_real_samples(chips, 2 * ms * per_ms + 64)
    data = C.pack_msb_first(C.quantise_2sm(x, s["sigma"]), 2).tobytes()
    f = O.fmt("2sm", real=True)
    u = O.evaluate(f, data, O.auto_gain(f, data), 0, 0, ms * per_ms, "complex64")
    grid = [-2000.0, 2200.0, 200.0]
    metric, code, doppler = acq_oracle.search(u.astype(np.complex128), chips, grid, ms, fs=s["fs"] / 2.0, n=per_ms, normalised=True)
    print("metric %.1f code %.3f doppler %.0f" % (metric, code, doppler))
    assert doppler == 1200.0                                        # the bin nearest to 1234.5 Hz: IF - fs/4 = 0
    assert abs((code - s["code0"] + 511.5) % 1023.0 - 511.5) <= 1023.0 / per_ms
