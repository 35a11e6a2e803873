"""CPU: the numpy definition of the down-converter (tests/ddc_oracle.py) against its own bounds and the filter's promises, the
library's table, default taps, phase increments and rates against the oracle's, the refusals of gacq_ddc_check without a device, the
command line's parser and report lines, and the pipeline test's scene through the oracle and the reference search."""
import ctypes

import numpy as np
import pytest

import ddc_cases as C
import ddc_oracle as O
from gnss_dsp_tools_amd import _native as nat
from gnss_dsp_tools_amd import ddc
from oracle import acq_oracle, codes_oracle

BAD_ARG, SHORT_INPUT = -1, -6
DEFAULT_D = (2, 3, 4, 8, 16, 32, 64)


def test_table_is_numpys():
    w = ddc.table()
    assert w.dtype == np.int16 and w.shape == (4096, 2) and np.array_equal(w, O.table())
    assert tuple(w[0]) == (16384, 0) and tuple(w[1024]) == (0, 16384) and tuple(w[2048]) == (-16384, 0)


def test_default_taps_are_the_oracles_and_sum_to_unity():
    for D in range(1, 65):
        g = ddc.design_taps(D)
        assert g.dtype == np.int32 and np.array_equal(g, O.design_taps(D)) and int(g.sum()) == 32768, D
        assert len(g) == (1 if D == 1 else 8 * D + 1) and int(np.abs(g).sum()) <= 65536
    assert ddc.design_taps(1).tolist() == [32768]
    for D, T in C.SHAPES:
        assert np.array_equal(ddc.design_taps(D, T), O.design_taps(D, T)), (D, T)
    # a cutoff in Hz: 0.4 fs / D is the default
    assert np.array_equal(ddc.design_taps(8, cutoff_hz=0.4 * 8.0e6 / 8, fs=8.0e6), ddc.design_taps(8))
    assert np.array_equal(ddc.design_taps(1, cutoff_hz=1.0e6, fs=8.0e6), O.design_taps(1, 9, 0.25))
    for bad in (dict(D=0), dict(D=65), dict(D=4, T=32), dict(D=4, T=515), dict(D=4, cutoff_hz=1.0e6), dict(D=4, cutoff_hz=5.0e6, fs=8.0e6)):
        with pytest.raises(ValueError):
            ddc.design_taps(**bad)


def test_mixed_samples_fit_an_int16_pair_exhaustively():
    """every int8 pair against every table entry: |z| <= 23171"""
    w = O.table().astype(np.int64)
    v = np.arange(-128, 128, dtype=np.int64)
    top = 0
    for xr in (-128, 127):                                   # the extremes of one component bound the product; the other runs through all
        pr = xr * w[:, 0][:, None] + v[None, :] * w[:, 1][:, None]
        pi = v[None, :] * w[:, 0][:, None] - xr * w[:, 1][:, None]
        top = max(top, int(np.max(np.abs((pr + 64) >> 7))), int(np.max(np.abs((pi + 64) >> 7))))
    xr, xi = np.meshgrid(v, v, indexing="ij")
    for t in range(0, 4096, 7):                              # and every pair against a spread of entries
        pr, pi = xr * w[t, 0] + xi * w[t, 1], xi * w[t, 0] - xr * w[t, 1]
        top = max(top, int(np.max(np.abs((pr + 64) >> 7))), int(np.max(np.abs((pi + 64) >> 7))))
    print("max |z| = %d" % top)
    assert top <= 23171 and 23171 * 65536 < 2 ** 31


@pytest.mark.parametrize("D", DEFAULT_D)
def test_default_filter_keeps_its_passband_and_stopband(D):
    g = O.design_taps(D)
    assert int(np.abs(g).sum()) <= 65536
    f_pass = np.linspace(0.0, 0.2, 201)
    f_stop = np.linspace(0.6, D / 2.0, 40 * D + 1)          # up to the input's Nyquist rate
    p, s = O.response_db(g, D, f_pass), O.response_db(g, D, f_stop)
    print("D %d: sum |g| %d, passband %.3f .. %.3f dB, stopband at most %.1f dB" % (D, int(np.abs(g).sum()), p.min(), p.max(), s.max()))
    assert p.min() >= -0.1 and p.max() <= 0.1
    assert s.max() <= -40.0


def _tone_out(freq, amp=100.0):
    """amplitude of the D = 8 default band's output for a tone `freq` (in output rates) above the shift"""
    D, fs, shift = 8, 8.0e6, 1.0e6
    g = O.design_taps(D)
    n = 8 * 4000 + len(g)
    j = np.arange(n, dtype=np.float64)
    x = amp * np.exp(2j * np.pi * np.mod((shift + freq * fs / D) * j / fs, 1.0))
    v = np.empty(2 * n, dtype=np.int8)
    v[0::2], v[1::2] = np.rint(x.real), np.rint(x.imag)
    u = O.evaluate(shift, fs, D, g, v, 1.0, 0, 100, 3000, "complex64").astype(np.complex128)
    return float(np.sqrt(np.mean(np.abs(u) ** 2)))


def test_a_tone_in_the_band_passes_and_one_outside_does_not_alias():
    inband, alias = _tone_out(0.05), _tone_out(0.9)
    print("in-band tone of 100 comes out at %.2f, the tone at 0.9 fs_out at %.2f" % (inband, alias))
    assert abs(inband - 100.0) <= 1.0
    assert alias < 1.0


def test_phase_increments_and_rates():
    fs = 32.736e6
    assert ddc.phase_increment(fs / 8.0, fs) == O.phase_increment(fs / 8.0, fs) == 1 << 61
    b = ddc.Band(fs / 8.0, 8)
    assert b.rates(fs, 4.092e6) == (4.092e6, 0.0) == O.rates(fs / 8.0, 8, fs, 4.092e6)
    assert b.rates(fs, 1.0e6) == (fs / 8.0, 1.0e6 - fs / 8.0)
    # a negative shift: dP in the upper half, the applied shift negative
    assert ddc.phase_increment(-fs / 4.0, fs) == O.phase_increment(-fs / 4.0, fs) == 3 << 62
    assert ddc.Band(-fs / 4.0, 2).rates(fs, 0.0) == (fs / 2.0, fs / 4.0)
    dp = ddc.phase_increment(-1.0e-3, C.FS)
    assert dp == O.phase_increment(-1.0e-3, C.FS) and dp >> 44 == (1 << 20) - 1
    # no exact ratio: the increment is the rounded quotient, the reported offset is that of the shift actually applied
    for f, rate in ((1.2345678e6, C.FS), (-7.1e6 / 3.0, 16.3676e6), (0.1, 1.0e7)):
        dp = ddc.phase_increment(f, rate)
        assert dp == O.phase_increment(f, rate)
        exact = f / rate * 2.0 ** 64
        assert abs(O.signed(dp) - exact) <= max(1.0, abs(exact) * 2.0 ** -51)
        got = ddc.Band(f, 4).rates(rate, 2.5e6)
        assert got == O.rates(f, 4, rate, 2.5e6) and abs(got[1] - (2.5e6 - f)) <= 1e-6 and got[0] == rate / 4
    assert ddc.phase_increment(0.0, fs) == 0 and ddc.Band(0.0, 1).rates(fs, 5.0) == (fs, 5.0)


def raw_check(D=4, taps=None, T=None, dphase=12345, in_first=0, in_count=1000, out_first=0, n_out=100, gain=1.0, cplx=0, cfg=True, null_taps=False,
              handle=None, src=1 << 20, dst=1 << 21):
    """gacq_ddc_check (no device), or with a handle gacq_ddc_run_dev; the addresses are only looked at by the checks"""
    if handle is not None:
        return nat.lib.gacq_ddc_run_dev(handle, ctypes.c_void_p(src), in_first, in_count, out_first, n_out, gain, cplx, ctypes.c_void_p(dst))
    g = np.ascontiguousarray(O.design_taps(4, 33) if taps is None else taps, dtype=np.int32)
    st = ddc.DdcCfg(dphase=dphase, decim=D)
    return nat.lib.gacq_ddc_check(ctypes.addressof(st) if cfg else None, None if null_taps else ctypes.c_void_p(g.ctypes.data), len(g) if T is None else T,
                                  in_first, in_count, out_first, n_out, gain, cplx)


def bad_config_calls():
    """(label, expected code, changed arguments): what gacq_ddc_check and gacq_ddc_open refuse"""
    big = np.zeros(33, dtype=np.int64)
    big[0], big[5] = 40000, -25537
    out = [("NULL cfg", BAD_ARG, dict(cfg=False)), ("NULL taps", BAD_ARG, dict(null_taps=True)), ("sum |g| 65537", BAD_ARG, dict(taps=big))]
    out += [("D %d" % v, BAD_ARG, dict(D=v)) for v in (0, -1, 65)]
    out += [("T %d" % v, BAD_ARG, dict(T=v)) for v in (0, -1, 32, 2)] + [("T 515", BAD_ARG, dict(taps=np.ones(515, dtype=np.int64)))]
    return out


def bad_run_calls():
    """... and what gacq_ddc_check and gacq_ddc_run_dev refuse; the default call is D = 4, T = 33, 1000 inputs from 0, outputs 0 .. 99"""
    nan, inf = float("nan"), float("inf")
    out = [("gain %r" % v, BAD_ARG, dict(gain=v)) for v in (0.0, -1.0, nan, inf, 1e39, 1e-46)]
    for k in ("in_first", "in_count", "out_first", "n_out"):
        out += [("%s %s" % (k, v), BAD_ARG, {k: v}) for v in (-1, (1 << 48) + 1)]
    out += [("one short at the end", SHORT_INPUT, dict(in_count=99 * 4 + 16)), ("nothing present", SHORT_INPUT, dict(in_count=0)),
            ("input starts one late", SHORT_INPUT, dict(in_first=25, in_count=975, out_first=10, n_out=50)),
            ("below 0 is zero, but 0 must be there", SHORT_INPUT, dict(in_first=1, in_count=999, out_first=3, n_out=50))]
    return out


def test_every_refusal_through_gacq_ddc_check_without_a_device():
    for label, code, change in bad_config_calls() + bad_run_calls():
        assert raw_check(**change) == code, (label, nat.lib.gacq_last_error(None))
        assert nat.lib.gacq_last_error(None).startswith(b"gacq_ddc: "), label       # every message names its own tool
    assert raw_check() == 0 and raw_check(in_count=99 * 4 + 17) == 0 and raw_check(n_out=0, in_count=0) == 0
    assert raw_check(in_first=24, in_count=976, out_first=10, n_out=50) == 0
    good = np.zeros(33, dtype=np.int64)
    good[0], good[5] = 40000, -25536
    assert raw_check(taps=good) == 0 and raw_check(D=1, taps=[32768], in_count=100) == 0 and raw_check(D=64, taps=np.ones(513), in_count=99 * 64 + 257) == 0
    assert nat.lib.gacq_ddc_run_dev(None, ctypes.c_void_p(1 << 20), 0, 1000, 0, 100, 1.0, 0, ctypes.c_void_p(1 << 21)) == BAD_ARG      # no handle
    h = ctypes.c_void_p()
    st = ddc.DdcCfg(dphase=1, decim=4)
    g = np.ascontiguousarray(O.design_taps(4, 33), dtype=np.int32)
    assert nat.lib.gacq_ddc_open(None, ctypes.addressof(st), ctypes.c_void_p(g.ctypes.data), 33, ctypes.byref(h)) == BAD_ARG and not h.value
    assert nat.lib.gacq_ddc_table(None) == BAD_ARG
    assert [nat.lib.gacq_ddc_tile(D) for D in (1, 8, 9, 16, 17, 32, 33, 64)] == [C.tile(D) for D in (1, 8, 9, 16, 17, 32, 33, 64)]
    assert [nat.lib.gacq_ddc_tile(D) for D in (0, -3, 65)] == [BAD_ARG] * 3
    assert ctypes.sizeof(ddc.DdcCfg) == 16


def test_out_range_of_the_module_is_the_oracles():
    for D, T in ((1, 1), (4, 33), (5, 3), (64, 513)):
        b = ddc.Band(0.0, D, taps=O.design_taps(D, T))
        for in_first in (0, 1, 7, 256, 257, 1000):
            for count in (0, 1, 2, 256, 257, 512, 513, 514, 5000):
                first, n = b.out_range(in_first, count)
                assert (first, n) == O.out_range(D, T, in_first, count)
                if n:
                    lo, hi = O.needed(D, T, first, n)
                    assert in_first <= lo and hi < in_first + count and b.first_needed(first) == lo
                    assert O.needed(D, T, first, n + 1)[1] >= in_first + count
                    assert in_first == 0 or O.needed(D, T, first - 1, 1)[0] < in_first or first == 0
    # a recording of N samples ends at output (N - 1 - H) div D
    assert ddc.Band(0.0, 8).out_range(0, 100000) == (0, (100000 - 1 - 32) // 8 + 1)


def test_command_line_parser_and_report_lines():
    a, bands, outs = ddc.parse(["--decim", "8", "--band", "4.092e6", "l1.iq", "in.iq", "32.736e6", "4.092e6"])
    assert (a.input_filename, a.fs, a.coffset, a.gain, a.target_rms, a.complex64, outs) == ("in.iq", 32.736e6, 4.092e6, None, 32.0, False, ["l1.iq"])
    assert len(bands) == 1 and (bands[0].f_shift, bands[0].D, bands[0].T) == (4.092e6, 8, 65)
    assert ddc.report_line(bands[0], a.fs, a.coffset, 2.5, 1000) == "band 4092000.0 fs 4092000.0 coffset 0.0 gain 2.5 samples 1000"
    a, bands, outs = ddc.parse(["--decim", "16", "--taps", "97", "--cutoff", "1.5e6", "--gain", "3", "--complex64", "--band", "-562500", "a", "--band",
                                "1.125e6", "b", "-", "65.472e6", "0"])
    assert a.gain == 3.0 and a.complex64 and a.input_filename == "-" and outs == ["a", "b"] and [b.f_shift for b in bands] == [-562500.0, 1.125e6]
    assert all(b.T == 97 and b.D == 16 and b.cutoff_hz == 1.5e6 for b in bands)
    assert np.array_equal(bands[0].taps_for(a.fs), O.design_taps(16, 97, 1.5e6 / (0.5 * 65.472e6)))
    line = ddc.report_line(bands[0], a.fs, a.coffset, 3.0, 7)
    assert line == "band -562500.0 fs 4092000.0 coffset %r gain 3.0 samples 7" % O.rates(-562500.0, 16, 65.472e6, 0.0)[1]
    assert abs(O.rates(-562500.0, 16, 65.472e6, 0.0)[1] - 562500.0) <= 1e-6
    assert ddc.parse(["--decim", "1", "--band", "1e6", "-", "-", "4e6", "0"])[2] == ["-"]
    assert ddc.parse(["--decim", "2", "--band", "-1.0e6", "o", "in", "4e6", "-2.5e5"])[1][0].f_shift == -1.0e6
    for bad in (["--band", "1e6", "o", "in", "4e6", "0"], ["--decim", "65", "--band", "1e6", "o", "in", "4e6", "0"], ["--decim", "4", "in", "4e6", "0"],
                ["--decim", "4", "--taps", "32", "--band", "1e6", "o", "in", "4e6", "0"], ["--decim", "4", "--band", "1e6", "o", "in", "0", "0"],
                ["--decim", "4", "--gain", "0", "--band", "1e6", "o", "in", "4e6", "0"], ["--decim", "4", "--cutoff", "3e6", "--band", "1e6", "o", "in", "4e6", "0"],
                ["--decim", "4", "--gain", "2", "--target-rms", "3", "--band", "1e6", "o", "in", "4e6", "0"],
                ["--decim", "4", "--band", "1e6", "-", "--band", "2e6", "o", "in", "4e6", "0"], ["--decim", "4", "--band", "x", "o", "in", "4e6", "0"]):
        with pytest.raises((SystemExit, ValueError)):
            ddc.parse(bad)


@pytest.mark.parametrize("ts", [C.TAP_SETS[3], C.TAP_SETS[6], C.TAP_SETS[8]], ids=lambda ts: ts.name)
def test_the_oracle_does_not_depend_on_how_the_input_is_cut(ts):
    T = len(ts.taps)
    n_out = 300
    lo, hi = O.needed(ts.D, T, 0, n_out)
    data = C.random_int8(hi + 1, 7)
    f = C.SHIFTS[2]
    whole = O.evaluate(f, C.FS, ts.D, ts.taps, data, C.GAIN, 0, 0, n_out, "complex64")
    parts, m = [], 0
    for n in (1, 99, 200):
        lo, hi = O.needed(ts.D, T, m, n)
        parts.append(O.evaluate(f, C.FS, ts.D, ts.taps, data[2 * lo:2 * (hi + 1)], C.GAIN, lo, m, n, "complex64"))
        m += n
    assert np.array_equal(np.concatenate(parts).view(np.float32), whole.view(np.float32))
    assert np.array_equal(O.evaluate(f, C.FS, ts.D, ts.taps, data, C.GAIN), O.to_int8(whole))          # every output the data supports: the same 300


def test_scene_of_the_pipeline_test_is_found_by_the_acquisition_oracle():
    """4 ms of the scene through the oracle's down-converter, then the reference's search at the output rate: the true Doppler bin and
    the code phase within one output sample"""
    s = C.SCENE
    chips = codes_oracle.chips("gps.ca", s["prn"])
    ms, per_ms = 4, 4092
    g = O.design_taps(s["D"])
    raw = C.scene_int8(chips, s["D"] * ms * per_ms + len(g))
    gain = O.auto_gain(s["coffset"], s["fs"], s["D"], g, raw)
    u = O.evaluate(s["coffset"], s["fs"], s["D"], g, raw, gain, 0, 0, ms * per_ms, "int8").astype(np.float64)
    assert O.rates(s["coffset"], s["D"], s["fs"], s["coffset"]) == (4.092e6, 0.0)
    rms = float(np.sqrt(np.mean(u[0::2] ** 2 + u[1::2] ** 2)))
    metric, code, doppler = acq_oracle.search(u[0::2] + 1j * u[1::2], chips, [-2000.0, 2200.0, 200.0], ms, fs=4.092e6, n=per_ms, normalised=True)
    print("gain %.4f rms %.2f: metric %.1f code %.3f doppler %.0f" % (gain, rms, metric, code, doppler))
    assert abs(rms - 32.0) <= 0.05 * 32.0
    assert doppler == 1200.0                                        # the bin nearest to 1234.5 Hz
    assert abs((code - s["code0"] + 511.5) % 1023.0 - 511.5) <= 1023.0 / per_ms
