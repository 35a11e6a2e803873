"""CPU: the host side of the utilities (spectrum, squaring, cn0) -- restatements against the reference's goldens, the chunk start
phases, command-line parsing, the file readers at end of file, and the argument checks of the two C entry points (no launch)."""
import ctypes
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import utilities_cases as C
import utilities_oracle as O
from gnss_dsp_tools_amd import _native as nat
from gnss_dsp_tools_amd import cn0, rawfile, spectrum, squaring, trackloop

GOLDEN = C.load()
ROOT = os.path.dirname(C.HERE)


@pytest.mark.parametrize("case", sorted(C.SPECTRUM))
def test_fp64_spectrum_restatement_matches_reference_frames(case):
    g = GOLDEN["spectrum"][case]
    n, ns, frames, fc, fs = C.SPECTRUM[case]
    assert (g["n"], g["ns"], g["frames"], g["fc"], g["fs"]) == (n, ns, frames, fc, fs)
    x = C.checked_recording(GOLDEN, "spectrum", case)
    want = C.unpack(g["db"], np.float64).reshape(frames, n)
    got = O.psd_fp64(x, n, ns)               # drops the trailing half frame of the recording
    assert got.shape == want.shape
    assert np.max(np.abs(got - want)) <= 1e-9
    assert 0 < g["complex64_deviation_db"] < 1e-4


def test_golden_covers_every_kernel_length_and_ns_from_1_to_50():
    ns = {C.SPECTRUM[c][0]: C.SPECTRUM[c][1] for c in C.SPECTRUM}
    assert set(spectrum.KERNEL_LENGTHS) == {64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384} and set(spectrum.KERNEL_LENGTHS) <= set(ns)
    assert min(ns.values()) == 1 and max(ns.values()) >= 50
    assert any(n not in spectrum.KERNEL_LENGTHS for n in ns)


def test_freq_axis_mhz():
    x = spectrum.freq_axis_mhz(1584754875.0, 69984000.0, 2048)
    assert x.shape == (2048,) and x.dtype == np.float64
    assert x[1024] == 1584754875.0 / 1e6
    assert x[0] == (1584754875.0 - 69984000.0 / 2) / 1e6
    np.testing.assert_allclose(np.diff(x), 69984000.0 / 2048 / 1e6, rtol=1e-9)
    odd = spectrum.freq_axis_mhz(0.0, 1000.0, 5)
    np.testing.assert_array_equal(odd, (np.arange(5) - 2.5) * 200.0 / 1e6)


@pytest.mark.parametrize("case", sorted(C.SQUARING))
def test_fp64_squaring_restatement_against_reference(case):
    """The restatement is complex128 throughout (the compiled program); the reference as run for the golden sums in complex64, so
    the two differ by what the generator measured -- and by no more."""
    g = GOLDEN["squaring"][case]
    b, n, m, chunks, fs, coffset = C.SQUARING[case]
    x = C.checked_recording(GOLDEN, "squaring", case)
    r_ref = C.unpack(g["r"], np.complex128).reshape(chunks, b)
    stream_ref = C.unpack(g["stream"], np.int16)
    r, stream, clamped = O.squaring_fp64(x, fs, coffset, b, n, m)
    assert clamped == 0 and r.shape == r_ref.shape
    # the stored difference to a few ulp of 20 r: another numpy build may add the n products of a boxcar in another order
    assert abs(np.max(np.abs(20 * r - 20 * r_ref)) - g["max_diff_20r"]) <= 8 * np.finfo(np.float64).eps * np.max(np.abs(20 * r_ref))
    assert g["max_diff_20r"] <= 2e-7 * np.max(np.abs(20 * r_ref))
    ok, share = C.stream_check(stream, stream_ref, r_ref, C.HALF_FACTOR * g["max_diff_20r"])
    assert ok and share <= C.HALF_SHARE, (ok, share)


def test_phase_case_has_three_chunks_and_a_fractional_phase_step():
    b, n, m, chunks, fs, coffset = C.SQUARING["script"]
    assert (b, n, m) == (squaring.B, squaring.N, squaring.M) == (1000, 16, 100) and chunks >= 3
    step = b * n * m * coffset / fs
    assert abs(step - round(step)) > 0.1


@pytest.mark.parametrize("case", sorted(C.SQUARING))
def test_chunk_start_phases_equal_the_scripts_expression(case):
    b, n, m, chunks, fs, coffset = C.SQUARING[case]
    chunk = b * n * m
    got, after = squaring.chunk_phases(chunks + 2, chunk, fs, coffset)
    coffset_phase = 0.0
    for c in range(chunks + 2):
        assert got[c] == coffset_phase and 0.0 <= got[c] < 1.0
        coffset_phase = coffset_phase - chunk * coffset / fs
        coffset_phase = np.mod(coffset_phase, 1)
    assert after == coffset_phase
    # a second call that starts where the first ended continues the sequence (the command line's pieces)
    head, mid = squaring.chunk_phases(2, chunk, fs, coffset)
    tail, _ = squaring.chunk_phases(chunks, chunk, fs, coffset, mid)
    np.testing.assert_array_equal(np.concatenate([head, tail]), got)
    np.testing.assert_array_equal(got[:chunks], O.chunk_phase_sequence(chunks, chunk, fs, coffset))


def test_command_line_parsing():
    a = squaring.parse(["/dev/stdin", "69984000", "-9334875"])
    assert (a.filename, a.fs, a.coffset) == ("/dev/stdin", 69984000.0, -9334875.0)
    a = squaring.parse(["f.iq", "4e6", "1.5e5"])
    assert (a.fs, a.coffset) == (4e6, 1.5e5)
    with pytest.raises(SystemExit):
        squaring.parse(["f.iq", "4e6"])
    s = spectrum.parse(["/dev/stdin", "1584754875", "69984000", "2048", "1000"])
    assert (s.filename, s.fc, s.fs, s.n, s.ns, s.out, s.plot) == ("/dev/stdin", 1584754875.0, 69984000.0, 2048, 1000, None, False)
    s = spectrum.parse(["f.iq", "-1e6", "4e6", "1000", "3", "--out", "o.f64", "--plot"])
    assert (s.fc, s.n, s.ns, s.out, s.plot) == (-1e6, 1000, 3, "o.f64", True)
    with pytest.raises(SystemExit):
        spectrum.parse(["f.iq", "0", "4e6", "0", "3"])
    assert cn0.parse([]) == 300 and cn0.parse(["--time", "2000"]) == 2000
    assert cn0.parse(["track.dat", "--time", "50"]) == 300          # interspersed arguments disabled, as in the script
    assert spectrum.frame_line(3, np.array([1.0, 2.0, 3.0]), np.array([-1.0, 7.25, 0.5])) == "3 2.000000 7.250 0.500"


@pytest.mark.parametrize("name", sorted(GOLDEN["cn0"]))
def test_cn0_lines_equal_the_scripts(name):
    if name == "synthetic":
        lines = C.cn0_synthetic_lines()
        assert C.sha256(np.frombuffer("\n".join(lines).encode(), dtype=np.uint8)) == GOLDEN["cn0_synthetic_sha256"]
    else:
        with open(os.path.join(C.GOLD, "trackloop_cases.json")) as f:
            lines = json.load(f)["cases"][name.split("/", 1)[1]]["stdout_lines"]
    for g in GOLDEN["cn0"][name]:
        argv = [] if g["time"] == 300 else ["--time", str(g["time"])]
        out = io.StringIO()
        got = cn0.run(argv, io.StringIO("".join(ln + "\n" for ln in lines)), out)
        assert got == g["lines"] and out.getvalue().split() == g["lines"]
        assert len(got) == len(lines) // g["time"] and len(got) >= 1
        assert O.cn0_lines(lines, g["time"]) == g["lines"]
        # the same numbers from a record array
        recs = np.zeros(len(lines), dtype=trackloop.RECORD_DTYPE)
        recs["p_re"] = [float(ln.split()[1]) for ln in lines]
        recs["p_im"] = [float(ln.split()[2]) for ln in lines]
        assert cn0.format_lines(cn0.from_records(recs, g["time"])) == g["lines"]


def test_cn0_uses_population_std_and_abs_of_the_real_part():
    x = np.array([3.0 + 1.0j, -5.0 - 1.0j, 4.0 + 3.0j, -4.0 - 3.0j])
    want = 20 * np.log10(4.0 / (np.sqrt(2) * np.sqrt(5.0))) + 30          # mean |I| = 4, Q = (1, -1, 3, -3): variance 5 with ddof 0
    assert abs(cn0.cn0(x) - want) < 1e-12
    assert cn0.from_records(np.zeros(7, dtype=trackloop.RECORD_DTYPE), 8).shape == (0,)


def test_cn0_module_runs_as_a_program():
    lines = C.cn0_synthetic_lines()
    p = subprocess.run([sys.executable, "-m", "gnss_dsp_tools_amd.cn0", "--time", "100"], input="".join(ln + "\n" for ln in lines), cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    want = [g["lines"] for g in GOLDEN["cn0"]["synthetic"] if g["time"] == 100][0]
    assert p.stdout.split() == want


class _Dribble(io.RawIOBase):
    """a pipe that hands out at most 7 bytes per read"""
    def __init__(self, data):
        self.data, self.at = data, 0

    def read(self, n=-1):
        k = min(7, len(self.data) - self.at) if n < 0 else min(7, n, len(self.data) - self.at)
        self.at += k
        return self.data[self.at - k:self.at]


def test_file_readers_drop_a_trailing_partial_unit_and_stop():
    data = bytes(range(256)) * 4                                   # 1024 bytes
    for unit, piece in ((100, 250), (100, 1 << 20), (1024, 10), (1025, 4096), (64, 64)):
        for fp in (io.BytesIO(data), _Dribble(data)):
            got = list(rawfile.read_pieces(fp, unit, piece))
            whole = (len(data) // unit) * unit
            assert all(len(p) % unit == 0 and 0 < len(p) <= max(unit, piece) and p.dtype == np.int8 for p in got)
            assert b"".join(p.tobytes() for p in got) == data[:whole]
    assert list(rawfile.read_pieces(io.BytesIO(b""), 8)) == []
    with pytest.raises(ValueError):
        list(rawfile.read_pieces(io.BytesIO(data), 0))


def _err():
    return nat.lib.gacq_last_error(None).decode()


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """No context exists without a GPU: every call here must come back with GACQ_ERR_BAD_ARG and the reason, never crash."""
    lib = nat.lib
    buf = np.zeros(1 << 16, dtype=np.int8)
    p = ctypes.c_void_p(buf.ctypes.data)
    for n in (0, -64, 32, 63, 96, 1000, 32768, 1 << 20):
        assert lib.gacq_psd_int8_dev(None, p, 1, n, 4, p, 0, p) == -1 and "power of two" in _err(), n
    assert lib.gacq_psd_int8_dev(None, p, 1, 64, 0, p, 0, p) == -1 and "no frames" in _err()
    assert lib.gacq_psd_int8_dev(None, p, 0, 64, 4, p, 0, p) == -1 and "no frames" in _err()
    assert lib.gacq_psd_int8_dev(None, p, 1, 64, 4, p, -1, p) == -1 and "split" in _err()
    assert lib.gacq_psd_int8_dev(None, p, 1, 64, 4, p, 0, p) == -1 and "NULL" in _err()            # the context
    assert lib.gacq_psd_int8_dev(None, None, 1, 64, 4, p, 0, p) == -1 and "NULL" in _err()
    ph = ctypes.c_void_p(buf.ctypes.data)
    for chunk, n, m in ((1601, 16, 100), (0, 16, 100), (1600, 0, 100), (1600, 16, 0), (1600, -16, -100), (100, 16, 100)):
        assert lib.gacq_squaring_int8_dev(None, p, 1, chunk, n, m, ph, -0.1, p, p, p) == -1 and "multiple of n*m" in _err(), (chunk, n, m)
    assert lib.gacq_squaring_int8_dev(None, p, 0, 1600, 16, 100, ph, -0.1, p, p, p) == -1 and "no chunks" in _err()
    for f in (float("nan"), float("inf"), 8.0):
        assert lib.gacq_squaring_int8_dev(None, p, 1, 1600, 16, 100, ph, f, p, p, p) == -1 and "cycles per sample" in _err()
    assert lib.gacq_squaring_int8_dev(None, p, 1, 1600, 16, 100, ph, -0.1, p, p, p) == -1 and "NULL" in _err()
    assert lib.gacq_squaring_int8_dev(None, p, 1, 1600, 16, 100, None, -0.1, p, p, None) == -1 and "NULL" in _err()
