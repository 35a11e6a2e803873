"""GPU: the Welch spectrum and squaring kernels (csrc/gacq_spectrum.hip) and the three utilities' command lines against the
reference's goldens (tools/make_goldens_utilities.py) and the fp64 restatements of tests/utilities_oracle.py.

Bounds.  Spectrum, kernel lengths: four times the deviation of a CPU complex64 transform from the reference's fp64 frames, measured
per case by the generator (the factor covers a radix order and twiddle tables that differ from pocketfft's); other lengths (torch.fft
in complex128): 1e-9 dB.  Squaring: r within 1e-12 of max |r| of the fp64 restatement (two fp64 sums in different orders, the bar
tests/test_track_loop_gpu.py uses) and the int16 stream identical to it; against the reference as run for the golden (complex64 inner
sums without numba) r within twice the generator's measured difference, the stream equal or off by one next to a half-integer."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest

import track_loop_cases as T
import utilities_cases as C
import utilities_oracle as O
from gnss_dsp_tools_amd import _native as nat
from gnss_dsp_tools_amd import cn0, spectrum, squaring, trackloop

GOLDEN = C.load()
ROOT = os.path.dirname(C.HERE)
KERNEL_CASES = sorted(c for c in C.SPECTRUM if C.SPECTRUM[c][0] in spectrum.KERNEL_LENGTHS)


def _frames(case):
    n, ns, frames, _, _ = C.SPECTRUM[case]
    return C.unpack(GOLDEN["spectrum"][case]["db"], np.float64).reshape(frames, n)


@pytest.mark.gpu
@pytest.mark.parametrize("case", KERNEL_CASES)
def test_spectrum_kernel_against_reference_frames(engine, case):
    n, ns, frames, _, _ = C.SPECTRUM[case]
    x = C.checked_recording(GOLDEN, "spectrum", case)
    got = spectrum.psd(x, n, ns, engine)
    want = _frames(case)
    bound = 4.0 * GOLDEN["spectrum"][case]["complex64_deviation_db"]
    assert got.shape == want.shape and got.dtype == np.float64
    dev = float(np.max(np.abs(got - want)))
    print("spectrum %s: n %d ns %d deviation %.3g dB, bound %.3g dB (complex64 on the CPU: %.3g dB)" % (case, n, ns, dev, bound, bound / 4))
    assert dev <= bound, (case, dev, bound)


@pytest.mark.gpu
def test_every_kernel_length_is_covered():
    assert sorted(C.SPECTRUM[c][0] for c in KERNEL_CASES) == [1 << k for k in range(6, 15)]


def _split_input(case):
    """a golden recording, or for the two largest lengths seeded noise with enough frames for several segments (the golden cases of
    8192 and 16384 have two segments and one)"""
    if case in C.SPECTRUM:
        n, ns, _, _, _ = C.SPECTRUM[case]
        return C.checked_recording(GOLDEN, "spectrum", case), n, ns
    n, ns = {"n8192_ns40": (8192, 40), "n16384_ns20": (16384, 20)}[case]
    rng = np.random.Generator(np.random.PCG64(n + ns))
    return rng.integers(-60, 61, size=2 * n * ns * 2).astype(np.int8), n, ns


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["n64", "n1024", "n2048", "n8192_ns40", "n16384_ns20"])
def test_spectrum_bits_do_not_depend_on_the_split_or_the_run(engine, case):
    x, n, ns = _split_input(case)
    assert -(-ns // max(8, -(-ns // 16))) >= 3                  # at least three segments, so a split really spreads them
    one = spectrum.psd(x, n, ns, engine, split=1)               # one workgroup per spectrum
    for split in (0, 2, 3, 16, 1000):
        np.testing.assert_array_equal(spectrum.psd(x, n, ns, engine, split=split).view(np.uint64), one.view(np.uint64))
    np.testing.assert_array_equal(spectrum.psd(x, n, ns, engine, split=1).view(np.uint64), one.view(np.uint64))
    np.testing.assert_array_equal(spectrum.psd(x, n, ns, engine).view(np.uint64), spectrum.psd(x, n, ns, engine).view(np.uint64))
    dev = float(np.max(np.abs(one - O.psd_fp64(x, n, ns))))
    print("split %s: deviation from the fp64 restatement %.3g dB" % (case, dev))
    assert dev < 1e-4                                           # fp32 transform: ~1e-6 of a bin's power; a misplaced segment moves dB


@pytest.mark.gpu
def test_many_spectra_in_one_call(engine):
    """300 spectra of 5 frames in one launch equal the same spectra computed one call each (nothing leaks between workgroups)."""
    rng = np.random.Generator(np.random.PCG64(5))
    n, ns, F = 256, 5, 300
    x = rng.integers(-40, 41, size=2 * n * ns * F).astype(np.int8)
    got = spectrum.psd(x, n, ns, engine)
    assert got.shape == (F, n)
    for f in (0, 1, 150, 299):
        np.testing.assert_array_equal(got[f], spectrum.psd(x[2 * n * ns * f:2 * n * ns * (f + 1)], n, ns, engine)[0])
    assert np.max(np.abs(got - O.psd_fp64(x, n, ns))) < 1e-4


@pytest.mark.gpu
def test_spectrum_other_lengths_go_through_torch_fft(engine):
    n, ns, frames, _, _ = C.SPECTRUM["n1000"]
    x = C.checked_recording(GOLDEN, "spectrum", "n1000")
    got = spectrum.psd(x, n, ns, engine)
    dev = float(np.max(np.abs(got - _frames("n1000"))))
    print("spectrum n1000 (torch.fft complex128): deviation %.3g dB" % dev)
    assert got.shape == (frames, n) and dev <= 1e-9


@pytest.mark.gpu
def test_zero_power_gives_minus_infinity(engine):
    got = spectrum.psd(np.zeros(2 * 512 * 3, dtype=np.int8), 512, 3, engine)
    assert got.shape == (1, 512) and np.all(np.isneginf(got))
    # a constant input: everything but the three bins the Hann window reaches is (numerically) empty, and nothing faults
    dc = spectrum.psd(np.full(2 * 64 * 2, 5, dtype=np.int8), 64, 2, engine)
    assert np.argmax(dc[0]) == 32 and not np.any(np.isnan(dc))
    assert spectrum.psd(np.zeros(100, dtype=np.int8), 64, 1, engine).shape == (0, 64)          # less than one group of frames


@pytest.mark.gpu
def test_numpy_and_device_tensor_inputs_agree(engine):
    torch = nat.require_torch()
    n, ns, _, _, _ = C.SPECTRUM["n512"]
    x = C.checked_recording(GOLDEN, "spectrum", "n512")
    xd = torch.from_numpy(x).to("cuda:%d" % engine.device)
    a, b = spectrum.psd(x, n, ns, engine), spectrum.psd(xd, n, ns, engine)
    np.testing.assert_array_equal(a.view(np.uint64), b.view(np.uint64))
    np.testing.assert_array_equal(spectrum.psd(x.reshape(-1, 2), n, ns, engine).view(np.uint64), a.view(np.uint64))
    # a misaligned view of a device tensor is accepted too
    pad = torch.zeros(x.size + 2, dtype=torch.int8, device=xd.device)
    pad[2:] = xd
    np.testing.assert_array_equal(spectrum.psd(pad[2:], n, ns, engine).view(np.uint64), a.view(np.uint64))
    bq, nq, mq, chunks, fs, coffset = C.SQUARING["n12"]
    s = C.checked_recording(GOLDEN, "squaring", "n12")
    sd = torch.from_numpy(s).to("cuda:%d" % engine.device)
    r1, y1, c1 = squaring.squaring(s, fs, coffset, bq, nq, mq, engine)
    r2, y2, c2 = squaring.squaring(sd, fs, coffset, bq, nq, mq, engine)
    np.testing.assert_array_equal(r1.view(np.uint64), r2.view(np.uint64))
    np.testing.assert_array_equal(y1, y2)
    assert c1 == c2 == 0


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(C.SQUARING))
def test_squaring_against_restatement_and_reference(engine, case):
    g = GOLDEN["squaring"][case]
    b, n, m, chunks, fs, coffset = C.SQUARING[case]
    x = C.checked_recording(GOLDEN, "squaring", case)
    r, stream, clamped = squaring.squaring(x, fs, coffset, b, n, m, engine)
    assert r.shape == (chunks, b) and r.dtype == np.complex128 and stream.shape == (2 * chunks * b,) and stream.dtype == np.int16
    # 1. the fp64 restatement
    r64, stream64, _ = O.squaring_fp64(x, fs, coffset, b, n, m)
    rel = float(np.max(np.abs(r - r64)) / np.max(np.abs(r64)))
    # 2. the reference as run for the golden
    r_ref = C.unpack(g["r"], np.complex128).reshape(chunks, b)
    d_ref = float(np.max(np.abs(20 * r - 20 * r_ref)))
    ok, share = C.stream_check(stream, C.unpack(g["stream"], np.int16), r_ref, C.HALF_FACTOR * g["max_diff_20r"])
    print("squaring %s: |r - r_fp64| / max|r| %.3g (bound 1e-12); |20 r - 20 r_ref| %.3g (bound %.3g); stream values off by one %.4f (cap %.2f)"
          % (case, rel, d_ref, 2 * g["max_diff_20r"], share, C.HALF_SHARE))
    assert clamped == 0
    assert rel <= 1e-12, (case, rel)
    np.testing.assert_array_equal(stream, stream64)
    assert d_ref <= 2 * g["max_diff_20r"], (case, d_ref, g["max_diff_20r"])
    assert ok and share <= C.HALF_SHARE, (case, ok, share)


@pytest.mark.gpu
def test_squaring_chunk_phases_matter_and_a_start_phase_continues_a_stream(engine):
    """The multi-chunk case: chunks 1 and 2 start at phases 0.3525... and 0.7051...; the same samples squared one chunk per call
    with the phase carried over give the same bits, and with the phase dropped they do not."""
    b, n, m, chunks, fs, coffset = C.SQUARING["script"]
    x = C.checked_recording(GOLDEN, "squaring", "script")
    chunk = 2 * b * n * m
    r, stream, _ = squaring.squaring(x, fs, coffset, engine=engine)
    phases, _ = squaring.chunk_phases(chunks, b * n * m, fs, coffset)
    assert phases[1] != 0.0 and phases[2] != 0.0
    for c in range(chunks):
        rc, yc, _ = squaring.squaring(x[c * chunk:(c + 1) * chunk], fs, coffset, engine=engine, phase=phases[c])
        np.testing.assert_array_equal(rc[0].view(np.uint64), r[c].view(np.uint64))
        np.testing.assert_array_equal(yc, stream[2 * b * c:2 * b * (c + 1)])
    wrong, _, _ = squaring.squaring(x[chunk:2 * chunk], fs, coffset, engine=engine)
    assert np.max(np.abs(wrong[0] - r[1])) > 1e-3 * np.max(np.abs(r[1]))


@pytest.mark.gpu
def test_squaring_clamps_and_counts_what_leaves_the_int16_range(engine):
    b, n, m = 6, 16, 100
    x = np.full(2 * b * n * m * 2, 127, dtype=np.int8)
    r, stream, clamped = squaring.squaring(x, 4.0e6, 0.0, b, n, m, engine)              # coffset 0: the NCO stays at table[0] = 1
    assert r.shape == (2, b)
    np.testing.assert_array_equal(r.real, 0.0)
    np.testing.assert_array_equal(r.imag, float(m * n * 2 * 127 * 127))
    np.testing.assert_array_equal(stream[0::2], 0)
    np.testing.assert_array_equal(stream[1::2], 32767)
    assert clamped == 2 * b
    _, low, cl = squaring.squaring(np.stack([x[0::2], -x[1::2]], axis=1), 4.0e6, 0.0, b, n, m, engine)
    np.testing.assert_array_equal(low[1::2], -32768)
    assert cl == 2 * b


@pytest.mark.gpu
def test_spectrum_command_line(engine, tmp_path):
    case = "n2048"
    n, ns, frames, fc, fs = C.SPECTRUM[case]
    x = C.checked_recording(GOLDEN, "spectrum", case)
    x2 = np.concatenate([x[:2 * n * ns * frames]] * 3 + [x[:n]])                         # three frames and a partial one
    path = tmp_path / "rec.iq"
    x2.tofile(path)
    out = tmp_path / "frames.f64"
    assert spectrum.run([str(path), repr(fc), repr(fs), str(n), str(ns), "--out", str(out)], engine=engine) == 3 * frames
    got = np.fromfile(out, dtype=np.float64).reshape(-1, n)
    want = np.concatenate([_frames(case)] * 3)
    bound = 4.0 * GOLDEN["spectrum"][case]["complex64_deviation_db"]
    assert got.shape == want.shape and np.max(np.abs(got - want)) <= bound
    # text mode, in this process and as a program: one line per frame, its figures derived from the golden frames
    text = io.StringIO()
    assert spectrum.run([str(path), repr(fc), repr(fs), str(n), str(ns)], text, engine) == 3 * frames
    p = subprocess.run([sys.executable, "-m", "gnss_dsp_tools_amd.spectrum", str(path), repr(fc), repr(fs), str(n), str(ns)], cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout == text.getvalue()
    axis = spectrum.freq_axis_mhz(fc, fs, n)
    tone = fc / 1e6 + C.SPECTRUM_TONES[0][0] * fs / 1e6
    lines = text.getvalue().splitlines()
    assert len(lines) == len(want)
    for k, (ln, y) in enumerate(zip(lines, want)):
        idx, peak, top, med = ln.split()
        i = int(np.argmax(y))
        assert int(idx) == k
        assert abs(float(peak) - axis[i]) <= 5.1e-7 and abs(axis[i] - tone) <= fs / n / 1e6        # printed with six decimals
        assert abs(float(top) - y[i]) <= 5.1e-4 + bound and abs(float(med) - np.median(y)) <= 5.1e-4 + bound    # three decimals
        assert float(top) > float(med) + 10


@pytest.mark.gpu
def test_squaring_command_line(engine, tmp_path):
    g = GOLDEN["squaring"]["script"]
    b, n, m, chunks, fs, coffset = C.SQUARING["script"]
    x = C.checked_recording(GOLDEN, "squaring", "script")                                 # three chunks and a third of one
    path = tmp_path / "rec.iq"
    x.tofile(path)
    sink = io.BytesIO()
    assert squaring.run([str(path), repr(fs), repr(coffset)], sink, engine) == (chunks, 0)
    _, stream64, _ = O.squaring_fp64(x, fs, coffset, b, n, m)
    assert sink.getvalue() == stream64.tobytes()
    r_ref = C.unpack(g["r"], np.complex128).reshape(chunks, b)
    ok, share = C.stream_check(np.frombuffer(sink.getvalue(), dtype=np.int16), C.unpack(g["stream"], np.int16), r_ref,
                               C.HALF_FACTOR * g["max_diff_20r"])
    assert ok and share <= C.HALF_SHARE, (ok, share)
    # as a program writing to a pipe, the negative COFFSET on its command line
    p = subprocess.run([sys.executable, "-m", "gnss_dsp_tools_amd.squaring", str(path), repr(fs), repr(coffset)], cwd=ROOT, capture_output=True,
                       timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    assert coffset < 0 and p.stdout == stream64.tobytes()


@pytest.mark.gpu
def test_track_loop_records_go_straight_into_cn0(engine):
    torch = nat.require_torch()
    name = "gps_l2cm"                                                                      # 60 records, the longest golden track
    case = T.load()["cases"][name]
    tl = trackloop.TrackLoop([T.channel_of(case)], engine)
    try:
        recs = tl.run([torch.from_numpy(T.recording(case)).to("cuda:%d" % engine.device)])[0]
    finally:
        tl.close()
    g = GOLDEN["cn0"]["track/" + name][0]
    assert len(recs) == len(case["stdout_lines"])
    assert cn0.format_lines(cn0.from_records(recs, g["time"])) == g["lines"]
    assert len(g["lines"]) == 60 // C.CN0_TRACK_TIME
