"""A band out of a wide recording, on the GPU (csrc/gacq_ddc.hip, gacq_ddc_*): a table NCO mixer, an integer FIR low-pass and integer
decimation, interleaved int8 I/Q in, int8 I/Q (or complex64) out at FS / D -- the stage in front of ingest -> mitigate -> scan /
handoff / track -> navdata for a recording wider than the signal, or one that holds several signals (the 14 GLONASS FDMA channels of a
G1 capture).  The output is an exact function of (configuration, gain, absolute sample index): a recording converts to the same bytes
however it is cut into calls or chunks.

    python -m gnss_dsp_tools_amd.ddc --decim D [--taps T] [--cutoff HZ] [--gain G | --target-rms R] [--complex64]
           --band SHIFT_HZ OUT [--band SHIFT_HZ OUT ...] IN FS COFFSET

reads IN (or - for stdin) once and writes, for every --band, the band centred on SHIFT_HZ (relative to the centre of IN) to OUT (-
for stdout, with one band), and prints one line per band (to stderr when OUT is -):

    band <SHIFT> fs <FS_OUT> coffset <COFFSET_OUT> gain <G> samples <N>

the sample rate and carrier offset to hand to the tools that read OUT: FS_OUT = FS / D and COFFSET_OUT = COFFSET - the shift the NCO
applies, SHIFT_HZ rounded to FS / 2^64.  The filter: T taps (default 8 D + 1; odd, at most 513), a Hann-windowed sinc with its -6 dB
point at --cutoff HZ (default 0.4 FS_OUT), in integers that sum to 32768; D = 1 without a cutoff is a pure shift.  Output m is centred
on input m D (no group delay: code phases carry over) and needs inputs m D - T/2 .. m D + T/2, so a recording of N samples ends at
output (N - 1 - T/2) div D.  Without --gain the gain of a band is target_rms (default 32) over the rms of its first 65536 output
samples at gain 1.  The definition is in include/gacq.h; tests/ddc_oracle.py restates it in numpy."""
import argparse
import ctypes
import math
import sys
from fractions import Fraction

import numpy as np

from . import _native as nat
from . import ingest, rawfile, streaming

MAX_DECIM, MAX_TAPS = 64, 513
MAX_TAP_SUM = 65536
UNITY = 32768                                       # taps that sum to this have unity gain at gain 1
AUTO_SAMPLES = ingest.AUTO_SAMPLES
TARGET_RMS = ingest.TARGET_RMS


DdcCfg = nat.struct("gacq_ddc_cfg")


def phase_increment(f_shift, fs):
    """dP = rint(f_shift / fs 2^64) mod 2^64, exactly from the two doubles"""
    return int(round(Fraction(float(f_shift)) / Fraction(float(fs)) * (1 << 64))) % (1 << 64)


def applied_shift(dphase, fs):
    """the shift dP stands for: dP as a signed 64-bit number, over 2^64, times fs (the exact product, rounded once)"""
    signed = dphase - (1 << 64) if dphase >> 63 else dphase
    return float(Fraction(signed, 1 << 64) * Fraction(float(fs)))


def table():
    """the NCO's table as the library forms it: int16 [4096, 2], (cos, sin)"""
    w = np.empty((4096, 2), dtype=np.int16)
    nat.check(nat.lib.gacq_ddc_table(ctypes.c_void_p(w.ctypes.data)))
    return w


def firwin_hann(ntaps, cutoff_norm):
    """gacq_firwin_hann's formula (scipy.signal.firwin(ntaps, cutoff_norm, window='hann')) on the host in numpy: the library's entry
    point stops at the front-end's 512 taps, one short of D = 64"""
    i = np.arange(int(ntaps), dtype=np.float64)
    arg = float(cutoff_norm) * (i - 0.5 * (ntaps - 1))
    h = float(cutoff_norm) * np.sinc(arg) * (0.5 - 0.5 * np.cos(2.0 * np.pi * i / float(ntaps - 1)))
    return h / h.sum()


def design_taps(D, T=None, cutoff_hz=None, fs=None):
    """The default filter of decimation D as int32 taps g[-H .. H]: T = 8 D + 1 taps of the Hann-windowed sinc
    firwin_hann(T, 0.8 / D) (the -6 dB point at 0.4 fs / D; with cutoff_hz and fs at cutoff_hz), g = rint(32768 h) with the centre
    tap adjusted so that the taps sum to 32768.  D = 1 without a cutoff: the single tap 32768, a pure shift."""
    D = int(D)
    if not 1 <= D <= MAX_DECIM:
        raise ValueError("the decimation lies in 1..%d, not %d" % (MAX_DECIM, D))
    if T is None:
        T = 1 if (D == 1 and cutoff_hz is None) else 8 * D + 1
    T = int(T)
    if not 1 <= T <= MAX_TAPS or T % 2 == 0:
        raise ValueError("the number of taps is odd and in 1..%d, not %d" % (MAX_TAPS, T))
    if T == 1:
        return np.array([UNITY], dtype=np.int32)
    if cutoff_hz is None:
        cutoff = 0.8 / D
    else:
        if fs is None:
            raise ValueError("a cutoff in Hz needs the sample rate")
        cutoff = float(cutoff_hz) / (0.5 * float(fs))
    if not 0.0 < cutoff < 1.0:
        raise ValueError("the cutoff must lie inside (0, fs / 2)")
    g = np.rint(UNITY * firwin_hann(T, cutoff)).astype(np.int64)
    g[T // 2] += UNITY - int(g.sum())
    if int(np.abs(g).sum()) > MAX_TAP_SUM:
        raise ValueError("the taps' magnitudes sum to more than %d" % MAX_TAP_SUM)
    return g.astype(np.int32)


class Band:
    """Band(f_shift, D, taps=None, cutoff_hz=None): the band centred on f_shift (Hz from the centre of the recording), decimated by D;
    taps: integers g[-H .. H] (odd count up to 513, sum |g| <= 65536) instead of design_taps(D, cutoff_hz=cutoff_hz, fs=fs)."""

    def __init__(self, f_shift, D, taps=None, cutoff_hz=None, ntaps=None):
        self.f_shift, self.D = float(f_shift), int(D)
        if not 1 <= self.D <= MAX_DECIM:
            raise ValueError("the decimation lies in 1..%d, not %d" % (MAX_DECIM, self.D))
        if not math.isfinite(self.f_shift):
            raise ValueError("the shift must be finite")
        self.cutoff_hz = None if cutoff_hz is None else float(cutoff_hz)
        self.taps = None if taps is None else np.ascontiguousarray(np.asarray(taps, dtype=np.int64).reshape(-1).astype(np.int32))
        if self.taps is not None:
            if self.cutoff_hz is not None or ntaps is not None:
                raise ValueError("taps and a cutoff or a tap count exclude each other")
            self.T = len(self.taps)
        elif ntaps is not None:
            self.T = int(ntaps)
        else:
            self.T = 1 if (self.D == 1 and self.cutoff_hz is None) else 8 * self.D + 1
        if not 1 <= self.T <= MAX_TAPS or self.T % 2 == 0:
            raise ValueError("the number of taps is odd and in 1..%d, not %d" % (MAX_TAPS, self.T))
        self.H = self.T // 2

    def taps_for(self, fs):
        return self.taps if self.taps is not None else design_taps(self.D, self.T, self.cutoff_hz, fs)

    def dphase(self, fs):
        return phase_increment(self.f_shift, fs)

    def rates(self, fs, coffset):
        """(fs, coffset) of the converted recording"""
        fs = float(fs)
        return fs / self.D, float(coffset) - applied_shift(self.dphase(fs), fs)

    def out_range(self, in_first, in_count):
        """(first, count) of the output samples that input samples in_first .. in_first + in_count - 1 support"""
        first = 0 if in_first == 0 else -(-(in_first + self.H) // self.D)
        last = (in_first + in_count - 1 - self.H) // self.D
        return first, max(0, last - first + 1)

    def first_needed(self, out):
        """the first input sample that output `out` needs"""
        return max(0, out * self.D - self.H)


def _device_iq(engine, data):
    """flat uint8 CUDA tensor (any byte offset) of a flat int8 / uint8 CUDA tensor or a bytes-like object of int8 pairs"""
    return streaming.device_flat(engine, data, ("uint8", "int8"), "data must be a flat int8 or uint8 CUDA tensor or a bytes-like object", "uint8")


class Converter(streaming.Handle):
    """The open device side of one band at one sample rate (gacq_ddc_open: the table and the taps are uploaded once); run() is one
    asynchronous launch on torch's current stream.  Closed with its engine at the latest."""
    _close, _what = "gacq_ddc_close", "converter"

    def __init__(self, engine, band, fs):
        self.band, self.fs = band, float(fs)
        if not self.fs > 0.0 or not math.isfinite(self.fs):
            raise ValueError("the sample rate must be positive and finite")
        self.taps = np.ascontiguousarray(band.taps_for(self.fs), dtype=np.int32)
        self.cfg = DdcCfg(dphase=band.dphase(self.fs), decim=band.D)
        self._open(engine, nat.lib.gacq_ddc_open, ctypes.addressof(self.cfg), ctypes.c_void_p(self.taps.ctypes.data), len(self.taps))

    def run(self, d, in_first, out_first, n_out, gain, dtype="int8"):
        """outputs out_first .. out_first + n_out - 1 of the recording whose samples in_first .. are the int8 pairs of the flat uint8
        CUDA tensor d"""
        n_out = int(n_out)
        cplx, out = streaming.iq_out(n_out, dtype, d.device)
        self._check_open()
        return streaming.launch(self.engine, [d], d.numel(), out, n_out, lambda src, dst: nat.check(
            nat.lib.gacq_ddc_run_dev(self._h, ctypes.c_void_p(src[0]), int(in_first), d.numel() // 2, int(out_first), n_out, float(gain), int(cplx),
                                     ctypes.c_void_p(dst)), self.engine._ctx))


def convert(engine, band, fs, data, gain, in_first=0, out_first=None, n_out=None, dtype="int8"):
    """Output samples out_first .. out_first + n_out - 1 of the recording whose input samples in_first .. are at `data` (a flat int8 or
    uint8 CUDA tensor or a bytes-like object of int8 pairs): a flat int8 CUDA tensor [2 n_out] of interleaved I/Q, or complex64
    [n_out].  By default every output sample the data supports."""
    d = _device_iq(engine, data)
    in_first = int(in_first)
    first, count = band.out_range(in_first, d.numel() // 2)
    out_first = first if out_first is None else int(out_first)
    n_out = max(0, first + count - out_first) if n_out is None else int(n_out)
    with Converter(engine, band, fs) as conv:
        return conv.run(d, in_first, out_first, n_out, gain, dtype)


def auto_gain(engine, band, fs, first_piece, target_rms=TARGET_RMS):
    """target_rms over the rms of the first P output samples at gain 1, P = min(what first_piece supports, 65536): the rule and the
    rms_gain of ingest.py, evaluated on the host in float64 from the device's own complex64 output."""
    d = _device_iq(engine, first_piece)
    first, count = band.out_range(0, d.numel() // 2)
    p = min(count, AUTO_SAMPLES)
    if p < 1:
        raise ValueError("automatic gain: the first piece holds no whole output sample")
    return ingest.rms_gain(convert(engine, band, fs, d, 1.0, 0, 0, p, "complex64").cpu().numpy(), target_rms)


def auto_window(band):
    """input samples that hold the automatic gain's window"""
    return (AUTO_SAMPLES - 1) * band.D + band.H + 1


class Splitter(streaming.Chunks):
    """One recording fed chunk by chunk into several bands: feed(chunk) uploads the chunk once, launches every band on it and returns
    each band's output samples that the chunk completes; the concatenation of what the calls return for a band is what one convert()
    of the whole recording gives.  The input tail that some band's next output still needs, and the byte of a sample that a chunk
    cut, stay on the device."""

    def __init__(self, engine, bands, fs, gains, dtype="int8"):
        self.engine, self.bands, self.fs, self.dtype = engine, list(bands), float(fs), dtype
        self.gains = [float(g) for g in gains]
        if len(self.gains) != len(self.bands) or not self.bands:
            raise ValueError("one gain per band, and at least one band")
        self.convs = [Converter(engine, b, fs) for b in self.bands]
        super().__init__(16, lambda in_first, in_count: [sum(b.out_range(in_first, in_count)) for b in self.bands],
                         lambda ds, in_first, in_count, out_first, n_out, k: self.convs[k].run(ds[0], in_first, out_first, n_out, self.gains[k], dtype),
                         lambda nexts: min(b.first_needed(m) for b, m in zip(self.bands, nexts)), outputs=len(self.bands))

    def feed(self, chunk):
        return self.feed_all([_device_iq(self.engine, chunk)])

    def close(self):
        for c in self.convs:
            c.close()


class Downconverter:
    """A recording fed chunk by chunk into one band: feed(chunk) returns the output samples the chunk completes."""

    def __init__(self, engine, band, fs, gain, dtype="int8"):
        self._s = Splitter(engine, [band], fs, [gain], dtype)
        self.engine, self.band, self.fs, self.gain, self.dtype = engine, band, float(fs), float(gain), dtype

    @property
    def next_out(self):
        return self._s.next_out[0]

    @property
    def in_first(self):
        return self._s.in_first

    def feed(self, chunk):
        return self._s.feed(chunk)[0]

    def close(self):
        self._s.close()


def split_file(engine, bands, fs, fin, fouts, gain=None, target_rms=TARGET_RMS, dtype="int8", piece_bytes=rawfile.PIECE_BYTES):
    """Read the open binary file fin once, in pieces, and write every band to its file of fouts: each piece is uploaded once and every
    band launched on it.  gain: one for all bands, one per band, or None for each band's automatic gain: that of its first 65536
    outputs whatever the piece size (pieces shorter than that window are read ahead until they hold it).
    (gains, samples written per band)."""
    bands = list(bands)
    if len(bands) != len(fouts) or not bands:
        raise ValueError("one output per band, and at least one band")
    gains = None if gain is None else ([float(g) for g in gain] if np.ndim(gain) else [float(gain)] * len(bands))
    sp = None
    window = 0 if gains is not None else max(auto_window(b) for b in bands)

    def start(held):
        nonlocal sp, gains
        if len(held) == 1:                          # one piece holds the window (or all there is): uploaded once, it serves the gain and the bands
            held[0] = _device_iq(engine, held[0])
        if gains is None:
            first = held[0] if len(held) == 1 else np.concatenate(held)[:2 * window]
            gains = [auto_gain(engine, b, fs, first[:2 * auto_window(b)], target_rms) for b in bands]
        sp = Splitter(engine, bands, fs, gains, dtype)
        return sp.feed

    try:                                            # pieces shorter than the window wait on the host
        n = streaming.pump(rawfile.read_pieces(fin, 2, piece_bytes), start, fouts, 2 if dtype == "int8" else 1, 2 * window)
    finally:
        if sp is not None:
            sp.close()
    if n is None:
        raise ValueError("the input holds no whole sample")
    return gains, n


def build_parser():
    ap = argparse.ArgumentParser(prog="ddc", description="Down-convert and decimate bands of an int8 I/Q recording on the GPU")
    ap.add_argument("--decim", type=int, required=True, help="decimation factor D, 1..%d" % MAX_DECIM)
    ap.add_argument("--taps", type=int, default=None, help="number of filter taps, odd, at most %d (default 8 D + 1)" % MAX_TAPS)
    ap.add_argument("--cutoff", type=float, default=None, help="-6 dB point of the filter in Hz (default 0.4 FS / D)")
    g = ap.add_mutually_exclusive_group()
    g.add_argument("--gain", type=float, default=None, help="gain (default: automatic, per band)")
    g.add_argument("--target-rms", type=float, default=TARGET_RMS, help="rms the automatic gain aims at (default %(default)s)")
    ap.add_argument("--complex64", action="store_true", help="write complex64 instead of int8")
    ap.add_argument("--band", nargs=2, action="append", required=True, metavar=("SHIFT_HZ", "OUT"),
                    help="a band: its centre in Hz from the centre of IN, and the file to write (- for stdout, with one band)")
    ap.add_argument("--device", type=int, default=0, help="GPU index")
    ap.add_argument("input_filename")
    ap.add_argument("fs", type=float)
    ap.add_argument("coffset", type=float)
    return ap


def parse(argv):
    """(argparse namespace, [Band], [output file names]) of a command line"""
    argv = list(argv)
    for i, v in enumerate(argv):
        # '--band -1.0e6 OUT', a COFFSET of -2.5e5: a leading blank keeps a negative number with an exponent from being taken for an option
        if v.startswith("-") and v != "-" and not v.startswith("--"):
            try:
                float(v)
                argv[i] = " " + v
            except ValueError:
                pass
    a = build_parser().parse_args(argv)
    bad = None
    if not (a.fs > 0.0 and math.isfinite(a.fs)) or not math.isfinite(a.coffset):
        bad = "need a positive, finite FS and a finite COFFSET"
    elif (a.gain is not None and not streaming.positive_finite(a.gain)) or not streaming.positive_finite(a.target_rms):
        bad = "need a positive, finite --gain / --target-rms"
    elif a.cutoff is not None and not 0.0 < a.cutoff < 0.5 * a.fs:
        bad = "--cutoff must lie inside (0, FS / 2)"
    elif len(a.band) > 1 and any(o == "-" for _, o in a.band):
        bad = "- (stdout) goes with one band"
    if bad:
        raise SystemExit("ddc: %s" % bad)
    try:
        bands = [Band(float(s), a.decim, cutoff_hz=a.cutoff, ntaps=a.taps) for s, _ in a.band]
        for b in bands:
            b.taps_for(a.fs)
    except ValueError as e:
        raise SystemExit("ddc: %s" % e)
    return a, bands, [o for _, o in a.band]


def report_line(band, fs, coffset, gain, samples):
    fs_out, coffset_out = band.rates(fs, coffset)
    return "band %r fs %r coffset %r gain %r samples %d" % (band.f_shift, fs_out, coffset_out, float(gain), int(samples))


def run(argv, out=None, piece_bytes=rawfile.PIECE_BYTES):
    a, bands, names = parse(argv)
    with streaming.shell(a.device, [a.input_filename], names, report=out) as sh:
        gains, n = split_file(sh.engine, bands, a.fs, sh.fins[0], sh.fouts, a.gain, a.target_rms, "complex64" if a.complex64 else "int8", piece_bytes)
    lines = [report_line(b, a.fs, a.coffset, g, k) for b, g, k in zip(bands, gains, n)]
    for line in lines:
        print(line, file=sh.report)
    return lines


def main(argv=None):
    return streaming.main(argv, __doc__, run)


if __name__ == "__main__":
    sys.exit(main())
