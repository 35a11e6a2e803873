"""Recordings in other sample formats, converted on the GPU (csrc/gacq_ingest.hip, gacq_ingest_dev) to the interleaved int8 I/Q (or
complex64) that acquire, scan, handoff, refine, coherent, the tracking loops, spectrum and squaring take: 1 / 2 / 4-bit codes packed
into bytes, signed and unsigned 8-bit, 16-bit, float32; I/Q pairs or real IF samples.  The output is an exact function of (format,
gain, absolute sample index): a recording converts to the same bytes however it is cut into calls or chunks.

    python -m gnss_dsp_tools_amd.ingest --format FMT [--lsb-first] [--lut a,b,..] [--real] [--conj] [--gain G | --target-rms R]
           [--complex64] IN FS COFFSET OUT

reads IN (or - for stdin), writes OUT (or - for stdout) and prints one line (to stderr when OUT is -):

    fs <FS_OUT> coffset <COFFSET_OUT> gain <G> samples <N>

the sample rate and carrier offset to hand to the tools that read OUT.  FMT: s8, u8, s16, f32 (little-endian), or BITS + coding for
packed codes: 1sm 1ob 2sm 2ob 2tc 4sm 4ob 4tc (sm: sign / magnitude, +-(2 mag + 1), sign bit 1 negative; ob: offset binary,
2 code - (2^bits - 1); tc: two's complement, 2 signed(code) + 1); --lut gives the 2^bits values instead.  The first code of a byte is in
its top bits unless --lsb-first.  --real: real IF samples; they are shifted down by fs/4, low-pass filtered by a 47-tap half-band
filter and decimated by two, in integers, so FS_OUT = FS / 2 and COFFSET_OUT = COFFSET - FS / 4.  --conj negates the imaginary part
(and COFFSET_OUT).  Without --gain the gain is target_rms (default 32) over the rms of the first 65536 output samples at gain 1.
The definition is in include/gacq.h; tests/ingest_oracle.py restates it in numpy."""
import argparse
import ctypes
import math
import sys

import numpy as np

from . import _native as nat
from . import rawfile, streaming

S8, U8, S16, F32, PACKED = (nat.CONSTANTS["GACQ_INGEST_" + k] for k in ("S8", "U8", "S16", "F32", "PACKED"))
CONTAINERS = {"s8": S8, "u8": U8, "s16": S16, "f32": F32}
PACKED_NAMES = ("1sm", "1ob", "2sm", "2ob", "2tc", "4sm", "4ob", "4tc")
NAMES = tuple(CONTAINERS) + PACKED_NAMES
HALF = 21                                           # real mode: output m reads inputs 2m - HALF .. 2m + HALF
AUTO_SAMPLES = 65536
MAX_INDEX = 1 << 48
TARGET_RMS = 32.0


IngestFmt = nat.struct("gacq_ingest_fmt")


def preset_lut(bits, coding):
    """The 2^bits values of a coding: 'sm' sign / magnitude, 'ob' offset binary, 'tc' two's complement"""
    n = 1 << bits
    if coding == "sm":
        return [(-1 if c >> (bits - 1) else 1) * (2 * (c & (n // 2 - 1)) + 1) for c in range(n)]
    if coding == "ob":
        return [2 * c - (n - 1) for c in range(n)]
    if coding == "tc":
        return [2 * (c - n if c >> (bits - 1) else c) + 1 for c in range(n)]
    raise ValueError("unknown coding %r" % (coding,))


class Format:
    """A sample format: Format("2sm", real=True), Format("s16", conj=True), Format("2ob", lut=[-3, -1, 1, 3], msb_first=False)."""

    def __init__(self, name, real=False, conj=False, msb_first=True, lut=None):
        name = str(name).lower()
        self.name, self.real, self.conj, self.msb_first = name, bool(real), bool(conj), bool(msb_first)
        if name in CONTAINERS:
            self.container, self.bits, self.value_bits = CONTAINERS[name], 0, {S8: 8, U8: 8, S16: 16, F32: 32}[CONTAINERS[name]]
            if lut is not None:
                raise ValueError("a LUT goes with packed codes, not with %s" % name)
            self.lut = []
        elif name in PACKED_NAMES:
            self.container, self.bits = PACKED, int(name[0])
            self.value_bits = self.bits
            self.lut = preset_lut(self.bits, name[1:]) if lut is None else [int(v) for v in lut]
            if len(self.lut) != 1 << self.bits or not all(-128 <= v <= 127 for v in self.lut):
                raise ValueError("the LUT of %s needs %d values in -128..127" % (name, 1 << self.bits))
        else:
            raise ValueError("unknown format %r (the formats: %s)" % (name, ", ".join(NAMES)))
        if self.real and self.container in (S16, F32):
            raise ValueError("real mode takes s8, u8 and packed input only")
        self.sample_bits = self.value_bits * (1 if self.real else 2)

    def struct(self):
        return IngestFmt(container=self.container, real=int(self.real), bits=self.bits, msb_first=int(self.msb_first), conj=int(self.conj),
                         lut=(ctypes.c_int8 * 16)(*(self.lut + [0] * (16 - len(self.lut)))))

    def samples(self, nbytes):
        """whole input samples in nbytes bytes"""
        return int(nbytes) * 8 // self.sample_bits

    def out_range(self, in_first, in_count):
        """(first, count) of the output samples that input samples in_first .. in_first + in_count - 1 support"""
        if not self.real:
            return in_first, in_count
        first = 0 if in_first == 0 else -(-(in_first + HALF) // 2)
        last = (in_first + in_count - 1 - HALF) // 2
        return first, max(0, last - first + 1)

    def rates(self, fs, coffset):
        """(fs, coffset) of the converted recording"""
        fs, coffset = float(fs), float(coffset)
        if self.real:
            fs, coffset = fs / 2.0, coffset - fs / 4.0
        return fs, (-coffset if self.conj else coffset)


def as_format(fmt):
    return fmt if isinstance(fmt, Format) else Format(fmt)


def _device_bytes(engine, data):
    """uint8 CUDA tensor (any byte offset) of a uint8 CUDA tensor or a bytes-like object"""
    return streaming.device_flat(engine, data, ("uint8",), "data must be a flat uint8 CUDA tensor or a bytes-like object")


def convert(engine, fmt, data, gain, in_first=0, out_first=None, n_out=None, dtype="int8"):
    """Output samples out_first .. out_first + n_out - 1 of the recording whose input samples in_first .. are at `data` (a flat uint8
    CUDA tensor or a bytes-like object): a flat int8 CUDA tensor [2 n_out] of interleaved I/Q, or complex64 [n_out].  By default
    every output sample the data supports.  Asynchronous on torch's current stream."""
    fmt = as_format(fmt)
    d = _device_bytes(engine, data)
    in_first = int(in_first)
    in_count = fmt.samples(d.numel())
    first, count = fmt.out_range(in_first, in_count)
    out_first = first if out_first is None else int(out_first)
    n_out = max(0, first + count - out_first) if n_out is None else int(n_out)
    cplx, out = streaming.iq_out(n_out, dtype, d.device)
    st = fmt.struct()
    return streaming.launch(engine, [d], d.numel(), out, n_out, lambda src, dst: nat.check(
        nat.lib.gacq_ingest_dev(engine._ctx, ctypes.addressof(st), ctypes.c_void_p(src[0]), in_first, in_count, out_first, n_out, float(gain), int(cplx),
                                ctypes.c_void_p(dst)), engine._ctx))


def rms_gain(u, target_rms=TARGET_RMS):
    """target_rms / sqrt(mean |u|^2) in numpy float64 of complex64 samples; zero power is refused"""
    u = np.asarray(u)
    power = float(np.mean(u.real.astype(np.float64) ** 2 + u.imag.astype(np.float64) ** 2)) if len(u) else 0.0
    if not power > 0.0 or not math.isfinite(power):
        raise ValueError("automatic gain: the first samples have no power (or are not finite)")
    return float(target_rms) / math.sqrt(power)


def auto_gain(engine, fmt, first_piece, target_rms=TARGET_RMS):
    """target_rms over the rms of the first P output samples at gain 1, P = min(what first_piece supports, 65536): a defined function of
    the recording, evaluated on the host from the device's own complex64 output (exact values for every format but f32)."""
    fmt = as_format(fmt)
    d = _device_bytes(engine, first_piece)
    first, count = fmt.out_range(0, fmt.samples(d.numel()))
    p = min(count, AUTO_SAMPLES)
    if p < 1:
        raise ValueError("automatic gain: the first piece holds no whole output sample")
    return rms_gain(convert(engine, fmt, d, 1.0, 0, 0, p, "complex64").cpu().numpy(), target_rms)


class Ingest(streaming.Chunks):
    """A recording fed chunk by chunk: feed(chunk) returns the output samples the chunk completes, and the concatenation of what the
    calls return is what one convert() of the whole recording gives.  What the next call still needs stays on the device: the bytes of
    a sample (or of a byte of packed codes) that the chunk cut, and in real mode the input tail under the next outputs' supports; the
    tail kept always starts on a byte boundary.  A real-mode recording ends at the last output whose 43-sample support is present:
    the last 10 or 11 output samples that the input would otherwise give are not produced."""

    def __init__(self, engine, fmt, gain, dtype="int8"):
        self.engine, self.fmt, self.gain, self.dtype = engine, as_format(fmt), float(gain), dtype
        fmt = self.fmt
        # real mode keeps the tail from the first input sample the next output needs, moved down to a multiple of 16 samples: a byte
        # boundary in every format, and a 16-byte boundary of 8-bit real input
        # (I/Q: whole samples are whole bytes, or whole bytes hold whole samples, so the end of the whole samples is on a byte boundary)
        super().__init__(fmt.sample_bits, lambda in_first, in_count: sum(fmt.out_range(in_first, in_count)),
                         lambda ds, in_first, in_count, out_first, n_out, k: convert(engine, fmt, ds[0], self.gain, in_first, out_first, n_out, dtype),
                         lambda out: (2 * out - HALF) // 16 * 16 if fmt.real else out)

    def feed(self, chunk):
        return self.feed_all([_device_bytes(self.engine, chunk)])


def convert_file(engine, fmt, fin, fout, gain=None, target_rms=TARGET_RMS, dtype="int8", piece_bytes=rawfile.PIECE_BYTES):
    """Convert the open binary file fin into fout piece by piece; gain None: the automatic gain of the first piece.  (gain, samples)."""
    fmt = as_format(fmt)

    def start(held):
        nonlocal gain
        if gain is None:                        # 16 bytes per output sample and 64 more hold 65536 output samples of every format
            gain = auto_gain(engine, fmt, held[0][:AUTO_SAMPLES * 16 + 64], target_rms)
        ing = Ingest(engine, fmt, gain, dtype)
        return lambda piece: [ing.feed(piece)]

    n = streaming.pump(rawfile.read_pieces(fin, max(1, fmt.sample_bits // 8), piece_bytes), start, [fout], 2 if dtype == "int8" else 1)
    if n is None:
        raise ValueError("the input holds no whole sample")
    return float(gain), n[0]


def build_parser():
    ap = argparse.ArgumentParser(prog="ingest", description="Convert a recording to int8 I/Q (or complex64) on the GPU")
    ap.add_argument("--format", required=True, help="sample format: %s" % " ".join(NAMES))
    ap.add_argument("--lsb-first", action="store_true", help="packed codes: the first code of a byte is in its low bits")
    ap.add_argument("--lut", default=None, help="packed codes: the 2^bits values, comma separated")
    ap.add_argument("--real", action="store_true", help="real IF samples: fs/4 down-shift, half-band filter, decimation by two")
    ap.add_argument("--conj", action="store_true", help="negate the imaginary part (spectral inversion)")
    g = ap.add_mutually_exclusive_group()
    g.add_argument("--gain", type=float, default=None, help="gain (default: automatic)")
    g.add_argument("--target-rms", type=float, default=TARGET_RMS, help="rms the automatic gain aims at (default %(default)s)")
    ap.add_argument("--complex64", action="store_true", help="write complex64 instead of int8")
    ap.add_argument("--device", type=int, default=0, help="GPU index")
    ap.add_argument("input_filename")
    ap.add_argument("fs", type=float)
    ap.add_argument("coffset", type=float)
    ap.add_argument("output_filename")
    return ap


def parse(argv):
    """(argparse namespace, Format) of a command line"""
    argv = list(argv)
    for i, v in enumerate(argv[:-1]):
        if v == "--lut":                        # '--lut -3,-1,1,3' -> '--lut=-3,-1,1,3', so that the value is never taken for an option
            argv[i:i + 2] = ["--lut=" + argv[i + 1]]
            break
    a = build_parser().parse_args(argv)
    try:
        lut = None if a.lut is None else [int(v) for v in a.lut.split(",")]
        fmt = Format(a.format, real=a.real, conj=a.conj, msb_first=not a.lsb_first, lut=lut)
    except ValueError as e:
        raise SystemExit("ingest: %s" % e)
    if not a.fs > 0.0 or (a.gain is not None and not streaming.positive_finite(a.gain)) or not streaming.positive_finite(a.target_rms):
        raise SystemExit("ingest: need FS > 0 and a positive, finite --gain / --target-rms")
    return a, fmt


def report_line(fmt, fs, coffset, gain, samples):
    fs_out, coffset_out = fmt.rates(fs, coffset)
    return "fs %r coffset %r gain %r samples %d" % (fs_out, coffset_out, float(gain), int(samples))


def run(argv, out=None, piece_bytes=rawfile.PIECE_BYTES):
    a, fmt = parse(argv)
    with streaming.shell(a.device, [a.input_filename], [a.output_filename], report=out) as sh:
        gain, n = convert_file(sh.engine, fmt, sh.fins[0], sh.fouts[0], a.gain, a.target_rms, "complex64" if a.complex64 else "int8", piece_bytes)
    line = report_line(fmt, a.fs, a.coffset, gain, n)
    print(line, file=sh.report)
    return line


def main(argv=None):
    return streaming.main(argv, __doc__, run)


if __name__ == "__main__":
    sys.exit(main())
