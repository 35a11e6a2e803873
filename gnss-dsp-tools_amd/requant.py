"""Level control (AGC) and requantiser on the GPU (csrc/gacq_requant.hip, gacq_requant_*): the inverse of ingest.  Interleaved int8 (or
int16) I/Q in; int8, offset uint8, int16, float32 or 1 / 2 / 4-bit codes packed into bytes out, under a gain that follows the power of
the recording block by block.  The output is an exact function of (configuration, tables, absolute sample index): a recording converts
to the same bytes however it is cut into calls or chunks.

    python -m gnss_dsp_tools_amd.requant --format s8|u8|s16|f32|1sm|1ob|2sm|2ob|2tc|4sm|4ob|4tc [--in-format s8|s16] [--lsb-first]
           [--block N] [--window W] [--target-rms R | --gain G] [--trace FILE] IN OUT

reads IN (or - for stdin), writes OUT (or - for stdout) and prints two lines (to stderr when OUT is -):

    format <FMT> block <N> window <W> gain <LOWEST> .. <HIGHEST> clipped <COMPONENTS> samples <SAMPLES>
    ingest --format <FMT> [--lsb-first]

the second being the arguments with which ingest reads OUT back.  The level of block b (N samples, default 4096) is the power of the
W blocks before it (default 8; of the first W blocks during the warm-up); the gain is the largest entry of a table of 128 gains, 0.75 dB
apart, that keeps the rms of the complex sample at or below --target-rms (defaults: s8 / u8 32, s16 8192, f32 32, 2-bit 2.84, 4-bit
8.44, the values at which a uniform quantiser loses least on Gaussian input; 1-bit output keeps the sign, whatever the gain).  --gain
gives one fixed gain instead.  --trace writes the index of the gain of every block, one byte each.  Packed output holds whole bytes:
up to three trailing samples are dropped.  A recording shorter than W blocks gives no output.  The definition is in include/gacq.h;
tests/requant_oracle.py restates it in numpy."""
import argparse
import ctypes
import sys
from fractions import Fraction

import numpy as np

from . import _native as nat
from . import ingest, rawfile, streaming
from .streaming import first_needed                           # first_needed(block, window, out), part of this module as before

S8, U8, S16, F32, PACKED = ingest.S8, ingest.U8, ingest.S16, ingest.F32, ingest.PACKED
NAMES = ingest.NAMES
MAX_GAINS, MAX_WINDOW, MAX_BLOCK = 256, 64, 65536
BLOCK, WINDOW = 4096, 8
STEP, GAINS, G_MAX = 8, 128, 64.0                   # 2^(1/8) = 0.75 dB a step, 128 steps = 96 dB, from 64 down
# rms of the complex sample; the few-bit values put the step of 2 at 0.996 sigma (2 bits) and 0.335 sigma (4 bits) per component
TARGET_RMS = {"s8": ingest.TARGET_RMS, "u8": ingest.TARGET_RMS, "s16": 8192.0, "f32": ingest.TARGET_RMS, 1: 2.84, 2: 2.84, 4: 8.44}


RequantCfg = nat.struct("gacq_requant_cfg")


def tables(target_rms, block, window, step=STEP, K=GAINS, g_max=G_MAX):
    """(G, T): G[k] = float32(g_max 2^(-k / step)), T[i] = floor(target_rms^2 W Lb / G[i]^2), the largest level at which gain i keeps
    the rms at or below the target -- so k(b), the number of thresholds below the level, is the first gain that does.  T is exact in
    the float32 gains and the double target (Fractions), capped at 2^64 - 1, which no level reaches; the library takes both tables as
    they are."""
    target_rms, K, step = float(target_rms), int(K), int(step)
    if not streaming.positive_finite(target_rms) or not 1 <= K <= MAX_GAINS or step < 1 or not streaming.positive_finite(g_max):
        raise ValueError("tables: need a positive, finite target rms and g_max, 1..%d gains, a step of at least 1" % MAX_GAINS)
    G = np.array([g_max * 2.0 ** (-k / step) for k in range(K)], dtype=np.float32)
    if not (np.all(np.isfinite(G)) and np.all(G > 0)):
        raise ValueError("tables: a gain is not finite and positive in float32")
    top = Fraction(target_rms) ** 2 * int(window) * int(block)
    T = np.array([min(int(top / Fraction(float(g)) ** 2), (1 << 64) - 1) for g in G[:-1]], dtype=np.uint64)
    return G, T


def fixed(gain):
    """the tables of one fixed gain"""
    return np.array([gain], dtype=np.float32), np.zeros(0, dtype=np.uint64)


class OutFormat:
    """An output format: one of ingest's names, OutFormat("2sm"), OutFormat("4ob", msb_first=False), OutFormat("s16")."""

    def __init__(self, name, msb_first=True):
        name = str(name).lower()
        self.name, self.msb_first = name, bool(msb_first)
        if name in ingest.CONTAINERS:
            self.container, self.bits, self.enc = ingest.CONTAINERS[name], 0, []
            self.sample_bits = {S8: 16, U8: 16, S16: 32, F32: 64}[self.container]
            self.target_rms = TARGET_RMS[name]
        elif name in ingest.PACKED_NAMES:
            self.container, self.bits = PACKED, int(name[0])
            n = 1 << self.bits
            lut = ingest.preset_lut(self.bits, name[1:])
            self.enc = [lut.index(2 * q - (n - 1)) for q in range(n)]       # enc[q]: the code whose value is 2q - (n - 1)
            self.sample_bits = 2 * self.bits
            self.target_rms = TARGET_RMS[self.bits]
        else:
            raise ValueError("unknown format %r (the formats: %s)" % (name, ", ".join(NAMES)))
        self.unit = max(1, 8 // self.sample_bits)                          # samples per output byte

    def nbytes(self, n):
        return int(n) * self.sample_bits // 8

    def ingest_args(self):
        """the arguments of the ingest command line that reads the output back"""
        return "--format %s" % self.name + ("" if self.msb_first or self.container != PACKED else " --lsb-first")

    def torch_dtype(self, torch):
        return {S8: torch.int8, U8: torch.uint8, S16: torch.int16, F32: torch.complex64, PACKED: torch.uint8}[self.container]


def as_format(fmt):
    return fmt if isinstance(fmt, OutFormat) else OutFormat(fmt)


def make_cfg(fmt, block, window, ngains, in_bits=8):
    fmt = as_format(fmt)
    return RequantCfg(in_bits=int(in_bits), container=fmt.container, bits=fmt.bits, msb_first=int(fmt.msb_first), block=int(block), window=int(window),
                      ngains=int(ngains), enc=(ctypes.c_uint8 * 16)(*(fmt.enc + [0] * (16 - len(fmt.enc)))))


def out_end(fmt, block, window, in_end):
    """the end of the outputs that a recording known up to input sample in_end - 1 supports: all of it once W whole blocks are there,
    in whole output bytes"""
    return streaming.out_end(block, window, in_end, fmt.unit)


def _device_bytes(engine, data):
    return streaming.device_flat(engine, data, ("uint8", "int8", "int16"), "data must be a flat int8, uint8 or int16 CUDA tensor or a bytes-like object",
                                 "uint8")


class Requantizer(streaming.Handle):
    """The open device side of one configuration (gacq_requant_open: the tables are uploaded once); run() is asynchronous on torch's
    current stream.  stats() reads what the runs so far have counted.  Closed with its engine at the latest."""
    _close, _what = "gacq_requant_close", "requantizer"

    def __init__(self, engine, fmt, gains, thresholds, block=BLOCK, window=WINDOW, in_bits=8):
        self.engine, self.fmt, self.block, self.window, self.in_bits = engine, as_format(fmt), int(block), int(window), int(in_bits)
        self.gains = np.ascontiguousarray(gains, dtype=np.float32).reshape(-1)
        self.thresholds = np.ascontiguousarray(thresholds, dtype=np.uint64).reshape(-1)
        if len(self.thresholds) != max(len(self.gains), 1) - 1:
            raise ValueError("K gains take K - 1 thresholds")
        self.cfg = make_cfg(self.fmt, self.block, self.window, len(self.gains), self.in_bits)
        self.in_bytes = 2 * self.in_bits // 8                               # per input sample
        thr = self.thresholds if len(self.thresholds) else np.zeros(1, dtype=np.uint64)
        self._open(engine, nat.lib.gacq_requant_open, ctypes.addressof(self.cfg), ctypes.c_void_p(self.gains.ctypes.data), ctypes.c_void_p(thr.ctypes.data),
                   stats=True)

    def run(self, d, in_first, out_first, n_out, trace=False):
        """outputs out_first .. out_first + n_out - 1 of the recording whose samples in_first .. are the bytes of the flat uint8 CUDA
        tensor d: a flat tensor of the format's type (int8 / uint8 / int16 pairs, complex64, bytes of packed codes); with trace also
        the uint8 gain indices of the blocks that begin in the range"""
        torch = nat.require_torch()
        self._check_open()
        n_out, out_first = int(n_out), int(out_first)
        out = torch.empty(self.fmt.nbytes(max(n_out, 0)), dtype=torch.uint8, device=d.device)
        nblk = streaming.owned_blocks(self.block, out_first, n_out)
        kidx = torch.empty(nblk, dtype=torch.uint8, device=d.device) if trace else None
        streaming.launch(self.engine, [d], d.numel(), out, n_out, lambda src, dst: nat.check(
            nat.lib.gacq_requant_run_dev(self._h, ctypes.c_void_p(src[0]), int(in_first), d.numel() // self.in_bytes, out_first, n_out, ctypes.c_void_p(dst),
                                         ctypes.c_void_p(self._stats.data_ptr()), ctypes.c_void_p(kidx.data_ptr()) if trace and nblk else None),
            self.engine._ctx))
        out = out.view(self.fmt.torch_dtype(torch))
        return (out, kidx) if trace else out


def convert(engine, fmt, data, gains, thresholds, block=BLOCK, window=WINDOW, in_bits=8, trace=False):
    """One whole recording (a flat CUDA tensor or a bytes-like object of int8 or int16 pairs, from sample 0): every output it
    supports.  (output tensor, (clipped, blocks)) and with trace the gain indices as a third."""
    fmt = as_format(fmt)
    d = _device_bytes(engine, data)
    with Requantizer(engine, fmt, gains, thresholds, block, window, in_bits) as rq:
        n_in = d.numel() // rq.in_bytes
        got = rq.run(d, 0, 0, out_end(fmt, block, window, n_in), trace)
        st = rq.stats()
    return (got[0], st, got[1]) if trace else (got, st)


class Stream(streaming.Chunks):
    """A recording fed chunk by chunk: feed(chunk) returns the outputs the chunk completes, and the concatenation of what the calls
    return is what one convert() of the whole recording gives; so are stats() and, with trace, the gain indices.  What the next
    outputs still need stays on the device: the W blocks under the next output's level, the samples of an output byte that the chunk
    cut, and the bytes of a cut sample."""

    def __init__(self, engine, fmt, gains, thresholds, block=BLOCK, window=WINDOW, in_bits=8, trace=False):
        self.rq = Requantizer(engine, fmt, gains, thresholds, block, window, in_bits)
        self.engine, self.fmt, self.trace = engine, self.rq.fmt, bool(trace)
        self.indices = []            # trace: the gain indices, call by call
        rq = self.rq
        super().__init__(8 * rq.in_bytes, lambda in_first, in_count: out_end(self.fmt, rq.block, rq.window, in_first + in_count), self._run,
                         lambda out: first_needed(rq.block, rq.window, out))

    def _run(self, ds, in_first, in_count, out_first, n_out, k):
        got = self.rq.run(ds[0], in_first, out_first, n_out, self.trace)
        if self.trace:
            got, kidx = got
            self.indices.append(kidx)
        return got

    def feed(self, chunk):
        return self.feed_all([_device_bytes(self.engine, chunk)])

    def stats(self):
        return self.rq.stats()

    def close(self):
        self.rq.close()


def convert_file(engine, fmt, fin, fout, gains, thresholds, block=BLOCK, window=WINDOW, in_bits=8, ftrace=None, piece_bytes=rawfile.PIECE_BYTES):
    """Convert the open binary file fin into fout piece by piece.  (samples written, clipped components, lowest and highest gain index
    used; None, None without output)."""
    st = Stream(engine, fmt, gains, thresholds, block, window, in_bits, trace=True)
    n, lo, hi = 0, None, None

    def feed(piece):
        nonlocal n, lo, hi
        out = st.feed(piece)
        n += out.numel() * out.element_size() * 8 // st.fmt.sample_bits
        k = st.indices.pop().cpu().numpy()
        if len(k):
            lo = int(k.min()) if lo is None else min(lo, int(k.min()))
            hi = int(k.max()) if hi is None else max(hi, int(k.max()))
            if ftrace is not None:
                ftrace.write(k.tobytes())
        return [out]

    try:
        streaming.pump(rawfile.read_pieces(fin, 2 * in_bits // 8, piece_bytes), lambda held: feed, [fout], 1)
        clipped = st.stats()[0]
    finally:
        st.close()
    return n, clipped, lo, hi


def build_parser():
    ap = argparse.ArgumentParser(prog="requant", description="Level control and requantisation of an int8 / int16 I/Q recording on the GPU")
    ap.add_argument("--format", required=True, help="output format: %s" % " ".join(NAMES))
    ap.add_argument("--in-format", default="s8", choices=("s8", "s16"), help="input format (default %(default)s)")
    ap.add_argument("--lsb-first", action="store_true", help="packed codes: the first code of a byte goes into its low bits")
    ap.add_argument("--block", type=int, default=BLOCK, help="samples per power block, a multiple of 16 in 16..%d (default %%(default)s)" % MAX_BLOCK)
    ap.add_argument("--window", type=int, default=WINDOW, help="blocks the level sums over, 1..%d (default %%(default)s)" % MAX_WINDOW)
    g = ap.add_mutually_exclusive_group()
    g.add_argument("--gain", type=float, default=None, help="one fixed gain instead of the level control")
    g.add_argument("--target-rms", type=float, default=None, help="rms of the complex output sample the level control aims at (default: by format)")
    ap.add_argument("--trace", default=None, help="file for the gain index of every block, one byte each")
    ap.add_argument("--device", type=int, default=0, help="GPU index")
    ap.add_argument("input_filename")
    ap.add_argument("output_filename")
    return ap


def parse(argv):
    """(argparse namespace, OutFormat, G, T) of a command line"""
    a = build_parser().parse_args(list(argv))
    try:
        fmt = OutFormat(a.format, msb_first=not a.lsb_first)
    except ValueError as e:
        raise SystemExit("requant: %s" % e)
    if a.block < 16 or a.block > MAX_BLOCK or a.block % 16 or not 1 <= a.window <= MAX_WINDOW:
        raise SystemExit("requant: --block is a multiple of 16 in 16..%d and --window lies in 1..%d" % (MAX_BLOCK, MAX_WINDOW))
    for v in (a.gain, a.target_rms):
        if v is not None and not streaming.positive_finite_fp32(v):
            raise SystemExit("requant: need a positive, finite --gain / --target-rms")
    if a.gain is not None:
        G, T = fixed(a.gain)
    else:
        G, T = tables(fmt.target_rms if a.target_rms is None else a.target_rms, a.block, a.window)
    return a, fmt, G, T


def report_lines(fmt, block, window, G, lo, hi, clipped, samples):
    g_lo, g_hi = (float(G[hi]), float(G[lo])) if lo is not None else (float("nan"), float("nan"))        # a higher index is a lower gain
    return ["format %s block %d window %d gain %r .. %r clipped %d samples %d" % (fmt.name, block, window, g_lo, g_hi, int(clipped), int(samples)),
            "ingest " + fmt.ingest_args()]


def run(argv, out=None, piece_bytes=rawfile.PIECE_BYTES):
    a, fmt, G, T = parse(argv)
    with streaming.shell(a.device, [a.input_filename], [a.output_filename], a.trace, out) as sh:
        n, clipped, lo, hi = convert_file(sh.engine, fmt, sh.fins[0], sh.fouts[0], G, T, a.block, a.window, 16 if a.in_format == "s16" else 8, sh.ftrace,
                                          piece_bytes)
    lines = report_lines(fmt, a.block, a.window, G, lo, hi, clipped, n)
    for line in lines:
        print(line, file=sh.report)
    return lines


def main(argv=None):
    return streaming.main(argv, __doc__, run)


if __name__ == "__main__":
    sys.exit(main())
