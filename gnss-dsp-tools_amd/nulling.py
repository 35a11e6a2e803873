"""Spatial nulling with an antenna array on the GPU (csrc/gacq_null.hip, gacq_null_*): M int8 I/Q recordings sampled on one clock in,
one recording out, under block-wise weights that minimise the output power subject to one linear constraint -- with the default
constraint the reference antenna (the first file) passes with gain 1 and up to M - 1 directions of interference are nulled, a
broadband jammer included.  The output is an exact function of (configuration, absolute sample index): a recording converts to the
same bytes however it is cut into calls or pieces.

    python -m gnss_dsp_tools_amd.nulling [--block N] [--window W] [--load-shift S] [--constraint RE,IM ...] [--gain G | --target-rms R]
           [--complex64] [--weights-trace FILE] --out OUT IN0 IN1 [IN2 ...]

reads the M files (or FIFOs) piece by piece in lockstep, writes OUT (or - for stdout) and prints one line (to stderr when OUT is -):

    antennas <M> block <Lb> window <W> gain <G> clipped <C> samples <N>

The weights of block b (N samples, default 4096) come from the covariance of the W blocks before it (default 8; of the first W blocks
during the warm-up), loaded with (trace >> S) + 1 on the diagonal (default S = 10).  --constraint gives the M complex entries of an MVDR
steering vector instead of (1, 0, .., 0).  Without --gain the gain is --target-rms (default 32) over the rms of the first 65536 output
samples at gain 1.  --weights-trace writes the quantised weights of every block, M int32 pairs each (weight = value / 16384).  Files
of unequal length end at the shortest; a recording shorter than W blocks gives no output.  The definition is in include/gacq.h;
tests/nulling_oracle.py restates it in numpy."""
import argparse
import ctypes
import sys

import numpy as np

from . import _native as nat
from . import ingest, rawfile, streaming
from .streaming import first_needed, out_end, owned_blocks      # the block / window algebra, part of this module as before

MAX_ANTENNAS, MAX_WINDOW, MAX_BLOCK, MAX_SHIFT = 8, 64, 32768, 40
BLOCK, WINDOW, LOAD_SHIFT = 4096, 8, 10
AUTO_SAMPLES = ingest.AUTO_SAMPLES
TARGET_RMS = ingest.TARGET_RMS
WQ = 1 << 14


class NullCfg(ctypes.Structure):                    # gacq_null_cfg
    _fields_ = [("antennas", ctypes.c_int), ("block", ctypes.c_int), ("window", ctypes.c_int), ("load_shift", ctypes.c_int), ("c", ctypes.c_double * 16)]


def make_cfg(M, block=BLOCK, window=WINDOW, load_shift=LOAD_SHIFT, constraint=None):
    M = int(M)
    c = np.zeros(16, dtype=np.float64)
    if constraint is None:
        c[0] = 1.0
    else:
        z = np.asarray(constraint, dtype=np.complex128).reshape(-1)
        if len(z) != M or not 1 <= M <= MAX_ANTENNAS:
            raise ValueError("the constraint takes one complex entry per antenna")
        c[0:2 * M:2], c[1:2 * M:2] = z.real, z.imag
    return NullCfg(antennas=M, block=int(block), window=int(window), load_shift=int(load_shift), c=(ctypes.c_double * 16)(*c))


def _device_int8(engine, data):
    return streaming.device_flat(engine, data, ("uint8", "int8"), "an antenna's data must be a flat int8 or uint8 CUDA tensor or a bytes-like object", "int8")


class Nuller(streaming.Handle):
    """The open device side of one configuration (gacq_null_open); run() is asynchronous on torch's current stream.  stats() reads what
    the runs so far have counted.  Closed with its engine at the latest."""
    _close, _what = "gacq_null_close", "nuller"

    def __init__(self, engine, M, block=BLOCK, window=WINDOW, load_shift=LOAD_SHIFT, constraint=None):
        self.engine, self.M, self.block, self.window, self.load_shift = engine, int(M), int(block), int(window), int(load_shift)
        self.cfg = make_cfg(self.M, block, window, load_shift, constraint)
        self._open(engine, nat.lib.gacq_null_open, ctypes.addressof(self.cfg), stats=True)

    def run(self, d_inputs, in_first, out_first, n_out, gain, dtype="int8", weights=False, cov=False):
        """outputs out_first .. out_first + n_out - 1 of the recordings whose samples in_first .. are the int8 pairs of the M flat int8
        CUDA tensors d_inputs (two entries may be one tensor): a flat int8 tensor [2 n_out] or complex64 [n_out]; with weights also the
        int32 weights [owned blocks][M][2] of the blocks that begin in the range, with cov their int64 window sums [blocks][M][M][2]"""
        torch = nat.require_torch()
        self._check_open()
        d_inputs = list(d_inputs)
        if len(d_inputs) != self.M:
            raise ValueError("%d antennas take %d inputs" % (self.M, self.M))
        n_out, out_first = int(n_out), int(out_first)
        dev = d_inputs[0].device
        cplx, out = streaming.iq_out(n_out, dtype, dev)
        nblk = owned_blocks(self.block, out_first, n_out)
        wq = torch.empty((nblk, self.M, 2), dtype=torch.int32, device=dev) if weights else None
        cv = torch.empty((nblk, self.M, self.M, 2), dtype=torch.int64, device=dev) if cov else None
        count = min(d.numel() for d in d_inputs) // 2

        def call(src, dst):
            ptrs = (ctypes.c_void_p * self.M)(*src)
            nat.check(nat.lib.gacq_null_run_dev(self._h, ctypes.cast(ptrs, ctypes.c_void_p), int(in_first), count, out_first, n_out, float(gain), int(cplx),
                                                ctypes.c_void_p(dst), ctypes.c_void_p(self._stats.data_ptr()),
                                                ctypes.c_void_p(wq.data_ptr()) if weights and nblk else None,
                                                ctypes.c_void_p(cv.data_ptr()) if cov and nblk else None), self.engine._ctx)

        streaming.launch(self.engine, d_inputs, count, out, n_out, call)
        res = (out,) + ((wq,) if weights else ()) + ((cv,) if cov else ())
        return res if len(res) > 1 else out


def convert(engine, xs, block=BLOCK, window=WINDOW, load_shift=LOAD_SHIFT, constraint=None, gain=1.0, dtype="int8", weights=False):
    """Whole recordings (one flat CUDA tensor or bytes-like object of int8 pairs per antenna, from sample 0): every output they support.
    (output tensor, (clipped, blocks)) and with weights the int32 weights as a third."""
    ds = [_device_int8(engine, x) for x in xs]
    with Nuller(engine, len(ds), block, window, load_shift, constraint) as nl:
        n_in = min(d.numel() for d in ds) // 2
        got = nl.run(ds, 0, 0, out_end(block, window, n_in), gain, dtype, weights=weights)
        st = nl.stats()
    return (got[0], st, got[1]) if weights else (got, st)


def auto_window(block, window):
    """input samples that hold the automatic gain's window"""
    return max(AUTO_SAMPLES, int(block) * int(window))


def auto_gain(engine, firsts, block=BLOCK, window=WINDOW, load_shift=LOAD_SHIFT, constraint=None, target_rms=TARGET_RMS):
    """target_rms over the rms of the first P output samples at gain 1, P = min(what the first pieces support, 65536): the rule and the
    rms_gain of ingest.py, evaluated on the host in float64 from the device's own complex64 output"""
    ds = [_device_int8(engine, x) for x in firsts]
    p = min(out_end(block, window, min(d.numel() for d in ds) // 2), AUTO_SAMPLES)
    if p < 1:
        raise ValueError("automatic gain: the recordings are shorter than the window's %d blocks" % int(window))
    with Nuller(engine, len(ds), block, window, load_shift, constraint) as nl:
        return ingest.rms_gain(nl.run(ds, 0, 0, p, 1.0, "complex64").cpu().numpy(), target_rms)


class Stream(streaming.Chunks):
    """Recordings fed piece by piece: feed(pieces) takes one piece per antenna (of equal length) and returns the outputs the pieces
    complete; the concatenation of what the calls return is what one convert() of the whole recordings gives, and so are stats() and
    the weights.  The W blocks under the next output's weights stay on the device."""

    def __init__(self, engine, M, gain, block=BLOCK, window=WINDOW, load_shift=LOAD_SHIFT, constraint=None, dtype="int8", weights=False):
        self.nl = Nuller(engine, M, block, window, load_shift, constraint)
        self.engine, self.gain, self.dtype, self.weights = engine, float(gain), dtype, bool(weights)
        self.traces = []             # weights: the weights, call by call
        nl = self.nl
        super().__init__(16, lambda in_first, in_count: out_end(nl.block, nl.window, in_first + in_count), self._run,
                         lambda out: first_needed(nl.block, nl.window, out))

    def _run(self, ds, in_first, in_count, out_first, n_out, k):
        got = self.nl.run(ds, in_first, out_first, n_out, self.gain, self.dtype, weights=self.weights)
        if self.weights:
            got, w = got
            self.traces.append(w)
        return got

    def feed(self, pieces):
        ds = [_device_int8(self.engine, p) for p in pieces]
        if len(ds) != self.nl.M or len(set(d.numel() for d in ds)) != 1 or ds[0].numel() % 2:
            raise ValueError("one piece per antenna, all of one length, in whole samples")
        return self.feed_all(ds)

    def stats(self):
        return self.nl.stats()

    def close(self):
        self.nl.close()


def lockstep(fins, piece_bytes=rawfile.PIECE_BYTES):
    """Yield lists of one int8 piece per file, cut to the shortest; ends where the first file ends"""
    its = [rawfile.read_pieces(f, 2, piece_bytes) for f in fins]
    while True:
        ps = [next(it, None) for it in its]
        if any(p is None for p in ps):
            return
        n = min(len(p) for p in ps)
        yield [p[:n] for p in ps]
        if any(len(p) != len(ps[0]) for p in ps) or n < max(1, int(piece_bytes) // 2) * 2:
            return


def convert_files(engine, fins, fout, block=BLOCK, window=WINDOW, load_shift=LOAD_SHIFT, constraint=None, gain=None, target_rms=TARGET_RMS,
                  dtype="int8", ftrace=None, piece_bytes=rawfile.PIECE_BYTES):
    """Read the open binary files fins in lockstep, piece by piece, and write the nulled recording to fout.  gain None: the automatic
    gain, that of the first 65536 outputs whatever the piece size (shorter pieces are read ahead until they hold its window).
    (gain, samples written, clipped components)."""
    M = len(fins)
    st = None
    window_in = 0 if gain is not None else auto_window(block, window)

    def feed(ps):
        out = st.feed(ps)
        w = st.traces.pop()
        if ftrace is not None and w.numel():
            ftrace.write(w.cpu().numpy().tobytes())
        return [out]

    def start(held):
        nonlocal st, gain
        if gain is None and not held:
            gain = 1.0
        if gain is None:
            firsts = [np.concatenate([h[p] for h in held])[:2 * window_in] for p in range(M)]
            gain = auto_gain(engine, firsts, block, window, load_shift, constraint, target_rms) if out_end(block, window, len(firsts[0]) // 2) else 1.0
        st = Stream(engine, M, gain, block, window, load_shift, constraint, dtype, weights=True)
        return feed

    try:
        n = streaming.pump(lockstep(fins, piece_bytes), start, [fout], 2 if dtype == "int8" else 1, 2 * window_in, lambda ps: len(ps[0]))
        if n is None:
            start([])
        clipped = st.stats()[0]
    finally:
        if st is not None:
            st.close()
    return gain, n[0] if n else 0, clipped


def _complex(text):
    try:
        re, im = text.split(",")
        return complex(float(re), float(im))
    except ValueError:
        raise argparse.ArgumentTypeError("a constraint entry is RE,IM, not %r" % (text,))


def build_parser():
    ap = argparse.ArgumentParser(prog="nulling", description="Null interference with an antenna array: adaptive weights over int8 I/Q recordings on the GPU")
    ap.add_argument("--block", type=int, default=BLOCK, help="samples per covariance block, a multiple of 64 in 64..%d (default %%(default)s)" % MAX_BLOCK)
    ap.add_argument("--window", type=int, default=WINDOW, help="blocks the covariance sums over, 1..%d (default %%(default)s)" % MAX_WINDOW)
    ap.add_argument("--load-shift", type=int, default=LOAD_SHIFT, help="diagonal loading (trace >> S) + 1, S in 0..%d (default %%(default)s)" % MAX_SHIFT)
    ap.add_argument("--constraint", type=_complex, nargs="+", default=None, metavar="RE,IM", help="steering vector, one entry per antenna (default 1,0 0,0 ..)")
    g = ap.add_mutually_exclusive_group()
    g.add_argument("--gain", type=float, default=None, help="a fixed gain instead of the automatic one")
    g.add_argument("--target-rms", type=float, default=TARGET_RMS, help="rms the automatic gain aims at (default %(default)s)")
    ap.add_argument("--complex64", action="store_true", help="write complex64 instead of int8")
    ap.add_argument("--weights-trace", default=None, metavar="FILE", help="file for the quantised weights of every block, M int32 pairs each")
    ap.add_argument("--device", type=int, default=0, help="GPU index")
    ap.add_argument("--out", required=True, help="output file, or - for stdout")
    ap.add_argument("inputs", nargs="+", metavar="IN", help="one int8 I/Q recording per antenna, the reference antenna first")
    return ap


def parse(argv):
    """the argparse namespace of a command line, checked"""
    a = build_parser().parse_args(list(argv))
    M = len(a.inputs)
    if not 2 <= M <= MAX_ANTENNAS:
        raise SystemExit("nulling: need 2..%d input files, one per antenna" % MAX_ANTENNAS)
    if a.block < 64 or a.block > MAX_BLOCK or a.block % 64 or not 1 <= a.window <= MAX_WINDOW or not 0 <= a.load_shift <= MAX_SHIFT:
        raise SystemExit("nulling: --block is a multiple of 64 in 64..%d, --window lies in 1..%d and --load-shift in 0..%d" % (MAX_BLOCK, MAX_WINDOW, MAX_SHIFT))
    if a.constraint is not None:
        z = np.asarray(a.constraint, dtype=np.complex128)
        if len(z) != M or not np.all(np.isfinite(z.view(np.float64))) or not np.any(z != 0):
            raise SystemExit("nulling: --constraint takes %d finite entries RE,IM, not all zero" % M)
    for v in (a.gain, a.target_rms):
        if v is not None and not streaming.positive_finite_fp32(v):
            raise SystemExit("nulling: need a positive, finite --gain / --target-rms")
    return a


def report_line(M, block, window, gain, clipped, samples):
    return "antennas %d block %d window %d gain %r clipped %d samples %d" % (M, block, window, float(gain), int(clipped), int(samples))


def run(argv, out=None, piece_bytes=rawfile.PIECE_BYTES):
    a = parse(argv)
    with streaming.shell(a.device, a.inputs, [a.out], a.weights_trace, out, stdin=False) as sh:
        gain, n, clipped = convert_files(sh.engine, sh.fins, sh.fouts[0], a.block, a.window, a.load_shift, a.constraint, a.gain, a.target_rms,
                                         "complex64" if a.complex64 else "int8", sh.ftrace, piece_bytes)
    line = report_line(len(a.inputs), a.block, a.window, gain, clipped, n)
    print(line, file=sh.report)
    return line


def main(argv=None):
    return streaming.main(argv, __doc__, run)


if __name__ == "__main__":
    sys.exit(main())
