"""Space-time adaptive nulling on the GPU (csrc/gacq_stap.hip, gacq_stap_*): M int8 I/Q recordings sampled on one clock in, one
recording out, every antenna under T taps.  The weight vector has M T entries and M T - 1 degrees of freedom, so narrowband
interferers are separated in frequency as well as in direction: a broadband jammer together with a few tones on a small array, or --
with one file -- an adaptive FIR notch that needs no frames or thresholds.  With the default constraint the reference antenna (the first
file) passes at its own sample index with gain 1.  T = 1 is nulling.py.  The output is an exact function of (configuration, absolute
sample index): a recording converts to the same bytes however it is cut into calls or pieces.

    python -m gnss_dsp_tools_amd.stap [--taps T] [--block N] [--window W] [--load-shift S] [--constraint RE,IM ...] [--gain G | --target-rms R]
           [--complex64] [--weights-trace FILE] --out OUT IN0 [IN1 ...]

reads the M files (or FIFOs; - is stdin) piece by piece in lockstep, writes OUT (or - for stdout) and prints one line (to stderr when
OUT is -):

    antennas <M> taps <T> block <Lb> window <W> gain <G> clipped <C> samples <N>

T is odd, 1..15 (default 5), and M T at most 56.  The weights of block b (N samples, default 4096) come from the space-time covariance
of the W blocks before it (default 8; of the first W blocks during the warm-up), loaded with (trace >> S) + 1 on the diagonal (default
S = 10).  --constraint gives the M complex entries of a steering vector, placed on the centre taps, instead of (1, 0, .., 0).  Without
--gain the gain is --target-rms (default 32) over the rms of the first 65536 output samples at gain 1.  --weights-trace writes the
quantised weights of every block, M T int32 pairs each, antenna-major (weight = value / 16384).  The last (T - 1) / 2 samples of a
recording have no output: their taps reach past its end.  The definition is in include/gacq.h; tests/stap_oracle.py restates it."""
import argparse
import ctypes
import sys

import numpy as np

from . import _native as nat
from . import ingest, nulling, rawfile, streaming
from .nulling import lockstep

MAX_ANTENNAS, MAX_TAPS, MAX_WEIGHTS, MAX_WINDOW, MAX_BLOCK, MAX_SHIFT = 8, 15, 56, 64, 32768, 40
TAPS, BLOCK, WINDOW, LOAD_SHIFT = 5, 4096, 8, 10
AUTO_SAMPLES = ingest.AUTO_SAMPLES
TARGET_RMS = ingest.TARGET_RMS
WQ = 1 << 14


class StapCfg(ctypes.Structure):                    # gacq_stap_cfg
    _fields_ = [("antennas", ctypes.c_int), ("taps", ctypes.c_int), ("block", ctypes.c_int), ("window", ctypes.c_int), ("load_shift", ctypes.c_int),
                ("c", ctypes.c_double * 16)]


def make_cfg(M, taps=TAPS, block=BLOCK, window=WINDOW, load_shift=LOAD_SHIFT, constraint=None):
    c = nulling.make_cfg(M, block, window, load_shift, constraint).c
    return StapCfg(antennas=int(M), taps=int(taps), block=int(block), window=int(window), load_shift=int(load_shift), c=c)


def centre(taps):
    """t_c: the taps reach this many samples either side"""
    return (int(taps) - 1) // 2


def out_end(block, window, in_end, taps):
    """the end of the outputs that a recording known up to input sample in_end - 1 supports: all but the last t_c once W whole blocks
    and the t_c samples after them are there"""
    tc = centre(taps)
    return in_end - tc if in_end >= int(window) * int(block) + tc else 0


def first_needed(block, window, out, taps):
    """the first input sample that output `out` needs: t_c samples before the first block of its window"""
    return max(streaming.first_needed(block, window, out) - centre(taps), 0)


owned_blocks = streaming.owned_blocks


class Stap(streaming.Handle):
    """The open device side of one configuration (gacq_stap_open); run() is asynchronous on torch's current stream.  stats() reads what
    the runs so far have counted.  Closed with its engine at the latest."""
    _close, _what = "gacq_stap_close", "space-time nuller"

    def __init__(self, engine, M, taps=TAPS, block=BLOCK, window=WINDOW, load_shift=LOAD_SHIFT, constraint=None):
        self.engine, self.M, self.taps, self.block, self.window, self.load_shift = engine, int(M), int(taps), int(block), int(window), int(load_shift)
        self.N = self.M * self.taps
        self.cfg = make_cfg(self.M, taps, block, window, load_shift, constraint)
        self._open(engine, nat.lib.gacq_stap_open, ctypes.addressof(self.cfg), stats=True)

    def run(self, d_inputs, in_first, out_first, n_out, gain, dtype="int8", weights=False, cov=False):
        """outputs out_first .. out_first + n_out - 1 of the recordings whose samples in_first .. are the int8 pairs of the M flat int8
        CUDA tensors d_inputs (two entries may be one tensor): a flat int8 tensor [2 n_out] or complex64 [n_out]; with weights also the
        int32 weights [owned blocks][M T][2] of the blocks that begin in the range, with cov their int64 window sums [blocks][M T][M T][2]"""
        torch = nat.require_torch()
        self._check_open()
        d_inputs = list(d_inputs)
        if len(d_inputs) != self.M:
            raise ValueError("%d antennas take %d inputs" % (self.M, self.M))
        n_out, out_first = int(n_out), int(out_first)
        dev = d_inputs[0].device
        cplx, out = streaming.iq_out(n_out, dtype, dev)
        nblk = owned_blocks(self.block, out_first, n_out)
        wq = torch.empty((nblk, self.N, 2), dtype=torch.int32, device=dev) if weights else None
        cv = torch.empty((nblk, self.N, self.N, 2), dtype=torch.int64, device=dev) if cov else None
        count = min(d.numel() for d in d_inputs) // 2

        def call(src, dst):
            ptrs = (ctypes.c_void_p * self.M)(*src)
            nat.check(nat.lib.gacq_stap_run_dev(self._h, ctypes.cast(ptrs, ctypes.c_void_p), int(in_first), count, out_first, n_out, float(gain), int(cplx),
                                                ctypes.c_void_p(dst), ctypes.c_void_p(self._stats.data_ptr()),
                                                ctypes.c_void_p(wq.data_ptr()) if weights and nblk else None,
                                                ctypes.c_void_p(cv.data_ptr()) if cov and nblk else None), self.engine._ctx)

        streaming.launch(self.engine, d_inputs, count, out, n_out, call)
        res = (out,) + ((wq,) if weights else ()) + ((cv,) if cov else ())
        return res if len(res) > 1 else out


def _device_int8(engine, data):
    return streaming.device_flat(engine, data, ("uint8", "int8"), "an antenna's data must be a flat int8 or uint8 CUDA tensor or a bytes-like object", "int8")


def convert(engine, xs, taps=TAPS, block=BLOCK, window=WINDOW, load_shift=LOAD_SHIFT, constraint=None, gain=1.0, dtype="int8", weights=False):
    """Whole recordings (one flat CUDA tensor or bytes-like object of int8 pairs per antenna, from sample 0): every output they support.
    (output tensor, (clipped, blocks)) and with weights the int32 weights as a third."""
    ds = [_device_int8(engine, x) for x in xs]
    with Stap(engine, len(ds), taps, block, window, load_shift, constraint) as sp:
        n_in = min(d.numel() for d in ds) // 2
        got = sp.run(ds, 0, 0, out_end(block, window, n_in, taps), gain, dtype, weights=weights)
        st = sp.stats()
    return (got[0], st, got[1]) if weights else (got, st)


def auto_window(block, window, taps):
    """input samples that hold the automatic gain's window"""
    return max(AUTO_SAMPLES, int(block) * int(window)) + centre(taps)


def auto_gain(engine, firsts, taps=TAPS, block=BLOCK, window=WINDOW, load_shift=LOAD_SHIFT, constraint=None, target_rms=TARGET_RMS):
    """target_rms over the rms of the first P output samples at gain 1, P = min(what the first pieces support, 65536): the rule and the
    rms_gain of ingest.py, evaluated on the host in float64 from the device's own complex64 output"""
    ds = [_device_int8(engine, x) for x in firsts]
    p = min(out_end(block, window, min(d.numel() for d in ds) // 2, taps), AUTO_SAMPLES)
    if p < 1:
        raise ValueError("automatic gain: the recordings are shorter than the window's %d blocks" % int(window))
    with Stap(engine, len(ds), taps, block, window, load_shift, constraint) as sp:
        return ingest.rms_gain(sp.run(ds, 0, 0, p, 1.0, "complex64").cpu().numpy(), target_rms)


class Stream(streaming.Chunks):
    """Recordings fed piece by piece: feed(pieces) takes one piece per antenna (of equal length) and returns the outputs the pieces
    complete; the concatenation of what the calls return is what one convert() of the whole recordings gives, and so are stats() and
    the weights.  The tail kept on the device starts t_c samples before the first block the next output's window needs."""

    def __init__(self, engine, M, gain, taps=TAPS, block=BLOCK, window=WINDOW, load_shift=LOAD_SHIFT, constraint=None, dtype="int8", weights=False):
        self.sp = Stap(engine, M, taps, block, window, load_shift, constraint)
        self.engine, self.gain, self.dtype, self.weights = engine, float(gain), dtype, bool(weights)
        self.traces = []             # weights: the weights, call by call
        sp = self.sp
        super().__init__(16, lambda in_first, in_count: out_end(sp.block, sp.window, in_first + in_count, sp.taps), self._run,
                         lambda out: first_needed(sp.block, sp.window, out, sp.taps))

    def _run(self, ds, in_first, in_count, out_first, n_out, k):
        got = self.sp.run(ds, in_first, out_first, n_out, self.gain, self.dtype, weights=self.weights)
        if self.weights:
            got, w = got
            self.traces.append(w)
        return got

    def feed(self, pieces):
        ds = [_device_int8(self.engine, p) for p in pieces]
        if len(ds) != self.sp.M or len(set(d.numel() for d in ds)) != 1 or ds[0].numel() % 2:
            raise ValueError("one piece per antenna, all of one length, in whole samples")
        return self.feed_all(ds)

    def stats(self):
        return self.sp.stats()

    def close(self):
        self.sp.close()


def convert_files(engine, fins, fout, taps=TAPS, block=BLOCK, window=WINDOW, load_shift=LOAD_SHIFT, constraint=None, gain=None, target_rms=TARGET_RMS,
                  dtype="int8", ftrace=None, piece_bytes=rawfile.PIECE_BYTES):
    """Read the open binary files fins in lockstep, piece by piece, and write the filtered recording to fout.  gain None: the automatic
    gain, that of the first 65536 outputs whatever the piece size (shorter pieces are read ahead until they hold its window).
    (gain, samples written, clipped components)."""
    M = len(fins)
    st = None
    window_in = 0 if gain is not None else auto_window(block, window, taps)

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
            some = out_end(block, window, len(firsts[0]) // 2, taps) > 0
            gain = auto_gain(engine, firsts, taps, block, window, load_shift, constraint, target_rms) if some else 1.0
        st = Stream(engine, M, gain, taps, block, window, load_shift, constraint, dtype, weights=True)
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


def build_parser():
    ap = argparse.ArgumentParser(prog="stap", description="Space-time adaptive nulling: M antennas x T taps over int8 I/Q recordings on the GPU")
    ap.add_argument("--taps", type=int, default=TAPS, help="taps per antenna, odd, 1..%d, antennas x taps <= %d (default %%(default)s)" % (MAX_TAPS, MAX_WEIGHTS))
    ap.add_argument("--block", type=int, default=BLOCK, help="samples per covariance block, a multiple of 64 in 64..%d (default %%(default)s)" % MAX_BLOCK)
    ap.add_argument("--window", type=int, default=WINDOW, help="blocks the covariance sums over, 1..%d (default %%(default)s)" % MAX_WINDOW)
    ap.add_argument("--load-shift", type=int, default=LOAD_SHIFT, help="diagonal loading (trace >> S) + 1, S in 0..%d (default %%(default)s)" % MAX_SHIFT)
    ap.add_argument("--constraint", type=nulling._complex, nargs="+", default=None, metavar="RE,IM",
                    help="steering vector on the centre taps, one entry per antenna (default 1,0 0,0 ..)")
    g = ap.add_mutually_exclusive_group()
    g.add_argument("--gain", type=float, default=None, help="a fixed gain instead of the automatic one")
    g.add_argument("--target-rms", type=float, default=TARGET_RMS, help="rms the automatic gain aims at (default %(default)s)")
    ap.add_argument("--complex64", action="store_true", help="write complex64 instead of int8")
    ap.add_argument("--weights-trace", default=None, metavar="FILE", help="file for the quantised weights of every block, M T int32 pairs each")
    ap.add_argument("--device", type=int, default=0, help="GPU index")
    ap.add_argument("--out", required=True, help="output file, or - for stdout")
    ap.add_argument("inputs", nargs="+", metavar="IN", help="one int8 I/Q recording per antenna, the reference antenna first; - is stdin")
    return ap


def parse(argv):
    """the argparse namespace of a command line, checked"""
    a = build_parser().parse_args(list(argv))
    M = len(a.inputs)
    if not 1 <= M <= MAX_ANTENNAS:
        raise SystemExit("stap: need 1..%d input files, one per antenna" % MAX_ANTENNAS)
    if not 1 <= a.taps <= MAX_TAPS or a.taps % 2 == 0 or M * a.taps > MAX_WEIGHTS:
        raise SystemExit("stap: --taps is odd in 1..%d and antennas x taps at most %d" % (MAX_TAPS, MAX_WEIGHTS))
    if a.inputs.count("-") > 1:
        raise SystemExit("stap: only one input can be stdin")
    if a.block < 64 or a.block > MAX_BLOCK or a.block % 64 or not 1 <= a.window <= MAX_WINDOW or not 0 <= a.load_shift <= MAX_SHIFT:
        raise SystemExit("stap: --block is a multiple of 64 in 64..%d, --window lies in 1..%d and --load-shift in 0..%d" % (MAX_BLOCK, MAX_WINDOW, MAX_SHIFT))
    if a.constraint is not None:
        z = np.asarray(a.constraint, dtype=np.complex128)
        if len(z) != M or not np.all(np.isfinite(z.view(np.float64))) or not np.any(z != 0):
            raise SystemExit("stap: --constraint takes %d finite entries RE,IM, not all zero" % M)
    for v in (a.gain, a.target_rms):
        if v is not None and not streaming.positive_finite_fp32(v):
            raise SystemExit("stap: need a positive, finite --gain / --target-rms")
    return a


def report_line(M, taps, block, window, gain, clipped, samples):
    return "antennas %d taps %d block %d window %d gain %r clipped %d samples %d" % (M, taps, block, window, float(gain), int(clipped), int(samples))


def run(argv, out=None, piece_bytes=rawfile.PIECE_BYTES):
    a = parse(argv)
    with streaming.shell(a.device, a.inputs, [a.out], a.weights_trace, out) as sh:
        gain, n, clipped = convert_files(sh.engine, sh.fins, sh.fouts[0], a.taps, a.block, a.window, a.load_shift, a.constraint, a.gain, a.target_rms,
                                         "complex64" if a.complex64 else "int8", sh.ftrace, piece_bytes)
    line = report_line(len(a.inputs), a.taps, a.block, a.window, gain, clipped, n)
    print(line, file=sh.report)
    return line


def main(argv=None):
    return streaming.main(argv, __doc__, run)


if __name__ == "__main__":
    sys.exit(main())
