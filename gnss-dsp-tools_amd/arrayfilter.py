"""The Python core that the antenna-array tools share -- nulling, stap, beams: each takes M int8 I/Q recordings in lockstep and gives one
recording (beams: K recordings, one per constraint, and then a list wherever the others have one output, gain or clip count) under
block-wise weights, through gacq_*_open / gacq_*_run_dev / gacq_*_close entry points of one shape (csrc/gacq_arrayhost.h).
Here are the open handle and its run(), the one-call convert, the automatic gain, the piece-by-piece Stream, the file pump, the common
command-line options with their checks, and the command-line run.  A tool's module keeps its --help text, its cfg, its handle subclass,
its tap algebra, its own options and its report line, and describes itself to this one with a Tool."""
import argparse
import collections
import ctypes

import numpy as np

from . import _native as nat
from . import ingest, rawfile, streaming

MAX_ANTENNAS, MAX_WINDOW, MAX_BLOCK, MAX_SHIFT = 8, 64, 32768, 40
BLOCK, WINDOW, LOAD_SHIFT = 4096, 8, 10
AUTO_SAMPLES = ingest.AUTO_SAMPLES
TARGET_RMS = ingest.TARGET_RMS
WQ = 1 << 14

# What this module knows of a tool: its name in messages; its handle class, opened as handle(engine, M, *opts) where opts are the tool's
# options in that order; and for those opts the window in blocks and the tap algebra: out_end(opts, in_end), first_needed(opts, out),
# auto_window(opts).
Tool = collections.namedtuple("Tool", "name handle window out_end first_needed auto_window")


def constraint_c(M, constraint):
    """the c of a cfg: (1, 0, .., 0), or the M complex entries of `constraint`, as 16 doubles"""
    c = np.zeros(16, dtype=np.float64)
    if constraint is None:
        c[0] = 1.0
    else:
        z = np.asarray(constraint, dtype=np.complex128).reshape(-1)
        if len(z) != M or not 1 <= M <= MAX_ANTENNAS:
            raise ValueError("the constraint takes one complex entry per antenna")
        c[0:2 * M:2], c[1:2 * M:2] = z.real, z.imag
    return (ctypes.c_double * 16)(*c)


def _device_int8(engine, data):
    return streaming.device_flat(engine, data, ("uint8", "int8"), "an antenna's data must be a flat int8 or uint8 CUDA tensor or a bytes-like object", "int8")


class Handle(streaming.Handle):
    """The open device side of one configuration; run() is asynchronous on torch's current stream.  stats() reads what the runs so far
    have counted.  Closed with its engine at the latest.  A subclass names its gacq_*_open, gacq_*_run_dev and gacq_*_close and calls
    _start() with its cfg and the weights it has per block -- and, if its run_dev takes K gains and K outputs (beams), with K."""
    _opener = _runner = None

    def _start(self, engine, cfg, weights_per_block, outputs=None):
        self.cfg, self.weights_per_block, self.outputs = cfg, int(weights_per_block), outputs
        self.M, self.block, self.window, self.load_shift = cfg.antennas, cfg.block, cfg.window, cfg.load_shift
        self._open(engine, getattr(nat.lib, self._opener), ctypes.addressof(cfg), stats=2 if outputs is None else outputs + 1)

    def stats(self):
        """(components the clip changed, blocks) over the runs so far; with K outputs the first is a list, one count per output"""
        if self.outputs is None:
            return super().stats()
        st = [int(v) for v in self._stats.cpu().tolist()]
        return st[:-1], st[-1]

    def run(self, d_inputs, in_first, out_first, n_out, gain, dtype="int8", weights=False, cov=False):
        """outputs out_first .. out_first + n_out - 1 of the recordings whose samples in_first .. are the int8 pairs of the M flat int8
        CUDA tensors d_inputs (two entries may be one tensor): a flat int8 tensor [2 n_out] or complex64 [n_out]; with weights also the
        int32 weights [owned blocks][N][2] of the blocks that begin in the range, with cov their int64 window sums [blocks][N][N][2],
        N = weights_per_block.  With K outputs: `gain` holds K gains, the output is a list of K tensors and the weights are
        [owned blocks][K][N][2]."""
        torch = nat.require_torch()
        self._check_open()
        d_inputs = list(d_inputs)
        if len(d_inputs) != self.M:
            raise ValueError("%d antennas take %d inputs" % (self.M, self.M))
        n_out, out_first, N = int(n_out), int(out_first), self.weights_per_block
        dev = d_inputs[0].device
        K = self.outputs
        if K is not None:
            gain = [float(g) for g in gain]
            if len(gain) != K:
                raise ValueError("%d beams take %d gains" % (K, K))
        cplx, out = streaming.iq_out(n_out, dtype, dev)
        outs = [out] + [streaming.iq_out(n_out, dtype, dev)[1] for _ in range(1, K or 1)]
        nblk = streaming.owned_blocks(self.block, out_first, n_out)
        wq = torch.empty((nblk, N, 2) if K is None else (nblk, K, N, 2), dtype=torch.int32, device=dev) if weights else None
        cv = torch.empty((nblk, N, N, 2), dtype=torch.int64, device=dev) if cov else None
        count = min(d.numel() for d in d_inputs) // 2
        run_dev = getattr(nat.lib, self._runner)

        def call(src, dst):
            ptrs = (ctypes.c_void_p * self.M)(*src)
            if K is None:
                g, to = float(gain), ctypes.c_void_p(dst)
            else:                                    # an output without elements borrows an address, as streaming.launch has it
                gains = (ctypes.c_double * K)(*gain)
                dsts = (ctypes.c_void_p * K)(*[o.data_ptr() if o.numel() else dst for o in outs])
                g, to = ctypes.cast(gains, ctypes.c_void_p), ctypes.cast(dsts, ctypes.c_void_p)
            nat.check(run_dev(self._h, ctypes.cast(ptrs, ctypes.c_void_p), int(in_first), count, out_first, n_out, g, int(cplx),
                              to, ctypes.c_void_p(self._stats.data_ptr()), ctypes.c_void_p(wq.data_ptr()) if weights and nblk else None,
                              ctypes.c_void_p(cv.data_ptr()) if cov and nblk else None), self.engine._ctx)

        streaming.launch(self.engine, d_inputs, count, out, n_out, call)
        out = out if K is None else outs
        res = (out,) + ((wq,) if weights else ()) + ((cv,) if cov else ())
        return res if len(res) > 1 else out


def convert(tool, engine, xs, opts, gain=1.0, dtype="int8", weights=False):
    """Whole recordings (one flat CUDA tensor or bytes-like object of int8 pairs per antenna, from sample 0): every output they support.
    (output tensor, (clipped, blocks)) and with weights the int32 weights as a third."""
    ds = [_device_int8(engine, x) for x in xs]
    with tool.handle(engine, len(ds), *opts) as h:
        n_in = min(d.numel() for d in ds) // 2
        got = h.run(ds, 0, 0, tool.out_end(opts, n_in), gain, dtype, weights=weights)
        st = h.stats()
    return (got[0], st, got[1]) if weights else (got, st)


def auto_gain(tool, engine, firsts, opts, target_rms=TARGET_RMS):
    """target_rms over the rms of the first P output samples at gain 1, P = min(what the first pieces support, 65536): the rule and the
    rms_gain of ingest.py, evaluated on the host in float64 from the device's own complex64 output"""
    ds = [_device_int8(engine, x) for x in firsts]
    p = min(tool.out_end(opts, min(d.numel() for d in ds) // 2), AUTO_SAMPLES)
    if p < 1:
        raise ValueError("automatic gain: the recordings are shorter than the window's %d blocks" % int(tool.window(opts)))
    with tool.handle(engine, len(ds), *opts) as h:
        if h.outputs is None:
            return ingest.rms_gain(h.run(ds, 0, 0, p, 1.0, "complex64").cpu().numpy(), target_rms)
        return [ingest.rms_gain(y.cpu().numpy(), target_rms) for y in h.run(ds, 0, 0, p, [1.0] * h.outputs, "complex64")]


class Stream(streaming.Chunks):
    """Recordings fed piece by piece: feed(pieces) takes one piece per antenna (of equal length) and returns the outputs the pieces
    complete (a tool of K outputs: a list of K tensors); the concatenation of what the calls return is what one convert() of the whole
    recordings gives, and so are stats(), the weights and, with cov, the window sums.  The tail kept on the device starts at the first input sample the next output's window
    needs."""

    def __init__(self, tool, engine, M, gain, opts, dtype="int8", weights=False, cov=False):
        self.handle = tool.handle(engine, M, *opts)
        self.engine, self.dtype, self.weights, self.cov = engine, dtype, bool(weights), bool(cov)
        self.gain = float(gain) if self.handle.outputs is None else [float(g) for g in gain]
        self.traces = []             # weights: the weights, call by call
        self.covs = []               # cov: the window sums of the owned blocks, call by call
        super().__init__(16, lambda in_first, in_count: tool.out_end(opts, in_first + in_count), self._run, lambda out: tool.first_needed(opts, out))

    def _run(self, ds, in_first, in_count, out_first, n_out, k):
        got = self.handle.run(ds, in_first, out_first, n_out, self.gain, self.dtype, weights=self.weights, cov=self.cov)
        got = list(got) if isinstance(got, tuple) else [got]        # the output (K outputs: their list), then the weights, then the sums
        if self.cov:
            self.covs.append(got.pop())
        if self.weights:
            self.traces.append(got.pop())
        return got[0]

    def feed(self, pieces):
        ds = [_device_int8(self.engine, p) for p in pieces]
        if len(ds) != self.handle.M or len(set(d.numel() for d in ds)) != 1 or ds[0].numel() % 2:
            raise ValueError("one piece per antenna, all of one length, in whole samples")
        return self.feed_all(ds)

    def stats(self):
        return self.handle.stats()

    def close(self):
        self.handle.close()


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


def convert_files(tool, engine, fins, fout, opts, gain=None, target_rms=TARGET_RMS, dtype="int8", ftrace=None, piece_bytes=rawfile.PIECE_BYTES,
                  on_cov=None):
    """Read the open binary files fins in lockstep, piece by piece, and write the filtered recording to fout (a tool of K outputs: fout
    is the list of its K files, and gain, if given, and the gain and the clipped count returned are lists).  gain None: the automatic
    gain, that of the first 65536 outputs whatever the piece size (shorter pieces are read ahead until they hold its window).
    on_cov(b, cov), if given, is called piece by piece with the int64 window sums of the blocks the piece's outputs own, the first of
    them absolute block b (bearing.py).  (gain, samples written, clipped components)."""
    M = len(fins)
    many = isinstance(fout, (list, tuple))
    st = None
    window_in = 0 if gain is not None else tool.auto_window(opts)

    def feed(ps):
        first_owned = -(-st.next_out // st.handle.block)
        out = st.feed(ps)
        w = st.traces.pop()
        if ftrace is not None and w.numel():
            ftrace.write(w.cpu().numpy().tobytes())
        if on_cov is not None:
            on_cov(first_owned, st.covs.pop())
        return out if many else [out]

    def start(held):
        nonlocal st, gain
        if gain is None and not held:
            gain = [1.0] * len(fout) if many else 1.0
        if gain is None:
            firsts = [np.concatenate([h[p] for h in held])[:2 * window_in] for p in range(M)]
            gain = auto_gain(tool, engine, firsts, opts, target_rms) if tool.out_end(opts, len(firsts[0]) // 2) > 0 else ([1.0] * len(fout) if many else 1.0)
        st = Stream(tool, engine, M, gain, opts, dtype, weights=True, cov=on_cov is not None)
        return feed

    try:
        n = streaming.pump(lockstep(fins, piece_bytes), start, list(fout) if many else [fout], 2 if dtype == "int8" else 1, 2 * window_in, lambda ps: len(ps[0]))
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


def add_options(ap, weights="M", centre="", stdin="", single=True):
    """The options every array tool has, behind the tool's own; the three texts are where the help of stap differs from nulling's.
    single False (beams): without --constraint, --out and the positional inputs, which a tool of several outputs names its own way"""
    ap.add_argument("--block", type=int, default=BLOCK, help="samples per covariance block, a multiple of 64 in 64..%d (default %%(default)s)" % MAX_BLOCK)
    ap.add_argument("--window", type=int, default=WINDOW, help="blocks the covariance sums over, 1..%d (default %%(default)s)" % MAX_WINDOW)
    ap.add_argument("--load-shift", type=int, default=LOAD_SHIFT, help="diagonal loading (trace >> S) + 1, S in 0..%d (default %%(default)s)" % MAX_SHIFT)
    if single:
        ap.add_argument("--constraint", type=_complex, nargs="+", default=None, metavar="RE,IM",
                        help="steering vector%s, one entry per antenna (default 1,0 0,0 ..)" % centre)
    g = ap.add_mutually_exclusive_group()
    g.add_argument("--gain", type=float, default=None, help="a fixed gain instead of the automatic one")
    g.add_argument("--target-rms", type=float, default=TARGET_RMS, help="rms the automatic gain aims at (default %(default)s)")
    ap.add_argument("--complex64", action="store_true", help="write complex64 instead of int8")
    ap.add_argument("--weights-trace", default=None, metavar="FILE", help="file for the quantised weights of every block, %s int32 pairs each" % weights)
    ap.add_argument("--device", type=int, default=0, help="GPU index")
    if single:
        ap.add_argument("--out", required=True, help="output file, or - for stdout")
        ap.add_argument("inputs", nargs="+", metavar="IN", help="one int8 I/Q recording per antenna, the reference antenna first%s" % stdin)
    return ap


def parse(name, parser, argv, min_antennas, extra=None):
    """the argparse namespace of a command line, checked: the antennas, what extra(a, M) checks, then the common options"""
    a = parser.parse_args(list(argv))
    M = len(a.inputs)
    if not min_antennas <= M <= MAX_ANTENNAS:
        raise SystemExit("%s: need %d..%d input files, one per antenna" % (name, min_antennas, MAX_ANTENNAS))
    if extra is not None:
        extra(a, M)
    return check_options(name, a, M)


def check_options(name, a, M):
    """the checks of the common options of a parsed namespace of M antennas; the namespace"""
    if a.block < 64 or a.block > MAX_BLOCK or a.block % 64 or not 1 <= a.window <= MAX_WINDOW or not 0 <= a.load_shift <= MAX_SHIFT:
        raise SystemExit("%s: --block is a multiple of 64 in 64..%d, --window lies in 1..%d and --load-shift in 0..%d" % (name, MAX_BLOCK, MAX_WINDOW, MAX_SHIFT))
    if getattr(a, "constraint", None) is not None:
        z = np.asarray(a.constraint, dtype=np.complex128)
        if len(z) != M or not np.all(np.isfinite(z.view(np.float64))) or not np.any(z != 0):
            raise SystemExit("%s: --constraint takes %d finite entries RE,IM, not all zero" % (name, M))
    for v in (a.gain, a.target_rms):
        if v is not None and not streaming.positive_finite_fp32(v):
            raise SystemExit("%s: need a positive, finite --gain / --target-rms" % name)
    return a


def run(tool, a, opts, report_line, out=None, piece_bytes=rawfile.PIECE_BYTES, stdin=True):
    """The command line of a parsed namespace: the files, the conversion and the line report_line(gain, clipped, samples) makes"""
    with streaming.shell(a.device, a.inputs, [a.out], a.weights_trace, out, stdin=stdin) as sh:
        gain, n, clipped = convert_files(tool, sh.engine, sh.fins, sh.fouts[0], opts, a.gain, a.target_rms, "complex64" if a.complex64 else "int8",
                                         sh.ftrace, piece_bytes)
    line = report_line(gain, clipped, n)
    print(line, file=sh.report)
    return line
