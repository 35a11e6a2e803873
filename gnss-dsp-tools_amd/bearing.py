"""Bearings of interferers from antenna-array recordings on the GPU (csrc/gacq_bearing.hip, gacq_bearing_*): the minimum-variance
(Capon) spatial spectrum of every block's window covariance -- the int64 ``cov`` of ``nulling`` -- over a grid of directions, and the K
strongest peaks that lie at least --sep apart.  The results are an exact function of (configuration, absolute block index): a
recording gives the same trace however it is cut into pieces.

    python -m gnss_dsp_tools_amd.bearing --element E,N,U ... [--step DEG] [--el-min DEG] [--peaks K] [--sep DEG] [--every E] [--block N]
           [--window W] [--load-shift S] [--out OUT] [--trace FILE] IN0 IN1 [IN2 ...]

reads the M files piece by piece in lockstep (one ``--element`` east,north,up in wavelengths per file, as ``scene`` takes them), evaluates
the blocks b with b mod E = 0 (default every block), writes one line per evaluated block to --trace,

    block <b> sample <b N> <az> <el> <dB> ...        (one triple per rank; - - - where no cell is left)

and prints

    antennas <M> block <N> window <W> cells <G> blocks <B> rank 0 az <AZ> el <EL> count <C> ...

with, per rank, the cell most blocks put there (ties to the lowest cell).  dB is the contrast 10 log10(floor / q): the Capon power of
the cell over the weakest of the grid.  The grid runs over azimuths 0 <= az < 360 and elevations --el-min <= el <= 90 in steps of
--step (default 5 degrees, 1368 cells).  The covariance of block b is that of the W blocks before it (``nulling``'s window), loaded
with (trace >> S) + 1.  With --out the nulled recording of the same pass is written as ``nulling`` writes it at its defaults.  The
definition is in include/gacq.h; tests/bearing_oracle.py restates it in numpy."""
import argparse
import collections
import ctypes
import math
import sys

import numpy as np

from . import _native as nat
from . import arrayfilter, nulling, rawfile, scene, streaming

MAX_CELLS, MAX_PEAKS = 32768, 4
STEP, PEAKS, SEP = 5.0, 3, 20.0
PEAK = np.dtype([("cell", "<i4"), ("zero", "<i4"), ("q", "<f8")])     # a record of gacq_bearing_run_dev


BearingCfg = nat.struct("gacq_bearing_cfg")


def grid(step_deg, el_min=0.0):
    """The (az, el) cells in degrees, float64 [G, 2], elevation-major: el_min, el_min + step, .. <= 90, and under each 0, step, .. < 360"""
    step, el_min = float(step_deg), float(el_min)
    if not (step > 0.0 and math.isfinite(step) and 0.0 <= el_min <= 90.0):
        raise ValueError("the grid needs a step > 0 and 0 <= el_min <= 90")
    az = [i * step for i in range(int(math.ceil(360.0 / step)) + 1) if i * step < 360.0]
    el = [el_min + i * step for i in range(int(math.floor((90.0 - el_min) / step + 1e-9)) + 1)]
    return np.array([(a, e) for e in el for a in az], dtype=np.float64).reshape(-1, 2)


def tables(elements, cells):
    """(a, u) of gacq_bearing_open: a[g] = scene.steering(elements, az_g, el_g), complex128 [G, M], and u[g] its direction, float64 [G, 3]"""
    cells = np.asarray(cells, dtype=np.float64).reshape(-1, 2)
    a = np.stack([scene.steering(elements, az, el) for az, el in cells])
    az, el = np.deg2rad(cells[:, 0]), np.deg2rad(cells[:, 1])
    u = np.stack([np.cos(el) * np.sin(az), np.cos(el) * np.cos(az), np.sin(el)], axis=1)
    return np.ascontiguousarray(a, dtype=np.complex128), np.ascontiguousarray(u, dtype=np.float64)


def records(peaks):
    """the records of a run as a numpy structured array [n][K] (fields cell, zero, q)"""
    if isinstance(peaks, np.ndarray) and peaks.dtype == PEAK:
        return peaks
    p = peaks.cpu().numpy() if hasattr(peaks, "cpu") else np.asarray(peaks)
    return np.ascontiguousarray(p).view(np.uint8).reshape(p.shape[0], -1).view(PEAK)


class Finder(streaming.Handle):
    """The open device side of one array and grid (gacq_bearing_open): run() is asynchronous on torch's current stream.  Closed with its
    engine at the latest.  ``elements`` [M, 3] in wavelengths, ``cells`` [G, 2] (az, el) in degrees; from_tables() takes a and u as
    they are."""
    _close, _what = "gacq_bearing_close", "finder"

    def __init__(self, engine, elements, cells, load_shift=arrayfilter.LOAD_SHIFT, peaks=PEAKS, sep_deg=SEP):
        self.cells = np.asarray(cells, dtype=np.float64).reshape(-1, 2)
        a, u = tables(elements, self.cells)
        self._start(engine, a, u, load_shift, peaks, math.cos(math.radians(float(sep_deg))))

    @classmethod
    def from_tables(cls, engine, a, u, load_shift=arrayfilter.LOAD_SHIFT, peaks=PEAKS, cos_sep=1.0):
        self = cls.__new__(cls)
        self.cells = None
        self._start(engine, a, u, load_shift, peaks, cos_sep)
        return self

    def _start(self, engine, a, u, load_shift, peaks, cos_sep):
        a = np.ascontiguousarray(a, dtype=np.complex128)
        u = np.ascontiguousarray(u, dtype=np.float64)
        if a.ndim != 2 or u.shape != (a.shape[0], 3):
            raise ValueError("the tables are a [G, M] and u [G, 3]")
        self.cfg = BearingCfg(antennas=a.shape[1], load_shift=int(load_shift), cells=a.shape[0], peaks=int(peaks), cos_sep=float(cos_sep))
        self.M, self.G, self.K = a.shape[1], a.shape[0], int(peaks)
        self._open(engine, nat.lib.gacq_bearing_open, ctypes.addressof(self.cfg), a.ctypes.data, u.ctypes.data)

    def run(self, cov, stride=1, spectrum=False):
        """(peaks, floor) of the blocks whose covariances are rows 0, stride, 2 stride, .. of cov, an int64 CUDA tensor [rows][M][M][2]
        as Nuller.run(.., cov=True) returns it (or a numpy array, which is uploaded): peaks a uint8 tensor [n][K][16] of records (see
        records()), floor float64 [n]; with spectrum also q, float64 [n][G]"""
        torch = nat.require_torch()
        self._check_open()
        if not torch.is_tensor(cov):
            cov = torch.from_numpy(np.ascontiguousarray(cov, dtype=np.int64)).to("cuda:%d" % self.engine.device)
        stride = int(stride)
        if cov.dtype != torch.int64 or not cov.is_cuda or tuple(cov.shape[1:]) != (self.M, self.M, 2) or not cov.is_contiguous() or stride < 1:
            raise ValueError("cov is a contiguous int64 CUDA tensor [rows][%d][%d][2], stride >= 1" % (self.M, self.M))
        n = -(-cov.shape[0] // stride)
        dev = cov.device
        pk = torch.empty((n, self.K, 16), dtype=torch.uint8, device=dev)
        fl = torch.empty((n,), dtype=torch.float64, device=dev)
        sp = torch.empty((n, self.G), dtype=torch.float64, device=dev) if spectrum else None
        if n:
            self.engine.use_torch_stream(dev)
            nat.check(nat.lib.gacq_bearing_run_dev(self._h, ctypes.c_void_p(cov.data_ptr()), n, stride, ctypes.c_void_p(pk.data_ptr()),
                                                   ctypes.c_void_p(fl.data_ptr()), ctypes.c_void_p(sp.data_ptr()) if spectrum else None),
                      self.engine._ctx)
        return (pk, fl, sp) if spectrum else (pk, fl)

    def report(self, peaks, floor):
        """[n][K] triples (az, el, contrast_db) as float64 [n, K, 3], contrast_db = 10 log10(floor / q); nan where no cell is left"""
        return report(self.cells, peaks, floor)


def report(cells, peaks, floor):
    rec = records(peaks)
    fl = floor.cpu().numpy() if hasattr(floor, "cpu") else np.asarray(floor, dtype=np.float64)
    out = np.full(rec.shape + (3,), np.nan)
    have = rec["cell"] >= 0
    out[have, 0:2] = np.asarray(cells, dtype=np.float64)[rec["cell"][have]]
    with np.errstate(all="ignore"):
        out[have, 2] = 10.0 * np.log10(np.broadcast_to(fl[:, None], rec.shape)[have] / rec["q"][have])
    return out


def trace_line(b, block, triples):
    """the trace line of absolute block b"""
    return "block %d sample %d %s" % (b, b * block, " ".join("- - -" if math.isnan(t[0]) else "%.2f %.2f %.2f" % tuple(t) for t in triples))


def most_frequent(cells_of_rank):
    """(cell, count) of the cell most blocks have, ties to the lowest cell; None when no block has one"""
    count = collections.Counter(int(g) for g in cells_of_rank if g >= 0)
    return min(count.items(), key=lambda kv: (-kv[1], kv[0])) if count else None


def summary_line(M, block, window, cells, rec):
    """the printed line of all evaluated blocks' records [B][K]"""
    text = "antennas %d block %d window %d cells %d blocks %d" % (M, block, window, len(cells), rec.shape[0])
    for k in range(rec.shape[1]):
        top = most_frequent(rec["cell"][:, k])
        text += " rank %d none" % k if top is None else " rank %d az %.2f el %.2f count %d" % (k, cells[top[0]][0], cells[top[0]][1], top[1])
    return text


def evaluated(first_owned, nblk, every):
    """(offset of the first evaluated row, the absolute blocks) among owned blocks first_owned .. first_owned + nblk - 1: those that
    are multiples of `every`"""
    off = (-first_owned) % every
    return off, list(range(first_owned + off, first_owned + nblk, every))


class _Sink:
    def write(self, data):
        return len(data)


def find_files(engine, fins, elements, cells, block=arrayfilter.BLOCK, window=arrayfilter.WINDOW, load_shift=arrayfilter.LOAD_SHIFT, peaks=PEAKS,
               sep_deg=SEP, every=1, fout=None, ftrace=None, piece_bytes=rawfile.PIECE_BYTES):
    """Read the open binary files in lockstep through nulling's pump; (absolute blocks, records [B][K], floor [B]) of the evaluated
    blocks, the trace lines to ftrace (binary) and with fout the nulled recording at nulling's automatic gain"""
    blocks, recs, floors = [], [], []
    with Finder(engine, elements, cells, load_shift, peaks, sep_deg) as fd:
        def on_cov(first_owned, cov):
            off, bs = evaluated(first_owned, cov.shape[0], every)
            if not bs:
                return
            pk, fl = fd.run(cov[off:], every)
            rec, fl = records(pk), fl.cpu().numpy()
            if ftrace is not None:
                for b, triples in zip(bs, report(fd.cells, rec, fl)):
                    ftrace.write((trace_line(b, block, triples) + "\n").encode())
            blocks.extend(bs)
            recs.append(rec)
            floors.append(fl)

        arrayfilter.convert_files(nulling.TOOL, engine, fins, _Sink() if fout is None else fout, (block, window, load_shift, None),
                                  1.0 if fout is None else None, piece_bytes=piece_bytes, on_cov=on_cov)
    K = int(peaks)
    return blocks, np.concatenate(recs) if recs else np.zeros((0, K), dtype=PEAK), np.concatenate(floors) if floors else np.zeros(0)


def _element(text):
    try:
        p = [float(v) for v in text.split(",")]
    except ValueError:
        p = []
    if len(p) != 3:
        raise argparse.ArgumentTypeError("an element is E,N,U in wavelengths, not %r" % (text,))
    return p


def build_parser():
    ap = argparse.ArgumentParser(prog="bearing", description="Find interferer bearings from antenna-array recordings: Capon scan on the GPU")
    ap.add_argument("--element", type=_element, action="append", default=[], metavar="E,N,U", help="one per input file: east,north,up in wavelengths")
    ap.add_argument("--step", type=float, default=STEP, help="grid step in degrees (default %(default)s)")
    ap.add_argument("--el-min", type=float, default=0.0, help="lowest elevation of the grid in degrees (default %(default)s)")
    ap.add_argument("--peaks", type=int, default=PEAKS, help="peaks per block, 1..%d (default %%(default)s)" % MAX_PEAKS)
    ap.add_argument("--sep", type=float, default=SEP, help="cells closer than this to a peak leave the later ranks, degrees (default %(default)s)")
    ap.add_argument("--every", type=int, default=1, help="evaluate the blocks whose absolute index is a multiple of this (default %(default)s)")
    ap.add_argument("--block", type=int, default=arrayfilter.BLOCK, help="samples per covariance block, a multiple of 64 in 64..%d (default %%(default)s)" % arrayfilter.MAX_BLOCK)
    ap.add_argument("--window", type=int, default=arrayfilter.WINDOW, help="blocks the covariance sums over, 1..%d (default %%(default)s)" % arrayfilter.MAX_WINDOW)
    ap.add_argument("--load-shift", type=int, default=arrayfilter.LOAD_SHIFT, help="diagonal loading (trace >> S) + 1, S in 0..%d (default %%(default)s)" % arrayfilter.MAX_SHIFT)
    ap.add_argument("--out", default=None, help="file for the nulled recording of the same pass")
    ap.add_argument("--trace", default=None, metavar="FILE", help="file for one line per evaluated block")
    ap.add_argument("--device", type=int, default=0, help="GPU index")
    ap.add_argument("inputs", nargs="+", metavar="IN", help="one int8 I/Q recording per antenna element")
    return ap


def parse(argv):
    """the argparse namespace of a command line, checked; .cells is the grid"""
    argv = list(argv)
    # --element values may begin with '-': hand them over in the form argparse never takes for an option
    for i in range(len(argv) - 1):
        if argv[i] == "--element":
            argv[i:i + 2] = ["--element=" + argv[i + 1], None]
    a = build_parser().parse_args([v for v in argv if v is not None])
    M = len(a.inputs)
    if not 2 <= M <= arrayfilter.MAX_ANTENNAS or len(a.element) != M:
        raise SystemExit("bearing: need 2..%d input files and one --element per file (%d files, %d elements)" % (arrayfilter.MAX_ANTENNAS, M, len(a.element)))
    if a.block < 64 or a.block > arrayfilter.MAX_BLOCK or a.block % 64 or not 1 <= a.window <= arrayfilter.MAX_WINDOW or not 0 <= a.load_shift <= arrayfilter.MAX_SHIFT:
        raise SystemExit("bearing: --block is a multiple of 64 in 64..%d, --window lies in 1..%d and --load-shift in 0..%d"
                         % (arrayfilter.MAX_BLOCK, arrayfilter.MAX_WINDOW, arrayfilter.MAX_SHIFT))
    if not 1 <= a.peaks <= MAX_PEAKS or a.every < 1 or not 0.0 <= a.sep <= 180.0:
        raise SystemExit("bearing: --peaks lies in 1..%d, --every is at least 1 and --sep lies in 0..180" % MAX_PEAKS)
    try:
        a.cells = grid(a.step, a.el_min)
    except ValueError as e:
        raise SystemExit("bearing: %s" % e)
    if not 1 <= len(a.cells) <= MAX_CELLS:
        raise SystemExit("bearing: the grid has %d cells, at most %d fit" % (len(a.cells), MAX_CELLS))
    if a.out == "-":
        raise SystemExit("bearing: --out is a file")
    return a


def run(argv, out=None, piece_bytes=rawfile.PIECE_BYTES):
    a = parse(argv)
    with streaming.shell(a.device, a.inputs, [a.out] if a.out else [], a.trace, out, stdin=False) as sh:
        blocks, rec, _ = find_files(sh.engine, sh.fins, a.element, a.cells, a.block, a.window, a.load_shift, a.peaks, a.sep, a.every,
                                    sh.fouts[0] if a.out else None, sh.ftrace, piece_bytes)
    line = summary_line(len(a.inputs), a.block, a.window, a.cells, rec)
    print(line, file=sh.report)
    return line


def main(argv=None):
    return streaming.main(argv, __doc__, run)


if __name__ == "__main__":
    sys.exit(main())
