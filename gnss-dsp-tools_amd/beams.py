"""Per-satellite beams from an antenna array on the GPU (csrc/gacq_beams.hip, gacq_beams_*): M int8 I/Q recordings sampled on one clock
in, K recordings out in one pass.  Output k is what nulling writes under ``--constraint`` c_k -- the block-wise minimum-power (MVDR)
weights that keep gain 1 toward the steering vector c_k and null the interference -- bit for bit; the block covariance, the window and
the loading, which do not depend on the constraint, are formed once for all K, and the recordings are read once.

    python -m gnss_dsp_tools_amd.beams [--block N] [--window W] [--load-shift S] [--gain G | --target-rms R] [--complex64]
           [--weights-trace FILE] --antenna IN0 --antenna IN1 [...] --beam OUT RE,IM RE,IM ... [--beam OUT ...]

reads the M files (or FIFOs) piece by piece in lockstep and writes one file per --beam (1..16 of them).  The entries of a beam, one per
antenna, are what ``python -m gnss_dsp_tools_amd.arrayprompt`` prints after ``steering``.  It prints

    antennas <M> beams <K> block <Lb> window <W> samples <N>
    beam <k> gain <G> clipped <C>            (one line per beam)

--block, --window and --load-shift are nulling's.  Without --gain every beam gets a gain of its own: --target-rms (default 32) over the
rms of its first 65536 output samples at gain 1.  --weights-trace writes the quantised weights of every block, K x M int32 pairs each
(weight = value / 16384).  Files of unequal length end at the shortest; a recording shorter than W blocks gives no output.  The
definition is in include/gacq.h; beam k is tests/nulling_oracle.py under c_k."""
import argparse
import re
import sys

import numpy as np

from . import _native as nat
from . import arrayfilter, rawfile, streaming
from .arrayfilter import BLOCK, LOAD_SHIFT, MAX_ANTENNAS, TARGET_RMS, WINDOW, _complex
from .nulling import auto_window
from .streaming import first_needed, out_end

MAX_BEAMS = 16


BeamsCfg = nat.struct("gacq_beams_cfg")


def make_cfg(M, constraints, block=BLOCK, window=WINDOW, load_shift=LOAD_SHIFT):
    """constraints: K rows of M complex entries; a row that is None is the default (1, 0, .., 0)"""
    rows = list(constraints)
    if not 1 <= len(rows) <= MAX_BEAMS:
        raise ValueError("need 1..%d beams, got %d" % (MAX_BEAMS, len(rows)))
    cfg = BeamsCfg(antennas=int(M), beams=len(rows), block=int(block), window=int(window), load_shift=int(load_shift))
    for k, row in enumerate(rows):
        cfg.c[k] = arrayfilter.constraint_c(int(M), row)
    return cfg


class Beamformer(arrayfilter.Handle):
    """The open device side of one configuration (gacq_beams_open): arrayfilter.Handle with K outputs.  run() takes K gains and returns
    a list of K tensors (with weights the int32 weights [owned blocks][K][M][2]); stats() returns (clipped[K], blocks)."""
    _opener, _runner, _close, _what = "gacq_beams_open", "gacq_beams_run_dev", "gacq_beams_close", "beamformer"

    def __init__(self, engine, M, constraints, block=BLOCK, window=WINDOW, load_shift=LOAD_SHIFT):
        cfg = make_cfg(M, constraints, block, window, load_shift)
        self.K = cfg.beams
        self._start(engine, cfg, M, outputs=cfg.beams)

    def run(self, d_inputs, in_first, out_first, n_out, gains, dtype="int8", weights=False, cov=False):
        return super().run(d_inputs, in_first, out_first, n_out, gains, dtype, weights, cov)


# opts, in Beamformer's order: (constraints, block, window, load_shift)
TOOL = arrayfilter.Tool("beams", Beamformer, window=lambda o: o[2], out_end=lambda o, in_end: out_end(o[1], o[2], in_end),
                        first_needed=lambda o, out: first_needed(o[1], o[2], out), auto_window=lambda o: auto_window(o[1], o[2]))


def _gains(constraints, gains):
    K = len(list(constraints))
    return [float(gains)] * K if np.isscalar(gains) else [float(g) for g in gains]


def convert(engine, xs, constraints, block=BLOCK, window=WINDOW, load_shift=LOAD_SHIFT, gains=1.0, dtype="int8", weights=False):
    """Whole recordings: (list of K output tensors, (clipped[K], blocks)) and with weights the int32 weights as a third.  gains: one
    per beam, or one number for all."""
    return arrayfilter.convert(TOOL, engine, xs, (constraints, block, window, load_shift), _gains(constraints, gains), dtype, weights)


def auto_gains(engine, firsts, constraints, block=BLOCK, window=WINDOW, load_shift=LOAD_SHIFT, target_rms=TARGET_RMS):
    """one gain per beam: target_rms over the rms of the beam's first min(supported, 65536) outputs at gain 1, from one complex64 run"""
    return arrayfilter.auto_gain(TOOL, engine, firsts, (constraints, block, window, load_shift), target_rms)


class Stream(arrayfilter.Stream):
    """arrayfilter.Stream of a Beamformer: feed() returns K tensors per piece, whose concatenations are convert()'s outputs"""

    def __init__(self, engine, M, gains, constraints, block=BLOCK, window=WINDOW, load_shift=LOAD_SHIFT, dtype="int8", weights=False):
        super().__init__(TOOL, engine, M, _gains(constraints, gains), (constraints, block, window, load_shift), dtype, weights)


def convert_files(engine, fins, fouts, constraints, block=BLOCK, window=WINDOW, load_shift=LOAD_SHIFT, gains=None, target_rms=TARGET_RMS,
                  dtype="int8", ftrace=None, piece_bytes=rawfile.PIECE_BYTES):
    """arrayfilter.convert_files with one open file per beam: (gains[K], samples written per file, clipped[K])"""
    fouts = list(fouts)
    if len(fouts) != len(list(constraints)):
        raise ValueError("one output file per beam")
    return arrayfilter.convert_files(TOOL, engine, fins, fouts, (constraints, block, window, load_shift),
                                     None if gains is None else _gains(constraints, gains), target_rms, dtype, ftrace, piece_bytes)


def build_parser():
    ap = argparse.ArgumentParser(prog="beams", description="Per-satellite MVDR beams from an antenna array: K outputs from one pass on the GPU")
    ap.add_argument("--antenna", action="append", default=[], metavar="IN", help="one int8 I/Q recording per antenna, 2..%d of them" % MAX_ANTENNAS)
    ap.add_argument("--beam", action="append", nargs="+", default=[], metavar=("OUT", "RE,IM"),
                    help="an output file and its steering vector, one entry per antenna; 1..%d of them" % MAX_BEAMS)
    return arrayfilter.add_options(ap, weights="K x M", single=False)


def parse(argv):
    """the argparse namespace of a command line, checked; .outputs are the beams' files and .constraints their vectors"""
    # an entry such as -0.5,0.25 is no option: behind a blank argparse takes it as a value, and float() does not mind the blank
    a = build_parser().parse_args([" " + t if re.match(r"-[0-9.]", t) and "," in t else t for t in argv])
    M = len(a.antenna)
    if not 2 <= M <= MAX_ANTENNAS:
        raise SystemExit("beams: need 2..%d --antenna files" % MAX_ANTENNAS)
    if not 1 <= len(a.beam) <= MAX_BEAMS:
        raise SystemExit("beams: need 1..%d --beam outputs" % MAX_BEAMS)
    a.outputs, a.constraints = [], []
    for k, b in enumerate(a.beam):
        try:
            z = np.array([_complex(t) for t in b[1:]], dtype=np.complex128)
        except argparse.ArgumentTypeError as e:
            raise SystemExit("beams: --beam %d: %s" % (k, e))
        if len(z) != M or not np.all(np.isfinite(z.view(np.float64))) or not np.any(z != 0):
            raise SystemExit("beams: --beam %d takes OUT and %d finite entries RE,IM, not all zero" % (k, M))
        a.outputs.append(b[0])
        a.constraints.append(z)
    return arrayfilter.check_options("beams", a, M)


def report_lines(M, block, window, gains, clipped, samples):
    return ["antennas %d beams %d block %d window %d samples %d" % (M, len(gains), block, window, int(samples))] + \
           ["beam %d gain %r clipped %d" % (k, float(g), int(c)) for k, (g, c) in enumerate(zip(gains, clipped))]


def run(argv, out=None, piece_bytes=rawfile.PIECE_BYTES):
    a = parse(argv)
    with streaming.shell(a.device, a.antenna, a.outputs, a.weights_trace, out, stdin=False) as sh:
        gains, n, clipped = convert_files(sh.engine, sh.fins, sh.fouts, a.constraints, a.block, a.window, a.load_shift, a.gain, a.target_rms,
                                          "complex64" if a.complex64 else "int8", sh.ftrace, piece_bytes)
    lines = report_lines(len(a.antenna), a.block, a.window, gains, clipped, n)
    print("\n".join(lines), file=sh.report)
    return lines


def main(argv=None):
    return streaming.main(argv, __doc__, run)


if __name__ == "__main__":
    sys.exit(main())
