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
import sys

from . import _native as nat
from . import arrayfilter, rawfile, streaming
# what both array tools share and the block / window algebra, part of this module as before
from .arrayfilter import AUTO_SAMPLES, BLOCK, LOAD_SHIFT, MAX_ANTENNAS, MAX_BLOCK, MAX_SHIFT, MAX_WINDOW, TARGET_RMS, WINDOW, WQ, _complex, lockstep
from .streaming import first_needed, out_end, owned_blocks


NullCfg = nat.struct("gacq_null_cfg")


def make_cfg(M, block=BLOCK, window=WINDOW, load_shift=LOAD_SHIFT, constraint=None):
    return NullCfg(antennas=int(M), block=int(block), window=int(window), load_shift=int(load_shift), c=arrayfilter.constraint_c(int(M), constraint))


class Nuller(arrayfilter.Handle):
    """The open device side of one configuration (gacq_null_open): arrayfilter.Handle with M weights per block"""
    _opener, _runner, _close, _what = "gacq_null_open", "gacq_null_run_dev", "gacq_null_close", "nuller"

    def __init__(self, engine, M, block=BLOCK, window=WINDOW, load_shift=LOAD_SHIFT, constraint=None):
        self._start(engine, make_cfg(M, block, window, load_shift, constraint), M)


def auto_window(block, window):
    """input samples that hold the automatic gain's window"""
    return max(AUTO_SAMPLES, int(block) * int(window))


# opts, in Nuller's order: (block, window, load_shift, constraint)
TOOL = arrayfilter.Tool("nulling", Nuller, window=lambda o: o[1], out_end=lambda o, in_end: out_end(o[0], o[1], in_end),
                        first_needed=lambda o, out: first_needed(o[0], o[1], out), auto_window=lambda o: auto_window(o[0], o[1]))


def convert(engine, xs, block=BLOCK, window=WINDOW, load_shift=LOAD_SHIFT, constraint=None, gain=1.0, dtype="int8", weights=False):
    """arrayfilter.convert: (output tensor, (clipped, blocks)) and with weights the int32 weights as a third"""
    return arrayfilter.convert(TOOL, engine, xs, (block, window, load_shift, constraint), gain, dtype, weights)


def auto_gain(engine, firsts, block=BLOCK, window=WINDOW, load_shift=LOAD_SHIFT, constraint=None, target_rms=TARGET_RMS):
    return arrayfilter.auto_gain(TOOL, engine, firsts, (block, window, load_shift, constraint), target_rms)


class Stream(arrayfilter.Stream):
    """arrayfilter.Stream of a Nuller: the W blocks under the next output's weights stay on the device"""

    def __init__(self, engine, M, gain, block=BLOCK, window=WINDOW, load_shift=LOAD_SHIFT, constraint=None, dtype="int8", weights=False):
        super().__init__(TOOL, engine, M, gain, (block, window, load_shift, constraint), dtype, weights)


def convert_files(engine, fins, fout, block=BLOCK, window=WINDOW, load_shift=LOAD_SHIFT, constraint=None, gain=None, target_rms=TARGET_RMS,
                  dtype="int8", ftrace=None, piece_bytes=rawfile.PIECE_BYTES):
    """arrayfilter.convert_files: (gain, samples written, clipped components)"""
    return arrayfilter.convert_files(TOOL, engine, fins, fout, (block, window, load_shift, constraint), gain, target_rms, dtype, ftrace, piece_bytes)


def build_parser():
    ap = argparse.ArgumentParser(prog="nulling", description="Null interference with an antenna array: adaptive weights over int8 I/Q recordings on the GPU")
    return arrayfilter.add_options(ap)


def parse(argv):
    """the argparse namespace of a command line, checked"""
    return arrayfilter.parse("nulling", build_parser(), argv, 2)


def report_line(M, block, window, gain, clipped, samples):
    return "antennas %d block %d window %d gain %r clipped %d samples %d" % (M, block, window, float(gain), int(clipped), int(samples))


def run(argv, out=None, piece_bytes=rawfile.PIECE_BYTES):
    a = parse(argv)
    return arrayfilter.run(TOOL, a, (a.block, a.window, a.load_shift, a.constraint),
                           lambda gain, clipped, n: report_line(len(a.inputs), a.block, a.window, gain, clipped, n), out, piece_bytes, stdin=False)


def main(argv=None):
    return streaming.main(argv, __doc__, run)


if __name__ == "__main__":
    sys.exit(main())
