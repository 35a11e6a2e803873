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
import sys

from . import _native as nat
from . import arrayfilter, rawfile, streaming
# what both array tools share, part of this module as before
from .arrayfilter import AUTO_SAMPLES, BLOCK, LOAD_SHIFT, MAX_ANTENNAS, MAX_BLOCK, MAX_SHIFT, MAX_WINDOW, TARGET_RMS, WINDOW, WQ, _complex, lockstep
from .streaming import owned_blocks

MAX_TAPS, MAX_WEIGHTS = 15, 56
TAPS = 5


StapCfg = nat.struct("gacq_stap_cfg")


def make_cfg(M, taps=TAPS, block=BLOCK, window=WINDOW, load_shift=LOAD_SHIFT, constraint=None):
    return StapCfg(antennas=int(M), taps=int(taps), block=int(block), window=int(window), load_shift=int(load_shift),
                   c=arrayfilter.constraint_c(int(M), constraint))


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


def auto_window(block, window, taps):
    """input samples that hold the automatic gain's window"""
    return max(AUTO_SAMPLES, int(block) * int(window)) + centre(taps)


class Stap(arrayfilter.Handle):
    """The open device side of one configuration (gacq_stap_open): arrayfilter.Handle with N = M T weights per block"""
    _opener, _runner, _close, _what = "gacq_stap_open", "gacq_stap_run_dev", "gacq_stap_close", "space-time nuller"

    def __init__(self, engine, M, taps=TAPS, block=BLOCK, window=WINDOW, load_shift=LOAD_SHIFT, constraint=None):
        self.taps = int(taps)
        self.N = int(M) * self.taps
        self._start(engine, make_cfg(M, taps, block, window, load_shift, constraint), self.N)


# opts, in Stap's order: (taps, block, window, load_shift, constraint)
TOOL = arrayfilter.Tool("stap", Stap, window=lambda o: o[2], out_end=lambda o, in_end: out_end(o[1], o[2], in_end, o[0]),
                        first_needed=lambda o, out: first_needed(o[1], o[2], out, o[0]), auto_window=lambda o: auto_window(o[1], o[2], o[0]))


def convert(engine, xs, taps=TAPS, block=BLOCK, window=WINDOW, load_shift=LOAD_SHIFT, constraint=None, gain=1.0, dtype="int8", weights=False):
    """arrayfilter.convert: (output tensor, (clipped, blocks)) and with weights the int32 weights as a third"""
    return arrayfilter.convert(TOOL, engine, xs, (taps, block, window, load_shift, constraint), gain, dtype, weights)


def auto_gain(engine, firsts, taps=TAPS, block=BLOCK, window=WINDOW, load_shift=LOAD_SHIFT, constraint=None, target_rms=TARGET_RMS):
    return arrayfilter.auto_gain(TOOL, engine, firsts, (taps, block, window, load_shift, constraint), target_rms)


class Stream(arrayfilter.Stream):
    """arrayfilter.Stream of a Stap: the tail kept on the device starts t_c samples before the first block the next output's window needs"""

    def __init__(self, engine, M, gain, taps=TAPS, block=BLOCK, window=WINDOW, load_shift=LOAD_SHIFT, constraint=None, dtype="int8", weights=False):
        super().__init__(TOOL, engine, M, gain, (taps, block, window, load_shift, constraint), dtype, weights)


def convert_files(engine, fins, fout, taps=TAPS, block=BLOCK, window=WINDOW, load_shift=LOAD_SHIFT, constraint=None, gain=None, target_rms=TARGET_RMS,
                  dtype="int8", ftrace=None, piece_bytes=rawfile.PIECE_BYTES):
    """arrayfilter.convert_files: (gain, samples written, clipped components)"""
    return arrayfilter.convert_files(TOOL, engine, fins, fout, (taps, block, window, load_shift, constraint), gain, target_rms, dtype, ftrace, piece_bytes)


def build_parser():
    ap = argparse.ArgumentParser(prog="stap", description="Space-time adaptive nulling: M antennas x T taps over int8 I/Q recordings on the GPU")
    ap.add_argument("--taps", type=int, default=TAPS, help="taps per antenna, odd, 1..%d, antennas x taps <= %d (default %%(default)s)" % (MAX_TAPS, MAX_WEIGHTS))
    return arrayfilter.add_options(ap, weights="M T", centre=" on the centre taps", stdin="; - is stdin")


def _check_taps(a, M):
    if not 1 <= a.taps <= MAX_TAPS or a.taps % 2 == 0 or M * a.taps > MAX_WEIGHTS:
        raise SystemExit("stap: --taps is odd in 1..%d and antennas x taps at most %d" % (MAX_TAPS, MAX_WEIGHTS))
    if a.inputs.count("-") > 1:
        raise SystemExit("stap: only one input can be stdin")


def parse(argv):
    """the argparse namespace of a command line, checked"""
    return arrayfilter.parse("stap", build_parser(), argv, 1, _check_taps)


def report_line(M, taps, block, window, gain, clipped, samples):
    return "antennas %d taps %d block %d window %d gain %r clipped %d samples %d" % (M, taps, block, window, float(gain), int(clipped), int(samples))


def run(argv, out=None, piece_bytes=rawfile.PIECE_BYTES):
    a = parse(argv)
    return arrayfilter.run(TOOL, a, (a.taps, a.block, a.window, a.load_shift, a.constraint),
                           lambda gain, clipped, n: report_line(len(a.inputs), a.taps, a.block, a.window, gain, clipped, n), out, piece_bytes)


def main(argv=None):
    return streaming.main(argv, __doc__, run)


if __name__ == "__main__":
    sys.exit(main())
