"""C/N0 estimates from a tracker's prompt correlator, the job of the reference's cn0.py.

The input is a track sampled at 1 kHz: text lines whose second and third columns are prompt I and Q (what
`python -m gnss_dsp_tools_amd.track` prints), or a trackloop.RECORD_DTYPE array.  Each whole block of `time` values gives one
estimate: the mean of |I| over sqrt(2) times the population standard deviation of Q, as 20 log10 plus 30 dB for the 1 kHz rate.
A trailing partial block gives nothing.

Host numpy on purpose: 1000 values per second and channel, already in host memory.

    python -m gnss_dsp_tools_amd.cn0 [--time MS] < track.dat
"""
import optparse
import sys

import numpy as np

DEFAULT_TIME_MS = 300


def block_estimates(i, q, time_ms=DEFAULT_TIME_MS):
    """one dB-Hz value per whole block of time_ms entries of the prompt I and Q arrays"""
    time_ms = int(time_ms)
    if time_ms < 1:
        raise ValueError("time must be at least 1 ms")
    i = np.asarray(i, dtype=np.float64)
    q = np.asarray(q, dtype=np.float64)
    nblocks = min(len(i), len(q)) // time_ms
    i = i[:nblocks * time_ms].reshape(nblocks, time_ms)
    q = q[:nblocks * time_ms].reshape(nblocks, time_ms)
    if nblocks == 0:
        return np.zeros(0, dtype=np.float64)
    signal = np.abs(i).mean(axis=1)
    noise = np.sqrt(2) * q.std(axis=1)             # ddof = 0
    return 20 * np.log10(signal / noise) + 30


def cn0(x):
    """the estimate of one block of complex prompt values"""
    x = np.asarray(x)
    return float(block_estimates(x.real, x.imag, len(x))[0])


def from_records(recs, time_ms=DEFAULT_TIME_MS):
    """estimates from a record array with p_re and p_im fields: one channel of a TrackLoop.run result goes straight in"""
    recs = np.asarray(recs)
    return block_estimates(recs["p_re"], recs["p_im"], time_ms)


def from_lines(lines, time_ms=DEFAULT_TIME_MS):
    """estimates from a track's text lines (blank lines ignored)"""
    cols = [ln.split() for ln in lines]
    cols = [c for c in cols if c]
    return block_estimates([float(c[1]) for c in cols], [float(c[2]) for c in cols], time_ms)


def format_lines(values):
    return ["%.2f" % v for v in values]


def parse(argv):
    """--time MS only; option parsing stops at the first positional argument"""
    parser = optparse.OptionParser(usage="python -m gnss_dsp_tools_amd.cn0 [--time MS] < track.dat",
                                   description="Print one C/N0 estimate (dB-Hz, two decimals) per block of a 1 kHz track read from standard input.")
    parser.disable_interspersed_args()
    parser.add_option("--time", default=str(DEFAULT_TIME_MS), metavar="MS", help="block length in milliseconds, %default unless given")
    options, _ = parser.parse_args(list(argv))
    return int(options.time)


def run(argv, inp=None, out=None):
    time_ms = parse(argv)
    lines = format_lines(from_lines((inp or sys.stdin).read().splitlines(), time_ms))
    for ln in lines:
        print(ln, file=out or sys.stdout)
    return lines


if __name__ == "__main__":
    run(sys.argv[1:])
