"""Device-resident tracking loops with the on-device chip accumulator: track-beidou-b2bi.py and track-beidou-b2bq.py on the GPU.

Their main loop and ``track()`` are the template's (trackloop.py; ratio 118 as E5b, 10230-chip codes at 10.23 Mcps).  On top of the
loop, from frame ``accum_after + 1`` on (the scripts: ``if s.nframe > 200``), every block after both wipe-offs is folded into a
10230-bin complex128 chip accumulator, ``nco.accum(+-x, code_p, cf, chips, L)`` with the sign of real(p_prompt), and the script
writes the bins to ``track-chips.dat`` at exit -- the spreading code read off a live recording.  ``ChipTrackLoop`` runs K such
channels in one launch (csrc/gacq_chiptrack.hip, one workgroup per channel); loop state and accumulator stay on the device between
launches, so a recording fed in chunks gives the same records and bins, bit for bit, as one ``run()``.  Each bin is the reference's
sequential fp64 sum in sample order.

    python -m gnss_dsp_tools_amd.chiptrack <name> [--loop-dwells A,B] [--carrier-phase P] FILE FS COFFSET PRN DOPPLER CODE_OFFSET

prints the script's lines and writes ./track-chips.dat, as the scripts do.
"""
import ctypes
import sys

import numpy as np

from . import _native as nat
from . import codes
from . import track
from . import trackloop
from .trackloop import RECORD_DTYPE, STATE_DTYPE, Channel, Tracker, TrackSpec  # noqa: F401  (re-exported)

CHIP_TRACKERS = {
    "beidou-b2bi": Tracker("beidou.b2bi", 0, 0.5, 118.0, 0.001, 1000.0, 1),
    "beidou-b2bq": Tracker("beidou.b2bq", 0, 0.5, 118.0, 0.001, 1000.0, 1),
}

ACCUM_AFTER = 200            # if s.nframe > 200: nco.accum(...)
CHIPS_FILE = "track-chips.dat"


def chip_channel_spec(ch):
    """gacq_track_spec of a B2b channel: trackloop.channel_spec's arithmetic with CHIP_TRACKERS' constants."""
    if ch.name not in CHIP_TRACKERS:
        raise KeyError("unknown chip tracker %r (%s)" % (ch.name, ", ".join(sorted(CHIP_TRACKERS))))
    return trackloop.channel_spec(ch, CHIP_TRACKERS)


class ChipTrackLoop(trackloop.TrackLoop):
    """K B2b channels tracked on the device with TrackLoop's interface and guarantees (``run``, ``feed``, ``state``, ``close``), plus
    ``chips(k)``: channel k's accumulator, complex128[L].  ``accum_after``: one frame threshold per channel (or one for all); frame
    ``f`` is accumulated when ``f > accum_after``, as the scripts' ``nframe > 200``."""

    def __init__(self, channels, engine=None, max_records=100, accum_after=ACCUM_AFTER):
        channels = list(channels)
        self.accum_after = np.broadcast_to(np.asarray(accum_after, dtype=np.int64), (len(channels),)).copy()
        self.L = [codes.code_length(CHIP_TRACKERS[c.name].code) if c.name in CHIP_TRACKERS else 0 for c in channels]
        super().__init__(channels, engine, max_records)

    _lib = "gacq_chiptrack"

    @staticmethod
    def _trackers():
        return CHIP_TRACKERS

    @staticmethod
    def _channel_spec(ch):
        return chip_channel_spec(ch)

    def _open(self):
        h = ctypes.c_void_p()
        nat.check(self._call("open", self.eng._ctx, self._specs, self.K, self.accum_after.ctypes.data_as(ctypes.c_void_p), ctypes.byref(h)),
                  self.eng._ctx)
        return h

    def chips(self, k):
        """Channel k's chip accumulator: complex128[L], the script's s.chips."""
        out = np.zeros(2 * self.L[k], dtype=np.float64)
        nat.check(self._call("chips", self._h, k, out.ctypes.data_as(ctypes.c_void_p)), self.eng._ctx)
        return out.view(np.complex128)


def format_chips(chips):
    """track-chips.dat's lines ('%f %f' of each bin's real and imaginary part)."""
    return ['%f %f' % (np.real(c), np.imag(c)) for c in chips]


def format_lines(name, recs):
    """The script's output lines ('%d %f %f %f %f %f %f %f %f')."""
    return trackloop.format_lines(name, recs, trackers=CHIP_TRACKERS)


def track_file(*args, accum_after=ACCUM_AFTER, **kw):
    """One script run on one file, trackloop.track_file's arguments: returns (records, output lines, chips)."""
    return trackloop.track_file(*args, loop=ChipTrackLoop, accum_after=accum_after, **kw)


def build_parser(name):
    return track.build_parser(name, CHIP_TRACKERS)


def parse(name, argv):
    """(path, Channel) of one command line (argv after the tracker name), with the script's own argument conversions."""
    return track.parse(name, argv, CHIP_TRACKERS, "chip tracker")


def run(name, argv, out=sys.stdout, chips_path=CHIPS_FILE):
    """The script: print its lines to `out`, write the bins to `chips_path` (relative to the working directory).  Returns
    (lines, chips)."""
    path, ch = parse(name, argv)
    _, lines, chips = track_file(name, path, ch.fs, ch.coffset, ch.prn, ch.doppler, ch.code_offset, ch.loop_dwells, ch.carrier_phase)
    for line in lines:
        out.write(line + "\n")
    with open(chips_path, "w") as f:
        for line in format_chips(chips):
            f.write(line + "\n")
    return lines, chips


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    if not argv or argv[0] in ("-h", "--help"):
        sys.stdout.write(__doc__ + "\nchip trackers: " + " ".join(sorted(CHIP_TRACKERS)) + "\n")
        return 0
    run(argv[0], argv[1:])
    return 0


if __name__ == "__main__":
    sys.exit(main())
