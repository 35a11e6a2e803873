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
import optparse
import sys

import numpy as np

from . import _native as nat
from . import acquire
from . import codes
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
    t = CHIP_TRACKERS[ch.name]
    wide, narrow = float(ch.loop_dwells[0]), float(ch.loop_dwells[1])
    phase = 0.0
    if ch.carrier_phase is not None:
        wide, narrow = 0.0, 0.0                  # loop_dwells = 0,0
        phase = float(ch.carrier_phase)
    return TrackSpec(code=t.code.encode(), prn=int(ch.prn), kind=t.kind, subs=t.subs, fixed_pll=0, glonass=0, pad=0, fs=float(ch.fs),
                     period=t.period, rate=t.rate, ratio=t.ratio, spacing=t.spacing, chip_rate=float(codes.chip_rate(t.code)),
                     fll_k_wide=t.fll[0], fll_k_narrow=t.fll[1], pll_k1=float(t.pll[0]), pll_k2=float(t.pll[1]),
                     dll_k1=float(t.dll[0]), dll_k2=float(t.dll[1]), coffset=float(ch.coffset), fm=0.0,
                     code_offset=float(ch.code_offset), doppler=float(ch.doppler), carrier_phase=phase, dwell_wide=wide,
                     dwell_narrow=narrow)


class ChipTrackLoop(trackloop.TrackLoop):
    """K B2b channels tracked on the device with TrackLoop's interface and guarantees (``run``, ``feed``, ``state``, ``close``), plus
    ``chips(k)``: channel k's accumulator, complex128[L].  ``accum_after``: one frame threshold per channel (or one for all); frame
    ``f`` is accumulated when ``f > accum_after``, as the scripts' ``nframe > 200``."""

    def __init__(self, channels, engine=None, max_records=100, accum_after=ACCUM_AFTER):
        channels = list(channels)
        self.accum_after = np.broadcast_to(np.asarray(accum_after, dtype=np.int64), (len(channels),)).copy()
        self.L = [codes.code_length(CHIP_TRACKERS[c.name].code) if c.name in CHIP_TRACKERS else 0 for c in channels]
        super().__init__(channels, engine, max_records)

    @staticmethod
    def _trackers():
        return CHIP_TRACKERS

    @staticmethod
    def _channel_spec(ch):
        return chip_channel_spec(ch)

    def _open(self):
        h = ctypes.c_void_p()
        nat.check(nat.lib.gacq_chiptrack_open(self.eng._ctx, self._specs, self.K, self.accum_after.ctypes.data_as(ctypes.c_void_p),
                                              ctypes.byref(h)), self.eng._ctx)
        return h

    def close(self):
        if self._h:
            nat.lib.gacq_chiptrack_close(self._h)
            self._h = None

    def state(self, k):
        out = np.zeros(1, dtype=STATE_DTYPE)
        nat.check(nat.lib.gacq_chiptrack_state(self._h, k, out.ctypes.data_as(ctypes.c_void_p)), self.eng._ctx)
        return out[0]

    def chips(self, k):
        """Channel k's chip accumulator: complex128[L], the script's s.chips."""
        out = np.zeros(2 * self.L[k], dtype=np.float64)
        nat.check(nat.lib.gacq_chiptrack_chips(self._h, k, out.ctypes.data_as(ctypes.c_void_p)), self.eng._ctx)
        return out.view(np.complex128)

    def _run_dev(self, ptrs, base, avail, recs, cap, counts, status):
        return nat.lib.gacq_chiptrack_run_dev(self._h, ptrs, base, avail, self.max_records, recs, cap, counts, status)


def format_chips(chips):
    """track-chips.dat's lines ('%f %f' of each bin's real and imaginary part)."""
    return ['%f %f' % (np.real(c), np.imag(c)) for c in chips]


def format_lines(name, recs):
    """The script's output lines ('%d %f %f %f %f %f %f %f %f')."""
    cr = float(codes.chip_rate(CHIP_TRACKERS[name].code))
    out = []
    for r in recs:
        p = complex(float(r["p_re"]), float(r["p_im"]))
        v = (int(r["block"]), np.real(p), np.imag(p), float(r["carrier_f"]), float(r["code_f"]) - cr, (180 / np.pi) * np.angle(p),
             float(r["early"]), float(r["prompt"]), float(r["late"]))
        out.append('%d %f %f %f %f %f %f %f %f' % v)
    return out


def track_file(name, path, fs, coffset, prn, doppler, code_offset, loop_dwells=(500.0, 500.0), carrier_phase=None, engine=None,
               accum_after=ACCUM_AFTER):
    """One script run on one file: returns (records, output lines, chips)."""
    ch = Channel(name, fs, coffset, prn, doppler, code_offset, tuple(loop_dwells), carrier_phase)
    eng = engine or acquire.default_engine()
    tl = ChipTrackLoop([ch], eng, accum_after=accum_after)
    try:
        recs = tl.run([trackloop.load_int8(path, eng.device)])[0]
        chips = tl.chips(0)
    finally:
        tl.close()
    return recs, format_lines(name, recs), chips


def build_parser(name):
    p = optparse.OptionParser(usage="%s [options] input_filename sample_rate carrier_offset PRN doppler code_offset" % name)
    p.disable_interspersed_args()
    p.add_option("--loop-dwells", default="500,500", help="initial time intervals for wide FLL, then narrow FLL, in milliseconds "
                                                          "(default %default)")
    p.add_option("--carrier-phase", help="initial carrier phase in cycles (disables FLL: uses PLL from the start)")
    return p


def parse(name, argv):
    """(path, Channel) of one command line (argv after the tracker name), with the script's own argument conversions."""
    if name not in CHIP_TRACKERS:
        raise SystemExit("unknown chip tracker %r; the chip trackers: %s" % (name, " ".join(sorted(CHIP_TRACKERS))))
    options, args = build_parser(name).parse_args(list(argv))
    if len(args) < 6:
        raise SystemExit("%s: need input_filename sample_rate carrier_offset PRN doppler code_offset" % name)
    dwells = tuple(map(float, options.loop_dwells.split(",")))        # util.parse_list_floats
    phase = float(options.carrier_phase) if options.carrier_phase is not None else None
    ch = Channel(name, float(args[1]), float(args[2]), int(args[3]), float(args[4]), float(args[5]), dwells, phase)
    return args[0], ch


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
