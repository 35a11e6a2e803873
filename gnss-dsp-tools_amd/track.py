"""Command-line drop-in for the track-*.py scripts on the GPU: the template family (trackloop) and the long-code scripts
gps-l2cl, glonass-l1-p and glonass-l2-p (longtrack); beidou-b2bi and beidou-b2bq, which also write track-chips.dat, are handed to
python -m gnss_dsp_tools_amd.chiptrack:

    python -m gnss_dsp_tools_amd.track <name> [--loop-dwells A,B] [--carrier-phase P] FILE FS COFFSET PRN|CHAN DOPPLER CODE_OFFSET

The options are parsed by optparse with interspersed arguments disabled, exactly as the scripts do (track-gps-l1.py:99-136), so
negative positional values (carrier offset, GLONASS channel, Doppler) and a negative --carrier-phase value behave the same.
Output: the script's lines ('%d %f ...', 9 or 14 columns), one per track() call, up to the first outer block the file cannot fill."""
import optparse
import sys

from . import longtrack, trackloop

TRACKERS = {**trackloop.TRACKERS, **longtrack.LONG_TRACKERS}


def names():
    """Every tracker name the command line accepts."""
    return sorted(TRACKERS)


def _usage(name, trackers):
    return "input_filename sample_rate carrier_offset %s doppler code_offset" % ("chan" if trackers[name].glonass else "PRN")


def build_parser(name, trackers=TRACKERS):
    p = optparse.OptionParser(usage="%s [options] %s" % (name, _usage(name, trackers)))
    p.disable_interspersed_args()
    p.add_option("--loop-dwells", default="500,500", help="initial time intervals for wide FLL, then narrow FLL, in milliseconds "
                                                          "(default %default)")
    p.add_option("--carrier-phase", help="initial carrier phase in cycles (disables FLL: uses PLL from the start)")
    return p


def parse(name, argv, trackers=TRACKERS, what="tracker"):
    """(path, Channel) of one command line (argv after the tracker name), with the script's own argument conversions."""
    if name not in trackers:
        raise SystemExit("unknown %s %r; the %ss: %s" % (what, name, what, " ".join(sorted(trackers))))
    options, args = build_parser(name, trackers).parse_args(list(argv))
    if len(args) < 6:
        raise SystemExit("%s: need %s" % (name, _usage(name, trackers)))
    dwells = tuple(map(float, options.loop_dwells.split(",")))        # util.parse_list_floats
    phase = float(options.carrier_phase) if options.carrier_phase is not None else None
    ch = trackloop.Channel(name, float(args[1]), float(args[2]), int(args[3]), float(args[4]), float(args[5]), dwells, phase)
    return args[0], ch


def run(name, argv, out=sys.stdout):
    path, ch = parse(name, argv)
    mod = longtrack if name in longtrack.LONG_TRACKERS else trackloop
    _, lines = mod.track_file(name, path, ch.fs, ch.coffset, ch.prn, ch.doppler, ch.code_offset, ch.loop_dwells, ch.carrier_phase)
    for line in lines:
        out.write(line + "\n")
    return lines


def main(argv=None):
    from . import chiptrack            # it imports this module for the parser
    argv = sys.argv[1:] if argv is None else argv
    if not argv or argv[0] in ("-h", "--help"):
        sys.stdout.write(__doc__ + "\ntrackers: " + " ".join(names() + sorted(chiptrack.CHIP_TRACKERS)) + "\n")
        return 0
    if argv[0] in chiptrack.CHIP_TRACKERS:
        return chiptrack.main(argv)
    run(argv[0], argv[1:])
    return 0


if __name__ == "__main__":
    sys.exit(main())
