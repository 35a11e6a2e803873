"""Acquire-to-track hand-off: from a recording to running tracking channels, with no number typed by hand.

    python -m gnss_dsp_tools_amd.handoff <signal> [--prn|--channel LIST] [--doppler-search MIN,MAX,INCR] [--time MS]
           [--min-metric X] [--min-ratio R] [--blocks M] [--loop-dwells A,B] [--out-dir DIR] [--nav] FILE FS COFFSET

runs the acquisition of ``python -m gnss_dsp_tools_amd.cli <signal>`` (same options, same output lines), refines every kept result on the
raw recording (refine.py), prints one line per handed-off channel

    handoff <tracker> <item> doppler %.3f code_offset %.4f ratio %.2f[ edge]

whose first fields are the arguments one would give ``python -m gnss_dsp_tools_amd.track``, and, with --out-dir, tracks all channels
in one batched TrackLoop run and writes track-<tracker>-<item>.txt per channel: the lines that track command prints for exactly the
values on the handoff line (the channels are built from the printed, rounded values).  With --nav the channels are tracked as well
and, for the trackers of navdata.FORMATS, the navigation frames of what was tracked are printed after the handoff lines, one
``nav ...`` line per frame (navdata.py); without it the output is what it was before the option existed.

Signals without a template tracker are refused: beidou-b2bi/-b2bq belong to chiptrack, and the long-code trackers (gps-l2cl,
glonass-l1-p, glonass-l2-p) need a prior from another signal."""
import argparse
import os
import sys

import numpy as np

from . import _native as nat
from . import acquire, chiptrack, codes, longtrack, navdata, refine as _refine, signals, trackloop

_RENAMED = {"xona-x1": "xona-x1p"}


class HandoffError(ValueError):
    """The signal has no template tracker to hand off to."""


def tracker_name(signal_name):
    """The tracker an acquisition signal hands off to: the same name, except xona-x1 -> xona-x1p."""
    key = signal_name.lower().replace("_", "-")
    name = _RENAMED.get(key, key)
    if name in chiptrack.CHIP_TRACKERS:
        raise HandoffError("%s is tracked by chiptrack (the loop with the chip accumulator), not by the template trackers: no hand-off" % key)
    if name in longtrack.LONG_TRACKERS:
        raise HandoffError("%s is a long-code tracker: it needs a prior from another signal, not an acquisition of its own: no hand-off" % key)
    if name not in trackloop.TRACKERS:
        raise HandoffError("no template tracker for %r (the trackers: %s)" % (signal_name, ", ".join(sorted(trackloop.TRACKERS))))
    return name


def _printed(tracker, r):
    """(doppler, code_offset) as the handoff line prints them: what the channel is built from, so that the line reproduces the run"""
    L = codes.code_length(trackloop.TRACKERS[tracker].code)
    doppler, code = float("%.3f" % r.doppler), float("%.4f" % r.code_offset)
    return doppler, (code - L if code >= L else code)


def format_line(tracker, item, r):
    doppler, code = _printed(tracker, r)
    return "handoff %s %d doppler %.3f code_offset %.4f ratio %.2f%s" % (tracker, item, doppler, code, r.ratio, " edge" if r.edge else "")


def handoff(name, iq_int8, fs, coffset, items=None, doppler_search=None, ms=None, min_metric=None, min_ratio=None, M=16,
            loop_dwells=(500, 500), engine=None):
    """Acquire `name` on the interleaved int8 recording iq_int8 (numpy, host) exactly as the acquire command line does, keep the items
    whose metric reaches min_metric (default: all), upload the recording once, refine the kept results on it, drop those below
    min_ratio (default: none) and build one tracking channel per remaining item.
    Returns (acquisition results, [(item, Refined)], TrackLoop or None when nothing is left, device tensor)."""
    tracker = tracker_name(name)                     # refuses before any GPU work
    sig = signals.get(name)
    torch = nat.require_torch()
    eng = engine or acquire.default_engine()
    fs, coffset = float(fs), float(coffset)
    if items is None:
        items = acquire.parse_list_ranges(sig.default_items, sep=sig.item_sep) if sig.default_items else codes.prns(sig.code)
    items = [int(i) for i in items]
    doppler_search = list(sig.default_doppler if doppler_search is None else doppler_search)
    ms = 80 if ms is None else int(ms)
    ms_pad = ms + 5
    n = int(fs * 0.001 * ms_pad)
    iq = np.ascontiguousarray(iq_int8, dtype=np.int8).reshape(-1)
    iq = iq[:len(iq) // 2 * 2]
    if len(iq) < 2 * n:
        raise ValueError("recording too short: the acquisition needs %d complex int8 samples, it has %d" % (n, len(iq) // 2))
    results = eng.acquire_int8(sig, iq[:2 * n], fs, coffset, ms_pad, items, acquire.doppler_grid(doppler_search), max(sig.blocks(ms), 0))
    kept = [(it, r) for it, r in zip(items, results) if min_metric is None or float(r[0]) >= float(min_metric)]
    x_dev = torch.from_numpy(iq).to("cuda:%d" % eng.device)
    chip_rate = float(codes.chip_rate(trackloop.TRACKERS[tracker].code))
    cands = [_refine.Candidate(tracker, it, fs, coffset, float(r[2]), float(r[1]), float(doppler_search[2]), chip_rate / sig.fs)
             for it, r in kept]
    refined = list(zip([it for it, _ in kept], _refine.refine(cands, x_dev, M=M, engine=eng))) if cands else []
    refined = [(it, r) for it, r in refined if min_ratio is None or r.ratio >= float(min_ratio)]
    chans = [trackloop.Channel(tracker, fs, coffset, it, *_printed(tracker, r), tuple(float(v) for v in loop_dwells)) for it, r in refined]
    loop = trackloop.TrackLoop(chans, eng) if chans else None
    return results, refined, loop, x_dev


def track_all(name, iq_int8, fs, coffset, **kw):
    """handoff() and one batched run of the loop over the whole recording.
    Returns (acquisition results, [(item, Refined)], one record array per channel)."""
    results, refined, loop, x_dev = handoff(name, iq_int8, fs, coffset, **kw)
    if loop is None:
        return results, refined, []
    try:
        recs = loop.run([x_dev] * loop.K)
    finally:
        loop.close()
    return results, refined, recs


_VALUE_OPTS = ("--prn", "--channel", "--doppler-search", "--time", "--device", "--min-metric", "--min-ratio", "--blocks", "--loop-dwells",
               "--out-dir")


def _join_option_values(argv):
    """'--doppler-search -7000,7000,200' and '--channel -7:7' as the reference's optparse takes them: 'opt value' -> 'opt=value'"""
    out, i = [], 0
    while i < len(argv):
        if argv[i] in _VALUE_OPTS and i + 1 < len(argv):
            out.append(argv[i] + "=" + argv[i + 1])
            i += 2
        else:
            out.append(argv[i])
            i += 1
    return out


def build_parser(sig):
    ap = argparse.ArgumentParser(prog="handoff %s" % sig.name, description="Acquire %s, refine on the raw recording and hand off to the trackers" % sig.name)
    ap.add_argument(sig.item_opt, dest="items", default=sig.default_items, help="items to search, e.g. 1,3,7%s14 (default %%(default)s)" % sig.item_sep)
    ap.add_argument("--doppler-search", metavar="MIN,MAX,INCR", default=",".join("%g" % v for v in sig.default_doppler))
    ap.add_argument("--time", type=int, default=80, help="acquisition integration time in milliseconds (default %(default)s)")
    ap.add_argument("--device", type=int, default=0, help="GPU index")
    ap.add_argument("--min-metric", type=float, default=None, help="hand off only items whose acquisition metric reaches this (default: all)")
    ap.add_argument("--min-ratio", type=float, default=None, help="hand off only items whose refined peak/floor ratio reaches this (default: all)")
    ap.add_argument("--blocks", type=int, default=16, help="1 ms blocks of the fine search (default %(default)s)")
    ap.add_argument("--loop-dwells", default="500,500", help="wide FLL, then narrow FLL, in milliseconds (default %(default)s)")
    ap.add_argument("--out-dir", default=None, help="track every handed-off channel and write track-<tracker>-<item>.txt there")
    ap.add_argument("--nav", action="store_true", help="track every handed-off channel and print its navigation frames (trackers of navdata.FORMATS)")
    ap.add_argument("input_filename")
    ap.add_argument("sample_rate", type=float)
    ap.add_argument("carrier_offset", type=float)
    return ap


def parse(name, argv):
    """(signal, argparse namespace with .items as a list, .doppler_search and .loop_dwells as floats)"""
    tracker_name(name)
    sig = signals.get(name)
    a = build_parser(sig).parse_args(_join_option_values(list(argv)))
    a.items = acquire.parse_list_ranges(a.items, sep=sig.item_sep) if a.items else codes.prns(sig.code)
    a.doppler_search = acquire.parse_list_floats(a.doppler_search)
    a.loop_dwells = tuple(acquire.parse_list_floats(a.loop_dwells))
    return sig, a


def run(name, argv, out=sys.stdout):
    sig, a = parse(name, argv)
    tracker = tracker_name(name)
    raw = np.fromfile(a.input_filename, dtype=np.int8)
    need = int(a.sample_rate * 0.001 * (a.time + 5))
    if len(raw) // 2 < need:
        raise SystemExit("input file too short: need %d complex int8 samples" % need)
    eng = acquire.Engine(a.device)
    lines = []
    try:
        results, refined, loop, x_dev = handoff(name, raw, a.sample_rate, a.carrier_offset, a.items, a.doppler_search, a.time, a.min_metric,
                                                a.min_ratio, a.blocks, a.loop_dwells, eng)
        try:
            lines += [acquire.format_result(sig, it, r) for it, r in zip(a.items, results)]
            lines += [format_line(tracker, it, r) for it, r in refined]
            for line in lines:
                print(line, file=out)
            nav = a.nav and tracker in navdata.FORMATS
            if (a.out_dir is not None or nav) and loop is not None:
                tracked = loop.run([x_dev] * loop.K)
                if a.out_dir is not None:
                    os.makedirs(a.out_dir, exist_ok=True)
                    for (it, _), recs in zip(refined, tracked):
                        with open(os.path.join(a.out_dir, "track-%s-%d.txt" % (tracker, it)), "w") as f:
                            for line in trackloop.format_lines(tracker, recs):
                                f.write(line + "\n")
                if nav:
                    frames = navdata.decode_many([(recs, tracker, it) for (it, _), recs in zip(refined, tracked)], engine=eng)
                    more = [navdata.format_frame(tracker, it, fr) for (it, _), frs in zip(refined, frames) for fr in frs]
                    for line in more:
                        print(line, file=out)
                    lines += more
        finally:
            if loop is not None:
                loop.close()
    finally:
        eng.close()
    return lines


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    if not argv or argv[0] in ("-h", "--help"):
        print(__doc__)
        ok = []
        for s in sorted(signals.SIGNALS):
            try:
                tracker_name(s)
                ok.append(s)
            except HandoffError:
                pass
        print("signals:", ", ".join(ok))
        return 0
    run(argv[0], argv[1:])
    return 0


if __name__ == "__main__":
    sys.exit(main())
