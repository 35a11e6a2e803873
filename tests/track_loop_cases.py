"""Shared helpers of the tracking-loop tests: the golden cases of tools/make_goldens_trackloop.py and the line comparison."""
import json
import os

import numpy as np

from gnss_dsp_tools_amd import track, trackloop

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")

# columns printed with %d: block; and code_cyc, carrier_cyc, samp in the 14-column scripts
INT_COLS = {9: (0,), 14: (0, 9, 11, 13)}
# Float columns: the reference prints 6 decimals, so a value that agrees to well below 1e-6 still shows up to half a unit of the last
# digit away from the printed string (5e-7), plus what the two computations may legitimately differ by.  They differ in the order of
# the correlator sums (sequential vs. a tree / dot product: a few ulp of sums of |x| <= 4e5, ~1e-10) and in the closed-form code
# phases (tracking_oracle: one rounding instead of a repeated sum), which the feedback loops carry into the states.  Measured on the
# golden cases: the largest deviation from the printed value is below 6e-7 (see test_oracle_reproduces_golden_lines); the bound
# leaves room for one printed digit and nothing more.  Every plausible bug below moves some column by far more (>= 1e-3).
LINE_ABS = 1.0e-6
LINE_REL = 1.0e-9


def load():
    with open(os.path.join(GOLD, "trackloop_cases.json")) as f:
        return json.load(f)


def channel_of(case):
    """trackloop.Channel of a golden case, parsed from its stored command line by the CLI's parser."""
    argv = list(case["argv"]) + [case["file"], repr(case["fs"]), repr(case["coffset"]), str(case["prn"]), repr(case["doppler"]),
                                 repr(case["code_offset"])]
    _, ch = track.parse(case["tracker"], argv)
    return ch


def recording(case):
    return np.fromfile(os.path.join(GOLD, case["file"]), dtype=np.int8)


def line_deviation(got, want):
    """(max over float columns of |got - want| / (LINE_ABS + LINE_REL |want|), integer columns equal?) of two output lines."""
    g, w = got.split(), want.split()
    if len(g) != len(w):
        return np.inf, False
    ints = INT_COLS[len(w)]
    ok = all(int(g[i]) == int(w[i]) for i in ints)
    worst = 0.0
    for i in range(len(w)):
        if i in ints:
            continue
        a, b = float(g[i]), float(w[i])
        worst = max(worst, abs(a - b) / (LINE_ABS + LINE_REL * abs(b)))
    return worst, ok


def lines_match(got, want):
    """(all lines within the bound, worst ratio, worst absolute deviation)"""
    if len(got) != len(want):
        return False, np.inf, np.inf
    worst, worst_abs, ok = 0.0, 0.0, True
    for a, b in zip(got, want):
        r, iok = line_deviation(a, b)
        ok = ok and iok
        worst = max(worst, r)
        worst_abs = max(worst_abs, max((abs(float(x) - float(y)) for x, y in zip(a.split(), b.split())), default=0.0))
    return ok and worst <= 1.0, worst, worst_abs


def oracle_lines(name, spec, chips01, iq, **kw):
    from track_loop_oracle import track as oracle_track
    recs = oracle_track(spec, chips01, iq, **kw)
    arr = np.zeros(len(recs), dtype=trackloop.RECORD_DTYPE)
    for i, r in enumerate(recs):
        for k, v in r.items():
            arr[i][k] = v
    return arr, trackloop.format_lines(name, arr)
