#!/usr/bin/env python3
"""Generate tests/golden/trackloop_cases.json (+ trackloop_*_int8.iq) by RUNNING THE REFERENCE'S track-*.py SCRIPTS, unmodified, as
subprocesses on synthetic int8 recordings written here (as tools/make_goldens_cli.py does for the acquire scripts).

  1. a seeded recording -- noise sigma 18 per component plus one satellite (its code, subcarrier and carrier at the file rate),
     rounded and clipped to int8, interleaved I/Q -- is written to tests/golden/trackloop_<file>_int8.iq;
  2. `<reference>/track-<name>.py [--loop-dwells A,B] [--carrier-phase P] FILE FS COFFSET PRN|CHAN DOPPLER CODE_OFFSET` runs
     (PYTHONPATH=<reference>, cwd=/tmp) and its stdout lines become the case's `stdout_lines`;
  3. each script's constants are read off its source (regular expressions over the template's lines) and stored as `params`, which
     tests/test_track_loop_cpu.py holds trackloop.TRACKERS to.

Without numba the reference's loops are interpreted, but correlate() still accumulates in complex128 (x[i] is complex64, the
chip weight float64), so the lines carry the same numerics as the compiled scripts.  Re-running this script must leave
`git diff tests/golden/trackloop_*` empty.  Needs the reference checkout and a built libgacq.so (host part); no GPU.
"""
import glob
import json
import os
import re
import subprocess
import sys

import numpy as np

REF = os.environ.get("GNSS_REFERENCE", "/root/reference")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)

from gnss_dsp_tools_amd import codes  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
SEED = 20261015
NOISE = 18.0
OUT_OF_SCOPE = ("beidou-b2bi", "beidou-b2bq", "gps-l2cl", "glonass-l1-p", "glonass-l2-p")

# file: (tracker, fs, coffset, prn or chan, doppler, code_offset, seconds, amplitude)
FILES = {
    "gps_l1": ("gps-l1", 21.0e6, 123456.0, 7, 1200.0, 300.25, 0.0145, 10.0),
    "xona_x1d": ("xona-x1d", 2.5e6, -40000.0, 0, -800.0, 111.5, 0.0125, 10.0),
    "galileo_e1b": ("galileo-e1b", 6.0e6, 250000.0, 11, 1500.0, 1000.75, 0.0205, 6.0),
    "gps_l1cp": ("gps-l1cp", 5.5e6, -100000.0, 5, -2000.0, 2500.5, 0.0405, 4.0),
    "beidou_b1cd": ("beidou-b1cd", 5.5e6, 60000.0, 30, 900.0, 7000.25, 0.0355, 4.0),   # ends in the middle of its 4th outer block
    "gps_l2cm": ("gps-l2cm", 2.1e6, 50000.0, 1, 700.0, 5000.5, 0.0805, 4.0),
    "glonass_l1": ("glonass-l1", 2.5e6, 180000.0, -3, 1100.0, 200.5, 0.0145, 10.0),
    "gps_l5i": ("gps-l5i", 21.0e6, -70000.0, 12, -1500.0, 4000.25, 0.0125, 6.0),
}

# case: (file, argv options)
CASES = {
    "gps_l1": ("gps_l1", ["--loop-dwells", "4,4"]),
    "gps_l1_carrier_phase": ("gps_l1", ["--carrier-phase", "-0.214"]),
    "xona_x1d": ("xona_x1d", ["--loop-dwells", "4,4"]),
    "galileo_e1b": ("galileo_e1b", ["--loop-dwells", "6,8"]),
    "gps_l1cp": ("gps_l1cp", ["--loop-dwells", "5,15"]),
    "beidou_b1cd": ("beidou_b1cd", ["--loop-dwells", "10,10"]),
    "gps_l2cm": ("gps_l2cm", ["--loop-dwells", "20,20"]),
    "glonass_l1": ("glonass_l1", ["--loop-dwells", "4,4"]),
    "gps_l5i": ("gps_l5i", ["--loop-dwells", "4,4"]),
}


def script_params(path):
    """The constants of one template track script, read off its source."""
    s = open(path).read()
    mod = re.search(r"import gnsstools\.(\w+)\.(\w+) as (\w+)", s)
    code = mod.group(1) + "." + mod.group(2)
    alias = mod.group(3)
    live = "\n".join(l for l in s.split("\n") if not l.lstrip().startswith("#"))
    p = {"code": code}
    m = re.search(r"correlate\(x, (?:s\.prn, )?0, s\.code_p-([0-9.]+), cf, [^)]*\)(, %s\.boc11)?\)" % alias, live)
    p["spacing"] = float(m.group(1))
    m = re.search(r"cf = \(s\.code_f\+s\.carrier_f/([0-9.]+)\)/fs", live)
    p["ratio"] = float(m.group(1)) if m else None
    m = re.search(r"rf_carrier = ([0-9.]+) \+ ([0-9.]+)\*chan\n\s*scale_factor = rf_carrier/([0-9.]+)", live)
    m2 = re.search(r"fm = -\(coffset\+(\d+)\*chan\)/fs", live)
    p["glonass"] = [float(m.group(1)), float(m.group(2)), float(m.group(3)), int(m2.group(1))] if m else None
    m = re.search(r"n = int\(fs\*([0-9.]+)\*\(\(%s\.code_length-code_offset\)" % alias, live)
    p["period"] = float(m.group(1))
    m = re.search(r"code_offset \+= n\*([0-9.]+)\*%s\.code_length/fs" % alias, live)
    p["rate"] = float(m.group(1))
    m = re.search(r"for j in range\((\d+)\):", live)
    p["subs"] = int(m.group(1)) if m else 1
    p["pll"] = [float(re.search(r"pll_k1 = ([0-9.]+)", live).group(1)), float(re.search(r"pll_k2 = ([0-9.]+)", live).group(1))]
    p["dll"] = [float(re.search(r"dll_k1 = ([0-9.]+)", live).group(1)), float(re.search(r"dll_k2 = ([0-9.]+)", live).group(1))]
    p["fll"] = [float(x) for x in re.findall(r"fll_k = ([0-9.]+)", live)]
    p["cols"] = max(len(re.findall(r"%[df]", l)) for l in live.split("\n") if "print(" in l)
    p["fixed_pll"] = "mode='PLL')" in live and "s.mode = 'FLL_NARROW'" not in live
    p["carrier_phase"] = "carrier_p=carrier_p," in live
    kind = 0
    if "boc11" in live:
        kind = {"galileo.e1b": 2, "galileo.e1c": 2, "gps.l1cp": 3}.get(code, 1)
    if code == "gps.l2cm":
        kind = 4
    p["kind"] = kind
    return p


def recording(name, tracker, fs, coffset, prn, doppler, code_offset, seconds, amp, seed):
    """noise + amp * code(code_offset + chip_rate/fs * i) [* subcarrier] * exp(2 pi i (coffset + doppler) i / fs), int8 I/Q."""
    params = script_params(os.path.join(REF, "track-%s.py" % tracker))
    code = params["code"]
    n = int(round(fs * seconds))
    i = np.arange(n, dtype=np.float64)
    rng = np.random.Generator(np.random.PCG64(seed))
    x = NOISE * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    c = codes.chips(code, 0 if params["glonass"] else prn)
    L = len(c)
    rate = codes.chip_rate(code) / fs
    ph = code_offset + rate * i
    w = 1.0 - 2.0 * c[np.mod(np.floor(ph).astype(np.int64), L)]
    if params["kind"] in (1, 2, 3):
        w = w * (1.0 - 2.0 * (np.floor(2 * ph).astype(np.int64) & 1))
    elif params["kind"] == 4:
        w = w * ((np.floor(2 * ph).astype(np.int64) & 1) == 0)
    f = coffset + doppler
    if params["glonass"]:
        f = coffset + params["glonass"][3] * prn + doppler
    x = x + amp * w * np.exp(2j * np.pi * f * i / fs)
    iq = np.empty((n, 2), dtype=np.int8)
    iq[:, 0] = np.clip(np.round(x.real), -127, 127)
    iq[:, 1] = np.clip(np.round(x.imag), -127, 127)
    path = os.path.join(GOLD, "trackloop_%s_int8.iq" % name)
    iq.tofile(path)
    return path


# The Weil / Legendre codes (B1C, L1C) are built from sympy's legendre_symbol, which current sympy returns as a sympy Integer:
# the chip arrays become object arrays and the scripts' correlate() fails on them.  Older sympy returned a Python int, which is
# what the scripts were written against; this shim restores that before the script runs (the script itself is run unmodified).
SHIM = ("import runpy, sys\n"
        "import sympy.ntheory as nt\n"
        "_ls = nt.legendre_symbol\n"
        "nt.legendre_symbol = lambda a, p: int(_ls(a, p))\n"
        "sys.argv = sys.argv[1:]\n"
        "runpy.run_path(sys.argv[0], run_name='__main__')\n")


def run_reference(tracker, argv, path, fs, coffset, prn, doppler, code_offset):
    cmd = [sys.executable, "-c", SHIM, os.path.join(REF, "track-%s.py" % tracker)] + list(argv) + [
        os.path.abspath(path), repr(float(fs)), repr(float(coffset)), str(int(prn)), repr(float(doppler)), repr(float(code_offset))]
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1", PYTHONPATH=REF)
    out = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd="/tmp")
    if out.returncode != 0:
        raise RuntimeError("%s failed: %s" % (" ".join(cmd), out.stderr[-2000:]))
    return cmd[4:-6], out.stdout.splitlines()


def main():
    params = {}
    for path in sorted(glob.glob(os.path.join(REF, "track-*.py"))):
        name = os.path.basename(path)[len("track-"):-3]
        if name not in OUT_OF_SCOPE:
            params[name] = script_params(path)
    files = {}
    for k, (fname, (tracker, fs, coffset, prn, doppler, code_offset, seconds, amp)) in enumerate(sorted(FILES.items())):
        path = recording(fname, tracker, fs, coffset, prn, doppler, code_offset, seconds, amp, SEED + k)
        files[fname] = dict(tracker=tracker, fs=fs, coffset=coffset, prn=prn, doppler=doppler, code_offset=code_offset,
                            file=os.path.basename(path), nsamp=os.path.getsize(path) // 2)
    cases = {}
    for case, (fname, argv) in sorted(CASES.items()):
        f = files[fname]
        opts, lines = run_reference(f["tracker"], argv, os.path.join(GOLD, f["file"]), f["fs"], f["coffset"], f["prn"], f["doppler"],
                                    f["code_offset"])
        cases[case] = dict(f, argv=opts, stdout_lines=lines)
        print(case, len(lines), "lines", file=sys.stderr)
    out = {"generator": "reference track-*.py scripts run as subprocesses on the synthetic int8 recordings next to this file "
                        "(tools/make_goldens_trackloop.py)",
           "params": params, "cases": cases}
    with open(os.path.join(GOLD, "trackloop_cases.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()
