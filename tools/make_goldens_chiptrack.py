#!/usr/bin/env python3
"""Generate tests/golden/chiptrack_cases.json.gz by RUNNING THE REFERENCE'S track-beidou-b2bi.py and track-beidou-b2bq.py, unmodified,
as subprocesses in a temporary working directory on seeded synthetic int8 recordings.

  1. a recording -- noise sigma 18 per component plus one satellite (or none), tests/chiptrack_cases.synth() -- is written to a
     temporary file; only its seed and SHA-256 are stored, and the tests regenerate it;
  2. the numpy oracle (tests/chiptrack_oracle.py) walks the case and, for every accumulated frame, the closed-form prompt indices
     (tracking_oracle.closed_form_indices, the device kernel's bins) are checked against the repeated addition the reference's
     nco.accum does (sequential_indices).  A seed where they disagree is replaced by the next one, and this script says so;
  3. `<reference>/track-<name>.py [--loop-dwells A,B] [--carrier-phase P] FILE FS COFFSET PRN DOPPLER CODE_OFFSET` runs; its stdout
     lines become `stdout_lines` and the track-chips.dat it writes becomes `chips_gz` (gzip, hex);
  4. each script's constants are read off its source (make_goldens_longtrack's expressions) and stored as `params`.

numba is absent, so the reference runs interpreted.  Needs the reference checkout and a built libgacq.so (host part); no GPU.
"""
import gzip
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ProcessPoolExecutor

import numpy as np

REF = os.environ.get("GNSS_REFERENCE", "/root/reference")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from gnss_dsp_tools_amd import chiptrack, codes  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
SEED = 20261017
TRIES = 6
L = 10230

# case: (tracker, argv options, fs, coffset, prn, doppler, code_offset, seconds, amplitude)
CASES = {
    # FLL_WIDE -> FLL_NARROW -> PLL well before frame 201; 14 accumulated frames; the recording ends inside frame 215
    "b2bi_modes": ("beidou-b2bi", ["--loop-dwells", "60,80"], 20.7e6, 150000.0, 21, 1300.0, L - 1200.25, 0.2157, 5.0),
    # PLL from the start with a negative initial phase
    "b2bq_carrier_phase": ("beidou-b2bq", ["--carrier-phase", "-0.3"], 21.3e6, -90000.0, 33, -700.0, 3000.5, 0.2125, 6.0),
    # ends before frame 201: every bin stays zero
    "b2bi_short": ("beidou-b2bi", [], 20.1e6, 50000.0, 44, 400.0, 7000.75, 0.15, 5.0),
    # weak signal (a noise-only loop wanders chaotically, and the last-ulp differences of the correlator sums grow into printed ones)
    "b2bq_weak": ("beidou-b2bq", ["--loop-dwells", "100,50"], 21.0e6, 0.0, 27, 300.0, 5000.0, 0.214, 1.5),
}


def script_params(path):
    """The constants of one B2b track script, read off its source with make_goldens_longtrack's expressions, plus the accumulation
    threshold, the chips file and its length."""
    s = open(path).read()
    mod = re.search(r"import gnsstools\.(\w+)\.(\w+) as (\w+)", s)
    alias = mod.group(3)
    live = "\n".join(l for l in s.split("\n") if not l.lstrip().startswith("#"))
    p = {"code": mod.group(1) + "." + mod.group(2)}
    m = re.search(r"for j in range\((\d+)\):", live)                   # track() calls per block: none of these scripts splits a block
    p["subs"] = int(m.group(1)) if m else 1
    m = re.search(r"rf_carrier = ([0-9.]+) \+ ([0-9.]+)\*chan\n\s*scale_factor = rf_carrier/([0-9.]+)", live)
    m2 = re.search(r"fm = -\(coffset\+(\d+)\*chan\)/fs", live)
    p["glonass"] = [float(m.group(1)), float(m.group(2)), float(m.group(3)), int(m2.group(1))] if m else None
    # correlator kind from the code module's correlate(): a BOC / RZ table in it would make it other than plain (kind 0)
    src = open(os.path.join(REF, "gnsstools", mod.group(1), mod.group(2) + ".py")).read()
    corr = re.search(r"def correlate\(.*?(?=\n\S|\Z)", src, re.S).group(0)
    p["kind"] = 0 if not re.search(r"boc|rz|tmboc", corr) else None
    p["spacing"] = float(re.search(r"correlate\(x, s\.prn, 0, s\.code_p-([0-9.]+), cf, [^)]*\)\)", live).group(1))
    p["ratio"] = float(re.search(r"cf = \(s\.code_f\+s\.carrier_f/([0-9.]+)\)/fs", live).group(1))
    p["period"] = float(re.search(r"n = int\(fs\*([0-9.]+)\*\(\(%s\.code_length-code_offset\)" % alias, live).group(1))
    p["rate"] = float(re.search(r"code_offset \+= n\*([0-9.]+)\*%s\.code_length/fs" % alias, live).group(1))
    p["pll"] = [float(re.search(r"pll_k1 = ([0-9.]+)", live).group(1)), float(re.search(r"pll_k2 = ([0-9.]+)", live).group(1))]
    p["dll"] = [float(re.search(r"dll_k1 = ([0-9.]+)", live).group(1)), float(re.search(r"dll_k2 = ([0-9.]+)", live).group(1))]
    p["fll"] = [float(x) for x in re.findall(r"fll_k = ([0-9.]+)", live)]
    p["cols"] = max(len(re.findall(r"%[df]", l)) for l in live.split("\n") if "print(" in l)
    p["fixed_pll"] = "mode='PLL')" in live and "s.mode = 'FLL_NARROW'" not in live
    p["carrier_phase"] = "carrier_p=carrier_p," in live
    p["accum_after"] = int(re.search(r"if s\.nframe>(\d+):", live).group(1))
    p["chips_file"] = re.search(r'open\("([^"]+)","w"\)', live).group(1)
    p["code_length"] = int(re.search(r"np\.zeros\((\d+)\)\.astype\('complex'\)", live).group(1))
    return p


def indices_agree(spec, chips01, iq):
    """closed_form_indices == sequential_indices for the prompt of every frame the oracle accumulates."""
    from chiptrack_oracle import track
    from oracle import tracking_oracle as T
    trace = []
    track(spec, chips01, iq, trace=trace)
    for j, (code_p, cf, m) in enumerate(trace):
        sidx = T.sequential_indices(L, 0, [code_p], cf, m)[0][0]
        idx = T.closed_form_indices(L, 0, code_p, cf, m)[0]
        if not np.array_equal(idx, sidx):
            return "accumulated frame %d" % j
    return None


def run_reference(tracker, argv, path, fs, coffset, prn, doppler, code_offset):
    cmd = [sys.executable, os.path.join(REF, "track-%s.py" % tracker)] + list(argv) + [
        path, repr(float(fs)), repr(float(coffset)), str(int(prn)), repr(float(doppler)), repr(float(code_offset))]
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1", PYTHONPATH=REF)
    with tempfile.TemporaryDirectory() as wd:
        out = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=wd)
        if out.returncode != 0:
            raise RuntimeError("%s failed: %s" % (" ".join(cmd), out.stderr[-2000:]))
        chips = open(os.path.join(wd, "track-chips.dat")).read()
    return out.stdout.splitlines(), chips


def make_case(k, cid):
    import chiptrack_cases as C
    from chiptrack_oracle import track
    tracker, argv, fs, coffset, prn, doppler, code_offset, seconds, amp = CASES[cid]
    chips01 = codes.chips(chiptrack.CHIP_TRACKERS[tracker].code, prn)
    for attempt in range(TRIES):
        seed = SEED + 100 * k + attempt
        iq = C.synth(tracker, fs, coffset, prn, doppler, code_offset, seconds, amp, seed)
        case = dict(tracker=tracker, argv=list(argv), fs=fs, coffset=coffset, prn=prn, doppler=doppler, code_offset=code_offset,
                    seconds=seconds, amp=amp, seed=seed, nsamp=len(iq) // 2, sha256=hashlib.sha256(iq.tobytes()).hexdigest())
        spec = chiptrack.chip_channel_spec(C.channel_of(case))
        bad = indices_agree(spec, chips01, iq)
        if bad is None:
            break
        print("%s: seed %d replaced -- the reference's repeated addition crosses a chip boundary the closed form does not (%s)"
              % (cid, seed, bad), file=sys.stderr)
    else:
        raise RuntimeError("%s: no seed in %d tries" % (cid, TRIES))
    _, _, signs = track(spec, chips01, iq)
    case["signs"] = sorted(set(signs.values()))
    if cid == "b2bi_modes":              # the residual frequency turns the prompt: both sign branches are taken
        assert case["signs"] == [-1.0, 1.0], case["signs"]
    with tempfile.NamedTemporaryFile(suffix=".iq") as f:
        iq.tofile(f.name)
        case["stdout_lines"], chips = run_reference(tracker, argv, f.name, fs, coffset, prn, doppler, code_offset)
    case["chips_gz"] = gzip.compress(chips.encode(), compresslevel=9, mtime=0).hex()
    print(cid, "seed", case["seed"], len(case["stdout_lines"]), "lines", file=sys.stderr)
    return cid, case


def main():
    params = {name: script_params(os.path.join(REF, "track-%s.py" % name)) for name in sorted(chiptrack.CHIP_TRACKERS)}
    ids = sorted(CASES)
    with ProcessPoolExecutor(len(ids)) as pool:
        cases = dict(pool.map(make_case, range(len(ids)), ids))
    out = {"generator": "reference track-beidou-b2bi.py / track-beidou-b2bq.py run as subprocesses on seeded synthetic int8 recordings "
                        "(tools/make_goldens_chiptrack.py; tests/chiptrack_cases.synth regenerates them)",
           "params": params, "cases": cases}
    text = json.dumps(out, indent=1, sort_keys=True) + "\n"
    with open(os.path.join(GOLD, "chiptrack_cases.json.gz"), "wb") as raw:
        with gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0, compresslevel=9) as fh:
            fh.write(text.encode())


if __name__ == "__main__":
    main()
