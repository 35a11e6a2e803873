#!/usr/bin/env python3
"""Generate tests/golden/secondary_codes.json by IMPORTING THE REFERENCE's code modules and dumping every module-level
`secondary_code`: a +-1 array, or a per-PRN table of +-1 arrays (galileo.e5aq, galileo.e5bq, galileo.e6c).  Modules whose secondary
code is a function of the PRN (gps.l1cp, beidou.b1cp, beidou.b2ap: 1800-chip overlays generated on demand) have no module-level array
and are not covered.  tests/test_coherent_cpu.py holds gnss_dsp_tools_amd.coherent.SECONDARY to this file.

Re-running must leave `git diff tests/golden/` empty.  Needs the reference checkout and no GPU."""
import importlib
import json
import os
import pkgutil
import sys

import numpy as np

REF = os.environ.get("GNSS_REFERENCE", "/root/reference")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "secondary_codes.json")
sys.dont_write_bytecode = True
sys.path.insert(0, REF)


def as_pm1(a):
    a = np.asarray(a, dtype=np.float64)
    assert a.ndim == 1 and np.all(np.abs(a) == 1.0), a
    return [int(v) for v in a]


def main():
    import gnsstools
    found = {}
    for system in ("gps", "galileo", "beidou", "glonass", "xona"):
        pkg = importlib.import_module("gnsstools." + system)
        for m in pkgutil.iter_modules(pkg.__path__):
            mod = importlib.import_module("gnsstools.%s.%s" % (system, m.name))
            sc = getattr(mod, "secondary_code", None)
            if sc is None or callable(sc):
                continue
            name = "%s.%s" % (system, m.name)
            if isinstance(sc, dict):
                found[name] = {str(prn): as_pm1(sc[prn]) for prn in sorted(sc)}
            else:
                found[name] = as_pm1(sc)
    single = sorted(k for k, v in found.items() if isinstance(v, list))
    tables = sorted(k for k, v in found.items() if isinstance(v, dict))
    print("single arrays (%d): %s" % (len(single), ", ".join("%s[%d]" % (k, len(found[k])) for k in single)))
    print("per-PRN tables (%d): %s" % (len(tables), ", ".join("%s[%d x %d]" % (k, len(found[k]), len(next(iter(found[k].values())))) for k in tables)))
    with open(OUT, "w") as f:
        json.dump({"generator": "tools/make_goldens_secondary.py", "codes": found}, f, sort_keys=True, separators=(",", ":"))
        f.write("\n")
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
