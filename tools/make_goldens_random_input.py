#!/usr/bin/env python3
"""Generate tests/golden/random_input_b1i.json by RUNNING THE REFERENCE in this container.

The reference's unmodified search() of acquire-beidou-b1i.py (exec'd up to its "# main program" marker, as in
tools/make_goldens.py) on plain seeded Gaussian noise -- numpy default_rng(7), 4 x 8192 complex128 samples, not the synthetic
IQ of synth.py -- so that tests/test_oracle_golden.py::test_oracle_against_live_reference holds the oracle to the reference on
input no other golden case uses.  Data only: the spec, a SHA-256 of the sample bytes and search()'s (metric, code, doppler).

Needs the reference (GNSS_REFERENCE, default /root/reference).  Never runs on the GPU box.
"""
import hashlib
import json
import os
import sys

import numpy as np

REF = os.environ.get("GNSS_REFERENCE", "/root/reference")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.dont_write_bytecode = True
sys.path.insert(0, REF)

SPEC = {"script": "beidou-b1i", "seed": 7, "nsamp": 4 * 8192, "item": 9, "doppler_search": [-600.0, 600.0, 300.0], "ms": 2}


def make_x(spec):
    rng = np.random.default_rng(spec["seed"])
    return rng.standard_normal(spec["nsamp"]) + 1j * rng.standard_normal(spec["nsamp"])


def main():
    path = os.path.join(REF, "acquire-%s.py" % SPEC["script"])
    src = open(path).read().split("#\n# main program\n#")[0]
    ns = {}
    exec(compile(src, path, "exec"), ns)
    x = make_x(SPEC)
    metric, code, doppler = ns["search"](x, SPEC["item"], SPEC["doppler_search"], SPEC["ms"])
    out = dict(SPEC, x_sha256=hashlib.sha256(x.tobytes()).hexdigest(),
               result=[float(metric), float(code), float(doppler)],
               generator="tools/make_goldens_random_input.py", reference="pmonta/GNSS-DSP-tools @ 2025-08-29")
    with open(os.path.join(ROOT, "tests", "golden", "random_input_b1i.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(out)


if __name__ == "__main__":
    main()
