"""Call times of the navigation-data entry points (navdata.py on csrc/gacq_navbits.hip) at user sizes, and the numpy definition
(tests/navdata_oracle.py) on subsets, scaled and labelled as such:

    python tools/bench_navdata.py [CALLS] [--no-oracle]

1. 4096 I/NAV block jobs in one launch; 2. one stream of 2^20 symbols at the default chunking; 3. navsym for 1024 channels of 60 000
records, R = 20.  The call times include the upload and the download; kernel times come from a run of this script under
``rocprofv3 --kernel-trace --stats`` (kernels navsym_kernel, viterbi_kernel)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import navdata_cases as C
import navdata_oracle as O
from gnss_dsp_tools_amd import acquire, navdata
import torch

REPS = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 5
ORACLE = "--no-oracle" not in sys.argv
eng = acquire.Engine(0)


def timed(label, fn, work, unit):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(REPS):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t)
    ts.sort()
    print("%s: call (upload + kernel + download) median %.3f ms, min %.3f ms, max %.3f ms over %d calls; %.3g %s/s of call time"
          % (label, 1e3 * ts[len(ts) // 2], 1e3 * ts[0], 1e3 * ts[-1], REPS, work / ts[len(ts) // 2], unit), flush=True)


# 1. 4096 I/NAV block jobs in one launch
J = 4096
rx = np.stack([C.block(C.BLOCK_KINDS[k % 3], 120, k, (8, 30), True)[0] for k in range(64)])
blocks = np.tile(rx, (J // 64, 1))
timed("1. %d I/NAV block jobs (120 steps, gathered)" % J, lambda: navdata.viterbi_blocks(blocks, (8, 30), True, engine=eng), J, "jobs")
if ORACLE:
    t = time.perf_counter()
    for r in rx[:16]:
        O.viterbi(r, 120, 8, 30, 0, 0, True)
    dt = time.perf_counter() - t
    print("   numpy definition: 16 jobs in %.3f s -> %.1f s for %d jobs (scaled from 16)" % (dt, dt * J / 16, J), flush=True)

# 2. one stream of 2^20 symbols at the default chunking
q, _ = C.noisy_stream(5, 1 << 19, 0.6)
timed("2. stream of 2^20 symbols (2^19 steps, 512 jobs of <= 1216 steps)", lambda: navdata.viterbi_stream(q, engine=eng), 1 << 20, "symbols")
if ORACLE:
    t = time.perf_counter()
    O.stream(q[:2 * 4096])
    dt = time.perf_counter() - t
    print("   numpy definition: 8192 symbols in %.3f s -> %.1f s for 2^20 symbols (scaled from 8192)" % (dt, dt * (1 << 20) / 8192), flush=True)

# 3. navsym: 1024 channels of 60 000 records, R = 20
K, n, R = 1024, 60000, 20
o = np.ones(R, dtype=np.int8)
base = [C.symbol_prompts(k, R, o, n, k % R) for k in range(8)]
chans = [base[k % 8] for k in range(K)]
timed("3. navsym, %d channels of %d records, R = %d" % (K, n, R), lambda: navdata.symbols_many(chans, [R] * K, [o] * K, engine=eng), K * (n // R), "symbols")
if ORACLE:
    t = time.perf_counter()
    for p in base:
        O.symbols(p, R, o)
    dt = time.perf_counter() - t
    print("   numpy definition: 8 channels in %.3f s -> %.1f s for %d channels (scaled from 8)" % (dt, dt * K / 8, K), flush=True)
eng.close()
