"""Call times of the bearing scan (bearing.py on csrc/gacq_bearing.hip) at a user size, beside the numpy definition:

    python tools/bench_bearing.py [CALLS] [--no-oracle]

M = 4 and 8 antennas on a ring, 16384 blocks of covariances resident on the device, the 5 degree grid (G = 1368) and the 2 degree grid
(G = 8280), K = 3 peaks 20 degrees apart, no spectrum output.  A call is the launches of gacq_bearing_run_dev (factors, spectrum and
peaks, per chunk of blocks) between two events on the stream, median of CALLS (default 5) after a warm-up call.  The line gives cells/s
and the fp64 operations/s that the definition's count implies: per cell M (M - 1) / 2 complex multiply-subtracts of 4 real
multiplications and 4 additions each in the elimination of b, then 2 M multiplications, M additions, M divisions and M - 1 additions
for q -- 4 M^2 + M - 1 operations (263 at M = 8, 67 at M = 4), a division counted as one.  The numpy definition
(tests/bearing_oracle.py) is timed on 16 blocks and scaled.
Kernel times come from a run of this script under ``rocprofv3 --kernel-trace --stats`` with --no-oracle (kernels
bearing_factor_kernel, bearing_spectrum_kernel)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from gnss_dsp_tools_amd import acquire, bearing
import torch

REPS = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 5
ORACLE = "--no-oracle" not in sys.argv
NBLK, K, SEP, SHIFT, SUBSET = 16384, 3, 20.0, 10, 16


def ring(M, radius=0.5):
    ang = 2.0 * np.pi * np.arange(M - 1) / (M - 1)
    return np.concatenate([np.zeros((1, 3)), np.stack([radius * np.cos(ang), radius * np.sin(ang), np.zeros(M - 1)], axis=1)])


def covariances(M, n, seed):
    """n Hermitian positive int64 matrices [n][M][M][2]: a jammer of varying strength and direction over noise, as window sums look"""
    rng = np.random.default_rng(seed)
    s = rng.normal(size=(n, M, 2 * M)) + 1j * rng.normal(size=(n, M, 2 * M))
    s[:, :, 0] *= 8.0
    R = np.einsum("npk,nqk->npq", s, np.conj(s)) * 4096.0
    return np.ascontiguousarray(np.stack([np.rint(R.real), np.rint(R.imag)], axis=3).astype(np.int64))


eng = acquire.Engine(0)
dev = "cuda:%d" % eng.device
rows = []
for M in (4, 8):
    R = covariances(M, NBLK, 11 + M)
    cov = torch.from_numpy(R).to(dev)
    for step in (5.0, 2.0):
        cells = bearing.grid(step)
        G = len(cells)
        with bearing.Finder(eng, ring(M), cells, SHIFT, K, SEP) as fd:
            fd.run(cov)
            torch.cuda.synchronize()
            ts = []
            for _ in range(REPS):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                out = fd.run(cov)
                b.record()
                torch.cuda.synchronize()
                ts.append(a.elapsed_time(b))
            ts.sort()
            ms = ts[len(ts) // 2]
            pk = bearing.records(out[0])
        ops = 4 * M * M + M - 1
        row = dict(antennas=M, cells=G, blocks=NBLK, peaks=K, ms=ms, ms_min=ts[0], ms_max=ts[-1], gcells_per_s=NBLK * G / ms * 1e-6,
                   fp64_ops_per_cell=ops, fp64_tops=NBLK * G * ops / ms * 1e-9, oracle_ms=None)
        if ORACLE:
            import bearing_oracle as B
            a_tab, u_tab = bearing.tables(ring(M), cells)
            t0 = time.perf_counter()
            want = B.run(R[:SUBSET, ..., 0], R[:SUBSET, ..., 1], SHIFT, a_tab, u_tab, K, float(np.cos(np.deg2rad(SEP))))
            row["oracle_ms"] = (time.perf_counter() - t0) * 1e3 * NBLK / SUBSET
            assert pk[:SUBSET].tobytes() == want[0].tobytes(), "the device's records are not the oracle's"
        rows.append(row)
        print("M %d G %5d: %.3f ms (min %.3f, max %.3f over %d calls)  %.2f Gcell/s  %.2f Top/s fp64%s"
              % (M, G, ms, ts[0], ts[-1], REPS, row["gcells_per_s"], row["fp64_tops"],
                 "" if row["oracle_ms"] is None else "   numpy: %.0f ms scaled from %d blocks, x%.0f" % (row["oracle_ms"], SUBSET, row["oracle_ms"] / ms)), flush=True)
    del cov
print(json.dumps(dict(tool="bench_bearing", rows=rows)))
eng.close()
