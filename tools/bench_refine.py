#!/usr/bin/env python3
"""Time of the fine search's correlation grid (refine.corr_grid, csrc/gacq_corrgrid.hip): K = 32 GPS L1 candidates, M = 16 blocks, the
default grid (D = 5, P = 9 + the floor entry) on one 69.984 MS/s noise recording resident on the device; HIP events around the call,
warm-up, then the median of 20 runs.

Against the same grid built from what the package had before, in the same process: Engine.mix_int8_dev once, then one
tracking.correlate_batch call (K x P correlators) per block and Doppler hypothesis.  That baseline is a timing stand-in and a
conservative one: correlate_batch has no carrier argument, so the per-hypothesis Doppler wipe-off it would need (one more mix per
hypothesis) is left out, and all candidates read one common block instead of their own code-aligned ones.  Prints one JSON line.
usage: tools/bench_refine.py [--k 32] [--blocks 16] [--runs 20]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gnss_dsp_tools_amd import acquire, refine, tracking  # noqa: E402

FS = 69.984e6


def timed(torch, fn, warmup, runs):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=32)
    ap.add_argument("--blocks", type=int, default=16)
    ap.add_argument("--runs", type=int, default=20)
    a = ap.parse_args()
    torch = refine.nat.require_torch()
    eng = acquire.default_engine()
    eng.use_torch_stream(torch.device("cuda", eng.device))
    n = int(FS * 0.001)
    nsamp = (a.blocks + 2) * n
    rng = np.random.Generator(np.random.PCG64(7))
    x = torch.from_numpy(np.clip(np.round(rng.normal(0.0, 12.0, size=2 * nsamp)), -127, 127).astype(np.int8)).to("cuda:%d" % eng.device)
    cands = [refine.Candidate("gps-l1", 1 + k % 32, FS, 250000.0, -3000.0 + 200.0 * k, 31.7 * k + 0.4, 200.0, 1.023e6 / 4.096e6)
             for k in range(a.k)]
    grids = [refine.default_grid(c, a.blocks) for c in cands]
    new_med, new_min = timed(torch, lambda: refine.corr_grid(grids, x, eng), 3, a.runs)

    g0 = grids[0]
    prns = np.repeat([g.prn for g in grids], g0.P)
    frac = np.concatenate([g.code0 + g.offsets for g in grids])
    incr = np.repeat([(g.chip_rate + g.doppler0 / g.ratio) / FS for g in grids], g0.P)

    def baseline():
        y = eng.mix_int8_dev(x, FS, 250000.0)
        for m in range(a.blocks):
            seg = y[n + m * n:n + (m + 1) * n]
            for _ in range(g0.D):
                tracking.correlate_batch("gps.ca", seg, prns, 0.0, frac, incr, eng)

    old_med, old_min = timed(torch, baseline, 1, max(3, a.runs // 4))
    print(json.dumps({"fs": FS, "K": a.k, "M": a.blocks, "D": g0.D, "P": g0.P, "n": n, "corr_grid_ms_median": new_med, "corr_grid_ms_min": new_min,
                      "mix_plus_correlate_batch_ms_median": old_med, "mix_plus_correlate_batch_ms_min": old_min,
                      "speedup_median": old_med / new_med}))


if __name__ == "__main__":
    main()
