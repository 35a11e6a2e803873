#!/usr/bin/env python3
"""Time of the array prompts (gnss_dsp_tools_amd/arrayprompt.py, gacq_aprompt_dev) against the only other way to the same numbers.

One second of int8 I/Q at 4.092 MHz per antenna, resident in HBM; 8 GPS L1 C/A satellites with 1000 back-to-back 1 ms segments each.
Per M in 2, 4, 8: the median over --reps warm calls of arrayprompt.project on the M rows, and beside it the median of M calls of
cancel.apply(estimate=True) on the single rows, which rebuild the replica M times and run the subtraction kernel for an output that is
thrown away.  Both are whole calls as a user makes them (segment conversion, upload, launch, wait, download), timed on the host in one
process; the two results are compared bit for bit before anything is timed.

usage: tools/time_arrayprompt.py [--reps 20] [--warmup 3]
prints one line per M and a JSON summary line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gnss_dsp_tools_amd import _native as nat  # noqa: E402
from gnss_dsp_tools_amd import acquire, arrayprompt, cancel  # noqa: E402

FS, SEG, K, NSEG = 4.092e6, 4092, 8, 1000
MS = (2, 4, 8)


def scene():
    sats, segs = [], []
    for k in range(K):
        g = np.zeros(NSEG, dtype=cancel.SEG_DTYPE)
        dopp = -4000.0 + 1000.0 * k
        rate = 1.023e6 + dopp / 1540.0
        g["s0"] = np.arange(NSEG) * SEG
        g["n"] = SEG
        g["carrier_hz"] = dopp
        g["carrier_phase"] = (g["s0"] * (dopp / FS) + k / 32.0) % 1.0
        g["code_rate_hz"] = rate
        g["code_phase"] = (37.5 * k + g["s0"] * (rate / FS)) % 1023.0
        sats.append(cancel.Sat("gps.ca", k + 1, 0))
        segs.append(g)
    return sats, segs


def timed(torch, fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t))
    return float(np.median(ms)), float(np.min(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    torch = nat.require_torch()
    eng = acquire.Engine(0)
    dev = "cuda:0"
    n = SEG * NSEG
    g = torch.Generator(device=dev)
    g.manual_seed(20261021)
    x = torch.clamp(torch.round(12.0 * torch.randn(max(MS), 2 * n, generator=g, device=dev, dtype=torch.float32)), -127, 127).to(torch.int8)
    out = torch.empty(2 * n, dtype=torch.int8, device=dev)
    sats, segs = scene()
    rows = []
    for M in MS:
        xs = [x[p] for p in range(M)]
        singles = lambda: [cancel.apply(eng, sats, segs, FS, r, estimate=True, out=out)[1] for r in xs]
        together = lambda: arrayprompt.project(eng, sats, segs, FS, xs)[0]
        want, got = singles(), together()
        same = all(np.array_equal(np.ascontiguousarray(got[k][:, p]).view(np.uint64), want[p][k].view(np.uint64)) for k in range(K) for p in range(M))
        ms_p, min_p = timed(torch, together, a.reps, a.warmup)
        ms_c, min_c = timed(torch, singles, a.reps, a.warmup)
        rows.append(dict(M=M, satellites=K, segments=K * NSEG, samples=n, project_ms=ms_p, project_min_ms=min_p, cancel_calls_ms=ms_c, cancel_calls_min_ms=min_c,
                         ratio=ms_c / ms_p, bits_equal=bool(same)))
        print("M %d  project %8.3f ms (min %8.3f)  |  %d calls of cancel.apply(estimate=True) %8.3f ms (min %8.3f)  |  x%.2f  |  bits equal: %s"
              % (M, ms_p, min_p, M, ms_c, min_c, ms_c / ms_p, same))
    eng.close()
    print(json.dumps(dict(tool="time_arrayprompt", fs=FS, segment=SEG, reps=a.reps, rows=rows)))


if __name__ == "__main__":
    main()
