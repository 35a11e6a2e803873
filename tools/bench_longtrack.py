#!/usr/bin/env python3
"""Throughput of the long-code tracking loops (longtrack.LongTrackLoop) at 69.984 MS/s on a resident int8 recording (one 1.5 s L2CL
outer block, one 1 s GLONASS P block; random samples, shared by every channel).  Reports, per tracker:
  - us_per_ms: wall time of one launch per record (1 ms sub-block) per channel at K = 1 -- the kernel dominates the launch; run under
    `rocprofv3 --kernel-trace --stats` for the kernel's own time;
  - ms of signal tracked per second of wall time at K = 1, 8 and 32 (per channel and in aggregate);
  - feed() with 10 ms chunks against run() on the whole recording, K = 1.
Prints one JSON line.  usage: tools/bench_longtrack.py [--ks 1,8,32] [--repeats 3]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gnss_dsp_tools_amd import acquire, codes, longtrack, trackloop  # noqa: E402

FS = 69.984e6
SECONDS = 1.52


def channels(name, K):
    L = codes.code_length(longtrack.LONG_TRACKERS[name].code)
    out = []
    for k in range(K):
        prn = 1 + k % 32 if name == "gps-l2cl" else k % 15 - 7
        out.append(trackloop.Channel(name, FS, 0.0, prn, 0.0, L - 100.5 - k, (500.0, 500.0)))
    return out


def timed(fn, repeats):
    torch = longtrack.nat.require_torch()
    best = None
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best, out


def run_once(eng, chans, x):
    tl = longtrack.LongTrackLoop(chans, eng)
    try:
        return tl.run([x] * len(chans))
    finally:
        tl.close()


def feed_once(eng, chans, x, chunk):
    tl = longtrack.LongTrackLoop(chans, eng)
    n = x.numel() // 2
    got = []
    try:
        for a in range(0, n, chunk):
            got.append(tl.feed([x[2 * a:2 * min(n, a + chunk)]] * len(chans))[0])
    finally:
        tl.close()
    return got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="1,8,32")
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    torch = longtrack.nat.require_torch()
    eng = acquire.default_engine()
    n = int(FS * SECONDS)
    g = torch.Generator(device="cuda:%d" % eng.device)
    g.manual_seed(7)
    x = torch.randint(-20, 21, (2 * n,), dtype=torch.int8, device="cuda:%d" % eng.device, generator=g)
    res = {"fs": FS, "seconds": SECONDS}
    for name in ("gps-l2cl", "glonass-l1-p"):
        r = {"K": []}
        for K in [int(k) for k in a.ks.split(",")]:
            chans = channels(name, K)
            run_once(eng, chans, x)                              # chips uploaded, code objects loaded
            dt, recs = timed(lambda: run_once(eng, chans, x), a.repeats)
            ms = float(len(recs[0]))
            r["K"].append(dict(K=K, ms_signal=ms, wall_s=dt, ms_per_s_per_channel=ms / dt, ms_per_s_aggregate=K * ms / dt))
            if K == 1:
                r["us_per_ms_K1"] = 1e6 * dt / ms
        chans = channels(name, 1)
        dt_run, whole = timed(lambda: run_once(eng, chans, x), a.repeats)
        dt_feed, parts = timed(lambda: feed_once(eng, chans, x, int(FS * 0.010)), a.repeats)
        same = np.concatenate(parts).tobytes() == whole[0].tobytes()
        r["feed_10ms"] = dict(run_s=dt_run, feed_s=dt_feed, feed_over_run=dt_feed / dt_run, identical=bool(same))
        res[name] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
