#!/usr/bin/env python3
"""Cost of the chip accumulator (chiptrack.ChipTrackLoop) at 69.984 MS/s on a resident int8 recording of random samples shared by every
channel (B2I codes, PRNs 19.. in turn).  For each K (default 1, 32 and 256 channels), runs over the same recording with
  - accumulation on  (accum_after = -1: every frame is folded into the bins);
  - accumulation off (accum_after past the recording: the template loop alone, in the same kernel).
Only run() is timed: the loop is opened before the clock starts and closed after it stops, so the timed region is run()'s two
launches (one that tracks every block, one that finds nothing left) with their state and record copies.  Reports that wall time per
1 ms block (per launch, all K channels in parallel) and per block per channel (divided by K), ms of signal per second, and the on/off
ratio.  The kernel's own time comes from a run under `rocprofv3 --kernel-trace` (tools/kernel_trace_us.py).  Prints one JSON line.
usage: tools/bench_chiptrack.py [--ks 1,32,256] [--modes on,off] [--seconds 0.2] [--repeats 3]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gnss_dsp_tools_amd import acquire, chiptrack, trackloop  # noqa: E402

FS = 69.984e6
PRNS = [19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 32, 33, 34, 35, 36, 37, 38, 39, 40, 41, 42, 43, 44, 45, 46, 47, 48]


def channels(K):
    return [trackloop.Channel("beidou-b2bi", FS, 0.0, PRNS[k % len(PRNS)], 0.0, 10230 - 100.5 - k % 1000, (500.0, 500.0))
            for k in range(K)]


def timed_run(eng, chans, x, accum_after, repeats):
    """best wall time of run() over `repeats` fresh loops (open and close outside the clock), and the last run's records"""
    torch = chiptrack.nat.require_torch()
    best, recs = None, None
    for _ in range(repeats):
        tl = chiptrack.ChipTrackLoop(chans, eng, max_records=1000, accum_after=accum_after)
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            recs = tl.run([x] * len(chans))
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        finally:
            tl.close()
        best = dt if best is None else min(best, dt)
    return best, recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="1,32,256")
    ap.add_argument("--modes", default="on,off")
    ap.add_argument("--seconds", type=float, default=0.2)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    torch = chiptrack.nat.require_torch()
    eng = acquire.default_engine()
    n = int(FS * a.seconds)
    g = torch.Generator(device="cuda:%d" % eng.device)
    g.manual_seed(11)
    x = torch.randint(-20, 21, (2 * n,), dtype=torch.int8, device="cuda:%d" % eng.device, generator=g)
    res = {"fs": FS, "seconds": a.seconds, "K": []}
    modes = {"on": -1, "off": 1 << 40}
    for K in [int(k) for k in a.ks.split(",")]:
        chans = channels(K)
        row = {"K": K}
        for label in a.modes.split(","):
            timed_run(eng, chans, x, modes[label], 1)                  # chips uploaded, code objects loaded
            dt, recs = timed_run(eng, chans, x, modes[label], a.repeats)
            ms = float(len(recs[0]))
            row[label] = dict(ms_signal=ms, wall_s=dt, wall_us_per_block=1e6 * dt / ms, wall_us_per_block_per_channel=1e6 * dt / (ms * K),
                              ms_per_s_per_channel=ms / dt, ms_per_s_aggregate=K * ms / dt)
        if "on" in row and "off" in row:
            row["wall_on_over_off"] = row["on"]["wall_s"] / row["off"]["wall_s"]
        res["K"].append(row)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
