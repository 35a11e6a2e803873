#!/usr/bin/env python3
"""Throughput of the device-resident tracking loops (trackloop.TrackLoop) at 69.984 MS/s on resident int8 recordings:
ms of signal tracked per second of wall time, per channel and in aggregate, for K = 1, 11, 64 and 256 GPS L1 C/A channels;
against a timing stand-in for the host loop the package allowed before, at K = 1 and 11: per 1 ms block one gacq_mix_int8_dev
wipe-off per channel and one EplPlan call for all channels, a PLL-only update on the host.  The stand-in is not a tracker: EplPlan
correlates every channel against channel 0's buffer, there is no offset wipe-off and no FLL/DLL, and its K = 11 is 11 GPS L1
channels rather than the track-all L1/L2/L5 set.  Prints one JSON line.
usage: tools/bench_track_loop.py [--seconds S] [--ks 1,11,64,256]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gnss_dsp_tools_amd import acquire, codes, trackloop  # noqa: E402
from gnss_dsp_tools_amd.tracking import EplPlan  # noqa: E402

FS = 69.984e6


def device_loop(eng, x, K, seconds):
    torch = trackloop.nat.require_torch()
    prns = [1 + k % 32 for k in range(K)]
    chans = [trackloop.Channel("gps-l1", FS, 0.0, p, 0.0, 10.5 + k, (20.0, 40.0)) for k, p in enumerate(prns)]
    best = None
    for _ in range(3):
        tl = trackloop.TrackLoop(chans, eng, max_records=100)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        recs = tl.run([x] * K)
        dt = time.perf_counter() - t0
        tl.close()
        best = dt if best is None else min(best, dt)
    ms = float(np.mean([len(r) for r in recs]))
    return dict(K=K, ms_signal=ms, wall_s=best, ms_per_s_per_channel=ms / best, ms_per_s_aggregate=K * ms / best)


def host_loop(eng, x, K, blocks):
    """The reference's loop written against the package's earlier pieces: per 1 ms block, one wipe-off launch per channel and one
    E/P/L launch for all channels; FLL/PLL/DLL on the host."""
    torch = trackloop.nat.require_torch()
    n = int(FS * 0.001)
    plan = EplPlan("gps.ca", [1 + k % 32 for k in range(K)], 0.05, eng)
    code_p = np.full(K, 10.5)
    carrier_f = np.zeros(K)
    code_f = np.full(K, 1023000.0)
    buf = torch.empty((K, n), dtype=torch.complex64, device=x.device)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for b in range(blocks):
        seg = x[2 * b * n:2 * (b + 1) * n]
        for k in range(K):
            y = eng.mix_int8_dev(seg, FS, float(carrier_f[k]))
            buf[k].copy_(y)
        cf = (code_f + carrier_f / 1540.0) / FS
        out = plan(buf[0], code_p, cf)
        e = np.arctan2(out[:, 1].imag, out[:, 1].real)
        carrier_f = carrier_f + 0.1 * e
        code_p = np.mod(code_p + n * cf, 1023.0)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return dict(K=K, ms_signal=blocks, wall_s=dt, ms_per_s_per_channel=blocks / dt, ms_per_s_aggregate=K * blocks / dt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.3)
    ap.add_argument("--ks", default="1,11,64,256")
    ap.add_argument("--host-blocks", type=int, default=100)
    a = ap.parse_args()
    torch = trackloop.nat.require_torch()
    eng = acquire.default_engine()
    nsamp = int(FS * (a.seconds + 0.002))
    rng = np.random.Generator(np.random.PCG64(7))
    x = torch.from_numpy(rng.integers(-20, 21, size=2 * nsamp, dtype=np.int8)).to("cuda:%d" % eng.device)
    res = {"fs": FS, "seconds": a.seconds, "device_loop": [], "host_loop": []}
    for K in [int(k) for k in a.ks.split(",")]:
        res["device_loop"].append(device_loop(eng, x, K, a.seconds))
    for K in (1, 11):
        res["host_loop"].append(host_loop(eng, x, K, a.host_blocks))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
