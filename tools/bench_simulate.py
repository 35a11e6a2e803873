#!/usr/bin/env python3
"""Rates of the recording synthesis (gnss_dsp_tools_amd/simulate.py) on one GPU: HIP events, median of 20 after three warm-ups, output
resident in HBM.  Scenes of K = 1, 12 and 32 GPS L1 C/A satellites (20 ms data bits, spread Dopplers and code phases) at 69.984 MS/s,
int8 and complex64 output, against two baselines timed in the same run:

  (a) the same formula with torch operations on the device -- torch.randn noise, the code position in fp64, a gather from the chip
      table, the carrier phase in wrapping int64, cos / sin in fp64 -- which is what the package could do without the kernel.  It
      leaves out the data bits, so it is favoured if anything;
  (b) tests/handoff_cases.py:recording on the host (numpy, one core), on a shorter stretch.

usage: tools/bench_simulate.py [--n 16777216] [--n-torch 4194304] [--n-host 524288] [--reps 20] [--warmup 3]
prints one line per figure and a JSON summary line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from gnss_dsp_tools_amd import acquire, codes, simulate, trackloop  # noqa: E402

FS = 69.984e6
COFFSET = 250000.0
SIGMA = 12.0


def timed(torch, fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms))


def scene(K):
    rng = np.random.Generator(np.random.PCG64(K))
    return [simulate.Satellite("gps-l1", k + 1, 3.0, float(rng.uniform(-5000, 5000)), float(rng.uniform(0, 1023)),
                               symbols=simulate.symbols("gps-l1", k + 1, 64, 20, 1000 + k)) for k in range(K)]


def torch_scene(torch, sats, dev):
    """per satellite: (chip table as +-1 float32 on the device, L, carrier step as a wrapping int64, chips per sample, code0, amp)"""
    out = []
    t = trackloop.TRACKERS["gps-l1"]
    for s in sats:
        c = codes.chips(t.code, s.item)
        F = int(np.floor(np.ldexp((s.carrier_hz(COFFSET) / FS) % 1.0, 64)))
        out.append((torch.from_numpy(1.0 - 2.0 * c.astype(np.float32)).to(dev), len(c), F - (1 << 64) if F >= (1 << 63) else F,
                    s.code_rate_hz() / FS, s.code0, s.amp))
    return out


def torch_recording(torch, ts, n, dtype, dev):
    j = torch.arange(n, device=dev, dtype=torch.float64)
    ji = torch.arange(n, device=dev, dtype=torch.int64)
    x = torch.randn(n, 2, device=dev, dtype=torch.float32) * SIGMA
    re, im = x[:, 0], x[:, 1]
    for chips, L, F, cf, code0, amp in ts:
        idx = torch.remainder(torch.floor(code0 + cf * j), L).to(torch.int64)
        a = chips[idx] * amp
        ang = (ji * F).to(torch.float64) * (2.0 * np.pi / 2.0 ** 64)
        re = re + a * torch.cos(ang).to(torch.float32)
        im = im + a * torch.sin(ang).to(torch.float32)
    if dtype == "complex64":
        return torch.complex(re, im)
    return torch.stack((re, im), dim=1).round().clamp(-127, 127).to(torch.int8).view(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 24)
    ap.add_argument("--n-torch", type=int, default=1 << 22)
    ap.add_argument("--n-host", type=int, default=1 << 19)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch
    import handoff_cases
    eng = acquire.Engine(0)
    dev = torch.device("cuda", 0)
    summary = {}
    try:
        for K in (1, 12, 32):
            sats = scene(K)
            ts = torch_scene(torch, sats, dev)
            host_sats = [dict(tracker=s.tracker, item=s.item, amp=s.amp, doppler=s.doppler, code0=s.code0, bit=20) for s in sats]
            t0 = time.perf_counter()
            handoff_cases.recording(7, FS, a.n_host, COFFSET, host_sats, SIGMA)
            host_rate = a.n_host / (time.perf_counter() - t0)
            print("K %2d  host numpy (tests/handoff_cases.recording, %d samples): %.3g samples/s = %.4f x real time" % (K, a.n_host, host_rate, host_rate / FS))
            for dtype in ("int8", "complex64"):
                out = simulate.recording(sats, FS, COFFSET, a.n, 7, SIGMA, dtype=dtype, engine=eng)
                k_ms, k_min = timed(torch, lambda: simulate.recording(sats, FS, COFFSET, a.n, 7, SIGMA, dtype=dtype, engine=eng, out=out), a.reps, a.warmup)
                t_ms, t_min = timed(torch, lambda: torch_recording(torch, ts, a.n_torch, dtype, dev), a.reps, a.warmup)
                k_rate, t_rate = a.n / (k_ms * 1e-3), a.n_torch / (t_ms * 1e-3)
                gbs = out.numel() * out.element_size() / (k_ms * 1e-3) / 1e9
                print("K %2d %-9s kernel %8.3f ms (min %.3f) for %d samples: %.3g samples/s = %7.1f x real time, writes %.0f GB/s | "
                      "torch %8.3f ms (min %.3f) for %d: %.3g samples/s = %.2f x real time | kernel / torch %.1f, kernel / host %.0f"
                      % (K, dtype, k_ms, k_min, a.n, k_rate, k_rate / FS, gbs, t_ms, t_min, a.n_torch, t_rate, t_rate / FS, k_rate / t_rate, k_rate / host_rate))
                summary["K%d_%s" % (K, dtype)] = dict(kernel_ms=k_ms, kernel_min_ms=k_min, n=a.n, kernel_samples_per_s=k_rate, kernel_x_realtime=k_rate / FS,
                                                      torch_ms=t_ms, n_torch=a.n_torch, torch_samples_per_s=t_rate, host_samples_per_s=host_rate,
                                                      kernel_over_torch=k_rate / t_rate, kernel_over_host=k_rate / host_rate)
    finally:
        eng.close()
    print(json.dumps({"bench_simulate": summary}))


if __name__ == "__main__":
    main()
