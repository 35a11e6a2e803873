#!/usr/bin/env python3
"""Rates of the cancellation of tracked signals (gnss_dsp_tools_amd/cancel.py, gacq_cancel_dev) on one GPU.

A recording of --samples int8 I/Q samples resident in HBM, GPS L1 C/A satellites with back-to-back 1 ms segments (4092 samples at
4.092 MHz), int8 in and int8 out.  A call converts and uploads its segments, launches and waits, so the time of a call (HIP events
around it, median of --reps after --warmup) holds host work that grows with the segment count.  The kernels' times are therefore
differences of calls that do the same host work: per K in 1, 4, 8, 32, cancel_subtract_kernel = a call over all samples minus a call
with the same segments over the first 2048 samples, both with given amplitudes, as samples/s, satellite-samples/s and bytes/s in + out;
cancel_project_kernel = what the call over all samples takes longer with estimate on, as segments/s.  (A kernel trace of the same
program gives the kernels' own times to hold these against.)  Beside it, from the same process: the
copy rate Engine.stream_probe reports (the subtraction reads and writes every byte once: that is its ceiling) and the same subtraction
written in torch operations (fp64 phases, chips gathered from a table, complex64 rotation; checked here against the kernel's bytes), with
the shader clock sampled meanwhile (bench.ClockSampler).

usage: tools/bench_cancel.py [--samples 16777216] [--reps 20] [--warmup 3]
prints one line per case and a JSON summary line."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from gnss_dsp_tools_amd import _native as nat  # noqa: E402
from gnss_dsp_tools_amd import acquire, cancel, codes  # noqa: E402

FS, SEG = 4.092e6, 4092
KS = (1, 4, 8, 32)


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


def scene(K, n):
    """K satellites, each with back-to-back 1 ms segments over n samples"""
    nseg = n // SEG
    sats, segs = [], []
    for k in range(K):
        g = np.zeros(nseg, dtype=cancel.SEG_DTYPE)
        dopp = -4000.0 + 250.0 * k
        rate = 1.023e6 + dopp / 1540.0
        g["s0"] = np.arange(nseg) * SEG
        g["n"] = SEG
        g["carrier_hz"] = dopp
        g["carrier_phase"] = (g["s0"] * (dopp / FS) + k / 32.0) % 1.0
        g["code_rate_hz"] = rate
        g["code_phase"] = (37.5 * k + g["s0"] * (rate / FS)) % 1023.0
        g["amp_re"], g["amp_im"] = 3.0 * np.cos(0.4 * k), 3.0 * np.sin(0.4 * k)
        sats.append(cancel.Sat("gps.ca", k + 1, 0))
        segs.append(g)
    return sats, segs


def torch_cancel(torch, x, sats, segs, chunk=1 << 22):
    """the same subtraction in torch operations: int8 in, int8 out; phases in fp64, the rotation and the subtraction in complex64"""
    dev = x.device
    n = x.numel() // 2
    out = torch.empty_like(x)
    tabs = [torch.from_numpy(1.0 - 2.0 * codes.chips(s.code, s.prn).astype(np.float32)).to(dev) for s in sats]
    par = [{k: torch.from_numpy(np.ascontiguousarray(g[k])).to(dev) for k in ("carrier_hz", "carrier_phase", "code_rate_hz", "code_phase", "amp_re", "amp_im")}
           for g in segs]
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        j = torch.arange(lo, hi, device=dev)
        q = torch.clamp(j // SEG, max=len(segs[0]) - 1)
        i = (j - q * SEG).to(torch.float64)
        live = (j // SEG) < len(segs[0])
        xi = x[2 * lo:2 * hi].view(-1, 2).to(torch.float32)
        v = torch.complex(xi[:, 0], xi[:, 1])
        for t, p in zip(tabs, par):
            ph = p["carrier_phase"][q] + i * (p["carrier_hz"][q] / FS)
            pos = p["code_phase"][q] + i * (p["code_rate_hz"][q] / FS)
            w = t[torch.floor(pos).to(torch.int64) % t.numel()]
            ang = (2.0 * np.pi) * (ph - torch.floor(ph))
            r = torch.complex((w * torch.cos(ang).to(torch.float32)), (w * torch.sin(ang).to(torch.float32)))
            a = torch.complex(p["amp_re"][q].to(torch.float32), p["amp_im"][q].to(torch.float32))
            v = v - torch.where(live, a * r, torch.zeros_like(r))
        o = torch.clamp(torch.round(torch.view_as_real(v)), -127, 127).to(torch.int8)
        out[2 * lo:2 * hi] = o.reshape(-1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1 << 24)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    torch = nat.require_torch()
    eng = acquire.Engine(0)
    dev = "cuda:0"
    copy = eng.stream_probe("copy")
    print("stream probe: copy %.0f GB/s (read + write bytes)" % copy)
    g = torch.Generator(device=dev)
    g.manual_seed(20261019)
    x = torch.clamp(torch.round(12.0 * torch.randn(2 * a.samples, generator=g, device=dev, dtype=torch.float32)), -127, 127).to(torch.int8)
    out = torch.empty_like(x)
    rows = []
    for K in KS:
        sats, segs = scene(K, a.samples)
        nseg = sum(len(s) for s in segs)
        sampler = bench.ClockSampler(0).start()
        call_ms, _ = timed(torch, lambda: cancel.apply(eng, sats, segs, FS, x, estimate=False, out=out), a.reps, a.warmup)
        clk = sampler.stop()
        small_ms, _ = timed(torch, lambda: cancel.apply(eng, sats, segs, FS, x, 0, 0, 2048, estimate=False, out=out[:4096]), a.reps, a.warmup)
        ms_est, _ = timed(torch, lambda: cancel.apply(eng, sats, segs, FS, x, estimate=True, out=out), a.reps, a.warmup)
        ms = max(call_ms - small_ms, 1e-6)
        got = cancel.apply(eng, sats, segs, FS, x, estimate=False)[0]
        ref = torch_cancel(torch, x, sats, segs)
        diff = (got.to(torch.int16) - ref.to(torch.int16)).abs()
        differ, worst = int((diff > 0).sum().item()), int(diff.max().item())
        del ref, diff
        t_ms, _ = timed(torch, lambda: torch_cancel(torch, x, sats, segs), 3, 1)
        gbs = 4.0 * a.samples / ms * 1e-6
        proj_ms = max(ms_est - call_ms, 0.0)
        row = dict(K=K, samples=a.samples, segments=nseg, call_ms=call_ms, call_small_ms=small_ms, ms=ms, gsamples_per_s=a.samples / ms * 1e-6,
                   gsatsamples_per_s=K * a.samples / ms * 1e-6, gbs=gbs, of_copy=gbs / copy, ms_with_estimate=ms_est, project_ms=proj_ms,
                   project_msegments_per_s=(nseg / proj_ms * 1e-3) if proj_ms > 0 else None,
                   project_gsamples_per_s=(K * a.samples / proj_ms * 1e-6) if proj_ms > 0 else None, torch_ms=t_ms, over_torch=t_ms / ms,
                   components_off_torch=differ, worst_off_torch=worst, sclk_mhz_mean=clk.get("sclk_mhz_mean"))
        rows.append(row)
        print("K %2d  call %8.3f ms, over 2048 samples %7.3f ms: subtract %8.3f ms  %6.2f Gsample/s  %6.2f Gsat-sample/s  %6.1f GB/s = %4.1f %% of copy | project %8.3f ms  %s Msegment/s | "
              "torch %9.3f ms: x%.1f, %d of %d components differ (by at most %d) | sclk %s MHz"
              % (K, call_ms, small_ms, ms, row["gsamples_per_s"], row["gsatsamples_per_s"], gbs, 100.0 * gbs / copy, proj_ms,
                 "%.2f" % row["project_msegments_per_s"] if proj_ms > 0 else "-", t_ms, t_ms / ms, differ, 2 * a.samples, worst, clk.get("sclk_mhz_mean")))
    eng.close()
    print(json.dumps(dict(tool="bench_cancel", copy_gbs=copy, fs=FS, segment=SEG, rows=rows)))


if __name__ == "__main__":
    main()
