#!/usr/bin/env python3
"""Rates of the level control and requantiser (gnss_dsp_tools_amd/requant.py, gacq_requant_run_dev) on one GPU.

Kernel time of one call (HIP events, median of --reps after --warmup calls; a call is two launches) and input GB/s on a recording of
2^26 I/Q samples resident in HBM: int8 input to s8, 2sm and 4ob, int16 input to 2sm, with the default block, window and tables.  Beside
it, from the same run, the fill and read rates Engine.stream_probe reports (the stage reads its input twice and writes at most as much
as it reads: the read rate is the ceiling to compare with) and the same definition written in torch operations on the device (checked
here to give the same bytes), with the shader clock sampled meanwhile (bench.ClockSampler).

usage: tools/bench_requant.py [--samples 67108864] [--reps 30] [--warmup 5] [--block 4096] [--window 8]
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
from gnss_dsp_tools_amd import acquire, requant  # noqa: E402

CASES = (("s8", 8), ("2sm", 8), ("4ob", 8), ("2sm", 16))


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


def torch_requant(torch, x, fmt, G, T, Lb, W):
    """the definition of include/gacq.h in torch operations, for a recording of whole blocks: the output's bytes as a uint8 tensor"""
    dev = x.device
    nb = x.numel() // (2 * Lb)
    P = (x.view(nb, 2 * Lb).to(torch.int64) ** 2).sum(dim=1)
    c = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), P.cumsum(0)])
    b = torch.arange(nb, device=dev)
    S = torch.where(b < W, c[W], c[b] - c[torch.clamp(b - W, min=0)])
    Tt = torch.from_numpy(np.minimum(T, np.uint64((1 << 63) - 1)).astype(np.int64)).to(dev)
    k = torch.searchsorted(Tt, S, right=False)                               # the thresholds below the level
    g = torch.from_numpy(G).to(dev)[k].repeat_interleave(2 * Lb)
    v = x.to(torch.float32) * g
    if fmt.container == requant.S8:
        return torch.clamp(torch.round(v), -127, 127).to(torch.int8).view(torch.uint8)
    n = 1 << fmt.bits
    q = torch.clamp(torch.floor(v * 0.5) + n // 2, 0, n - 1).to(torch.int64)
    code = torch.tensor(fmt.enc, dtype=torch.uint8, device=dev)[q]
    per = 8 // fmt.bits
    shifts = torch.tensor([(8 - fmt.bits * (i + 1)) if fmt.msb_first else fmt.bits * i for i in range(per)], dtype=torch.uint8, device=dev)
    return torch.bitwise_left_shift(code.view(-1, per), shifts[None, :]).sum(dim=1, dtype=torch.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1 << 26)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--block", type=int, default=requant.BLOCK)
    ap.add_argument("--window", type=int, default=requant.WINDOW)
    a = ap.parse_args()
    torch = nat.require_torch()
    eng = acquire.Engine(0)
    dev = "cuda:0"
    fill, read = eng.stream_probe("fill"), eng.stream_probe("read")
    print("stream probe: fill %.0f GB/s, read %.0f GB/s" % (fill, read))
    g = torch.Generator(device=dev)
    g.manual_seed(20261019)
    z = torch.randn(2 * a.samples, generator=g, device=dev, dtype=torch.float32)
    z[a.samples:] *= 0.125                                                    # the second half eight times weaker
    x8 = torch.clamp(torch.round(12.0 * z), -127, 127).to(torch.int8)
    x16 = torch.clamp(torch.round(3000.0 * z), -32767, 32767).to(torch.int16)
    del z
    rows = []
    for name, in_bits in CASES:
        fmt = requant.OutFormat(name)
        G, T = requant.tables(fmt.target_rms, a.block, a.window)
        x = x8 if in_bits == 8 else x16
        d = x.view(torch.uint8)
        with requant.Requantizer(eng, fmt, G, T, a.block, a.window, in_bits) as rq:
            sampler = bench.ClockSampler(0).start()
            ms, ms_min = timed(torch, lambda: rq.run(d, 0, 0, a.samples), a.reps, a.warmup)
            clk = sampler.stop()
            out = rq.run(d, 0, 0, a.samples)
        ref = torch_requant(torch, x, fmt, G, T, a.block, a.window)
        same = bool(torch.equal(out.view(torch.uint8), ref))
        del ref
        t_ms, t_min = timed(torch, lambda: torch_requant(torch, x, fmt, G, T, a.block, a.window), max(3, a.reps // 6), 1)
        in_bytes = 2.0 * a.samples * in_bits / 8
        gbs = in_bytes / ms * 1e-6
        row = dict(format=name, in_bits=in_bits, samples=a.samples, block=a.block, window=a.window, ms=ms, ms_min=ms_min, in_gbs=gbs, of_read=gbs / read,
                   of_fill=gbs / fill, gsamples_per_s=a.samples / ms * 1e-6, torch_ms=t_ms, torch_in_gbs=in_bytes / t_ms * 1e-6, over_torch=t_ms / ms,
                   same_bytes_as_torch=same, sclk_mhz_mean=clk.get("sclk_mhz_mean"))
        rows.append(row)
        print("int%-2d -> %-3s  %7.3f ms (min %.3f)  %7.1f GB/s in = %4.1f %% of read, %4.1f %% of fill  %5.1f Gsample/s | torch %8.3f ms %6.1f GB/s: x%.1f, "
              "bytes %s | sclk %s MHz" % (in_bits, name, ms, ms_min, gbs, 100.0 * gbs / read, 100.0 * gbs / fill, row["gsamples_per_s"], t_ms,
                                           row["torch_in_gbs"], t_ms / ms, "equal" if same else "DIFFER", clk.get("sclk_mhz_mean")))
    eng.close()
    print(json.dumps(dict(tool="bench_requant", fill_gbs=fill, read_gbs=read, rows=rows)))


if __name__ == "__main__":
    main()
