#!/usr/bin/env python3
"""Rates of the down-converter (gnss_dsp_tools_amd/ddc.py, gacq_ddc_run_dev) on one GPU, and what it buys the tracking loop.

1. Kernel time (HIP events, median of --reps after --warmup calls) and input GB/s for D = 4, 16 and 64 with the default taps, int8 out,
   on a recording of 2^26 int8 I/Q samples resident in HBM, beside the fill and read rates Engine.stream_probe reports in the same run,
   with the shader clock sampled meanwhile (bench.ClockSampler).
2. The tracking loop of one GPS L1 C/A channel (trackloop.TrackLoop, K = 1) on a 65.472 MS/s recording and on that recording after
   D = 16: wall time of run() per 1 ms block, best of three fresh loops, the method of tools/bench_track_loop.py.

usage: tools/bench_ddc.py [--samples 67108864] [--reps 30] [--warmup 5] [--seconds 0.3] [--decims 4,16,64]
prints one line per case and a JSON summary line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from gnss_dsp_tools_amd import _native as nat  # noqa: E402
from gnss_dsp_tools_amd import acquire, ddc, simulate, trackloop  # noqa: E402

FS_WIDE, D_TRACK = 65.472e6, 16


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


def track_ms_per_block(eng, x, fs, coffset, doppler, code0):
    torch = nat.require_torch()
    chans = [trackloop.Channel("gps-l1", fs, coffset, 7, doppler, code0, (20.0, 40.0))]
    best, recs = None, None
    for _ in range(3):
        tl = trackloop.TrackLoop(chans, eng, max_records=100)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        recs = tl.run([x])
        dt = time.perf_counter() - t0
        tl.close()
        best = dt if best is None else min(best, dt)
    return 1e3 * best / len(recs[0]), len(recs[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1 << 26)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.3)
    ap.add_argument("--decims", default="4,16,64")
    a = ap.parse_args()
    torch = nat.require_torch()
    eng = acquire.Engine(0)
    dev = "cuda:0"
    fill, read = eng.stream_probe("fill"), eng.stream_probe("read")
    print("stream probe: fill %.0f GB/s, read %.0f GB/s" % (fill, read))
    g = torch.Generator(device=dev)
    g.manual_seed(20261019)
    x = torch.clamp(torch.round(12.0 * torch.randn(2 * a.samples, generator=g, device=dev, dtype=torch.float32)), -127, 127).to(torch.int8)
    rows = []
    for D in [int(v) for v in a.decims.split(",")]:
        band = ddc.Band(FS_WIDE / 8.0 + 1234.5, D)
        n_out = band.out_range(0, a.samples)[1]
        with ddc.Converter(eng, band, FS_WIDE) as conv:
            d = x.view(torch.uint8)
            sampler = bench.ClockSampler(0).start()
            ms, ms_min = timed(torch, lambda: conv.run(d, 0, 0, n_out, 1.0, "int8"), a.reps, a.warmup)
            clk = sampler.stop()
        gbs = 2.0 * a.samples / ms * 1e-6
        row = dict(D=D, taps=band.T, samples_in=a.samples, samples_out=n_out, ms=ms, ms_min=ms_min, in_gbs=gbs, of_read=gbs / read, of_fill=gbs / fill,
                   gsamples_per_s=a.samples / ms * 1e-6, sclk_mhz_mean=clk.get("sclk_mhz_mean"))
        rows.append(row)
        print("D %2d T %3d  %8.3f ms (min %.3f)  %7.1f GB/s in = %4.1f %% of read, %4.1f %% of fill  %6.1f Gsample/s  sclk %s MHz"
              % (D, band.T, ms, ms_min, gbs, 100.0 * gbs / read, 100.0 * gbs / fill, row["gsamples_per_s"], clk.get("sclk_mhz_mean")))
    del x
    # tracking: one GPS L1 channel on the wide recording and on its D = 16 band
    n = int(FS_WIDE * (a.seconds + 0.002))
    sats = [simulate.Satellite("gps-l1", 7, 3.0, 1234.5, 417.3)]
    wide = simulate.recording(sats, FS_WIDE, 0.0, n, 31, 12.0, dtype="int8", engine=eng)
    band = ddc.Band(0.0, D_TRACK)
    gain = ddc.auto_gain(eng, band, FS_WIDE, wide[:2 * ddc.auto_window(band)])
    narrow = ddc.convert(eng, band, FS_WIDE, wide, gain)
    torch.cuda.synchronize()
    wide_ms, wide_n = track_ms_per_block(eng, wide, FS_WIDE, 0.0, 1234.5, 417.3)
    narrow_ms, narrow_n = track_ms_per_block(eng, narrow, FS_WIDE / D_TRACK, 0.0, 1234.5, 417.3)
    track = dict(fs_wide=FS_WIDE, D=D_TRACK, wide_ms_per_block=wide_ms, wide_blocks=wide_n, narrow_ms_per_block=narrow_ms, narrow_blocks=narrow_n,
                 ratio=wide_ms / narrow_ms)
    print("tracking, one GPS L1 channel: %.1f us per 1 ms block at %.3f MS/s (%d blocks), %.1f us at %.3f MS/s after D = %d (%d blocks): x%.2f"
          % (1e3 * wide_ms, FS_WIDE * 1e-6, wide_n, 1e3 * narrow_ms, FS_WIDE / D_TRACK * 1e-6, D_TRACK, narrow_n, wide_ms / narrow_ms))
    eng.close()
    print(json.dumps(dict(tool="bench_ddc", fill_gbs=fill, read_gbs=read, rows=rows, track=track)))


if __name__ == "__main__":
    main()
