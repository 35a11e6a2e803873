#!/usr/bin/env python3
"""Rates of the recording scan (gnss_dsp_tools_amd/scan.py) on one GPU: HIP events, median of 20 after three warm-ups, the recording
(random int8) resident in HBM, back-to-back windows.  gps-l1 --time 1 at 69.984 MS/s with E = 64 and 1024 windows, galileo-e1b --time 8
with E = 16, default item lists and Doppler grids.  Timed in the same process:

  batched   gacq_frontend_batch_dev for all E windows; gacq_search_batch_dev with nepoch = E; gacq_scan_int8_dev (both, end to end)
  loop      what there was before: Engine.frontend_dev, then search_batch_dev with nepoch = 1, per window

and reported per window, with windows/s, the multiple of real time (a window advances the recording by --time + 5 ms) and the bytes
the batched front-end moves per window -- int8 in, y1 out and in again (all of it: the fused kernel's tiles cover every sample),
complex64 out -- against 8 TB/s.

usage: tools/bench_scan.py [--reps 20] [--loop-reps 20] [--warmup 3] [--cases gps-l1:1:64,gps-l1:1:1024,galileo-e1b:8:16]
prints one line per figure and a JSON summary line."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gnss_dsp_tools_amd import acquire, codes, scan, signals  # noqa: E402

FS = 69.984e6
COFFSET = 250000.0
HBM_BYTES_PER_S = 8.0e12


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
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--loop-reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cases", default="gps-l1:1:64,gps-l1:1:1024,galileo-e1b:8:16")
    a = ap.parse_args()
    import torch
    eng = acquire.Engine(0)
    dev = torch.device("cuda", 0)
    summary = {}
    try:
        for case in a.cases.split(","):
            name, ms, E = case.split(":")
            ms, E = int(ms), int(E)
            sig = signals.get(name)
            items = acquire.parse_list_ranges(sig.default_items, sep=sig.item_sep) if sig.default_items else codes.prns(sig.code)
            dop = acquire.doppler_grid(sig.default_doppler)
            blocks = max(sig.blocks(ms), 0)
            ms_pad = ms + 5
            n_in = int(FS * 0.001 * ms_pad)
            n_out = ms_pad * int(round(sig.fs * 0.001))
            starts = scan.window_starts(FS, float(ms_pad), n_in * E, n_in)
            assert len(starts) == E
            rec = torch.randint(-128, 128, (2 * n_in * E,), dtype=torch.int8, device=dev)
            x = torch.empty((E, n_out), dtype=torch.complex64, device=dev)
            peaks = torch.empty((E, len(items), 2), dtype=torch.float64, device=dev)
            peak1 = torch.empty((1, len(items), 2), dtype=torch.float64, device=dev)

            def fe_batched():
                eng.frontend_batch_dev(sig, rec, starts, n_in, FS, COFFSET, ms_pad, out=x)

            def fe_loop():
                for s in starts:
                    eng.frontend_dev(sig, rec[2 * s:2 * (s + n_in)], FS, COFFSET, ms_pad)

            def search_batched():
                eng.search_batch_dev(sig, x, items, dop, blocks, out=peaks)

            def search_loop():
                for e in range(E):
                    eng.search_batch_dev(sig, x[e:e + 1], items, dop, blocks, out=peak1)

            def scan_batched():
                eng.scan_int8_dev(sig, rec, starts, n_in, FS, COFFSET, ms_pad, items, dop, blocks, out=peaks)

            def scan_loop():
                for s in starts:
                    eng.search_batch_dev(sig, eng.frontend_dev(sig, rec[2 * s:2 * (s + n_in)], FS, COFFSET, ms_pad).view(1, -1), items, dop, blocks, out=peak1)

            r = {}
            for key, fn, reps in (("fe_batched", fe_batched, a.reps), ("fe_loop", fe_loop, a.loop_reps), ("search_batched", search_batched, a.reps),
                                  ("search_loop", search_loop, a.loop_reps), ("scan_batched", scan_batched, a.reps), ("scan_loop", scan_loop, a.loop_reps)):
                r[key + "_ms_per_window"] = timed(torch, fn, reps, a.warmup) / E
            fe_bytes = 2 * n_in + 2 * 8 * (n_in + 6 * 161) + 8 * n_out
            for path in ("batched", "loop"):
                w = 1e3 / r["scan_%s_ms_per_window" % path]
                r["%s_windows_per_s" % path], r["%s_x_realtime" % path] = w, w * ms_pad * 1e-3
            r["fe_bytes_per_window"] = fe_bytes
            r["fe_batched_fraction_of_8TBps"] = fe_bytes / (r["fe_batched_ms_per_window"] * 1e-3) / HBM_BYTES_PER_S
            print("%-12s --time %d E %4d (%d items x %d bins, n_in %d): per window  front-end %.4f ms batched / %.4f ms loop (%.2f x) | "
                  "search %.4f / %.4f ms (%.2f x) | scan %.4f / %.4f ms (%.2f x) = %.0f / %.0f windows/s = %.1f / %.1f x real time | "
                  "batched front-end moves %.2f MB per window: %.0f GB/s, %.1f %% of 8 TB/s"
                  % (name, ms, E, len(items), len(dop), n_in, r["fe_batched_ms_per_window"], r["fe_loop_ms_per_window"],
                     r["fe_loop_ms_per_window"] / r["fe_batched_ms_per_window"], r["search_batched_ms_per_window"], r["search_loop_ms_per_window"],
                     r["search_loop_ms_per_window"] / r["search_batched_ms_per_window"], r["scan_batched_ms_per_window"], r["scan_loop_ms_per_window"],
                     r["scan_loop_ms_per_window"] / r["scan_batched_ms_per_window"], r["batched_windows_per_s"], r["loop_windows_per_s"],
                     r["batched_x_realtime"], r["loop_x_realtime"], fe_bytes / 1e6, fe_bytes / (r["fe_batched_ms_per_window"] * 1e-3) / 1e9,
                     100 * r["fe_batched_fraction_of_8TBps"]), flush=True)
            summary["%s_time%d_E%d" % (name, ms, E)] = r
            del rec, x, peaks
    finally:
        eng.close()
    print(json.dumps({"bench_scan": summary}))


if __name__ == "__main__":
    main()
