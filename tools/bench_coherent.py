#!/usr/bin/env python3
"""Times of the coherent search (gnss_dsp_tools_amd/coherent.py) on one GPU: HIP events, median of 20 after warm-up, inputs resident
in HBM.  For galileo-e1c (M = 25, the 25 phases of CS25, 41 Doppler values 10 Hz apart) and gps-l1 (M = 20, data_flip: 20 patterns,
41 Doppler values 25 Hz apart):

  (a) the fold alone: gacq_fold_dev against the same fold written with torch on the device -- gather of the M windows, complex
      multiply by the rotation (phase in fp64, as exact as torch gets it), einsum with W -- which is what the package could do before
      the kernel existed;
  (b) coherent.search end to end, and the same search with the torch fold in the kernel's place; the fold's share of (b).
The torch fold ends in .contiguous(): [D, H, n_out] rows are what the search takes and what the kernel writes.

usage: tools/bench_coherent.py [--items 1,2,3,4] [--reps 20] [--warmup 3]      prints one line per figure and a JSON summary line."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gnss_dsp_tools_amd import acquire, coherent, signals  # noqa: E402

CASES = (("galileo-e1c", 25, "builtin", False, 10.0), ("gps-l1", 20, None, True, 25.0))
D = 41


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


def torch_fold(torch, x_dev, n_out, st, f, fs, W):
    """y[d,h,i] = sum_m W[h,m] x[st[d,m] + i] exp(-2 pi i frac(f_d (st[d,m] + i) / fs)) with torch operations"""
    dev = x_dev.device
    idx = torch.from_numpy(st).to(dev)[:, :, None] + torch.arange(n_out, device=dev)[None, None, :]
    ph = torch.remainder(idx.to(torch.float64) * (torch.from_numpy(f).to(dev) / fs)[:, None, None], 1.0) * (-2.0 * np.pi)
    rot = torch.complex(torch.cos(ph).to(torch.float32), torch.sin(ph).to(torch.float32))
    v = x_dev[idx] * rot
    return torch.einsum("hm,dmn->dhn", torch.from_numpy(W.astype(np.float32)).to(dev).to(torch.complex64), v).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", default="1,2,3,4")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch
    items = acquire.parse_list_ranges(a.items)
    eng = acquire.Engine(0)
    summary = {}
    try:
        for name, M, secondary, flip, df in CASES:
            sig = signals.get(name)
            sec = coherent.builtin_secondary(sig) if secondary == "builtin" else secondary
            W, labels = coherent.patterns(sec, M, flip)
            f = (np.arange(D) - D // 2) * df + 1000.0
            st = coherent.starts(sig, f, M)
            n_out = sig.samples_needed(1)
            nsamp = int(st.max()) + n_out
            rng = np.random.Generator(np.random.PCG64(7))
            x = (rng.standard_normal(nsamp) + 1j * rng.standard_normal(nsamp)).astype(np.complex64)
            x_dev = torch.from_numpy(x).to("cuda:0")
            H = len(W)
            y = coherent.fold_dev(x_dev, n_out, st, f, sig.fs, W, 0, eng)
            yt = torch_fold(torch, x_dev, n_out, st, f, sig.fs, W)
            dev = float((y - yt).abs().max() / yt.abs().max())
            del yt
            k_ms, k_min = timed(torch, lambda: coherent.fold_dev(x_dev, n_out, st, f, sig.fs, W, 0, eng), a.reps, a.warmup)
            t_ms, t_min = timed(torch, lambda: torch_fold(torch, x_dev, n_out, st, f, sig.fs, W), a.reps, a.warmup)

            def search_torch():
                yy = torch_fold(torch, x_dev, n_out, st, f, sig.fs, W)
                return eng.search_batch_dev(sig, yy.view(D * H, n_out), items, [0.0], 1).cpu()

            s_ms, s_min = timed(torch, lambda: coherent.search(sig, x_dev, items, f, M, sec, flip, engine=eng), a.reps, a.warmup)
            st_ms, st_min = timed(torch, search_torch, a.reps, a.warmup)
            out_gb = D * H * n_out * 8 / 1e9
            print("%s M %d H %d D %d n_out %d items %d: y %.3f GB, kernel vs torch fold differ by %.2g of max |y|" % (name, M, H, D, n_out, len(items), out_gb, dev))
            print("  (a) fold   kernel %8.3f ms (min %.3f)  torch %8.3f ms (min %.3f)  ratio %.1f  kernel writes y at %.0f GB/s"
                  % (k_ms, k_min, t_ms, t_min, t_ms / k_ms, out_gb / (k_ms * 1e-3)))
            print("  (b) search kernel fold %8.3f ms (min %.3f)  torch fold %8.3f ms (min %.3f)  fold share of the search %.1f %%"
                  % (s_ms, s_min, st_ms, st_min, 100.0 * k_ms / s_ms))
            summary[name] = dict(M=M, H=H, D=D, n_out=n_out, items=len(items), fold_kernel_ms=k_ms, fold_torch_ms=t_ms, search_ms=s_ms,
                                 search_torch_fold_ms=st_ms, fold_share=k_ms / s_ms, kernel_vs_torch=dev)
    finally:
        eng.close()
    print(json.dumps({"bench_coherent": summary}))


if __name__ == "__main__":
    main()
