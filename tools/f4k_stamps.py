#!/usr/bin/env python3
"""Where the workgroups of one headline-shape launch of lds_fused4k_kernel run, and when: per compute unit, how long the prologue
(kernel entry to the first row) is, how much of it co-resident workgroups spend in their prologues together, how evenly the
workgroups' lifetimes and the compute units' finishing times come out, and which block indices share a compute unit.

Needs the stamp variant of the library (the product library has no stamps):

    tools/build_variant.sh stamps -DGACQ_F4K_STAMPS gnss-dsp-tools_amd/csrc/gacq_ldsfft.hip
    tools/variant.py stamps tools/f4k_stamps.py [f4k_run | claim ...]          (default: 1 10 40 claim)

A number is a run length of the static map (option f4k_run, with f4k_claim = 0); `claim` is claimed work (f4k_claim = 1).

Clock: the 100 MHz wall clock (10 ns a tick).  HW_ID (gfx9): cu_id [11:8], sh_id [12], se_id [15:13]; XCC_ID: xcc_id [3:0]."""
import ctypes
import os
import sys
from collections import defaultdict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from gnss_dsp_tools_amd import _native as nat
from gnss_dsp_tools_amd import acquire, signals, synth

TICK_US = 0.01
E, NBINS, NITEMS = 1024, 40, 32


def overlap_fraction(intervals):
    """Of the summed length of the intervals, the part during which at least one other interval of the list is open."""
    ev = sorted([(a, 1) for a, b in intervals] + [(b, -1) for a, b in intervals])
    open_now, last, shared = 0, 0, 0.0
    for t, k in ev:
        if open_now >= 2:
            shared += (t - last) * open_now
        open_now += k
        last = t
    total = float(sum(b - a for a, b in intervals))
    return shared / total if total else 0.0


def report(run, st, grid):
    st = st[:grid]
    live = st[:, 0] != 0
    t0, t1, t2 = (st[live, k].astype(np.int64) for k in range(3))
    hw, xcc = st[live, 3] & 0xffffffff, (st[live, 3] >> 32) & 15
    cu = (xcc << 8) | (((hw >> 13) & 7) << 5) | (((hw >> 12) & 1) << 4) | ((hw >> 8) & 15)
    blocks = np.nonzero(live)[0]
    start, end = t0.min(), t2.max()
    span = float(end - start)
    pro, life = (t1 - t0) * TICK_US, (t2 - t0) * TICK_US
    print("%s: %d workgroups on %d compute units, launch %.1f us" % ("claimed work" if run == "claim" else "f4k_run = %d" % run, live.sum(), len(np.unique(cu)), span * TICK_US))
    print("  prologue window (entry -> first row): median %.2f us, p10 %.2f, p90 %.2f, max %.2f; first round (entry within 5 us of the launch) median %.2f us"
          % (np.median(pro), np.percentile(pro, 10), np.percentile(pro, 90), pro.max(), np.median(pro[t0 - start < 500]) if np.any(t0 - start < 500) else float("nan")))
    print("  workgroup lifetime: median %.1f us, p1 %.1f, p99 %.1f; prologues are %.2f %% of the summed lifetimes" % (np.median(life), np.percentile(life, 1), np.percentile(life, 99), 100 * pro.sum() / life.sum()))
    by_cu = defaultdict(list)
    for k in range(len(cu)):
        by_cu[int(cu[k])].append(k)
    shared, busy, last_end, lock = [], [], [], []
    for c, ks in by_cu.items():
        ks = np.array(ks)
        shared.append(overlap_fraction([(int(t0[k]), int(t1[k])) for k in ks]))
        busy.append(float((t2[ks] - t0[ks]).sum()) / (4 * span))
        last_end.append(float(end - t2[ks].max()) / span)
        s = np.sort(t0[ks])
        lock.append(np.mean(np.diff(s) * TICK_US < np.median(pro)))        # starts that follow another start on the CU within one prologue window
    print("  per compute unit: prologue time spent while another workgroup of the CU is in its prologue: median %.1f %%, p90 %.1f %%, max %.1f %%"
          % (100 * np.median(shared), 100 * np.percentile(shared, 90), 100 * np.max(shared)))
    print("  per compute unit: workgroup starts within one prologue window of the previous start on that CU: median %.1f %%" % (100 * np.median(lock)))
    print("  per compute unit: resident-slot occupancy (summed lifetimes / 4 x launch): median %.1f %%, min %.1f %%; idle tail before the launch ends: median %.2f %%, max %.2f %%"
          % (100 * np.median(busy), 100 * np.min(busy), 100 * np.median(last_end), 100 * np.max(last_end)))
    per_x = [np.mean(life[xcc == x]) for x in range(8) if np.any(xcc == x)]
    per_x_end = [(t2[xcc == x].max() - start) * TICK_US for x in range(8) if np.any(xcc == x)]
    print("  per XCD: mean lifetime %s us; last workgroup ends at %s us" % (np.round(per_x, 1), np.round(per_x_end, 0)))
    print("  XCC_IDs seen per block %% 8: %s" % ", ".join("%d -> %s" % (k, sorted(set(int(v) for v in xcc[blocks % 8 == k]))) for k in range(8)))
    first = [c for c in sorted(by_cu)][:3]
    for c in first:
        ks = np.array(by_cu[c])
        ks = ks[np.argsort(t0[ks])][:8]
        print("  CU %#05x first workgroups (block, entry us): %s" % (c, ", ".join("%d @ %.1f" % (blocks[k], (t0[k] - start) * TICK_US) for k in ks)))
    sys.stdout.flush()


def main():
    runs = [a if a == "claim" else int(a) for a in sys.argv[1:]] or [1, 10, 40, "claim"]
    if not hasattr(nat.lib, "gacq_debug_f4k_stamps"):
        sys.exit("this library has no stamps: build the variant (see the module docstring) and run through tools/variant.py")
    nat.lib.gacq_debug_f4k_stamps.argtypes = [ctypes.c_void_p, ctypes.c_uint]
    sig = signals.get("gps-l1")
    items = list(range(1, NITEMS + 1))
    dop = acquire.doppler_grid([-5000.0, 5000.0, 250.0])[:NBINS]
    base = synth.make_epochs(sig, 1, 77, synth.default_sats(items), 8, nsamp=4096)
    xd = torch.from_numpy(np.concatenate([base] * (E // 8))).cuda()
    eng = acquire.Engine(0)
    eng.use_torch_stream()
    nblocks = 8 * ((E + 7) // 8) * NBINS
    stamps = torch.zeros((nblocks, 4), dtype=torch.int64, device="cuda")
    for run in runs:
        eng.set_option("f4k_run", 1 if run == "claim" else run)
        eng.set_option("f4k_claim", 1 if run == "claim" else 0)
        info = (ctypes.c_int * 4)()
        nat.lib.gacq_debug_f4k_map(E, len(dop), 1, -1 if run == "claim" else run, torch.cuda.get_device_properties(0).multi_processor_count, info, None, 0)
        assert info[3] <= nblocks
        assert nat.lib.gacq_debug_f4k_stamps(None, 0) == 0
        for _ in range(3):
            eng.search_batch_dev(sig, xd, items, dop, 1)
        torch.cuda.synchronize()
        stamps.zero_()
        torch.cuda.synchronize()
        assert nat.lib.gacq_debug_f4k_stamps(ctypes.c_void_p(stamps.data_ptr()), nblocks) == 0
        eng.search_batch_dev(sig, xd, items, dop, 1)
        torch.cuda.synchronize()
        assert nat.lib.gacq_debug_f4k_stamps(None, 0) == 0
        report(run, stamps.cpu().numpy(), info[3])
    eng.close()


if __name__ == "__main__":
    main()
