"""Call times of the per-satellite beams (beams.py on csrc/gacq_beams.hip) beside the K nulling calls they replace:

    python tools/bench_beams.py [CALLS] [--no-probe]

M = 4 and 8 antennas, K = 1, 4, 8 and 16 beams, block 4096, window 8, 2^26 samples per antenna resident on the device, int8 and
complex64 output.  Both sides run in this process on the same inputs: one gacq_beams_run_dev call between two events on the stream,
and the K gacq_null_run_dev calls (one open Nuller per constraint) between two events; the bits are compared first, then the median
of CALLS (default 5) after a warm-up.  The yardstick is the K nulling calls, never beams against itself.  With int8 output the K calls
move K (4 M + 2) bytes per sample and the one pass 4 M + 2 K: the line gives the measured ratio beside that model's, and the fraction
of Engine.stream_probe("copy"), measured in this process, that the one pass's traffic amounts to.  Kernel times come from a run of this
script under ``rocprofv3 --kernel-trace --stats`` with --no-probe (kernels null_cov_kernel, beams_weights_kernel, beams_apply_kernel)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from gnss_dsp_tools_amd import acquire, beams, nulling
import torch

REPS = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 5
PROBE = "--no-probe" not in sys.argv
N, LB, W = 1 << 26, 4096, 8
eng = acquire.Engine(0)
dev = "cuda:%d" % eng.device
copy_gbs = eng.stream_probe("copy") if PROBE else None
if PROBE:
    print("stream probe: copy %.0f GB/s (read + write bytes)" % copy_gbs, flush=True)


def timed(call):
    call()
    torch.cuda.synchronize()
    ts = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = call()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
        del out
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


rows = []
for M in (4, 8):
    g = torch.Generator(device=dev)
    g.manual_seed(5 + M)
    common = torch.randn(2 * N, device=dev, generator=g) * 30.0
    xs = []
    for p in range(M):
        xs.append((common * (0.5 + 0.1 * p) + torch.randn(2 * N, device=dev, generator=g) * 6.0).round().clamp(-127, 127).to(torch.int8))
    del common
    rng = np.random.default_rng(40 + M)
    for K in (1, 4, 8, 16):
        cs = [None] + [rng.uniform(0.3, 1.5, M) * np.exp(2j * np.pi * rng.uniform(0.0, 1.0, M)) for _ in range(K - 1)]
        gains = [1.0 + 0.125 * k for k in range(K)]
        nullers = [nulling.Nuller(eng, M, LB, W, constraint=c) for c in cs]
        with beams.Beamformer(eng, M, cs, LB, W) as bf:
            for dtype in ("int8", "complex64"):
                got = bf.run(xs, 0, 0, N, gains, dtype)
                same = True
                for k, nl in enumerate(nullers):                     # the bits first
                    same = same and bool((nl.run(xs, 0, 0, N, gains[k], dtype) == got[k]).all())
                del got
                if not same:
                    raise SystemExit("beams and nulling differ at M %d K %d %s" % (M, K, dtype))
                ms, lo, hi = timed(lambda: bf.run(xs, 0, 0, N, gains, dtype))
                ms_n, lo_n, hi_n = timed(lambda: [nl.run(xs, 0, 0, N, gains[k], dtype) for k, nl in enumerate(nullers)])
                per = 2 if dtype == "int8" else 8
                nbytes = (4 * M + per * K) * N
                model = (4 * M + per) * K / (4 * M + per * K)
                row = dict(antennas=M, beams=K, dtype=dtype, samples=N, block=LB, window=W, ms=ms, ms_min=lo, ms_max=hi, nulling_ms=ms_n, nulling_ms_min=lo_n,
                           nulling_ms_max=hi_n, ratio=ms_n / ms, model=model, gbs=nbytes / ms * 1e-6,
                           of_copy=None if copy_gbs is None else nbytes / ms * 1e-6 / copy_gbs)
                rows.append(row)
                print("M %d K %2d -> %-9s beams %8.3f ms (min %.3f, max %.3f)  %2d nulling calls %8.3f ms (min %.3f, max %.3f)  ratio %.2f (byte model %.2f)  %.0f GB/s%s"
                      % (M, K, dtype, ms, lo, hi, K, ms_n, lo_n, hi_n, row["ratio"], model, row["gbs"],
                         "" if copy_gbs is None else " = %.1f %% of the probed copy rate" % (100.0 * row["of_copy"])), flush=True)
        for nl in nullers:
            nl.close()
    del xs
print(json.dumps(dict(tool="bench_beams", copy_gbs=copy_gbs, rows=rows)))
eng.close()
