"""Call times of spatial nulling (nulling.py on csrc/gacq_null.hip) at a user size, beside the device's own copy rate:

    python tools/bench_nulling.py [CALLS] [--no-probe]

M = 4 and 8 antennas, block 4096, window 8, 2^26 samples per antenna resident on the device, int8 and complex64 output.  A call is the
three launches of gacq_null_run_dev (covariances, weights, outputs) between two events on the stream, median of CALLS (default 5) after
a warm-up call.  The three kernels move about 4 M + 2 bytes per sample with int8 output (the covariance kernel and the apply kernel
each read the 2 M input bytes, the apply kernel writes 2): the line gives samples/s and the fraction of Engine.stream_probe("copy"),
measured in this process, that this traffic amounts to.  Kernel times come from a run of this script under
``rocprofv3 --kernel-trace --stats`` with --no-probe (kernels null_cov_kernel, null_weights_kernel, null_apply_kernel)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gnss_dsp_tools_amd import acquire, nulling
import torch

REPS = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 5
PROBE = "--no-probe" not in sys.argv
N, LB, W = 1 << 26, 4096, 8
eng = acquire.Engine(0)
dev = "cuda:%d" % eng.device
copy_gbs = eng.stream_probe("copy") if PROBE else None
if PROBE:
    print("stream probe: copy %.0f GB/s (read + write bytes)" % copy_gbs, flush=True)
rows = []
for M in (4, 8):
    g = torch.Generator(device=dev)
    g.manual_seed(5 + M)
    common = torch.randn(2 * N, device=dev, generator=g) * 30.0
    xs = []
    for p in range(M):
        x = (common * (0.5 + 0.1 * p) + torch.randn(2 * N, device=dev, generator=g) * 6.0).round().clamp(-127, 127).to(torch.int8)
        xs.append(x)
    del common
    with nulling.Nuller(eng, M, LB, W) as nl:
        for dtype in ("int8", "complex64"):
            nl.run(xs, 0, 0, N, 1.0, dtype)
            torch.cuda.synchronize()
            ts = []
            for _ in range(REPS):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                out = nl.run(xs, 0, 0, N, 1.0, dtype)
                b.record()
                torch.cuda.synchronize()
                ts.append(a.elapsed_time(b))
                del out
            ts.sort()
            ms = ts[len(ts) // 2]
            nbytes = (4 * M + (2 if dtype == "int8" else 8)) * N
            row = dict(antennas=M, dtype=dtype, samples=N, block=LB, window=W, ms=ms, ms_min=ts[0], ms_max=ts[-1], gsamples_per_s=N / ms * 1e-6,
                       gbs=nbytes / ms * 1e-6, of_copy=None if copy_gbs is None else nbytes / ms * 1e-6 / copy_gbs)
            rows.append(row)
            print("M %d -> %-9s %.3f ms (min %.3f, max %.3f over %d calls)  %.2f Gsample/s  %.0f GB/s%s"
                  % (M, dtype, ms, ts[0], ts[-1], REPS, row["gsamples_per_s"], row["gbs"],
                     "" if copy_gbs is None else " = %.1f %% of the probed copy rate" % (100.0 * row["of_copy"])), flush=True)
    del xs
print(json.dumps(dict(tool="bench_nulling", copy_gbs=copy_gbs, rows=rows)))
eng.close()
