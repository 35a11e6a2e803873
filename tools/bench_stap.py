"""Call times of space-time nulling (stap.py on csrc/gacq_stap.hip) at a user size, beside the device's own copy rate, beside nulling.py
at one tap and beside a torch formulation of the same computation:

    python tools/bench_stap.py [CALLS] [--no-probe] [--no-torch]

(M, T) = (1, 9), (4, 5), (8, 7) and (4, 1), block 4096, window 8, 2^26 samples per antenna resident on the device, int8 output.  A call
is the three launches of gacq_stap_run_dev (covariances, weights, outputs) between two events on the stream, median of CALLS (default 5)
after a warm-up call.  The kernels move 4 M + 2 bytes per sample through HBM (the covariance kernel and the apply kernel each read the
2 M input bytes, the apply kernel writes 2; the taps re-read through the caches): the line gives samples/s and the fraction of
Engine.stream_probe("copy"), measured in this process, that this traffic amounts to.  (4, 1) runs beside a Nuller on the same tensors:
the price of the general path.  The torch formulation -- unfold for the taps, einsum for the block covariances, a cumulative sum for the
window, torch.linalg.solve, einsum for the apply, complex64 / complex128 -- runs on the first 2^22 samples (the stacked tensor of 2^26
would not fit), and so does a kernel call beside it.  Kernel times come from a run of this script under
``rocprofv3 --kernel-trace --stats`` with --no-probe --no-torch (kernels stap_cov_kernel, stap_weights_kernel, stap_apply_kernel)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gnss_dsp_tools_amd import acquire, nulling, stap
import torch

REPS = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 5
PROBE = "--no-probe" not in sys.argv
TORCH = "--no-torch" not in sys.argv
N, NT, LB, W, SHIFT = 1 << 26, 1 << 22, 4096, 8, 10
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


def torch_stap(xs, T, n):
    """outputs 0 .. n - 1 (n a multiple of the block) by torch alone: complex64 samples, complex128 solve"""
    M, tc = len(xs), (T - 1) // 2
    x = torch.stack([torch.view_as_complex(d[:2 * (n + tc)].to(torch.float32).reshape(-1, 2)) for d in xs])
    x = torch.cat([torch.zeros((M, tc), dtype=x.dtype, device=x.device), x], 1)   # samples below 0 are zeros
    z = x.unfold(1, T, 1).flip(2)                                       # [M][n][T]: z[p][j][t] = x_p(j + tc - t)
    z = z.reshape(M, n // LB, LB, T).permute(1, 2, 0, 3).reshape(n // LB, LB, M * T)
    C = torch.einsum("bje,bjf->bef", z, z.conj()).to(torch.complex128)
    S = torch.cumsum(C, 0)
    R = torch.cat([S[W - 1:W].expand(W + 1, -1, -1), S[W:-1] - S[:-W - 1]])       # blocks 0 .. W the warm-up, block b the W before it
    d = torch.floor(torch.diagonal(R, dim1=1, dim2=2).real.sum(1) / (1 << SHIFT)) + 1.0
    A = R + torch.diag_embed(d[:, None].expand(-1, M * T)).to(torch.complex128)
    c = torch.zeros(M * T, dtype=torch.complex128, device=x.device)
    c[tc] = 1.0
    u = torch.linalg.solve(A, c.expand(A.shape[0], -1))
    w = (u / (u @ c.conj())[:, None]).to(torch.complex64)
    return torch.einsum("bje,be->bj", z, w.conj()).reshape(-1)


rows = []
for M, T in ((1, 9), (4, 5), (8, 7), (4, 1)):
    g = torch.Generator(device=dev)
    g.manual_seed(5 + M)
    common = torch.randn(2 * N, device=dev, generator=g) * 30.0
    xs = [(common * (0.5 + 0.1 * p) + torch.randn(2 * N, device=dev, generator=g) * 6.0).round().clamp(-127, 127).to(torch.int8) for p in range(M)]
    del common
    n = stap.out_end(LB, W, N, T)
    nbytes = (4 * M + 2) * n
    row = dict(antennas=M, taps=T, samples=n, block=LB, window=W)
    with stap.Stap(eng, M, T, LB, W, SHIFT) as sp:
        row["ms"], row["ms_min"], row["ms_max"] = timed(lambda: sp.run(xs, 0, 0, n, 1.0, "int8"))
        row["gsamples_per_s"], row["gbs"] = n / row["ms"] * 1e-6, nbytes / row["ms"] * 1e-6
        row["of_copy"] = None if copy_gbs is None else row["gbs"] / copy_gbs
        print("M %d T %2d -> int8  %.3f ms (min %.3f, max %.3f over %d calls)  %.2f Gsample/s  %.0f GB/s%s"
              % (M, T, row["ms"], row["ms_min"], row["ms_max"], REPS, row["gsamples_per_s"], row["gbs"],
                 "" if copy_gbs is None else " = %.1f %% of the probed copy rate" % (100.0 * row["of_copy"])), flush=True)
        if T == 1:
            with nulling.Nuller(eng, M, LB, W, SHIFT) as nl:
                row["nulling_ms"] = timed(lambda: nl.run(xs, 0, 0, n, 1.0, "int8"))[0]
                same = bool((nl.run(xs, 0, 0, n, 1.0, "int8") == sp.run(xs, 0, 0, n, 1.0, "int8")).all())
            print("          nulling.py on the same tensors %.3f ms: one tap through the general path costs %.2f x (same bytes: %s)"
                  % (row["nulling_ms"], row["ms"] / row["nulling_ms"], same), flush=True)
        elif TORCH:
            row["small_samples"] = NT
            row["small_ms"] = timed(lambda: sp.run(xs, 0, 0, NT, 1.0, "complex64"))[0]
            row["torch_ms"] = timed(lambda: torch_stap(xs, T, NT))[0]
            a, b = sp.run(xs, 0, 0, NT, 1.0, "complex64"), torch_stap(xs, T, NT)
            row["torch_rel_diff"] = float((a - b)[(W + 1) * LB:].abs().max() / a.abs().max())
            del a, b
            print("          first 2^22 samples, complex64: kernels %.3f ms, torch (unfold, einsum, linalg.solve) %.1f ms = %.0f x; outputs differ by %.1e of the largest"
                  % (row["small_ms"], row["torch_ms"], row["torch_ms"] / row["small_ms"], row["torch_rel_diff"]), flush=True)
            torch.cuda.empty_cache()
    rows.append(row)
    del xs
print(json.dumps(dict(tool="bench_stap", copy_gbs=copy_gbs, rows=rows)))
eng.close()
