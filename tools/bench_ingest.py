#!/usr/bin/env python3
"""Rates of the recording ingest (gnss_dsp_tools_amd/ingest.py, gacq_ingest_dev) on one GPU: HIP events, median of 20 after three
warm-up calls, 2^26 input bytes resident in HBM, int8 output into a buffer allocated before.  For u8, s16, f32 and 2sm I/Q and for 2sm
and s8 real IF: input plus output bytes per second, that rate as a share of the copy rate Engine.stream_probe reports in the same
run, and two baselines timed in the same run:

  (a) the same conversion written in torch operations on the device (what the package could do without the kernel); its output is
      compared with the kernel's, and the number of differing bytes is printed.  Real IF: on the first 2^24 input values;
  (b) tests/ingest_oracle.py (numpy, one core) on the host, on a shorter stretch.

usage: tools/bench_ingest.py [--bytes 67108864] [--host-bytes 4194304] [--torch-values 16777216] [--reps 20] [--warmup 3]
prints one line per format and a JSON summary line."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from gnss_dsp_tools_amd import _native as nat  # noqa: E402
from gnss_dsp_tools_amd import acquire, ingest  # noqa: E402

CASES = [("u8", False, 0.73), ("s16", False, 0.0031), ("f32", False, 1.7), ("2sm", False, 9.7), ("2sm", True, 9.3), ("s8", True, 0.61)]
G_ODD = (10382, -3333, 1852, -1175, 774, -506, 320, -188, 97, -40, 9)


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


def host_bytes(name, nbytes):
    rng = np.random.Generator(np.random.PCG64(len(name) + nbytes))
    if name == "f32":
        return (20.0 * rng.standard_normal(nbytes // 4)).astype("<f4").view(np.uint8)
    return rng.integers(0, 256, size=nbytes, dtype=np.uint8)


def to_int8(torch, v, gain):
    return torch.clamp(torch.round(v * gain), -127.0, 127.0).to(torch.int8)


def torch_convert(torch, name, real, x, gain, n_out):
    """the conversion in torch operations: flat int8 [2 n_out]"""
    if name == "u8":
        v = x.to(torch.float32) - 128.0
    elif name == "s8":
        v = x.view(torch.int8).to(torch.float32)
    elif name == "s16":
        v = x.view(torch.int16).to(torch.float32)
    elif name == "f32":
        v = x.view(torch.float32)
    else:
        shifts = torch.tensor([6, 4, 2, 0], dtype=torch.uint8, device=x.device)
        lut = torch.tensor([1.0, 3.0, -1.0, -3.0], dtype=torch.float32, device=x.device)
        v = lut[((x[:, None] >> shifts[None, :]) & 3).reshape(-1).to(torch.int64)]
    if not real:
        return to_int8(torch, v[:2 * n_out], gain)
    # fs/4 down-shift, then the 43 taps at stride two on the two components: integers below 2^24, so fp32 is exact
    n = 2 * (n_out - 1) + 22
    v = v[:n]
    k = torch.arange(n, device=x.device) % 4
    rot = torch.stack([torch.tensor([1.0, 0.0, -1.0, 0.0], device=x.device)[k], torch.tensor([0.0, -1.0, 0.0, 1.0], device=x.device)[k]])
    g = np.zeros(43)
    g[21] = 16384
    for i, t in enumerate(G_ODD):
        g[21 + 2 * i + 1] = g[21 - 2 * i - 1] = t
    w = torch.tensor(g[::-1].copy(), dtype=torch.float32, device=x.device).reshape(1, 1, 43)
    acc = torch.nn.functional.conv1d((rot * v[None, :])[:, None, :], w, stride=2, padding=21)[:, 0, :n_out]      # [2, n_out]
    return to_int8(torch, (acc * 2.0 ** -14).t().reshape(-1), gain)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=1 << 26)
    ap.add_argument("--host-bytes", type=int, default=1 << 22)
    ap.add_argument("--torch-values", type=int, default=1 << 24, help="real IF: input values of the torch formulation")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    torch = nat.require_torch()
    import ingest_oracle as O
    eng = acquire.Engine(0)
    dev = "cuda:0"
    eng.use_torch_stream()
    copy = eng.stream_probe("copy")
    print("stream_probe copy %.0f GB/s (read + write bytes)" % copy)
    summary = {"copy_gbs": copy, "formats": {}}
    for name, real, gain in CASES:
        fmt = ingest.Format(name, real=real)
        h = host_bytes(name, a.bytes)
        x = torch.from_numpy(h).to(dev)
        in_count = fmt.samples(a.bytes)
        _, n_out = fmt.out_range(0, in_count)
        out = torch.empty(2 * n_out, dtype=torch.int8, device=dev)
        st = fmt.struct()

        def kernel():
            nat.check(nat.lib.gacq_ingest_dev(eng._ctx, ctypes.addressof(st), ctypes.c_void_p(x.data_ptr()), 0, in_count, 0, n_out, gain, 0,
                                              ctypes.c_void_p(out.data_ptr())), eng._ctx)

        k_ms, k_min = timed(torch, kernel, a.reps, a.warmup)
        # real IF: the torch formulation runs on 2^24 values (one convolution over 2^28 is more than the library is asked for here)
        t_in = a.bytes if not real else min(a.bytes, a.torch_values * fmt.sample_bits // 8)
        t_out = n_out if not real else fmt.out_range(0, fmt.samples(t_in))[1]
        try:
            t_ms, _ = timed(torch, lambda: torch_convert(torch, name, real, x[:t_in], gain, t_out), a.reps, a.warmup)
            differ = int((torch_convert(torch, name, real, x[:t_in], gain, t_out) != out[:2 * t_out]).sum())
        except RuntimeError as e:
            print("%s: the torch formulation failed: %s" % (name, str(e).splitlines()[0]))
            t_ms, differ = float("nan"), -1
        torch.cuda.synchronize()
        t_rate = (t_in + 2 * t_out) / (t_ms * 1e-3) / 1e9
        # the host oracle, once, on a shorter stretch
        hb = bytes(h[:a.host_bytes])
        f = O.fmt(name, real=real)
        t0 = time.perf_counter()
        ref = O.evaluate(f, hb, gain)
        host_s = time.perf_counter() - t0
        same = bool(np.array_equal(ref, out[:len(ref)].cpu().numpy()))
        moved = a.bytes + 2 * n_out
        host_moved = len(hb) + len(ref)
        rate = moved / (k_ms * 1e-3) / 1e9
        label = "%s %s" % (name, "real" if real else "I/Q")
        print("%-9s kernel %8.3f ms (min %.3f)  %7.1f GB/s in+out  %5.1f %% of copy | torch (%d bytes in) %8.3f ms  %6.1f GB/s  kernel x%.1f  "
              "differing bytes %d | host oracle %.4f GB/s (%d bytes in, equal %s)" % (label, k_ms, k_min, rate, 100.0 * rate / copy, t_in, t_ms, t_rate,
                                                                                      rate / t_rate, differ, host_moved / host_s / 1e9, len(hb), same))
        summary["formats"][label] = dict(kernel_ms=k_ms, gbs=rate, share_of_copy=rate / copy, torch_ms=t_ms, torch_in_bytes=t_in, torch_gbs=t_rate,
                                         torch_differing_bytes=differ,
                                         host_gbs=host_moved / host_s / 1e9, host_equal=same, in_bytes=a.bytes, out_bytes=2 * n_out)
        del x, out
    eng.close()
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
