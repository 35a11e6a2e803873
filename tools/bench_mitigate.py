#!/usr/bin/env python3
"""Rates of the interference mitigation (gnss_dsp_tools_amd/mitigate.py, gacq_mitigate_dev) on one GPU: HIP events, median of 20 after
three warm-up calls, 2^26 input bytes (2^25 int8 I/Q samples of noise, a chirped CW and a pulse train) resident in HBM, int8 output.
Excision at N = 256, 1024 and 4096, blanking alone, and both stages at N = 1024: input plus output bytes per second, that rate as a
share of the copy rate Engine.stream_probe reports in the same run, and two baselines timed in the same run:

  (a) the same filter written in torch operations on the device (unfold framing, torch.fft, torch.median, max_pool1d for the hold);
      its int8 output is compared with the kernel's and the number of differing bytes is printed;
  (b) tests/mitigate_oracle.py (numpy fp64, one core) on the host, on a shorter stretch.

usage: tools/bench_mitigate.py [--bytes 67108864] [--host-samples 1048576] [--reps 20] [--warmup 3]
prints one line per case and a JSON summary line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from gnss_dsp_tools_amd import _native as nat  # noqa: E402
from gnss_dsp_tools_amd import acquire, mitigate  # noqa: E402

BLANK, HOLD, RATIO, GUARD, GAIN = 85.0, 2, 12.0, 2, 4.7
CASES = [("excise N=256", None, 256), ("excise N=1024", None, 1024), ("excise N=4096", None, 4096), ("blank", BLANK, 0), ("both N=1024", BLANK, 1024)]


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


def recording(torch, n, dev):
    """n samples as interleaved int8: Gaussian noise (sigma 4), a chirped CW of amplitude 60 near +317 kHz of 4.096 MS/s, 24-sample pulses
    of amplitude 110 every 1000 samples"""
    g = torch.Generator(device=dev)
    g.manual_seed(20261019)
    j = torch.arange(n, dtype=torch.float64, device=dev)
    t = j / 4.096e6
    ph = 2.0 * np.pi * (317.0e3 * t + 1.0e6 * t * t)
    x = 4.0 * torch.randn(n, 2, generator=g, device=dev, dtype=torch.float32)
    x[:, 0] += (60.0 * torch.cos(ph)).float()
    x[:, 1] += (60.0 * torch.sin(ph)).float()
    on = ((j.to(torch.int64) + 400) % 1000) < 24
    pp = 2.0 * np.pi * -523.0e3 * t + 0.7
    x[:, 0] += torch.where(on, 110.0 * torch.cos(pp), 0.0).float()
    x[:, 1] += torch.where(on, 110.0 * torch.sin(pp), 0.0).float()
    return torch.clamp(torch.round(x), -127, 127).to(torch.int8).reshape(-1)


def torch_filter(torch, x, blank, nfft, n_out):
    """the filter in torch operations: flat int8 [2 n_out]"""
    v = x.view(-1, 2)
    if blank:
        p = v[:, 0].to(torch.int32) ** 2 + v[:, 1].to(torch.int32) ** 2
        hit = (p > int(blank * blank)).to(torch.float32).view(1, 1, -1)
        forced = torch.nn.functional.max_pool1d(hit, 2 * HOLD + 1, 1, HOLD).view(-1) > 0
        v = torch.where(forced.unsqueeze(1), torch.zeros_like(v), v)
    z = torch.complex(v[:, 0].float(), v[:, 1].float())
    if nfft:
        h = nfft // 2
        w = torch.sin(np.pi * (torch.arange(nfft, dtype=torch.float64, device=x.device) + 0.5) / nfft).float()
        nb = n_out // h
        fr = torch.cat([torch.zeros(h, dtype=z.dtype, device=z.device), z[:(nb + 1) * h]]).unfold(0, nfft, h) * w
        spec = torch.fft.fft(fr, dim=1)
        p = spec.real ** 2 + spec.imag ** 2
        hit = p > RATIO * torch.median(p, dim=1, keepdim=True).values
        zero = hit.clone()
        for d in range(1, GUARD + 1):
            zero |= torch.roll(hit, d, 1) | torch.roll(hit, -d, 1)
        y = torch.fft.ifft(torch.where(zero, torch.zeros_like(spec), spec), dim=1) * w
        z = (y[:-1, h:] + y[1:, :h]).reshape(-1)
    out = torch.view_as_real(z[:n_out]) * GAIN
    return torch.clamp(torch.round(out), -127.0, 127.0).to(torch.int8).reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=1 << 26)
    ap.add_argument("--host-samples", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    torch = nat.require_torch()
    import mitigate_oracle as O
    eng = acquire.Engine(0)
    dev = "cuda:0"
    copy_gbs = eng.stream_probe("copy")
    print("copy probe %.0f GB/s" % copy_gbs)
    n = a.bytes // 2
    x = recording(torch, n, dev)
    rows = []
    for name, blank, nfft in CASES:
        cfg = mitigate.Config(blank=blank, hold=HOLD, nfft=nfft, ratio=RATIO if nfft else None, guard=GUARD)
        n_out = cfg.out_range(0, n)[1]
        out, st = mitigate.apply(eng, cfg, x, GAIN, 0, 0, n_out, "int8", True)
        ms, ms_min = timed(torch, lambda: mitigate.apply(eng, cfg, x, GAIN, 0, 0, n_out, "int8"), a.reps, a.warmup)
        gbs = (2.0 * n + 2.0 * n_out) / ms * 1e-6
        ref = torch_filter(torch, x, blank, nfft, n_out)
        diff = int((ref != out).sum())
        tms, _ = timed(torch, lambda: torch_filter(torch, x, blank, nfft, n_out), max(3, a.reps // 4), 1)
        del ref
        hn = min(a.host_samples, n)
        hx = x[:2 * hn].cpu().numpy()
        ocfg = O.config(blank=blank, hold=HOLD, nfft=nfft, ratio=RATIO, guard=GUARD)
        t0 = time.perf_counter()
        r = O.evaluate(ocfg, hx, GAIN)
        host_ms = (time.perf_counter() - t0) * 1e3 * n_out / max(1, len(r.c64))
        hdiff = int((r.i8 != out[:len(r.i8)].cpu().numpy()).sum())
        row = dict(case=name, samples=n_out, ms=ms, ms_min=ms_min, gbs=gbs, of_copy=gbs / copy_gbs, torch_ms=tms, torch_diff_bytes=diff,
                   host_ms_scaled=host_ms, host_diff_bytes=hdiff, blanked=st.blanked / float(n_out),
                   bins=(st.bins / float(st.frames * nfft)) if nfft else 0.0)
        rows.append(row)
        print("%-14s %8.3f ms (min %.3f) %7.1f GB/s in+out = %4.1f %% of copy | torch ops %8.2f ms (x%.1f, %d bytes differ) | host oracle "
              "%9.0f ms scaled (x%.0f, %d of %d bytes differ) | blanked %.4f excised %.4f"
              % (name, ms, ms_min, gbs, 100.0 * gbs / copy_gbs, tms, tms / ms, diff, host_ms, host_ms / ms, hdiff, len(r.i8), row["blanked"], row["bins"]))
    eng.close()
    print(json.dumps(dict(tool="bench_mitigate", bytes=a.bytes, copy_gbs=copy_gbs, rows=rows)))


if __name__ == "__main__":
    main()
