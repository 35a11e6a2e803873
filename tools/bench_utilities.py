#!/usr/bin/env python3
"""Throughput of the two utility kernels (csrc/gacq_spectrum.hip) at the reference's example rate, 69.984 MS/s:

  resident   int8 I/Q already on the device: gacq_psd_int8_dev at several FFT lengths (ns = 1000 as in spectrum.py's example, and
             ns = 8) and gacq_squaring_int8_dev at the script's (b, n, m); device events around batches of launches, median of 7
  file       end to end from a file on disk through the command lines' readers (read, upload, kernel, download / write)
  cpu        the same work in vectorised numpy (tests/utilities_oracle.py) on this node, on a shorter input, for comparison

  reference  with --reference DIR (a checkout of the reference, where one is at hand): its nco.mix and squaring functions on one chunk

input_GBps is the int8 traffic a kernel needs (2 bytes per sample; the spectrum's fp64 partial sums come on top: 256 / ns of it for ns >= 128, none for ns <= 8): the
figure to set against the read rate tools/hbm_bandwidth.hip reports on the same node.  One JSON line per measurement; no pass/fail."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

from gnss_dsp_tools_amd import acquire, spectrum, squaring

FS, COFFSET = 69984000.0, -9334875.0


def device_ms(fn, inner, reps=7):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) / inner)
    return float(np.median(times)), float(min(times)), float(max(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0, help="length of the resident recording")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--reference", metavar="DIR", help="a checkout of the reference: also time its own nco.mix and squaring functions on one chunk")
    a = ap.parse_args()
    eng = acquire.Engine(0)
    eng.use_torch_stream()
    nsamp = int(FS * a.seconds)
    rng = np.random.default_rng(1)
    host = (rng.integers(0, 4, size=2 * nsamp, dtype=np.int8) * 2 - 3).astype(np.int8)          # 2-bit samples: +-1, +-3
    dev = torch.from_numpy(host).cuda()
    for n, ns in ((2048, 1000), (2048, 8), (256, 1000), (4096, 100), (16384, 8), (64, 1000)):
        F = nsamp // (n * ns)
        med, lo, hi = device_ms(lambda: spectrum.psd_dev(dev, n, ns, eng), 5)
        used = F * n * ns
        print(json.dumps({"kernel": "psd", "where": "resident", "n": n, "ns": ns, "spectra": F, "ms": med, "ms_min": lo, "ms_max": hi,
                          "Msamples_per_s": used / med / 1e3, "x_realtime": used / FS / (med * 1e-3), "input_GBps": 2 * used / med / 1e6}), flush=True)
    chunk = squaring.B * squaring.N * squaring.M
    med, lo, hi = device_ms(lambda: squaring.squaring_dev(dev, FS, COFFSET, engine=eng), 5)
    used = (nsamp // chunk) * chunk
    print(json.dumps({"kernel": "squaring", "where": "resident", "chunks": nsamp // chunk, "ms": med, "ms_min": lo, "ms_max": hi,
                      "Msamples_per_s": used / med / 1e3, "x_realtime": used / FS / (med * 1e-3), "input_GBps": 2 * used / med / 1e6}), flush=True)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "rec.iq")
        host.tofile(path)
        null = open(os.devnull, "wb")
        for label, fn in (("psd", lambda: spectrum.run([path, "1584754875", repr(FS), "2048", "1000", "--out", os.path.join(tmp, "o.f64")], engine=eng)),
                          ("squaring", lambda: squaring.run([path, repr(FS), repr(COFFSET)], null, eng))):
            fn()
            t = []
            for _ in range(3):
                t0 = time.perf_counter()
                fn()
                t.append(time.perf_counter() - t0)
            print(json.dumps({"kernel": label, "where": "file", "samples": nsamp, "s": float(np.median(t)), "Msamples_per_s": nsamp / np.median(t) / 1e6,
                              "x_realtime": a.seconds / float(np.median(t))}), flush=True)
        null.close()
    if not a.no_cpu:
        import utilities_oracle as O
        short = host[:2 * 4 * chunk]
        t0 = time.perf_counter()
        O.psd_fp64(short, 2048, 1000)
        t1 = time.perf_counter()
        O.squaring_fp64(short, FS, COFFSET, squaring.B, squaring.N, squaring.M)
        t2 = time.perf_counter()
        print(json.dumps({"kernel": "psd", "where": "cpu numpy fp64", "samples": 4 * chunk, "Msamples_per_s": (4 * chunk // 2048000) * 2048000 / (t1 - t0) / 1e6}))
        print(json.dumps({"kernel": "squaring", "where": "cpu numpy fp64", "samples": 4 * chunk, "Msamples_per_s": 4 * chunk / (t2 - t1) / 1e6}), flush=True)
    if a.reference:
        sys.path.insert(0, a.reference)
        import gnsstools.nco as ref_nco
        import gnsstools.squaring as ref_squaring
        x = np.empty(chunk, dtype=np.complex64)
        x.real, x.imag = host[0:2 * chunk:2], host[1:2 * chunk:2]
        r = np.zeros(squaring.B, dtype=np.complex128)
        t0 = time.perf_counter()
        ref_nco.mix(x, -COFFSET / FS, 0.0)
        ref_squaring.squaring(x, r, squaring.N, squaring.M)
        dt = time.perf_counter() - t0
        print(json.dumps({"kernel": "squaring", "where": "reference functions on the CPU", "samples": chunk, "Msamples_per_s": chunk / dt / 1e6}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
