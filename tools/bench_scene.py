#!/usr/bin/env python3
"""Rates of the array-and-interference scene generator (gnss_dsp_tools_amd/scene.py, gacq_scene_dev) on one GPU: HIP events, median of
20 after three warm-up calls, 2^24 samples per antenna, int8 output.  Three cases (M antennas, K satellites, I emitters):

  (1, 1, 0) beside gacq_simulate_dev on the same scene in the same run: the same work, so the ratio is what the generality costs;
  (4, 8, 2) and (8, 8, 4) beside the only way to make such a scene without the generator: M calls of simulate.recording in complex64
      (each antenna walks all K satellites again, under its own carrier phases), the jammers drawn with torch.randn and the tones and
      chirps evaluated with torch operations, the gains applied and the sum rounded to int8 in torch.  That baseline cannot share the
      satellites across antennas, and its jammers are not a function of the absolute sample index.

usage: tools/bench_scene.py [--samples 16777216] [--reps 20] [--warmup 3]
prints one line per case and a JSON summary line."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gnss_dsp_tools_amd import _native as nat  # noqa: E402
from gnss_dsp_tools_amd import acquire, scene, simulate  # noqa: E402

FS, COFFSET, SIGMA, SEED = 16.368e6, 250000.0, 6.0, 20261020
PRNS = (3, 7, 11, 14, 17, 19, 22, 30)


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


def make_scene(M, K, I):
    sats = [simulate.Satellite("gps-l1", PRNS[k], 2.0 + 0.1 * k, -3000.0 + 900.0 * k, 100.5 * (k + 1), 0.1 * k) for k in range(K)]
    kinds = [scene.NoiseJammer(30.0), scene.Chirp(40.0, -5.0e6, 5.0e6, 2050), scene.Tone(25.0, 1.234e6, gate=(2000, 16000, 100)),
             scene.Chirp(20.0, 3.0e6, -2.0e6, 4096, triangle=True)]
    rng = np.random.default_rng(7)
    gains = np.exp(2j * np.pi * rng.random((M, K + I)))
    return sats, kinds[:I], gains


def torch_scene(torch, eng, sats, emitters, gains, n):
    """the scene from M single-antenna recordings, with the jammers and the gains in torch: int8 [M, 2 n]"""
    dev = "cuda:%d" % eng.device
    M, K = gains.shape[0], len(sats)
    j = torch.arange(n, dtype=torch.float64, device=dev)
    z = []
    for e in emitters:
        if isinstance(e, scene.NoiseJammer):
            w = torch.complex(torch.randn(n, device=dev), torch.randn(n, device=dev)) * e.sigma
        else:
            if isinstance(e, scene.Tone):
                turns = e.hz / FS * j
            else:
                half = e.sweep // 2 if e.triangle else e.sweep
                u = torch.remainder(j, e.sweep)
                r = torch.where(u < half, u, e.sweep - 1 - u) if e.triangle else u
                turns = torch.cumsum((e.f0 + (e.f1 - e.f0) / half * r) / FS, 0)
            ang = 2.0 * np.pi * torch.remainder(turns, 1.0)
            w = torch.complex(torch.cos(ang).float(), torch.sin(ang).float()) * e.amp
        if e.gate is not None:
            w = torch.where(torch.remainder(j - e.gate[2], e.gate[1]) < e.gate[0], w, torch.zeros_like(w))
        z.append(w)
    rows = []
    for p in range(M):
        own = [simulate.Satellite(s.tracker, s.item, s.amp * abs(gains[p, k]), s.doppler, s.code0, s.carrier_phase + np.angle(gains[p, k]) / (2 * np.pi))
               for k, s in enumerate(sats)]
        v = simulate.recording(own, FS, COFFSET, n, SEED + p, SIGMA, dtype="complex64", engine=eng)
        for i, w in enumerate(z):
            v = v + w * complex(gains[p, K + i])
        rows.append(torch.view_as_real(v).round().clamp(-127, 127).to(torch.int8).reshape(-1))
    return torch.stack(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1 << 24)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    torch = nat.require_torch()
    eng = acquire.Engine(0)
    n = a.samples
    rows = []
    for M, K, I in ((1, 1, 0), (4, 8, 2), (8, 8, 4)):
        sats, emitters, gains = make_scene(M, K, I)
        ms, ms_min = timed(torch, lambda: scene.recording(sats, emitters, gains, FS, COFFSET, n, SEED, SIGMA, engine=eng), a.reps, a.warmup)
        if (M, I) == (1, 0):
            base, what = timed(torch, lambda: simulate.recording(sats, FS, COFFSET, n, SEED, SIGMA, engine=eng), a.reps, a.warmup)[0], "gacq_simulate_dev"
        else:
            base, what = timed(torch, lambda: torch_scene(torch, eng, sats, emitters, gains, n), max(3, a.reps // 4), 1)[0], "M simulate calls + torch"
        rate = n / ms * 1e-6
        rows.append(dict(M=M, K=K, I=I, samples=n, ms=ms, ms_min=ms_min, gs_per_antenna=rate, gs_all_antennas=rate * M, baseline=what, baseline_ms=base))
        print("M %d K %d I %d: %8.3f ms (min %.3f) %6.2f GS/s per antenna, %6.2f GS/s over all antennas | %s %8.3f ms (x%.2f)"
              % (M, K, I, ms, ms_min, rate, rate * M, what, base, base / ms))
    eng.close()
    print(json.dumps(dict(tool="bench_scene", samples=n, rows=rows)))


if __name__ == "__main__":
    main()
