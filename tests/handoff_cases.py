"""Synthetic int8 recordings for the refine / hand-off tests: noise of sigma 12 per component plus satellites at off-grid Dopplers and
fractional code phases, with data bits that flip on code-period boundaries.  A satellite is a dict:
    tracker   name in trackloop.TRACKERS          item     PRN, or the RF channel for GLONASS L1/L2
    amp       amplitude per component             doppler  Hz, on top of the recording's carrier offset (+ the FDMA channel offset)
    code0     code phase at sample 0, chips
    bit       optional: code periods per data bit (default 1: every code period draws its own sign)
The code runs at chip_rate + doppler / ratio, as the trackers and the correlation grid model it."""
import numpy as np

import refine_oracle
from gnss_dsp_tools_amd import codes, trackloop


def carrier_hz(tracker, item, coffset):
    t = trackloop.TRACKERS[tracker]
    return float(coffset) + (t.glonass[3] * int(item) if t.glonass else 0.0)


def recording(seed, fs, nsamp, coffset, sats, sigma=12.0):
    """interleaved int8 I/Q, flat [2 nsamp]"""
    rng = np.random.Generator(np.random.PCG64(seed))
    j = np.arange(nsamp, dtype=np.float64)
    x = rng.normal(0.0, sigma, size=(nsamp, 2))
    for s in sats:
        t = trackloop.TRACKERS[s["tracker"]]
        item = int(s["item"])
        c = codes.chips(t.code, 0 if t.glonass else item)
        L = len(c)
        cf = (codes.chip_rate(t.code) + s["doppler"] / t.scale(item)) / fs
        w = refine_oracle.weight(c, t.kind, float(s["code0"]), cf, j)
        period = np.floor((float(s["code0"]) + cf * j) / L).astype(np.int64)
        period //= int(s.get("bit", 1))
        bits = 1.0 - 2.0 * rng.integers(0, 2, size=int(period[-1]) + 2)
        ang = np.mod((carrier_hz(s["tracker"], item, coffset) + s["doppler"]) * j / fs, 1.0) * (2 * np.pi)
        a = s["amp"] * w * bits[period]
        x[:, 0] += a * np.cos(ang)
        x[:, 1] += a * np.sin(ang)
    return np.clip(np.round(x), -127, 127).astype(np.int8).ravel()
