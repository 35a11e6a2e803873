"""Cases shared by the nulling tests (test_nulling_cpu.py, test_nulling_gpu.py): array recordings that are asymmetric between the
antennas and between I and Q, the configurations they run under, their oracle results (computed once, never changed) and the
rounding-tie margin of every case -- equality of the quantised weights is claimed only where no scaled weight component lies within
1e-6 of a half-integer, and check_margins() asserts that of every block of every case, so the seeds below were chosen on the CPU."""
import functools

import numpy as np

import nulling_oracle as O

MARGIN = 1e-6
TILE = 16384                                        # gacq_null_tile: samples a workgroup of the apply kernel owns
RUN = 8                                             # samples of a lane's run


def recording(M, N, seed, jam=30.0, loud_until=None):
    """M interleaved int8 arrays [2 N]: one broadband source under a different complex coefficient per antenna plus independent noise
    whose I and Q deviations differ from each other and from antenna to antenna; a few components are put at -128 and 127.  With
    loud_until the samples before it are four times as strong."""
    rng = np.random.default_rng(seed)
    g = rng.normal(0.0, jam, N) + 1j * rng.normal(0.0, jam, N)
    xs = []
    for p in range(M):
        a = (0.55 + 0.09 * p) * np.exp(2j * np.pi * (0.137 * p * p + 0.21 * p))
        z = a * g + rng.normal(0.0, 5.0 + 0.7 * p, N) + 1j * rng.normal(0.0, 3.0 + 0.4 * p, N)
        if loud_until is not None:
            z[:loud_until] *= 4.0
        x = np.empty(2 * N, dtype=np.float64)
        x[0::2], x[1::2] = z.real, z.imag
        x = np.clip(np.rint(x), -128, 127).astype(np.int8)
        x[rng.integers(0, 2 * N, 16)] = -128
        x[rng.integers(0, 2 * N, 16)] = 127
        xs.append(x)
    return xs


def length(Lb, W):
    """W + 3 whole blocks and a partial one"""
    return (W + 3) * Lb + Lb // 2 + 5


# name -> (M, Lb, W, seed, kind); kind: "noise" (recording), "min" (every component -128), "shared" (antennas 0 and 2 one array),
# "steer" (a non-default constraint), "loud", "long"
CASES = {}
for _M in (2, 3, 5, 8):
    for _Lb in (64, 128, 4096, 32768):
        for _W in (1, 3):
            CASES["m%d-b%d-w%d" % (_M, _Lb, _W)] = (_M, _Lb, _W, 1000 * _M + _Lb % 997 + _W, "noise")
CASES["min-m8-b32768-w1"] = (8, 32768, 1, 0, "min")
CASES["min-m3-b64-w3"] = (3, 64, 3, 0, "min")
CASES["shared-m3-b128-w3"] = (3, 128, 3, 77, "shared")
CASES["steer-m5-b128-w3"] = (5, 128, 3, 78, "steer")
CASES["loud-m4-b256-w3"] = (4, 256, 3, 79, "loud")          # the first W blocks four times as strong
# recordings longer than a workgroup tile of the apply kernel; 192 does not divide the tile, 4096 puts a block edge on the tile's
CASES["long-m3-b128-w3"] = (3, 128, 3, 80, "long")
CASES["long-m8-b4096-w1"] = (8, 4096, 1, 81, "long")
CASES["long-m2-b192-w2"] = (2, 192, 2, 82, "long")
STEER = np.array([1.0 + 0.0j, 0.3 - 0.8j, -0.5 + 0.25j, 0.0 + 1.0j, 0.7 + 0.7j])
OUTPUT_CASES = ["m2-b64-w3", "m3-b128-w1", "m5-b4096-w3", "m8-b128-w3", "shared-m3-b128-w3", "steer-m5-b128-w3"]


def constraint(name):
    return STEER if CASES[name][4] == "steer" else None


@functools.lru_cache(maxsize=None)
def data(name):
    M, Lb, W, seed, kind = CASES[name]
    N = TILE + 5 * Lb + 37 if kind == "long" else length(Lb, W)
    if kind == "min":
        return tuple(np.full(2 * N, -128, dtype=np.int8) for _ in range(M))
    xs = recording(M, N, seed, loud_until=W * Lb if kind == "loud" else None)
    if kind == "shared":
        xs[2] = xs[0]
    return tuple(xs)


@functools.lru_cache(maxsize=None)
def reference(name, complex64=False, gain=1.0):
    """the oracle on the whole recording of a case"""
    M, Lb, W, seed, kind = CASES[name]
    xs = data(name)
    return O.run(list(xs), 0, 0, len(xs[0]) // 2, Lb, W, 10, constraint(name), gain, complex64)


def check_margins():
    """name -> margin, after asserting the margin of every case"""
    out = {}
    for name in CASES:
        out[name] = reference(name)["margin"]
        assert out[name] >= MARGIN, (name, out[name])
    return out


def cuts(Lb, W, N, tile=TILE):
    """where calls end and start: a workgroup tile, a block edge, one lane's run before and after each, and odd places"""
    pts = set()
    for edge in (tile, (W + 1) * Lb, (W + 2) * Lb):
        for d in (-RUN, 0, RUN):
            pts.add(edge + d)
    pts.update((W * Lb + 3, N - 11))
    return sorted(p for p in pts if 0 < p < N)


# ---- the end-to-end scene: 4 antennas, GPS L1 C/A at 4.092 MS/s, PRN 17 at amplitude 1 with a carrier phase of its own on every antenna,
# independent noise of sigma 6 per antenna, one broadband jammer (pure noise under a per-antenna phasor), summed, rounded, clipped to
# +-127.  The jammer level was chosen on the CPU before any device run: the scene from tests/simulate_oracle.py (fp64), the nulling
# oracle at block 4096, window 8, gain 1, int8 output, then oracle/frontend_oracle.py and the 20 ms search of oracle/acq_oracle.py over
# -5000 .. 5000 Hz in 200 Hz steps on the 25 ms from sample 36864 (the first sample of block W + 1).  PRN 17's true cell there: code
# 342.26, Doppler bin 1200 Hz; one sample is 0.25 chip.  Power is per component over the window.
#   jammer   antenna 0: metric, code, Doppler, power      nulled output (load_shift 10): metric, code, Doppler, power
#      0     8.20  342.42   1200            36.7            8.18  342.42  1200   36.7
#     10     4.21  342.42   1200           137.0            6.63  342.42  1200   47.4
#     20     2.32  342.42   1200           438.1            6.81  342.42  1200   48.4
#     30     1.59  547.22  -2400  (wrong)  939.7            6.84  342.42  1200   48.6
#     42     1.57  547.22  -2400  (wrong) 1797.6            6.83  342.42  1200   48.6      <- chosen
#     60     1.57  376.88   1400  (wrong) 3417.2            6.52  342.42  1200   50.0
# load_shift 8 / 10 / 12 at jammer 42: metric 6.81 / 6.83 / 6.83, power 48.6 each; at 60: 6.53 / 6.52 / 6.51, power 50.3 / 50.0 / 49.9.
# At amplitude 0.8 the nulled metric is 5.55 (jammer 42) and 5.30 (60).  No output component clipped in any row.
E2E = dict(signal="gps-l1", fs=4.092e6, prn=17, doppler=1250.0, code_phase=333.25, amp=1.0, sigma=6.0, jam=42.0, ms=20, block=4096, window=8,
           doppler_search=(-5000.0, 5000.0, 200.0),
           sat_phase=(0.0, 0.31, 0.62, 0.13), jam_phase=(0.0, 0.45, 0.83, 0.27), noise_seeds=(101, 102, 103, 104), jam_seed=900)
