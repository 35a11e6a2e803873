"""Cases shared by the space-time nulling tests (test_stap_cpu.py, test_stap_gpu.py): the recordings of nulling_cases.recording
(asymmetric between the antennas and between I and Q, with planted -128 / 127), the (antennas, taps) shapes they run under, their oracle
results (computed once, never changed) and the rounding-tie margin of every case -- equality of the quantised weights is claimed only
where no scaled weight component lies within 1e-6 of a half-integer; check_margins() asserts that of every block of every case, so the
seeds below were chosen on the CPU."""
import functools

import numpy as np

import nulling_cases as NC
import stap_oracle as O

MARGIN = NC.MARGIN
TILE = NC.TILE                                      # gacq_stap_tile: samples a workgroup of the apply kernel owns
RUN = NC.RUN                                        # samples of a lane's run

# (M, T): one and two 16-row tiles, a partial tile, T = 1 (gacq_null's computation), the most taps, the most weights (56: seven tiles)
SHAPES = [(1, 3), (1, 15), (2, 1), (2, 5), (3, 3), (5, 5), (4, 13), (8, 1), (8, 7)]
REDUCED = [(1, 15), (3, 3), (8, 7)]

# name -> (M, T, Lb, W, seed, kind); kind: "noise" (recording), "min" (every component -128), "shared" (antennas 0 and 2 one array),
# "steer" (a non-default constraint), "long" (longer than a workgroup tile of the apply kernel)
CASES = {}
for _M, _T in SHAPES:
    CASES["m%d-t%d-b128-w3" % (_M, _T)] = (_M, _T, 128, 3, 3000 + 100 * _M + _T, "noise")
for _M, _T in REDUCED:
    for _Lb in (64, 4096):
        CASES["m%d-t%d-b%d-w1" % (_M, _T, _Lb)] = (_M, _T, _Lb, 1, 4000 + 100 * _M + _T + _Lb % 997, "noise")
CASES["m8-t7-b64-w1"] = (8, 7, 64, 1, 4872, "noise")        # the seed of the rule leaves a margin of 7.9e-7
CASES["min-m8-t7-b32768-w1"] = (8, 7, 32768, 1, 0, "min")
CASES["shared-m3-t3-b128-w3"] = (3, 3, 128, 3, 77, "shared")
CASES["steer-m5-t5-b128-w3"] = (5, 5, 128, 3, 78, "steer")
# 192 does not divide the tile, 4096 puts a block edge on the tile's
CASES["long-m3-t3-b128-w3"] = (3, 3, 128, 3, 80, "long")
CASES["long-m8-t7-b4096-w1"] = (8, 7, 4096, 1, 81, "long")
CASES["long-m1-t15-b192-w2"] = (1, 15, 192, 2, 82, "long")
STEER = NC.STEER
OUTPUT_CASES = ["m1-t3-b128-w3", "m2-t5-b128-w3", "m3-t3-b4096-w1", "m4-t13-b128-w3", "shared-m3-t3-b128-w3", "steer-m5-t5-b128-w3"]
NULLING_SHAPES = [2, 5, 8]                          # T = 1 beside a Nuller run


def constraint(name):
    return STEER if CASES[name][5] == "steer" else None


@functools.lru_cache(maxsize=None)
def data(name):
    M, T, Lb, W, seed, kind = CASES[name]
    if kind == "min":
        return tuple(np.full(2 * ((W + 1) * Lb + 40), -128, dtype=np.int8) for _ in range(M))
    N = TILE + 5 * Lb + 37 if kind == "long" else NC.length(Lb, W)
    xs = NC.recording(M, N, seed)
    if kind == "shared":
        xs[2] = xs[0]
    return tuple(xs)


def outputs(name):
    """the outputs a case's recording supports: all but the last t_c"""
    return len(data(name)[0]) // 2 - O.centre(CASES[name][1])


@functools.lru_cache(maxsize=None)
def reference(name, complex64=False, gain=1.0):
    """the oracle on the whole recording of a case"""
    M, T, Lb, W, seed, kind = CASES[name]
    return O.run(list(data(name)), 0, 0, outputs(name), Lb, W, T, 10, constraint(name), gain, complex64)


def check_margins():
    """name -> margin, after asserting the margin of every case"""
    out = {}
    for name in CASES:
        out[name] = reference(name)["margin"]
        assert out[name] >= MARGIN, (name, out[name])
    return out


def cuts(Lb, W, N, tile=TILE):
    """where calls end and start: nulling_cases.cuts -- a workgroup tile, a block edge, one lane's run before and after each, odd places"""
    return NC.cuts(Lb, W, N, tile)


# ---- the end-to-end scenes: GPS L1 C/A at 4.092 MS/s, PRN 17 at amplitude 1 (Doppler 1250 Hz, code phase 333.25 at sample 0) with a
# carrier phase of its own on every antenna, independent noise of sigma 6 per antenna, tones amp exp(2 pi i (j num / den + step p)) on
# antenna p (num / den of the sample rate: 155 / 2046 is +310 kHz, -45 / 341 is -540 kHz), in scene (b) one broadband jammer (pure noise
# under a per-antenna phasor); summed, rounded, clipped to +-127.  The levels were fixed on the CPU before any device run: the scene from
# tests/simulate_oracle.py (fp64), tests/stap_oracle.py at block 4096, window 8, load_shift 10, gain 1, int8 output, then
# oracle/frontend_oracle.py and the 20 ms search of oracle/acq_oracle.py over -5000 .. 5000 Hz in 200 Hz steps on the 25 ms from sample
# 36864 (the first sample of block W + 1).  PRN 17's true cell there: code 342.26, Doppler bin 1200 Hz; one sample is 0.25 chip.  Each
# entry: metric, code, Doppler; power is per component over the window.  No output component clipped in any row but those marked.
#
# (a) one antenna, two tones:
#   tones   input                          T = 5                              T = 9                              T = 15
#     20    2.62 886.88 3400 wrong  437    4.40 342.91 1200 wrong  60.9      6.71 342.42 1200 true 47.7         6.66 342.42 1200 true 42.6
#     30    2.62 886.88 3400 wrong  937    4.81 342.91 1200 wrong  61.7      6.68 342.42 1200 true 47.9  <-     6.63 342.42 1200 true 42.7
#     45    2.63 126.13 1400 wrong 2062    5.00 342.91 1200 wrong  62.2      6.69 342.42 1200 true 48.0         6.65 342.42 1200 true 42.7
#   (five taps find the Doppler bin and miss the code by 0.65 chip: the short filter's group delay across the band is not flat)
#
# (b) three antennas, a jammer and two tones.  The directions matter as much as the levels: with the tones at steps 0.17 / 0.38 and the
# jammer at (0, 0.45, 0.83), close to the satellite's (0, 0.31, 0.62), the weights that null them attenuate the satellite as well and T = 3
# reaches 1.56 .. 3.5 only.  With the tones at steps 0.55 / 0.8 and the jammer at (0, 0.05, 0.1):
#   jammer tones   antenna 0                      T = 1 (what nulling.py computes)                T = 3
#     25    40     2.48 404.35  2600 wrong 2252   2.71 342.42  1000 wrong 1546 (29 clipped)       10.78 342.42 1200 true  76.8
#     25    50     2.54 404.35  2600 wrong 3117   2.37 506.75  -400 wrong 2025 (435 clipped)      10.35 342.42 1200 true  81.0   <- chosen
#     25    60     2.57 403.11  2600 wrong 4091   2.31 506.75  -400 wrong 2377 (1384 clipped)      9.04 342.42 1200 true  99.8
#     35    50     2.44 404.35  2600 wrong 3600   2.49 404.60  2600 wrong 2449 (682 clipped)       9.16 342.42 1200 true 104.7
#     40    60     2.45 404.35  2600 wrong 4695   2.50 805.21 -3400 wrong 3205 (3362 clipped)      6.47 342.42 1200 true 193.0
#   (at 40 the single tap's miss is by one Doppler bin only; from 50 on it lands in a far cell.  The input itself clips at these levels.)
_E2E = dict(signal="gps-l1", fs=4.092e6, prn=17, doppler=1250.0, code_phase=333.25, amp=1.0, sigma=6.0, ms=20, block=4096, window=8,
            doppler_search=(-5000.0, 5000.0, 200.0))
E2E_TONES = dict(_E2E, antennas=1, taps=9, jam=0.0, tones=((30.0, 155, 2046, 0.0), (30.0, -45, 341, 0.0)), sat_phase=(0.0,), jam_phase=(0.0,),
                 noise_seeds=(101,), jam_seed=900)
E2E_ARRAY = dict(_E2E, antennas=3, taps=3, jam=25.0, tones=((50.0, 155, 2046, 0.55), (50.0, -45, 341, 0.8)), sat_phase=(0.0, 0.31, 0.62),
                 jam_phase=(0.0, 0.05, 0.1), noise_seeds=(101, 102, 103), jam_seed=900)
