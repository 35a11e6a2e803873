"""Cases shared by the beams tests (test_beams_cpu.py, test_beams_gpu.py).  Beam k of a case is tests/nulling_oracle.py under constraint
c_k and gain_k, so there is no oracle of its own: recordings from nulling_cases.recording, K constraints per case, the oracle's
results per (case, beam) computed once, and the rounding-tie margin of every beam of every case -- equality of the quantised weights
is claimed only where no scaled weight component lies within nulling_cases.MARGIN of a half-integer; check_margins() asserts it, so
the seeds below were chosen on the CPU.

The grid: M in {2, 3, 8} x K in {1, 2, 8, 9, 16} (1 degenerate, 8 fills a group of right-hand sides, 9 crosses it, 16 the maximum),
every (M, K) pair under two of the six (Lb, W) of {64, 128, 4096} x {1, 3}, so that every value of every axis occurs: 30 cases.
Seeds: 7000 + the case's index in the grid; none was rejected.  Smallest margin over all beams of all 34 cases: SMALLEST_MARGIN below
(test_beams_cpu.py asserts that check_margins() still finds it).  The end-to-end scene and the CPU experiment that fixed its one
free level are at the end of the file."""
import functools

import numpy as np

import nulling_cases as NC
import nulling_oracle as O

TILE, RUN, MARGIN = NC.TILE, NC.RUN, NC.MARGIN
LOAD_SHIFT = 10
REJECTED_SEEDS = ()                                 # seeds tried and dropped for a margin under MARGIN
SMALLEST_MARGIN = 6.975103497097734e-05            # ("long-m3-k9-b192-w2", beam 5)

_COMBOS = [(64, 1), (128, 3), (4096, 1), (64, 3), (128, 1), (4096, 3)]

# name -> (M, K, Lb, W, seed, kind); kind: "noise", "min" (every component -128), "twin" (beams 1 and 2 identical), "shared" (antennas 0
# and 2 one array), "long" (longer than a workgroup tile of the apply kernel; 192 does not divide the tile)
CASES = {}
_i = 0
for _M in (2, 3, 8):
    for _K in (1, 2, 8, 9, 16):
        for _Lb, _W in _COMBOS[2 * (_i % 3):2 * (_i % 3) + 2]:
            CASES["m%d-k%d-b%d-w%d" % (_M, _K, _Lb, _W)] = (_M, _K, _Lb, _W, 7000 + len(CASES), "noise")
        _i += 1
CASES["min-m8-k16-b128-w3"] = (8, 16, 128, 3, 7100, "min")
CASES["twin-m3-k3-b64-w3"] = (3, 3, 64, 3, 7101, "twin")
CASES["shared-m3-k2-b128-w3"] = (3, 2, 128, 3, 7102, "shared")
CASES["long-m3-k9-b192-w2"] = (3, 9, 192, 2, 7103, "long")


def steer(M, seed):
    """beam 1: nulling_cases.STEER, which has five entries, continued for M = 8 by three seeded ones of modulus 0.3..1.5"""
    rng = np.random.default_rng(seed + 50000)
    more = rng.uniform(0.3, 1.5, 3) * np.exp(2j * np.pi * rng.uniform(0.0, 1.0, 3))
    return np.concatenate([NC.STEER, more])[:M]


@functools.lru_cache(maxsize=None)
def constraints(name):
    """K complex vectors [K][M]: the default (1, 0, .., 0), steer(), then seeded vectors with entries of modulus 0.3..1.5"""
    M, K, Lb, W, seed, kind = CASES[name]
    cs = [O.default_constraint(M), steer(M, seed)]
    for k in range(2, K):
        rng = np.random.default_rng(100 * seed + k)
        cs.append(rng.uniform(0.3, 1.5, M) * np.exp(2j * np.pi * rng.uniform(0.0, 1.0, M)))
    if kind == "twin":
        cs[2] = cs[1]
    cs = np.array(cs[:K])
    cs.setflags(write=False)
    return cs


def gains(name):
    """a different clipping gain for every beam of an int8 output"""
    return [6.5 + 0.25 * k for k in range(CASES[name][1])]


@functools.lru_cache(maxsize=None)
def data(name):
    M, K, Lb, W, seed, kind = CASES[name]
    N = TILE + 5 * Lb + 37 if kind == "long" else NC.length(Lb, W)
    if kind == "min":
        return tuple(np.full(2 * N, -128, dtype=np.int8) for _ in range(M))
    xs = NC.recording(M, N, seed)
    if kind == "shared":
        xs[2] = xs[0]
    return tuple(xs)


@functools.lru_cache(maxsize=None)
def reference(name, k, complex64=False):
    """the nulling oracle on the whole recording of a case under beam k's constraint: int8 at gains(name)[k], complex64 at gain 1"""
    M, K, Lb, W, seed, kind = CASES[name]
    xs = data(name)
    return O.run(list(xs), 0, 0, len(xs[0]) // 2, Lb, W, LOAD_SHIFT, constraints(name)[k], 1.0 if complex64 else gains(name)[k], complex64)


@functools.lru_cache(maxsize=None)
def check_margins():
    """(name, k) -> margin, after asserting the margin of every beam of every case"""
    out = {}
    for name in CASES:
        for k in range(CASES[name][1]):
            out[name, k] = reference(name, k)["margin"]
            assert out[name, k] >= MARGIN, (name, k, out[name, k])
    return out


# ---- the end-to-end scene: bearing_cases.ring(4), GPS L1 C/A at 4.092 MS/s, noise of sigma 6 per antenna, PRNs 5, 9 and 21 from
# arrayprompt_cases.DIRECTIONS at one common amplitude, a noise jammer of 42 per component from (az 70, el 20); block 4096, window 8,
# load_shift 10, gain 1, int8 outputs.  Beam 0 is the default constraint (power inversion), beam 1 + i the true scene.steering vector of
# satellite i scaled to entry 0 = 1.  The 20 ms search over -5000 .. 5000 Hz in 200 Hz steps runs on the 25 ms from sample 36864 (the
# first sample of block W + 1).  True cells there: PRN 5 code 342.26 bin 1200, PRN 9 code 110.49 bin -2400, PRN 21 code 786.77 bin 3000
# (one sample is 0.25 chip; the Dopplers sit a quarter bin off the grid).
# The satellites' amplitude was fixed on the CPU before any device run, by e2e_cpu_rows() below: tests/scene_oracle.py (fp64, seed 411)
# -> nulling_oracle.run per beam -> oracle/frontend_oracle.py -> oracle/acq_oracle.py.  Per PRN: metric, code, Doppler bin, and the
# power per component over the window; antenna 0's power is 1781 +- 1 in every row and it misses every PRN at every amplitude (metric
# 1.50 .. 1.63).  No output component clipped in any row.
#   amp   PRN   power inversion (beam 0)             the PRN's own beam
#   1.0    5    4.19  342.42   1200        51.3      12.68  342.42   1200  13.3
#          9   10.97  110.39  -2400        51.3      11.30  110.39  -2400  16.5
#         21    9.46  786.98   3000        51.3      12.01  786.98   3000  13.6
#   0.7    5    3.08  342.42   1200        49.8       9.20  342.42   1200  13.0
#          9    8.09  110.39  -2400        49.8       8.32  110.39  -2400  16.1
#         21    6.94  786.98   3000        49.8       8.79  786.98   3000  13.3
#   0.5    5    2.29  342.42   1200        49.1       6.76  342.42   1200  12.8
#          9    6.00  110.39  -2400        49.1       6.17  110.39  -2400  15.9
#         21    5.10  786.98   3000        49.1       6.47  786.98   3000  13.1
#   0.35   5    1.67  342.42   1200        48.7       4.81  342.42   1200  12.8
#          9    4.34  110.39  -2400        48.7       4.43  110.39  -2400  15.8
#         21    3.66  786.98   3000        48.7       4.63  786.98   3000  13.0
#   0.25   5    1.58  954.82   2400 (wrong) 48.6      3.49  342.42   1200  12.7      <- chosen: the largest scanned amplitude at which
#          9    3.21  110.39  -2400        48.6       3.27  110.39  -2400  15.7         power inversion puts a PRN into a wrong cell
#         21    2.69  786.98   3000        48.6       3.42  786.98   3000  13.0         while every beam finds its own
# What the table shows of the array algebra: power inversion protects antenna 0 alone and happens to put a shallow null near PRN 5
# (its metric is a third of its beam's); toward PRN 9 it loses almost nothing.  A beam's output power is a quarter of the power
# inversion output's, its metric up to three times as large.
E2E = dict(signal="gps-l1", fs=4.092e6, prns=(5, 9, 21), dopplers=(1250.0, -2350.0, 3050.0), code_phases=(333.25, 101.5, 777.75), amp=0.25,
           sigma=6.0, jammer=(42.0, 70.0, 20.0), seed=411, ms=20, block=4096, window=8, doppler_search=(-5000.0, 5000.0, 200.0), missed=(5,))


def e2e_scene():
    """(satellites, emitters, gains [4, 4], constraints [4][4], first sample of the search, samples) of the end-to-end scene"""
    import arrayprompt_cases
    import bearing_cases
    from gnss_dsp_tools_amd import scene, simulate
    E = E2E
    el = bearing_cases.ring(4)
    st = [scene.steering(el, az, e) for az, e in arrayprompt_cases.DIRECTIONS]
    gains = np.stack(st + [scene.steering(el, E["jammer"][1], E["jammer"][2])], axis=1)
    sats = [simulate.Satellite(E["signal"], prn, E["amp"], dop, cp) for prn, dop, cp in zip(E["prns"], E["dopplers"], E["code_phases"])]
    w0 = (E["window"] + 1) * E["block"]
    return sats, [scene.NoiseJammer(E["jammer"][0])], gains, [None] + [s / s[0] for s in st], w0, w0 + int(E["fs"] * 0.001 * (E["ms"] + 5)) + 8


def e2e_true_cell(sat, w0):
    """(code phase at sample w0 in chips, Doppler bin) of a satellite of the scene"""
    E = E2E
    return (sat.code0 + w0 * sat.code_rate_hz() / E["fs"]) % 1023.0, E["doppler_search"][2] * round(sat.doppler / E["doppler_search"][2])


def e2e_hit(result, sat, w0):
    """whether a (metric, code, Doppler) result lies in the satellite's true cell: the Doppler bin, the code within one sample"""
    code, dop = e2e_true_cell(sat, w0)
    return result[2] == dop and abs((result[1] - code + 511.5) % 1023.0 - 511.5) <= 1.023e6 / E2E["fs"]


def e2e_cpu_rows(amp=None):
    """the rows of the table above at one amplitude: PRN -> {"pi": (metric, code, Doppler, power), "beam": (..)}, all on the CPU"""
    import scene_oracle
    import simulate_cases
    import simulate_oracle
    from gnss_dsp_tools_amd import signals
    from oracle import acq_oracle, frontend_oracle
    E = dict(E2E, amp=E2E["amp"] if amp is None else amp)
    sats, _, gains, cs, w0, n = e2e_scene()
    sats = [type(s)(s.tracker, s.item, E["amp"], s.doppler, s.code0) for s in sats]
    v = scene_oracle.evaluate(simulate_cases.oracle_sats(sats, 0.0), [dict(kind=scene_oracle.NOISE, amp=E["jammer"][0])], gains, E["fs"], E["sigma"],
                              E["seed"], 0, 0, n)
    xs = [simulate_oracle.to_int8(v[p]) for p in range(4)]
    outs = [O.run(xs, 0, 0, n, E["block"], E["window"], LOAD_SHIFT, c, 1.0, False) for c in cs]
    assert not any(o["clipped"] for o in outs)
    sig = signals.get(E["signal"])

    def cell(y, prn):
        x = frontend_oracle.condition(frontend_oracle.iq_to_complex(y[2 * w0:].reshape(-1, 2)), E["fs"], 0.0, sig, E["ms"] + 5)
        return tuple(acq_oracle.search_script(E["signal"], x, prn, list(E["doppler_search"]), E["ms"])) + (float(np.mean(y[2 * w0:].astype(np.float64) ** 2)),)

    return {s.item: {"pi": cell(outs[0]["out"], s.item), "beam": cell(outs[1 + k]["out"], s.item)} for k, s in enumerate(sats)}, sats, w0
