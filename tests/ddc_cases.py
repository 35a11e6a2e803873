"""Seeded inputs and sizes of the down-converter tests, and their oracle results, computed once per process and shared read-only."""
import types

import numpy as np

import ddc_oracle as O

SEED = 20261019
FS = 69.984e6
GAIN = 0.61

_REF = {}


def reference(key, make):
    """make() once per key"""
    if key not in _REF:
        _REF[key] = make()
    return _REF[key]


def tile(D):
    """outputs one workgroup owns (the tests check gacq_ddc_tile against it)"""
    return 1024 if D <= 8 else 512 if D <= 16 else 256 if D <= 32 else 128


def random_taps(T, seed=SEED):
    """asymmetric taps with sum |g| = 65536 exactly"""
    rng = np.random.Generator(np.random.PCG64([seed, T]))
    g = rng.integers(-2000, 2001, size=T).astype(np.int64)
    g[g == 0] = 1
    g = g * (60000 // int(np.abs(g).sum()))
    g[T // 3] += (65536 - int(np.abs(g).sum())) * (1 if g[T // 3] > 0 else -1)
    assert int(np.abs(g).sum()) == 65536 and not np.array_equal(g, g[::-1])
    return g


# (D, T): T = 1 at D = 1 and 8 D + 1 elsewhere are the default designs; the others take the default cutoff at their length
SHAPES = [(1, 1), (1, 17), (2, 17), (3, 25), (8, 65), (16, 129), (64, 513), (5, 3)]


def _tap_sets():
    out = []
    for D, T in SHAPES:
        out.append(types.SimpleNamespace(name="D%d T%d" % (D, T), D=D, taps=O.design_taps(D, T)))
    out.append(types.SimpleNamespace(name="D4 T41 random", D=4, taps=random_taps(41)))
    return out


TAP_SETS = _tap_sets()

# shifts: an exact ratio (dP = 2^61), one just below zero (every high bit of dP set), one without an exact ratio
SHIFTS = (FS / 8.0, -1.0e-3, 1.2345678e6)


def sizes(D):
    t = tile(D)
    return (1, 7, t - 1, t, t + 1, 2 * t + 3)


def starts(D, T, kind):
    """(in_first, out_first): 0: the recording's start, whose history is zero; 1: an input that starts just where the outputs need it,
    both indices off every wide load's alignment; 2: the same near 2^40, where n dP has wrapped many times"""
    H = T // 2
    if kind == 0:
        return 0, 0
    base = 3 if kind == 1 else (1 << 40) - 5
    out_first = -(-(base + H) // D) + (3 if kind == 1 else 1)
    return out_first * D - H, out_first


def random_int8(n, seed):
    rng = np.random.Generator(np.random.PCG64([SEED, seed, n]))
    v = rng.integers(-128, 128, size=2 * n).astype(np.int8)
    k = min(4, len(v))
    v[:k] = (-128, -128, 127, -128)[:k]
    return v


def case(ts, i):
    """size i of a tap set: (data, in_first, out_first, n_out, f_shift)"""
    T = len(ts.taps)
    n_out = sizes(ts.D)[i]
    in_first, out_first = starts(ts.D, T, i % 3)
    lo, hi = O.needed(ts.D, T, out_first, n_out)
    assert in_first <= lo
    return random_int8(hi + 1 - in_first, 100 * ts.D + i), in_first, out_first, n_out, SHIFTS[(i + ts.D) % 3]


def case_reference(ts, i):
    def make():
        data, in_first, out_first, n_out, f_shift = case(ts, i)
        c = O.evaluate(f_shift, FS, ts.D, ts.taps, data, GAIN, in_first, out_first, n_out, "complex64")
        return c, O.to_int8(c)
    return reference((ts.name, i), make)


# ---- the scene of the end-to-end tests: one GPS L1 C/A satellite 4.092 MHz above the centre of a 32.736 MS/s recording
# 32 samples a chip: the code phase at sample 0 is fixed to 1 / 32 chip, and the truth is that interval's middle (tests/ingest_cases.py)
SCENE = dict(fs=32.736e6, coffset=4.092e6, prn=7, amp=3.0, sigma=12.0, doppler=1234.5, code0=417.0 + 10.5 / 32.0, noise_prn=25, D=8)


def scene_int8(chips, n, seed=SEED):
    """the scene in plain numpy fp64 as interleaved int8: amp c(j) exp(2 pi i (coffset + doppler) j / fs) + Gaussian noise, rounded"""
    s = SCENE
    rng = np.random.Generator(np.random.PCG64(seed))
    j = np.arange(n, dtype=np.float64)
    chip = np.floor(s["code0"] + j * ((1.023e6 + s["doppler"] / 1540.0) / s["fs"])).astype(np.int64) % len(chips)
    x = s["amp"] * (1.0 - 2.0 * np.asarray(chips, dtype=np.float64)[chip]) * np.exp(2j * np.pi * np.mod((s["coffset"] + s["doppler"]) * j / s["fs"], 1.0))
    x = x + s["sigma"] * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    v = np.empty(2 * n, dtype=np.int8)
    v[0::2], v[1::2] = np.clip(np.rint(x.real), -127, 127), np.clip(np.rint(x.imag), -127, 127)
    return v
