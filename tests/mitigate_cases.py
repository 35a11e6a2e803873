"""Seeded inputs of the mitigation tests and their oracle results, computed once per process and shared read-only."""
import types

import numpy as np

import mitigate_oracle as O

SEED = 20261019
TILE = 8                                   # output blocks per workgroup of the excision kernel (the GPU test checks gacq_mitigate_tile)
TONE_AMP = float(np.sqrt(2000.0))          # 30 dB above the noise power 2 sigma^2, sigma = 1 per component
GAIN = 0.61

_REF = {}


def reference(key, make):
    """make() once per key"""
    if key not in _REF:
        _REF[key] = make()
    return _REF[key]


def tones(n, nfft, seed, in_complex64, first=0):
    """samples first .. first + n - 1 of unit Gaussian noise plus a tone on bin nfft / 8 and one 0.37 bins off bin -(nfft / 4 + 3), each 30
    dB above the noise: interleaved int8 (rounded) or complex64"""
    rng = np.random.Generator(np.random.PCG64([seed, nfft, n]))
    j = np.arange(first, first + n, dtype=np.float64)
    x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    x += TONE_AMP * np.exp(2j * np.pi * (nfft // 8) / nfft * j) + TONE_AMP * np.exp(-2j * np.pi * (nfft // 4 + 3 - 0.37) / nfft * j + 1.0j)
    if in_complex64:
        return x.astype(np.complex64)
    v = np.empty(2 * n, dtype=np.int8)
    v[0::2], v[1::2] = np.clip(np.rint(x.real), -127, 127), np.clip(np.rint(x.imag), -127, 127)
    return v


def _case(name, nfft, blocks, out_first=0, guard=2, in_complex64=False, in_at_need=False, seed=SEED, ratio=12.0, blank=None, hold=2):
    return types.SimpleNamespace(name=name, nfft=nfft, blocks=blocks, out_first=out_first, guard=guard, in_complex64=in_complex64,
                                 in_at_need=in_at_need, seed=seed, ratio=ratio, blank=blank, hold=hold)


def _excise_cases():
    out = []
    for nfft in (64, 128, 1024):
        h = nfft // 2
        firsts = (0, 5, h + 1)
        for i, nb in enumerate((1, TILE - 1, TILE, TILE + 1, 2 * TILE + 3)):
            out.append(_case("N%d blocks%d" % (nfft, nb), nfft, nb, firsts[i % 3], guard=(0, 2)[i % 2], in_complex64=bool((i + nfft // 64) % 2)))
        # the data starts at the first input the outputs need, not at sample 0
        out.append(_case("N%d input from in_first" % nfft, nfft, TILE + 1, 3 * h + 1, in_complex64=nfft == 128, in_at_need=True))
    out.append(_case("N4096 blocks3", 4096, 3, 5, in_complex64=True))
    return out


EXCISE_CASES = _excise_cases()
# seeds moved off SEED where the decision margin of the fp64 oracle came out below 1e-4 (test_mitigate_cpu.py holds every case to it)
SEEDS = {}


def cfg_of(c):
    return O.config(blank=c.blank, hold=c.hold, nfft=c.nfft, ratio=c.ratio, guard=c.guard)


def case_input(c):
    """(data, in_first, out_first, n_out) of an excision case"""
    cfg = cfg_of(c)
    h = c.nfft // 2
    n_out = c.blocks * h
    lo, hi = O.needed(cfg, c.out_first, n_out)
    in_first = lo if c.in_at_need else 0
    data = tones(hi + 1 - in_first, c.nfft, SEEDS.get(c.name, c.seed), c.in_complex64, in_first)
    return data, in_first, c.out_first, n_out


def case_reference(c):
    """(fp64 oracle result, value bound relative to max |y|, max |y|): the bound is four times the deviation of the float32
    evaluation of the definition from the fp64 oracle"""
    def make():
        data, in_first, out_first, n_out = case_input(c)
        ref = O.evaluate(cfg_of(c), data, GAIN, c.in_complex64, in_first, out_first, n_out)
        f32 = O.evaluate(cfg_of(c), data, GAIN, c.in_complex64, in_first, out_first, n_out, precision="f32")
        top = float(np.max(np.abs(ref.y)))
        dev = float(np.max(np.abs(f32.y - ref.y))) / top if top > 0 else 0.0
        assert np.array_equal(f32.frame_bins, ref.frame_bins), c.name
        return ref, 4.0 * dev, top
    return reference(("excise", c.name), make)


# ---- blanking alone
BLANK_SIZES = (1, 7, 8, 9, 4099)
BLANK_HOLDS = (0, 2, 64)
BLANK_THR = 90.0


def pulses(n, seed, in_complex64, extra=()):
    """n samples of Gaussian noise (sigma 12) with pulses of magnitude about 120 at samples 0, n - 1, a few seeded places and `extra`"""
    rng = np.random.Generator(np.random.PCG64([seed, n, 77]))
    x = 12.0 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    at = sorted(set([0, n - 1] + [int(v) for v in rng.integers(0, n, size=max(1, n // 300))] + [int(e) for e in extra if 0 <= e < n]))
    for a in at:
        x[a] = 120.0 * np.exp(1j * rng.uniform(0, 2 * np.pi))
    if in_complex64:
        return x.astype(np.complex64)
    v = np.empty(2 * n, dtype=np.int8)
    v[0::2], v[1::2] = np.clip(np.rint(x.real), -127, 127), np.clip(np.rint(x.imag), -127, 127)
    return v


# ---- the interference scene of the end-to-end tests: GPS L1 C/A PRN 7 under a chirped CW and a pulse train
SCENE = dict(fs=4.096e6, prn=7, amp=1.0, sigma=4.0, doppler=1234.5, code0=417.3, cw_amp=60.0, cw_hz=317.0e3, cw_rate=2.0e6, pulse_amp=110.0,
             pulse_len=24, pulse_period=1000, pulse_hz=-523.0e3, ms=4, blank=85.0, hold=2, nfft=1024, ratio=12.0, guard=2, noise_prn=25)


def interference(j, fs=SCENE["fs"]):
    """the CW and the pulse train at sample indices j (fp64 numpy)"""
    s = SCENE
    t = j / fs
    cw = s["cw_amp"] * np.exp(2j * np.pi * (s["cw_hz"] * t + 0.5 * s["cw_rate"] * t * t))
    on = ((j.astype(np.int64) + 400) % s["pulse_period"]) < s["pulse_len"]
    return cw + np.where(on, s["pulse_amp"] * np.exp(2j * np.pi * s["pulse_hz"] * t + 0.7j), 0.0)


def scene_int8(chips, seed=SEED, ms=None):
    """the scene as interleaved int8, 4 ms unless told otherwise: amp c(j) exp(2 pi i doppler j / fs) + noise + interference, rounded and clipped"""
    s = SCENE
    n = int(s["fs"] * 1e-3) * (s["ms"] if ms is None else ms)
    rng = np.random.Generator(np.random.PCG64(seed))
    j = np.arange(n, dtype=np.float64)
    chip = np.floor(s["code0"] + j * ((1.023e6 + s["doppler"] / 1540.0) / s["fs"])).astype(np.int64) % len(chips)
    x = s["amp"] * (1.0 - 2.0 * np.asarray(chips, dtype=np.float64)[chip]) * np.exp(2j * np.pi * s["doppler"] * j / s["fs"])
    x = x + s["sigma"] * (rng.standard_normal(n) + 1j * rng.standard_normal(n)) + interference(j)
    v = np.empty(2 * n, dtype=np.int8)
    v[0::2], v[1::2] = np.clip(np.rint(x.real), -127, 127), np.clip(np.rint(x.imag), -127, 127)
    return v


def scene_cfg():
    s = SCENE
    return O.config(blank=s["blank"], hold=s["hold"], nfft=s["nfft"], ratio=s["ratio"], guard=s["guard"])


SCENE_DOPPLERS = [-2000.0, 2000.0, 200.0]
