"""Seeded inputs shared by tests/test_ingest_cpu.py and tests/test_ingest_gpu.py, and the oracle results of the device cases, each
computed once and left as it is.

Sizes: a lane of the kernels owns 8 output samples and a workgroup of the real-IF kernel a tile of 2048, so 1, 7, 8, 9 and 4099 I/Q
samples and 1, 2047, 2048, 2049 and 5000 real-IF outputs cover a partial run, a whole one, one more, more than one workgroup and
both sides of the tile edge."""
import numpy as np

import ingest_oracle as O

SEED = 20261019

# I/Q: format name -> gain (so that the int8 output neither stays tiny nor clips everywhere)
IQ_GAIN = {"s8": 0.73, "u8": 0.73, "s16": 0.0031, "f32": 1.7, "1ob": 21.3, "2sm": 9.7, "2ob": 9.7, "4tc": 5.3}
IQ_SIZES = (1, 7, 8, 9, 4099)
IQ_FIRST = (16, 21)                       # in_first, out_first of the offset case: 5 samples in, which is mid-byte for the packed ones
PACKED_LUT = {1: [5, -7], 2: [-9, 2, 11, -4], 4: [3, -5, 7, -9, 11, -13, 15, -17, 19, -21, 23, -25, 27, -29, 31, -128]}

REAL_GAIN = {"s8": 0.61, "u8": 0.61, "2sm": 9.3, "1sm": 17.9}
REAL_OUT_FIRST = (0, 1, 5, 10, 11, 12, 1001)
REAL_N_OUT = (1, 2047, 2048, 2049, 5000)
REAL_IN_FIRST_1001 = 1976                 # a multiple of 16 at or below 2 * 1001 - 21: the input of that case starts there

CUT_N, CUT_PIECES = 20000, (4099, 1, 15900)
FEED_CHUNKS = (1, 3, 4097)                # bytes; then the rest: they cut an s16 sample, an f32 sample and a byte of packed codes


def raw(name, nbytes, seed=SEED):
    """nbytes seeded input bytes of a container: every byte value for the integer ones, Gaussian floats (sigma 20) for f32"""
    rng = np.random.Generator(np.random.PCG64([seed, sum(map(ord, name)), nbytes]))
    if name == "f32":
        return (20.0 * rng.standard_normal(nbytes // 4 + 1)).astype("<f4").tobytes()[:nbytes]
    return rng.integers(0, 256, size=nbytes, dtype=np.uint8).tobytes()


def iq_bytes(f, nsamples):
    return -(-nsamples * O.sample_bits(f) // 8)


def real_bytes(f, in_first, out_first, n_out):
    """bytes that hold input samples in_first .. 2 (out_first + n_out - 1) + 21"""
    return -(-(2 * (out_first + n_out - 1) + O.HALF + 1 - in_first) * O.sample_bits(f) // 8)


_REF = {}


def reference(key, make):
    """make() once per key; the arrays are shared and read-only"""
    if key not in _REF:
        out = make()
        out.setflags(write=False)
        _REF[key] = out
    return _REF[key]


def gaussian_recordings():
    """name -> (oracle format, bytes) of the automatic-gain cases: 16-bit I/Q of sigma 1000 and real 2-bit sign / magnitude codes of
    Gaussian samples with the threshold at sigma, 70000 output samples' worth each"""
    if "gaussian" not in _REF:
        rng = np.random.Generator(np.random.PCG64(SEED))
        s16 = np.clip(np.rint(1000.0 * rng.standard_normal(2 * 70000)), -32768, 32767).astype("<i2").tobytes()
        two = pack_msb_first(quantise_2sm(12.0 * rng.standard_normal(2 * 70000 + 64), 12.0), 2).tobytes()
        _REF["gaussian"] = {"s16": (O.fmt("s16"), s16), "2sm real": (O.fmt("2sm", real=True), two)}
    return _REF["gaussian"]


# the end-to-end scene: GPS L1 C/A sampled real at 8.184 MS/s with the carrier at fs/4 + Doppler, quantised to two bits (sign and
# magnitude, threshold at sigma), four codes per byte, first code in the top bits.
# The code phase: this plan samples the code at exactly 8 samples per chip (but for the code Doppler, 0.8 chip/s here), so every code
# phase within one eighth of a chip gives the same chips at the same samples until the drift carries an edge across a sample -- the
# recording itself fixes the phase at sample 0 only to that interval, and an estimate can be held to 0.03 chip of the truth only
# where the truth is the interval's middle: 417 + 2.5 / 8.
SCENE = dict(fs=8.184e6, if_hz=2.046e6, prn=7, amp=6.0, sigma=12.0, doppler=1234.5, code0=417.3125, noise_prn=25)


def quantise_2sm(x, threshold):
    """codes of real samples: sign bit 1 negative, magnitude bit 1 above the threshold"""
    x = np.asarray(x)
    return ((x < 0).astype(np.uint8) << 1) | (np.abs(x) > threshold).astype(np.uint8)


def pack_msb_first(codes, bits):
    per = 8 // bits
    c = np.asarray(codes, dtype=np.uint8)
    c = np.concatenate([c, np.zeros(-len(c) % per, dtype=np.uint8)]).reshape(-1, per)
    out = np.zeros(len(c), dtype=np.uint8)
    for i in range(per):
        out |= c[:, i] << (8 - bits * (i + 1))
    return out


def scene_real_samples(chips, n, seed=SEED):
    """the scene in plain numpy fp64: amp c(n) cos(2 pi (IF + Doppler) n / fs) + Gaussian noise"""
    s = SCENE
    rng = np.random.Generator(np.random.PCG64(seed))
    j = np.arange(n, dtype=np.float64)
    chip = np.floor(s["code0"] + j * ((1.023e6 + s["doppler"] / 1540.0) / s["fs"])).astype(np.int64) % len(chips)
    c = 1.0 - 2.0 * np.asarray(chips, dtype=np.float64)[chip]
    return s["amp"] * c * np.cos(2.0 * np.pi * np.mod((s["if_hz"] + s["doppler"]) * j / s["fs"], 1.0)) + s["sigma"] * rng.standard_normal(n)
