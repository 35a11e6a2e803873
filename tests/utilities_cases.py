"""Shared by the utilities tests and tools/make_goldens_utilities.py: the case specifications, the seeded recordings (regenerated,
never committed: one squaring chunk alone is 3.2 MB) and the golden file tests/golden/utilities_cases.json.gz."""
import base64
import gzip
import hashlib
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
GOLDEN_FILE = os.path.join(GOLD, "utilities_cases.json.gz")

SEED = 20261017

# spectrum: case -> (n, ns, frames, fc, fs).  Every power of two the kernel takes, ns from 1 to 200, and one length (1000) that
# goes through torch.fft.  Recording: noise sigma 18 per component plus two tones, rounded and clipped to int8.
SPECTRUM = {
    "n64": (64, 200, 2, 1575.42e6, 4.0e6),
    "n128": (128, 1, 3, 1575.42e6, 4.0e6),
    "n256": (256, 7, 2, 1227.6e6, 8.0e6),
    "n512": (512, 50, 1, 1227.6e6, 8.0e6),
    "n1024": (1024, 17, 2, 1176.45e6, 20.0e6),
    "n2048": (2048, 50, 1, 1584754875.0, 69984000.0),
    "n4096": (4096, 20, 1, 1584754875.0, 69984000.0),
    "n8192": (8192, 9, 1, 1227727126.0, 69984000.0),
    "n16384": (16384, 8, 1, 1227727126.0, 69984000.0),
    "n1000": (1000, 10, 2, 1575.42e6, 5.0e6),
}
SPECTRUM_TONES = ((0.1234, 9.0), (-0.3071, 4.0))          # (cycles per sample, amplitude)
SPECTRUM_SIGMA = 18.0

# squaring: case -> (b, n, m, chunks, fs, coffset).  "script" is squaring.py's own (b, n, m) over three chunks with a coffset for
# which chunk * coffset / fs is not an integer (the start phase of chunks 1 and 2 is 0.3525..., 0.7051...); the others cover n not a
# power of two, n not a multiple of 8 (the narrow loads) and m above the workgroup size.
SQUARING = {
    "script": (1000, 16, 100, 3, 69984000.0, -9334875.0),
    "n12": (50, 12, 7, 4, 69984000.0, 1234567.0),
    "n5": (20, 5, 33, 2, 4.0e6, -1.0e6 / 3.0),
    "n8_m300": (7, 8, 300, 3, 16.368e6, 4.092e6 + 17.0),
}
# the int16 stream may differ from the reference's by one where the reference's own 20 r lies this many measured differences from a
# half-integer, on at most this share of the positions
HALF_FACTOR = 10.0
HALF_SHARE = 0.05

# cn0: --time values for the golden track cases (11 to 60 lines each) and the seeded synthetic track (2000 lines)
CN0_TRACK_TIME = 5
CN0_SYNTH = {"lines": 2000, "times": (300, 100, 2000)}


def _rng(tag):
    return np.random.Generator(np.random.PCG64([SEED, int(hashlib.sha256(tag.encode()).hexdigest()[:8], 16)]))


def spectrum_recording(case):
    """flat interleaved int8 I/Q, frames * ns * n samples plus half a frame that every reader must drop"""
    n, ns, frames, _, _ = SPECTRUM[case]
    nsamp = frames * ns * n + n // 2
    rng = _rng("spectrum/" + case)
    x = rng.normal(0.0, SPECTRUM_SIGMA, size=(nsamp, 2))
    i = np.arange(nsamp, dtype=np.float64)
    for f, amp in SPECTRUM_TONES:
        ang = 2 * np.pi * np.mod(f * i, 1.0)
        x[:, 0] += amp * np.cos(ang)
        x[:, 1] += amp * np.sin(ang)
    return np.clip(np.round(x), -127, 127).astype(np.int8).reshape(-1)


def squaring_recording(case):
    """2-bit samples (+-1, +-3) as a 2-bit front-end gives: unit noise plus a weak carrier near coffset, quantised at |v| = 1; the
    chunks plus a third of a chunk that every reader must drop"""
    b, n, m, chunks, fs, coffset = SQUARING[case]
    nsamp = chunks * b * n * m + (b * n * m) // 3
    rng = _rng("squaring/" + case)
    v = rng.normal(0.0, 1.0, size=(nsamp, 2))
    i = np.arange(nsamp, dtype=np.float64)
    ang = 2 * np.pi * np.mod((coffset + 300.0) / fs * i, 1.0)
    v[:, 0] += 0.2 * np.cos(ang)
    v[:, 1] += 0.2 * np.sin(ang)
    q = np.where(np.abs(v) < 1.0, 1, 3) * np.where(v < 0, -1, 1)
    return q.astype(np.int8).reshape(-1)


def cn0_synthetic_lines():
    """a track's first three columns: block index, prompt I with a sign-flipping data bit, prompt Q"""
    rng = _rng("cn0/synthetic")
    nl = CN0_SYNTH["lines"]
    bits = np.repeat(rng.integers(0, 2, size=nl // 20 + 1) * 2 - 1, 20)[:nl]
    amp = 9000.0 * (1.0 + 0.3 * np.sin(np.arange(nl) / 250.0))
    i = bits * amp + rng.normal(0.0, 1500.0, size=nl)
    q = rng.normal(0.0, 1500.0, size=nl)
    return ["%d %f %f" % (k, i[k], q[k]) for k in range(nl)]


def sha256(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def pack(a):
    return base64.b64encode(np.ascontiguousarray(a).tobytes()).decode("ascii")


def unpack(s, dtype):
    return np.frombuffer(base64.b64decode(s), dtype=dtype).copy()


def load():
    with gzip.open(GOLDEN_FILE, "rt") as f:
        return json.load(f)


def checked_recording(golden, kind, case):
    """the regenerated recording of a case, held to the SHA-256 the generator stored"""
    x = spectrum_recording(case) if kind == "spectrum" else squaring_recording(case)
    assert sha256(x) == golden[kind][case]["sha256"], (kind, case, "the regenerated recording differs from the generator's")
    return x


def stream_check(got, want, r_ref, gap):
    """the int16 stream against the reference's: (every value equal or off by one where the reference's own 20 r lies within `gap` of
    a half-integer, share of such positions that differ)"""
    got, want = np.asarray(got, dtype=np.int64), np.asarray(want, dtype=np.int64)
    v = np.empty(2 * r_ref.size)
    v[0::2], v[1::2] = 20 * r_ref.real.reshape(-1), 20 * r_ref.imag.reshape(-1)
    near = np.abs(np.abs(v - np.floor(v)) - 0.5) <= gap
    diff = got != want
    ok = bool(np.all(np.abs(got - want)[diff] == 1) and np.all(near[diff]))
    return ok, float(np.mean(diff))
