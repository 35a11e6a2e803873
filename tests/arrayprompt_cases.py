"""The cases of the array-prompt tests (test_arrayprompt_cpu.py, test_arrayprompt_gpu.py): the estimate cases of tests/cancel_cases.py
seen by up to eight antennas, and the synthetic prompts of the steering estimate.  Everything is computed once per process.

Antenna 0 is cancel_cases.estimate_case(name)["x"] itself; antenna p > 0 is fresh noise of another seed (int8 with both ends of the
range, or complex for "complex64 in") plus the case's own signals at the segments' amplitudes times GAINS[p].  To every satellite's
segments up to four are added where there is room: one wholly before the input, one that straddles its first sample, one that straddles
its last, one wholly after it."""
import functools

import numpy as np

import cancel_cases as C
import cancel_oracle as O

M_MAX = 8
GAINS = np.array([(0.6 + 0.1 * p) * np.exp(0.9j * p) for p in range(M_MAX)])
GAINS[0] = 1.0
INSIDE, STRADDLE, OUTSIDE = 0, 1, 2


def _extra(g, s0, n):
    """a segment with the parameters of g over samples s0 .. s0 + n - 1"""
    return C.seg(s0, n, float(g["carrier_hz"]), float(g["carrier_phase"]), float(g["code_rate_hz"]), float(g["code_phase"]))


@functools.lru_cache(maxsize=None)
def array_case(name):
    """dict(fs, sats, in_first, n, in_complex64, rows: M_MAX read-only arrays as cancel.apply takes them, base: the case's own segments
    per satellite, segs: those and the extra ones, where: per satellite INSIDE / STRADDLE / OUTSIDE of every entry of segs, own: per
    satellite the indices of the case's own segments in segs)"""
    c = C.estimate_case(name)
    lo, n = int(c["in_first"]), int(c["n_out"])
    hi = lo + n
    sats = [C.oracle_sat(s) for s in c["sats"]]
    rows = [c["x"]]
    for p in range(1, M_MAX):
        seed = C.SEED + 1000 + 16 * sorted(C.CASES).index(name) + p
        if c["in_complex64"]:
            r = np.random.Generator(np.random.PCG64(seed))
            noise = r.normal(0.0, 12.0, n) + 1j * r.normal(0.0, 12.0, n)
        else:
            noise = C.as_complex(C.noise_int8(n, seed), False)
        v = O.evaluate(sats, c["segs"], [-GAINS[p] * a for a in C.given_amps(c)], c["fs"], noise, lo, lo, n)
        rows.append(v.astype(np.complex64) if c["in_complex64"] else O.to_int8(v))
    for r in rows:
        r.setflags(write=False)
    segs, where, own = [], [], []
    for g in c["segs"]:
        first, last_end = int(g["s0"][0]), int(g["s0"][-1] + g["n"][-1])
        head, tail = [], []
        if lo >= 30:
            head.append((_extra(g[0], lo - 30, 10), OUTSIDE))
        if lo >= 8 and first > lo:
            head.append((_extra(g[0], lo - 8, 8 + min(first - lo, 50)), STRADDLE))
        if last_end < hi:
            tail.append((_extra(g[-1], max(last_end, hi - 40), hi - max(last_end, hi - 40) + 9), STRADDLE))
        tail.append((_extra(g[-1], hi + 20, 10), OUTSIDE))
        segs.append(C.segs(*([e for e, _ in head] + list(g) + [e for e, _ in tail])))
        where.append(np.array([w for _, w in head] + [INSIDE] * len(g) + [w for _, w in tail]))
        own.append(np.arange(len(head), len(head) + len(g)))
    return dict(fs=c["fs"], sats=c["sats"], in_first=lo, n=n, in_complex64=c["in_complex64"], rows=rows, base=c["segs"], segs=segs, where=where, own=own)


def bits(a):
    """complex128 or float64 as the uint64 words that hold it"""
    return np.ascontiguousarray(a).view(np.uint64)


# ---- synthetic prompts of steering_estimate: M = 4, D = 100, |s| / sigma_c = 21 (a 1 ms segment at amplitude 4 under sigma 12 per
# component at 4.092 MHz: sigma_c = 12 / sqrt(4092) = 0.1876 per component of a prompt)
D, RATIO = 100, 21.0
DIRECTIONS = ((40.0, 60.0), (160.0, 35.0), (280.0, 50.0))


def unit(D=D, ratio=RATIO):
    """the bound of one entry of a_hat, in units of which the tests speak: 6 sqrt(2) sigma_c / (|s| sqrt(D)).  An entry is the ratio
    of two averages over D prompts, each with an error of sigma_c / (|s| sqrt(D)) per component: sqrt(2) of that, six deviations
    allowed (the worst entry over 50 seeds seen in numpy: 4.0 deviations)"""
    return 6.0 * np.sqrt(2.0) / (ratio * np.sqrt(D))


def synthetic(seed, a, s=RATIO, sigma_c=1.0, jammer=None, jam_power=0.0, D=D):
    """(P [D, M], signs, phases): P[g] = b_g e^(i phi_g) s a + noise, the noise Gaussian of deviation sigma_c per component; with
    ``jammer`` (a vector) a rank-one term z_g jammer is added, z_g complex Gaussian of variance jam_power |s|^2: for vectors of equal
    norm, jam_power times the signal's power in every segment"""
    r = np.random.Generator(np.random.PCG64(seed))
    a = np.asarray(a, dtype=np.complex128)
    b = r.choice([-1.0, 1.0], D)
    phi = r.uniform(0.0, 2.0 * np.pi, D)
    noise = sigma_c * (r.normal(0.0, 1.0, (D, len(a))) + 1j * r.normal(0.0, 1.0, (D, len(a))))
    P = (b * np.exp(1j * phi) * s)[:, None] * a[None, :] + noise
    if jammer is not None:
        z = np.sqrt(jam_power) * abs(s) * (r.normal(0.0, np.sqrt(0.5), D) + 1j * r.normal(0.0, np.sqrt(0.5), D))
        P = P + z[:, None] * np.asarray(jammer, dtype=np.complex128)[None, :]
    return P, b, phi
