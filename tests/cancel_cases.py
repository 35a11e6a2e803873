"""The cases of the cancellation tests (test_cancel_cpu.py, test_cancel_gpu.py): small scenes -- fs 2.046 or 4.092 MHz, at most a few
tens of segments, tens of thousands of samples -- and their references, computed once per process from tests/cancel_oracle.py."""
import functools

import numpy as np

import cancel_oracle as O
from gnss_dsp_tools_amd import cancel, codes

SEED = 20240

# chip weight kind -> a code it is used with (kind 5, the second RZ half, goes with L2CM's code as kind 4 does); 10230 chips: gps.l1cd,
# gps.l1cp, gps.l2cm
KIND_CODE = {0: ("gps.ca", 7), 1: ("gps.l1cd", 3), 2: ("galileo.e1b", 11), 3: ("gps.l1cp", 5), 4: ("gps.l2cm", 9), 5: ("gps.l2cm", 12)}


def seg(s0, n, carrier_hz, carrier_phase, code_rate_hz, code_phase, amp=0j):
    g = np.zeros(1, dtype=cancel.SEG_DTYPE)[0]
    g["s0"], g["n"], g["carrier_hz"], g["carrier_phase"], g["code_rate_hz"], g["code_phase"] = s0, n, carrier_hz, carrier_phase, code_rate_hz, code_phase
    g["amp_re"], g["amp_im"] = complex(amp).real, complex(amp).imag
    return g


def segs(*gs):
    return np.array(list(gs), dtype=cancel.SEG_DTYPE)


def oracle_sat(sat):
    return dict(chips=codes.chips(sat.code, sat.prn), kind=sat.kind)


def noise_int8(n, seed, sigma=12.0):
    """interleaved int8 noise with a few samples at both ends of the range (-128 included)"""
    r = np.random.Generator(np.random.PCG64(seed))
    x = np.clip(np.rint(r.normal(0.0, sigma, 2 * n)), -128, 127).astype(np.int8)
    x[5], x[6], x[2 * n - 3] = -128, 127, -128
    return x


def as_complex(x, in_complex64):
    x = np.asarray(x)
    return x.astype(np.complex128) if in_complex64 else x[0::2].astype(np.float64) + 1j * x[1::2].astype(np.float64)


def _kinds(fs=4.092e6):
    """every chip weight; a gap, a boundary inside a lane's run of 8, a one-sample segment, a code-phase wrap, amplitude zero; the
    output starts inside a run and ends inside a segment; segments before and after the output range"""
    sats, sg = [], []
    for kind in range(6):
        code, prn = KIND_CODE[kind]
        L = codes.code_length(code)
        rate = codes.chip_rate(code) * (1.0 + (kind - 2.5) * 1.0e-6)
        dopp = 1000.0 * (kind - 2) + 123.4
        s0 = 37 + 3 * kind                                      # no multiple of 8
        n1 = 4092 + kind
        sats.append(cancel.Sat(code, prn, kind))
        sg.append(segs(seg(s0, n1, dopp, 0.1 * kind, rate, L - 20.25 - kind, 3.0 + 1j * kind),              # wraps past L after a few samples
                       seg(s0 + n1, 1, dopp + 1.0, 0.3, rate, 100.5, -20.0 + 5j),                            # n = 1, adjacent
                       seg(s0 + n1 + 1, 2049, dopp + 2.0, 0.7, rate, 511.125, 0j if kind == 1 else 4.0 - 2.0j),
                       seg(s0 + n1 + 2050 + 301, 4092, dopp - 3.0, 0.9, rate, 0.0, 1.5j),                      # after a gap of 301 samples
                       seg(s0 + n1 + 2050 + 301 + 4092, 3000, dopp, 0.2, rate, 17.0, 2.0)))                    # past the output range in part
    n = 13000
    return dict(fs=fs, sats=sats, segs=sg, x=noise_int8(n, SEED + 1), in_complex64=False, in_first=0, out_first=3, n_out=12345)


def _overlap32(fs=2.046e6):
    """32 satellites on every sample; fs 2.046 MHz; segment boundaries of the satellites at 32 different places"""
    sats, sg = [], []
    for k in range(32):
        sats.append(cancel.Sat("gps.ca", k + 1, 0))
        b = 2046 + 13 * k
        sg.append(segs(seg(0, b, -4000.0 + 250.0 * k, k / 32.0, 1.023e6 + 0.1 * k, (31.7 * k) % 1023.0, (1.0 + 0.1 * k) * np.exp(0.4j * k)),
                       seg(b, 4600 - b, -4000.0 + 250.0 * k + 0.5, 0.5 + k / 64.0, 1.023e6 + 0.1 * k, (77.3 * k + 5) % 1023.0, 2.0 * np.exp(-0.3j * k))))
    n = 4600
    return dict(fs=fs, sats=sats, segs=sg, x=noise_int8(n, SEED + 2), in_complex64=False, in_first=0, out_first=0, n_out=n)


def _far(fs=4.092e6):
    """in_first below 2^33, the last output above it"""
    base = (1 << 33) - 3001
    sats = [cancel.Sat("gps.ca", 5, 0), cancel.Sat("galileo.e1b", 2, 2)]
    sg = [segs(seg(base + 11, 4092, 2500.0, 0.25, 1.023e6 + 1.6, 1000.5, 10.0 - 3.0j), seg(base + 11 + 4092, 4091, 2501.0, 0.6, 1.023e6 + 1.6, 1000.9, 10.0 - 3.0j)),
          segs(seg(base + 500, 6000, -1200.0, 0.0, 1.023e6, 4000.0, 6.0j))]
    n = 9000
    return dict(fs=fs, sats=sats, segs=sg, x=noise_int8(n, SEED + 3), in_complex64=False, in_first=base, out_first=base + 5, n_out=n - 5 - 2)


def _clip(fs=2.046e6):
    """amplitudes that drive the int8 output to both limits"""
    sats = [cancel.Sat("gps.ca", 21, 0), cancel.Sat("gps.ca", 22, 0)]
    sg = [segs(seg(0, 2046, 300.0, 0.0, 1.023e6, 3.0, 200.0)), segs(seg(1000, 2000, -700.0, 0.1, 1.023e6, 900.0, 90.0j))]
    n = 3100
    return dict(fs=fs, sats=sats, segs=sg, x=noise_int8(n, SEED + 4), in_complex64=False, in_first=0, out_first=0, n_out=n)


def _cplx(fs=4.092e6):
    """complex64 input"""
    r = np.random.Generator(np.random.PCG64(SEED + 5))
    n = 5000
    x = (r.normal(0.0, 12.0, n) + 1j * r.normal(0.0, 12.0, n)).astype(np.complex64)
    sats = [cancel.Sat("gps.l1cd", 14, 1), cancel.Sat("gps.ca", 30, 0)]
    sg = [segs(seg(9, 4092, 1750.0, 0.4, 1.023e6 - 1.1, 10229.75, 5.0 + 5.0j)), segs(seg(100, 2046, 0.0, 0.0, 1.023e6, 0.0, -7.0), seg(2146, 2046, 10.0, 0.5, 1.023e6, 1.5, -7.0))]
    return dict(fs=fs, sats=sats, segs=sg, x=x, in_complex64=True, in_first=0, out_first=1, n_out=n - 1)


CASES = {"kinds": _kinds(), "overlap32": _overlap32(), "far": _far(), "clip": _clip(), "complex64 in": _cplx()}


def given_amps(case):
    return [(g["amp_re"] + 1j * g["amp_im"]).astype(np.complex128) for g in case["segs"]]


@functools.lru_cache(maxsize=None)
def reference(name):
    """(fp64 v, numpy float32 v) of a case with the amplitudes given in its segments; read-only"""
    c = CASES[name]
    x = as_complex(c["x"], c["in_complex64"])
    sats = [oracle_sat(s) for s in c["sats"]]
    out = tuple(O.evaluate(sats, c["segs"], given_amps(c), c["fs"], x, c["in_first"], c["out_first"], c["n_out"], f32=f) for f in (False, True))
    for a in out:
        a.setflags(write=False)
    return out


# ---- estimate: inputs that hold the signals, so that the projection has something to find
def _with_signal(case, seed):
    """the case with its input replaced by noise plus the case's own signals at the segments' amplitudes (int8, or complex64), and
    with the output range widened to whole segments"""
    c = dict(case)
    lo = min(int(g["s0"][0]) for g in c["segs"])
    hi = max(int(g["s0"][-1] + g["n"][-1]) for g in c["segs"])
    n = hi - lo
    r = np.random.Generator(np.random.PCG64(seed))
    noise = r.normal(0.0, 12.0, n) + 1j * r.normal(0.0, 12.0, n)
    sats = [oracle_sat(s) for s in c["sats"]]
    v = O.evaluate(sats, c["segs"], [-a for a in given_amps(c)], c["fs"], noise, lo, lo, n)
    if c["in_complex64"]:
        c["x"] = v.astype(np.complex64)
    else:
        c["x"] = O.to_int8(v)
    c["in_first"], c["out_first"], c["n_out"] = lo, lo, n
    return c


@functools.lru_cache(maxsize=None)
def estimate_case(name):
    return _with_signal(CASES[name], SEED + 100 + sorted(CASES).index(name))


ESTIMATE_CASES = ("kinds", "far", "complex64 in")


@functools.lru_cache(maxsize=None)
def estimate_reference(name):
    """([fp64 A per satellite], [A from float32 products and fp64 sums per satellite])"""
    c = estimate_case(name)
    x = as_complex(c["x"], c["in_complex64"])
    out = []
    for f in (False, True):
        out.append([np.array([O.estimate(oracle_sat(s), g, c["fs"], x, c["in_first"], f32=f) for g in sg], dtype=np.complex128)
                    for s, sg in zip(c["sats"], c["segs"])])
    return tuple(out)


# ---- the near-far scene (test 6): GPS L1 at fs 4.092 MHz, sigma 12; PRN 5 strong with data symbols, PRN 9 weak, PRN 17 absent.
# The weak amplitude was chosen on the CPU before any device run: the scene of tests/simulate_oracle.py over the search window, PRN 5
# cancelled by tests/cancel_oracle.py with ideal segments (one per code period, true parameters, estimated amplitudes), both int8
# forms through oracle/frontend_oracle.py and the 20 ms search of oracle/acq_oracle.py, amplitudes 0.8 .. 1.5 in steps of 0.1.
# PRN 9's true cell at the window's first sample: code 911.21, Doppler bin -2200 Hz.
#   amp   input: metric, code, Doppler       residual: metric, code, Doppler
#   0.8   3.03   21.23    400  (wrong)      3.18  911.11  -2200
#   1.0   3.03   21.23    400  (wrong)      3.97  911.11  -2200      <- chosen
#   1.2   3.05  911.11  -2200               4.75  911.11  -2200
#   1.5   3.80  911.11  -2200               5.90  911.11  -2200
# PRN 5: 29.45 on the input, 1.51 on the residual; PRN 17 (absent): 3.08 (a cross-correlation peak of PRN 5) and 1.56.
NEARFAR = dict(fs=4.092e6, coffset=0.0, sigma=12.0, seed=77, ms=300,
               strong=dict(item=5, amp=12.0, doppler=1510.0, code0=417.3, bit=20),
               weak=dict(item=9, amp=1.0, doppler=-2210.0, code0=305.6),
               absent=17, doppler_search=(-5000.0, 5000.0, 200.0), search_ms=20,
               skip=60, loop_dwells=(20.0, 20.0), window=411623)                 # the search window starts at sample 411623 (100.6 ms)
