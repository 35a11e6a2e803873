"""Scenes shared by tests/test_simulate_cpu.py and tests/test_simulate_gpu.py: each case is the argument set of one
simulate.recording call; oracle_sats() turns its satellites into the dicts of tests/simulate_oracle.py from the very doubles the
package hands to gacq_simulate_dev.

The seven-satellite scene runs at 125 kS/s: every code rate stays below 16 chips per sample and 4099 samples then span 32 periods of
the 1 ms codes, so symbols of 1 and of 20 periods change inside the window, mid-lane and between lanes."""
import numpy as np

from gnss_dsp_tools_amd import codes, simulate

SEED = 20261018
NOISE_SEEDS = (20261, 0xDEADBEEFCAFEF00D)        # the seeds of the noise statistics, on the oracle (CPU) and on the device
NOISE_N = 1 << 20


def _l1(**kw):
    args = dict(tracker="gps-l1", item=7, amp=3.0, doppler=1234.5, code0=417.37, carrier_phase=0.3125)
    args.update(kw)
    return simulate.Satellite(**args)


SEVEN = [
    simulate.Satellite("gps-l1", 7, 3.0, 1234.5, 417.37, 0.1, np.array([1, -1, -1, 1, -1, 1, 1], dtype=np.int8), 1),              # kind 0
    simulate.Satellite("gps-l1cd", 12, 2.5, -840.25, 10229.6, 0.2, np.array([-1], dtype=np.int8), 1),                               # kind 1
    simulate.Satellite("galileo-e1b", 5, 4.0, 2100.0, 4000.9, 0.3),                                                                  # kind 2
    simulate.Satellite("gps-l1cp", 3, 3.5, -3071.9, 77.125, 0.4, np.array([1, 1, -1, 1, -1, -1, -1], dtype=np.int8), 1),            # kind 3
    simulate.Satellite("gps-l2cm", 9, 2.0, 455.5, 5000.5, 0.5),                                                                      # kind 4
    simulate.Satellite("gps-l2cl", 9, 2.0, 455.5, 767249.75, 0.6, np.array([-1], dtype=np.int8), 20),                               # kind 5, 767250 chips
    simulate.Satellite("glonass-l1", -3, 3.0, 777.7, 301.81, 0.7, np.array([-1, 1, 1, -1, 1, -1, -1], dtype=np.int8), 20),          # FDMA channel -3
]

FS_CHIPSKIP = 1.023e6 / 1.7                       # 1.7 chips per sample: chips are skipped

# name -> dict(sats, fs, coffset, n, seed, sigma, j0)
CASES = {
    "l1 j0=0": dict(sats=[_l1()], fs=6.0e6, coffset=250000.0, n=4099, sigma=12.0, j0=0),
    "l1 j0=2^40+12345": dict(sats=[_l1()], fs=6.0e6, coffset=250000.0, n=4099, sigma=12.0, j0=2 ** 40 + 12345),
    "seven kinds sigma=0": dict(sats=SEVEN, fs=125.0e3, coffset=10000.0, n=4099, sigma=0.0, j0=0),
    "seven kinds sigma=12": dict(sats=SEVEN, fs=125.0e3, coffset=10000.0, n=4099, sigma=12.0, j0=0),
    "n=1": dict(sats=[_l1()], fs=6.0e6, coffset=250000.0, n=1, sigma=12.0, j0=5),
    "n=257 up to 2^48": dict(sats=[_l1()], fs=6.0e6, coffset=250000.0, n=257, sigma=12.0, j0=2 ** 48 - 257),
    "1.7 chips per sample": dict(sats=[_l1(doppler=0.0, symbols=np.array([1, -1, 1, 1, -1, -1, 1], dtype=np.int8))], fs=FS_CHIPSKIP, coffset=20000.0,
                                 n=4099, sigma=12.0, j0=0),
    "code wraps in the first run": dict(sats=[_l1(code0=1023 - 0.25, symbols=np.array([1, -1], dtype=np.int8))], fs=6.0e6, coffset=250000.0, n=4099,
                                        sigma=12.0, j0=0),
}
# int8 only: both clip limits occur
CLIP_CASE = dict(sats=[_l1(amp=200.0)], fs=6.0e6, coffset=250000.0, n=4099, sigma=12.0, j0=0)
# one call against three: crosses 2^32 in the low word of the noise counter
CUT_CASE = dict(sats=SEVEN, fs=125.0e3, coffset=10000.0, sigma=12.0, j0=2 ** 33 - 7000)
CUT_N, CUT_PIECES = 20000, (4099, 1, 15900)


def oracle_sats(sats, coffset):
    out = []
    for s in sats:
        st, sym = s.struct(coffset)
        out.append(dict(chips=codes.chips(st.code.decode(), st.prn), kind=st.kind, amp=st.amp, carrier_hz=st.carrier_hz,
                        carrier_phase=st.carrier_phase, code_rate_hz=st.code_rate_hz, code_phase=st.code_phase, symbols=sym,
                        periods_per_symbol=st.periods_per_symbol))
    return out


_REF = {}


def reference(name):
    """(fp64 oracle, float32 evaluation) of a case of CASES, computed once and shared; callers leave the arrays as they are"""
    if name not in _REF:
        import simulate_oracle as O
        c = CASES[name]
        sats = oracle_sats(c["sats"], c["coffset"])
        _REF[name] = tuple(O.evaluate(sats, c["fs"], c["sigma"], SEED, c["j0"], c["n"], f32=f) for f in (False, True))
        for a in _REF[name]:
            a.setflags(write=False)
    return _REF[name]
