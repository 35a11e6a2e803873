"""Scenes shared by tests/test_scene_cpu.py and tests/test_scene_gpu.py: each case is the argument set of one scene.recording call;
reference() evaluates it once with tests/scene_oracle.py from the very doubles the package hands to gacq_scene_dev.

Sweeps of 37 (sawtooth) and 38 (triangle) samples put dozens of sweep wraps and both halves of the triangle inside one call and inside
single lanes' runs; the gate (5, 13, 7) opens and closes inside runs of 8, 4 and 2 samples alike."""
import numpy as np

import simulate_cases as S
from gnss_dsp_tools_amd import scene, simulate

SEED = 20261020
FS = 6.0e6
COFFSET = 250000.0
N = 4099
GATE = (5, 13, 7)

TONE = scene.Tone(40.0, 151234.5, 0.3125)
SAW = scene.Chirp(35.0, -1.1e6, 2.3e6, 37, phase=0.17)
TRI = scene.Chirp(35.0, 1.9e6, -0.4e6, 38, triangle=True, phase=0.71)               # falls first: a negative ramp step
JAM = scene.NoiseJammer(30.0)
SATS2 = [simulate.Satellite("gps-l1", 7, 3.0, 1234.5, 417.37, 0.3125, np.array([1, -1, 1, 1, -1], dtype=np.int8), 1),
         simulate.Satellite("galileo-e1b", 5, 4.0, -2100.0, 4000.9, 0.3)]
EMIT3 = [scene.Tone(25.0, -801234.5, 0.4, gate=(700, 1500, 333)), scene.Chirp(20.0, -2.0e6, 2.2e6, 205), scene.NoiseJammer(18.0)]


def full_gains(M, E, seed=5):
    """a full complex gain matrix [M, E]: magnitudes 0.5 .. 1.5, every phase different"""
    rng = np.random.default_rng(seed)
    return (0.5 + rng.random((8, 8))[:M, :E]) * np.exp(2j * np.pi * rng.random((8, 8))[:M, :E])


def _case(sats=(), emitters=(), gains=None, n=N, sigma=0.0, j0=0, first_antenna=0):
    sats, emitters = list(sats), list(emitters)
    if gains is None:
        gains = full_gains(1, len(sats) + len(emitters))
    return dict(sats=sats, emitters=emitters, gains=np.asarray(gains, dtype=np.complex128), fs=FS, coffset=COFFSET, n=n, sigma=sigma, j0=j0,
                first_antenna=first_antenna)


# name -> dict(sats, emitters, gains, fs, coffset, n, sigma, j0, first_antenna)
CASES = {
    "tone alone": _case(emitters=[TONE]),                                                       # K = 0 with I = 1, like the next five
    "sawtooth P=37 alone": _case(emitters=[SAW]),
    "triangle P=38 alone": _case(emitters=[TRI]),
    "jammer alone": _case(emitters=[JAM]),
    "gated tone": _case(emitters=[scene.Tone(40.0, 151234.5, 0.3125, gate=GATE)]),
    "gated jammer": _case(emitters=[scene.NoiseJammer(30.0, gate=GATE)]),
    "n=1": _case(sats=SATS2[:1], emitters=[SAW], n=1, sigma=12.0, j0=5),
    "chirp j0=2^40+12345": _case(sats=SATS2[:1], emitters=[SAW, TRI], gains=full_gains(2, 3), sigma=12.0, j0=2 ** 40 + 12345),
    "n=257 up to 2^48": _case(sats=SATS2[:1], emitters=[TRI, TONE], gains=full_gains(2, 3), n=257, sigma=12.0, j0=2 ** 48 - 257),
    # the longest sweep ends and a gate of 2^40 samples opens inside the call: the place in the gate period does not fit 32 bits
    "sweep 2^31, gate period 2^40": _case(emitters=[scene.Tone(40.0, 151234.5, 0.3125, gate=(2 ** 39, 2 ** 40, 2 ** 31 - 1000)),
                                                    scene.Chirp(30.0, -1.0e6, 2.0e6, 2 ** 31, phase=0.4)],
                                          gains=full_gains(2, 2), sigma=12.0, j0=2 ** 40 + 2 ** 31 - 2000),
    "first_antenna=5": _case(sats=SATS2, emitters=EMIT3, gains=full_gains(2, 5), sigma=12.0, first_antenna=5),
}
for _M in (1, 2, 3, 5, 8):
    CASES["K=2 I=3 M=%d" % _M] = _case(sats=SATS2, emitters=EMIT3, gains=full_gains(_M, 5), sigma=12.0)

# int8 only: both clip limits occur
CLIP_CASE = _case(sats=SATS2[:1], emitters=[scene.Tone(200.0, 151234.5)], gains=full_gains(3, 2), sigma=12.0)
# one call against three, M = 3: crosses 2^32 in the low word of the noise counters
CUT_CASE = _case(sats=SATS2, emitters=EMIT3, gains=full_gains(3, 5), sigma=12.0, j0=2 ** 33 - 7000)
CUT_N, CUT_PIECES = 20000, (4099, 1, 15900)


def oracle_emitters(emitters):
    out = []
    for e in emitters:
        s = e.struct()
        out.append(dict(kind=s.kind, amp=s.amp, f0_hz=s.f0_hz, f1_hz=s.f1_hz, phase=s.phase, sweep=s.sweep,
                        gate=(s.gate_on, s.gate_period, s.gate_first) if s.gate_period else None))
    return out


def oracle_args(c):
    """the arguments of scene_oracle.evaluate before seed: (sats, emitters, gains, fs, sigma)"""
    return S.oracle_sats(c["sats"], c["coffset"]), oracle_emitters(c["emitters"]), c["gains"], c["fs"], c["sigma"]


_REF = {}


def reference(name):
    """(fp64 oracle, float32 evaluation) [M, n] of a case of CASES, computed once and shared; callers leave the arrays as they are"""
    if name not in _REF:
        import scene_oracle as O
        c = CASES[name]
        _REF[name] = tuple(O.evaluate(*oracle_args(c), SEED, c["first_antenna"], c["j0"], c["n"], f32=f) for f in (False, True))
        for a in _REF[name]:
            a.setflags(write=False)
    return _REF[name]


# ---- the two pipelines; the levels were fixed on the CPU with the oracle chain before any device run (the tables are in DESIGN 5.28)
#
# 1. Array: the end-to-end scene of tests/nulling_cases.py (E2E) through the generator -- GPS L1 at 4.092 MS/s, PRN 17 at amplitude 1,
#    Doppler 1250 Hz, code 333.25, sigma 6 on four antennas under exp(2 pi i sat_phase), one noise jammer of sigma 42 under
#    exp(2 pi i jam_phase) -- then nulling (block 4096, window 8), the front-end and the 20 ms search.
#    The noise realisation is not that of the numpy scene of nulling_cases.py, so the chain was run again: tests/scene_oracle.py (fp64,
#    seed 101) rounded to int8, the nulling oracle (gain 1, load_shift 10), oracle/frontend_oracle.py and the 20 ms search of
#    oracle/acq_oracle.py over -5000 .. 5000 Hz in 200 Hz steps on the 25 ms from sample 36864.  True cell: code 342.26, bin 1200 Hz.
#      jammer   antenna 0: metric, code, Doppler, power         nulled output: metric, code, Doppler, power
#        42     1.71   61.44   1600  (wrong)  1792.9            6.75  342.42  1200   48.6      no output component clipped
#    Both outcomes at the level of nulling_cases.E2E: the jammer level was not moved.
ARRAY_SEED = 101


def array_scene():
    """(sats, emitters, gains [4, 2]) of the array pipeline"""
    import nulling_cases as NC
    e = NC.E2E
    sats = [simulate.Satellite(e["signal"], e["prn"], e["amp"], e["doppler"], e["code_phase"])]
    gains = np.stack([np.exp(2j * np.pi * np.array(e["sat_phase"])), np.exp(2j * np.pi * np.array(e["jam_phase"]))], axis=1)
    return sats, [scene.NoiseJammer(e["jam"])], gains


# 2. Single antenna, swept jammer: GPS L1 at 4.096 MS/s, PRN 17 at amplitude 1, sigma 4, a sawtooth chirp of amplitude 60 across 0.7 fs
#    every 205 samples, int8.  The oracle chain: tests/scene_oracle.py (fp64, seed 202) rounded to int8, tests/mitigate_oracle.py
#    (excision alone, ratio 12, guard 2, automatic gain), oracle/frontend_oracle.py and the 20 ms search over -5000 .. 5000 Hz in 200 Hz
#    steps on the 25 ms from sample 0.  True cell: code 333.25, bin 1200 Hz; one sample is 0.25 chip.
#      input to the search                  metric   code    Doppler   found     bins zeroed per frame
#      raw                                   1.42   914.11    1200     no
#      excision, 1024-sample frames          2.38   238.27    3800     no        750.9 of 1024
#      excision, 64-sample frames            8.22   333.17    1200     yes        18.7 of 64
#      the same scene without the jammer    11.28   333.17    1200     yes
#    A 1024-sample frame holds five sweeps, so the chirp fills 0.7 of its bins, and zeroing them takes the main lobe of the satellite
#    with the jammer; a 64-sample frame holds under a third of a sweep, 19 of its 64 bins, in another place in every frame.
SWEPT = dict(signal="gps-l1", fs=4.096e6, prn=17, doppler=1250.0, code_phase=333.25, amp=1.0, sigma=4.0, jam=60.0, sweep=205, span=0.7, ms=20,
             doppler_search=(-5000.0, 5000.0, 200.0), seed=202)


def swept_scene():
    s = SWEPT
    sats = [simulate.Satellite(s["signal"], s["prn"], s["amp"], s["doppler"], s["code_phase"])]
    return sats, [scene.Chirp(s["jam"], -0.5 * s["span"] * s["fs"], 0.5 * s["span"] * s["fs"], s["sweep"])], np.ones((1, 2), dtype=np.complex128)
