"""CPU: the definition of the array-and-interference scene (tests/scene_oracle.py) against brute force and hand values -- the chirps'
closed-form phase, the gate, the antennas' and jammers' noise streams, the steering vectors -- the argument checks of gacq_scene_check
through the raw ABI, the command line of scene.py, and the oracle chains (scene, nulling or mitigate, front-end, 20 ms search) that fix the
levels of the two pipelines of tests/scene_cases.py."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

import scene_cases as C
import scene_oracle as O
import simulate_cases as SC
import simulate_oracle as SO
from gnss_dsp_tools_amd import _native as nat
from gnss_dsp_tools_amd import scene, simulate
from test_simulate_cpu import _sat

FS = 4.0e6


def _chirp(kind, P, f0, f1, phase=0.3):
    return dict(kind=kind, amp=1.0, f0_hz=f0, f1_hz=f1, phase=phase, sweep=P, gate=None)


CHIRPS = [(O.SAWTOOTH, P) for P in (2, 3, 4, 37, 38)] + [(O.TRIANGLE, P) for P in (2, 4, 38)]


@pytest.mark.parametrize("kind,P", CHIRPS)
@pytest.mark.parametrize("f0,f1", [(-1.1e6, 1.7e6), (1.3e6, -0.9e6), (-2.0e6, 2.0e6)])      # the second: a negative R; the third: |f1 - f0| = fs
def test_closed_form_chirp_phase_is_the_brute_force_sum(kind, P, f0, f1):
    w = O.chirp_words(_chirp(kind, P, f0, f1), FS)
    R = w[2]
    if w[4] >= 3:                                                    # a step below half a turn per sample: the sign is the top bit
        assert (R >> 63) == (1 if f1 < f0 else 0)
    if w[4] == 1 and f1 - f0 == FS:
        assert R == 0                                                # a whole turn per sample
    th = w[0]                                                        # the definition: one frequency word added per sample
    for j in range(3 * P + 1):
        assert O.chirp_phase(j, *w) == th & O.M64, (kind, P, j)
        th += O.frequency_word(j % P, *w[1:])
    assert O.chirp_phase_brute(3 * P, *w) == O.chirp_phase(3 * P, *w)


@pytest.mark.parametrize("kind,P", [(O.SAWTOOTH, 37), (O.TRIANGLE, 38), (O.SAWTOOTH, 2 ** 31), (O.TRIANGLE, 2 ** 31)])
@pytest.mark.parametrize("j", [2 ** 40 + 12345, 2 ** 48 - 1])
def test_closed_form_far_from_zero_by_an_independent_route(kind, P, j):
    for f0, f1 in [(-1.1e6, 1.7e6), (1.3e6, -0.9e6)]:
        w = O.chirp_words(_chirp(kind, P, f0, f1), FS)
        if P <= 38:                                                  # whole sweeps and the rest, each added up word by word
            assert O.chirp_phase(j, *w) == O.chirp_phase_by_sweeps(j, *w)
            continue
        # a sweep too long to add up: the ramp sums as arithmetic series (terms x (first + last) / 2), rising and falling part apart
        p0, F0, R, _, H = w
        s, u = divmod(j, P)

        def series(u):
            up, down = min(u, H), max(u - H, 0)
            return Fraction(up * (0 + up - 1), 2) + Fraction(down * ((P - 1 - H) + (P - u)), 2)

        T, TP = series(u), series(P)
        assert T.denominator == TP.denominator == 1
        assert O.chirp_phase(j, *w) == (p0 + s * (P * F0 + R * int(TP)) + u * F0 + R * int(T)) % (1 << 64)


@pytest.mark.parametrize("kind,P", [(O.SAWTOOTH, 37), (O.TRIANGLE, 38), (O.SAWTOOTH, 205)])
def test_instantaneous_frequency_runs_from_f0_to_within_a_step_of_f1(kind, P):
    for f0, f1 in [(-1.1e6, 1.7e6), (1.3e6, -0.9e6)]:
        p0, F0, R, P_, H = O.chirp_words(_chirp(kind, P, f0, f1), FS)
        hz = []
        for u in range(P):
            w = O.frequency_word(u, F0, R, P, H)
            hz.append((w - (1 << 64) if w >> 63 else w) * FS / 2.0 ** 64)
        step = (f1 - f0) / H
        assert abs(hz[0] - f0) < 1e-6 and abs(hz[H - 1] - (f1 - step)) < 1e-6
        assert np.allclose(np.diff(hz[:H]), step, atol=1e-6)
        if kind == O.TRIANGLE:                                       # and back again: the same frequencies in reverse
            assert np.allclose(hz[H:], hz[:H][::-1], atol=1e-6) and abs(hz[P - 1] - f0) < 1e-6


@pytest.mark.parametrize("gate", [(5, 13, 7), (1, 1, 0), (13, 13, 0)])
def test_gate_over_three_periods(gate):
    on, period, first = gate
    for j in range(3 * period):
        k = j - first
        while k < 0:
            k += period
        while k >= period:
            k -= period
        assert O.gate_on(j, gate) == (k < on)
    assert O.gate_on(12345, None)
    if gate == (5, 13, 7):
        assert [j for j in range(26) if O.gate_on(j, gate)] == [7, 8, 9, 10, 11, 20, 21, 22, 23, 24]


def test_one_antenna_unit_gain_no_emitter_is_the_single_antenna_recording():
    c = SC.CASES["seven kinds sigma=12"]
    sats = SC.oracle_sats(c["sats"], c["coffset"])
    got = O.evaluate(sats, [], np.ones((1, len(sats))), c["fs"], c["sigma"], SC.SEED, 0, c["j0"], 600)
    want = SO.evaluate(sats, c["fs"], c["sigma"], SC.SEED, c["j0"], 600)
    assert got.shape == (1, 600) and np.array_equal(got[0], want)


def test_noise_streams_of_antennas_and_jammers():
    seed, sigma, n = SC.NOISE_SEEDS[1], 12.0, 1 << 20
    j0 = 2 ** 33 - 1000
    streams = [O.antenna_noise(seed, sigma, a, j0, n) for a in range(8)] + [O.jammer_noise(seed, sigma, i, j0, n) for i in range(8)]
    want = SO.noise(seed, sigma, j0, n)
    assert np.array_equal(streams[0][0], want[0]) and np.array_equal(streams[0][1], want[1])      # antenna 0: the single-antenna stream
    w = SO.philox4x32_10((5, 0, 3, 1), (seed & 0xffffffff, seed >> 32))                           # the counter layout, against scalar Philox
    r0, r1 = O.philox_words(seed, 5, 1, 3, 1)
    assert (int(r0[0]), int(r1[0])) == w[:2]
    for p in range(16):
        for q in range(p):
            assert abs(np.corrcoef(streams[p][0], streams[q][0])[0, 1]) < 5.0 / np.sqrt(n), (p, q)
    for p, (re, im) in enumerate(streams):
        got, cap = SO.noise_statistics(re, im, sigma)
        for k in got:
            assert got[k] <= cap[k], (p, k, got[k], cap[k])


def test_steering_against_hand_values():
    assert np.allclose(scene.steering([[0.5, 0.0, 0.0]], 90.0, 0.0), [-1.0])
    assert np.allclose(scene.steering([[0.5, 0.0, 0.0]], 0.0, 0.0), [1.0])
    for z in (0.3, 1.25):
        assert np.allclose(scene.steering([[0.7, -0.2, z]], 33.0, 90.0), [np.exp(2j * np.pi * z)])
    s = scene.steering([[0.0, 0.0, 0.0], [0.0, 0.25, 0.0], [0.25, 0.0, 0.0]], 0.0, 0.0)          # from the north: the north element leads
    assert s.dtype == np.complex128 and np.allclose(s, [1.0, 1j, 1.0])


# ---- the raw ABI

def _emitter(**kw):
    args = dict(kind=1, pad=0, amp=20.0, f0_hz=-1.0e6, f1_hz=1.0e6, phase=0.1, sweep=38, gate_period=13, gate_on=5, gate_first=7)
    args.update(kw)
    return scene.SceneEmitter(**args)


def bad_calls():
    """(label, expected code, keyword changes) of every refusal of gacq_scene_check; shared with the GPU test"""
    nan, inf = float("nan"), float("inf")
    sym = np.array([1, -1, 1], dtype=np.int8)
    bad_sym = np.array([1, 0, -1], dtype=np.int8)
    out = [("K 33", -1, dict(K=33)), ("K -1", -1, dict(K=-1)), ("I 9", -1, dict(I=9)), ("I -1", -1, dict(I=-1)), ("M 0", -1, dict(M=0)),
           ("M 9", -1, dict(M=9)), ("first_antenna -1", -1, dict(first=-1)), ("first_antenna > 2^31 - M", -1, dict(first=2 ** 31 - 1)),
           ("n 0", -1, dict(n=0)), ("n -5", -1, dict(n=-5)), ("j0 -1", -1, dict(j0=-1)), ("j0 + n > 2^48", -1, dict(j0=2 ** 48 - 99)),
           ("j0 > 2^48", -1, dict(j0=2 ** 48 + 1)), ("n > 2^48", -1, dict(n=2 ** 48 + 1)), ("fs nan", -1, dict(fs=nan)), ("fs inf", -1, dict(fs=inf)),
           ("fs 0", -1, dict(fs=0.0)), ("fs < 0", -1, dict(fs=-6.0e6)), ("sigma < 0", -1, dict(sigma=-1.0)), ("sigma nan", -1, dict(sigma=nan)),
           ("sigma inf", -1, dict(sigma=inf)), ("sats NULL", -1, dict(sats=None)), ("emitters NULL", -1, dict(emitters=None)),
           ("gains NULL", -1, dict(gains=None)), ("out NULL", -1, dict(out=None)), ("a row NULL", -1, dict(row1=0)),
           ("gain nan", -1, dict(gain=nan)), ("gain inf", -1, dict(gain=inf)), ("gain beyond fp32", -1, dict(gain=1e39))]
    for field in ("amp", "carrier_hz", "carrier_phase", "code_rate_hz", "code_phase"):
        out += [("sat %s nan" % field, -1, dict(sat={field: nan})), ("sat %s inf" % field, -1, dict(sat={field: inf}))]
    out += [("code rate 0", -1, dict(sat=dict(code_rate_hz=0.0))), ("code rate / fs = 16", -1, dict(sat=dict(code_rate_hz=16 * 6.0e6))),
            ("code phase < 0", -1, dict(sat=dict(code_phase=-0.5))), ("code phase = L", -1, dict(sat=dict(code_phase=1023.0))),
            ("sat kind 6", -1, dict(sat=dict(kind=6))), ("nsym -1", -1, dict(sat=dict(nsym=-1))), ("symbol 0", -1, dict(sat=dict(sym=bad_sym))),
            ("symbols NULL", -1, dict(sat=dict(nsym=3))), ("periods_per_symbol 0", -1, dict(sat=dict(periods_per_symbol=0, sym=sym))),
            ("code NULL", -1, dict(sat=dict(code=None))), ("unknown code", -2, dict(sat=dict(code=b"gps.nope")))]
    for field in ("amp", "f0_hz", "f1_hz", "phase"):
        out += [("emitter %s nan" % field, -1, dict(em={field: nan})), ("emitter %s inf" % field, -1, dict(em={field: inf}))]
    out += [("kind -1", -1, dict(em=dict(kind=-1))), ("kind 4", -1, dict(em=dict(kind=4))), ("sweep 1", -1, dict(em=dict(sweep=1))),
            ("sweep 0", -1, dict(em=dict(sweep=0))), ("sweep 2^31 + 1", -1, dict(em=dict(sweep=2 ** 31 + 1))),
            ("odd triangle sweep", -1, dict(em=dict(kind=2, sweep=37))), ("|f1 - f0| > fs", -1, dict(em=dict(f0_hz=-3.1e6, f1_hz=3.0e6))),
            ("gate_period < 0", -1, dict(em=dict(gate_period=-1))), ("gate_period > 2^48", -1, dict(em=dict(gate_period=2 ** 48 + 1))),
            ("gate_first < 0", -1, dict(em=dict(gate_first=-1))), ("gate_first = gate_period", -1, dict(em=dict(gate_first=13))),
            ("gate_on 0", -1, dict(em=dict(gate_on=0))), ("gate_on > gate_period", -1, dict(em=dict(gate_on=14)))]
    return out


GOOD = [("the unchanged call", {}), ("K 0", dict(K=0, sats=None)), ("I 0", dict(I=0, emitters=None)), ("odd sawtooth sweep", dict(em=dict(sweep=37))),
        ("sweep 2^31", dict(em=dict(sweep=2 ** 31))), ("|f1 - f0| = fs", dict(em=dict(f0_hz=-3.0e6, f1_hz=3.0e6))),
        ("gate_on = gate_period", dict(em=dict(gate_on=13))), ("no gate, fields unused", dict(em=dict(gate_period=0, gate_on=0, gate_first=99))),
        ("a tone ignores the sweep", dict(em=dict(kind=0, sweep=0))), ("first_antenna = 2^31 - M", dict(first=2 ** 31 - 2))]


def raw_call(ctx, rows, K=2, I=2, M=2, n=100, j0=0, fs=6.0e6, sigma=12.0, seed=1, cplx=0, first=0, sats="default", emitters="default", gains="default",
             out="default", sat=None, em=None, gain=None, row1=None, check=False):
    """gacq_scene_dev (or, with check, gacq_scene_check) with two good satellites and two good emitters, the second of each changed by
    `sat` / `em`, one gain by `gain`; rows: M device (or any, for the check) addresses"""
    sarr = (simulate.SimSat * 33)(*([_sat(), _sat(**(sat or {}))] + [_sat() for _ in range(31)]))
    earr = (scene.SceneEmitter * 9)(*([_emitter(kind=0), _emitter(**(em or {}))] + [_emitter() for _ in range(7)]))
    g = np.ones((9, 41, 2), dtype=np.float64)
    if gain is not None:
        g[0, 1, 1] = gain
    rows = list(rows) + [rows[0]] * 9
    if row1 is not None:
        rows[1] = row1
    ptrs = (ctypes.c_void_p * 9)(*rows[:9])
    head = (None if sats is None else ctypes.addressof(sarr), K, None if emitters is None else ctypes.addressof(earr), I,
            None if gains is None else g.ctypes.data, fs, sigma)
    tail = (first, M, j0, n, cplx, None if out is None else ctypes.cast(ptrs, ctypes.c_void_p))
    if check:
        return nat.lib.gacq_scene_check(*head, *tail)
    return nat.lib.gacq_scene_dev(ctx, *head, seed, *tail)


def test_every_refusal_without_a_device():
    buf = np.zeros(1024, dtype=np.int8)
    rows = [buf.ctypes.data, buf.ctypes.data + 512]
    assert ctypes.sizeof(scene.SceneEmitter) == 72
    for label, change in GOOD:
        assert raw_call(None, rows, check=True, **change) == 0, (label, nat.lib.gacq_last_error(None))
        assert raw_call(None, rows, **change) == -1, label          # a NULL context: nothing may be touched
    for label, code, change in bad_calls():
        assert raw_call(None, rows, check=True, **change) == code, (label, nat.lib.gacq_last_error(None))
        assert nat.lib.gacq_last_error(None), label
        assert raw_call(None, rows, **change) < 0, label
    odd = [buf.ctypes.data + 8, buf.ctypes.data + 516]
    assert raw_call(None, odd, check=True, cplx=1) == -1 and raw_call(None, odd, check=True, cplx=0) == 0
    assert not buf.any()


def test_recording_refuses_before_it_needs_a_device():
    sats, emitters, gains = C.SATS2, C.EMIT3, C.full_gains(2, 5)
    for kw in (dict(n=0), dict(j0=2 ** 48), dict(first_antenna=2 ** 31 - 1), dict(sigma=-1.0), dict(fs=0.0)):
        args = dict(fs=C.FS, coffset=0.0, n=100, seed=1)
        args.update(kw)
        with pytest.raises(nat.GacqError):
            scene.recording(sats, emitters, gains, engine=object(), **args)
    with pytest.raises(nat.GacqError):
        scene.recording(sats, [scene.Chirp(1.0, 0.0, 1.0e6, 37, triangle=True)], C.full_gains(2, 3), C.FS, 0.0, 100, 1, engine=object())
    with pytest.raises(ValueError):
        scene.recording(sats, emitters, C.full_gains(2, 4), C.FS, 0.0, 100, 1, engine=object())
    with pytest.raises(ValueError):
        scene.recording(sats, emitters, gains, C.FS, 0.0, 100, 1, dtype="int16", engine=object())


# ---- the command line

BASE = ["--fs", "4.092e6", "--coffset", "-250000", "--seconds", "0.01", "--seed", "31"]


def test_command_line_parsing():
    argv = BASE + ["--element", "0,0,0", "--element", "0.5,0,0", "--sat", "gps-l1,7,3,1234.5,417.37,20@90,0", "--sat", "gps-l1,19,3.0,-1840.2,88.71",
                   "--tone", "25,-801234.5@0,0", "--gate", "700,1500", "--chirp", "60,-1.4e6,1.4e6,205", "--chirp=20,1e6,-1e6,38,tri@90,0",
                   "--gate", "5,13,7", "--jammer", "42@90,60", "--sigma", "6", "a.bin", "b.bin"]
    a, sats, emitters, elements, gains = scene.parse(argv)
    assert (a.fs, a.coffset, a.seconds, a.seed, a.sigma, a.outputs) == (4.092e6, -250000.0, 0.01, 31, 6.0, ["a.bin", "b.bin"])
    assert [(s.tracker, s.item, s.doppler) for s in sats] == [("gps-l1", 7, 1234.5), ("gps-l1", 19, -1840.2)]
    assert np.array_equal(sats[0].symbols, simulate.parse_sat("gps-l1,7,3,1234.5,417.37,20", 0, 31, 0.01).symbols) and sats[1].symbols is None
    assert emitters == [scene.Tone(25.0, -801234.5, gate=(700, 1500, 0)), scene.Chirp(60.0, -1.4e6, 1.4e6, 205),
                        scene.Chirp(20.0, 1e6, -1e6, 38, triangle=True, gate=(5, 13, 7)), scene.NoiseJammer(42.0)]
    assert np.array_equal(elements, [[0, 0, 0], [0.5, 0, 0]]) and gains.shape == (2, 6)
    want = np.ones((2, 6), dtype=np.complex128)
    want[1, 0] = want[1, 4] = -1.0                                  # @90,0 on an element half a wavelength east
    want[1, 5] = np.exp(2j * np.pi * 0.25)                         # @90,60: cos 60 = 1/2
    assert np.allclose(gains, want)                                 # no direction, and @0,0 on this array: gain 1
    # no --element: one antenna at the origin, one file
    a, sats, emitters, elements, gains = scene.parse(BASE + ["--jammer", "30", "o.bin"])
    assert sats == [] and emitters == [scene.NoiseJammer(30.0)] and np.array_equal(elements, [[0, 0, 0]]) and np.array_equal(gains, [[1.0]])
    assert a.sigma == 12.0
    for bad in (BASE + ["o.bin"],                                                                # no source
                BASE + ["--gate", "5,13", "--tone", "1,2", "o.bin"],                            # a gate before any emitter
                BASE + ["--sat", "gps-l1,7,3,0,0", "--gate", "5,13", "o.bin"],                  # a gate after a satellite
                BASE + ["--tone", "1,2", "--gate", "5,13", "--gate", "5,13", "o.bin"],          # two gates on one emitter
                BASE + ["--tone", "1,2", "--gate", "5", "o.bin"], BASE + ["--tone", "1", "o.bin"], BASE + ["--tone", "1,2@90", "o.bin"],
                BASE + ["--chirp", "1,2,3,37,saw", "o.bin"], BASE + ["--chirp", "1,2,3,x", "o.bin"], BASE + ["--jammer", "1,2", "o.bin"],
                BASE + ["--element", "0,0", "--tone", "1,2", "o.bin"],
                BASE + ["--element", "0,0,0", "--element", "1,0,0", "--tone", "1,2", "o.bin"],  # two elements, one file
                BASE + ["--tone", "1,2", "o.bin", "p.bin"],                                     # one element, two files
                BASE + ["--tone", "1,2", "--sat", "gps-l9,7,3,0,0", "o.bin"], BASE + ["--tone"]):
        with pytest.raises(SystemExit):
            scene.parse(bad)


# ---- the oracle chains behind the two pipelines of scene_cases.py (the device tests assert the same outcomes)

def _search(i8, start, fs, E):
    from gnss_dsp_tools_amd import signals
    from oracle import acq_oracle, frontend_oracle
    n = int(fs * 0.001 * (E["ms"] + 5))
    x = frontend_oracle.iq_to_complex(i8[2 * start:2 * (start + n)])
    y = frontend_oracle.condition(x, fs, 0.0, signals.get(E["signal"]), E["ms"] + 5)
    return acq_oracle.search_script(E["signal"], y, E["prn"], list(E["doppler_search"]), E["ms"])


def _found(result, true_code, doppler, fs):
    m, code, dop = result
    return dop == 200.0 * round(doppler / 200.0) and abs((code - true_code + 511.5) % 1023.0 - 511.5) <= 1.023e6 / fs


def test_oracle_chain_of_the_array_pipeline_shows_both_outcomes():
    import nulling_cases as NC
    import nulling_oracle as NO
    E = NC.E2E
    fs, W, Lb = E["fs"], E["window"], E["block"]
    w0 = (W + 1) * Lb
    n = w0 + int(fs * 0.001 * (E["ms"] + 5)) + 8
    sats, emitters, gains = C.array_scene()
    v = O.evaluate(SC.oracle_sats(sats, 0.0), C.oracle_emitters(emitters), gains, fs, E["sigma"], C.ARRAY_SEED, 0, 0, n)
    xs = [O.to_int8(row) for row in v]
    y = NO.run(xs, 0, 0, n, Lb, W, 10, None, 1.0)["out"]
    before, after = _search(xs[0], w0, fs, E), _search(y, w0, fs, E)
    true_code = (E["code_phase"] + w0 * sats[0].code_rate_hz() / fs) % 1023.0
    print("antenna 0: metric %.2f code %.2f doppler %.0f   nulled: metric %.2f code %.2f doppler %.0f" % (tuple(before) + tuple(after)))
    assert _found(after, true_code, E["doppler"], fs) and not _found(before, true_code, E["doppler"], fs)


def test_oracle_chain_of_the_swept_jammer_shows_both_outcomes():
    import mitigate_oracle as MO
    s = C.SWEPT
    fs = s["fs"]
    n = int(fs * 0.001 * (s["ms"] + 5)) + 4096
    sats, emitters, gains = C.swept_scene()
    raw = O.to_int8(O.evaluate(SC.oracle_sats(sats, 0.0), C.oracle_emitters(emitters), gains, fs, s["sigma"], s["seed"], 0, 0, n)[0])
    got = {"raw": _search(raw, 0, fs, s)}
    for nfft in (1024, 64):
        cfg = MO.config(blank=None, nfft=nfft)
        got[nfft] = _search(MO.evaluate(cfg, raw, MO.auto_gain(cfg, raw)).i8, 0, fs, s)
    print(got)
    assert _found(got[64], s["code_phase"], s["doppler"], fs)
    assert not _found(got["raw"], s["code_phase"], s["doppler"], fs) and not _found(got[1024], s["code_phase"], s["doppler"], fs)
