"""CPU: the definition of the synthetic recording (tests/simulate_oracle.py) against known answers, exact fractions and the host numpy
generator of tests/handoff_cases.py; the argument checks of gacq_simulate_dev that need no device; simulate.Satellite and the
command line."""
import ctypes
import math
from fractions import Fraction

import numpy as np
import pytest

import handoff_cases as H
import refine_oracle
import simulate_cases as C
import simulate_oracle as O
from gnss_dsp_tools_amd import _native as nat
from gnss_dsp_tools_amd import chiptrack, codes, longtrack, secondary, simulate, trackloop


def test_philox_known_answers():
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        assert O.philox4x32_10(ctr, key) == want
    # the vectorised form the noise uses: counter (j lo, j hi, 0, 0), key = seed, against the scalar one
    seed, j0 = 0xDEADBEEFCAFEF00D, 2 ** 33 - 3
    r0, r1 = O.philox_words(seed, j0, 6)
    for i in range(6):
        j = j0 + i
        w = O.philox4x32_10((j & 0xffffffff, j >> 32, 0, 0), (seed & 0xffffffff, seed >> 32))
        assert (int(r0[i]), int(r1[i])) == w[:2]


def test_fixed_point_conversions_against_exact_fractions():
    two64 = 1 << 64
    for carrier, fs in [(251234.5, 6.0e6), (-1677222.3, 12.5e6), (0.0, 6.0e6), (-1e-30, 6.0e6), (5999999.999, 6.0e6), (1.0e9 + 0.1, 69.984e6)]:
        r = carrier / fs
        t = r - math.floor(r)                                        # IEEE double operations, as the definition has them
        F = O.turns_fixed(r)
        assert F == math.floor(Fraction(t) * two64) % two64
        if abs(carrier) <= fs:                                       # the frequency produced is within fs 2^-53 of the request
            exact = Fraction(carrier) / Fraction(fs)
            err = (Fraction(F, two64) - exact) % 1
            assert min(err, 1 - err) < Fraction(1, 2 ** 53)
    assert O.turns_fixed(-1e-30 / 6.0e6) == 0                        # frac rounds to 1.0: a whole turn
    for phase in (0.0, 0.3125, -0.25, 0.999999999, 7.75):
        p = Fraction(phase)
        assert O.turns_fixed(phase) == math.floor((p - math.floor(p)) * two64)
    for rate, fs in [(1.023e6 + 1234.5 / 1540.0, 6.0e6), (1.023e6, C.FS_CHIPSKIP), (10.23e6, 69.984e6), (511.0e3, 125.0e3), (15.999999 * 6.0e6, 6.0e6)]:
        assert O.chips_fixed(rate / fs) == math.floor(Fraction(rate / fs) * two64)
    for phase, L in [(417.37, 1023), (1023 - 0.25, 1023), (0.0, 1023), (767249.75, 767250), (math.nextafter(10230.0, 0.0), 10230)]:
        c0 = O.chips_fixed(phase)
        assert c0 == math.floor(Fraction(phase) * two64) and 0 <= c0 < L * two64


def test_oracle_agrees_with_the_host_generator_of_the_handoff_tests():
    """sigma = 0, one gps-l1 satellite, 6 MS/s, 6000 samples: handoff_cases.recording's formula (cf * j in fp64) before rounding"""
    fs, n, coffset = 6.0e6, 6000, 250000.0
    sat = simulate.Satellite("gps-l1", 7, 3.0, 1234.5, 417.37)
    t = trackloop.TRACKERS["gps-l1"]
    chips = codes.chips(t.code, 7)
    j = np.arange(n, dtype=np.float64)
    cf = (codes.chip_rate(t.code) + sat.doppler / t.scale(7)) / fs
    w = refine_oracle.weight(chips, t.kind, sat.code0, cf, j)
    ang = np.mod((H.carrier_hz("gps-l1", 7, coffset) + sat.doppler) * j / fs, 1.0) * (2 * np.pi)
    want = sat.amp * w * (np.cos(ang) + 1j * np.sin(ang))
    got = O.evaluate(C.oracle_sats([sat], coffset), fs, 0.0, 1, 0, n)
    pos = sat.code0 + cf * j
    away = np.abs(pos - np.rint(pos)) > 1e-6                         # farther than 1e-6 chip from a chip edge
    assert np.count_nonzero(~away) <= 0.001 * n
    assert np.max(np.abs(got - want)[away]) <= 1e-6 * sat.amp


@pytest.mark.parametrize("seed", C.NOISE_SEEDS)
def test_noise_statistics_of_the_oracle(seed):
    sigma = 12.0
    nr, ni = O.noise(seed, sigma, 0, C.NOISE_N)
    got, cap = O.noise_statistics(nr, ni, sigma)
    print(seed, got, cap)
    for k in got:
        assert got[k] <= cap[k], (k, got[k], cap[k])


def _sat(**kw):
    sym = kw.pop("sym", None)
    args = dict(code=b"gps.ca", prn=7, kind=0, periods_per_symbol=1, nsym=0 if sym is None else len(sym), pad=0,
                symbols=None if sym is None else sym.ctypes.data, amp=3.0, carrier_hz=251234.5, carrier_phase=0.0, code_rate_hz=1.023e6, code_phase=417.37)
    args.update(kw)
    return simulate.SimSat(**args)


def bad_calls():
    """(label, expected code or None for any error, keyword changes) of every refusal of gacq_simulate_dev; shared with the GPU test"""
    nan, inf = float("nan"), float("inf")
    sym = np.array([1, -1, 1], dtype=np.int8)
    bad_sym = np.array([1, 0, -1], dtype=np.int8)
    two = np.array([1, 2], dtype=np.int8)
    out = [("K 0", -1, dict(K=0)), ("K 33", -1, dict(K=33)), ("K -1", -1, dict(K=-1)), ("n 0", -1, dict(n=0)), ("n -5", -1, dict(n=-5)),
           ("j0 -1", -1, dict(j0=-1)), ("j0 + n > 2^48", -1, dict(j0=2 ** 48 - 99)), ("j0 > 2^48", -1, dict(j0=2 ** 48 + 1)),
           ("n > 2^48", -1, dict(n=2 ** 48 + 1)), ("fs nan", -1, dict(fs=nan)), ("fs inf", -1, dict(fs=inf)), ("fs 0", -1, dict(fs=0.0)),
           ("fs < 0", -1, dict(fs=-6.0e6)), ("sigma < 0", -1, dict(sigma=-1.0)), ("sigma nan", -1, dict(sigma=nan)), ("sigma inf", -1, dict(sigma=inf)),
           ("sats NULL", -1, dict(sats=None)), ("out NULL", -1, dict(out=None))]
    for field in ("amp", "carrier_hz", "carrier_phase", "code_rate_hz", "code_phase"):
        out += [("%s nan" % field, -1, dict(sat={field: nan})), ("%s inf" % field, -1, dict(sat={field: inf}))]
    out += [("code rate 0", -1, dict(sat=dict(code_rate_hz=0.0))), ("code rate < 0", -1, dict(sat=dict(code_rate_hz=-1.023e6))),
            ("code rate / fs = 16", -1, dict(sat=dict(code_rate_hz=16 * 6.0e6))), ("code phase < 0", -1, dict(sat=dict(code_phase=-0.5))),
            ("code phase = L", -1, dict(sat=dict(code_phase=1023.0))), ("kind -1", -1, dict(sat=dict(kind=-1))), ("kind 6", -1, dict(sat=dict(kind=6))),
            ("nsym -1", -1, dict(sat=dict(nsym=-1))), ("nsym > 2^20", -1, dict(sat=dict(nsym=2 ** 20 + 1, symbols=sym.ctypes.data))),
            ("symbol 0", -1, dict(sat=dict(sym=bad_sym))), ("symbol 2", -1, dict(sat=dict(sym=two))), ("symbols NULL", -1, dict(sat=dict(nsym=3))),
            ("periods_per_symbol 0", -1, dict(sat=dict(periods_per_symbol=0, sym=sym))), ("code NULL", -1, dict(sat=dict(code=None))),
            ("unknown code", -2, dict(sat=dict(code=b"gps.nope"))), ("unknown PRN", -3, dict(sat=dict(prn=999)))]
    return out


def raw_call(ctx, out_ptr, K=2, n=100, j0=0, fs=6.0e6, sigma=12.0, seed=1, cplx=0, sats="default", sat=None, out="default"):
    """gacq_simulate_dev with two good satellites, the second changed by `sat`"""
    arr = (simulate.SimSat * 33)(*([_sat(), _sat(**(sat or {}))] + [_sat() for _ in range(31)]))
    return nat.lib.gacq_simulate_dev(ctx, None if sats is None else ctypes.addressof(arr), K, fs, sigma, seed, j0, n, cplx,
                                     ctypes.c_void_p(None if out is None else out_ptr))


def test_every_refusal_without_a_device():
    """a NULL context: nothing may be touched, every call comes back with an error"""
    buf = np.zeros(256, dtype=np.int8)
    assert raw_call(None, buf.ctypes.data) < 0
    for label, code, change in bad_calls():
        assert raw_call(None, buf.ctypes.data, **change) < 0, label
    assert not buf.any()
    assert ctypes.sizeof(simulate.SimSat) == 80


def test_satellite_fills_the_struct_as_the_trackers_model_a_signal():
    coffset = 250000.0
    s, sym = simulate.Satellite("gps-l1", 7, 3.0, 1234.5, 417.37, 0.25, [1, -1, -1], 20).struct(coffset)
    assert (s.code, s.prn, s.kind, s.periods_per_symbol, s.nsym) == (b"gps.ca", 7, 0, 20, 3) and sym.dtype == np.int8 and s.symbols == sym.ctypes.data
    assert (s.amp, s.carrier_hz, s.carrier_phase, s.code_rate_hz, s.code_phase) == (3.0, coffset + 1234.5, 0.25, 1.023e6 + 1234.5 / 1540.0, 417.37)
    s, sym = simulate.Satellite("gps-l2cl", 9, 2.0, -455.5, 1000.5).struct(coffset)          # a long-code tracker
    t = longtrack.LONG_TRACKERS["gps-l2cl"]
    assert (s.code, s.prn, s.kind, s.nsym, s.symbols, sym) == (b"gps.l2cl", 9, 5, 0, None, None)
    assert s.code_rate_hz == codes.chip_rate(t.code) - 455.5 / 2400.0 and s.carrier_hz == coffset - 455.5
    s, _ = simulate.Satellite("beidou-b2bi", 21, 2.0, 900.0, 10.0).struct(coffset)           # a chip tracker
    assert (s.code, s.prn, s.kind) == (b"beidou.b2bi", 21, chiptrack.CHIP_TRACKERS["beidou-b2bi"].kind) and s.code_rate_hz == 10.23e6 + 900.0 / 118.0
    for chan in (-3, 5):                                                                       # GLONASS L1: an RF channel of either sign
        s, _ = simulate.Satellite("glonass-l1", chan, 3.0, 777.7, 301.81).struct(coffset)
        t = trackloop.TRACKERS["glonass-l1"]
        assert (s.code, s.prn, s.kind) == (b"glonass.ca", 0, 0)
        assert s.carrier_hz == coffset + 562500 * chan + 777.7 == H.carrier_hz("glonass-l1", chan, coffset) + 777.7
        assert s.code_rate_hz == 511000.0 + 777.7 / ((1602.0 + 0.5625 * chan) / 0.511) == 511000.0 + 777.7 / t.scale(chan)
    s, _ = simulate.Satellite("glonass-l2-p", -7, 3.0, 100.0, 5.0).struct(0.0)
    assert (s.code, s.prn) == (b"glonass.p", 0) and s.carrier_hz == 437500 * -7 + 100.0
    with pytest.raises(KeyError):
        simulate.Satellite("gps-l9", 1, 1.0, 0.0, 0.0).struct(0.0)


def test_symbols_are_overlay_times_data_bits():
    bits = 1 - 2 * np.random.Generator(np.random.PCG64(5)).integers(0, 2, size=13)
    s = simulate.symbols("gps-l1", 7, 13, 20, 5)                     # no overlay: the bits, 20 periods each
    assert s.dtype == np.int8 and len(s) == 260 and np.array_equal(s, np.repeat(bits, 20)) and set(np.unique(s)) == {-1, 1}
    s = simulate.symbols("beidou-b1i", 8, 13, 20, 5)                 # the 20-chip Neumann-Hoffman code under every bit
    assert np.array_equal(s.reshape(13, 20), bits[:, None] * secondary.SECONDARY["beidou.b1i"][None, :])
    s = simulate.symbols("galileo-e5aq", 3, 2, 100, 9)               # a per-PRN overlay
    bits = 1 - 2 * np.random.Generator(np.random.PCG64(9)).integers(0, 2, size=2)
    assert np.array_equal(s.reshape(2, 100), bits[:, None] * secondary.SECONDARY["galileo.e5aq"][3][None, :])
    with pytest.raises(ValueError):
        simulate.symbols("gps-l1", 7, 2 ** 20, 2, 5)


def test_command_line_parsing():
    a, sats = simulate.parse(["--fs", "6e6", "--coffset", "-250000", "--seconds", "0.25", "--seed", "31", "--sat", "gps-l1,7,3,1234.5,417.37,20",
                              "--sat", "glonass-l1,-3,3.0,-777.7,301.81", "--sigma", "10", "out.bin"])
    assert (a.fs, a.coffset, a.seconds, a.seed, a.sigma, a.output_filename) == (6.0e6, -250000.0, 0.25, 31, 10.0, "out.bin")
    assert [(s.tracker, s.item, s.amp, s.doppler, s.code0) for s in sats] == [("gps-l1", 7, 3.0, 1234.5, 417.37), ("glonass-l1", -3, 3.0, -777.7, 301.81)]
    assert sats[1].symbols is None and sats[0].periods_per_symbol == 1
    assert len(sats[0].symbols) == 260 and np.array_equal(sats[0].symbols, simulate.symbols("gps-l1", 7, 13, 20, 31))      # 251 periods -> 13 bits
    assert simulate.track_line(sats[1], "out.bin", a.fs, a.coffset).split() == ["glonass-l1", "out.bin", "6000000.0", "-250000.0", "-3", "-777.7", "301.81"]
    assert simulate.parse(["--fs", "6e6", "--coffset", "0", "--seconds", "1", "--seed", "1", "--sat", "gps-l1,7,3,0,0", "o"])[0].sigma == 12.0
    for bad in (["--fs", "6e6", "--coffset", "0", "--seconds", "1", "--seed", "1", "o"],                                    # no satellite
                ["--fs", "6e6", "--coffset", "0", "--seconds", "1", "--seed", "1", "--sat", "gps-l1,7,3,0", "o"],          # a field short
                ["--fs", "6e6", "--coffset", "0", "--seconds", "1", "--seed", "1", "--sat", "gps-l9,7,3,0,0", "o"],        # unknown tracker
                ["--fs", "0", "--coffset", "0", "--seconds", "1", "--seed", "1", "--sat", "gps-l1,7,3,0,0", "o"]):
        with pytest.raises(SystemExit):
            simulate.parse(bad)
