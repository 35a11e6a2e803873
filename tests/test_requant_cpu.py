"""CPU: the numpy definition of the level control and requantiser (tests/requant_oracle.py) read against include/gacq.h -- the tables,
the packed codes read back through ingest's oracle, the loop's answer to an amplitude step, the default target levels of the few-bit
formats against a sweep -- and, of the library, what needs no device: the refusals of gacq_requant_check, the parser and the report."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

import ingest_oracle as IO
import requant_cases as C
import requant_oracle as O
from gnss_dsp_tools_amd import _native as nat
from gnss_dsp_tools_amd import ingest, requant

BAD_ARG, SHORT_INPUT = -1, -6


def test_tables_are_monotone_and_the_thresholds_exact():
    for target, Lb, W in ((32.0, 4096, 8), (2.84, 16, 1), (8192.0, 65536, 64), (8.44, 1024, 3)):
        G, T = requant.tables(target, Lb, W)
        assert G.dtype == np.float32 and T.dtype == np.uint64 and len(G) == 128 and len(T) == 127
        assert np.all(G[1:] < G[:-1]) and G[0] == np.float32(64.0) and np.all(np.isfinite(G)) and np.all(G > 0)
        assert all(int(T[i]) <= int(T[i + 1]) for i in range(126))
        assert np.array_equal(G[::8], np.float32(64.0) * np.float32(2.0) ** -np.arange(16, dtype=np.float32))           # every eighth step a factor of 2
        for i in range(127):
            assert int(T[i]) == min(Fraction(target) ** 2 * W * Lb // Fraction(float(G[i])) ** 2, (1 << 64) - 1), i     # the cap lies above every level
        # what the threshold means: a level just above T[i] puts gain i over the target, T[i] itself does not
        for i in (0, 17, 100):
            g2 = Fraction(float(G[i])) ** 2
            assert g2 * int(T[i]) <= Fraction(target) ** 2 * W * Lb < g2 * (int(T[i]) + 1)
    G, T = requant.tables(32.0, 4096, 8, step=4, K=5, g_max=2.0)
    assert len(G) == 5 and len(T) == 4 and G[4] == 1.0
    G, T = requant.fixed(2.5)
    assert G.tolist() == [2.5] and len(T) == 0
    for bad in (dict(target_rms=0.0), dict(target_rms=float("nan")), dict(K=0), dict(K=257), dict(step=0), dict(g_max=0.0)):
        with pytest.raises(ValueError):
            requant.tables(**dict(dict(target_rms=32.0, block=4096, window=8), **bad))


def test_enc_inverts_the_presets_of_ingest():
    for name in C.PRESETS:
        f = requant.OutFormat(name)
        n = 1 << f.bits
        assert sorted(f.enc) == list(range(n)) and f.enc == O.enc_of_lut(IO.preset(f.bits, name[1:]))
        assert [ingest.preset_lut(f.bits, name[1:])[f.enc[q]] for q in range(n)] == [2 * q - (n - 1) for q in range(n)]
        assert f.unit == 4 // f.bits and f.nbytes(8) == 2 * f.bits
    assert [requant.OutFormat(n).sample_bits for n in C.CONTAINERS] == [16, 16, 32, 64]
    assert requant.OutFormat("2sm").ingest_args() == "--format 2sm" and requant.OutFormat("4tc", msb_first=False).ingest_args() == "--format 4tc --lsb-first"
    with pytest.raises(ValueError):
        requant.OutFormat("3sm")


@pytest.mark.parametrize("name", C.PRESETS)
@pytest.mark.parametrize("msb", [True, False], ids=["msb", "lsb"])
def test_packed_output_read_back_by_ingest_gives_the_levels(name, msb):
    fmt = requant.OutFormat(name, msb)
    n = 1 << fmt.bits
    x = C.signal(4096, 11)
    G, T = C.tables_for(fmt, 64, 3)
    c = C.ocfg(fmt, 64, 3)
    out, clipped, blocks, k = O.evaluate(c, G, T, x)
    assert len(out) == fmt.nbytes(4096) and blocks == 64 and len(k) == 64 and len(set(k.tolist())) > 3
    # the levels from the definition, in float64 of the float32 product
    g = np.repeat(G[k.astype(np.int64)[np.arange(4096) // 64]], 2)
    v = (x.astype(np.float32) * g).astype(np.float64)
    q = np.clip(np.floor(v / 2.0) + n // 2, 0, n - 1).astype(np.int64)
    got = IO.values(IO.fmt(name, msb_first=msb), out.tobytes())
    assert np.array_equal(got, 2 * q - (n - 1)) and np.array_equal(got, O.levels_of_codes(c, out))
    assert clipped == int(np.count_nonzero((np.floor(v / 2.0) + n // 2 < 0) | (np.floor(v / 2.0) + n // 2 > n - 1)))
    assert set(np.unique(got).tolist()) == set(range(-(n - 1), n, 2))                        # every level is used
    # v in [0, 2) is +1, [-2, 0) is -1
    assert np.all(got[(v >= 0) & (v < 2)] == 1) and (n == 2 or np.all(got[(v >= -2) & (v < 0)] == -1))


def test_every_container_of_the_oracle_on_a_ramp():
    """all int8 values under gains that put them on ties, on the level edges and past both clip limits"""
    x = np.arange(-128, 128, dtype=np.int8)
    data = np.stack([x, x[::-1]], axis=1).reshape(-1)
    for gain in (0.5, 1.0, 1.5):
        G, T = requant.fixed(gain)
        v = x.astype(np.float64) * gain
        s8 = O.evaluate(O.cfg("s8", 16, 1), G, T, data)
        want = np.clip(np.rint(v), -127, 127)
        assert np.array_equal(s8[0].view(np.int8)[0::2], want) and s8[1] == 2 * int(np.count_nonzero(np.abs(np.rint(v)) > 127)) and s8[2] == 16
        assert np.array_equal(s8[0].view(np.int8), IO.evaluate(IO.fmt("s8"), data.tobytes(), gain))        # ingest's rule for int8
        u8 = O.evaluate(O.cfg("u8", 16, 1), G, T, data)
        assert np.array_equal(u8[0][0::2].astype(np.int64), want + 128) and u8[1] == s8[1]
        s16 = O.evaluate(O.cfg("s16", 16, 1), G, T, data)
        assert np.array_equal(s16[0].view("<i2")[0::2], np.rint(v)) and s16[1] == 0
        f32 = O.evaluate(O.cfg("f32", 16, 1), G, T, data)
        assert np.array_equal(f32[0].view("<f4")[0::2], v.astype(np.float32)) and f32[1] == 0
    G, T = requant.fixed(0.5)
    s8 = O.evaluate(O.cfg("s8", 16, 1), G, T, data)[0].view(np.int8)[0::2]
    assert s8[128 + 1] == 0 and s8[128 + 3] == 2 and s8[128 + 5] == 2 and s8[128 - 1] == 0 and s8[128 - 3] == -2          # ties to even
    ob = O.evaluate(O.cfg("packed", 16, 1, bits=2, enc=[0, 1, 2, 3]), G, T, data)
    lev = O.levels_of_codes(O.cfg("packed", 16, 1, bits=2, enc=[0, 1, 2, 3]), ob[0])[0::2]
    assert lev[128 + 4] == 3 and lev[128 + 3] == 1 and lev[128] == 1 and lev[128 - 1] == -1 and lev[128 - 4] == -1 and lev[128 - 5] == -3
    assert ob[1] == 2 * int(np.count_nonzero((x * 0.5 >= 4) | (x * 0.5 < -4)))


def test_warm_up_and_sliding_level():
    c = O.cfg("s8", 16, 3)
    P = np.array([10, 20, 30, 40, 50, 60], dtype=np.uint64)
    assert O.levels(c, P, 7).tolist() == [60, 60, 60, 60, 90, 120, 150]
    assert O.gain_indices([59, 60, 61, 149], O.levels(c, P, 7)).tolist() == [1, 1, 1, 1, 3, 3, 4]
    assert O.out_count(c, 47) == 0 and O.out_count(c, 48) == 48 and O.out_count(c, 49) == 49
    p2 = O.cfg("packed", 16, 3, bits=1, enc=[0, 1])
    assert O.out_count(p2, 51) == 48 and O.unit(p2) == 4
    x = np.full(2 * 48, -32768, dtype=np.int16)
    assert O.block_powers(O.cfg("s8", 16, 3, in_bits=16), x).tolist() == [16 << 31] * 3


def test_the_loop_settles_after_an_amplitude_step():
    """per-component sigma 3 steps to 24: the output clips until the window holds only loud blocks, then the rms is back inside one
    table step below the target"""
    Lb, W, target = 1024, 4, 32.0
    rng = np.random.default_rng(3)
    nb, step_block = 40, 16
    v = rng.standard_normal((nb * Lb, 2)) * 3.0
    v[step_block * Lb:] *= 8.0
    x = np.clip(np.rint(v), -128, 127).astype(np.int8).reshape(-1)
    G, T = requant.tables(target, Lb, W)
    c = O.cfg("s8", Lb, W)
    out = O.evaluate(c, G, T, x)[0].view(np.int8).astype(np.float64).reshape(nb, 2 * Lb)
    rms = np.sqrt((out ** 2).sum(axis=1) / Lb)
    settled = np.sqrt(np.mean(rms[step_block + W + 1:] ** 2))
    before = np.sqrt(np.mean(rms[W + 1:step_block] ** 2))
    print("rms before the step %.2f, per block after it %s, settled %.2f" % (before, np.round(rms[step_block:step_block + W + 2], 1), settled))
    lo, hi = target * 2.0 ** (-1.0 / 8.0) * 0.95, target * 1.05
    assert lo <= before <= hi and lo <= settled <= hi
    assert np.all((rms[step_block + W + 1:] >= lo) & (rms[step_block + W + 1:] <= hi))
    # until then the output clips: the first loud block under the quiet blocks' gain most of all (later ones may happen not to)
    assert O.evaluate(c, G, T, x, step_block * Lb, Lb)[1] > 100
    assert O.evaluate(c, G, T, x, step_block * Lb, W * Lb)[1] > 0
    assert O.evaluate(c, G, T, x, (step_block + W + 1) * Lb, Lb)[1] == 0


def _rho(a, b):
    return float(np.dot(a, b) / np.sqrt(np.dot(a, a) * np.dot(b, b)))


@pytest.mark.parametrize("bits", [2, 4])
def test_default_target_lies_within_one_percent_of_the_best_correlation(bits):
    """Gaussian noise of per-component sigma 4.2, rounded to int8, through the level control to `bits` bits at target levels from a
    quarter to four times the default: the correlation coefficient of the levels with the unrounded noise.  Measured: 2 bits 0.9352 at
    the default 2.84, the best of the sweep (0.9329 a quarter octave up, 0.9252 down); 4 bits 0.9909 at 8.44, the best as well (0.9902 up,
    0.9900 down).  The level control leaves the level up to one table step (0.75 dB) below the target, which is part of what is measured."""
    rng = np.random.default_rng(2)
    n, Lb, W = 1 << 16, 1024, 8
    z = rng.standard_normal(2 * n) * 4.2
    x = np.clip(np.rint(z), -128, 127).astype(np.int8)
    fmt = requant.OutFormat("%dob" % bits)
    c = C.ocfg(fmt, Lb, W)
    rho = {}
    for j in range(-8, 9):
        target = fmt.target_rms * 2.0 ** (j / 4.0)
        G, T = requant.tables(target, Lb, W)
        rho[j] = _rho(O.levels_of_codes(c, O.evaluate(c, G, T, x)[0]).astype(np.float64), z)
    best = max(rho.values())
    print("%d bits: default %.4f, best %.4f at %.2f x default; sweep %s" % (bits, rho[0], best, 2.0 ** (max(rho, key=rho.get) / 4.0),
                                                                           " ".join("%.4f" % rho[j] for j in sorted(rho))))
    assert rho[0] >= 0.99 * best
    assert abs(rho[0] - (0.936 if bits == 2 else 0.993)) <= 0.005


def raw_check(container=0, in_bits=8, bits=0, block=64, window=3, K=4, enc=None, gains=None, thresholds=None, in_first=0, in_count=1000, out_first=0,
              n_out=1000, cfg=True, null_gains=False, null_thr=False, handle=None, src=1 << 20, dst=1 << 21, stats=0, gidx=0):
    """gacq_requant_check (no device), or with a handle gacq_requant_run_dev; the addresses are only looked at by the checks"""
    if handle is not None:
        return nat.lib.gacq_requant_run_dev(handle, ctypes.c_void_p(src), in_first, in_count, out_first, n_out, ctypes.c_void_p(dst), ctypes.c_void_p(stats),
                                            ctypes.c_void_p(gidx))
    g = np.ascontiguousarray([4.0, 2.0, 1.0, 0.5][:K] if gains is None else gains, dtype=np.float32)
    t = np.ascontiguousarray([100, 200, 200][:max(K - 1, 0)] if thresholds is None else thresholds, dtype=np.uint64)
    e = list(range(min(1 << bits, 16))) if enc is None else list(enc)
    st = requant.RequantCfg(in_bits=in_bits, container=container, bits=bits, msb_first=1, block=block, window=window, ngains=K,
                            enc=(ctypes.c_uint8 * 16)(*(e + [0] * (16 - len(e)))))
    return nat.lib.gacq_requant_check(ctypes.addressof(st) if cfg else None, None if null_gains else ctypes.c_void_p(g.ctypes.data),
                                      None if null_thr or not len(t) else ctypes.c_void_p(t.ctypes.data), in_first, in_count, out_first, n_out)


def bad_config_calls():
    """(label, expected code, changed arguments): what gacq_requant_check and gacq_requant_open refuse"""
    nan, inf = float("nan"), float("inf")
    out = [("NULL cfg", BAD_ARG, dict(cfg=False)), ("NULL gains", BAD_ARG, dict(null_gains=True)), ("NULL thresholds", BAD_ARG, dict(null_thr=True))]
    out += [("in_bits %d" % v, BAD_ARG, dict(in_bits=v)) for v in (0, 4, 12, 32)]
    out += [("container %d" % v, BAD_ARG, dict(container=v)) for v in (-1, 5)]
    out += [("block %d" % v, BAD_ARG, dict(block=v)) for v in (0, -16, 8, 24, 65552, 1 << 17)]
    out += [("window %d" % v, BAD_ARG, dict(window=v)) for v in (0, -1, 65)]
    out += [("K %d" % v, BAD_ARG, dict(K=v, gains=np.ones(max(v, 1)), thresholds=np.zeros(max(v - 1, 1)))) for v in (0, -1, 257)]
    out += [("bits %d" % v, BAD_ARG, dict(container=4, bits=v)) for v in (0, 3, 8)]
    out += [("enc %r" % (v,), BAD_ARG, dict(container=4, bits=2, enc=v)) for v in ([0, 1, 2, 2], [0, 1, 2, 4], [1, 1, 1, 1])]
    out += [("gain %r" % v, BAD_ARG, dict(gains=[4.0, v, 1.0, 0.5])) for v in (0.0, -1.0, nan, inf, 1e-46)]
    out += [("thresholds descend", BAD_ARG, dict(thresholds=[100, 99, 200])), ("the last threshold descends", BAD_ARG, dict(thresholds=[100, 200, 199]))]
    return out


def bad_run_calls():
    """... and what gacq_requant_check and gacq_requant_run_dev refuse; the default call is Lb = 64, W = 3, 1000 samples from 0, all of them out"""
    out = []
    for k in ("in_first", "in_count", "out_first", "n_out"):
        out += [("%s %s" % (k, v), BAD_ARG, {k: v}) for v in (-1, (1 << 48) + 1)]
    out += [("the output's last sample is missing", SHORT_INPUT, dict(in_count=999)), ("nothing present", SHORT_INPUT, dict(in_count=0)),
            ("fewer than W blocks", SHORT_INPUT, dict(in_count=191, n_out=191)), ("fewer than W blocks, one output", SHORT_INPUT, dict(in_count=191, n_out=1)),
            ("the window's first block is cut", SHORT_INPUT, dict(in_first=257, in_count=743, out_first=448, n_out=552)),
            ("the warm-up needs block 0", SHORT_INPUT, dict(in_first=64, in_count=936, out_first=64, n_out=936))]
    return out


def test_every_refusal_through_gacq_requant_check_without_a_device():
    for label, code, change in bad_config_calls() + bad_run_calls():
        assert raw_check(**change) == code, (label, nat.lib.gacq_last_error(None))
        assert nat.lib.gacq_last_error(None).startswith(b"gacq_requant: "), label   # every message names its own tool
    assert b"need input samples" in nat.lib.gacq_last_error(None)
    assert raw_check() == 0 and raw_check(n_out=0, in_count=0) == 0 and raw_check(in_count=192, n_out=192) == 0 and raw_check(in_count=193, n_out=193) == 0
    assert raw_check(in_first=256, in_count=744, out_first=448, n_out=552) == 0                 # block 7 needs blocks 4 .. 6
    assert raw_check(thresholds=[100, 100, 100]) == 0 and raw_check(K=1) == 0 and raw_check(K=1, null_thr=True) == 0
    assert raw_check(K=256, gains=np.ones(256), thresholds=np.arange(255)) == 0 and raw_check(block=65536, window=64, in_count=1 << 22, n_out=1 << 22) == 0
    # packed: whole bytes
    for bits, unit in ((1, 4), (2, 2), (4, 1)):
        assert raw_check(container=4, bits=bits) == 0
        for k in ("out_first", "n_out"):
            assert raw_check(**dict(dict(container=4, bits=bits, out_first=200, n_out=400), **{k: 201})) == (BAD_ARG if unit > 1 else 0), (bits, k)
            assert raw_check(**dict(dict(container=4, bits=bits, out_first=200, n_out=400), **{k: 202})) == (BAD_ARG if unit > 2 else 0), (bits, k)
    assert nat.lib.gacq_requant_run_dev(None, ctypes.c_void_p(1 << 20), 0, 1000, 0, 1000, ctypes.c_void_p(1 << 21), None, None) == BAD_ARG   # no handle
    h = ctypes.c_void_p()
    st = requant.make_cfg("s8", 64, 3, 1)
    g = np.ones(1, dtype=np.float32)
    assert nat.lib.gacq_requant_open(None, ctypes.addressof(st), ctypes.c_void_p(g.ctypes.data), None, ctypes.byref(h)) == BAD_ARG and not h.value
    assert ctypes.sizeof(requant.RequantCfg) == 48
    for name in C.CONTAINERS + C.PRESETS:
        st = requant.make_cfg(name, 64, 3, 1)
        assert nat.lib.gacq_requant_tile(ctypes.addressof(st)) == C.tile(name), name
    st = requant.make_cfg("s8", 65, 3, 1)
    assert nat.lib.gacq_requant_tile(ctypes.addressof(st)) == BAD_ARG and nat.lib.gacq_requant_tile(None) == BAD_ARG


def test_out_end_and_first_needed():
    f1, f8 = requant.OutFormat("1ob"), requant.OutFormat("s8")
    for fmt in (f1, f8):
        for n in (0, 1, 191, 192, 193, 194, 195, 196, 1000):
            assert requant.out_end(fmt, 64, 3, n) == O.out_count(C.ocfg(fmt, 64, 3), n)
    assert [requant.first_needed(64, 3, o) for o in (0, 63, 64, 191, 192, 255, 256, 1000)] == [0, 0, 0, 0, 0, 0, 64, 768]


def test_command_line_parser_and_report_lines():
    a, fmt, G, T = requant.parse(["--format", "2sm", "in.iq", "out.2b"])
    assert (a.input_filename, a.output_filename, a.block, a.window, a.gain, a.target_rms, a.in_format, a.trace) == ("in.iq", "out.2b", 4096, 8, None, None, "s8",
                                                                                                                     None)
    assert fmt.name == "2sm" and fmt.msb_first and len(G) == 128
    G2, T2 = requant.tables(2.84, 4096, 8)
    assert np.array_equal(G, G2) and np.array_equal(T, T2)
    a, fmt, G, T = requant.parse(["--format", "4ob", "--lsb-first", "--in-format", "s16", "--block", "1024", "--window", "3", "--target-rms", "9.5", "--trace",
                                  "k.bin", "-", "-"])
    assert (a.block, a.window, a.in_format, a.trace, a.input_filename, a.output_filename) == (1024, 3, "s16", "k.bin", "-", "-") and not fmt.msb_first
    assert np.array_equal(T, requant.tables(9.5, 1024, 3)[1])
    a, fmt, G, T = requant.parse(["--format", "s16", "--gain", "2.5", "a", "b"])
    assert G.tolist() == [2.5] and len(T) == 0
    assert [requant.OutFormat(n).target_rms for n in ("s8", "u8", "s16", "f32", "1sm", "2tc", "4sm")] == [32.0, 32.0, 8192.0, 32.0, 2.84, 2.84, 8.44]
    lines = requant.report_lines(requant.OutFormat("2sm"), 4096, 8, G2, 40, 64, 17, 123456)
    assert lines == ["format 2sm block 4096 window 8 gain %r .. %r clipped 17 samples 123456" % (float(G2[64]), float(G2[40])), "ingest --format 2sm"]
    assert float(G2[64]) == 0.25 and float(G2[40]) == 2.0
    assert requant.report_lines(requant.OutFormat("1ob", False), 16, 1, G2, None, None, 0, 0)[1] == "ingest --format 1ob --lsb-first"
    for bad in (["in", "out"], ["--format", "3sm", "in", "out"], ["--format", "s8", "--block", "100", "in", "out"], ["--format", "s8", "--window", "0", "in", "out"],
                ["--format", "s8", "--gain", "0", "in", "out"], ["--format", "s8", "--gain", "2", "--target-rms", "3", "in", "out"],
                ["--format", "s8", "--target-rms", "nan", "in", "out"], ["--format", "s8", "--in-format", "u8", "in", "out"], ["--format", "s8", "in"]):
        with pytest.raises((SystemExit, ValueError)):
            requant.parse(bad)
