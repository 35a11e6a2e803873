"""CPU: the numpy definition of space-time nulling (tests/stap_oracle.py) read against include/gacq.h -- its solve against numpy's at
the sizes the taps bring, its covariance against the plain complex sum of the stacked vectors, T = 1 against tests/nulling_oracle.py,
the independence of cuts, the reference element's unit weight, the int32 bound, the rounding-tie margin of every shared case -- and,
of the library, what needs no device: the refusals of gacq_stap_check through the raw ABI in their pinned order, the block / window /
tap algebra, the parser and the report."""
import ctypes

import numpy as np
import pytest

import nulling_cases as NC
import nulling_oracle as NO
import stap_cases as C
import stap_oracle as O
from gnss_dsp_tools_amd import _native as nat
from gnss_dsp_tools_amd import stap

BAD_ARG, SHORT_INPUT = -1, -6


@pytest.mark.parametrize("M,T", [(1, 3), (1, 15), (5, 5), (8, 7)])
def test_the_solve_agrees_with_numpy_and_the_covariance_is_the_sum_of_stacked_vectors(M, T):
    N, Lb, tc = M * T, 256, O.centre(T)
    assert N in (3, 15, 25, 56)
    xs = NC.recording(M, 5 * Lb + tc, 60 + N)
    Cre, Cim = O.block_cov(xs, T, Lb, 0, 0, 5)
    c = O.constraint(M, T, None if M % 2 else np.exp(2j * np.pi * 0.17 * np.arange(M) ** 2))
    assert np.count_nonzero(c) == (1 if M % 2 else M) == np.count_nonzero(c[tc::T]) and c[tc] == 1.0
    Are, Aim = NO.loaded(Cre.sum(axis=0)[None], Cim.sum(axis=0)[None], 10)                       # five blocks: 1280 samples under 56 weights
    ur, ui = NO.solve(Are, Aim, c)
    want = np.linalg.solve(Are[0] + 1j * Aim[0], c)
    assert np.max(np.abs(ur[0] + 1j * ui[0] - want)) <= 1e-9 * np.max(np.abs(want)), (M, T)
    # the stacked vector of sample j, written out: z_e(j) = x_p(j + t_c - t), zero below the recording
    z = np.zeros((N, 2 * Lb), dtype=np.complex128)
    for p in range(M):
        i, q = NO.split(xs[p])
        x = i + 1j * q
        for t in range(T):
            for j in range(2 * Lb):
                if j + tc - t >= 0:
                    z[p * T + t, j] = x[j + tc - t]
    for b in range(2):
        S = z[:, b * Lb:(b + 1) * Lb] @ np.conj(z[:, b * Lb:(b + 1) * Lb]).T
        assert np.array_equal(Cre[b], np.rint(S.real).astype(np.int64)) and np.array_equal(Cim[b], np.rint(S.imag).astype(np.int64)), (M, T, b)
        assert np.array_equal(Cre[b], Cre[b].T) and np.array_equal(Cim[b], -Cim[b].T)
    if T > 1:                                       # exact, not Toeplitz: the diagonal of one antenna's taps differs by the edge samples
        assert Cre[1, 0, 0] != Cre[1, 1, 1]


@pytest.mark.parametrize("name", ["m2-b64-w3", "m5-b128-w1", "m8-b128-w3"])
def test_one_tap_is_the_nulling_oracle_bit_for_bit(name):
    M, Lb, W = NC.CASES[name][:3]
    xs = list(NC.data(name))
    n = len(xs[0]) // 2
    for complex64 in (False, True):
        a = NO.run(xs, 0, 0, n, Lb, W, 10, None, 0.75, complex64)
        b = O.run(xs, 0, 0, n, Lb, W, 1, 10, None, 0.75, complex64)
        assert all(np.array_equal(a[k], b[k]) and a[k].dtype == b[k].dtype for k in ("out", "wq", "cov", "wq_all", "blocks"))
        assert (a["clipped"], a["owned"], a["margin"]) == (b["clipped"], b["owned"], b["margin"])
    assert O.needed(Lb, W, 1, 5 * Lb + 1, 7) == NO.needed(Lb, W, 5 * Lb + 1, 7) and O.supported(Lb, W, 1, 0, n) == NO.supported(Lb, W, 0, n)


@pytest.mark.parametrize("name", ["m2-t5-b128-w3", "m1-t15-b64-w1", "m8-t7-b128-w3"])
@pytest.mark.parametrize("complex64", [False, True], ids=["int8", "complex64"])
def test_the_oracle_on_cuts_is_the_oracle_on_the_whole(name, complex64):
    M, T, Lb, W = C.CASES[name][:4]
    xs = C.data(name)
    n = C.outputs(name)
    whole = C.reference(name, complex64, 0.75)
    pts = [0, W * Lb + 3, (W + 1) * Lb, (W + 1) * Lb + 8, n - 11, n]
    outs, clipped, owned, wq = [], 0, 0, []
    for a, b in zip(pts, pts[1:]):
        lo, hi = O.needed(Lb, W, T, a, b - a)
        r = O.run([x[2 * lo:2 * hi] for x in xs], lo, a, b - a, Lb, W, T, 10, C.constraint(name), 0.75, complex64)
        outs.append(r["out"])
        clipped, owned = clipped + r["clipped"], owned + r["owned"]
        wq.append(r["wq"])
        short = [([x[2 * lo:2 * hi - 2] for x in xs], lo)] + ([([x[2 * lo + 2:2 * hi] for x in xs], lo + 1)] if lo else [])
        for cut, first in short:                                                                # one sample short at either end
            with pytest.raises(ValueError):
                O.run(cut, first, a, b - a, Lb, W, T, 10, C.constraint(name), 0.75, complex64)
    assert np.array_equal(np.concatenate(outs), whole["out"]) and (clipped, owned) == (whole["clipped"], whole["owned"])
    assert np.array_equal(np.concatenate(wq), whole["wq"]) and owned == -(-n // Lb)
    assert all(np.array_equal(whole["wq"][b], whole["wq"][0]) for b in range(W + 1)) and not np.array_equal(whole["wq"][W + 1], whole["wq"][0])


def test_the_reference_element_passes_with_unit_gain_and_the_constraint_holds():
    for name in C.CASES:
        M, T = C.CASES[name][:2]
        r = C.reference(name)
        tc = O.centre(T)
        if C.constraint(name) is None:
            assert np.all(r["wq_all"][:, tc, 0] == O.WQ) and np.all(r["wq_all"][:, tc, 1] == 0), name
        else:
            w = r["wq_all"].astype(np.float64) / O.WQ
            z = w[:, tc::T, 0] + 1j * w[:, tc::T, 1]
            assert np.max(np.abs(z @ np.conj(C.STEER) - 1.0)) < 1e-3, name                       # c^H w = 1 up to the quantisation


def test_the_int32_bound_of_the_apply():
    """N <= 56 keeps every partial sum below 2^31 whatever the weights: the oracle asserts the bound of each sample, and the largest
    configuration at the largest weights and samples stays inside; one more weight pair would not"""
    assert 2 * O.MAX_WEIGHTS * O.WQ_MAX * 128 < 1 << 31 <= 2 * 66 * O.WQ_MAX * 128
    xs = [np.full(2 * 200, -128, dtype=np.int8) for _ in range(8)]
    r = O.run(xs, 0, 0, 190, 64, 1, 7, 40, None, 1.0, True)                                       # no loading to speak of: large weights
    assert np.abs(r["wq_all"]).max() <= O.WQ_MAX
    with pytest.raises(AssertionError):
        O.run(xs + xs[:1], 0, 0, 190, 64, 1, 7)


def test_every_case_keeps_its_distance_from_a_rounding_tie():
    m = C.check_margins()
    assert len(m) == len(C.CASES) == 21 and min(m.values()) >= C.MARGIN, m
    assert set(C.CASES[n][:2] for n in C.CASES if n.endswith("b128-w3") and n[0] == "m") == set(C.SHAPES)


def _cfg(**kw):
    d = dict(M=4, taps=5, block=4096, window=8, load_shift=10, constraint=None)
    d.update(kw)
    return stap.make_cfg(d["M"], d["taps"], d["block"], d["window"], d["load_shift"], d["constraint"])


def _check(cfg, in_first=0, in_count=1 << 20, out_first=0, n_out=(1 << 20) - 7, gain=1.0, cplx=0):
    return nat.lib.gacq_stap_check(ctypes.addressof(cfg) if cfg is not None else None, in_first, in_count, out_first, n_out, gain, cplx)


def _error():
    return nat.lib.gacq_last_error(None).decode()


def test_gacq_stap_check_refuses_through_the_raw_abi():
    assert _check(_cfg()) == 0 and _check(_cfg(), cplx=1) == 0
    assert _check(None) == BAD_ARG
    for bad in (dict(M=0), dict(M=9), dict(taps=0), dict(taps=2), dict(taps=4), dict(taps=16), dict(taps=17), dict(taps=-1), dict(M=8, taps=9),
                dict(M=4, taps=15), dict(M=3, taps=19), dict(block=0), dict(block=32), dict(block=96), dict(block=65536), dict(block=32768 + 64),
                dict(window=0), dict(window=65), dict(load_shift=-1), dict(load_shift=41)):
        assert _check(_cfg(**bad)) == BAD_ARG, bad
        assert _error().startswith("gacq_stap: "), bad                                          # every message names its own tool
        c = _cfg(**bad)
        assert nat.lib.gacq_stap_tile(ctypes.addressof(c)) == BAD_ARG and nat.lib.gacq_stap_workspace(ctypes.addressof(c)) == BAD_ARG, bad
    # M T = 57 is refused, 56 accepted
    c = _cfg(M=3, taps=15)
    c.taps = 19
    assert _check(c) == BAD_ARG and "taps" in _error()
    assert _check(_cfg(M=8, taps=7)) == 0 and _check(_cfg(M=3, taps=15)) == 0 and _check(_cfg(M=8, taps=9)) == BAD_ARG and "at most 56" in _error()
    for ok in (dict(M=1), dict(M=1, taps=1), dict(M=8, taps=1), dict(M=1, taps=15), dict(block=64), dict(block=32768), dict(window=1),
               dict(window=64, block=64), dict(load_shift=0), dict(load_shift=40)):
        assert _check(_cfg(**ok)) == 0, ok
    c = _cfg()
    assert nat.lib.gacq_stap_tile(ctypes.addressof(c)) == C.TILE and nat.lib.gacq_stap_tile(None) == BAD_ARG
    # the pinned order: antennas, taps, their product, block, window, load_shift, constraint, gain, indices, support
    steps = [("antennas", dict(antennas=9)), ("taps", dict(taps=4)), ("at most", dict(antennas=8, taps=9)), ("block length", dict(block=100)),
             ("the window", dict(window=0)), ("load_shift", dict(load_shift=41)), ("constraint", dict(zero=1))]
    for k, (word, own) in enumerate(steps):
        c = _cfg()
        for change in [later for _, later in steps[k + 1:]] + [own]:                            # everything after it is wrong as well
            for key, v in change.items():
                if key == "zero":
                    c.c[0] = 0.0
                else:
                    setattr(c, key, v)
        assert _check(c, gain=0.0, in_first=-1, n_out=1 << 30) == BAD_ARG and word in _error(), (word, _error())
    assert _check(_cfg(), gain=0.0, in_first=-1) == BAD_ARG and "the gain" in _error()
    assert _check(_cfg(), in_first=-1, n_out=1 << 30) == BAD_ARG and "need 0 <=" in _error()
    # the constraint: finite, not all zero; entries past M are not looked at
    for z in ([0, 0, 0, 0], [1, float("nan"), 0, 0], [1, 0, float("inf"), 0], [1, 0, 0, complex(0, float("inf"))]):
        assert _check(_cfg(constraint=z)) == BAD_ARG, z
    c = _cfg(M=2, constraint=[0, 1j])
    c.c[4] = float("nan")
    assert _check(c) == 0
    for g in (0.0, -1.0, float("nan"), float("inf"), 1e-50, 1e39):
        assert _check(_cfg(), gain=g) == BAD_ARG and _error().startswith("gacq_stap: the gain"), g
    big = (1 << 48) + 1
    for kw in (dict(in_first=-1), dict(in_count=-1), dict(out_first=-1), dict(n_out=-1), dict(in_first=big), dict(in_count=big), dict(out_first=big),
               dict(n_out=big)):
        assert _check(_cfg(), **kw) == BAD_ARG and _error().startswith("gacq_stap: need 0 <=") and "2^48" in _error(), kw
    assert _check(_cfg(), (1 << 48) - 8 * 4096 - 2, 1 << 20, 1 << 48, 100) == 0                    # the last index the check accepts


def test_the_support_rule_one_sample_short_at_either_end():
    c = _cfg(M=2, taps=7, block=64, window=3)                                                   # t_c = 3
    assert _check(c, 0, 195, 0, 192) == 0 and _check(c, 0, 194, 0, 1) == SHORT_INPUT            # the warm-up needs W whole blocks and t_c more
    assert _check(c, 0, 200, 0, 197) == 0 and _check(c, 0, 200, 0, 198) == SHORT_INPUT          # a recording of n supports outputs 0 .. n - 1 - t_c
    assert _check(c, 61, 1000, 256, 10) == 0 and _check(c, 62, 1000, 256, 10) == SHORT_INPUT    # block 4 needs blocks 1 .. 3 and t_c before them
    assert _check(c, 61, 1000, 255, 10) == SHORT_INPUT                                          # block 3 needs block 0
    assert _check(c, 61, 208, 256, 10) == 0 and _check(c, 61, 207, 256, 10) == SHORT_INPUT      # outputs 256 .. 265 need samples up to 268
    assert "need input samples 61 .. 268, present are 61 .. 267" in _error() and _error().startswith("gacq_stap: outputs 256 .. 265 ")
    assert _check(c, 5, 0, 7, 0) == 0                                                           # n_out = 0 needs nothing
    one = _cfg(M=2, taps=1, block=64, window=3)                                                 # t_c = 0: gacq_null's rule
    assert _check(one, 0, 192, 0, 192) == 0 and _check(one, 0, 191, 0, 1) == SHORT_INPUT and _check(one, 64, 202, 256, 10) == 0


def test_block_window_and_tap_algebra():
    assert [stap.centre(T) for T in (1, 3, 15)] == [0, 1, 7]
    assert stap.out_end(64, 3, 194, 7) == 0 and stap.out_end(64, 3, 195, 7) == 192 and stap.out_end(64, 3, 1000, 7) == 997
    assert stap.out_end(64, 3, 191, 1) == 0 and stap.out_end(64, 3, 192, 1) == 192
    assert [stap.first_needed(64, 3, o, 7) for o in (0, 191, 192, 255, 256, 320)] == [0, 0, 0, 0, 61, 125]
    assert [stap.owned_blocks(64, a, n) for a, n in ((0, 64), (0, 65), (1, 63), (1, 64), (64, 1), (63, 0))] == [1, 2, 0, 1, 1, 0]
    assert stap.auto_window(4096, 8, 5) == 65538 and stap.auto_window(32768, 8, 15) == 262151
    for name in ("m3-t3-b128-w3", "m1-t15-b64-w1"):
        M, T, Lb, W = C.CASES[name][:4]
        lo, hi = O.needed(Lb, W, T, 5 * Lb + 1, 7)
        assert lo == stap.first_needed(Lb, W, 5 * Lb + 1, T) == (5 - W) * Lb - O.centre(T) and hi == 5 * Lb + 8 + O.centre(T)
        n_in = len(C.data(name)[0]) // 2
        assert stap.out_end(Lb, W, n_in, T) == O.supported(Lb, W, T, 0, n_in) == C.outputs(name)
    c = stap.make_cfg(3, 7, 128, 2, 9, [1, 2j, -1 - 1j])
    assert (c.antennas, c.taps, c.block, c.window, c.load_shift, list(c.c)[:7]) == (3, 7, 128, 2, 9, [1.0, 0.0, 0.0, 2.0, -1.0, -1.0, 0.0])
    assert ctypes.sizeof(c) == 24 + 128
    with pytest.raises(ValueError):
        stap.make_cfg(3, constraint=[1, 0])
    # the workspace: at most 64 MiB, the whole 2^14 blocks while the weights are few
    def ws(**kw):
        c = _cfg(**kw)
        return nat.lib.gacq_stap_workspace(ctypes.addressof(c))

    assert ws(M=8, taps=7, window=64) <= 1 << 26 and ws(M=8, taps=7, window=1) <= 1 << 26 and ws(M=8, taps=7, window=1) > (1 << 26) - 56 * 57 * 8
    assert ws(M=8, taps=1, window=8) == ((1 << 14) + 8) * 64 * 8 + (1 << 14) * 8 * 8


def test_the_parser_and_the_report():
    a = stap.parse(["--out", "o.bin", "a"])
    assert (a.taps, a.block, a.window, a.load_shift, a.constraint, a.gain, a.target_rms, a.complex64, a.weights_trace, a.inputs) == \
        (5, 4096, 8, 10, None, None, 32.0, False, None, ["a"])
    a = stap.parse(["--taps", "9", "--block", "128", "--window", "3", "--load-shift", "8", "--constraint", "1,0", "0.5,-0.5", "--gain", "2.5", "--complex64",
                    "--weights-trace", "w.bin", "--out", "-", "a", "-"])
    assert (a.taps, a.block, a.window, a.load_shift, a.constraint, a.gain, a.complex64, a.weights_trace, a.out, a.inputs) == \
        (9, 128, 3, 8, [1 + 0j, 0.5 - 0.5j], 2.5, True, "w.bin", "-", ["a", "-"])
    assert stap.parse(["--taps", "7", "--out", "o"] + ["a"] * 8).taps == 7 and stap.parse(["--taps", "1", "--out", "o", "a", "b"]).taps == 1
    for bad in (["--out", "o"], ["--out", "o"] + ["a"] * 9, ["--taps", "4", "--out", "o", "a"], ["--taps", "17", "--out", "o", "a"],
                ["--taps", "9", "--out", "o"] + ["a"] * 7, ["--block", "100", "--out", "o", "a", "b"], ["--window", "0", "--out", "o", "a", "b"],
                ["--load-shift", "41", "--out", "o", "a", "b"], ["--constraint", "1,0", "--out", "o", "a", "b"], ["--constraint", "0,0", "0,0", "--out", "o", "a", "b"],
                ["--constraint", "1", "2", "--out", "o", "a", "b"], ["--gain", "0", "--out", "o", "a", "b"], ["--gain", "1", "--target-rms", "2", "--out", "o", "a", "b"],
                ["--out", "o", "-", "-"], ["a", "b"]):
        with pytest.raises(SystemExit):
            stap.parse(bad)
    assert stap.report_line(4, 5, 4096, 8, 0.25, 3, 1000) == "antennas 4 taps 5 block 4096 window 8 gain 0.25 clipped 3 samples 1000"
