"""CPU: the numpy definition of spatial nulling (tests/nulling_oracle.py) read against include/gacq.h -- its solve against numpy's, the
reference antenna's unit weight, the independence of cuts, the rounding-tie margin of every shared case -- and, of the library, what
needs no device: the refusals of gacq_null_check through the raw ABI, the host helpers, the parser and the report."""
import ctypes
import io

import numpy as np
import pytest

import nulling_cases as C
import nulling_oracle as O
from gnss_dsp_tools_amd import _native as nat
from gnss_dsp_tools_amd import nulling

BAD_ARG, SHORT_INPUT = -1, -6


@pytest.mark.parametrize("M", range(2, 9))
def test_the_oracles_solve_agrees_with_numpy(M):
    xs = C.recording(M, 5 * 256, 40 + M)
    Cre, Cim = O.block_cov(xs, 256, 0, 5)
    c = O.default_constraint(M) if M % 2 else np.exp(2j * np.pi * 0.17 * np.arange(M) ** 2)
    Are, Aim = O.loaded(Cre, Cim, 10)
    ur, ui = O.solve(Are, Aim, c)
    for b in range(5):
        want = np.linalg.solve(Are[b] + 1j * Aim[b], c)
        got = ur[b] + 1j * ui[b]
        assert np.max(np.abs(got - want)) <= 1e-9 * np.max(np.abs(want)), (M, b)
    # the covariance itself: Hermitian, a real diagonal, and the plain complex sum
    z = [O.split(x)[0][:256] + 1j * O.split(x)[1][:256] for x in xs]
    for p in range(M):
        assert Cim[0, p, p] == 0
        for q in range(M):
            s = np.sum(z[p] * np.conj(z[q]))
            assert (Cre[0, p, q], Cim[0, p, q]) == (round(s.real), round(s.imag)) and (Cre[0, q, p], Cim[0, q, p]) == (Cre[0, p, q], -Cim[0, p, q])


def test_the_reference_antenna_passes_with_unit_gain_and_the_constraint_holds():
    for name in C.CASES:
        r = C.reference(name)
        w = r["wq_all"].astype(np.float64) / O.WQ
        if C.constraint(name) is None:
            assert np.all(r["wq_all"][:, 0, 0] == O.WQ) and np.all(r["wq_all"][:, 0, 1] == 0), name
        else:
            z = w[:, :, 0] + 1j * w[:, :, 1]
            assert np.max(np.abs(z @ np.conj(C.STEER) - 1.0)) < 1e-3, name                     # c^H w = 1 up to the quantisation


def test_the_weights_quieten_a_jammed_recording():
    name = "m5-b4096-w3"
    M, Lb, W = C.CASES[name][:3]
    r = C.reference(name, True)
    i, q = O.split(C.data(name)[0])
    p_in = np.mean(i.astype(np.float64) ** 2 + q.astype(np.float64) ** 2)
    assert np.mean(np.abs(r["out"][(W + 1) * Lb:]) ** 2) < 0.2 * p_in


def test_every_case_keeps_its_distance_from_a_rounding_tie():
    m = C.check_margins()
    assert len(m) == len(C.CASES) == 40 and min(m.values()) >= C.MARGIN, m


@pytest.mark.parametrize("name", ["m3-b128-w1", "m8-b128-w3", "m2-b64-w3"])
@pytest.mark.parametrize("complex64", [False, True], ids=["int8", "complex64"])
def test_the_oracle_on_cuts_is_the_oracle_on_the_whole(name, complex64):
    M, Lb, W = C.CASES[name][:3]
    xs = C.data(name)
    N = len(xs[0]) // 2
    whole = C.reference(name, complex64, 0.75)
    pts = [0] + [p for p in (W * Lb + 3, (W + 1) * Lb, (W + 1) * Lb + 8, N - 11)] + [N]
    outs, clipped, owned, wq = [], 0, 0, []
    for a, b in zip(pts, pts[1:]):
        lo, hi = O.needed(Lb, W, a, b - a)
        r = O.run([x[2 * lo:2 * hi] for x in xs], lo, a, b - a, Lb, W, 10, C.constraint(name), 0.75, complex64)
        outs.append(r["out"])
        clipped, owned = clipped + r["clipped"], owned + r["owned"]
        wq.append(r["wq"])
    assert np.array_equal(np.concatenate(outs), whole["out"]) and (clipped, owned) == (whole["clipped"], whole["owned"])
    assert np.array_equal(np.concatenate(wq), whole["wq"]) and owned == -(-N // Lb)
    # the warm-up: blocks 0 .. W share one weight vector
    assert all(np.array_equal(whole["wq"][b], whole["wq"][0]) for b in range(W + 1)) and not np.array_equal(whole["wq"][W + 1], whole["wq"][0])


def _cfg(**kw):
    d = dict(M=4, block=4096, window=8, load_shift=10, constraint=None)
    d.update(kw)
    return nulling.make_cfg(d["M"], d["block"], d["window"], d["load_shift"], d["constraint"])


def _check(cfg, in_first=0, in_count=1 << 20, out_first=0, n_out=1 << 20, gain=1.0, cplx=0):
    return nat.lib.gacq_null_check(ctypes.addressof(cfg) if cfg is not None else None, in_first, in_count, out_first, n_out, gain, cplx)


def test_gacq_null_check_refuses_through_the_raw_abi():
    assert _check(_cfg()) == 0 and _check(_cfg(), cplx=1) == 0
    assert _check(None) == BAD_ARG
    for bad in (dict(M=1), dict(M=9), dict(block=0), dict(block=32), dict(block=96), dict(block=65536), dict(block=32768 + 64), dict(window=0),
                dict(window=65), dict(load_shift=-1), dict(load_shift=41)):
        assert _check(_cfg(**bad)) == BAD_ARG, bad
        assert nat.lib.gacq_last_error(None).startswith(b"gacq_null: "), bad                    # every message names its own tool
        assert nat.lib.gacq_null_tile(ctypes.addressof(_cfg(**bad))) == BAD_ARG, bad
    for ok in (dict(M=2), dict(M=8), dict(block=64), dict(block=32768), dict(window=1), dict(window=64, block=64), dict(load_shift=0), dict(load_shift=40)):
        assert _check(_cfg(**ok)) == 0, ok
    assert nat.lib.gacq_null_tile(ctypes.addressof(_cfg())) == C.TILE and nat.lib.gacq_null_tile(None) == BAD_ARG
    # the constraint: finite, not all zero; entries past M are not looked at
    for z in ([0, 0, 0, 0], [1, float("nan"), 0, 0], [1, 0, float("inf"), 0], [1, 0, 0, complex(0, float("inf"))]):
        assert _check(_cfg(constraint=z)) == BAD_ARG, z
    c = _cfg(M=2, constraint=[0, 1j])
    c.c[4] = float("nan")
    assert _check(c) == 0
    # the gain: finite and positive, as a double and as a float
    for g in (0.0, -1.0, float("nan"), float("inf"), 1e-50, 1e39):
        assert _check(_cfg(), gain=g) == BAD_ARG and nat.lib.gacq_last_error(None).startswith(b"gacq_null: the gain"), g
    # indices and counts
    big = (1 << 48) + 1
    for kw in (dict(in_first=-1), dict(in_count=-1), dict(out_first=-1), dict(n_out=-1), dict(in_first=big), dict(in_count=big), dict(out_first=big),
               dict(n_out=big)):
        assert _check(_cfg(), **kw) == BAD_ARG and nat.lib.gacq_last_error(None).startswith(b"gacq_null: need 0 <="), kw
    assert b"2^48" in nat.lib.gacq_last_error(None)
    # ranges: output j in block b needs j and max(b - W, 0) Lb .. max(b, W) Lb - 1
    c = _cfg(block=64, window=3)
    assert _check(c, 0, 192, 0, 192) == 0 and _check(c, 0, 191, 0, 1) == SHORT_INPUT            # the warm-up needs W whole blocks
    assert _check(c, 0, 200, 0, 200) == 0 and _check(c, 0, 200, 0, 201) == SHORT_INPUT          # the last partial block is produced
    assert _check(c, 64, 1000, 256, 10) == 0 and _check(c, 65, 1000, 256, 10) == SHORT_INPUT    # block 4 needs blocks 1 .. 3
    assert _check(c, 64, 1000, 255, 10) == SHORT_INPUT                                          # block 3 needs block 0
    assert _check(c, 64, 202, 256, 10) == 0 and _check(c, 64, 201, 256, 10) == SHORT_INPUT
    assert b"need input samples" in nat.lib.gacq_last_error(None) and nat.lib.gacq_last_error(None).startswith(b"gacq_null: outputs 256 .. 265 ")
    assert _check(c, 5, 0, 7, 0) == 0                                                           # n_out = 0 needs nothing


def test_host_helpers():
    assert nulling.out_end(64, 3, 191) == 0 and nulling.out_end(64, 3, 192) == 192 and nulling.out_end(64, 3, 1000) == 1000
    assert [nulling.first_needed(64, 3, o) for o in (0, 191, 192, 255, 256, 320)] == [0, 0, 0, 0, 64, 128]
    assert [nulling.owned_blocks(64, a, n) for a, n in ((0, 64), (0, 65), (1, 63), (1, 64), (64, 1), (63, 0))] == [1, 2, 0, 1, 1, 0]
    assert nulling.auto_window(4096, 8) == 65536 and nulling.auto_window(32768, 8) == 262144
    for name in ("m3-b128-w3", "m2-b64-w1"):
        M, Lb, W = C.CASES[name][:3]
        lo, hi = O.needed(Lb, W, 5 * Lb + 1, 7)
        assert lo == nulling.first_needed(Lb, W, 5 * Lb + 1) == (5 - W) * Lb and hi == 5 * Lb + 8
    c = nulling.make_cfg(3, 128, 2, 7, [1, 2j, -1 - 1j])
    assert (c.antennas, c.block, c.window, c.load_shift, list(c.c)[:7]) == (3, 128, 2, 7, [1.0, 0.0, 0.0, 2.0, -1.0, -1.0, 0.0])
    with pytest.raises(ValueError):
        nulling.make_cfg(3, constraint=[1, 0])
    # lockstep reading: pieces of one length, cut at the shortest file
    a, b = bytes(range(100)), bytes(range(100, 190))
    got = list(nulling.lockstep([io.BytesIO(a), io.BytesIO(b)], 32))
    assert [len(p[0]) for p in got] == [32, 32, 26] and all(len(p[0]) == len(p[1]) for p in got)
    assert b"".join(p[1].tobytes() for p in got) == b and b"".join(p[0].tobytes() for p in got) == a[:90]
    assert list(nulling.lockstep([io.BytesIO(b""), io.BytesIO(b)], 32)) == []


def test_the_parser_and_the_report():
    a = nulling.parse(["--out", "o.bin", "a", "b"])
    assert (a.block, a.window, a.load_shift, a.constraint, a.gain, a.target_rms, a.complex64, a.weights_trace, a.inputs) == \
        (4096, 8, 10, None, None, 32.0, False, None, ["a", "b"])
    a = nulling.parse(["--block", "128", "--window", "3", "--load-shift", "8", "--constraint", "1,0", "0.5,-0.5", "--gain", "2.5", "--complex64",
                       "--weights-trace", "w.bin", "--out", "-", "a", "b"])
    assert (a.block, a.window, a.load_shift, a.constraint, a.gain, a.complex64, a.weights_trace, a.out) == \
        (128, 3, 8, [1 + 0j, 0.5 - 0.5j], 2.5, True, "w.bin", "-")
    for bad in (["--out", "o", "a"], ["--out", "o"] + ["a"] * 9, ["--block", "100", "--out", "o", "a", "b"], ["--window", "0", "--out", "o", "a", "b"],
                ["--load-shift", "41", "--out", "o", "a", "b"], ["--constraint", "1,0", "--out", "o", "a", "b"], ["--constraint", "0,0", "0,0", "--out", "o", "a", "b"],
                ["--constraint", "1", "2", "--out", "o", "a", "b"], ["--gain", "0", "--out", "o", "a", "b"], ["--gain", "1", "--target-rms", "2", "--out", "o", "a", "b"],
                ["a", "b"]):
        with pytest.raises(SystemExit):
            nulling.parse(bad)
    assert nulling.report_line(4, 4096, 8, 0.25, 3, 1000) == "antennas 4 block 4096 window 8 gain 0.25 clipped 3 samples 1000"
