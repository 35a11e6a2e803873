"""CPU: what of the per-satellite beams (gnss_dsp_tools_amd/beams.py, gacq_beams_*) needs no device -- the rounding-tie margin of every
beam of every shared case, the refusals and the accepted edges of gacq_beams_check through the raw ABI, gacq_beams_tile, the parser,
the report lines, the host helpers, and the chosen row of the end-to-end table through the CPU chain."""
import ctypes

import numpy as np
import pytest

import beams_cases as B
import nulling_oracle as O
from gnss_dsp_tools_amd import _native as nat
from gnss_dsp_tools_amd import beams

BAD_ARG, SHORT_INPUT = -1, -6


def test_every_beam_of_every_case_keeps_its_distance_from_a_rounding_tie():
    m = B.check_margins()
    assert len(B.CASES) == 34 and len(m) == sum(c[1] for c in B.CASES.values()) == 246
    assert min(m.values()) == B.SMALLEST_MARGIN >= B.MARGIN and B.REJECTED_SEEDS == ()
    # the grid keeps every value of every axis and every (M, K) pair
    grid = [c for c in B.CASES.values() if c[5] == "noise"]
    assert len(grid) == 30 and {(c[0], c[1]) for c in grid} == {(M, K) for M in (2, 3, 8) for K in (1, 2, 8, 9, 16)}
    assert {c[2] for c in grid} == {64, 128, 4096} and {c[3] for c in grid} == {1, 3}
    # the cases are worth their gains: the int8 outputs clip, each beam under a gain of its own
    for name in ("m2-k16-b64-w3", "m8-k9-b4096-w1", "long-m3-k9-b192-w2"):
        assert all(B.reference(name, k)["clipped"] > 0 for k in range(B.CASES[name][1])), name
        assert len(set(B.gains(name))) == B.CASES[name][1]
    cs = B.constraints("twin-m3-k3-b64-w3")
    assert np.array_equal(cs[1], cs[2]) and not np.array_equal(cs[0], cs[1])
    assert np.array_equal(B.reference("twin-m3-k3-b64-w3", 1, True)["out"], B.reference("twin-m3-k3-b64-w3", 2, True)["out"])
    for name in B.CASES:
        mod = np.abs(B.constraints(name)[2:])
        assert mod.size == 0 or (mod.min() >= 0.3 and mod.max() <= 1.5), name


def _cfg(**kw):
    d = dict(M=4, K=3, block=4096, window=8, load_shift=10, constraints=None)
    d.update(kw)
    cs = d["constraints"] if d["constraints"] is not None else [None] * d["K"]
    cfg = beams.make_cfg(d["M"], cs, d["block"], d["window"], d["load_shift"])
    cfg.beams = d["K"]                                                                          # also values make_cfg would not take
    return cfg


def _check(cfg, in_first=0, in_count=1 << 20, out_first=0, n_out=1 << 20, gains=None, cplx=0):
    g = (ctypes.c_double * 16)(*([1.0] * 16 if gains is None else list(gains) + [float("nan")] * (16 - len(gains))))
    return nat.lib.gacq_beams_check(ctypes.addressof(cfg) if cfg is not None else None, in_first, in_count, out_first, n_out,
                                    ctypes.cast(g, ctypes.c_void_p), cplx)


def test_gacq_beams_check_refuses_through_the_raw_abi():
    assert _check(_cfg()) == 0 and _check(_cfg(), cplx=1) == 0
    assert _check(None) == BAD_ARG
    # everything gacq_null refuses, and the beams
    for bad in (dict(M=1), dict(M=9), dict(block=0), dict(block=32), dict(block=96), dict(block=65536), dict(block=32768 + 64), dict(window=0),
                dict(window=65), dict(load_shift=-1), dict(load_shift=41)):
        assert _check(_cfg(**bad)) == BAD_ARG, bad
        assert nat.lib.gacq_last_error(None).startswith(b"gacq_beams: "), bad                   # every message names its own tool
        assert nat.lib.gacq_beams_tile(ctypes.addressof(_cfg(**bad))) == BAD_ARG, bad
    for K in (0, -1, 17):
        c = _cfg(K=1)
        c.beams = K
        assert _check(c) == BAD_ARG and b"beams: need 1..16" in nat.lib.gacq_last_error(None), K
        assert nat.lib.gacq_beams_tile(ctypes.addressof(c)) == BAD_ARG
    for ok in (dict(M=2), dict(M=8), dict(K=1), dict(K=16), dict(M=8, K=16), dict(M=2, K=16), dict(block=64), dict(block=32768), dict(window=1),
               dict(window=64, block=64), dict(load_shift=0), dict(load_shift=40)):
        assert _check(_cfg(**ok)) == 0, ok
    assert nat.lib.gacq_beams_tile(ctypes.addressof(_cfg())) == B.TILE and nat.lib.gacq_beams_tile(None) == BAD_ARG
    assert nat.lib.gacq_beams_tile(ctypes.addressof(_cfg(K=16, M=8))) == B.TILE
    # the constraints: every one finite and not all zero, and the message names the beam; entries past M and rows past K are not looked at
    for k in range(3):
        for z in ([0, 0, 0, 0], [1, float("nan"), 0, 0], [1, 0, float("inf"), 0], [1, 0, 0, complex(0, float("inf"))]):
            cs = [None, [1, 1j, 0, 0], None]
            cs[k] = z
            assert _check(_cfg(constraints=cs)) == BAD_ARG and (b"beam %d" % k) in nat.lib.gacq_last_error(None), (k, z)
    c = _cfg(M=2, K=2)
    c.c[0][4] = c.c[1][15] = float("nan")
    for i in range(16):
        c.c[2][i] = 0.0 if i % 2 else float("inf")
    assert _check(c) == 0
    # the gains: each finite and positive, as a double and as a float; those past K are not looked at; NULL is refused
    assert _check(_cfg(), gains=[1.0, 2.0, 0.5]) == 0
    for k in range(3):
        for g in (0.0, -1.0, float("nan"), float("inf"), 1e-50, 1e39):
            gs = [1.0, 2.0, 0.5]
            gs[k] = g
            assert _check(_cfg(), gains=gs) == BAD_ARG and nat.lib.gacq_last_error(None).startswith(b"gacq_beams: the gain of beam %d" % k), (k, g)
    assert nat.lib.gacq_beams_check(ctypes.addressof(_cfg()), 0, 1 << 20, 0, 1 << 20, None, 0) == BAD_ARG
    # indices and counts
    big = (1 << 48) + 1
    for kw in (dict(in_first=-1), dict(in_count=-1), dict(out_first=-1), dict(n_out=-1), dict(in_first=big), dict(in_count=big), dict(out_first=big),
               dict(n_out=big)):
        assert _check(_cfg(), **kw) == BAD_ARG and nat.lib.gacq_last_error(None).startswith(b"gacq_beams: need 0 <="), kw
    # ranges: nulling's support rule, one sample short at either end
    for K in (1, 16):
        c = _cfg(block=64, window=3, K=K)
        assert _check(c, 0, 192, 0, 192) == 0 and _check(c, 0, 191, 0, 1) == SHORT_INPUT        # the warm-up needs W whole blocks
        assert _check(c, 0, 200, 0, 200) == 0 and _check(c, 0, 200, 0, 201) == SHORT_INPUT      # the last partial block is produced
        assert _check(c, 64, 1000, 256, 10) == 0 and _check(c, 65, 1000, 256, 10) == SHORT_INPUT    # block 4 needs blocks 1 .. 3
        assert _check(c, 64, 1000, 255, 10) == SHORT_INPUT                                      # block 3 needs block 0
        assert _check(c, 64, 202, 256, 10) == 0 and _check(c, 64, 201, 256, 10) == SHORT_INPUT
        assert nat.lib.gacq_last_error(None).startswith(b"gacq_beams: outputs 256 .. 265 ")
        assert _check(c, 5, 0, 7, 0) == 0                                                       # n_out = 0 needs nothing


def test_host_helpers():
    c = beams.make_cfg(3, [None, [1, 2j, -1 - 1j]], 128, 2, 7)
    assert (c.antennas, c.beams, c.block, c.window, c.load_shift) == (3, 2, 128, 2, 7)
    assert list(c.c[0])[:7] == [1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0] and list(c.c[1])[:7] == [1.0, 0.0, 0.0, 2.0, -1.0, -1.0, 0.0]
    assert ctypes.sizeof(c) == 5 * 4 + 4 + 16 * 16 * 8                                          # gacq_beams_cfg: five ints, padding, the table
    for bad in ([], [None] * 17, [[1, 0]], [None, [1, 0, 0, 0]]):
        with pytest.raises(ValueError):
            beams.make_cfg(3, bad)
    o = ([None, None], 64, 3, 10)
    T = beams.TOOL
    assert (T.window(o), T.out_end(o, 191), T.out_end(o, 192), T.out_end(o, 1000)) == (3, 0, 192, 1000)
    assert [T.first_needed(o, x) for x in (0, 191, 192, 255, 256, 320)] == [0, 0, 0, 0, 64, 128]
    assert T.auto_window(o) == 65536 and T.auto_window(([None], 32768, 8, 10)) == 262144
    assert beams._gains([None] * 3, 2.0) == [2.0, 2.0, 2.0] and beams._gains([None] * 2, [1, 2.5]) == [1.0, 2.5]
    # beam k of a case is the nulling oracle under c_k: the constraint holds on the quantised weights
    name = "m3-k9-b128-w1"
    for k in (0, 1, 8):
        w = B.reference(name, k)["wq_all"].astype(np.float64) / O.WQ
        z = w[:, :, 0] + 1j * w[:, :, 1]
        assert np.max(np.abs(z @ np.conj(B.constraints(name)[k]) - 1.0)) < 2e-3, (name, k)


def test_the_parser_and_the_report():
    a = beams.parse(["--antenna", "a", "--antenna", "b", "--beam", "o0", "1,0", "0,0"])
    assert (a.block, a.window, a.load_shift, a.gain, a.target_rms, a.complex64, a.weights_trace, a.antenna, a.outputs) == \
        (4096, 8, 10, None, 32.0, False, None, ["a", "b"], ["o0"])
    assert np.array_equal(a.constraints[0], [1, 0])
    a = beams.parse(["--block", "128", "--window", "3", "--load-shift", "8", "--gain", "2.5", "--complex64", "--weights-trace", "w.bin",
                     "--antenna", "a", "--beam", "o0", "1,0", "-0.5,0.25", "-1e-3,-2", "--antenna", "b", "--antenna", "c", "--beam", "o1", "0,1", ".5,-.5", "-.25,0"])
    assert (a.block, a.window, a.load_shift, a.gain, a.complex64, a.weights_trace, a.antenna, a.outputs) == \
        (128, 3, 8, 2.5, True, "w.bin", ["a", "b", "c"], ["o0", "o1"])
    assert np.array_equal(a.constraints, [[1, -0.5 + 0.25j, -1e-3 - 2j], [1j, 0.5 - 0.5j, -0.25]])
    # what arrayprompt prints after `steering` comes back exactly
    z = np.array([1.0, -0.1234567890123456 + 0.3j, 1e-5 - 7.25j])
    text = ["%r,%r" % (float(v.real), float(v.imag)) for v in z]
    assert np.array_equal(beams.parse(["--antenna", "a", "--antenna", "b", "--antenna", "c", "--beam", "o"] + text).constraints[0], z)
    two = ["--antenna", "a", "--antenna", "b"]
    for bad in (two + ["--beam", "o", "1,0"],                                                   # too few entries
                two + ["--beam", "o", "1,0", "0,0", "0,0"],                                     # too many
                two + ["--beam", "o"],                                                          # none
                two + ["--beam", "o", "0,0", "0,0"],                                            # a zero vector
                two + ["--beam", "o", "1,0", "0,0", "--beam", "p", "0,0", "0,-0"],
                two + ["--beam", "o", "1,0", "nan,0"], two + ["--beam", "o", "1,0", "1"], two + ["--beam", "o", "1,0", "x,y"],
                two + ["--beam", "o", "1,0", "0,0"] * 17,                                       # more than 16 beams
                two,                                                                            # no beam
                ["--antenna", "a", "--beam", "o", "1,0"],                                       # fewer than 2 antennas
                ["--antenna", "a"] * 9 + ["--beam", "o"] + ["1,0"] * 9,
                two + ["--block", "100", "--beam", "o", "1,0", "0,0"], two + ["--window", "0", "--beam", "o", "1,0", "0,0"],
                two + ["--load-shift", "41", "--beam", "o", "1,0", "0,0"], two + ["--gain", "0", "--beam", "o", "1,0", "0,0"],
                two + ["--gain", "1", "--target-rms", "2", "--beam", "o", "1,0", "0,0"]):
        with pytest.raises(SystemExit):
            beams.parse(bad)
    assert len(beams.parse(two + ["--beam", "o", "1,0", "0,0"] * 16).outputs) == 16
    assert beams.report_lines(4, 4096, 8, [0.25, 2.0], [3, 0], 1000) == \
        ["antennas 4 beams 2 block 4096 window 8 samples 1000", "beam 0 gain 0.25 clipped 3", "beam 1 gain 2.0 clipped 0"]


def test_the_end_to_end_table_on_the_cpu():
    """the chosen row of beams_cases.E2E: on the power-inversion output the search misses PRN 5, every beam finds its own PRN in the true
    cell with a larger metric and a quarter of the output power"""
    rows, sats, w0 = B.e2e_cpu_rows()
    for s in sats:
        pi, beam = rows[s.item]["pi"], rows[s.item]["beam"]
        print("prn %d: power inversion %.2f %.2f %.0f %.1f   beam %.2f %.2f %.0f %.1f" % ((s.item,) + pi + beam))
        assert B.e2e_hit(beam, s, w0) and beam[0] > pi[0] and beam[0] > 3.0 and beam[3] < 0.5 * pi[3], (s.item, pi, beam)
        assert B.e2e_hit(pi, s, w0) == (s.item not in B.E2E["missed"]), (s.item, pi)
