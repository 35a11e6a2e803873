"""CPU: the numpy definition of the bearing scan (tests/bearing_oracle.py) read against include/gacq.h -- its q against numpy's inverse,
its peaks against a brute-force loop, the ties of the two-element array, the absolute-index rule of --every on cut streams -- and, of
the library, what needs no device: the refusals of gacq_bearing_check through the raw ABI, the grid, the tables, the parser and the
summary line."""
import ctypes

import numpy as np
import pytest

import bearing_cases as C
import bearing_oracle as B
import nulling_cases as NC
import nulling_oracle as N
from gnss_dsp_tools_amd import _native as nat
from gnss_dsp_tools_amd import bearing, scene

BAD_ARG = -1


@pytest.mark.parametrize("M", range(2, 9))
def test_the_oracles_q_agrees_with_numpys_inverse(M):
    a, u = C.table(M, 257)
    Rre, Rim = C.covariances(M)
    Are, Aim = N.loaded(Rre, Rim, C.SHIFT)
    q = B.q(Rre, Rim, C.SHIFT, a)
    assert q.shape == (C.N_BLOCKS, 257)
    for b in range(C.N_BLOCKS):
        want = np.real(np.einsum("gp,pq,gq->g", np.conj(a), np.linalg.inv(Are[b] + 1j * Aim[b]), a))
        assert np.max(np.abs(q[b] - want) / np.abs(want)) <= 1e-9, (M, b)
        assert np.all(q[b] > 0)


def _brute_peaks(q, u, K, cos_sep):
    """the peak rule of the header with Python floats, one cell at a time"""
    out = []
    left = [bool(np.isfinite(v) and v > 0.0) for v in q]
    for _ in range(K):
        best = None
        for g, v in enumerate(q):
            if left[g] and (best is None or float(v) < float(q[best])):
                best = g
        if best is None:
            out.append((-1, 0, float("inf")))
            continue
        out.append((best, 0, float(q[best])))
        for g in range(len(q)):
            d = (float(u[g][0]) * float(u[best][0]) + float(u[g][1]) * float(u[best][1])) + float(u[g][2]) * float(u[best][2])
            if d >= cos_sep:
                left[g] = False
    return out


@pytest.mark.parametrize("M,G,cos_sep", [(2, 257, C.COS_SEP), (8, 1368, C.COS_SEP), (3, 65, -1.0), (5, 257, 1.0), (3, 63, 0.0)])
def test_the_oracles_peaks_agree_with_a_brute_force_loop(M, G, cos_sep):
    a, u = C.table(M, G)
    rec, fl, q = B.run(*C.covariances(M), C.SHIFT, a, u, C.K, cos_sep)
    for i in range(C.N_BLOCKS):
        assert [tuple(r) for r in rec[i].tolist()] == _brute_peaks(q[i], u, C.K, cos_sep), (M, G, i)
        assert fl[i] == np.max(q[i])
    if cos_sep == -1.0:
        assert np.all(rec["cell"][:, 1:] == -1) and np.all(np.isinf(rec["q"][:, 1:])) and np.all(rec["cell"][:, 0] >= 0)


def test_ineligible_cells_the_floor_and_the_empty_record():
    a, u = C.table(3, 257)
    R = C.negative_pivot()
    rec, fl, q = B.run(R[..., 0], R[..., 1], C.SHIFT, a, u, C.K, C.COS_SEP)
    assert np.any(q <= 0) and np.any(q > 0) and fl[0] == np.max(q[q > 0]) and np.all(rec["q"] > 0)
    assert [tuple(r) for r in rec[0].tolist()] == _brute_peaks(q[0], u, C.K, C.COS_SEP)
    R = C.all_nan()
    rec, fl, q = B.run(R[..., 0], R[..., 1], 0, a, u, C.K, C.COS_SEP)
    assert np.all(np.isnan(q)) and np.isposinf(fl[0]) and np.all(rec["cell"] == -1) and np.all(np.isposinf(rec["q"])) and np.all(rec["zero"] == 0)
    Z = np.zeros((1, 3, 3), dtype=np.int64)
    rec, fl, q = B.run(Z, Z, C.SHIFT, a, u, C.K, C.COS_SEP)                      # A = I: q = |a|^2, close to 3 in every cell
    assert np.all(np.abs(q - 3.0) < 1e-12) and rec["cell"][0, 0] == int(np.argmin(q[0]))


def test_mirror_cells_of_the_two_element_array_tie_bit_for_bit():
    """the ties the device tests lean on: the smallest q of every block is shared by several cells, and rank 0 is the lowest of them"""
    cells = bearing.grid(5.0)
    a, u = bearing.tables(C.TIE_ELEMENTS, cells)
    rec, fl, q = B.run(*C.tie_covariances(), C.SHIFT, a, u, C.K, C.COS_SEP)
    for i in range(q.shape[0]):
        tied = np.flatnonzero(q[i] == rec["q"][i, 0])
        assert len(tied) >= 2 and rec["cell"][i, 0] == tied[0], (i, tied)


def _cfg(**kw):
    d = dict(antennas=4, load_shift=10, cells=1368, peaks=3, cos_sep=0.5)
    d.update(kw)
    return bearing.BearingCfg(**d)


def _check(cfg, n=5, stride=1):
    return nat.lib.gacq_bearing_check(ctypes.addressof(cfg) if cfg is not None else None, n, stride)


def test_gacq_bearing_check_refuses_through_the_raw_abi():
    assert _check(_cfg()) == 0
    assert _check(None) == BAD_ARG
    nan, inf = float("nan"), float("inf")
    for bad in (dict(antennas=1), dict(antennas=9), dict(load_shift=-1), dict(load_shift=41), dict(cells=0), dict(cells=32769), dict(peaks=0),
                dict(peaks=5), dict(cos_sep=nan), dict(cos_sep=inf), dict(cos_sep=-1.0000001), dict(cos_sep=1.0000001)):
        assert _check(_cfg(**bad)) == BAD_ARG, bad
        assert nat.lib.gacq_last_error(None).startswith(b"gacq_bearing: "), bad
    for ok in (dict(antennas=2), dict(antennas=8), dict(load_shift=0), dict(load_shift=40), dict(cells=1), dict(cells=32768), dict(peaks=1),
               dict(peaks=4), dict(cos_sep=-1.0), dict(cos_sep=1.0)):
        assert _check(_cfg(**ok)) == 0, ok
    big = 1 << 48
    for n, stride in ((-1, 1), (1, 0), (1, -1), (big + 1, 1), (1, big + 1), (2, big), (1 << 24, (1 << 24) + 1), (1 << 62, 4)):
        assert _check(_cfg(), n, stride) == BAD_ARG, (n, stride)
        assert b"2^48" in nat.lib.gacq_last_error(None)
    for n, stride in ((0, 1), (0, big), (big, 1), (1, big), (1 << 24, 1 << 24)):
        assert _check(_cfg(), n, stride) == 0, (n, stride)


def test_the_grid_and_the_tables():
    g = bearing.grid(5.0)
    assert g.shape == (1368, 2) and tuple(g[0]) == (0.0, 0.0) and tuple(g[1]) == (5.0, 0.0) and tuple(g[72]) == (0.0, 5.0) and tuple(g[-1]) == (355.0, 90.0)
    assert bearing.grid(2.0).shape == (8280, 2) and bearing.grid(5.0, 30.0).shape == (13 * 72, 2) and bearing.grid(5.0, 30.0)[0, 1] == 30.0
    assert bearing.grid(7.0).shape == (13 * 52, 2) and bearing.grid(7.0)[-1, 0] == 357.0 and bearing.grid(7.0)[-1, 1] == 84.0
    assert bearing.grid(360.0, 90.0).shape == (1, 2)
    for bad in ((0.0, 0.0), (-1.0, 0.0), (5.0, 91.0), (5.0, -1.0), (float("nan"), 0.0)):
        with pytest.raises(ValueError):
            bearing.grid(*bad)
    el = C.ring(5)
    a, u = bearing.tables(el, g)
    assert a.shape == (1368, 5) and a.dtype == np.complex128 and u.shape == (1368, 3) and u.dtype == np.float64
    k = 302
    assert tuple(g[k]) == (70.0, 20.0) and np.array_equal(a[k], scene.steering(el, 70.0, 20.0))
    az, e = np.deg2rad(70.0), np.deg2rad(20.0)
    assert np.array_equal(u[k], np.array([np.cos(e) * np.sin(az), np.cos(e) * np.cos(az), np.sin(e)]))
    assert np.array_equal(a[k], np.exp(2j * np.pi * (el @ u[k])))
    assert C.ring(8).shape == (8, 3) and np.allclose(np.linalg.norm(C.ring(8)[1:], axis=1), 0.5)


def test_the_parser():
    els = ["--element", "0,0,0", "--element", "-0.5,0,0"]
    a = bearing.parse(els + ["a", "b"])
    assert (a.step, a.el_min, a.peaks, a.sep, a.every, a.block, a.window, a.load_shift, a.out, a.trace, a.inputs) == \
        (5.0, 0.0, 3, 20.0, 1, 4096, 8, 10, None, None, ["a", "b"])
    assert a.element == [[0.0, 0.0, 0.0], [-0.5, 0.0, 0.0]] and a.cells.shape == (1368, 2)
    a = bearing.parse(els + ["--step", "2", "--el-min", "10", "--peaks", "4", "--sep", "15", "--every", "3", "--block", "128", "--window", "3",
                            "--load-shift", "8", "--out", "o.iq", "--trace", "t.txt", "a", "b"])
    assert (a.step, a.el_min, a.peaks, a.sep, a.every, a.block, a.window, a.load_shift, a.out, a.trace) == (2.0, 10.0, 4, 15.0, 3, 128, 3, 8, "o.iq", "t.txt")
    assert a.cells.shape == (41 * 180, 2)
    for bad in (["a", "b"], els + ["a"], els + ["a", "b", "c"], els + ["--peaks", "5", "a", "b"], els + ["--peaks", "0", "a", "b"],
                els + ["--every", "0", "a", "b"], els + ["--sep", "-1", "a", "b"], els + ["--block", "100", "a", "b"], els + ["--window", "0", "a", "b"],
                els + ["--load-shift", "41", "a", "b"], els + ["--step", "0", "a", "b"], els + ["--step", "0.5", "a", "b"], els + ["--el-min", "91", "a", "b"],
                els + ["--out", "-", "a", "b"], ["--element", "0,0", "--element", "1,0,0", "a", "b"]):
        with pytest.raises(SystemExit):
            bearing.parse(bad)


def test_the_report_the_trace_line_and_the_summary_rule():
    cells = bearing.grid(5.0)
    rec = np.zeros((5, 2), dtype=bearing.PEAK)
    rec["cell"][:, 0] = [302, 302, 770, 770, 14]                  # a tie between 302 and 770: the lowest cell
    rec["cell"][:, 1] = -1
    rec["q"][:, 0] = 0.001
    rec["q"][:, 1] = np.inf
    assert bearing.most_frequent(rec["cell"][:, 0]) == (302, 2) and bearing.most_frequent(rec["cell"][:, 1]) is None
    assert bearing.most_frequent([5, 9, 9, 5, 9]) == (9, 3)
    line = bearing.summary_line(8, 4096, 8, cells, rec)
    assert line == "antennas 8 block 4096 window 8 cells 1368 blocks 5 rank 0 az 70.00 el 20.00 count 2 rank 1 none"
    rep = bearing.report(cells, rec, np.full(5, 0.1))
    assert rep.shape == (5, 2, 3) and tuple(rep[0, 0]) == (70.0, 20.0, 20.0) and np.all(np.isnan(rep[:, 1]))
    assert bearing.trace_line(6, 4096, rep[0]) == "block 6 sample 24576 70.00 20.00 20.00 - - -"
    # records() reads the bytes of the device's [n][K][16] array
    raw = rec.view(np.uint8).reshape(5, 2, 16)
    assert np.array_equal(bearing.records(raw), rec)


@pytest.mark.parametrize("every", [1, 3, 4])
def test_every_counts_absolute_blocks_on_cut_streams(every):
    """the blocks a cut stream evaluates, call by call, are those of the one-call stream, and so are their records: with the oracle
    alone, on the window sums that nulling_oracle.run gives each call"""
    name = "long-m3-b128-w3"
    M, Lb, Wn = NC.CASES[name][:3]
    xs = NC.data(name)
    Nn = 40 * Lb + 17
    a, u = C.table(M, 65)
    whole_blocks = B.evaluated(Lb, 0, Nn, every)
    assert whole_blocks == list(range(0, 41, every))
    want = B.run(*B.window_sums(xs, Lb, Wn, whole_blocks), C.SHIFT, a, u, 2, C.COS_SEP)
    for pts in ([0, Nn], [0, Wn * Lb + 3, 7 * Lb, 7 * Lb + 1, 20 * Lb - 1, 33 * Lb + 64, Nn]):
        blocks, recs, floors = [], [], []
        for lo, hi in zip(pts, pts[1:]):
            in_lo, in_hi = N.needed(Lb, Wn, lo, hi - lo)
            r = N.run([x[2 * in_lo:2 * in_hi] for x in xs], in_lo, lo, hi - lo, Lb, Wn)
            first = -(-lo // Lb)
            off, bs = bearing.evaluated(first, r["cov"].shape[0], every)
            assert bs == B.evaluated(Lb, lo, hi - lo, every)
            if bs:
                cov = r["cov"][off::every]
                rec, fl, _ = B.run(cov[..., 0], cov[..., 1], C.SHIFT, a, u, 2, C.COS_SEP)
                recs.append(rec)
                floors.append(fl)
            blocks += bs
        assert blocks == whole_blocks
        assert np.concatenate(recs).tobytes() == want[0].tobytes() and np.concatenate(floors).tobytes() == want[1].tobytes()
