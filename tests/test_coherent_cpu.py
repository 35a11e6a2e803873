"""CPU: the host side of the coherent search (gnss_dsp_tools_amd/coherent.py) -- sign patterns, start tables, the built-in secondary
codes -- and the two facts the device path rests on, shown on the fp64 oracle: correlation commutes with the fold (linearity), and
the oracle chain (fp64 fold + oracle.acq_oracle) recovers a satellite that one code period does not show."""
import dataclasses
import json
import os
from fractions import Fraction

import numpy as np
import pytest

import coherent_cases as C
import coherent_oracle as O
from gnss_dsp_tools_amd import codes, coherent, signals
from oracle import acq_oracle, codes_oracle

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SEC = {1: None, 4: coherent.SECONDARY["galileo.e5bi"], 10: coherent.SECONDARY["gps.l5i"], 20: coherent.SECONDARY["beidou.b1i"],
       25: coherent.SECONDARY["galileo.e1c"]}
BUILTIN = {"xona-x1", "xona-x5p", "galileo-e1c", "beidou-b1i", "beidou-b2i", "gps-l5i", "galileo-e5ai", "galileo-e5aq", "galileo-e5bi",
           "galileo-e5bq", "beidou-b2ad", "beidou-b3i", "glonass-l3ocd", "glonass-l3ocp", "galileo-e6c"}


def _expected_patterns(sec, M, flip):
    """the rule of the issue, restated: rows in order, then duplicates up to a global sign removed"""
    sec = np.ones(1, dtype=int) if sec is None else np.asarray(sec, dtype=int)
    S = len(sec)
    rows = []
    for h in range(S):
        base = [int(sec[(m + h) % S]) for m in range(M)]
        rows.append((base, (h, None)))
        if flip:
            for k in range(1, M):
                if (k + h) % S == 0:             # the overlay restarts at period k: a data bit can change there
                    rows.append(([-v if m >= k else v for m, v in enumerate(base)], (h, k)))
    out, seen = [], []
    for row, label in rows:
        if row not in seen and [-v for v in row] not in seen:
            seen.append(row)
            out.append((row, label))
    return out


@pytest.mark.parametrize("S", [1, 4, 10, 20, 25])
@pytest.mark.parametrize("flip", [False, True])
def test_patterns_rows_labels_and_duplicates(S, flip):
    sec = SEC[S]
    for M in sorted({S, max(S // 2, 1), 5, 2 * S + 1}):
        W, labels = coherent.patterns(sec, M, flip)
        want = _expected_patterns(sec, M, flip)
        assert W.dtype == np.int8 and W.shape == (len(want), M) and len(labels) == len(want)
        assert [list(r) for r in W] == [r for r, _ in want] and labels == [l for _, l in want]
        assert set(np.unique(W)) <= {-1, 1}
        for a in range(len(W)):                  # no two rows equal up to a global sign
            for b in range(a):
                assert not (np.array_equal(W[a], W[b]) or np.array_equal(W[a], -W[b])), (S, M, a, b)
    # over one whole code every row is a rotation of it, and none is lost
    W, labels = coherent.patterns(sec, S, False)
    code = np.ones(1, dtype=np.int8) if sec is None else sec
    assert [l for l in labels] == [(h, None) for h in range(S)]
    for row, (h, _) in zip(W, labels):
        np.testing.assert_array_equal(row, np.roll(code, -h))


def test_patterns_counts_and_dropped_rows():
    count = lambda S, M, flip: len(coherent.patterns(SEC[S], M, flip)[0])
    assert [count(1, 20, f) for f in (False, True)] == [1, 20]                   # GPS L1 C/A: a bit edge at any of the 19 borders
    assert [count(4, 4, f) for f in (False, True)] == [4, 6]
    assert [count(10, 10, f) for f in (False, True)] == [10, 19]
    assert [count(20, 20, f) for f in (False, True)] == [20, 39]                 # one k = 20 - h per row h >= 1
    assert [count(25, 25, f) for f in (False, True)] == [25, 49]
    assert count(20, 5, False) == 15 and count(25, 5, False) == 16               # short windows of an overlay repeat up to sign
    # an alternating overlay: every rotation is the first one up to sign
    W, labels = coherent.patterns([1, -1, 1, -1], 4)
    assert labels == [(0, None)] and W.tolist() == [[1, -1, 1, -1]]
    W, labels = coherent.patterns([1, 1], 2, True)
    assert labels == [(0, None), (1, 1)] and W.tolist() == [[1, 1], [1, -1]]
    W, labels = coherent.patterns(None, 3, True)
    assert labels == [(0, None), (0, 1), (0, 2)] and W.tolist() == [[1, 1, 1], [1, -1, -1], [1, 1, -1]]
    for bad in ([], [1, 0, 1], [[1, -1]], [2]):
        with pytest.raises(ValueError):
            coherent.patterns(bad, 3)
    with pytest.raises(ValueError):
        coherent.patterns(None, 0)


def test_starts_with_and_without_code_doppler():
    sig = signals.get("gps-l5i")
    f = np.array([-7000.0, -200.0, 0.0, 200.0, 7000.0])
    st = coherent.starts(sig, f, 20)
    assert st.dtype == np.int64 and st.shape == (5, 20) and st.flags["C_CONTIGUOUS"]
    np.testing.assert_array_equal(st, np.tile(np.arange(20) * 30690, (5, 1)))
    carrier = 1176.45e6
    sl = coherent.starts(sig, f, 20, carrier_hz=carrier)
    want = np.array([[m * 30690 - int(np.rint(m * 30690 * fd / carrier)) for m in range(20)] for fd in f])
    np.testing.assert_array_equal(sl, want)
    np.testing.assert_array_equal(sl[2], st[2])                                   # zero Doppler: no slip
    assert np.all(sl[:2] >= st[:2]) and np.all(sl[3:] <= st[3:])                  # a receding satellite's periods arrive later
    assert sl[0, -1] - st[0, -1] == 3 and sl[4, -1] - st[4, -1] == -3             # 19 x 30690 x 7000 / 1176.45e6 = 3.47 samples
    assert np.all(np.diff(sl, axis=1) > 0) and np.all(sl[:, 0] == 0)              # monotone in m
    assert coherent.starts("gps-l1", 500.0, 3).tolist() == [[0, 4096, 8192]]      # a scalar Doppler is one row


def test_builtin_secondary_codes_equal_the_reference_arrays():
    with open(os.path.join(GOLD, "secondary_codes.json")) as f:
        gold = json.load(f)["codes"]
    assert set(gold) == set(coherent.SECONDARY)
    assert sum(isinstance(v, list) for v in gold.values()) == 11 and sum(isinstance(v, dict) for v in gold.values()) == 3
    for code, v in gold.items():
        got = coherent.SECONDARY[code]
        if isinstance(v, dict):
            assert sorted(got) == sorted(int(p) for p in v) == list(range(1, 51)), code
            for prn, arr in v.items():
                assert got[int(prn)].dtype == np.int8 and got[int(prn)].tolist() == arr, (code, prn)
        else:
            assert got.dtype == np.int8 and got.tolist() == v, code


def test_one_block_is_one_secondary_chip_for_every_signal():
    offered = set()
    for name, sig in signals.SIGNALS.items():
        L, rate = codes.code_length(sig.code), codes.chip_rate(sig.code)
        want = Fraction(L) / Fraction(rate) == Fraction(sig.n) / Fraction(sig.fs)
        assert coherent.one_block_per_secondary_chip(sig) == want, name
        if sig.code in coherent.SECONDARY:
            assert want, name
            sec = coherent.builtin_secondary(name)
            assert sec is coherent.SECONDARY[sig.code]
            offered.add(name)
        else:
            with pytest.raises(ValueError, match=name):
                coherent.builtin_secondary(name)
    assert offered == BUILTIN
    # a descriptor whose block is two code periods long is refused by name, whatever its code module offers
    double = dataclasses.replace(signals.get("beidou-b1i"), name="b1i-2ms", n=16384)
    assert not coherent.one_block_per_secondary_chip(double)
    with pytest.raises(ValueError, match="b1i-2ms"):
        coherent.builtin_secondary(double)
    with pytest.raises(ValueError, match="b1i-2ms"):
        coherent.search(double, None, [1], [0.0], 4)                              # before any GPU work: x_dev is never looked at


def test_search_refuses_before_any_gpu_work():
    for name in ("glonass-l1", "glonass-l2"):
        with pytest.raises(ValueError, match="FDMA"):
            coherent.search(name, None, [0], [0.0], 4, secondary=None)
    with pytest.raises(ValueError, match="gps-l1"):
        coherent.search("gps-l1", None, [1], [0.0], 4)                            # no built-in code: pass one, or None
    with pytest.raises(ValueError, match="item"):
        coherent.search("galileo-e6c", None, [1, 51], [0.0], 4)                   # the table has no PRN 51
    with pytest.raises(ValueError):
        coherent.search("gps-l1", None, [1], [0.0], 129, secondary=None)          # M > 128
    with pytest.raises(ValueError):
        long = 1 - 2 * np.random.Generator(np.random.PCG64(5)).integers(0, 2, size=300)
        assert len(coherent.patterns(long, 40)[0]) == 300
        coherent.search("gps-l1", None, [1], [0.0], 40, secondary=long)           # 300 hypotheses > 256


@pytest.mark.parametrize("name,M,delay", [("gps-l1", 4, 1201), ("beidou-b1i", 4, 5003)])
def test_correlation_of_a_folded_row_is_the_signed_sum_of_the_period_correlations(name, M, delay):
    """Linearity, on seeded noise plus signal: acq_oracle's correlation of y[d, h] equals sum_m W[h, m] times its correlation of the
    m-th carrier-wiped period, to 1e-9 of the peak."""
    sig = signals.get(name)
    prn = 9
    rng = np.random.Generator(np.random.PCG64(41 + M))
    n_out = sig.samples_needed(1)
    nsamp = (M - 1) * sig.n + n_out + 16
    x = rng.standard_normal(nsamp) + 1j * rng.standard_normal(nsamp)
    rep = codes.replica(sig.code, prn, sig.n, sig.boc).astype(np.float64)
    i = np.arange(nsamp)
    sec = np.array([1, 1, 1, -1])
    x += 0.5 * sec[((i - delay) // sig.n) % 4] * rep[(i - delay) % sig.n] * np.exp(2j * np.pi * 1537.0 * i / sig.fs)
    f = np.array([1500.0, 1537.0])
    W, _ = coherent.patterns(sec, M)
    assert W.shape == (4, M)
    st = coherent.starts(sig, f, M, carrier_hz=1575.42e6 / 2000.0) + 3              # odd starts, a slip of whole samples
    C_ = O.code_spectrum(sig, codes_oracle.chips(sig.code, prn))
    y = O.fold64(x, n_out, st, f, sig.fs, W, j0=12345)
    worst = 0.0
    for d in range(len(f)):
        per = np.stack([O.correlate(v, C_) for v in O.wiped(x, n_out, st[d], f[d], sig.fs, j0=12345)])
        for h in range(len(W)):
            r = O.correlate(y[d, h], C_)
            want = W[h].astype(np.float64) @ per
            worst = max(worst, float(np.max(np.abs(r - want)) / np.max(np.abs(want))))
    print("%s: max |corr(fold) - sum W corr(period)| / peak = %.3g" % (name, worst))
    assert worst <= 1e-9


@pytest.fixture(scope="module")
def chains():
    """the oracle chain on every recording and seed, once: {(key, seed, item): (met, idx, d, h)}"""
    out = {}
    for key, rec in C.RECORDINGS.items():
        sig = signals.get(rec["signal"])
        st = coherent.starts(sig, rec["dopplers"], rec["M"])
        for seed in rec["seeds"]:
            x = C.recording(key, seed).astype(np.complex128)
            for sat in rec["sats"]:
                W, _ = coherent.patterns(C.secondary_of(rec, sat["item"]), rec["M"], rec["data_flip"])
                y = O.fold64(x, sig.samples_needed(1), st, rec["dopplers"], sig.fs, W)
                out[key, seed, sat["item"]] = O.chain(sig, codes_oracle.chips(sig.code, sat["item"]), y)
    return out


@pytest.mark.parametrize("key", sorted(C.RECORDINGS))
def test_oracle_chain_recovers_the_truth(chains, key):
    """Every seed: the chain's first strictly greatest cell is the true (d, h) at the true code offset.  Printed: the margin (best
    metric over the best wrong cell) per seed, and how many seeds the plain non-coherent search over the same M periods and the
    one-period search find (code offset and Doppler) -- the figures of DESIGN 5.16."""
    rec = C.RECORDINGS[key]
    sig = signals.get(rec["signal"])
    assert len(rec["seeds"]) >= 6
    ds = rec["dopplers"]
    grid = [ds[0], ds[-1] + (ds[1] - ds[0]) / 2, ds[1] - ds[0]]
    margins, plain, single, total = [], 0, 0, 0
    for seed in rec["seeds"]:
        x = C.recording(key, seed).astype(np.complex128)
        for sat in rec["sats"]:
            met, idx, d, h = chains[key, seed, sat["item"]]
            td, th, tc = C.truth(key, sat)
            L = codes.code_length(sig.code)
            assert (d, h) == (td, th) and O.code_offset(sig, L, idx[d, h]) == tc, (key, seed, sat["item"], (d, h), (td, th))
            rest = met.copy()
            rest[td, th] = -np.inf
            margins.append(float(met[td, th] / rest.max()))
            for blocks in (rec["M"], 1):
                m_, c_, f_ = acq_oracle.search_script_blocks(rec["signal"], x, sat["item"], grid, blocks)
                hit = int(c_ == tc and f_ == ds[td])
                plain, single = plain + hit * (blocks > 1), single + hit * (blocks == 1)
            total += 1
    print("%-8s margin worst %.3f median %.3f | found by the non-coherent search over M periods %d/%d, by one period %d/%d"
          % (key, min(margins), float(np.median(margins)), plain, total, single, total))
    assert min(margins) > 1.0
