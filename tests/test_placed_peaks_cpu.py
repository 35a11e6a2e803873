"""The placed-peak inputs of tests/placed_cases.py against the fp64 oracle alone (no GPU): every epoch peaks where it was asked to,
with a margin that no fp32 rounding can close, and the lag lists are the ones DESIGN.md section 3 names.  Plus the host's last step
(acquire.finalize, gacq_finalize) on hand-made shard records with exactly equal metrics and with dead shards."""
import numpy as np
import pytest

import placed_cases as pc
from gnss_dsp_tools_amd import acquire

CASES = [(key, 1) for key in pc.FAMILIES] + [(key, 2) for key in pc.B2_FAMILIES]


def _table(R, stride, ts):
    return {stride * r + t for r in range(R) for t in ts}


# the lag table, restated: (FFT length, lags, epochs)
TABLE = {
    "gps-l1": (4096, _table(16, 256, (0, 15, 16, 63, 64, 255)), 96),
    "glonass-l1-ch0": (16384, _table(32, 512, (0, 63, 64, 511)), 128),
    "glonass-l1-ch-7": (16384, _table(32, 512, (0, 63, 64, 511)), 128),
    "beidou-b1i": (16384, _table(32, 512, (0, 63, 64, 511)), 128),
    "galileo-e1b": (65536, _table(16, 4096, (0, 1, 255, 256, 511, 512, 4095)), 112),
    "gps-l1cd": (81920, _table(20, 4096, (0, 255, 256, 4095)), 80),
    "gps-l2cm": (163840, _table(40, 4096, (0, 4095)) | {255, 256, 39 * 4096 + 255, 39 * 4096 + 256}, 84),
    "gps-l5i": (61380, _table(31, 1980, (0, 1, 219, 220, 1979)), 155),
    "xona-x5p": (30690, _table(31, 990, (0, 109, 110, 989)), 124),
    "galileo-e6b": (30690, _table(31, 990, (0, 109, 110, 989)), 124),
}
B2_REGISTERS = {"gps-l1": (16, 256), "glonass-l1-ch0": (32, 512), "gps-l1cd": (20, 4096), "xona-x5p": (31, 990), "beidou-b1i": (32, 512),
                "galileo-e1b": (16, 4096), "gps-l5i": (31, 1980)}


def test_the_lag_lists_are_the_table_plus_the_named_extras():
    assert set(pc.FAMILIES) == set(TABLE) and set(pc.B2_FAMILIES) == set(B2_REGISTERS)
    for key, (N, lags, count) in TABLE.items():
        name = pc.FAMILIES[key][0]
        _code, _fs, n, pad, _boc, _norm, _bias = pc.variant(name)
        assert (2 * n if pad else n) == N, key
        assert len(lags) == count and max(lags) < N, key
        got = pc.wanted_lags(key, 1)
        assert len(got) == len(set(got)), key
        assert set(got) == lags | set(pc.EXTRA.get(key, ())), key
        assert got[:count] == pc.FAMILIES[key][2] and set(got[:count]) == lags, key
    # the extras reach what they are for: every position class of the two scattered readers
    for M in (1980, 990):
        ts = {lag % M for lag in pc.pfa_extra_lags(M)}
        seg = (11 * (M // 99) + 15) & ~15
        for c in range(9):
            assert pc.pfa_time_index(M, c * seg) in ts and pc.pfa_time_index(M, c * seg + 11 * (M // 99) - 1) in ts, (M, c)
        assert sorted({pc.pfa_time_index(M, p) for p in range(9 * seg)} - {None}) == list(range(M))      # the map is a bijection onto [0, M)
    pos = {((n2 % 256) * 2 + ((n2 // 256) >> 1) * 512 + ((n2 // 256) & 1)) for n2 in (lag % 4096 for lag in pc.paired_extra_lags())}
    assert {256 * w for w in range(16)} | {256 * w + 255 for w in range(16)} <= pos       # first and last thread of every workgroup
    assert {lag // 4096 for lag in pc.paired_extra_lags()} == set(range(16))
    # B = 2: every register index at t = 0 and t = last, as far as two periods in a padded window reach
    for key, (R, stride) in B2_REGISTERS.items():
        name = pc.FAMILIES[key][0]
        _code, _fs, n, pad, _boc, _norm, _bias = pc.variant(name)
        want = [stride * r + t for r in range(R) for t in (0, stride - 1)]
        if pad:
            want = [lag for lag in want if lag == 0 or lag >= n]
            assert 0 in want and max(want) == 2 * n - 1
        assert pc.wanted_lags(key, 2) == want, key


@pytest.mark.parametrize("key,B", CASES, ids=["%s-B%d" % c for c in CASES])
def test_the_oracle_peaks_at_every_wanted_lag_with_a_wide_margin(key, B):
    f = pc.family(key, B)
    assert f["xs"].dtype == np.complex64 and f["xs"].shape[0] == len(f["lags"])
    np.testing.assert_array_equal(f["idx"], np.array(f["lags"]))
    # 1e-3: more than 100 x the tie threshold (8e-6) and the 1e-5 metric bar -- no fp32 engine may move or re-evaluate these peaks
    print(key, B, "min margin %.3g" % f["margin"].min())
    assert f["margin"].min() >= 1e-3, (key, B, int(np.argmin(f["margin"])), f["margin"].min())
    assert np.all(f["metric"] > 0) and np.all(np.isfinite(f["metric"]))


def _records(rows):
    p = np.zeros((len(rows), len(rows[0])), dtype=acquire.PEAK_DTYPE)
    for s, row in enumerate(rows):
        for i, (m, idx, d) in enumerate(row):
            p[s, i] = (m, idx, d)
    return p


def test_finalize_on_exactly_equal_metrics_keeps_the_lowest_global_doppler_index():
    dop = np.arange(12) * 250.0 - 1000.0
    m = 3.1415926535897931           # the same bits in every shard
    dead = (0.0, -1, -1)
    peaks = _records([[(m, 100, 3), (m, 7, 0), dead, (m, 5, 1)],
                      [(m, 200, 0), (np.nextafter(m, 4.0), 8, 2), dead, dead],
                      [(m, 300, 1), (m, 9, 3), (m, 11, 2), (m, 6, 0)]])
    got = acquire.finalize("gps-l1", [1, 2, 3, 4], peaks, dop, shard_d0=[0, 4, 8])
    code = lambda idx: 1023 * (float(idx) / 4096)
    assert got == [(m, code(100), dop[3]), (np.nextafter(m, 4.0), code(8), dop[6]), (m, code(11), dop[10]), (m, code(5), dop[1])]
    # one shard, no shard_d0: the record passes through
    assert acquire.finalize("gps-l1", [1], _records([[(m, 100, 3)]]), dop) == [(m, code(100), dop[3])]


def test_finalize_maps_dead_records_to_the_reference_initial_values():
    dop = np.arange(4) * 500.0
    dead = (0.0, -1, -1)
    for name in ("gps-l1", "beidou-b1i"):
        got = acquire.finalize(name, [1, 2], _records([[dead, dead]]), dop)
        assert got == [(0, 0, 0), (0, 0, 0)] and all(type(v) is int for r in got for v in r), (name, got)
        got = acquire.finalize(name, [1, 2], _records([[dead, dead], [dead, dead]]), dop, shard_d0=[0, 2])
        assert got == [(0, 0, 0), (0, 0, 0)], (name, got)
