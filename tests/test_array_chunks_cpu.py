"""CPU: what the multi-chunk tests of nulling and stap (test_array_chunks_gpu.py) rest on, established without a device -- the oracle alone
keeps every case of tests/array_chunk_cases.py away from a rounding tie; the chunk K of every case is the library's, not a constant of
the tests; every recording owns more than K blocks (case D more than 2 K), so the calls really take a second triple of launches; and
gacq_null_check / gacq_stap_check accept every call the GPU tests make and refuse it one sample short at either end."""
import ctypes

import pytest

import array_chunk_cases as C
from gnss_dsp_tools_amd import _native as nat
from gnss_dsp_tools_amd import nulling, stap

SHORT_INPUT = -6


def _stap_chunk(M, T, W):
    """K of a stap configuration, solved from gacq_stap_workspace(cfg) = ((K + W) N^2 + K N) 8"""
    cfg = stap.make_cfg(M, T, C.Lb, W, C.LOAD_SHIFT)
    ws, N = nat.lib.gacq_stap_workspace(ctypes.addressof(cfg)), M * T
    assert ws > 0 and ws % 8 == 0 and (ws // 8 - W * N * N) % (N * N + N) == 0, (M, T, W, ws)
    return (ws // 8 - W * N * N) // (N * N + N)


def test_no_scaled_weight_of_any_case_lies_within_the_margin_of_a_rounding_tie():
    m = C.margins()
    print({k: "%.3g" % v for k, v in m.items()})
    assert set(m) == set(C.CASES) and all(v >= C.MARGIN for v in m.values())
    for name in C.CASES:
        ref = C.reference(name)
        assert ref["clipped"] > 0 and ref["owned"] == -(-C.outputs(name) // C.Lb)             # the clip count has something to sum


def test_the_chunk_of_every_case_is_the_librarys():
    """stap: K from the workspace the library itself reports.  nulling: gacq_null.hip hands ar_run_dev the shared kArMaxChunk, which is
    what gacq_stap_workspace gives for (M, T) = (2, 1), whose 64 MiB would hold far more -- the assumption behind cases A and B, which
    this test writes down and checks as far as the library lets it."""
    for name, (tool, M, T, W, K, blocks, seed, cov) in C.CASES.items():
        if tool == "stap":
            assert _stap_chunk(M, T, W) == K, name
    assert C.CASES["C"][4] == 1 << 14 and C.CASES["D"][4] == 2627
    for W in (1, 3):
        assert _stap_chunk(2, 1, W) == 1 << 14 == C.CASES["A"][4] == C.CASES["B"][4]
    assert C.CASES["A"][:4] == ("nulling", 2, 1, 1) and C.CASES["B"][:4] == ("nulling", 2, 1, 3)


@pytest.mark.parametrize("name", list(C.CASES))
def test_every_recording_owns_more_blocks_than_a_chunk_holds(name):
    tool, M, T, W, K, blocks, seed, cov = C.CASES[name]
    n = C.outputs(name)
    owned = -(-n // C.Lb)
    assert owned > K * (C.MIN_CHUNKS[name] - 1) and C.chunks_of(name, 0, n) == C.MIN_CHUNKS[name]
    if name == "D":
        assert owned > 2 * K and C.chunks_of(name, 0, n) == 3                                  # a middle chunk
    o = C.mid_first(name)
    assert o % C.Lb and o // C.Lb >= W + 1 and (o // C.Lb * C.Lb) % 16384 and C.chunks_of(name, o, n - o) == C.MIN_CHUNKS[name]
    assert (o // C.Lb + K) * C.Lb % 16384                                                      # the later chunk starts inside an apply tile
    assert all(len(x) == 2 * C.samples(name) for x in C.data(name)) and len(C.data(name)) == M
    if name in C.EDGE_CASES:
        e = C.edge(name)
        assert e == K * C.Lb < n and C.chunks_of(name, 0, e) == 1 and C.chunks_of(name, 0, e + 1) == 2
    if name == "A":
        lo, cnt, first, count = C.calls(name)["far"]
        b0 = first // C.Lb
        assert C.FAR_SHIFT % C.Lb == 0 and first < 1 << 32 < (b0 + K) * C.Lb < first + count and C.chunks_of(name, first, count) == 2
        assert lo < 1 << 32                                                                    # the first chunk straddles, the second lies above


def _check(name, in_first, in_count, out_first, n_out):
    tool, M, T, W = C.CASES[name][:4]
    if tool == "stap":
        cfg = stap.make_cfg(M, T, C.Lb, W, C.LOAD_SHIFT)
        return nat.lib.gacq_stap_check(ctypes.addressof(cfg), in_first, in_count, out_first, n_out, C.GAIN_INT8, 0)
    cfg = nulling.make_cfg(M, C.Lb, W, C.LOAD_SHIFT)
    return nat.lib.gacq_null_check(ctypes.addressof(cfg), in_first, in_count, out_first, n_out, C.GAIN_INT8, 0)


@pytest.mark.parametrize("name", C.TABLE)
def test_the_checks_accept_every_call_of_the_gpu_tests_and_refuse_it_one_sample_short(name):
    got = C.calls(name)
    assert set(got) == {"whole", "mid"} | ({"edge", "edge + 1"} if name in C.EDGE_CASES else set()) | ({"far"} if name == "A" else set())
    for label, (in_first, in_count, out_first, n_out) in got.items():
        assert in_first + in_count <= C.samples(name) + (C.FAR_SHIFT if label == "far" else 0), (name, label)
        assert _check(name, in_first, in_count, out_first, n_out) == 0, (name, label, nat.lib.gacq_last_error(None))
        assert _check(name, in_first, in_count - 1, out_first, n_out) == SHORT_INPUT, (name, label, "high end")
        assert _check(name, in_first + 1, in_count - 1, out_first, n_out) == SHORT_INPUT, (name, label, "low end")
