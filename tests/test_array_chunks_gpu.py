"""GPU: nulling and stap calls that ar_run_dev (csrc/gacq_arrayhost.h) cuts into several triples of launches, on the recordings of
tests/array_chunk_cases.py.  Every comparison is equality with the oracle: the output bytes, stats as (clipped, owned), d_weights as
int32 and d_cov as int64 where it is requested.  Every call goes through the raw ABI on exactly the input it needs, a slice at an odd
address of a tensor whose neighbouring bytes are 127, and writes into tensors that carry sentinels past their ends.

  whole    the recording from output 0 in one call, int8 at gain 2.5 (the clip count is nonzero and sums over the launches) and complex64
           at gain 1: the first chunk holds the warm-up, the later ones run with pb0 > 0, p_off = W and warm = 0;
  mid      from (W + 1) Lb + 5 to the end: the second chunk starts inside an apply tile that the first chunk's launch also wrote, and
           own_first = b0 + 1; also equal to that range of the whole call, device against device;
  edge     cases A and D: n_out that ends exactly on (b0 + K) Lb is one chunk; one sample more is a second chunk of one output;
  far      case A with 2^32 - 2^19 added to every index: the first chunk straddles 2^32, the second lies above it;
  stream   stap.Stream given one piece of more than K blocks, then pieces of 4097 and 5 samples;
  file     stap.convert_files on case D's eight antennas: each arrives as one piece of 5257 blocks, the shape of the default command line.

test_array_chunks_cpu.py asserts on the CPU that the oracle keeps its margin on every case and that K is the library's."""
import ctypes

import numpy as np
import pytest

import array_chunk_cases as C
from gnss_dsp_tools_amd import _native as nat
from gnss_dsp_tools_amd import nulling, stap
from gnss_dsp_tools_amd.streaming import owned_blocks

SENT = 77
DTYPES = ["int8", "complex64"]
_WHOLE = {}                                         # (case, dtype) -> the device's result of the whole-recording call, kept for `mid` and `edge`


def _dev(engine, x, off=0):
    """the int8 array on the device, its first byte `off` bytes past a 256-byte boundary, in a tensor whose other bytes are 127"""
    torch = nat.require_torch()
    x = np.ascontiguousarray(x).view(np.int8).reshape(-1)
    buf = torch.full((len(x) + 1024,), 127, dtype=torch.int8, device="cuda:%d" % engine.device)
    off += 256 + (-buf.data_ptr()) % 256
    v = buf[off:off + len(x)]
    v.copy_(torch.from_numpy(x))
    return v


def _open(engine, name):
    tool, M, T, W = C.CASES[name][:4]
    return stap.Stap(engine, M, T, C.Lb, W, C.LOAD_SHIFT) if tool == "stap" else nulling.Nuller(engine, M, C.Lb, W, C.LOAD_SHIFT)


def _inputs(engine, name, call):
    """the inputs of a C.calls() entry (or of its near twin, for `far`): exactly the samples the call needs"""
    in_first, in_count = call[0] - C.FAR_SHIFT if call[0] >= C.FAR_SHIFT else call[0], call[1]
    return [_dev(engine, x, 2 * p + 1) for p, x in enumerate(C.cut(name, in_first, in_first + in_count))]


def _run(engine, h, name, ds, call, dtype, cov=None):
    """one gacq_*_run_dev call (in_first, in_count, out_first, n_out) into fresh tensors with sentinels past their ends: a dict of out
    (numpy, int8 or complex64), stats (clipped, owned), wq int32 [owned][N][2] and cov int64 [owned][N][N][2] or None"""
    torch = nat.require_torch()
    tool, M, T, W = C.CASES[name][:4]
    in_first, in_count, out_first, n_out = call
    cov = C.CASES[name][7] if cov is None else cov
    N, cplx, dev = M * T, dtype == "complex64", ds[0].device
    assert all(d.numel() == 2 * in_count for d in ds) and len(ds) == M
    nbytes, nblk = n_out * (8 if cplx else 2), owned_blocks(C.Lb, out_first, n_out)
    out = torch.full((nbytes + 64,), SENT, dtype=torch.uint8, device=dev)
    stats = torch.tensor([0, 0, SENT], dtype=torch.int64, device=dev)
    wq = torch.full((2 * N * nblk + 16,), SENT, dtype=torch.int32, device=dev)
    cv = torch.full((2 * N * N * nblk + 16,), SENT, dtype=torch.int64, device=dev) if cov else None
    ptrs = (ctypes.c_void_p * M)(*[d.data_ptr() for d in ds])
    engine.use_torch_stream(dev)
    rc = getattr(nat.lib, h._runner)(h._h, ctypes.cast(ptrs, ctypes.c_void_p), in_first, in_count, out_first, n_out, C.GAIN_C64 if cplx else C.GAIN_INT8,
                                     int(cplx), ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(stats.data_ptr()), ctypes.c_void_p(wq.data_ptr()),
                                     ctypes.c_void_p(cv.data_ptr()) if cov else None)
    assert rc == 0, (name, call, rc, nat.lib.gacq_last_error(engine._ctx))
    torch.cuda.synchronize()
    assert bool((out[nbytes:] == SENT).all()) and bool((wq[2 * N * nblk:] == SENT).all()) and int(stats[2]) == SENT, (name, call, "a sentinel was written")
    assert cv is None or bool((cv[2 * N * N * nblk:] == SENT).all()), (name, call, "a sentinel was written")
    st = stats.cpu().tolist()
    return {"out": out[:nbytes].cpu().numpy().view(np.complex64 if cplx else np.int8), "stats": (st[0], st[1]),
            "wq": wq[:2 * N * nblk].cpu().numpy().reshape(nblk, N, 2), "cov": None if cv is None else cv[:2 * N * N * nblk].cpu().numpy().reshape(nblk, N, N, 2)}


def _equals_the_oracle(got, want, label):
    print(label, "stats", got["stats"], "oracle", (want["clipped"], want["owned"]), "outputs", len(got["out"]))
    assert got["out"].dtype == want["out"].dtype and got["out"].tobytes() == want["out"].tobytes(), (label, "output bytes",
                                                                                                      np.flatnonzero(got["out"] != want["out"])[:4])
    assert got["stats"] == (want["clipped"], want["owned"]), (label, got["stats"], (want["clipped"], want["owned"]))
    assert got["wq"].dtype == np.int32 and got["wq"].shape == want["wq"].shape and np.array_equal(got["wq"], want["wq"]), (
        label, "weights", np.argwhere(got["wq"] != want["wq"])[:4])
    if got["cov"] is not None:
        assert got["cov"].dtype == np.int64 and got["cov"].shape == want["cov"].shape and np.array_equal(got["cov"], want["cov"]), (
            label, "window sums", np.argwhere(got["cov"] != want["cov"])[:4])


def _same(a, b, label):
    """two device results, bit for bit"""
    assert a["out"].tobytes() == b["out"].tobytes() and a["stats"] == b["stats"] and a["wq"].tobytes() == b["wq"].tobytes(), label
    assert (a["cov"] is None) == (b["cov"] is None) and (a["cov"] is None or a["cov"].tobytes() == b["cov"].tobytes()), label


def _whole(engine, name, dtype):
    if (name, dtype) not in _WHOLE:
        call = C.calls(name)["whole"]
        with _open(engine, name) as h:
            _WHOLE[name, dtype] = _run(engine, h, name, _inputs(engine, name, call), call, dtype)
    return _WHOLE[name, dtype]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", C.TABLE)
def test_the_whole_recording_in_one_call_equals_the_oracle(engine, name, dtype):
    """two chunks, three in case D: the clip count and the owned count are sums over the launches, the weights and window sums of the
    later chunks land at b - own_first behind those of the first"""
    call = C.calls(name)["whole"]
    assert C.chunks_of(name, call[2], call[3]) == C.MIN_CHUNKS[name] >= 2
    want = C.reference(name, dtype == "complex64")
    assert (want["clipped"] > 0) == (dtype == "int8") and want["owned"] > C.CASES[name][4]
    _equals_the_oracle(_whole(engine, name, dtype), want, "%s whole %s" % (name, dtype))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", C.TABLE)
def test_a_call_from_mid_block_past_the_warm_up_equals_the_oracle_and_the_whole_call(engine, name, dtype):
    """out_first = (W + 1) Lb + 5: no chunk holds a warm-up block, the first output's block is not owned, and the later chunks start
    inside an apply tile"""
    call = C.calls(name)["mid"]
    o, per = call[2], 1 if dtype == "complex64" else 2
    assert o == C.mid_first(name) and C.chunks_of(name, o, call[3]) == C.MIN_CHUNKS[name] and call[0] > 0
    with _open(engine, name) as h:
        got = _run(engine, h, name, _inputs(engine, name, call), call, dtype)
    _equals_the_oracle(got, C.reference_from(name, o, dtype == "complex64"), "%s mid %s" % (name, dtype))
    # the same range of the whole-recording call: a check that does not pass through the oracle
    whole, own = _whole(engine, name, dtype), -(-o // C.Lb)
    assert got["out"].tobytes() == whole["out"][per * o:].tobytes() and got["wq"].tobytes() == whole["wq"][own:].tobytes(), (name, dtype)
    assert got["stats"][1] == whole["stats"][1] - own and (got["cov"] is None or got["cov"].tobytes() == whole["cov"][own:].tobytes()), (name, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("name", C.EDGE_CASES)
def test_the_chunk_edge_itself(engine, name):
    """n_out ending exactly on (b0 + K) Lb from output 0 is one chunk; one sample more is a second chunk of one output in block K, whose
    weights see the W covariances before it (ncov = W): one more owned block, one more weights row, the rest unchanged"""
    e, K = C.edge(name), C.CASES[name][4]
    calls = C.calls(name)
    got = {}
    with _open(engine, name) as h:
        for label in ("edge", "edge + 1"):
            call = calls[label]
            assert call[2] == 0 and call[3] == e + (label != "edge") and C.chunks_of(name, 0, call[3]) == 1 + (label != "edge")
            got[label] = _run(engine, h, name, _inputs(engine, name, call), call, "int8")
            _equals_the_oracle(got[label], C.reference_call(name, 0, call[3]), "%s %s" % (name, label))
    a, b = got["edge"], got["edge + 1"]
    assert a["stats"][1] == K and b["stats"][1] == K + 1 and a["wq"].shape[0] == K and b["wq"].shape[0] == K + 1
    assert b["out"][:2 * e].tobytes() == a["out"].tobytes() and b["wq"][:K].tobytes() == a["wq"].tobytes() and 0 <= b["stats"][0] - a["stats"][0] <= 2
    whole = _whole(engine, name, "int8")
    assert b["out"].tobytes() == whole["out"][:2 * (e + 1)].tobytes() and b["wq"].tobytes() == whole["wq"][:K + 1].tobytes()
    assert b["cov"] is None or b["cov"].tobytes() == whole["cov"][:K + 1].tobytes()


@pytest.mark.gpu
def test_a_far_call_whose_first_chunk_straddles_two_to_the_32(engine):
    """case A, int8: the mid call with 2^32 - 2^19 added to in_first and out_first.  Equal to the oracle at those indices, and every
    output, count and side array equal to the near call's, bit for bit"""
    name = "A"
    near_call, far_call = C.calls(name)["mid"], C.calls(name)["far"]
    K, first, count = C.CASES[name][4], far_call[2], far_call[3]
    assert far_call == (near_call[0] + C.FAR_SHIFT, near_call[1], near_call[2] + C.FAR_SHIFT, near_call[3])
    assert first < 1 << 32 < (first // C.Lb + K) * C.Lb < first + count and C.chunks_of(name, first, count) == 2
    ds = _inputs(engine, name, far_call)
    with _open(engine, name) as h:
        near = _run(engine, h, name, ds, near_call, "int8")
        far = _run(engine, h, name, ds, far_call, "int8")
    want = C.oracle(name, C.cut(name, near_call[0], near_call[0] + near_call[1]), far_call[0], first, count)
    assert want["margin"] >= C.MARGIN
    _equals_the_oracle(far, want, "A far")
    _equals_the_oracle(near, C.reference_from(name, near_call[2]), "A near")
    _same(far, near, "A far against the near call")


@pytest.mark.gpu
def test_a_stream_piece_of_more_than_a_chunk_then_small_pieces(engine):
    """case C's configuration on the recording of case S: the first piece makes a call of two chunks, the tail it leaves and the pieces
    of 4097 and 5 samples that follow give the rest; the joined output and weight trace are the one-call result and the oracle's"""
    torch = nat.require_torch()
    name = "S"
    tool, M, T, W, K = C.CASES[name][:5]
    assert C.CASES["C"][:5] == C.CASES[name][:5] and tool == "stap"
    xs, n = C.data(name), C.samples(name)
    sizes = [(K + 1) * C.Lb + 7, 4097, 5, 4097, 5]
    sizes.append(n - sum(sizes))
    assert 0 < sizes[-1] < 4097 and sizes[0] - C.tc(name) > K * C.Lb
    one, st, wq = stap.convert(engine, list(xs), T, C.Lb, W, C.LOAD_SHIFT, None, C.GAIN_INT8, "int8", weights=True)
    want = C.reference(name)
    assert one.cpu().numpy().tobytes() == want["out"].tobytes() and st == (want["clipped"], want["owned"]) and np.array_equal(wq.cpu().numpy(), want["wq"])
    s = stap.Stream(engine, M, C.GAIN_INT8, T, C.Lb, W, C.LOAD_SHIFT, None, "int8", weights=True)
    try:
        outs, at = [], 0
        for size in sizes:
            outs.append(s.feed([x[2 * at:2 * (at + size)] for x in xs]))
            at += size
        assert at == n and outs[0].numel() == 2 * (sizes[0] - C.tc(name)) and s.traces[0].shape[0] == K + 2
        assert s.next_out == C.outputs(name) and all(o.numel() == 2 * z for o, z in zip(outs[1:], sizes[1:]))
        assert bool((torch.cat(outs) == one).all()) and s.stats() == st and bool((torch.cat(s.traces) == wq).all())
    finally:
        s.close()


@pytest.mark.gpu
def test_the_file_pump_hands_stap_one_piece_of_three_chunks(engine, tmp_path):
    """stap.convert_files on case D's eight antennas at a fixed gain: every file is shorter than a piece of the pump, so the device
    gets one call of 5257 blocks and a partial one, as the default command line gives it with 8 antennas; the file is the oracle's bytes"""
    name = "D"
    tool, M, T, W, K = C.CASES[name][:5]
    paths = [str(tmp_path / ("ant%d.iq" % p)) for p in range(M)]
    for x, path in zip(C.data(name), paths):
        x.tofile(path)
    want = C.reference(name)
    assert M == 8 and C.outputs(name) // C.Lb == 5257 > 2 * K
    fins = [open(p, "rb") for p in paths]
    try:
        with open(str(tmp_path / "out.iq"), "wb") as fout, open(str(tmp_path / "w.bin"), "wb") as ftrace:
            gain, n, clipped = stap.convert_files(engine, fins, fout, T, C.Lb, W, C.LOAD_SHIFT, None, C.GAIN_INT8, ftrace=ftrace)
    finally:
        for f in fins:
            f.close()
    assert (gain, n, clipped) == (C.GAIN_INT8, C.outputs(name), want["clipped"])
    assert open(str(tmp_path / "out.iq"), "rb").read() == want["out"].tobytes()
    assert open(str(tmp_path / "w.bin"), "rb").read() == want["wq"].tobytes()
