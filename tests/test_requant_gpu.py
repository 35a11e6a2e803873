"""GPU: the requantiser kernels (csrc/gacq_requant.hip) against the integer definition of tests/requant_oracle.py.  Every comparison
of output is an equality of bytes: every container, every packed preset in both bit orders and both input widths against the oracle,
with the gain indices and the statistics; device against device however the recording is cut into calls and chunks and wherever the
buffers lie.  Then the three-satellite GPS L1 scene, its second half eight times weaker, through the level control to two bits and
back through ingest into hand-off and tracking, beside the same scene at a static gain."""
import ctypes
import io

import numpy as np
import pytest

import requant_cases as C
import requant_oracle as O
from gnss_dsp_tools_amd import _native as nat
from gnss_dsp_tools_amd import codes, handoff, ingest, requant, simulate, trackloop
from test_requant_cpu import BAD_ARG, SHORT_INPUT, bad_config_calls, bad_run_calls, raw_check


def _bytes(t):
    return t.cpu().numpy().tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_bytes_gain_indices_and_statistics_equal_the_oracle(engine, case):
    name, msb, in_bits, Lb, W, n = case
    fmt = requant.OutFormat(name, msb)
    want, clipped, blocks, k = C.reference(*case)
    G, T = C.tables_for(fmt, Lb, W, in_bits)
    out, st, kidx = requant.convert(engine, fmt, C.signal(n, 5, in_bits), G, T, Lb, W, in_bits, trace=True)
    assert out.dtype == fmt.torch_dtype(nat.require_torch()) and out.numel() * out.element_size() == len(want) == fmt.nbytes(n // fmt.unit * fmt.unit)
    assert _bytes(out) == want.tobytes(), case
    assert np.array_equal(kidx.cpu().numpy(), k) and st == (clipped, blocks), (case, st, clipped, blocks)
    # the case is worth its name: the gain moves, and values clip (complex64 has no clip; int8 times 64 does not reach the int16 limit)
    assert blocks == -(-(n // fmt.unit * fmt.unit) // Lb) and len(set(k.tolist())) > 3 and (clipped > 0 or name == "f32" or (name, in_bits) == ("s16", 8))


# block lengths by the lanes the power kernel gives a block: int8 input has Lb / 8 16-byte words a block, int16 input Lb / 4; up to 64
# words a group of that many lanes, 65 .. 255 words 64 lanes and several words a lane, from 256 words on the whole workgroup
GROUP_CASES = [("s8", 8, 512, 3), ("s8", 8, 528, 2), ("2sm", 8, 1024, 3), ("s8", 8, 1024, 1), ("u8", 16, 272, 3), ("4ob", 16, 512, 2), ("s8", 8, 2032, 2),
               ("s8", 8, 2048, 2), ("s16", 16, 1008, 1), ("1ob", 16, 1024, 2), ("s8", 8, 256, 2), ("2tc", 16, 144, 3)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,in_bits,Lb,W", GROUP_CASES, ids=lambda v: str(v))
def test_every_group_width_of_the_power_kernel(engine, name, in_bits, Lb, W):
    n = 9 * Lb + 100
    fmt = requant.OutFormat(name)
    want, clipped, blocks, k = C.reference(name, True, in_bits, Lb, W, n)
    G, T = C.tables_for(fmt, Lb, W, in_bits)
    out, st, kidx = requant.convert(engine, fmt, C.signal(n, 5, in_bits), G, T, Lb, W, in_bits, trace=True)
    assert _bytes(out) == want.tobytes() and np.array_equal(kidx.cpu().numpy(), k) and st == (clipped, blocks)
    assert blocks == 10 and len(set(k.tolist())) > 2


@pytest.mark.gpu
@pytest.mark.parametrize("name,Lb,W", [("s8", 1024, 2), ("s8", 16, 3), ("2sm", 1024, 1), ("2sm", 48, 3), ("f32", 16, 8), ("1sm", 528, 2)], ids=lambda v: str(v))
def test_blocks_and_cuts_at_workgroup_boundaries(engine, name, Lb, W):
    """A workgroup owns C.tile() outputs from out_first on.  Outputs from 0: where Lb divides the tile a block starts exactly on the
    second and third workgroups' first component.  Outputs from one lane's run, or from one byte's samples, on: that block starts one
    run, or one byte, before the boundary and belongs to the workgroup in front.  Then a call that ends on the boundary and one that
    starts there: bytes, gain indices and statistics against the oracle's for the same ranges."""
    torch = nat.require_torch()
    fmt = requant.OutFormat(name)
    tile = C.tile(fmt)
    assert tile == nat.lib.gacq_requant_tile(ctypes.addressof(requant.make_cfg(fmt, Lb, W, 1)))
    n = 2 * tile + 2 * Lb + 36
    x = C.signal(n, 7)
    G, T = C.tables_for(fmt, Lb, W)
    c = C.ocfg(fmt, Lb, W)
    run = 16 * 8 // fmt.sample_bits                      # samples in a lane's 16 output bytes
    d = requant._device_bytes(engine, x)
    with requant.Requantizer(engine, fmt, G, T, Lb, W) as rq:
        done = (0, 0)
        for out_first, n_out in ((0, n), (run, n - run), (fmt.unit, n - fmt.unit), (0, tile), (tile, n - tile), (tile - run, 2 * run), (Lb, tile)):
            want = O.evaluate(c, G, T, x, out_first, n_out)
            out, kidx = rq.run(d, 0, out_first, n_out, trace=True)
            st = rq.stats()
            assert _bytes(out) == want[0].tobytes(), (name, Lb, out_first, n_out)
            assert np.array_equal(kidx.cpu().numpy(), want[3]) and (st[0] - done[0], st[1] - done[1]) == (want[1], want[2]), (name, Lb, out_first, n_out)
            done = st
    if tile % Lb == 0:
        assert O.evaluate(c, G, T, x, 0, n)[2] == n // Lb + 1 and (2 * tile) % Lb == 0      # blocks start on both boundaries


@pytest.mark.gpu
def test_warm_up_boundary(engine):
    """loud first W blocks, quiet afterwards: blocks 0 .. W share the warm-up level, W + 1 is the first whose window has a quiet block"""
    Lb, W = 64, 3
    x = np.tile(np.array([50, -50], dtype=np.int8), 16 * Lb)
    x[2 * W * Lb:] //= 10
    G, T = requant.tables(32.0, Lb, W)
    want = O.evaluate(O.cfg("s8", Lb, W), G, T, x)
    out, st, kidx = requant.convert(engine, "s8", x, G, T, Lb, W, trace=True)
    k = kidx.cpu().numpy()
    assert _bytes(out) == want[0].tobytes() and np.array_equal(k, want[3]) and st == (want[1], want[2])
    assert k[W - 1] == k[W] == k[0] and k[W + 1] < k[W] and k[W + 2] < k[W + 1] and k[2 * W] == k[2 * W + 1] < k[W + 2]


def _raw_run(engine, cfg, G, T, x, in_first, out_first, n_out, out, stats=None, gidx=None, off=0):
    """gacq_requant_run_dev through the raw ABI on device tensors; x holds the samples from in_first on"""
    G = np.ascontiguousarray(G, dtype=np.float32)
    T = np.ascontiguousarray(T if len(T) else [0], dtype=np.uint64)
    h = ctypes.c_void_p()
    assert nat.lib.gacq_requant_open(engine._ctx, ctypes.addressof(cfg), ctypes.c_void_p(G.ctypes.data), ctypes.c_void_p(T.ctypes.data), ctypes.byref(h)) == 0
    try:
        engine.use_torch_stream()
        return nat.lib.gacq_requant_run_dev(h, ctypes.c_void_p(x.data_ptr()), in_first, x.numel() * x.element_size() // (2 * cfg.in_bits // 8), out_first, n_out,
                                            ctypes.c_void_p(out.data_ptr() + off), ctypes.c_void_p(stats.data_ptr()) if stats is not None else None,
                                            ctypes.c_void_p(gidx.data_ptr()) if gidx is not None else None)
    finally:
        nat.lib.gacq_requant_close(h)


@pytest.mark.gpu
def test_level_exactly_at_a_threshold_and_one_above(engine):
    """constant input (3, 4): P = 25 Lb, S = 25 Lb W = 1200; S > T is strict"""
    torch = nat.require_torch()
    dev = "cuda:%d" % engine.device
    Lb, W, n = 16, 3, 100
    x = torch.from_numpy(np.tile(np.array([3, 4], dtype=np.int8), n)).to(dev)
    cfg = requant.make_cfg("s8", Lb, W, 3)
    for T, k in (([1200, 5000], 0), ([1199, 5000], 1), ([1199, 1199], 2), ([0, 1200], 1), ([1201, 1201], 0)):
        out = torch.zeros(2 * n, dtype=torch.int8, device=dev)
        gidx = torch.full((7,), 99, dtype=torch.uint8, device=dev)
        assert _raw_run(engine, cfg, [8.0, 2.0, 0.5], T, x, 0, 0, n, out, gidx=gidx) == 0
        g = [8.0, 2.0, 0.5][k]
        assert out.cpu().numpy().tolist() == [int(np.rint(3 * g)), 4 * int(g) if g >= 1 else 2] * n, (T, k)
        assert gidx.cpu().numpy().tolist() == [k] * 7


@pytest.mark.gpu
def test_int16_full_scale_gives_the_largest_power(engine):
    """-32768 throughout: P = Lb 2^31, S = W Lb 2^31 = 2^40 at Lb = 64, W = 8"""
    torch = nat.require_torch()
    dev = "cuda:%d" % engine.device
    Lb, W, n = 64, 8, 1000
    x = torch.full((2 * n,), -32768, dtype=torch.int16, device=dev)
    cfg = requant.make_cfg("s16", Lb, W, 2, in_bits=16)
    for T, k in (([1 << 40], 0), ([(1 << 40) - 1], 1)):
        out = torch.zeros(2 * n, dtype=torch.int16, device=dev)
        stats = torch.zeros(2, dtype=torch.int64, device=dev)
        gidx = torch.full((16,), 99, dtype=torch.uint8, device=dev)
        assert _raw_run(engine, cfg, [1.0, 0.5], T, x, 0, 0, n, out, stats, gidx) == 0
        assert out.cpu().numpy().tolist() == [-32767 if k == 0 else -16384] * (2 * n)
        assert stats.cpu().tolist() == [2 * n if k == 0 else 0, 16] and gidx.cpu().numpy().tolist() == [k] * 16
    x64 = np.full(2 * 65536 + 2, -32768, dtype=np.int16)                   # one block of the longest kind: 2^47
    want = O.evaluate(O.cfg("u8", 65536, 1, in_bits=16), [2.0 ** -8, 2.0 ** -9], [(1 << 47) - 1], x64)
    out, st, kidx = requant.convert(engine, "u8", x64, [2.0 ** -8, 2.0 ** -9], [(1 << 47) - 1], 65536, 1, 16, trace=True)
    assert _bytes(out) == want[0].tobytes() and kidx.cpu().numpy().tolist() == [1, 1] and set(out.cpu().numpy().tolist()) == {64} and st == (0, 2)


RAMP_GAINS = (0.5, 1.0, 1.5, 0.25, 127.5 / 127.0, 3.0, 300.0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", C.CONTAINERS + ("1ob", "2ob", "2sm", "4ob", "4tc"))
def test_level_edges_ties_and_clip_limits_under_one_fixed_gain(engine, name):
    """K = 1: every int8 value (and int16 values around the limits) under gains that put values on .5, on +-2.0 and the other level
    edges, and on and past the clip limits both ways"""
    x = np.arange(-128, 128, dtype=np.int8)
    data8 = np.stack([x, x[::-1]], axis=1).reshape(-1)
    y = np.concatenate([np.arange(-32768, -32768 + 128), np.arange(-64, 64), np.arange(32767 - 127, 32768), np.arange(-255, 257, 2)[:128]]).astype(np.int16)
    data16 = np.stack([y, y[::-1]], axis=1).reshape(-1)
    fmt = requant.OutFormat(name)
    for in_bits, data in ((8, data8), (16, data16)):
        for gain in RAMP_GAINS + ((2.0 ** -8, 127.0 / 32768.0, 1.0 / 258.0) if in_bits == 16 else ()):
            G, T = requant.fixed(gain)
            want = O.evaluate(C.ocfg(fmt, 16, 1, in_bits), G, T, data)
            out, st = requant.convert(engine, fmt, data, G, T, 16, 1, in_bits)
            assert _bytes(out) == want[0].tobytes() and st == (want[1], want[2]), (name, in_bits, gain, st, want[1:3])
    if name == "s8":
        i = requant.convert(engine, fmt, data8, *requant.fixed(0.5), 16, 1)[0].cpu().numpy()[0::2]
        assert i[128 + 1] == 0 and i[128 + 3] == 2 and i[128 + 5] == 2 and i[128 - 1] == 0 and i[128 - 3] == -2
        i = requant.convert(engine, fmt, data8, *requant.fixed(1.5), 16, 1)[0].cpu().numpy()[0::2]
        assert i[0] == -127 and i[255] == 127 and i[128 + 84] == 126 and i[128 + 85] == 127 and i[128 - 85] == -127
    if name == "2ob":
        out = requant.convert(engine, fmt, data8, *requant.fixed(0.5), 16, 1)[0].cpu().numpy()
        lev = O.levels_of_codes(C.ocfg(fmt, 16, 1), out)[0::2]
        assert lev[128 + 4] == 3 and lev[128 + 3] == 1 and lev[128] == 1 and lev[128 - 1] == -1 and lev[128 - 4] == -1 and lev[128 - 5] == -3


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["s8", "1sm", "4ob"])
def test_a_recording_of_w_blocks_and_one_sample_and_one_of_fewer(engine, name):
    torch = nat.require_torch()
    dev = "cuda:%d" % engine.device
    Lb, W = 64, 3
    fmt = requant.OutFormat(name)
    G, T = C.tables_for(fmt, Lb, W)
    n = W * Lb + fmt.unit                                        # one sample, or one byte of samples, into block W
    x = C.signal(4099, 5)[:2 * n]
    want = O.evaluate(C.ocfg(fmt, Lb, W), G, T, x)
    out, st, kidx = requant.convert(engine, fmt, x, G, T, Lb, W, trace=True)
    assert _bytes(out) == want[0].tobytes() and len(want[0]) == fmt.nbytes(n) and st == (want[1], W + 1) and kidx.cpu().numpy().tolist() == [want[3][0]] * (W + 1)
    # fewer than W blocks: nothing to convert, and a call that asks for output is refused before anything is written
    short = x[:2 * (W * Lb - 1)]
    out, st = requant.convert(engine, fmt, short, G, T, Lb, W)
    assert out.numel() == 0 and st == (0, 0)
    d = torch.from_numpy(short.copy()).to(dev)
    buf = torch.full((256,), 77, dtype=torch.uint8, device=dev)
    stats = torch.zeros(2, dtype=torch.int64, device=dev)
    for n_out in (fmt.unit, W * Lb - 4):
        assert _raw_run(engine, requant.make_cfg(fmt, Lb, W, len(G)), G, T, d, 0, 0, n_out, buf, stats) == SHORT_INPUT
    torch.cuda.synchronize()
    assert bool((buf == 77).all()) and stats.cpu().tolist() == [0, 0]


CUT_N = 20000
FEED_CHUNKS = (1, 3, 4097, 10001)


@pytest.mark.gpu
@pytest.mark.parametrize("name,msb,in_bits,Lb,W", [("s8", True, 8, 64, 3), ("1sm", True, 8, 16, 8), ("2tc", False, 16, 64, 1), ("4sm", True, 8, 16, 3),
                                                   ("s16", True, 16, 16, 1), ("f32", True, 8, 64, 8)], ids=lambda v: str(v))
def test_cutting_into_calls_and_chunks_does_not_matter(engine, name, msb, in_bits, Lb, W):
    """one call of 20000 samples against calls of 4099 (rounded up to whole output bytes), one byte's samples and the rest, each
    handed only the input it needs; then the stream fed ragged chunks of bytes"""
    torch = nat.require_torch()
    fmt = requant.OutFormat(name, msb)
    case = (name, msb, in_bits, Lb, W, CUT_N)
    want, clipped, blocks, k = C.reference(*case)
    G, T = C.tables_for(fmt, Lb, W, in_bits)
    raw = C.signal(CUT_N, 5, in_bits).tobytes()
    per = 2 * in_bits // 8
    first = -(-4099 // fmt.unit) * fmt.unit
    with requant.Requantizer(engine, fmt, G, T, Lb, W, in_bits) as rq:
        parts, ks, m = [], [], 0
        for n in (first, fmt.unit, CUT_N - first - fmt.unit):
            lo, hi = requant.first_needed(Lb, W, m), max(m + n, W * Lb)
            out, kidx = rq.run(requant._device_bytes(engine, raw[per * lo:per * hi]), lo, m, n, trace=True)
            parts.append(_bytes(out))
            ks.append(kidx.cpu().numpy())
            m += n
        assert m == CUT_N and b"".join(parts) == want.tobytes()
        assert np.array_equal(np.concatenate(ks), k) and rq.stats() == (clipped, blocks)
    st = requant.Stream(engine, fmt, G, T, Lb, W, in_bits, trace=True)
    got, at = [], 0
    for n in list(FEED_CHUNKS) + [len(raw) - sum(FEED_CHUNKS)]:
        got.append(_bytes(st.feed(raw[at:at + n])))
        at += n
    assert at == len(raw) and st.next_out == CUT_N and b"".join(got) == want.tobytes()
    assert np.array_equal(torch.cat(st.indices).cpu().numpy(), k) and st.stats() == (clipped, blocks)
    st.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,in_bits,off", [("s8", 8, 1), ("u8", 16, 7), ("1ob", 8, 1), ("2sm", 16, 3), ("4tc", 8, 13), ("s16", 8, 2), ("s16", 16, 6), ("f32", 8, 8)])
def test_misaligned_buffers_and_starts_give_the_same_bytes(engine, name, in_bits, off):
    """the output `off` bytes into an allocation (guard bytes on both sides stay), the input one element in, and a first output sample
    that is no multiple of 16, so that a lane's run straddles block boundaries"""
    torch = nat.require_torch()
    dev = "cuda:%d" % engine.device
    Lb, W, n = 16, 3, 4099
    fmt = requant.OutFormat(name)
    want = C.reference(name, True, in_bits, Lb, W, n)[0]
    G, T = C.tables_for(fmt, Lb, W, in_bits)
    raw = np.frombuffer(C.signal(n, 5, in_bits).tobytes(), dtype=np.uint8)
    cfg = requant.make_cfg(fmt, Lb, W, len(G), in_bits)
    esz = in_bits // 8
    src = torch.zeros(len(raw) + 32, dtype=torch.uint8, device=dev)
    src[esz:esz + len(raw)] = torch.from_numpy(raw.copy()).to(dev)
    total = n // fmt.unit * fmt.unit
    for out_first in (0, 4 * fmt.unit + 4, 52):
        n_out = total - out_first
        nbytes = fmt.nbytes(n_out)
        out = torch.full((nbytes + 64,), 77, dtype=torch.uint8, device=dev)
        assert _raw_run(engine, cfg, G, T, src[esz:esz + len(raw)], 0, out_first, n_out, out, off=off) == 0
        hst = out.cpu().numpy()
        assert hst[off:off + nbytes].tobytes() == want[fmt.nbytes(out_first):].tobytes(), (name, out_first)
        assert (hst[:off] == 77).all() and (hst[off + nbytes:] == 77).all()


@pytest.mark.gpu
def test_more_blocks_than_one_pair_of_launches_takes(engine):
    """2^16 + 3 blocks of 16 samples and 5 samples more: the call is cut at block 2^16, on a byte of 2-bit codes"""
    Lb, W = 16, 3
    n = (C.CHUNK_BLOCKS + 3) * Lb + 5
    case = ("2ob", True, 8, Lb, W, n)
    want, clipped, blocks, k = C.reference(*case)
    G, T = C.tables_for("2ob", Lb, W)
    out, st, kidx = requant.convert(engine, "2ob", C.signal(n, 5), G, T, Lb, W, trace=True)
    assert _bytes(out) == want.tobytes() and st == (clipped, blocks) and np.array_equal(kidx.cpu().numpy(), k) and blocks == C.CHUNK_BLOCKS + 4


@pytest.mark.gpu
def test_every_refusal_through_the_raw_abi_leaves_the_output_untouched(engine):
    torch = nat.require_torch()
    engine.use_torch_stream()
    dev = "cuda:%d" % engine.device
    src = torch.ones(4096, dtype=torch.int8, device=dev)
    out = torch.full((4096,), 77, dtype=torch.int8, device=dev)
    stats = torch.zeros(2, dtype=torch.int64, device=dev)
    g = np.array([4.0, 2.0, 1.0, 0.5], dtype=np.float32)
    t = np.array([100, 200, 200], dtype=np.uint64)
    # what the configuration decides is refused when the handle is opened
    for label, code, change in bad_config_calls():
        gains = np.ascontiguousarray(change.get("gains", g), dtype=np.float32)
        thr = np.ascontiguousarray(change.get("thresholds", t), dtype=np.uint64)
        bits = change.get("bits", 0)
        e = list(change.get("enc") or range(min(1 << bits, 16)))
        st = requant.RequantCfg(in_bits=change.get("in_bits", 8), container=change.get("container", 0), bits=bits, msb_first=1, block=change.get("block", 64),
                                window=change.get("window", 3), ngains=change.get("K", 4), enc=(ctypes.c_uint8 * 16)(*(e + [0] * (16 - len(e)))))
        h = ctypes.c_void_p()
        rc = nat.lib.gacq_requant_open(engine._ctx, ctypes.addressof(st) if change.get("cfg", True) else None,
                                       None if change.get("null_gains") else ctypes.c_void_p(gains.ctypes.data),
                                       None if change.get("null_thr") else ctypes.c_void_p(thr.ctypes.data), ctypes.byref(h))
        assert rc == code and not h.value, (label, rc)
    st = requant.make_cfg("s8", 64, 3, 4)
    assert nat.lib.gacq_requant_open(engine._ctx, ctypes.addressof(st), ctypes.c_void_p(g.ctypes.data), ctypes.c_void_p(t.ctypes.data), None) == BAD_ARG
    handles = {}
    try:
        for name, in_bits in (("s8", 8), ("s16", 16), ("f32", 8), ("1ob", 8)):
            h = ctypes.c_void_p()
            st = requant.make_cfg(name, 64, 3, 4, in_bits)
            assert nat.lib.gacq_requant_open(engine._ctx, ctypes.addressof(st), ctypes.c_void_p(g.ctypes.data), ctypes.c_void_p(t.ctypes.data), ctypes.byref(h)) == 0
            handles[name] = h
        kw = dict(handle=handles["s8"], src=src.data_ptr(), dst=out.data_ptr(), stats=stats.data_ptr())
        for label, code, change in bad_run_calls():
            assert raw_check(**dict(kw, **change)) == code, (label, nat.lib.gacq_last_error(engine._ctx))
        assert b"need input samples" in nat.lib.gacq_last_error(engine._ctx)
        assert raw_check(**dict(kw, src=0)) == BAD_ARG and raw_check(**dict(kw, dst=0)) == BAD_ARG                  # NULL pointers
        assert raw_check(**dict(kw, stats=stats.data_ptr() + 4)) == BAD_ARG                                         # statistics off 8 bytes
        k16 = dict(kw, handle=handles["s16"])
        assert raw_check(**dict(k16, src=src.data_ptr() + 1)) == BAD_ARG and raw_check(**dict(k16, dst=out.data_ptr() + 1)) == BAD_ARG      # int16 off 2 bytes
        assert raw_check(**dict(kw, handle=handles["f32"], n_out=100, dst=out.data_ptr() + 4)) == BAD_ARG           # complex64 off 8 bytes
        for change in (dict(n_out=999), dict(out_first=2, n_out=996), dict(out_first=1, n_out=996)):               # 1-bit codes: four samples a byte
            assert raw_check(**dict(kw, handle=handles["1ob"], **change)) == BAD_ARG, change
        assert raw_check(**dict(kw, n_out=0)) == 0                                                                  # nothing to do
        torch.cuda.synchronize()
        assert bool((out == 77).all()) and stats.cpu().tolist() == [0, 0]
        assert raw_check(**kw) == 0                                                                                 # the unchanged call writes 2000 bytes
        torch.cuda.synchronize()
        hst = out.cpu().numpy()
        want = O.evaluate(O.cfg("s8", 64, 3), g, t, np.ones(2000, dtype=np.int8))                                   # S = 2 * 64 * 3 = 384: k = 3
        assert np.array_equal(hst[:2000].view(np.uint8), want[0]) and (hst[2000:] == 77).all() and stats.cpu().tolist() == [0, 16] and want[3].tolist() == [3] * 16
    finally:
        for h in handles.values():
            nat.lib.gacq_requant_close(h)


@pytest.mark.gpu
def test_command_line_file_in_file_out(tmp_path, engine):
    n = 50000
    raw = C.signal(n, 5).tobytes()
    src, dst, trace = str(tmp_path / "in.iq"), str(tmp_path / "out.2b"), str(tmp_path / "k.bin")
    with open(src, "wb") as f:
        f.write(raw)
    out = io.StringIO()
    lines = requant.run(["--format", "2sm", "--block", "256", "--window", "4", "--trace", trace, src, dst], out, piece_bytes=1 << 14)      # seven pieces
    assert out.getvalue().splitlines() == lines and len(lines) == 2
    fmt = requant.OutFormat("2sm")
    G, T = requant.tables(2.84, 256, 4)
    want = O.evaluate(C.ocfg(fmt, 256, 4), G, T, C.signal(n, 5))
    assert np.fromfile(dst, dtype=np.uint8).tobytes() == want[0].tobytes() and np.fromfile(trace, dtype=np.uint8).tobytes() == want[3].tobytes()
    assert lines == requant.report_lines(fmt, 256, 4, G, int(want[3].min()), int(want[3].max()), want[1], n)
    assert lines[1] == "ingest --format 2sm"
    # the file read back by ingest holds the levels
    back = ingest.convert(engine, ingest.Format("2sm"), np.fromfile(dst, dtype=np.uint8), 1.0).cpu().numpy()
    assert np.array_equal(back, O.levels_of_codes(C.ocfg(fmt, 256, 4), want[0]))
    # int16 in, one fixed gain, int8 out
    with open(src, "wb") as f:
        f.write(C.signal(n, 5, 16).tobytes())
    lines = requant.run(["--format", "s8", "--in-format", "s16", "--gain", "0.03125", src, dst], io.StringIO(), piece_bytes=1 << 16)
    want = O.evaluate(O.cfg("s8", 4096, 8, in_bits=16), [0.03125], [], C.signal(n, 5, 16))
    assert np.fromfile(dst, dtype=np.uint8).tobytes() == want[0].tobytes()
    assert lines[0] == "format s8 block 4096 window 8 gain 0.03125 .. 0.03125 clipped %d samples %d" % (want[1], n)


MS = 250
DWELLS = (20, 20)
SATS = [dict(tracker="gps-l1", item=7, amp=3.0, bit=20, doppler=1234.5, code0=417.37),
        dict(tracker="gps-l1", item=19, amp=3.0, bit=20, doppler=-1840.2, code0=88.71),
        dict(tracker="gps-l1", item=30, amp=3.0, bit=20, doppler=3071.9, code0=1001.13)]


def _code_error(got, want, L):
    return abs((got - want + L / 2.0) % L - L / 2.0)


def _handoff_and_track(engine, label, x, fs, coffset, noise_item=25):
    """test_handoff_gpu._check_channels on the int8 recording x, with that test's caps; the figures are printed before they are held"""
    items = [s["item"] for s in SATS] + [noise_item]
    results, refined, loop, x_dev = handoff.handoff("gps-l1", x, fs, coffset, items=items, loop_dwells=DWELLS, ms=80, engine=engine)
    try:
        assert [it for it, _ in refined] == items and loop.K == len(items)
        L = codes.code_length(trackloop.TRACKERS[handoff.tracker_name("gps-l1")].code)
        for s, (it, r), res in zip(SATS, refined, results):
            print("%s %d: acquired doppler %.1f code %.2f -> refined doppler error %.3f Hz, code error %.5f chip, ratio %.1f"
                  % (label, it, res[2], res[1], r.doppler - s["doppler"], _code_error(r.code_offset, s["code0"], L), r.ratio))
        for s, (it, r) in zip(SATS, refined):
            assert abs(r.doppler - s["doppler"]) <= 10.0, (label, it, r)
            assert _code_error(r.code_offset, s["code0"], L) <= 0.03, (label, it, r)
        recs = loop.run([x_dev] * loop.K)
        assert list(loop.status) == [0] * loop.K
    finally:
        loop.close()
    noise = float(np.mean(recs[-1]["prompt"][:200]))
    for s, r in zip(SATS, recs):
        assert len(r) >= 200
        print("  %s %d: carrier_f[199] error %.3f Hz, mean prompt %.1f, noise channel %.1f, ratio %.2f"
              % (label, s["item"], r["carrier_f"][199] - s["doppler"], np.mean(r["prompt"][:200]), noise, np.mean(r["prompt"][:200]) / noise))
    for s, r in zip(SATS, recs):
        assert abs(r["carrier_f"][199] - s["doppler"]) <= 10.0, (label, s, r["carrier_f"][199])
        assert np.mean(r["prompt"][:200]) > 3.0 * noise, (label, s, np.mean(r["prompt"][:200]), noise)


@pytest.mark.gpu
def test_pipeline_level_step_to_two_bits_to_tracking(engine):
    """simulate's three-satellite GPS L1 scene (test_simulate_gpu) at sigma 12; the second half scaled down 8 times on the device ->
    requant to 2sm with the default tables -> ingest -> handoff -> 200 ms of tracking, held to the caps of
    test_handoff_gpu.test_gps_l1_three_satellites unchanged; the same scene at its static gain straight into handoff is the yardstick."""
    torch = nat.require_torch()
    fs, coffset = 6.0e6, 250000.0
    n = int(fs * MS * 0.001)
    scene = []
    for i, s in enumerate(SATS):
        t = simulate.tracker(s["tracker"])
        periods = int(MS * 0.001 * codes.chip_rate(t.code) / codes.code_length(t.code)) + 2
        scene.append(simulate.Satellite(s["tracker"], s["item"], s["amp"], s["doppler"], s["code0"],
                                        symbols=simulate.symbols(s["tracker"], s["item"], -(-periods // s["bit"]), s["bit"], 100 + i)))
    x = simulate.recording(scene, fs, coffset, n, 31, 12.0, engine=engine)
    _handoff_and_track(engine, "static gain", x.cpu().numpy(), fs, coffset)
    stepped = x.clone()
    stepped[n:] = torch.round(stepped[n:].to(torch.float32) / 8.0).to(torch.int8)          # from sample n / 2 on
    fmt = requant.OutFormat("2sm")
    G, T = requant.tables(fmt.target_rms, requant.BLOCK, requant.WINDOW)
    packed, st, kidx = requant.convert(engine, fmt, stepped, G, T, trace=True)
    k = kidx.cpu().numpy()
    half = n // 2 // requant.BLOCK
    print("2sm: %d bytes, clipped %d of %d components, gain index %d before the step, %d after" % (packed.numel(), st[0], 2 * n, k[half - 1], k[-1]))
    # 8 times the gain is 24 steps of 2^(1/8); rounding the weak half to integers adds 1/12 to a variance of 2.25, 0.16 dB of a 0.75 dB step
    assert packed.numel() == n // 2 and k[half - 1] - k[-1] in (23, 24)
    y = ingest.convert(engine, ingest.Format("2sm"), packed, 10.0)                         # levels +-10, +-30
    _handoff_and_track(engine, "2 bits", y.cpu().numpy(), fs, coffset)
