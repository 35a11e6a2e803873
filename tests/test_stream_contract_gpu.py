"""GPU: the seven recording converters -- ingest, mitigate, ddc, requant, cancel, nulling, stap -- held to the stream contract of DESIGN.md 5.26
on the device, by one harness over the case table of tests/stream_contract_cases.py:

  far indices    every configuration in one call whose indices straddle 2^31, straddle 2^32 and end at the largest index its own
                 check accepts: equal to the oracle at those absolute indices under the tool's own comparison rule, and, where the
                 contract makes the output independent of the shift, bit for bit the near output of the same bytes;
  random cuts    16 drawn cut points and the forced ones at the tile and block edges, every piece a call of its own on exactly the
                 input that needed() names, at a drawn misalignment: the concatenation is the one-call result bit for bit and the
                 statistics sum to its; one sample fewer at either end of the input is refused and writes nothing;
  random chunks  the same recording through the tool's Chunks subclass in drawn byte chunks, empty ones among them;
  torch stream   the call behind a delayed producer on a side stream sees the producer's data, also when the engine's context was
                 left on another stream by the tool before.

The preconditions of the comparison rules are asserted on the CPU in test_stream_contract_cpu.py."""
import numpy as np
import pytest

import stream_contract_cases as S
from gnss_dsp_tools_amd import _native as nat
from gnss_dsp_tools_amd import acquire, spectrum

BASE_CALLS = [(c, b) for c in S.CASES for b in S.BASES]
# torch.cuda._sleep(SLEEP_CYCLES): the delay in front of the producer.  Measured with events on the MI355X: 10^6 cycles
# last 0.42 ms, so this is 42 ms, below the 100 ms the test may cost; the slowest one-call form of the table (mitigate with excision, both
# output forms, read back) takes 0.30 ms, a margin of 139 -- the margin also has to cover the host's time between enqueuing the delay
# and issuing the control clone, which 0.8 ms did not.
SLEEP_CYCLES = 100000000
_NEAR = {}


def _run_all(h, case, ds, in_first, out_first, n_out):
    return {dt: h.run(ds, in_first, out_first, n_out, dt) for dt in case.dtypes}


def _same(a, b, label):
    """two result()s, bit for bit"""
    assert a.out.dtype == b.out.dtype and a.out.shape == b.out.shape and a.out.tobytes() == b.out.tobytes(), label
    assert a.stats == b.stats and len(a.side) == len(b.side), (label, a.stats, b.stats)
    for x, y in zip(a.side, b.side):
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), label


def _device_accepts(engine, case):
    """accepts() of Case.far_end for a tool without a check entry: the call itself, on buffers that hold what it may read and write"""
    torch = nat.require_torch()
    lo, o, n, cnt = case.near_call()
    dev = "cuda:%d" % engine.device
    buf = torch.zeros((cnt + 64) * case.in_bits // 8 + 16, dtype=torch.uint8, device=dev)
    out = torch.zeros(2 * n + 64, dtype=torch.int8, device=dev)

    def accepts(in_first, in_count, out_first, n_out, shift):
        assert in_count <= cnt + 64 and n_out <= n
        engine.use_torch_stream()
        rc = case.raw(engine, None, [buf], in_first, in_count, out_first, n_out, out)
        assert rc in (0, S.BAD_ARG), (case.name, rc, nat.lib.gacq_last_error(engine._ctx))
        return rc == 0

    return accepts


def _calls_of(engine, case, base):
    """(label, out_first of the near call, shift, k or None) of a base"""
    if base == "far end":
        o, s = case.far_end(case.accepts if case.check is not None else _device_accepts(engine, case))
        return [("far end", o, s, None)]
    k = int(base[2:])
    return [("%s %s" % (base, what), None, s, k) for what, s in case.straddles(k)]


def test_the_table_covers_what_the_contract_names():
    """the coverage of this file, asserted: seven tools, three bases each, indices that cross 2^31 and 2^32, cuts at a tile edge and a
    block edge, empty chunks and a first chunk that yields nothing"""
    assert sorted(set(c.tool for c in S.CASES)) == sorted(S.TOOLS) and len(S.TOOLS) == 7
    assert S.BASES == ("2^31", "2^32", "far end") and all(sum(1 for c, b in BASE_CALLS if c.tool == t) >= 3 for t in S.TOOLS)
    for tool in S.TOOLS:
        cases = [c for c in S.CASES if c.tool == tool]
        for k in (31, 32):
            crossing = 0
            for c in cases:
                lo, o, n, cnt = c.near_call()
                for what, s in c.straddles(k):
                    a, b = (o + s, o + s + n - 1) if what == "out" else (lo + c.ratio * s, lo + c.ratio * s + cnt - 1)
                    crossing += a < 1 << k <= b
            assert crossing >= 1, (tool, k)
    for c in S.CASES:
        pts = c.cut_points()
        assert c.tile in pts and (c.block_edge is None or c.block_edge in pts), c.name
        sizes = c.chunk_sizes()
        assert 0 in sizes[1:] and any(a == 0 and b == 0 for a, b in zip(sizes, sizes[1:])) and max(c.ends(0, c.samples(sizes[0]))) == 0, c.name
    # the tools that count blocks cut at a block edge; ingest, ddc and the blank-only path have none, cancel's is its segment edge
    assert all(c.block_edge is not None for c in S.CASES if c.tool in ("requant", "nulling", "stap", "cancel")) and S.BY_NAME["mitigate-n128-blank"].block_edge
    assert all(c.block_edge == (c.W + 1) * c.Lb and c.shift_unit == c.Lb for c in S.CASES if c.tool in ("nulling", "stap"))


@pytest.mark.gpu
@pytest.mark.parametrize("case,base", BASE_CALLS, ids=lambda v: v if isinstance(v, str) else v.name)
def test_far_indices(engine, case, base):
    for label, o, s, k in _calls_of(engine, case, base):
        lo, o, n, cnt = case.near_call(o)
        data = case.cut(*case.needed(o, n))
        in_first, out_first = lo + case.ratio * s, o + s
        if k is not None:
            assert (out_first < 1 << k < out_first + n - 1) if label.endswith("out") else (in_first < 1 << k < in_first + cnt - 1)
        offs = case.offsets(1)[0]
        ds = [S.place(engine, d, int(r)) for d, r in zip(data, offs)]
        with case.open(engine, shift=s) as h:
            got = _run_all(h, case, ds, in_first, out_first, n)
        label = "%s %s: outputs %d .. %d from input %d" % (case.name, label, out_first, out_first + n - 1, in_first)
        case.compare(got, case.oracle(data, in_first, out_first, n, shift=s), label)
        if case.shift_unit is None:
            continue
        # the same bytes near zero, a check that does not pass through the oracle
        assert s % case.shift_unit == 0
        key = (case.name, o)
        if key not in _NEAR:
            with case.open(engine) as h:
                _NEAR[key] = _run_all(h, case, [S.place(engine, d) for d in data], lo, o, n)
        for dt in case.dtypes:
            _same(got[dt], _NEAR[key][dt], (label, dt, "against the near call"))


@pytest.mark.gpu
@pytest.mark.parametrize("case", S.CASES, ids=S.case_id)
def test_random_cuts_into_calls(engine, case):
    torch = nat.require_torch()
    N, pts = case.total(), case.cut_points()
    whole_data = list(case.recording())
    pieces = list(zip([0] + pts, pts + [N]))
    offs = case.offsets(len(pieces))
    with case.open(engine) as h:
        whole = _run_all(h, case, [S.place(engine, d) for d in whole_data], 0, 0, N)
        case.compare(whole, case.oracle(whole_data, 0, 0, N), case.name + " in one call")
        parts = {dt: [] for dt in case.dtypes}
        for (a, b), off in zip(pieces, offs):
            lo, end = case.needed(a, b - a)
            ds = [S.place(engine, d, int(r)) for d, r in zip(case.cut(lo, end), off)]
            assert all(d.data_ptr() % 256 == int(r) for d, r in zip(ds, off))
            for dt in case.dtypes:
                parts[dt].append(h.run(ds, lo, a, b - a, dt))
        for dt in case.dtypes:
            w, ps = whole[dt], parts[dt]
            assert np.concatenate([p.out for p in ps]).tobytes() == w.out.tobytes(), (case.name, dt)
            assert tuple(sum(p.stats[i] for p in ps) for i in range(len(w.stats))) == w.stats, (case.name, dt)
            for i, side in enumerate(w.side):
                assert np.concatenate([p.side[i] for p in ps]).tobytes() == side.tobytes(), (case.name, dt, i)
        # the support rule at its edge: the least that can be missing at the low end, one sample at the high end
        dev = "cuda:%d" % engine.device
        step = max(1, len(pieces) // S.EDGE_PIECES)
        tried = 0
        for a, b in pieces[::step][:S.EDGE_PIECES]:
            lo, end = case.needed(a, b - a)
            out = torch.full((16 * (b - a) + 64,), 77, dtype=torch.uint8, device=dev)
            short = case.low_short(a)
            ds = [S.place(engine, d) for d in case.cut(short, max(end, short + 16))]
            engine.use_torch_stream()
            rc = case.raw(engine, h, ds, short, max(0, end - short), a, b - a, out)
            assert rc == S.SHORT_INPUT, (case.name, a, b, "low end", rc, nat.lib.gacq_last_error(engine._ctx))
            ds = [S.place(engine, d) for d in case.cut(lo, end)]
            rc = case.raw(engine, h, ds, lo, end - lo - 1, a, b - a, out)
            assert rc == S.SHORT_INPUT, (case.name, a, b, "high end", rc, nat.lib.gacq_last_error(engine._ctx))
            assert case.raw(engine, h, ds, lo, end - lo, a, 0, out) == 0                         # nothing to do: accepted
            torch.cuda.synchronize()
            assert bool((out == 77).all()), (case.name, a, b)
            tried += 1
        assert tried == S.EDGE_PIECES


@pytest.mark.gpu
@pytest.mark.parametrize("case", S.CASES, ids=S.case_id)
def test_random_chunks_through_the_stream(engine, case):
    torch = nat.require_torch()
    rec, sizes = case.recording(), case.chunk_sizes()
    want_next = case.ends(0, case.n_in())
    for dt in case.dtypes:
        ref = case.stream_reference(engine, dt)
        st = case.stream(engine, dt)
        try:
            got, at, empties = [[] for _ in ref], 0, 0
            for i, n in enumerate(sizes):
                outs = st.feed([r[at:at + n].tobytes() for r in rec])
                at += n
                assert len(outs) == len(ref)
                for k, out in enumerate(outs):
                    assert torch.is_tensor(out) and out.is_cuda and out.dim() == 1 and out.dtype == case.torch_dtype(torch, dt), (case.name, dt, i)
                    got[k].append(out)
                    empties += out.numel() == 0
                if i == 0:
                    assert all(out.numel() == 0 for out in outs) and all(v == 0 for v in st.next_out())
            assert at == len(rec[0]) and empties >= 3 and st.next_out() == want_next, (case.name, dt, st.next_out(), want_next)
            for k, r in enumerate(ref):
                assert S.host(torch.cat(got[k])).tobytes() == r.out.tobytes(), (case.name, dt, k)
            if len(ref) == 1 and ref[0].stats:
                assert tuple(int(v) for v in st.stats()) == ref[0].stats, (case.name, dt)
            if hasattr(st, "side"):
                for x, y in zip(st.side(), ref[0].side):
                    assert x.tobytes() == y.tobytes(), (case.name, dt)
        finally:
            st.close()


# ---- torch's current stream
PROBE_CYCLES = 12000000                                          # 5 ms
_SIDE = []


def _waits(torch, busy, other):
    """does work on stream `other` wait for work on stream `busy`?  Streams that the runtime puts on one hardware queue do."""
    done, flag = torch.cuda.Event(), torch.cuda.Event()
    torch.cuda.synchronize()
    with torch.cuda.stream(busy):
        torch.cuda._sleep(PROBE_CYCLES)
        done.record()
    with torch.cuda.stream(other):
        torch.zeros(8, device="cuda:0").add_(1)
        flag.record()
    flag.synchronize()
    waited = done.query()
    torch.cuda.synchronize()
    return waited


def _side_streams():
    """Two side streams, chosen once and used by every test below: with torch's default stream they are the three streams of this
    file.  The runtime spreads streams over a few hardware queues, and two streams on one queue run in order whatever the program
    says: a tool that launched on a stale stream would then pass.  So the two are taken from torch's pool such that neither shares a
    queue with the default stream or with the other, which a 5 ms delay on one and a marker on the other show."""
    if not _SIDE:
        torch = nat.require_torch()
        default = torch.cuda.default_stream()
        for _ in range(16):
            c = torch.cuda.Stream()
            if all(not _waits(torch, x, c) and not _waits(torch, c, x) for x in [default] + _SIDE):
                _SIDE.append(c)
            if len(_SIDE) == 2:
                break
        assert len(_SIDE) == 2, "no two streams of torch's pool run independently of the default stream and of each other"
    return _SIDE


def _behind_a_delayed_producer(eng, case, h, base, side, before=None):
    """The recording is copied into a zeroed buffer on the side stream behind a delay, and the tool called on that stream: it must see
    the recording.  A clone of the buffer issued on the default stream right after the copy is the control: it must still hold zeros,
    or the delay was too short to prove anything."""
    torch = nat.require_torch()
    dev = "cuda:%d" % eng.device
    data = list(case.recording())
    src = [torch.from_numpy(d.copy()).to(dev) for d in data]
    bufs = [torch.zeros(len(d), dtype=torch.uint8, device=dev) for d in data]
    torch.cuda.synchronize()
    if before is not None:
        before()
    with torch.cuda.stream(side):
        torch.cuda._sleep(SLEEP_CYCLES)
        for b, s in zip(bufs, src):
            b.copy_(s, non_blocking=True)
        with torch.cuda.stream(torch.cuda.default_stream()):
            control = [b.clone() for b in bufs]
        got = _run_all(h, case, bufs, 0, 0, case.total())                                  # reads the results back, still on the side stream
    torch.cuda.synchronize()
    assert not any(bool(c.any()) for c in control), "%s: the delay was too short: the control clone already holds the recording" % case.name
    case.compare(got, case.oracle(data, 0, 0, case.total()), case.name + " on a side stream")
    for dt in case.dtypes:
        _same(got[dt], base[dt], (case.name, dt, "against the default stream"))


@pytest.mark.gpu
@pytest.mark.parametrize("case", [S.BY_NAME[n] for n in ("ingest-2sm-real", "mitigate-n128-blank", "ddc-d5-t3", "requant-2sm", "cancel-two-sats",
                                                         "nulling-m3-b128-w3", "stap-m3-t3-b128-w3")], ids=S.case_id)
def test_the_call_runs_on_torchs_current_stream(case):
    torch = nat.require_torch()
    side = _side_streams()[0]
    eng = acquire.Engine(0)                                      # a private engine: the shared one is never left on a side stream
    try:
        with case.open(eng) as h:
            base = _run_all(h, case, [S.place(eng, d) for d in case.recording()], 0, 0, case.total())
            _behind_a_delayed_producer(eng, case, h, base, side)
        torch.cuda.synchronize()
    finally:
        eng.close()


def _spectrum_first(eng, s1):
    """a tool that takes torch's stream through rawfile.device_int8, not through streaming.launch, run under a side stream of its own"""
    torch = nat.require_torch()
    x = torch.from_numpy(S.BY_NAME["cancel-two-sats"].recording()[0].view(np.int8).copy()).to("cuda:%d" % eng.device)
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        p = spectrum.psd_dev(x[:2 * 2048], 1024, 2, eng).cpu()
    assert p.shape == (1, 1024) and bool(torch.isfinite(p).all())


@pytest.mark.gpu
@pytest.mark.parametrize("first,second", [("spectrum", "ingest-s16-iq"), ("cancel-two-sats", "nulling-m2-b192-w2"), ("requant-u8", "mitigate-blank-only"),
                                          ("nulling-m3-b128-w3", "stap-m1-t15-b192-w2")])
def test_the_stream_the_last_tool_left_behind_does_not_stick(first, second):
    """tool A under side stream s1, then tool B under s2 behind its own delayed producer, on one engine: B sees its real input"""
    torch = nat.require_torch()
    s1, s2 = _side_streams()
    eng = acquire.Engine(0)
    try:
        b = S.BY_NAME[second]

        def run_first():
            if first == "spectrum":
                return _spectrum_first(eng, s1)
            a = S.BY_NAME[first]
            ds = [S.place(eng, d) for d in a.recording()]
            torch.cuda.synchronize()
            with torch.cuda.stream(s1):
                with a.open(eng) as ha:
                    got = _run_all(ha, a, ds, 0, 0, a.total())
            a.compare(got, a.oracle(list(a.recording()), 0, 0, a.total()), a.name + " first, on a side stream")

        with b.open(eng) as h:
            base = _run_all(h, b, [S.place(eng, d) for d in b.recording()], 0, 0, b.total())
            _behind_a_delayed_producer(eng, b, h, base, s2, before=run_first)
        torch.cuda.synchronize()
    finally:
        eng.close()
