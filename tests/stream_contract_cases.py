"""The case table of the device-side stream-contract tests (test_stream_contract_cpu.py, test_stream_contract_gpu.py): one adapter per
recording converter -- ingest, mitigate, ddc, requant, cancel, nulling, stap -- that gives a seeded recording, the module's one-call form, its
Chunks subclass, the oracle of tests/*_oracle.py with its comparison rule, and the oracle's needed / supported.  DESIGN.md 5.26 has the
contract; every seed, cut and chunk list below is drawn from numpy.random.Generator(PCG64([SEED, the case's seed, a purpose number])).

Every recording holds one workgroup tile plus a few blocks (or lane runs) plus an odd remainder, from sample 0.  A call is described by
(in_first, out_first, n_out) and is handed the bytes of needed(out_first, n_out) only.  A far call is a near call of the same bytes with
`shift` added to its output indices and ratio * shift to its input indices.

Named findings: none -- every case passed on the kernels as they were."""
import contextlib
import ctypes
import functools
import types

import numpy as np

import cancel_cases
import cancel_oracle
import ddc_cases
import ddc_oracle
import ingest_cases
import ingest_oracle
import mitigate_cases
import mitigate_oracle
import nulling_cases
import nulling_oracle
import requant_cases
import requant_oracle
import stap_cases
import stap_oracle
from gnss_dsp_tools_amd import _native as nat
from gnss_dsp_tools_amd import cancel, ddc, ingest, mitigate, nulling, requant, stap

SEED = 20261020
BAD_ARG, SHORT_INPUT = -1, -6
BASES = ("2^31", "2^32", "far end")
CHUNK_SET = (0, 1, 2, 3, 5, 64, 4097)            # and the rest
MAX_CHUNKS = 40
DRAWN_CUTS = 16
EDGE_PIECES = 8
FAKE_IN, FAKE_OUT = 1 << 20, 1 << 21              # addresses that a gacq_*_check only looks at


def result(out, stats=(), side=()):
    """what one call gives: the output (numpy), the statistics that add over calls, the per-block arrays that concatenate over calls"""
    return types.SimpleNamespace(out=out, stats=tuple(int(v) for v in stats), side=tuple(side))


def host(t):
    return t.cpu().numpy()


def place(engine, data, r=0):
    """the bytes on the device, the first one r bytes past a 256-byte boundary: a flat uint8 CUDA tensor"""
    torch = nat.require_torch()
    h = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
    buf = torch.empty(len(h) + 512, dtype=torch.uint8, device="cuda:%d" % engine.device)
    off = (-buf.data_ptr()) % 256 + r
    v = buf[off:off + len(h)]
    v.copy_(torch.from_numpy(h.copy()))
    return v


class Case:
    """What the tests need of one configuration of one tool.  Sample indices are absolute; `unit` divides every out_first and n_out,
    `ratio` input samples pass per output sample, `shift_unit` (outputs) is the shift under which the contract makes the output the
    same bytes (None: the tool carries a phase of the index), `near_first` the first output past every effect of sample 0."""
    tool = name = None
    seed = 0
    dtypes = ("int8", "complex64")
    in_bits = 16
    unit = ratio = inputs = chunk_unit = 1
    shift_unit = far_unit = None
    block_edge = None
    outputs = 1

    def rng(self, what):
        return np.random.Generator(np.random.PCG64([SEED, self.seed, what]))

    def samples(self, nbytes):
        return nbytes * 8 // self.in_bits

    @functools.lru_cache(maxsize=None)
    def n_in(self):
        return self.samples(len(self.recording()[0]))

    def total(self):
        """the outputs the whole recording supports"""
        return self.supported(0, self.n_in())

    def cut(self, lo, end):
        """the bytes of input samples lo .. end - 1 (lo on a byte boundary), one array per input"""
        assert (lo * self.in_bits) % 8 == 0
        return [r[lo * self.in_bits // 8:-(-end * self.in_bits // 8)] for r in self.recording()]

    def low_short(self, out_first):
        """the in_first of the call that lacks the least at the low end: one sample past the first one needed, or where a byte holds
        several samples the next byte boundary past it"""
        per = max(1, 8 // self.in_bits)
        return (self.first_needed(out_first) // per + 1) * per

    def forced_cuts(self):
        """the tile edge, the block edge past the warm-up, and one lane's run before and after each"""
        return sorted(e + d for e in (self.tile, self.block_edge) if e is not None for d in (-self.run_len, 0, self.run_len))

    def cut_points(self):
        """16 drawn from 1 .. N - 1 and the forced ones, moved down to multiples of `unit`"""
        N = self.total()
        pts = set(int(p) for p in self.rng(1).integers(1, N, size=DRAWN_CUTS)) | set(self.forced_cuts())
        return sorted(set(p // self.unit * self.unit for p in pts if 0 < p // self.unit * self.unit < N))

    def offsets(self, count):
        """r of 0 .. 15 per piece and input"""
        return self.rng(2).integers(0, 16, size=(count, self.inputs))

    def chunk_sizes(self):
        """byte counts that sum to the recording's: the first too short for any output, then drawn from CHUNK_SET (times chunk_unit)
        with two empty ones in a row, at most MAX_CHUNKS in all, the last one the rest"""
        rng, u, nbytes = self.rng(3), self.chunk_unit, len(self.recording()[0])
        first = u if max(self.ends(0, self.samples(u))) == 0 else 0
        sizes = [first] + [int(v) * u for v in rng.choice(CHUNK_SET, size=MAX_CHUNKS - 4)]
        at = int(rng.integers(1, 4))
        sizes[at:at] = [0, 0]
        out = []
        for s in sizes:
            if sum(out) + s >= nbytes:
                break
            out.append(s)
        return out + [nbytes - sum(out)]

    def ends(self, in_first, in_count):
        """supported() per output, as a list"""
        return [self.supported(in_first, in_count)]

    # ---- the far calls
    def near_call(self, out_first=None):
        """(in_first, out_first, n_out, in_count) of the call from near_first (or out_first) to the end of the recording"""
        o = self.near_first if out_first is None else out_first
        n = (self.total() - o) // self.unit * self.unit
        lo, end = self.needed(o, n)
        return lo, o, n, self.samples(len(self.cut(lo, end)[0]))

    def straddles(self, k):
        """the shifts that put 2^k inside the output range and, where the two differ, inside the input range of the near call"""
        lo, o, n, cnt = self.near_call()
        A = self.shift_unit or 1
        out = [("out", ((1 << k) - o - n // 2) // A * A)]
        if self.ratio != 1:
            out.append(("in", (((1 << k) - lo - cnt // 2) // self.ratio) // A * A))
        for what, s in out:
            if what == "out":
                assert o + s < 1 << k < o + s + n - 1, (self.name, k)
            else:
                assert lo + self.ratio * s < 1 << k < lo + self.ratio * s + cnt - 1, (self.name, k)
        return out

    def far_end(self, accepts):
        """(out_first of the near call, shift) of the call that lies as far out as accepts(in_first, in_count, out_first, n_out,
        shift) -> bool admits: the largest out_first whose call, handed what needed() names, is accepted, found by bisection.
        Asserts that this call is accepted and that the same call one sample further is not."""
        lo, o, n, cnt = self.near_call()

        def ok(first):
            a, e = self.needed(first, n)
            return accepts(a, e - a, first, n, first - o)

        assert ok(o) and not ok(o + (self.unit << 50))
        a, b = 0, 1 << 50                                        # ok(o + a unit), not ok(o + b unit)
        while b - a > 1:
            m = (a + b) // 2
            a, b = (m, b) if ok(o + m * self.unit) else (a, m)
        last = o + a * self.unit
        # the near call begins a little later, so that the shift is one of the contract's and needed() cuts the same bytes
        F = self.far_unit or self.shift_unit or 1
        lo2, o2, n2, cnt2 = self.near_call(o + (last - o) % F)
        s = last - o2
        assert s % F == 0 and lo2 + self.ratio * s == self.needed(last, n2)[0]
        assert accepts(lo2 + self.ratio * s, cnt2, last, n2, s)
        assert not accepts(lo2 + self.ratio * s + self.ratio, cnt2, last + 1, n2, s + 1)
        return o2, s

    def accepts(self, in_first, in_count, out_first, n_out, shift):
        """through the tool's gacq_*_check: accepted, or refused with GACQ_ERR_BAD_ARG"""
        rc = self.check(in_first, in_count, out_first, n_out, shift)
        assert rc in (0, BAD_ARG), (self.name, rc, nat.lib.gacq_last_error(None))
        return rc == 0

    def stream_reference(self, engine, dtype):
        """what one call on the whole recording gives, one result() per output of the stream"""
        ds = [place(engine, r) for r in self.recording()]
        with self.open(engine) as h:
            return [h.run(ds, 0, 0, self.total(), dtype)]

    # ---- what a subclass gives
    def open(self, engine, shift=0):
        """a context manager: the open device side, whose run(ds, in_first, out_first, n_out, dtype) gives a result()"""
        raise NotImplementedError

    def torch_dtype(self, torch, dtype):
        return torch.int8 if dtype == "int8" else torch.complex64


class _Runner:
    """run() of a tool that keeps nothing open"""

    def __init__(self, fn):
        self.run = fn

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        pass


def _same(a, b, label):
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), label


def _equal_forms(got, c64, i8, label):
    """both output forms equal to the oracle's, bit for bit"""
    _same(got["complex64"].out, c64, (label, "complex64"))
    _same(got["int8"].out, i8, (label, "int8"))


# ---------------------------------------------------------------------------------------------- ingest
class IngestCase(Case):
    tool = "ingest"
    tile, run_len = 2048, 8                                      # the real-IF kernel's tile; a workgroup of the I/Q kernel owns as many

    def __init__(self, name, fmt, real, gain, seed):
        self.name, self.seed, self.real, self.gain = name, seed, real, gain
        self.fmt, self.ofmt = ingest.Format(fmt, real=real), ingest_oracle.fmt(fmt, real=real)
        self.in_bits = self.fmt.sample_bits
        per = max(1, 8 // self.in_bits)                          # samples a byte
        self.ratio = 2 if real else 1
        # I/Q: any shift that keeps the input on a byte boundary; real IF: an even number of outputs, from output 11 on
        self.shift_unit = 2 if real else per
        self.near_first = 40 if real else 37                     # its input begins at sample 48, or 32
        self.far_unit = 8 if real else 16                        # needed() begins at multiples of 16 input samples
        self.align = per

    @functools.lru_cache(maxsize=None)
    def recording(self):
        n_out = self.tile + 5 * self.run_len + 37
        n_in = 2 * (n_out - 1) + ingest_oracle.HALF + 1 if self.real else n_out
        return (np.frombuffer(ingest_cases.raw(self.fmt.name, -(-n_in * self.in_bits // 8), SEED + self.seed), dtype=np.uint8),)

    def first_needed(self, out_first):
        return max(0, 2 * out_first - ingest_oracle.HALF) if self.real else out_first

    def needed(self, out_first, n_out):
        end = 2 * (out_first + n_out - 1) + ingest_oracle.HALF + 1 if self.real else out_first + n_out
        return self.first_needed(out_first) // 16 * 16, end      # from a multiple of 16 samples, a byte boundary in every format

    def supported(self, in_first, in_count):
        return sum(ingest_oracle.out_range(self.ofmt, in_first, in_count))

    def open(self, engine, shift=0):
        return _Runner(lambda ds, in_first, out_first, n_out, dtype: result(
            host(ingest.convert(engine, self.fmt, ds[0], self.gain, in_first, out_first, n_out, dtype))))

    def oracle(self, inputs, in_first, out_first, n_out, shift=0):
        return ingest_oracle.evaluate(self.ofmt, inputs[0].tobytes(), self.gain, in_first, out_first, n_out, "complex64")

    def compare(self, got, ref, label):
        _equal_forms(got, ref, ingest_oracle.to_int8(ref), label)

    def stream(self, engine, dtype):
        s = ingest.Ingest(engine, self.fmt, self.gain, dtype)
        return types.SimpleNamespace(feed=lambda chunks: [s.feed(chunks[0])], next_out=lambda: [s.next_out], stats=lambda: (), close=lambda: None)

    def raw(self, engine, h, ds, in_first, in_count, out_first, n_out, out):
        st = self.fmt.struct()
        return nat.lib.gacq_ingest_dev(engine._ctx, ctypes.addressof(st), ctypes.c_void_p(ds[0].data_ptr()), in_first, in_count, out_first, n_out, self.gain, 0,
                                       ctypes.c_void_p(out.data_ptr()))

    check = None                                                 # gacq_ingest_dev makes its checks itself, and only with a context


# ---------------------------------------------------------------------------------------------- mitigate
class MitigateCase(Case):
    tool = "mitigate"
    gain = mitigate_cases.GAIN

    def __init__(self, name, seed, **cfg):
        self.name, self.seed = name, seed
        self.ocfg = mitigate_oracle.config(**cfg)
        o = self.ocfg
        self.cfg = mitigate.Config(blank=o.blank, hold=o.hold, nfft=o.nfft, ratio=o.ratio if o.nfft else None, guard=o.guard)
        if o.nfft:
            h = o.nfft // 2
            self.tile, self.run_len, self.block_edge = mitigate_cases.TILE * h, 8, (mitigate_cases.TILE + 2) * h
            self.shift_unit, self.near_first = h, 2 * h + 5      # a multiple of the frame hop; block 2 needs no sample below 0
        else:
            self.tile, self.run_len = 2048, 8                    # the blank-only kernel: 256 lanes of 8 outputs
            self.shift_unit, self.near_first = 1, o.hold + 7

    @functools.lru_cache(maxsize=None)
    def recording(self):
        o = self.ocfg
        if o.nfft:
            h = o.nfft // 2
            n = mitigate_oracle.needed(o, 0, self.tile + 5 * h + 37)[1] + 1 + 5
            x = mitigate_cases.tones(n, o.nfft, SEED + self.seed, False).copy()
            for m in (0, 3 * h - 1, self.tile - 1, self.tile + 2, self.tile + 4 * h + 9):      # pulses whose holds cross a block and the tile edge
                x[2 * m], x[2 * m + 1] = -100, 100
        else:
            n = self.tile + 5 * self.run_len + 37 + o.hold
            x = mitigate_cases.pulses(n, SEED + self.seed, False, extra=(self.tile - 1, self.tile, self.tile + 1, 700))
        return (x.view(np.uint8),)

    def first_needed(self, out_first):
        return mitigate_oracle.needed(self.ocfg, out_first, 1)[0]

    def needed(self, out_first, n_out):
        lo, hi = mitigate_oracle.needed(self.ocfg, out_first, n_out)
        return lo, hi + 1

    def supported(self, in_first, in_count):
        return sum(mitigate_oracle.out_range(self.ocfg, in_first, in_count))

    def open(self, engine, shift=0):
        def run(ds, in_first, out_first, n_out, dtype):
            out, st = mitigate.apply(engine, self.cfg, ds[0], self.gain, in_first, out_first, n_out, dtype, True)
            return result(host(out), (st.blanked, st.frames, st.bins), (st.frame_bins,))
        return _Runner(run)

    def oracle(self, inputs, in_first, out_first, n_out, shift=0):
        """(fp64 result, value bound relative to max |y|, max |y|): the bound is four times the deviation of the float32 evaluation of
        the definition, as in mitigate_cases.case_reference"""
        data = inputs[0].view(np.int8)
        ref = mitigate_oracle.evaluate(self.ocfg, data, self.gain, False, in_first, out_first, n_out)
        if not self.ocfg.nfft:
            return ref, 0.0, 0.0
        f32 = mitigate_oracle.evaluate(self.ocfg, data, self.gain, False, in_first, out_first, n_out, precision="f32")
        top = float(np.max(np.abs(ref.y)))
        assert np.array_equal(f32.frame_bins, ref.frame_bins)
        return ref, 4.0 * float(np.max(np.abs(f32.y - ref.y))) / top, top, f32

    def compare(self, got, ref, label):
        r = ref[0]
        for g in got.values():
            assert g.stats == (r.blanked, r.frames, r.bins) and np.array_equal(g.side[0], r.frame_bins), (label, g.stats)
        if not self.ocfg.nfft:                                   # the blank-only path: bit for bit
            _equal_forms(got, r.c64, r.i8, label)
            return
        from test_mitigate_gpu import _hold_to_the_oracle        # the excision path: the rule of test_mitigate_gpu, unchanged
        st = types.SimpleNamespace(blanked=r.blanked, frames=r.frames, bins=r.bins, frame_bins=got["int8"].side[0])
        _hold_to_the_oracle(label, got["complex64"].out, got["int8"].out, st, r, ref[1], ref[2])

    def stream(self, engine, dtype):
        s = mitigate.Mitigate(engine, self.cfg, self.gain, dtype)
        return types.SimpleNamespace(feed=lambda chunks: [s.feed(chunks[0])], next_out=lambda: [s.next_out],
                                     stats=lambda: (s.blanked, s.frames, s.bins), close=lambda: None)

    def _args(self, src, in_first, in_count, out_first, n_out, dst):
        c = self.cfg.struct()
        return c, [ctypes.addressof(c), ctypes.c_void_p(src), 0, in_first, in_count, out_first, n_out, self.gain, 0, ctypes.c_void_p(dst)]

    def raw(self, engine, h, ds, in_first, in_count, out_first, n_out, out):
        c, a = self._args(ds[0].data_ptr(), in_first, in_count, out_first, n_out, out.data_ptr())
        return nat.lib.gacq_mitigate_dev(engine._ctx, *a, None, None)

    def check(self, in_first, in_count, out_first, n_out, shift=0):
        c, a = self._args(FAKE_IN, in_first, in_count, out_first, n_out, FAKE_OUT)
        return nat.lib.gacq_mitigate_check(*a)


# ---------------------------------------------------------------------------------------------- ddc
class DdcCase(Case):
    tool = "ddc"
    gain, fs, run_len = ddc_cases.GAIN, ddc_cases.FS, 4
    near_first = 7

    def __init__(self, name, seed, D, T, f_shift, second):
        self.name, self.seed, self.D, self.T, self.f_shift = name, seed, D, T, f_shift
        self.taps = ddc_oracle.design_taps(D, T)
        self.band = ddc.Band(f_shift, D, taps=self.taps)
        self.ratio, self.tile = D, ddc_cases.tile(D)
        D2, T2, f2 = second                                      # the second band of the Splitter
        self.second = types.SimpleNamespace(D=D2, T=T2, f_shift=f2, taps=ddc_oracle.design_taps(D2, T2))
        self.second.band = ddc.Band(f2, D2, taps=self.second.taps)
        self.outputs = 2

    @functools.lru_cache(maxsize=None)
    def recording(self):
        n = ddc_oracle.needed(self.D, self.T, 0, self.tile + 5 * self.run_len + 37)[1] + 1 + 3
        return (ddc_cases.random_int8(n, SEED + self.seed).view(np.uint8),)

    def first_needed(self, out_first):
        return ddc_oracle.needed(self.D, self.T, out_first, 1)[0]

    def needed(self, out_first, n_out):
        lo, hi = ddc_oracle.needed(self.D, self.T, out_first, n_out)
        return lo, hi + 1

    def supported(self, in_first, in_count):
        return sum(ddc_oracle.out_range(self.D, self.T, in_first, in_count))

    def ends(self, in_first, in_count):
        return [self.supported(in_first, in_count), sum(ddc_oracle.out_range(self.second.D, self.second.T, in_first, in_count))]

    @contextlib.contextmanager
    def open(self, engine, shift=0, band=None):
        with ddc.Converter(engine, band or self.band, self.fs) as conv:
            r = _Runner(lambda ds, in_first, out_first, n_out, dtype: result(host(conv.run(ds[0], in_first, out_first, n_out, self.gain, dtype))))
            r.handle = conv._h
            yield r

    def oracle(self, inputs, in_first, out_first, n_out, shift=0, b=None):
        b = b or self
        return ddc_oracle.evaluate(b.f_shift, self.fs, b.D, b.taps, inputs[0].tobytes(), self.gain, in_first, out_first, n_out, "complex64")

    def compare(self, got, ref, label):
        _equal_forms(got, ref, ddc_oracle.to_int8(ref), label)

    def stream_reference(self, engine, dtype):
        ds = [place(engine, self.recording()[0])]
        out = []
        for band, end in zip((None, self.second.band), self.ends(0, self.n_in())):
            with self.open(engine, band=band) as h:
                out.append(h.run(ds, 0, 0, end, dtype))
        return out

    def stream(self, engine, dtype):
        s = ddc.Splitter(engine, [self.band, self.second.band], self.fs, [self.gain, self.gain], dtype)
        return types.SimpleNamespace(feed=lambda chunks: s.feed(chunks[0]), next_out=lambda: list(s.next_out), stats=lambda: (), close=s.close)

    def raw(self, engine, h, ds, in_first, in_count, out_first, n_out, out):
        return nat.lib.gacq_ddc_run_dev(h.handle, ctypes.c_void_p(ds[0].data_ptr()), in_first, in_count, out_first, n_out, self.gain, 0, ctypes.c_void_p(out.data_ptr()))

    def check(self, in_first, in_count, out_first, n_out, shift=0):
        c = ddc.DdcCfg(dphase=self.band.dphase(self.fs), decim=self.D)
        g = np.ascontiguousarray(self.taps, dtype=np.int32)
        return nat.lib.gacq_ddc_check(ctypes.addressof(c), ctypes.c_void_p(g.ctypes.data), len(g), in_first, in_count, out_first, n_out, self.gain, 0)


# ---------------------------------------------------------------------------------------------- requant
class RequantCase(Case):
    tool = "requant"
    dtypes = ("bytes",)
    Lb, W = 64, 3
    tile = 16384

    def __init__(self, name, fmt, seed):
        self.name, self.seed = name, seed
        self.fmt = requant.OutFormat(fmt)
        self.ocfg = requant_cases.ocfg(self.fmt, self.Lb, self.W)
        self.G, self.T = requant_cases.tables_for(self.fmt, self.Lb, self.W)
        self.unit = self.fmt.unit
        self.run_len = 16 * 8 // self.fmt.sample_bits           # samples in a lane's 16 output bytes
        self.block_edge = (self.W + 1) * self.Lb
        self.shift_unit, self.near_first = self.Lb, (self.W + 1) * self.Lb + 10

    @functools.lru_cache(maxsize=None)
    def recording(self):
        return (requant_cases.signal(self.tile + 5 * self.Lb + 37, SEED % 100000 + self.seed).view(np.uint8),)

    def first_needed(self, out_first):
        return requant_oracle.needed(self.ocfg, out_first, 1)[0]

    def needed(self, out_first, n_out):
        return requant_oracle.needed(self.ocfg, out_first, n_out)

    def supported(self, in_first, in_count):
        return requant_oracle.supported(self.ocfg, in_first, in_count)

    @contextlib.contextmanager
    def open(self, engine, shift=0):
        with requant.Requantizer(engine, self.fmt, self.G, self.T, self.Lb, self.W) as rq:
            seen = [0, 0]                                        # the handle's totals after the last run: nothing is read before a launch

            def run(ds, in_first, out_first, n_out, dtype):
                out, kidx = rq.run(ds[0], in_first, out_first, n_out, trace=True)
                after = rq.stats()
                st = (after[0] - seen[0], after[1] - seen[1])
                seen[:] = after
                return result(host(out), st, (host(kidx),))
            r = _Runner(run)
            r.handle = rq._h
            yield r

    def oracle(self, inputs, in_first, out_first, n_out, shift=0):
        return requant_oracle.evaluate(self.ocfg, self.G, self.T, inputs[0].view(np.int8), out_first, n_out, in_first)

    def compare(self, got, ref, label):
        g = got["bytes"]
        assert g.out.tobytes() == ref[0].tobytes(), label
        assert g.stats == (ref[1], ref[2]) and np.array_equal(g.side[0], ref[3]), (label, g.stats, ref[1:3])

    def torch_dtype(self, torch, dtype):
        return self.fmt.torch_dtype(torch)

    def stream(self, engine, dtype):
        torch = nat.require_torch()
        s = requant.Stream(engine, self.fmt, self.G, self.T, self.Lb, self.W, trace=True)
        return types.SimpleNamespace(feed=lambda chunks: [s.feed(chunks[0])], next_out=lambda: [s.next_out], stats=s.stats, close=s.close,
                                     side=lambda: (host(torch.cat(s.indices)),))

    def raw(self, engine, h, ds, in_first, in_count, out_first, n_out, out):
        return nat.lib.gacq_requant_run_dev(h.handle, ctypes.c_void_p(ds[0].data_ptr()), in_first, in_count, out_first, n_out, ctypes.c_void_p(out.data_ptr()),
                                            None, None)

    def check(self, in_first, in_count, out_first, n_out, shift=0):
        c = requant.make_cfg(self.fmt, self.Lb, self.W, len(self.G))
        return nat.lib.gacq_requant_check(ctypes.addressof(c), ctypes.c_void_p(self.G.ctypes.data), ctypes.c_void_p(self.T.ctypes.data), in_first, in_count,
                                          out_first, n_out)


# ---------------------------------------------------------------------------------------------- cancel
class CancelCase(Case):
    tool = "cancel"
    fs = 4.092e6
    tile, run_len = 2048, 8
    block_edge = 1211                                            # the segment edge inside the range
    near_first = 5

    def __init__(self, name, seed):
        self.name, self.seed = name, seed
        self.sats = [cancel.Sat("gps.ca", 5, 0), cancel.Sat("galileo.e1b", 2, 2)]
        S, G = cancel_cases.seg, cancel_cases.segs
        self.segs = [G(S(11, 1200, 2500.0, 0.25, 1.023e6 + 1.6, 1000.5, 10.0 - 3.0j), S(1211, 900, 2501.0, 0.6, 1.023e6 + 1.6, 1000.9, -4.0 + 9.0j)),
                     G(S(500, 1500, -1200.0, 0.0, 1.023e6, 4000.0, 6.0j))]

    def shifted(self, shift):
        out = []
        for g in self.segs:
            g = g.copy()
            g["s0"] += shift
            out.append(g)
        return out

    @functools.lru_cache(maxsize=None)
    def recording(self):
        return (cancel_cases.noise_int8(self.tile + 5 * self.run_len + 37, SEED + self.seed).view(np.uint8),)

    def first_needed(self, out_first):
        return out_first

    def needed(self, out_first, n_out):
        return out_first, out_first + n_out

    def supported(self, in_first, in_count):
        return in_first + in_count

    def open(self, engine, shift=0, estimate=False):
        def run(ds, in_first, out_first, n_out, dtype):
            out, amps, clipped = cancel.apply(engine, self.sats, self.shifted(shift), self.fs, ds[0], in_first, out_first, n_out, estimate, dtype)
            return result(host(out), (clipped,))
        return _Runner(run)

    def oracle(self, inputs, in_first, out_first, n_out, shift=0):
        """(fp64 v, the numpy float32 evaluation): four times their distance is the bound, as in test_cancel_gpu"""
        x = cancel_cases.as_complex(inputs[0].view(np.int8), False)
        sats = [cancel_cases.oracle_sat(s) for s in self.sats]
        amps = [(g["amp_re"] + 1j * g["amp_im"]).astype(np.complex128) for g in self.segs]
        return tuple(cancel_oracle.evaluate(sats, self.shifted(shift), amps, self.fs, x, in_first, out_first, n_out, f32=f) for f in (False, True))

    def compare(self, got, ref, label):
        want, f32 = ref
        c, i = got["complex64"], got["int8"]
        scale = float(np.max(np.abs(want)))
        dev32, err = float(np.max(np.abs(f32 - want))) / scale, float(np.max(np.abs(c.out - want))) / scale
        print("%s: numpy float32 deviation %.3g  bound %.3g  device %.3g" % (label, dev32, 4 * dev32, err))
        assert c.out.dtype == np.complex64 and c.out.shape == want.shape and err <= 4 * dev32, (label, err, dev32)
        assert np.array_equal(i.out, cancel_oracle.to_int8(c.out)), label
        assert c.stats == (0,) and i.stats == (cancel_oracle.clip_count(i.out),), label

    def stream_reference(self, engine, dtype):
        """with estimated amplitudes, as the Canceller has them"""
        with self.open(engine, estimate=True) as h:
            return [h.run([place(engine, self.recording()[0])], 0, 0, self.total(), dtype)]

    def stream(self, engine, dtype):
        s = cancel.Canceller(engine, self.sats, self.segs, self.fs, True, dtype)
        return types.SimpleNamespace(feed=lambda chunks: [s.feed(chunks[0])], next_out=lambda: [s.next_out], stats=lambda: (s.clipped,), close=lambda: None)

    def _args(self, shift, src, in_first, in_count, out_first, n_out, dst):
        arr, flat, _ = cancel._sat_structs(self.sats, self.shifted(shift))
        return (arr, flat), [ctypes.addressof(arr), len(arr), ctypes.c_void_p(flat.ctypes.data), self.fs, 0, ctypes.c_void_p(src), 0, in_first, in_count,
                             out_first, n_out, 0, ctypes.c_void_p(dst)]

    def raw(self, engine, h, ds, in_first, in_count, out_first, n_out, out):
        keep, a = self._args(0, ds[0].data_ptr(), in_first, in_count, out_first, n_out, out.data_ptr())
        return nat.lib.gacq_cancel_dev(engine._ctx, *a, None, None)

    def check(self, in_first, in_count, out_first, n_out, shift=0):
        keep, a = self._args(shift, FAKE_IN, in_first, in_count, out_first, n_out, FAKE_OUT)
        return nat.lib.gacq_cancel_check(*a)


# ---------------------------------------------------------------------------------------------- nulling
class NullingCase(Case):
    tool = "nulling"
    gain, load_shift = 2.5, 10
    tile, run_len = nulling_cases.TILE, nulling_cases.RUN
    chunk_unit = 2                                               # nulling.Stream.feed takes whole samples by its contract

    def __init__(self, name, seed, M, Lb, W):
        self.name, self.seed, self.M, self.Lb, self.W = name, seed, M, Lb, W
        self.inputs = M
        self.block_edge = (W + 1) * Lb
        self.shift_unit, self.near_first = Lb, (W + 1) * Lb + 5

    @functools.lru_cache(maxsize=None)
    def recording(self):
        return tuple(x.view(np.uint8) for x in nulling_cases.recording(self.M, self.tile + 5 * self.Lb + 37, self.seed))

    def first_needed(self, out_first):
        return nulling_oracle.needed(self.Lb, self.W, out_first, 1)[0]

    def needed(self, out_first, n_out):
        return nulling_oracle.needed(self.Lb, self.W, out_first, n_out)

    def supported(self, in_first, in_count):
        return nulling_oracle.supported(self.Lb, self.W, in_first, in_count)

    def _handle(self, engine):
        return nulling.Nuller(engine, self.M, self.Lb, self.W, self.load_shift)

    @contextlib.contextmanager
    def open(self, engine, shift=0):
        torch = nat.require_torch()
        with self._handle(engine) as nl:
            seen = [0, 0]                                        # the handle's totals after the last run: nothing is read before a launch

            def run(ds, in_first, out_first, n_out, dtype):
                out, wq, cov = nl.run([d.view(torch.int8) for d in ds], in_first, out_first, n_out, self.gain, dtype, weights=True, cov=True)
                after = nl.stats()
                st = (after[0] - seen[0], after[1] - seen[1])
                seen[:] = after
                return result(host(out), st, (host(wq), host(cov)))
            r = _Runner(run)
            r.handle = nl._h
            yield r

    def oracle(self, inputs, in_first, out_first, n_out, shift=0):
        xs = [x.view(np.int8) for x in inputs]
        return {dt: nulling_oracle.run(xs, in_first, out_first, n_out, self.Lb, self.W, self.load_shift, None, self.gain, dt == "complex64") for dt in self.dtypes}

    def compare(self, got, ref, label):
        for dt, g in got.items():
            r = ref[dt]
            assert g.out.tobytes() == r["out"].tobytes(), (label, dt)
            assert g.stats == (r["clipped"], r["owned"]), (label, dt, g.stats)
            assert np.array_equal(g.side[1], r["cov"]) and g.side[0].dtype == np.int32 and np.array_equal(g.side[0], r["wq"]), (label, dt)

    def stream(self, engine, dtype):
        torch = nat.require_torch()
        s = nulling.Stream(engine, self.M, self.gain, self.Lb, self.W, self.load_shift, None, dtype, weights=True)
        return types.SimpleNamespace(feed=lambda chunks: [s.feed(chunks)], next_out=lambda: [s.next_out], stats=s.stats, close=s.close,
                                     side=lambda: (host(torch.cat(s.traces)),))

    def raw(self, engine, h, ds, in_first, in_count, out_first, n_out, out):
        ptrs = (ctypes.c_void_p * self.M)(*[d.data_ptr() for d in ds])
        return nat.lib.gacq_null_run_dev(h.handle, ctypes.cast(ptrs, ctypes.c_void_p), in_first, in_count, out_first, n_out, self.gain, 0,
                                         ctypes.c_void_p(out.data_ptr()), None, None, None)

    def check(self, in_first, in_count, out_first, n_out, shift=0):
        c = nulling.make_cfg(self.M, self.Lb, self.W, self.load_shift)
        return nat.lib.gacq_null_check(ctypes.addressof(c), in_first, in_count, out_first, n_out, self.gain, 0)


# ---------------------------------------------------------------------------------------------- stap
class StapCase(NullingCase):
    """nulling's adapter with T taps on every antenna: t_c = (T - 1) / 2 samples more at either end of the input, N = M T weights a
    block; the comparison rule is NullingCase.compare, that of test_stap_gpu.py.  The recordings are those of stap_cases "long"."""
    tool = "stap"
    tile, run_len = stap_cases.TILE, stap_cases.RUN

    def __init__(self, name, long_name):
        M, T, Lb, W, seed, kind = stap_cases.CASES[long_name]
        assert kind == "long"
        NullingCase.__init__(self, name, seed, M, Lb, W)
        self.T, self.long_name = T, long_name

    def recording(self):
        return tuple(x.view(np.uint8) for x in stap_cases.data(self.long_name))

    def first_needed(self, out_first):
        return stap_oracle.needed(self.Lb, self.W, self.T, out_first, 1)[0]

    def needed(self, out_first, n_out):
        return stap_oracle.needed(self.Lb, self.W, self.T, out_first, n_out)

    def supported(self, in_first, in_count):
        return stap_oracle.supported(self.Lb, self.W, self.T, in_first, in_count)

    def _handle(self, engine):
        return stap.Stap(engine, self.M, self.T, self.Lb, self.W, self.load_shift)

    def oracle(self, inputs, in_first, out_first, n_out, shift=0):
        xs = [x.view(np.int8) for x in inputs]
        return {dt: stap_oracle.run(xs, in_first, out_first, n_out, self.Lb, self.W, self.T, self.load_shift, None, self.gain, dt == "complex64")
                for dt in self.dtypes}

    def stream(self, engine, dtype):
        torch = nat.require_torch()
        s = stap.Stream(engine, self.M, self.gain, self.T, self.Lb, self.W, self.load_shift, None, dtype, weights=True)
        return types.SimpleNamespace(feed=lambda chunks: [s.feed(chunks)], next_out=lambda: [s.next_out], stats=s.stats, close=s.close,
                                     side=lambda: (host(torch.cat(s.traces)),))

    def raw(self, engine, h, ds, in_first, in_count, out_first, n_out, out):
        ptrs = (ctypes.c_void_p * self.M)(*[d.data_ptr() for d in ds])
        return nat.lib.gacq_stap_run_dev(h.handle, ctypes.cast(ptrs, ctypes.c_void_p), in_first, in_count, out_first, n_out, self.gain, 0,
                                         ctypes.c_void_p(out.data_ptr()), None, None, None)

    def check(self, in_first, in_count, out_first, n_out, shift=0):
        c = stap.make_cfg(self.M, self.T, self.Lb, self.W, self.load_shift)
        return nat.lib.gacq_stap_check(ctypes.addressof(c), in_first, in_count, out_first, n_out, self.gain, 0)


# the seeds of the mitigate and nulling cases were chosen here, on the CPU, so that the preconditions of their comparison rules hold
# (test_stream_contract_cpu.py asserts them): the excision decisions keep 1e-4 from their thresholds, the scaled weights 1e-6 from a
# rounding tie; the stap cases take the "long" recordings of stap_cases, whose seeds (80, 82) were chosen there by the same rule
CASES = [
    IngestCase("ingest-2sm-real", "2sm", True, ingest_cases.REAL_GAIN["2sm"], 1),
    IngestCase("ingest-1ob-iq", "1ob", False, ingest_cases.IQ_GAIN["1ob"], 2),
    IngestCase("ingest-s16-iq", "s16", False, ingest_cases.IQ_GAIN["s16"], 3),
    MitigateCase("mitigate-n128-blank", 11, blank=100.0, hold=3, nfft=128, ratio=12.0, guard=2),
    MitigateCase("mitigate-blank-only", 12, blank=mitigate_cases.BLANK_THR, hold=2, nfft=0),
    DdcCase("ddc-d5-t3", 21, 5, 3, ddc_cases.SHIFTS[2], second=(3, 25, ddc_cases.SHIFTS[1])),
    RequantCase("requant-u8", "u8", 31),
    RequantCase("requant-2sm", "2sm", 32),
    CancelCase("cancel-two-sats", 41),
    NullingCase("nulling-m3-b128-w3", 51, 3, 128, 3),
    NullingCase("nulling-m2-b192-w2", 52, 2, 192, 2),
    StapCase("stap-m3-t3-b128-w3", "long-m3-t3-b128-w3"),
    StapCase("stap-m1-t15-b192-w2", "long-m1-t15-b192-w2"),
]
TOOLS = ("ingest", "mitigate", "ddc", "requant", "cancel", "nulling", "stap")
BY_NAME = {c.name: c for c in CASES}


def case_id(c):
    return c.name
