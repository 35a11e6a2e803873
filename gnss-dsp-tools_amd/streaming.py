"""The host path that the recording converters share -- ingest, mitigate, ddc, requant, cancel, nulling, stap: each is a filter from
absolute input sample indices to absolute output sample indices ("the stream contract").  Here are the uploader, the chunk
state machine, the open device handle, the pointer conventions of a launch, the block / window algebra, the file pump and the
command-line shell; what a tool computes, its gacq_*_dev call, its parser and its report line stay in the tool's module (nulling and
stap share theirs in arrayfilter.py)."""
import contextlib
import ctypes
import math
import sys
import types

import numpy as np

from . import _native as nat


def device_flat(engine, data, dtypes, what, view=None):
    """A flat CUDA tensor whose torch dtype is one of `dtypes` (names), made contiguous, or a fresh upload of the bytes of a bytes-like
    object or numpy array to cuda:<engine.device>; anything else raises ValueError(what).  view: the dtype name to see it as."""
    torch = nat.require_torch()
    if torch.is_tensor(data):
        if not data.is_cuda or data.dim() != 1 or data.dtype not in [getattr(torch, t) for t in dtypes]:
            raise ValueError(what)
        d = data if data.is_contiguous() else data.contiguous()
    else:
        h = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data).reshape(-1).view(np.uint8)
        d = torch.from_numpy(np.array(h, copy=True)).to("cuda:%d" % engine.device)
    return d if view is None else d.view(getattr(torch, view))


class Chunks:
    """The chunk state machine: recordings fed piece by piece, so that the concatenation of what the calls return is what one call on
    the whole recordings gives.  It owns in_first (the absolute index of the first input sample of the kept tails), next_out (the next
    output sample: a number, or with `outputs` a list, one per output) and the tails: the input that a later output still needs and
    the bytes of a sample that a chunk cut.  A tool says how many bits an input sample takes and hands in three callables:
        supported(in_first, in_count)  the end of the outputs that inputs in_first .. in_first + in_count - 1 support (per output)
        launch(ds, in_first, in_count, out_first, n_out, k)  output k's samples out_first .. out_first + n_out - 1 from the whole
                                       samples ds, one flat tensor of bytes per input; what it returns is what feed returns -- for
                                       outputs that share one index range (beams) a list, one tensor per output, under one k
        needed(next_out)               the first input sample that the outputs from next_out on still need; for samples of less
                                       than a byte, on a byte boundary
    Any device's tensors will do: the machine only joins, cuts and clones them."""

    def __init__(self, sample_bits, supported, launch, needed, outputs=None, start=0):
        self.sample_bits, self._supported, self._launch, self._needed = int(sample_bits), supported, launch, needed
        self.in_first = int(start)
        self.next_out = int(start) if outputs is None else [int(start)] * outputs
        self._tails = None

    def feed_all(self, chunks):
        """chunks: one flat tensor of bytes per input, all of one length.  A list of the outputs' results, or the one result."""
        torch = nat.require_torch()
        ds = list(chunks)
        if self._tails is not None and self._tails[0].numel():
            ds = [torch.cat([t, d]) for t, d in zip(self._tails, ds)]
        in_count = ds[0].numel() * 8 // self.sample_bits
        whole = [d[:in_count * self.sample_bits // 8] for d in ds]
        single = not isinstance(self.next_out, list)
        nexts = [self.next_out] if single else self.next_out
        ends = self._supported(self.in_first, in_count)
        got = []
        for k, end in enumerate([ends] if single else ends):
            n_out = max(0, end - nexts[k])
            got.append(self._launch(whole, self.in_first, in_count, nexts[k], n_out, k))
            nexts[k] += n_out
        self.next_out = nexts[0] if single else nexts
        keep = max(self.in_first, min(self._needed(self.next_out), self.in_first + in_count))
        at = (keep - self.in_first) * self.sample_bits // 8
        self._tails = [d[at:].clone() for d in ds]
        self.in_first = keep
        return got[0] if single else got


def out_end(block, window, in_end, unit=1):
    """Blocks of `block` samples under a window of `window` blocks: the end of the outputs that a recording known up to input sample
    in_end - 1 supports -- all of it once W whole blocks are there, in whole groups of `unit` samples"""
    return in_end // unit * unit if in_end >= int(window) * int(block) else 0


def first_needed(block, window, out):
    """the first input sample that output `out` needs"""
    return max(out // int(block) - int(window), 0) * int(block)


def owned_blocks(block, out_first, n_out):
    """blocks that begin in out_first .. out_first + n_out - 1"""
    block = int(block)
    return max(0, -(-(out_first + n_out) // block) - -(-out_first // block)) if n_out > 0 else 0


class Handle:
    """The open device side of one configuration: _open() opens it and registers it with its engine, which closes what lives on its
    context; closed by close(), at the end of a with block or with the object.  A subclass names its gacq_*_close and itself."""
    _close, _what = None, "handle"

    def _open(self, engine, opener, *args, stats=False):
        self.engine, self._h = engine, None
        h = ctypes.c_void_p()
        nat.check(opener(engine._ctx, *args, ctypes.byref(h)), engine._ctx)
        self._h = h
        if stats:                                    # True: the two counters most tools keep; a number: that many
            torch = nat.require_torch()
            self._stats = torch.zeros(2 if stats is True else int(stats), dtype=torch.int64, device="cuda:%d" % engine.device)
        engine._live.add(self)

    def _check_open(self):
        if not self._h:
            raise ValueError("the %s is closed" % self._what)

    def stats(self):
        """(components the clip changed, blocks) over the runs so far"""
        c, b = self._stats.cpu().tolist()
        return int(c), int(b)

    def close(self):
        if getattr(self, "_h", None):
            getattr(nat.lib, self._close)(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def iq_out(n_out, dtype, device):
    """(complex64?, the output of n_out samples: a flat int8 tensor [2 n_out] of interleaved I/Q, or complex64 [n_out])"""
    torch = nat.require_torch()
    if dtype not in ("int8", "complex64"):
        raise ValueError("dtype must be 'int8' or 'complex64', not %r" % (dtype,))
    cplx = dtype == "complex64"
    return cplx, torch.empty(max(n_out, 0) * (1 if cplx else 2), dtype=torch.complex64 if cplx else torch.int8, device=device)


def launch(engine, ins, n_in, out, n_out, call):
    """The pointer conventions of a gacq_*_dev launch on torch's current stream: call(input addresses, output address) makes the
    library call.  A tensor without elements has no address to speak of: an input goes as that of an input that has some (0 when
    none has) and the output borrows it too, so that the call still makes its checks; only with neither input nor output (n_in and
    n_out both 0) is there no call."""
    if n_in or n_out:
        engine.use_torch_stream(ins[0].device)
        some = next((d.data_ptr() for d in ins if d.numel()), 0)
        call([d.data_ptr() if d.numel() else some for d in ins], out.data_ptr() if out.numel() else some)
    return out


def pump(pieces, start, fouts, per, window=0, size=len):
    """The file pump: start(held) is called once, with the pieces read so far, as soon as they measure `window` (or the input ends
    short of that), and returns feed; feed(piece) returns one tensor per file of fouts, whose bytes are written, for the held pieces and
    then for every further one.  `per`: tensor elements per sample.  The samples written per file, or None if no piece came.
    The automatic gains differ and stay as they are: ddc, nulling and stap give the window that holds their first 65536 outputs, so the gain
    does not depend on the piece size; ingest and mitigate give none and take the gain from the first piece, whatever it holds."""
    feed, held, n = None, [], [0] * len(fouts)

    def run(piece):
        for k, out in enumerate(feed(piece)):
            n[k] += out.numel() // per
            fouts[k].write(out.cpu().numpy().tobytes())

    for piece in pieces:
        if feed is not None:
            run(piece)
            continue
        held.append(piece)
        if sum(size(h) for h in held) >= window:
            feed = start(held)
            for h in held:
                run(h)
    if feed is None and held:
        feed = start(held)
        for h in held:
            run(h)
    return n if feed is not None else None


def positive_finite(v):
    return v > 0.0 and math.isfinite(v)


def positive_finite_fp32(v):
    """... and as the float32 that a kernel multiplies with"""
    return positive_finite(v) and positive_finite(float(np.float32(v)))


@contextlib.contextmanager
def shell(device, inputs, outputs, trace=None, report=None, stdin=True):
    """The files and the engine of a command line: `-` among the inputs is stdin (unless stdin is False) and as the one output stdout;
    the report then goes to stderr, else to stdout (or to `report`).  Yields .engine, .fins, .fouts, .ftrace and .report; on the way out
    the outputs are flushed, and on every way out the engine and the files are closed."""
    from . import acquire
    to_stdout = list(outputs) == ["-"]
    files, eng = [], None

    def opened(name, mode, std):
        if name == "-" and std is not None:
            return std
        files.append(open(name, mode))
        return files[-1]

    try:
        fins = [opened(name, "rb", sys.stdin.buffer if stdin else None) for name in inputs]
        fouts = [opened(name, "wb", sys.stdout.buffer if to_stdout else None) for name in outputs]
        ftrace = opened(trace, "wb", None) if trace else None
        eng = acquire.Engine(device)
        yield types.SimpleNamespace(engine=eng, fins=fins, fouts=fouts, ftrace=ftrace,
                                    report=(sys.stderr if to_stdout else sys.stdout) if report is None else report)
        for f in fouts:
            f.flush()
    finally:
        if eng is not None:
            eng.close()
        for f in files:
            f.close()


def main(argv, doc, run):
    argv = list(sys.argv[1:] if argv is None else argv)
    if not argv or argv[0] in ("-h", "--help"):
        print(doc)
        return 0
    run(argv)
    return 0
