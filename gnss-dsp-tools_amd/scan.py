"""Acquisition along a whole recording: the acquire command at many file positions in one pass.

    python -m gnss_dsp_tools_amd.scan gps-l1 [--prn 1-32] [--doppler-search MIN,MAX,INCR] [--time MS] [--every T_MS] [--skip MS]
           [--epochs E] [--min-metric X] [--device D] FILE FS COFFSET

Epoch e = 0, 1, ... is the window of n_in = int(FS*0.001*(MS+5)) complex samples that starts at sample s_e = int(FS*0.001*T_MS*e)
(after --skip MS: int(FS*0.001*SKIP) samples further on), and its result is what ``python -m gnss_dsp_tools_amd.cli <signal>`` prints,
with the same options, for the file that begins at byte 2*s_e: the mixer phase restarts at 0, filtfilt extends the window on its own,
np.interp resamples it to MS+5 ms at the signal's rate.  Windows may overlap or leave gaps; the last epoch is the last one whose window
lies wholly inside the recording.  One line per epoch and item:

    epoch <e> start <s_e> <the acquire command's line>

The reference handles one file position per process run (acquire-gps-l1.py:80-108).  Here the windows of a piece of the recording go
through one batched front-end (gacq_frontend_batch_dev) and one batched search with the windows as its epochs (gacq_scan_int8_dev); a
file, or a pipe, is read piece by piece with the samples that two pieces share carried over, so the recording never has to fit in
host or device memory, and the upload of piece i+1 runs under the kernels of piece i (stream.EpochStreamer's two-slot scheme)."""
import argparse
import ctypes
import sys

import numpy as np

from . import _native as nat
from . import acquire, cli, codes, rawfile, signals


def _skip_samples(fs, skip_ms):
    return int(fs * 0.001 * skip_ms)


def _start(fs, every_ms, skip, e):
    return skip + int(fs * 0.001 * every_ms * e)


def _check(fs, every_ms, n_in, skip_ms, epochs):
    if not (fs > 0 and every_ms > 0 and skip_ms >= 0 and n_in >= 1) or (epochs is not None and epochs < 0):
        raise ValueError("need fs > 0, every_ms > 0, skip_ms >= 0, n_in >= 1 and epochs >= 0")


def window_starts(fs, every_ms, nsamp_total, n_in, skip_ms=0, epochs=None):
    """First sample of every epoch whose window of n_in samples lies wholly inside a recording of nsamp_total samples (at most
    ``epochs`` of them): int64 array.  The products are those of the definition, in Python floats, left to right."""
    _check(fs, every_ms, n_in, skip_ms, epochs)
    skip = _skip_samples(fs, skip_ms)
    room = int(nsamp_total) - int(n_in) - skip
    if room < 0:
        return np.zeros(0, dtype=np.int64)
    count = int(room / (fs * 0.001 * every_ms)) + 2            # an upper bound; the exact condition decides below
    if epochs is not None:
        count = min(count, int(epochs))
    s = np.array([_start(fs, every_ms, skip, e) for e in range(count)], dtype=np.int64)
    return s[s + int(n_in) <= int(nsamp_total)]


def _read(fp, nbytes):
    """nbytes (even) from fp through rawfile's bounded reader, which reads on after a pipe's short reads; fewer only at the end"""
    if nbytes <= 0:
        return np.zeros(0, dtype=np.int8)
    z = next(rawfile.read_pieces(fp, 2, nbytes), None)
    return np.zeros(0, dtype=np.int8) if z is None else z


def read_windows(fp, fs, every_ms, n_in, skip_ms=0, epochs=None, piece_bytes=rawfile.PIECE_BYTES, max_windows=None):
    """Read the recording piece by piece, strictly forward (a pipe will do).  Yields (e0, starts, base, buf): the windows of epochs
    e0, e0 + 1, ... begin at samples `starts` (int64) of the recording, and buf (flat interleaved int8) holds its samples from `base`
    on, so window k is buf[2*(starts[k]-base) : 2*(starts[k]-base+n_in)].  A piece holds as many whole windows as fit piece_bytes and
    max_windows, one at the least; the samples its last windows share with the next piece's first are kept, not read again."""
    _check(fs, every_ms, n_in, skip_ms, epochs)
    skip = _skip_samples(fs, skip_ms)
    piece_samples = max(int(piece_bytes) // 2, 1)
    buf, base = np.zeros(0, dtype=np.int8), 0                  # samples [base, pos) of the recording
    pos, e = 0, 0
    while epochs is None or e < epochs:
        s0 = _start(fs, every_ms, skip, e)
        m = 1
        while ((epochs is None or e + m < epochs) and (max_windows is None or m < max_windows)
               and _start(fs, every_ms, skip, e + m) + n_in - s0 <= piece_samples):
            m += 1
        starts = np.array([_start(fs, every_ms, skip, e + k) for k in range(m)], dtype=np.int64)
        end = int(starts[-1]) + n_in
        if s0 >= pos:                                          # a gap: nothing is kept, the samples in between are read and dropped
            while pos < s0:
                got = len(_read(fp, 2 * min(s0 - pos, piece_samples))) // 2
                if got == 0:
                    return
                pos += got
            buf, base = np.zeros(0, dtype=np.int8), s0
        else:
            buf, base = buf[2 * (s0 - base):], s0
        new = _read(fp, 2 * (end - pos))
        pos += len(new) // 2
        buf = np.concatenate((buf, new[:2 * (len(new) // 2)])) if len(new) else buf
        if pos < end:                                          # the recording is over: the windows that lie wholly inside it, then stop
            starts = starts[starts + n_in <= pos]
            if len(starts):
                yield e, starts, base, buf
            return
        yield e, starts, base, buf
        e += m


def _finalize(sig, nitems, peaks, dop):
    """gacq_peak records [E][nitems] -> gacq_result records [E][nitems] (acquire.RESULT_DTYPE), per epoch as gacq_acquire_int8 does"""
    peaks = np.ascontiguousarray(peaks).view(acquire.PEAK_DTYPE).reshape(-1, nitems)
    out = np.zeros(peaks.shape, dtype=acquire.RESULT_DTYPE)
    desc = acquire.descriptor(sig)
    dop_p = dop.ctypes.data_as(nat.c_double_p) if len(dop) else None
    for e in range(peaks.shape[0]):
        nat.check(nat.lib.gacq_finalize(ctypes.byref(desc), peaks[e].ctypes.data_as(ctypes.POINTER(nat.Peak)), 1, None, nitems, dop_p, len(dop),
                                        out[e].ctypes.data_as(ctypes.POINTER(nat.Result))))
    return out


class _Pieces:
    """Two pinned staging slots, as stream.EpochStreamer: the upload of a piece runs on a copy stream under the kernels of the piece
    before it, the dependency is one-way (compute waits for the copy), and a slot is reused only after its results were collected."""

    def __init__(self, eng, sig, n_in, fs, coffset, ms_pad, items, dop, blocks, slot_bytes, slot_windows):
        torch = nat.require_torch()
        self.torch, self.eng = torch, eng
        self.args = (sig, n_in, fs, coffset, ms_pad, items, dop, blocks)
        self.device = torch.device("cuda", eng.device)
        eng.use_torch_stream(self.device)
        self.compute = torch.cuda.current_stream(self.device)
        self.copy = torch.cuda.Stream(self.device)
        self.pin_in = [torch.empty(slot_bytes, dtype=torch.int8).pin_memory() for _ in range(2)]
        self.dev_in = [torch.empty(slot_bytes, dtype=torch.int8, device=self.device) for _ in range(2)]
        self.pin_out = [torch.empty((slot_windows, len(items), 2), dtype=torch.float64).pin_memory() for _ in range(2)]
        self.h2d_done = [torch.cuda.Event() for _ in range(2)]
        self.out_done = [torch.cuda.Event() for _ in range(2)]
        self.count = [0, 0]

    def submit(self, slot, starts, base, buf):
        torch = self.torch
        sig, n_in, fs, coffset, ms_pad, items, dop, blocks = self.args
        ctypes.memmove(self.pin_in[slot].data_ptr(), buf.ctypes.data, buf.nbytes)
        with torch.cuda.stream(self.copy):
            self.dev_in[slot][:buf.nbytes].copy_(self.pin_in[slot][:buf.nbytes], non_blocking=True)
            self.h2d_done[slot].record(self.copy)
        self.compute.wait_event(self.h2d_done[slot])
        self.eng.scan_int8_dev(sig, self.dev_in[slot][:buf.nbytes], starts - base, n_in, fs, coffset, ms_pad, items, dop, blocks,
                               out=self.pin_out[slot][:len(starts)])
        self.out_done[slot].record(self.compute)
        self.count[slot] = len(starts)

    def collect(self, slot):
        self.out_done[slot].synchronize()
        return self.pin_out[slot][:self.count[slot]].numpy().copy()


def scan(name, iq, fs, coffset, ms, every_ms, items=None, doppler_search=None, epochs=None, engine=None, skip_ms=0,
         piece_bytes=rawfile.PIECE_BYTES):
    """Acquire `items` of signal `name` at every epoch of the recording `iq`: a numpy int8 array ([n, 2] or flat interleaved), a
    torch int8 CUDA tensor, or a binary file object (read forward, piece by piece).  Returns (starts, results): the first sample of
    every epoch (int64 [E]) and a structured array [E][nitems] of acquire.RESULT_DTYPE, row e being what the acquire command finds in
    the file that begins at sample starts[e]."""
    torch = nat.require_torch()
    sig = signals.get(name) if isinstance(name, str) else name
    if items is None:
        items = acquire.parse_list_ranges(sig.default_items, sep=sig.item_sep) if sig.default_items else codes.prns(sig.code)
    items = [int(i) for i in items]
    dop = np.ascontiguousarray(acquire.doppler_grid(doppler_search if doppler_search is not None else sig.default_doppler), dtype=np.float64)
    ms_pad = int(ms) + 5                                       # acquire-gps-l1.py:80
    n_in = int(fs * 0.001 * ms_pad)
    blocks = max(sig.blocks(int(ms)), 0)
    eng = engine or acquire.default_engine()
    empty = (np.zeros(0, dtype=np.int64), np.zeros((0, len(items)), dtype=acquire.RESULT_DTYPE))
    if len(items) == 0:
        return empty
    if isinstance(iq, np.ndarray) or torch.is_tensor(iq):
        dev = rawfile.device_int8(eng, iq)
        starts = window_starts(fs, every_ms, dev.numel() // 2, n_in, skip_ms, epochs)
        if len(starts) == 0:
            return empty
        peaks = eng.scan_int8_dev(sig, dev, starts, n_in, fs, coffset, ms_pad, items, dop, blocks)
        return starts, _finalize(sig, len(items), peaks.cpu().numpy(), dop)
    # a file object: pieces of whole windows through two staging slots
    n_out = ms_pad * int(round(sig.fs * 0.001))
    slot_bytes = 2 * max(int(piece_bytes) // 2, n_in)
    # windows of a piece: what its samples can hold, and no more than 65536 (the pinned result slots are sized by it); the library cuts
    # a piece into chunks that fit its workspace on its own
    slot_windows = min(2 + int(max(slot_bytes // 2 - n_in, 0) / (fs * 0.001 * every_ms)), 1 << 16)
    pieces = None
    all_starts, all_peaks, inflight = [], [], []
    for i, (e0, starts, base, buf) in enumerate(read_windows(fp=iq, fs=fs, every_ms=every_ms, n_in=n_in, skip_ms=skip_ms, epochs=epochs,
                                                             piece_bytes=piece_bytes, max_windows=slot_windows)):
        if pieces is None:
            pieces = _Pieces(eng, sig, n_in, fs, coffset, ms_pad, items, dop, blocks, slot_bytes, slot_windows)
        slot = i % 2
        if len(inflight) == 2:
            all_peaks.append(pieces.collect(inflight.pop(0)))
        pieces.submit(slot, starts, base, buf)
        inflight.append(slot)
        all_starts.append(starts)
    while inflight:
        all_peaks.append(pieces.collect(inflight.pop(0)))
    if not all_starts:
        return empty
    return np.concatenate(all_starts), _finalize(sig, len(items), np.concatenate(all_peaks), dop)


VALUE_OPTS = cli.VALUE_OPTS + ("--every", "--skip", "--epochs", "--min-metric")


def build_parser(sig):
    ap = cli.build_parser(sig)
    ap.prog = "scan-%s" % sig.name
    ap.description = "Acquire %s signals at every epoch of a recording on MI355X" % sig.name
    ap.add_argument("--every", type=float, default=None, metavar="T_MS", help="milliseconds from one epoch to the next (default: --time + 5, "
                    "back-to-back windows)")
    ap.add_argument("--skip", type=float, default=0.0, metavar="MS", help="milliseconds to skip at the start of the file (default %(default)s)")
    ap.add_argument("--epochs", type=int, default=None, metavar="E", help="stop after E epochs (default: to the end of the file)")
    ap.add_argument("--min-metric", type=float, default=None, metavar="X", help="print only the lines whose metric is at least X")
    return ap


def parse(name, argv):
    """(signal, parsed arguments) of the command line that follows the signal's name; the long-code signals are refused by name"""
    if name in cli.LONGCODE:
        raise SystemExit("scan: %s is searched in the time domain around one code phase (python -m gnss_dsp_tools_amd.cli %s): "
                         "there is no scan of it" % (name, name))
    sig = signals.get(name)
    args = build_parser(sig).parse_args(cli.join_option_values(list(argv), VALUE_OPTS))
    if args.every is None:
        args.every = float(args.time + 5)
    if not args.every > 0 or args.skip < 0 or (args.epochs is not None and args.epochs < 0):
        raise SystemExit("scan: need --every > 0, --skip >= 0 and --epochs >= 0")
    return sig, args


def format_lines(sig, items, starts, results, min_metric=None):
    """The command's output: one line per epoch and item, epochs first; with min_metric, without the lines below it"""
    lines = []
    for e, s in enumerate(starts):
        for item, r, t in zip(items, results[e], acquire._as_tuples(results[e])):
            if min_metric is None or r["metric"] >= min_metric:
                lines.append("epoch %d start %d " % (e, s) + acquire.format_result(sig, item, t))
    return lines


def run(name, argv, out=sys.stdout, piece_bytes=rawfile.PIECE_BYTES):
    sig, args = parse(name, argv)
    if args.items:
        items = acquire.parse_list_ranges(args.items, sep=sig.item_sep)
    else:
        items = codes.prns(sig.code)
    doppler_search = acquire.parse_list_floats(args.doppler_search)
    eng = acquire.Engine(args.device)
    try:
        with open(args.input_filename, "rb") as fp:
            starts, results = scan(sig, fp, args.sample_rate, args.carrier_offset, args.time, args.every, items, doppler_search, args.epochs,
                                   engine=eng, skip_ms=args.skip, piece_bytes=piece_bytes)
    finally:
        eng.close()
    lines = format_lines(sig, items, starts, results, args.min_metric)
    for line in lines:
        print(line, file=out)
    return lines


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    if not argv or argv[0] in ("-h", "--help"):
        print(__doc__)
        print("signals:", ", ".join(sorted(signals.SIGNALS)))
        return 0
    run(argv[0], argv[1:])
    return 0


if __name__ == "__main__":
    sys.exit(main())
