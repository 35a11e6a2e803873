"""Cancellation of tracked strong signals on the GPU (csrc/gacq_cancel.hip, gacq_cancel_dev): every tracked satellite is rebuilt from its
loop's own estimates, one segment per tracking record, scaled by the projection of the input on that replica and taken out of the
recording -- parallel interference cancellation.  A 1023-chip code isolates two PRNs by 21 to 24 dB only: a satellite at 50 dB-Hz hides
one at 30 dB-Hz from the search; on the residual the weak one is found.

    python -m gnss_dsp_tools_amd.cancel <signal> [handoff's search options] [--min-metric X] [--skip RECORDS] [--reacquire]
           IN FS COFFSET OUT

acquires <signal> on the file IN as ``python -m gnss_dsp_tools_amd.handoff`` does (same options), tracks every handed-off channel over
the whole file, cancels what was tracked (leaving out the first RECORDS records of every channel: the pull-in) and writes the int8
residual to OUT (or - for stdout).  It prints one line (to stderr when OUT is -):

    cancelled <items> samples <N> clipped <components> power <dB before> -> <dB after>

--reacquire: a line ``residual searched from sample <S>`` (the first cancelled sample) and the ordinary acquisition lines of the signal's
remaining items, searched on the residual from there on (code offsets count from S).  Only the template trackers are covered.  The definition is in include/gacq.h;
tests/cancel_oracle.py restates it."""
import ctypes
import math
import sys
from dataclasses import dataclass

import numpy as np

from . import _native as nat
from . import acquire, chiptrack, codes, handoff as _handoff, longtrack, rawfile, signals, streaming, trackloop
from .mitigate import _count, _device_input

MAX_SATS = 32
MAX_SEGS = 1 << 20
MAX_SEG_SAMPLES = 1 << 24
MAX_INDEX = 1 << 48

SEG_DTYPE = np.dtype(nat.struct("gacq_cancel_seg"))
CancelSat = nat.struct("gacq_cancel_sat")


@dataclass(frozen=True)
class Sat:
    """A satellite: the code module, the PRN (GLONASS: 0) and the chip weight 0..5, as in gacq_sim_sat"""
    code: str
    prn: int
    kind: int


def sat_of(channel):
    """The Sat of a template-family tracking channel"""
    t = _tracker(channel)
    return Sat(t.code, 0 if t.glonass else int(channel.prn), int(t.kind))


def _tracker(channel):
    name = channel.name
    if name in longtrack.LONG_TRACKERS or name in chiptrack.CHIP_TRACKERS:
        raise ValueError("%s is no template tracker: the long-code and chip-accumulator loops are not covered" % name)
    if name not in trackloop.TRACKERS:
        raise ValueError("unknown tracker %r (the template family: %s)" % (name, ", ".join(sorted(trackloop.TRACKERS))))
    return trackloop.TRACKERS[name]


def segments_from_track(channel, state0, records, skip=0):
    """The segments (SEG_DTYPE, amplitude 0) of one template-family TrackLoop channel, one per record after the first ``skip``.
    ``state0`` is loop.state(k) read before the first run(): a record holds the values after its block's update, so block r ran with
    the values of record r - 1 and the first one with state0.  The loop's host-visible arithmetic (track_loop_kernel) in doubles: the
    block length int(nf) from the code phase at the block's start, sub-block bounds floor(j n / subs), fc = -carrier_f / fs,
    cf = (code_f + carrier_f / ratio) / fs, the offset phase advanced once per outer block.  The signal's phase is minus the sum of the
    two wipe-off phases."""
    t = _tracker(channel)
    fs, coffset = float(channel.fs), float(channel.coffset)
    Ld = float(codes.code_length(t.code))
    ratio = t.scale(int(channel.prn))
    fm = -(coffset + t.glonass[3] * int(channel.prn)) / fs if t.glonass else 0.0
    fo = fm if t.glonass else -coffset / fs                      # the offset wipe-off, turns per sample
    code_p, code_f = float(state0["code_p"]), float(state0["code_f"])
    carrier_p, carrier_f = float(state0["carrier_p"]), float(state0["carrier_f"])
    cph, pos = float(state0["coffset_phase"]), int(state0["pos"])
    skip = int(skip)
    out = np.zeros(max(len(records) - skip, 0), dtype=SEG_DTYPE)
    r = 0
    while r + t.subs <= len(records):
        nf = (fs * t.period * (Ld - code_p)) / Ld if code_p < Ld / 2 else (fs * t.period * (2 * Ld - code_p)) / Ld
        n = int(nf)
        for j in range(t.subs):
            a, b = int(float(j * n) / float(t.subs)), int(float((j + 1) * n) / float(t.subs))
            if r >= skip:
                g = out[r - skip]
                g["s0"], g["n"] = pos + a, b - a
                g["carrier_hz"] = (-fm * fs if t.glonass else coffset) + carrier_f
                g["carrier_phase"] = -((cph + a * fo) + carrier_p)
                g["code_rate_hz"] = ((code_f + carrier_f / ratio) / fs) * fs
                g["code_phase"] = code_p % Ld
            rec = records[r]
            code_p, code_f = float(rec["code_p"]), float(rec["code_f"])
            carrier_p, carrier_f = float(rec["carrier_p"]), float(rec["carrier_f"])
            r += 1
        cph = (cph + n * fm if t.glonass else cph - (n * coffset) / fs) % 1.0
        pos += n
    return out[:max(r - skip, 0)]


def _sat_structs(sats, segs):
    sats = list(sats)
    segs = [np.ascontiguousarray(s, dtype=SEG_DTYPE).reshape(-1) for s in segs]
    if len(sats) != len(segs):
        raise ValueError("need one segment array per satellite (%d), got %d" % (len(sats), len(segs)))
    if not 1 <= len(sats) <= MAX_SATS:
        raise ValueError("need 1..%d satellites, got %d" % (MAX_SATS, len(sats)))
    arr = (CancelSat * len(sats))(*[CancelSat(code=s.code.encode(), prn=int(s.prn), kind=int(s.kind), nseg=len(g), pad=0) for s, g in zip(sats, segs)])
    flat = np.concatenate(segs)
    if len(flat) == 0:
        flat = np.zeros(1, dtype=SEG_DTYPE)          # no segment at all: still a valid address
    if len(flat) > MAX_SEGS:
        raise ValueError("at most %d segments per call, got %d" % (MAX_SEGS, len(flat)))
    return arr, flat, segs


def apply(engine, sats, segs, fs, data, in_first=0, out_first=None, n_out=None, estimate=True, dtype="int8", in_complex64=False, out=None):
    """One call of gacq_cancel_dev.  ``sats``: Sat objects; ``segs``: one SEG_DTYPE array per satellite, ascending and not overlapping;
    ``data``: input samples in_first .. (a flat int8 or complex64 CUDA tensor, or bytes as mitigate.apply takes them).  Output samples
    out_first .. out_first + n_out - 1 (default: every sample of the input) as a flat int8 CUDA tensor [2 n_out] or complex64 [n_out];
    ``out``: a contiguous tensor of that shape and type to write into.
    Returns (output, [complex128 amplitudes per satellite, NaN for a segment that does not touch the output range], clipped components)."""
    torch = nat.require_torch()
    arr, flat, segs = _sat_structs(sats, segs)
    d, in_c = _device_input(engine, data, in_complex64)
    in_first = int(in_first)
    in_count = _count(d, in_c)
    out_first = in_first if out_first is None else int(out_first)
    n_out = max(0, in_first + in_count - out_first) if n_out is None else int(n_out)
    cplx, fresh = streaming.iq_out(n_out if out is None else 0, dtype, d.device)
    numel = max(n_out, 0) * (1 if cplx else 2)
    if out is None:
        out = fresh
    elif not (torch.is_tensor(out) and out.is_cuda and out.dtype == fresh.dtype and out.dim() == 1 and out.numel() == numel and out.is_contiguous()):
        raise ValueError("out must be a contiguous 1-D %s CUDA tensor of %d elements" % (dtype, numel))
    amps = np.full(len(flat), np.nan + 1j * np.nan, dtype=np.complex128)
    clipped = ctypes.c_ulonglong(0)
    if n_out > 0:                              # n_out = 0 does nothing
        engine.use_torch_stream(d.device)
        nat.check(nat.lib.gacq_cancel_dev(engine._ctx, ctypes.addressof(arr), len(arr), ctypes.c_void_p(flat.ctypes.data), float(fs), int(bool(estimate)),
                                          ctypes.c_void_p(d.data_ptr()), int(in_c), in_first, in_count, out_first, n_out, int(cplx),
                                          ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(amps.ctypes.data), ctypes.byref(clipped)), engine._ctx)
    cuts = np.cumsum([0] + [len(g) for g in segs])
    return out, [amps[cuts[k]:cuts[k + 1]] for k in range(len(segs))], int(clipped.value)


class Canceller(streaming.Chunks):
    """A recording fed chunk by chunk (bytes or int8 / uint8 / complex64 CUDA tensors): feed(chunk) returns the output samples the chunk
    completes, and the concatenation of what the calls return is what one apply() of the whole recording gives.  With estimate, a
    segment is cancelled once all its samples are there: the input from the first unfinished segment on -- at most one segment per
    satellite, because segments are sorted -- stays on the device.  ``start``: the absolute index of the first sample fed.  amps (one complex128 array per satellite, NaN where nothing was
    estimated yet), clipped, power_in and power_out (sums of squares of the output range) are the running results."""

    def __init__(self, engine, sats, segs, fs, estimate=True, dtype="int8", in_complex64=False, start=0):
        self.engine, self.sats, self.fs = engine, list(sats), float(fs)
        self.estimate, self.dtype, self.in_complex64 = bool(estimate), dtype, bool(in_complex64)
        _, _, self.segs = _sat_structs(self.sats, segs)
        self.amps = [np.full(len(g), np.nan + 1j * np.nan, dtype=np.complex128) for g in self.segs]
        self.clipped = 0
        self.power_in = self.power_out = 0.0
        super().__init__(64 if self.in_complex64 else 16, lambda in_first, in_count: self._whole(in_first + in_count), self._run, self._whole, start=start)

    def _power(self, t):
        torch = nat.require_torch()
        v = torch.view_as_real(t).reshape(-1) if t.dtype.is_complex else t
        return float(v.to(torch.float64).pow(2).sum().item()) if v.numel() else 0.0

    def _whole(self, end):
        """`end`, or with estimate the first sample of a segment that `end` cuts: such a segment holds the output back to its first
        sample, and one that reaches past the outputs is estimated again from there"""
        back = end
        if self.estimate:
            for g in self.segs:
                i = int(np.searchsorted(g["s0"] + g["n"], end, side="right"))
                if i < len(g) and g["s0"][i] < end:
                    back = min(back, int(g["s0"][i]))
        return back

    def _run(self, ds, in_first, in_count, out_first, n_out, k):
        torch = nat.require_torch()
        out_end, unit = out_first + n_out, self.sample_bits // 8
        lo = [int(np.searchsorted(g["s0"] + g["n"], out_first, side="right")) for g in self.segs]      # the segments that touch the outputs
        hi = [max(l, int(np.searchsorted(g["s0"], out_end, side="left"))) for l, g in zip(lo, self.segs)]
        x = ds[0] if self.in_complex64 else ds[0].view(torch.int8)
        out, amps, clipped = apply(self.engine, self.sats, [g[l:h] for g, l, h in zip(self.segs, lo, hi)], self.fs, x, in_first, out_first, n_out,
                                   self.estimate, self.dtype, self.in_complex64)
        self.clipped += clipped
        if n_out:
            for j, (l, h) in enumerate(zip(lo, hi)):
                self.amps[j][l:h] = amps[j]
            off = (out_first - in_first) * unit
            xin = ds[0][off:off + n_out * unit]
            self.power_in += self._power(xin.view(torch.complex64) if self.in_complex64 else xin.view(torch.int8))
            self.power_out += self._power(out)
        return out

    def feed(self, chunk):
        torch = nat.require_torch()
        d, _ = _device_input(self.engine, chunk, self.in_complex64)
        return self.feed_all([(torch.view_as_real(d).reshape(-1) if d.dtype.is_complex else d).view(torch.uint8)])


def cancel_file(engine, sats, segs, fs, fin, fout, estimate=True, dtype="int8", in_complex64=False, piece_bytes=rawfile.PIECE_BYTES):
    """Cancel the open binary file fin into fout piece by piece.  (samples written, Canceller with the totals)."""
    can = Canceller(engine, sats, segs, fs, estimate, dtype, in_complex64)
    n = streaming.pump(rawfile.read_pieces(fin, 8 if in_complex64 else 2, piece_bytes), lambda held: lambda piece: [can.feed(piece.view(np.uint8))], [fout],
                       2 if dtype == "int8" else 1)
    return n[0] if n else 0, can


def _cancel_tracked(name, iq_int8, fs, coffset, items=None, min_metric=None, skip=0, **handoff_kw):
    """cancel_tracked with everything the command line reports: (residual, results, refined, records, sats, segs, amps, clipped)"""
    results, refined, loop, x_dev = _handoff.handoff(name, iq_int8, fs, coffset, items=items, min_metric=min_metric, **handoff_kw)
    if loop is None:
        return x_dev, results, refined, [], [], [], [], 0
    try:
        state0 = [loop.state(k) for k in range(loop.K)]          # the loop has not run yet: what the first block runs with
        recs = loop.run([x_dev] * loop.K)
        chans = loop.channels
        eng = loop.eng
    finally:
        loop.close()
    sats = [sat_of(c) for c in chans]
    segs = [segments_from_track(c, s, r, skip) for c, s, r in zip(chans, state0, recs)]
    out, amps, clipped = apply(eng, sats, segs, fs, x_dev, estimate=True)
    return out, results, refined, recs, sats, segs, amps, clipped


def cancel_tracked(name, iq_int8, fs, coffset, items=None, min_metric=None, skip=0, **handoff_kw):
    """Acquire ``name`` on the interleaved int8 recording (numpy, host) and hand off as handoff.handoff does (its keywords pass through),
    track every channel over the whole recording, build each channel's segments from its records after the first ``skip`` and cancel
    them with estimated amplitudes.  Returns (residual: flat int8 CUDA tensor, (acquisition results, [(item, Refined)]), one record
    array per channel)."""
    out, results, refined, recs = _cancel_tracked(name, iq_int8, fs, coffset, items, min_metric, skip, **handoff_kw)[:4]
    return out, (results, refined), recs


def build_parser(sig):
    ap = _handoff.build_parser(sig)
    ap.prog = "cancel %s" % sig.name
    ap.description = "Acquire and track %s, cancel what was tracked and write the residual" % sig.name
    ap.add_argument("--skip", type=int, default=0, help="records of every channel left uncancelled: the pull-in (default %(default)s)")
    ap.add_argument("--reacquire", action="store_true", help="search the signal's remaining items on the residual and print the acquisition lines")
    ap.add_argument("output_filename")
    return ap


def parse(name, argv):
    """(signal, argparse namespace with .items as a list, .doppler_search and .loop_dwells as floats)"""
    _handoff.tracker_name(name)
    sig = signals.get(name)
    a = build_parser(sig).parse_args(_handoff._join_option_values(list(argv)))
    if a.out_dir is not None or a.nav:
        raise SystemExit("cancel: --out-dir and --nav belong to the handoff command")
    if a.skip < 0:
        raise SystemExit("cancel: --skip must not be negative")
    a.items = acquire.parse_list_ranges(a.items, sep=sig.item_sep) if a.items else codes.prns(sig.code)
    a.doppler_search = acquire.parse_list_floats(a.doppler_search)
    a.loop_dwells = tuple(acquire.parse_list_floats(a.loop_dwells))
    return sig, a


def _db(power, samples):
    return 10.0 * math.log10(power / (2.0 * samples)) if power > 0.0 and samples else float("-inf")


def report_line(items, samples, clipped, power_in, power_out):
    return "cancelled %s samples %d clipped %d power %.2f -> %.2f dB" % (",".join(str(i) for i in items) or "none", int(samples), int(clipped),
                                                                         _db(power_in, samples), _db(power_out, samples))


def reacquire(engine, sig, residual_int8, fs, coffset, start, items, doppler_search, ms=80):
    """The acquisition of the handoff command on the residual (numpy int8, interleaved) from sample ``start`` on: [(item, result)]"""
    ms_pad = int(ms) + 5
    n = int(float(fs) * 0.001 * ms_pad)
    win = residual_int8[2 * int(start):2 * (int(start) + n)]
    if len(win) < 2 * n:
        raise ValueError("residual too short: the acquisition needs %d samples after sample %d" % (n, start))
    res = engine.acquire_int8(sig, win, float(fs), float(coffset), ms_pad, list(items), acquire.doppler_grid(doppler_search), max(sig.blocks(int(ms)), 0))
    return list(zip(items, res))


def run(name, argv, out=None):
    sig, a = parse(name, argv)
    to_stdout = a.output_filename == "-"
    if out is None:
        out = sys.stderr if to_stdout else sys.stdout
    raw = np.fromfile(a.input_filename, dtype=np.int8)
    raw = raw[:len(raw) // 2 * 2]
    eng = acquire.Engine(a.device)
    lines = []
    try:
        res, _, refined, _, _, segs, _, clipped = _cancel_tracked(name, raw, a.sample_rate, a.carrier_offset, a.items, a.min_metric, a.skip,
                                                                  doppler_search=a.doppler_search, ms=a.time, min_ratio=a.min_ratio, M=a.blocks,
                                                                  loop_dwells=a.loop_dwells, engine=eng)
        host = res.cpu().numpy()
        done = [it for it, _ in refined]
        n = len(host) // 2
        p_in = float(np.sum(raw[:2 * n].astype(np.float64) ** 2))
        p_out = float(np.sum(host.astype(np.float64) ** 2))
        lines.append(report_line(done, n, clipped, p_in, p_out))
        if a.reacquire:
            all_items = acquire.parse_list_ranges(sig.default_items, sep=sig.item_sep) if sig.default_items else codes.prns(sig.code)
            rest = [it for it in all_items if it not in done]
            start = max([int(g["s0"][0]) for g in segs if len(g)], default=0)
            lines.append("residual searched from sample %d" % start)
            lines += [acquire.format_result(sig, it, r) for it, r in reacquire(eng, sig, host, a.sample_rate, a.carrier_offset, start, rest,
                                                                               a.doppler_search, a.time)]
        fout = sys.stdout.buffer if to_stdout else open(a.output_filename, "wb")
        try:
            fout.write(host.tobytes())
            fout.flush()
        finally:
            if not to_stdout:
                fout.close()
    finally:
        eng.close()
    for line in lines:
        print(line, file=out)
    return lines


def main(argv=None):
    return streaming.main(argv, __doc__, lambda argv: run(argv[0], argv[1:]))


if __name__ == "__main__":
    sys.exit(main())
