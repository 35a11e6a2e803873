"""Device-resident tracking loops for the long-code scripts: track-gps-l2cl.py and track-glonass-l1-p.py / -l2-p.py on the GPU.

Their ``track()`` and main loop are the template's (trackloop.py) with other constants: a 767 250- or 5 110 000-chip code, a 1.5 s or
1 s outer block split into 1500 or 1000 ``track()`` calls, ``np.mod`` phases without cycle counters and 9 printed columns.
``LongTrackLoop`` runs K such channels in one launch (csrc/gacq_longtrack.hip, one workgroup per channel); the code table stays in
device memory and each sub-block reads a window of it.  beidou-b2bi/-b2bq (nco.accum) run in chiptrack.
"""
import ctypes

import numpy as np

from . import _native as nat
from . import acquire
from . import codes
from . import trackloop
from .trackloop import RECORD_DTYPE, STATE_DTYPE, Channel, Tracker, TrackSpec  # noqa: F401  (re-exported)

LONG_TRACKERS = {
    "gps-l2cl": Tracker("gps.l2cl", 5, 0.5, 2400.0, 1.500, 1.0 / 1.500, 1500),
    "glonass-l1-p": Tracker("glonass.p", 0, 0.5, None, 1.000, 1.0, 1000, glonass=(1602.0, 0.5625, 5.11, 562500)),
    "glonass-l2-p": Tracker("glonass.p", 0, 0.5, None, 1.000, 1.0, 1000, glonass=(1246.0, 0.4375, 5.11, 437500)),
}

STATUS = {**trackloop.STATUS, 3: "code span of a sub-block exceeds the chip window"}


def long_channel_spec(ch):
    """gacq_track_spec of a long-code channel, with the script's own arithmetic for everything derived from its arguments (the same
    as trackloop.channel_spec's)."""
    if ch.name not in LONG_TRACKERS:
        raise KeyError("unknown long-code tracker %r (%s)" % (ch.name, ", ".join(sorted(LONG_TRACKERS))))
    t = LONG_TRACKERS[ch.name]
    fs, coffset = float(ch.fs), float(ch.coffset)
    wide, narrow = (float(ch.loop_dwells[0]), float(ch.loop_dwells[1]))
    phase = 0.0
    if ch.carrier_phase is not None:
        wide, narrow = 0.0, 0.0                  # loop_dwells = 0,0
        phase = float(ch.carrier_phase)
    fm = 0.0
    if t.glonass:
        fm = -(coffset + t.glonass[3] * int(ch.prn)) / fs
    return TrackSpec(code=t.code.encode(), prn=0 if t.glonass else int(ch.prn), kind=t.kind, subs=t.subs, fixed_pll=0,
                     glonass=int(bool(t.glonass)), pad=0, fs=fs, period=t.period, rate=t.rate, ratio=t.scale(int(ch.prn)),
                     spacing=t.spacing, chip_rate=float(codes.chip_rate(t.code)), fll_k_wide=t.fll[0], fll_k_narrow=t.fll[1],
                     pll_k1=float(t.pll[0]), pll_k2=float(t.pll[1]), dll_k1=float(t.dll[0]), dll_k2=float(t.dll[1]), coffset=coffset,
                     fm=fm, code_offset=float(ch.code_offset), doppler=float(ch.doppler), carrier_phase=phase, dwell_wide=wide,
                     dwell_narrow=narrow)


class _Pending:
    """feed()'s samples of one channel on the device: a growable int8 buffer holding samples [base, base + fill/2) of the recording.
    A chunk is appended in place; the consumed head is dropped only when the buffer must make room, so every sample is copied O(1)
    times however small the chunks are."""

    def __init__(self):
        self.buf = None
        self.fill = 0            # bytes in use
        self.base = 0            # recording sample index of buf[0]

    def append(self, chunk, next_block):
        """Append chunk (1-D int8 device tensor); next_block() gives the first sample still needed (read only when the buffer must
        make room)."""
        torch = nat.require_torch()
        c = chunk.reshape(-1)
        need = c.numel()
        if self.buf is None:
            self.buf = torch.empty(max(2 * need, 1 << 20), dtype=torch.int8, device=c.device)
        if self.fill + need > self.buf.numel():
            drop = 2 * max(0, min(next_block() - self.base, self.fill // 2))
            live = self.fill - drop
            cap = self.buf.numel()
            while live + need > cap // 2:          # keep at least half the buffer free after a move: moves stay rare
                cap *= 2
            new = torch.empty(cap, dtype=torch.int8, device=c.device)
            if live:
                new[:live].copy_(self.buf[drop:self.fill])
            self.buf, self.fill, self.base = new, live, self.base + drop // 2
        self.buf[self.fill:self.fill + need].copy_(c)
        self.fill += need

    def view(self):
        return None if self.buf is None else self.buf[:self.fill // 2 * 2]


class LongTrackLoop(trackloop.TrackLoop):
    """K long-code channels tracked on the device, with TrackLoop's interface and guarantees: ``run(recordings)`` tracks each
    channel over its whole int8 recording (channels may share a tensor), ``feed(chunks)`` takes successive chunks split anywhere, and
    records are bit-identical however the samples are split and whichever channels share the launch.  A launch runs whole outer
    blocks only, so ``max_records`` is at least the largest ``subs`` (1500 for L2CL)."""

    def __init__(self, channels, engine=None, max_records=3000):
        self.eng = engine or acquire.default_engine()
        self.channels = list(channels)
        if not self.channels:
            raise ValueError("LongTrackLoop needs at least one channel")
        specs = [long_channel_spec(c) for c in self.channels]
        self.trackers = [LONG_TRACKERS[c.name] for c in self.channels]
        self.K = len(specs)
        self._specs = (TrackSpec * self.K)(*specs)
        self.subs_max = max(t.subs for t in self.trackers)
        self.max_records = max(int(max_records), self.subs_max)
        h = ctypes.c_void_p()
        nat.check(nat.lib.gacq_longtrack_open(self.eng._ctx, self._specs, self.K, ctypes.byref(h)), self.eng._ctx)
        self._h = h
        self._pend = [_Pending() for _ in range(self.K)]
        self.records = [[] for _ in range(self.K)]
        self.status = [0] * self.K

    def close(self):
        if self._h:
            nat.lib.gacq_longtrack_close(self._h)
            self._h = None

    def state(self, k):
        out = np.zeros(1, dtype=STATE_DTYPE)
        nat.check(nat.lib.gacq_longtrack_state(self._h, k, out.ctypes.data_as(ctypes.c_void_p)), self.eng._ctx)
        return out[0]

    def _launch(self, xs, bases):
        torch = nat.require_torch()
        self.eng.use_torch_stream(torch.device("cuda", self.eng.device))
        ptrs = (ctypes.c_void_p * self.K)()
        base = np.ascontiguousarray(bases, dtype=np.int64)
        avail = np.zeros(self.K, dtype=np.int64)
        keep = []
        for k, x in enumerate(xs):
            if x is None:
                x = torch.zeros(2, dtype=torch.int8, device="cuda:%d" % self.eng.device)
                keep.append(x)
            else:
                if not (hasattr(x, "is_cuda") and x.is_cuda and x.dtype == torch.int8 and x.dim() == 1 and x.is_contiguous()):
                    raise ValueError("channel %d: samples must be a contiguous 1-D int8 CUDA tensor (interleaved I/Q)" % k)
                avail[k] = x.numel() // 2
            ptrs[k] = x.data_ptr()
        cap = self.max_records
        recs = np.zeros((self.K, cap), dtype=RECORD_DTYPE)
        counts = np.zeros(self.K, dtype=np.int32)
        status = np.zeros(self.K, dtype=np.int32)
        nat.check(nat.lib.gacq_longtrack_run_dev(self._h, ptrs, base.ctypes.data_as(ctypes.c_void_p), avail.ctypes.data_as(ctypes.c_void_p),
                                                 self.max_records, recs.ctypes.data_as(ctypes.c_void_p), cap,
                                                 counts.ctypes.data_as(nat.c_int_p), status.ctypes.data_as(nat.c_int_p)), self.eng._ctx)
        del keep
        out = [recs[k, :counts[k]].copy() for k in range(self.K)]
        for k in range(self.K):
            self.records[k].append(out[k])
            self.status[k] = int(status[k])
        return out

    def feed(self, chunks):
        """Append the next chunk of each channel's recording (a list of K int8 CUDA tensors or None) and track as far as the samples
        allow; the samples a channel's next outer block still needs stay on the device for the next call.  Returns the new records."""
        if len(chunks) != self.K:
            raise ValueError("need one chunk (or None) per channel (%d), got %d" % (self.K, len(chunks)))
        for k, c in enumerate(chunks):
            if c is not None:
                self._pend[k].append(c, lambda k=k: int(self.state(k)["pos"]))
        new = [[] for _ in range(self.K)]
        while True:
            got = self._launch([p.view() for p in self._pend], [p.base for p in self._pend])
            for k in range(self.K):
                new[k].append(got[k])
            if all(len(g) == 0 for g in got):
                break
        return [np.concatenate(n) for n in new]


def format_lines(name, recs, chip_rate=None):
    """The script's output lines ('%d %f %f %f %f %f %f %f %f') from a record array."""
    t = LONG_TRACKERS[name]
    cr = float(codes.chip_rate(t.code) if chip_rate is None else chip_rate)
    out = []
    for r in recs:
        p = complex(float(r["p_re"]), float(r["p_im"]))
        v = (int(r["block"]), np.real(p), np.imag(p), float(r["carrier_f"]), float(r["code_f"]) - cr, (180 / np.pi) * np.angle(p),
             float(r["early"]), float(r["prompt"]), float(r["late"]))
        out.append('%d %f %f %f %f %f %f %f %f' % v)
    return out


def track_file(name, path, fs, coffset, prn, doppler, code_offset, loop_dwells=(500.0, 500.0), carrier_phase=None, engine=None):
    """One script run on one file: returns (records, output lines)."""
    ch = Channel(name, fs, coffset, prn, doppler, code_offset, tuple(loop_dwells), carrier_phase)
    eng = engine or acquire.default_engine()
    tl = LongTrackLoop([ch], eng)
    try:
        recs = tl.run([trackloop.load_int8(path, eng.device)])[0]
    finally:
        tl.close()
    return recs, format_lines(name, recs)
