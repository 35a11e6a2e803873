"""Device-resident tracking loops for the long-code scripts: track-gps-l2cl.py and track-glonass-l1-p.py / -l2-p.py on the GPU.

Their ``track()`` and main loop are the template's (trackloop.py) with other constants: a 767 250- or 5 110 000-chip code, a 1.5 s or
1 s outer block split into 1500 or 1000 ``track()`` calls, ``np.mod`` phases without cycle counters and 9 printed columns.
``LongTrackLoop`` runs K such channels in one launch (csrc/gacq_longtrack.hip, one workgroup per channel); the code table stays in
device memory and each sub-block reads a window of it.  beidou-b2bi/-b2bq (nco.accum) run in chiptrack.
"""
import numpy as np

from . import _native as nat
from . import trackloop
from .trackloop import RECORD_DTYPE, STATE_DTYPE, Channel, Tracker, TrackSpec  # noqa: F401  (re-exported)

LONG_TRACKERS = {
    "gps-l2cl": Tracker("gps.l2cl", 5, 0.5, 2400.0, 1.500, 1.0 / 1.500, 1500),
    "glonass-l1-p": Tracker("glonass.p", 0, 0.5, None, 1.000, 1.0, 1000, glonass=(1602.0, 0.5625, 5.11, 562500)),
    "glonass-l2-p": Tracker("glonass.p", 0, 0.5, None, 1.000, 1.0, 1000, glonass=(1246.0, 0.4375, 5.11, 437500)),
}

STATUS = {**trackloop.STATUS, nat.CONSTANTS["GACQ_TRACK_BAD_WINDOW"]: "code span of a sub-block exceeds the chip window"}


def long_channel_spec(ch):
    """gacq_track_spec of a long-code channel: trackloop.channel_spec's arithmetic with LONG_TRACKERS' constants."""
    if ch.name not in LONG_TRACKERS:
        raise KeyError("unknown long-code tracker %r (%s)" % (ch.name, ", ".join(sorted(LONG_TRACKERS))))
    return trackloop.channel_spec(ch, LONG_TRACKERS)


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

    _lib = "gacq_longtrack"

    def __init__(self, channels, engine=None, max_records=3000):
        super().__init__(channels, engine, max_records)
        self._pend = [_Pending() for _ in range(self.K)]

    @staticmethod
    def _trackers():
        return LONG_TRACKERS

    @staticmethod
    def _channel_spec(ch):
        return long_channel_spec(ch)

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
    return trackloop.format_lines(name, recs, chip_rate, LONG_TRACKERS)


def track_file(*args, **kw):
    """One script run on one file, trackloop.track_file's arguments: returns (records, output lines)."""
    return trackloop.track_file(*args, loop=LongTrackLoop, **kw)
