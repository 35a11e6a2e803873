"""Device-resident tracking loops: the template family of the reference's track-*.py scripts on the GPU.

Every template script runs the same ``track()`` body (track-gps-l1.py:33-94) and the same main loop (:153-179); they differ only in
the constants of ``TRACKERS``.  ``TrackLoop`` runs K such channels in one launch (csrc/gacq_trackloop.hip, one workgroup per
channel), each on its own int8 recording resident on the device, and keeps the loop state on the device between calls, so a
recording can be fed in chunks.  Not template scripts: gps-l2cl and glonass-l1-p/-l2-p run in longtrack; beidou-b2bi/-b2bq run the
template loop plus the on-device chip accumulator (nco.accum) in chiptrack.
"""
import ctypes
from dataclasses import dataclass

import numpy as np

from . import _native as nat
from . import acquire
from . import codes


@dataclass(frozen=True)
class Tracker:
    code: str                  # code module (the package's code name)
    kind: int                  # correlator kind of tracking.KIND
    spacing: float             # early/late offset, chips
    ratio: float               # carrier/code frequency ratio; GLONASS: rf_carrier(chan) / divisor
    period: float              # seconds per outer block, as the script writes it (fs*period)
    rate: float                # n*rate*L/fs of the alignment
    subs: int                  # track() calls per outer block
    pll: tuple = (0.1, 3.5)
    dll: tuple = (0.00002, 0.2)
    fll: tuple = (3.0, 0.8)
    cols: int = 9              # printed columns: 14 with code_cyc, code_p, carrier_cyc, carrier_p, samp
    fixed_pll: bool = False    # mode='PLL' from the start, no switches (Xona)
    carrier_phase: bool = True # --carrier-phase sets the initial phase (L3OC starts at 0 regardless)
    glonass: tuple = None      # (rf_base, rf_step, divisor, offset_step): rf_carrier = base + step*chan, fm = -(coffset + offset_step*chan)/fs

    def scale(self, chan=0):
        """the carrier/code ratio of cf = (code_f + carrier_f/ratio)/fs, evaluated as the script does"""
        if self.glonass:
            base, step, div, _ = self.glonass
            return (base + step * chan) / div
        return self.ratio


_G1 = (1602.0, 0.5625, 0.511, 562500)
_G2 = (1246.0, 0.4375, 0.511, 437500)

TRACKERS = {
    "gps-l1": Tracker("gps.ca", 0, 0.05, 1540.0, 0.001, 1000.0, 1, cols=14),
    "gps-l1cd": Tracker("gps.l1cd", 1, 0.2, 1540.0, 0.01, 100.0, 10),
    "gps-l1cp": Tracker("gps.l1cp", 3, 0.2, 1540.0, 0.01, 100.0, 10),
    "gps-l2cm": Tracker("gps.l2cm", 4, 0.5, 2400.0, 0.020, 50.0, 20),
    "gps-l5i": Tracker("gps.l5i", 0, 0.5, 115.0, 0.001, 1000.0, 1),
    "gps-l5q": Tracker("gps.l5q", 0, 0.5, 115.0, 0.001, 1000.0, 1),
    "galileo-e1b": Tracker("galileo.e1b", 2, 0.2, 1540.0, 0.004, 250.0, 4),
    "galileo-e1c": Tracker("galileo.e1c", 2, 0.2, 1540.0, 0.004, 250.0, 4),
    "galileo-e5ai": Tracker("galileo.e5ai", 0, 0.2, 115.0, 0.001, 1000.0, 1),
    "galileo-e5aq": Tracker("galileo.e5aq", 0, 0.5, 115.0, 0.001, 1000.0, 1),
    "galileo-e5bi": Tracker("galileo.e5bi", 0, 0.2, 118.0, 0.001, 1000.0, 1),
    "galileo-e5bq": Tracker("galileo.e5bq", 0, 0.5, 118.0, 0.001, 1000.0, 1),
    "galileo-e6b": Tracker("galileo.e6b", 0, 0.5, 250.0, 0.001, 1000.0, 1),
    "galileo-e6c": Tracker("galileo.e6c", 0, 0.5, 250.0, 0.001, 1000.0, 1),
    "beidou-b1i": Tracker("beidou.b1i", 0, 0.5, 763.0, 0.001, 1000.0, 1),
    "beidou-b2i": Tracker("beidou.b1i", 0, 0.5, 590.0, 0.001, 1000.0, 1),
    "beidou-b3i": Tracker("beidou.b3i", 0, 0.5, 124.0, 0.001, 1000.0, 1),
    "beidou-b1cd": Tracker("beidou.b1cd", 1, 0.2, 1540.0, 0.01, 100.0, 10),
    "beidou-b1cp": Tracker("beidou.b1cp", 1, 0.2, 1540.0, 0.01, 100.0, 10),
    "beidou-b2ad": Tracker("beidou.b2ad", 0, 0.5, 115.0, 0.001, 1000.0, 1),
    "beidou-b2ap": Tracker("beidou.b2ap", 0, 0.5, 115.0, 0.001, 1000.0, 1),
    "glonass-l1": Tracker("glonass.ca", 0, 0.5, None, 0.001, 1000.0, 1, glonass=_G1),
    "glonass-l2": Tracker("glonass.ca", 0, 0.5, None, 0.001, 1000.0, 1, glonass=_G2),
    "glonass-l3ocd": Tracker("glonass.l3ocd", 0, 0.5, 117.5, 0.001, 1000.0, 1, carrier_phase=False),
    "glonass-l3ocp": Tracker("glonass.l3ocp", 0, 0.5, 117.5, 0.001, 1000.0, 1, carrier_phase=False),
    "xona-x1d": Tracker("xona.x1d", 0, 0.05, 1557.5, 0.001, 1000.0, 1, pll=(0.5, 15), cols=14, fixed_pll=True),
    "xona-x1p": Tracker("xona.x1p", 0, 0.05, 1557.5, 0.001, 1000.0, 1, pll=(0.5, 15), cols=14, fixed_pll=True),
    "xona-x5p": Tracker("xona.x5p", 0, 0.5, 116.375, 0.001, 1000.0, 1, pll=(0.5, 200), dll=(0.0002, 20), fixed_pll=True),
}

STATUS = {nat.CONSTANTS["GACQ_TRACK_RUNNING"]: "running", nat.CONSTANTS["GACQ_TRACK_BAD_BLOCK"]: "bad block length",
          nat.CONSTANTS["GACQ_TRACK_BAD_PHASE"]: "NCO phase or rate out of range"}

TrackSpec = nat.struct("gacq_track_spec")
RECORD_DTYPE = np.dtype(nat.struct("gacq_track_record"))
STATE_DTYPE = np.dtype(nat.struct("gacq_track_chstate"))


@dataclass
class Channel:
    """One channel: the script's name and its command line (PRN, or the RF channel for GLONASS L1/L2)."""
    name: str
    fs: float
    coffset: float
    prn: int
    doppler: float
    code_offset: float
    loop_dwells: tuple = (500.0, 500.0)
    carrier_phase: float = None


def channel_spec(ch, trackers=TRACKERS):
    """gacq_track_spec of a channel, with the script's own arithmetic for everything derived from its arguments.  ``trackers``: the
    table that holds the channel's name (longtrack.LONG_TRACKERS and chiptrack.CHIP_TRACKERS go through their own wrappers)."""
    if ch.name not in trackers:
        raise KeyError("unknown tracker %r (the template family: %s)" % (ch.name, ", ".join(sorted(trackers))))
    t = trackers[ch.name]
    fs, coffset = float(ch.fs), float(ch.coffset)
    wide, narrow = (float(ch.loop_dwells[0]), float(ch.loop_dwells[1]))
    phase = 0.0
    if ch.carrier_phase is not None:
        wide, narrow = 0.0, 0.0                  # loop_dwells = 0,0
        if t.carrier_phase:
            phase = float(ch.carrier_phase)
    fm = 0.0
    if t.glonass:
        fm = -(coffset + t.glonass[3] * int(ch.prn)) / fs
    return TrackSpec(code=t.code.encode(), prn=0 if t.glonass else int(ch.prn), kind=t.kind, subs=t.subs, fixed_pll=int(t.fixed_pll),
                     glonass=int(bool(t.glonass)), pad=0, fs=fs, period=t.period, rate=t.rate, ratio=t.scale(int(ch.prn)),
                     spacing=t.spacing, chip_rate=float(codes.chip_rate(t.code)), fll_k_wide=t.fll[0], fll_k_narrow=t.fll[1],
                     pll_k1=float(t.pll[0]), pll_k2=float(t.pll[1]), dll_k1=float(t.dll[0]), dll_k2=float(t.dll[1]), coffset=coffset,
                     fm=fm, code_offset=float(ch.code_offset), doppler=float(ch.doppler), carrier_phase=phase, dwell_wide=wide,
                     dwell_narrow=narrow)


class TrackLoop:
    """K channels tracked on the device.  ``run(recordings)`` takes one interleaved int8 I/Q torch CUDA tensor per channel (a channel
    may share another's tensor) and walks every channel up to ``max_records`` records (1 ms of signal each, whole outer blocks) per
    launch until its samples run out;
    ``feed()`` does the same with successive chunks of each recording.  Records are bit-identical however the samples are split
    and whichever channels share the launch."""

    def __init__(self, channels, engine=None, max_records=100):
        self.eng = engine or acquire.default_engine()
        self.channels = list(channels)
        if not self.channels:
            raise ValueError("%s needs at least one channel" % type(self).__name__)
        self.trackers = [self._trackers().get(c.name) for c in self.channels]
        specs = [self._channel_spec(c) for c in self.channels]
        self.K = len(specs)
        self._specs = (TrackSpec * self.K)(*specs)
        self.subs_max = max(t.subs for t in self.trackers)
        # a launch covers at most max_records ms of signal per channel, whatever each channel's block length (a record is one
        # track() call, 1 ms in every template script)
        self.max_records = max(int(max_records), self.subs_max)
        self._h = self._open()
        self._pending = [None] * self.K          # feed(): the unconsumed tail of each channel's samples and its first sample index
        self._base = [0] * self.K
        self.records = [[] for _ in range(self.K)]
        self.status = [0] * self.K

    # what a subclass with its own tracker table and C entry points overrides (longtrack.LongTrackLoop, chiptrack.ChipTrackLoop)
    _lib = "gacq_track"                    # the entry points are <_lib>_open, _run_dev, _state and _close

    def _call(self, what, *args):
        return getattr(nat.lib, "%s_%s" % (self._lib, what))(*args)

    @staticmethod
    def _trackers():
        return TRACKERS

    @staticmethod
    def _channel_spec(ch):
        return channel_spec(ch)

    def _open(self):
        h = ctypes.c_void_p()
        nat.check(self._call("open", self.eng._ctx, self._specs, self.K, ctypes.byref(h)), self.eng._ctx)
        return h

    def close(self):
        if self._h:
            self._call("close", self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def state(self, k):
        out = np.zeros(1, dtype=STATE_DTYPE)
        nat.check(self._call("state", self._h, k, out.ctypes.data_as(ctypes.c_void_p)), self.eng._ctx)
        return out[0]

    def _launch(self, xs, bases):
        torch = nat.require_torch()
        # the kernel runs on the context's stream: make that torch's current stream, so that it is ordered after whatever torch work
        # produced the samples (feed()'s torch.cat, the caller's own ops) and the caching allocator cannot recycle them under it
        self.eng.use_torch_stream(torch.device("cuda", self.eng.device))
        ptrs = (ctypes.c_void_p * self.K)()
        base = np.ascontiguousarray(bases, dtype=np.int64)
        avail = np.zeros(self.K, dtype=np.int64)
        keep = []
        for k, x in enumerate(xs):
            if x is None:
                x = torch.zeros(2, dtype=torch.int8, device="cuda:%d" % self.eng.device)
                keep.append(x)
                avail[k] = 0
            else:
                if not (hasattr(x, "is_cuda") and x.is_cuda and x.dtype == torch.int8 and x.dim() == 1 and x.is_contiguous()):
                    raise ValueError("channel %d: samples must be a contiguous 1-D int8 CUDA tensor (interleaved I/Q)" % k)
                avail[k] = x.numel() // 2
            ptrs[k] = x.data_ptr()
        cap = self.max_records
        recs = np.zeros((self.K, cap), dtype=RECORD_DTYPE)
        counts = np.zeros(self.K, dtype=np.int32)
        status = np.zeros(self.K, dtype=np.int32)
        nat.check(self._call("run_dev", self._h, ptrs, base.ctypes.data_as(ctypes.c_void_p), avail.ctypes.data_as(ctypes.c_void_p),
                             self.max_records, recs.ctypes.data_as(ctypes.c_void_p), cap, counts.ctypes.data_as(nat.c_int_p),
                             status.ctypes.data_as(nat.c_int_p)), self.eng._ctx)
        del keep
        out = [recs[k, :counts[k]].copy() for k in range(self.K)]
        for k in range(self.K):
            self.records[k].append(out[k])
            self.status[k] = int(status[k])
        return out

    def run(self, recordings):
        """Track every channel over its whole recording (a list of K int8 CUDA tensors); returns K record arrays (RECORD_DTYPE)."""
        if len(recordings) != self.K:
            raise ValueError("need one recording per channel (%d), got %d" % (self.K, len(recordings)))
        new = [[] for _ in range(self.K)]
        while True:
            got = self._launch(recordings, [0] * self.K)
            for k in range(self.K):
                new[k].append(got[k])
            if all(len(g) == 0 for g in got):
                break
        return [np.concatenate(n) for n in new]

    def feed(self, chunks):
        """Append the next chunk of each channel's recording (a list of K int8 CUDA tensors or None) and track as far as the samples
        allow; the samples a channel's next block still needs are kept on the device for the next call.  Returns the new records."""
        torch = nat.require_torch()
        if len(chunks) != self.K:
            raise ValueError("need one chunk (or None) per channel (%d), got %d" % (self.K, len(chunks)))
        for k, c in enumerate(chunks):
            if c is None:
                continue
            if self._pending[k] is None:
                self._pending[k] = c.contiguous()
            else:
                self._pending[k] = torch.cat([self._pending[k], c])
        new = [[] for _ in range(self.K)]
        while True:
            got = self._launch(self._pending, self._base)
            for k in range(self.K):
                new[k].append(got[k])
            if all(len(g) == 0 for g in got):
                break
        st = [self.state(k) for k in range(self.K)]
        for k in range(self.K):
            p = self._pending[k]
            if p is None:
                continue
            drop = min(int(st[k]["pos"]) - self._base[k], p.numel() // 2)
            if drop > 0:
                self._pending[k] = p[2 * drop:].contiguous()
                self._base[k] += drop
        return [np.concatenate(n) for n in new]


def format_lines(name, recs, chip_rate=None, trackers=TRACKERS):
    """The script's output lines ('%d %f ...' with the 9 or 14 columns of the tracker's entry) from a record array."""
    t = trackers[name]
    cr = float(codes.chip_rate(t.code) if chip_rate is None else chip_rate)
    out = []
    for r in recs:
        p = complex(float(r["p_re"]), float(r["p_im"]))
        v = (int(r["block"]), np.real(p), np.imag(p), float(r["carrier_f"]), float(r["code_f"]) - cr, (180 / np.pi) * np.angle(p),
             float(r["early"]), float(r["prompt"]), float(r["late"]))
        if t.cols == 14:
            v = v + (int(r["code_cyc"]), float(r["code_p"]), int(r["carrier_cyc"]), float(r["carrier_p"]), int(r["samp"]))
            out.append('%d %f %f %f %f %f %f %f %f %d %f %d %f %d' % v)
        else:
            out.append('%d %f %f %f %f %f %f %f %f' % v)
    return out


def load_int8(path, device=0):
    """A recording file (interleaved int8 I/Q) as a device tensor; an odd trailing byte is dropped."""
    torch = nat.require_torch()
    raw = np.fromfile(path, dtype=np.int8)
    raw = raw[:len(raw) // 2 * 2]
    return torch.from_numpy(raw).to("cuda:%d" % device)


def track_file(name, path, fs, coffset, prn, doppler, code_offset, loop_dwells=(500.0, 500.0), carrier_phase=None, engine=None,
               loop=TrackLoop, **loop_args):
    """One script run on one file with the loop class of the script's family: returns (records, output lines), and the chip
    accumulator as well from a loop that has one."""
    ch = Channel(name, fs, coffset, prn, doppler, code_offset, tuple(loop_dwells), carrier_phase)
    eng = engine or acquire.default_engine()
    tl = loop([ch], eng, **loop_args)
    try:
        recs = tl.run([load_int8(path, eng.device)])[0]
        more = (tl.chips(0),) if hasattr(tl, "chips") else ()
    finally:
        tl.close()
    return (recs, format_lines(name, recs, trackers=tl._trackers())) + more
