"""Interference mitigation on the GPU (csrc/gacq_mitigate.hip, gacq_mitigate_dev): a time-domain pulse blanker and a frequency-domain
excision filter with a per-frame median threshold, on the canonical recording -- interleaved int8 I/Q or complex64 in, int8 I/Q or
complex64 out -- to put in front of acquire, scan, handoff, refine and the tracking loops.  Every decision is a function of the
absolute sample index: a recording converts to the same bytes however it is cut into calls or chunks.

    python -m gnss_dsp_tools_amd.mitigate [--blank T] [--hold H] [--nfft N] [--ratio C] [--guard G] [--no-excise] [--in-complex64]
           [--gain G | --target-rms R] [--complex64] IN OUT

reads IN (or - for stdin), writes OUT (or - for stdout) and prints one line (to stderr when OUT is -):

    gain <G> samples <N> blanked <fraction of samples> excised <mean fraction of bins>

--blank T: samples with |x| > T and H (default 2) samples on either side are zeroed (default: no blanking).  Excision (on unless
--no-excise): frames of N (default 1024) samples, overlapping by half under a sine window; bins whose power exceeds C (default 12)
times the frame's lower-median power, and G (default 2) bins on either side, are zeroed.  Without --gain the gain is target_rms
(default 32) over the rms of the first 65536 output samples at gain 1.  The sample rate and the carrier offset are those of IN.  A
recording ends at the last output block whose support is present: up to 3 N / 2 + H samples at the end of IN give no output.
Limits: the median is the noise floor only while less than half the band is jammed; bins are zeroed, not clipped; the sine
window's sidelobes make a strong CW cost tens of bins.  The definition is in include/gacq.h; tests/mitigate_oracle.py restates it."""
import argparse
import ctypes
import math
import sys

import numpy as np

from . import _native as nat
from . import ingest, rawfile, streaming

MAX_HOLD, MAX_GUARD = 64, 8
AUTO_SAMPLES = ingest.AUTO_SAMPLES
TARGET_RMS = ingest.TARGET_RMS


MitigateCfg = nat.struct("gacq_mitigate_cfg")


class Config:
    """Config(blank=None, hold=2, nfft=1024, ratio=12.0, guard=2): blank None (or 0) turns blanking off, nfft 0 or ratio None excision."""

    def __init__(self, blank=None, hold=2, nfft=1024, ratio=12.0, guard=2):
        self.blank = 0.0 if blank is None else float(blank)
        self.hold, self.guard = int(hold), int(guard)
        self.nfft = 0 if (ratio is None or not nfft) else int(nfft)
        self.ratio = 0.0 if ratio is None else float(ratio)

    def struct(self):
        return MitigateCfg(blank_thr=self.blank, ratio=self.ratio, hold=self.hold, nfft=self.nfft, guard=self.guard)

    def out_range(self, in_first, in_count):
        """(first, count) of the output samples that input samples in_first .. in_first + in_count - 1 support"""
        end = in_first + in_count
        if self.nfft:
            h = self.nfft // 2
            qlo = 0 if in_first == 0 else -(-(in_first + self.hold) // h) + 1
            qhi = (end - self.hold) // h - 2
            return qlo * h, max(0, (qhi + 1 - qlo) * h)
        first = 0 if in_first == 0 else in_first + self.hold
        return first, max(0, end - self.hold - first)

    def first_needed(self, out):
        """the first input sample that output `out` needs"""
        if self.nfft:
            h = self.nfft // 2
            return max(0, (out // h - 1) * h - self.hold)
        return max(0, out - self.hold)


class Stats:
    """blanked samples, owned frames, zeroed bins and, per owned frame, its zeroed bins (numpy uint32)"""

    def __init__(self, blanked=0, frames=0, bins=0, frame_bins=None):
        self.blanked, self.frames, self.bins = int(blanked), int(frames), int(bins)
        self.frame_bins = np.zeros(0, dtype=np.uint32) if frame_bins is None else frame_bins


def _device_input(engine, data, in_complex64):
    """(tensor, complex64?) : a flat int8 or complex64 CUDA tensor as it is; a uint8 CUDA tensor or a bytes-like object as the bytes of
    int8 pairs, or of complex64 samples with in_complex64"""
    d = streaming.device_flat(engine, data, ("int8", "uint8", "complex64"), "data must be a flat int8, uint8 or complex64 CUDA tensor or a bytes-like object")
    torch = nat.require_torch()
    if torch.is_tensor(data):
        return d, (d.dtype == torch.complex64 or (d.dtype == torch.uint8 and bool(in_complex64)))
    return d, bool(in_complex64) or (isinstance(data, np.ndarray) and data.dtype == np.complex64)


def _count(d, cplx):
    return d.numel() if d.dtype.is_complex else d.numel() // (8 if cplx else 2)


def apply(engine, cfg, data, gain, in_first=0, out_first=None, n_out=None, dtype="int8", stats=False, in_complex64=False):
    """Output samples out_first .. out_first + n_out - 1 of the recording whose input samples in_first .. are at `data` (a flat int8
    or complex64 CUDA tensor, or bytes: of int8 pairs, of complex64 samples with in_complex64): a flat int8 CUDA tensor [2 n_out] of
    interleaved I/Q, or complex64 [n_out]; with stats, (that, Stats).  By default every output sample the data supports.
    Asynchronous on torch's current stream (reading the statistics waits for it)."""
    torch = nat.require_torch()
    d, in_c = _device_input(engine, data, in_complex64)
    in_first = int(in_first)
    in_count = _count(d, in_c)
    first, count = cfg.out_range(in_first, in_count)
    out_first = first if out_first is None else int(out_first)
    n_out = max(0, first + count - out_first) if n_out is None else int(n_out)
    cplx, out = streaming.iq_out(n_out, dtype, d.device)
    st = fb = None
    if stats:
        nfr = 0
        if cfg.nfft and n_out > 0:
            h = cfg.nfft // 2
            nfr = max(0, (out_first + n_out - 1) // h - (-(-out_first // h)) + 1)
        st = torch.zeros(3, dtype=torch.int64, device=d.device)
        fb = torch.zeros(max(nfr, 1), dtype=torch.int32, device=d.device)
    c = cfg.struct()
    streaming.launch(engine, [d], d.numel(), out, n_out, lambda src, dst: nat.check(
        nat.lib.gacq_mitigate_dev(engine._ctx, ctypes.addressof(c), ctypes.c_void_p(src[0]), int(in_c), in_first, in_count, out_first, n_out, float(gain),
                                  int(cplx), ctypes.c_void_p(dst), ctypes.c_void_p(st.data_ptr() if stats else 0),
                                  ctypes.c_void_p(fb.data_ptr() if stats else 0)), engine._ctx))
    if not stats:
        return out
    s = st.cpu().numpy()
    return out, Stats(s[0], s[1], s[2], fb.cpu().numpy().view(np.uint32)[:int(s[1])].copy())


def auto_gain(engine, cfg, first_piece, target_rms=TARGET_RMS, in_complex64=False):
    """target_rms over the rms of the first P output samples at gain 1, P = min(what first_piece supports, 65536): the rule and the
    rms_gain of ingest.py, evaluated on the host from the device's own complex64 output."""
    d, in_c = _device_input(engine, first_piece, in_complex64)
    first, count = cfg.out_range(0, _count(d, in_c))
    p = min(count, AUTO_SAMPLES)
    if p < 1:
        raise ValueError("automatic gain: the first piece holds no whole output sample")
    return ingest.rms_gain(apply(engine, cfg, d, 1.0, 0, 0, p, "complex64", in_complex64=in_c).cpu().numpy(), target_rms)


class Mitigate(streaming.Chunks):
    """A recording fed chunk by chunk (bytes or uint8 / int8 / complex64 CUDA tensors): feed(chunk) returns the output samples the
    chunk completes, and the concatenation of what the calls return is what one apply() of the whole recording gives.  The input tail
    under the next output block's support, and the bytes of a sample that a chunk cut, stay on the device.  blanked, frames and bins
    are the running totals."""

    def __init__(self, engine, cfg, gain, dtype="int8", in_complex64=False):
        self.engine, self.cfg, self.gain, self.dtype, self.in_complex64 = engine, cfg, float(gain), dtype, bool(in_complex64)
        self.blanked = self.frames = self.bins = 0
        super().__init__(64 if self.in_complex64 else 16, lambda in_first, in_count: sum(cfg.out_range(in_first, in_count)), self._run, cfg.first_needed)

    def _run(self, ds, in_first, in_count, out_first, n_out, k):
        x = ds[0] if self.in_complex64 else ds[0].view(nat.require_torch().int8)
        out, st = apply(self.engine, self.cfg, x, self.gain, in_first, out_first, n_out, self.dtype, True, self.in_complex64)
        self.blanked, self.frames, self.bins = self.blanked + st.blanked, self.frames + st.frames, self.bins + st.bins
        return out

    def feed(self, chunk):
        torch = nat.require_torch()
        d, _ = _device_input(self.engine, chunk, self.in_complex64)
        return self.feed_all([(torch.view_as_real(d).reshape(-1) if d.dtype.is_complex else d).view(torch.uint8)])


def mitigate_file(engine, cfg, fin, fout, gain=None, target_rms=TARGET_RMS, dtype="int8", in_complex64=False, piece_bytes=rawfile.PIECE_BYTES):
    """Filter the open binary file fin into fout piece by piece; gain None: the automatic gain of the first piece.
    (gain, samples, Mitigate with the totals)."""
    unit = 8 if in_complex64 else 2
    mit = None

    def start(held):
        nonlocal gain, mit
        if gain is None:                        # the first 65536 outputs need at most 65536 + 3 N / 2 + 2 hold inputs
            gain = auto_gain(engine, cfg, held[0].view(np.uint8)[:(AUTO_SAMPLES + 2 * 4096 + 2 * MAX_HOLD) * unit], target_rms, in_complex64)
        mit = Mitigate(engine, cfg, gain, dtype, in_complex64)
        return lambda piece: [mit.feed(piece.view(np.uint8))]

    n = streaming.pump(rawfile.read_pieces(fin, unit, piece_bytes), start, [fout], 2 if dtype == "int8" else 1)
    if n is None:
        raise ValueError("the input holds no whole sample")
    return float(gain), n[0], mit


def build_parser():
    ap = argparse.ArgumentParser(prog="mitigate", description="Pulse blanking and spectral excision of an int8 I/Q (or complex64) recording on the GPU")
    ap.add_argument("--blank", type=float, default=None, help="blank samples whose magnitude exceeds this (default: no blanking)")
    ap.add_argument("--hold", type=int, default=2, help="samples blanked on either side of a hit, 0..64 (default %(default)s)")
    ap.add_argument("--nfft", type=int, default=1024, help="excision frame length, a power of two in 64..4096 (default %(default)s)")
    ap.add_argument("--ratio", type=float, default=12.0, help="excise bins above this times the frame's median power (default %(default)s)")
    ap.add_argument("--guard", type=int, default=2, help="bins zeroed on either side of a hit bin, 0..8 (default %(default)s)")
    ap.add_argument("--no-excise", action="store_true", help="blanking only")
    ap.add_argument("--in-complex64", action="store_true", help="IN holds complex64 samples instead of int8 pairs")
    g = ap.add_mutually_exclusive_group()
    g.add_argument("--gain", type=float, default=None, help="gain (default: automatic)")
    g.add_argument("--target-rms", type=float, default=TARGET_RMS, help="rms the automatic gain aims at (default %(default)s)")
    ap.add_argument("--complex64", action="store_true", help="write complex64 instead of int8")
    ap.add_argument("--device", type=int, default=0, help="GPU index")
    ap.add_argument("input_filename")
    ap.add_argument("output_filename")
    return ap


def parse(argv):
    """(argparse namespace, Config) of a command line"""
    a = build_parser().parse_args(list(argv))
    nfft = 0 if a.no_excise else a.nfft
    bad = None
    if a.blank is not None and not (a.blank > 0.0 and math.isfinite(a.blank)):
        bad = "--blank must be positive and finite"
    elif not 0 <= a.hold <= MAX_HOLD or not 0 <= a.guard <= MAX_GUARD:
        bad = "--hold lies in 0..%d and --guard in 0..%d" % (MAX_HOLD, MAX_GUARD)
    elif nfft and (nfft < 64 or nfft > 4096 or nfft & (nfft - 1)):
        bad = "--nfft must be a power of two in 64..4096"
    elif nfft and not (a.ratio > 1.0 and math.isfinite(a.ratio)):
        bad = "--ratio must be finite and above 1"
    elif not nfft and a.blank is None:
        bad = "--no-excise needs --blank: both stages would be off"
    elif (a.gain is not None and not streaming.positive_finite(a.gain)) or not streaming.positive_finite(a.target_rms):
        bad = "need a positive, finite --gain / --target-rms"
    if bad:
        raise SystemExit("mitigate: %s" % bad)
    return a, Config(a.blank, a.hold, nfft, a.ratio, a.guard)


def report_line(cfg, gain, samples, blanked, frames, bins):
    excised = bins / float(frames * cfg.nfft) if frames and cfg.nfft else 0.0
    return "gain %r samples %d blanked %r excised %r" % (float(gain), int(samples), (blanked / float(samples)) if samples else 0.0, excised)


def run(argv, out=None, piece_bytes=rawfile.PIECE_BYTES):
    a, cfg = parse(argv)
    with streaming.shell(a.device, [a.input_filename], [a.output_filename], report=out) as sh:
        gain, n, mit = mitigate_file(sh.engine, cfg, sh.fins[0], sh.fouts[0], a.gain, a.target_rms, "complex64" if a.complex64 else "int8", a.in_complex64,
                                     piece_bytes)
    line = report_line(cfg, gain, n, mit.blanked, mit.frames, mit.bins)
    print(line, file=sh.report)
    return line


def main(argv=None):
    return streaming.main(argv, __doc__, run)


if __name__ == "__main__":
    sys.exit(main())
