"""Synthetic multi-satellite recordings on the GPU (csrc/gacq_simulate.hip, gacq_simulate_dev): raw int8 I/Q (or complex64) of any
tracker's signal, at any sample rate, as an exact function of (scene, seed, absolute sample index) -- the same bytes however the
recording is cut into calls, so a scene can be generated piece by piece, on the device, next to the acquisition and the trackers.

    python -m gnss_dsp_tools_amd.simulate --fs FS --coffset HZ --seconds T --seed S [--sigma X]
           --sat TRACKER,ITEM,AMP,DOPPLER,CODE0[,PERIODS_PER_BIT] ... OUT

writes the int8 file OUT and prints, per satellite, the arguments of ``python -m gnss_dsp_tools_amd.track`` that track it:

    <tracker> OUT FS COFFSET ITEM DOPPLER CODE0

A satellite is modelled as the trackers and the correlation grid model one: carrier = coffset (+ the FDMA channel offset of GLONASS
L1/L2) + doppler, code rate = chip_rate + doppler / (carrier / code ratio), chip weight of the tracker's correlator kind.  The carrier
frequency is held to a 2^-64 turn per sample grid: what is produced differs from the request by less than fs * 2^-53 Hz (for a
carrier within +-fs; beyond, by the rounding of carrier / fs in fp64).  The definition (fixed-point phases, Philox4x32-10 noise,
Box-Muller) is in include/gacq.h; tests/simulate_oracle.py restates it in Python integers and fp64."""
import argparse
import ctypes
import sys
from dataclasses import dataclass

import numpy as np

from . import _native as nat
from . import acquire, chiptrack, codes, longtrack, rawfile, secondary, trackloop

MAX_SATS = 32
MAX_SYMBOLS = 1 << 20
MAX_INDEX = 1 << 48


SimSat = nat.struct("gacq_sim_sat")


def tracker(name):
    """The Tracker entry of any tracker name: the template family, the long-code trackers, the chip trackers."""
    for table in (trackloop.TRACKERS, longtrack.LONG_TRACKERS, chiptrack.CHIP_TRACKERS):
        if name in table:
            return table[name]
    raise KeyError("unknown tracker %r (the trackers: %s)" % (name, ", ".join(sorted(
        {**trackloop.TRACKERS, **longtrack.LONG_TRACKERS, **chiptrack.CHIP_TRACKERS}))))


@dataclass
class Satellite:
    """One satellite of a scene: ``item`` is the PRN, or the RF channel for GLONASS L1/L2; ``amp`` the amplitude per component (LSB);
    ``doppler`` in Hz on top of the recording's carrier offset; ``code0`` the code phase at sample 0 in chips; ``carrier_phase`` in
    turns at sample 0; ``symbols``: +-1 values, one per ``periods_per_symbol`` code periods, repeated cyclically (None: all +1)."""
    tracker: str
    item: int
    amp: float
    doppler: float
    code0: float
    carrier_phase: float = 0.0
    symbols: object = None
    periods_per_symbol: int = 1

    def carrier_hz(self, coffset):
        t = tracker(self.tracker)
        return float(coffset) + (t.glonass[3] * int(self.item) if t.glonass else 0.0) + float(self.doppler)

    def code_rate_hz(self):
        t = tracker(self.tracker)
        return float(codes.chip_rate(t.code)) + float(self.doppler) / t.scale(int(self.item))

    def struct(self, coffset):
        """(gacq_sim_sat, the int8 symbol array it points to or None): keep the second alive as long as the first is in use"""
        t = tracker(self.tracker)
        sym = None
        if self.symbols is not None:
            sym = np.ascontiguousarray(self.symbols, dtype=np.int8).reshape(-1)
        s = SimSat(code=t.code.encode(), prn=0 if t.glonass else int(self.item), kind=int(t.kind), periods_per_symbol=int(self.periods_per_symbol),
                   nsym=0 if sym is None else len(sym), pad=0, symbols=None if sym is None or len(sym) == 0 else sym.ctypes.data,
                   amp=float(self.amp), carrier_hz=self.carrier_hz(coffset), carrier_phase=float(self.carrier_phase),
                   code_rate_hz=self.code_rate_hz(), code_phase=float(self.code0))
        return s, sym


def symbols(tracker_name, item, nbits, periods_per_bit, seed):
    """One +-1 value per code period, nbits * periods_per_bit of them (use with periods_per_symbol = 1): the built-in overlay code of
    secondary.SECONDARY for the tracker's code, where there is one, repeated from period 0, times data bits of periods_per_bit
    periods each drawn from PCG64(seed).  int8."""
    t = tracker(tracker_name)
    nbits, ppb = int(nbits), int(periods_per_bit)
    if nbits < 1 or ppb < 1 or nbits * ppb > MAX_SYMBOLS:
        raise ValueError("need nbits >= 1, periods_per_bit >= 1 and at most %d periods" % MAX_SYMBOLS)
    bits = 1 - 2 * np.random.Generator(np.random.PCG64(int(seed))).integers(0, 2, size=nbits)
    out = np.repeat(bits, ppb).astype(np.int8)
    sec = secondary.SECONDARY.get(t.code)
    if isinstance(sec, dict):
        sec = sec.get(int(item))
    if sec is not None:
        out = (out * np.resize(sec, len(out))).astype(np.int8)
    return out


def recording(sats, fs, coffset, n, seed, sigma=12.0, j0=0, dtype="int8", engine=None, out=None):
    """Samples j0 .. j0 + n - 1 of the scene as a flat CUDA tensor: int8 [2 n] (interleaved I/Q) or complex64 [n].  ``out``: a
    contiguous tensor of that shape and type to write into.  Asynchronous on torch's current stream."""
    torch = nat.require_torch()
    eng = engine or acquire.default_engine()
    sats = list(sats)
    n, j0 = int(n), int(j0)
    if dtype not in ("int8", "complex64"):
        raise ValueError("dtype must be 'int8' or 'complex64', not %r" % (dtype,))
    # what gacq_simulate_dev refuses for the call as a whole, here too: nothing is allocated for it
    if not 1 <= len(sats) <= MAX_SATS:
        raise ValueError("need 1..%d satellites, got %d" % (MAX_SATS, len(sats)))
    if n < 1 or j0 < 0 or j0 + n > MAX_INDEX:
        raise ValueError("need n >= 1, j0 >= 0 and j0 + n <= 2^48 (j0 %d, n %d)" % (j0, n))
    cplx = dtype == "complex64"
    tdtype, numel = (torch.complex64, n) if cplx else (torch.int8, 2 * n)
    device = torch.device("cuda", eng.device)
    if out is None:
        out = torch.empty(numel, dtype=tdtype, device=device)
    elif not (torch.is_tensor(out) and out.is_cuda and out.dtype == tdtype and out.dim() == 1 and out.numel() == numel and out.is_contiguous()):
        raise ValueError("out must be a contiguous 1-D %s CUDA tensor of %d elements" % (dtype, numel))
    eng.use_torch_stream(device)
    pairs = [s.struct(coffset) for s in sats]
    arr = (SimSat * len(pairs))(*[p[0] for p in pairs])
    nat.check(nat.lib.gacq_simulate_dev(eng._ctx, ctypes.addressof(arr), len(pairs), float(fs), float(sigma), int(seed) & (2 ** 64 - 1), j0, n,
                                        int(cplx), ctypes.c_void_p(out.data_ptr())), eng._ctx)
    del pairs
    return out


def parse_sat(text, index, seed, seconds):
    """--sat TRACKER,ITEM,AMP,DOPPLER,CODE0[,PERIODS_PER_BIT] -> Satellite; with PERIODS_PER_BIT, data bits (and the built-in overlay)
    from symbols() with seed + index, enough for `seconds` (repeated cyclically beyond 2^20 periods)"""
    f = text.split(",")
    if len(f) not in (5, 6):
        raise SystemExit("--sat needs TRACKER,ITEM,AMP,DOPPLER,CODE0[,PERIODS_PER_BIT], got %r" % text)
    try:
        t = tracker(f[0])
    except KeyError as e:
        raise SystemExit(str(e.args[0]))
    sat = Satellite(f[0], int(f[1]), float(f[2]), float(f[3]), float(f[4]))
    if len(f) == 6:
        ppb = int(f[5])
        if ppb < 1:
            raise SystemExit("--sat %s: PERIODS_PER_BIT must be at least 1" % text)
        periods = int(seconds * sat.code_rate_hz() / codes.code_length(t.code)) + 2
        nbits = max(1, min(-(-periods // ppb), MAX_SYMBOLS // ppb))
        sat.symbols = symbols(f[0], sat.item, nbits, ppb, int(seed) + index)
    return sat


def build_parser():
    ap = argparse.ArgumentParser(prog="simulate", description="Synthesize an int8 I/Q recording of a scene on the GPU")
    ap.add_argument("--fs", type=float, required=True, help="sample rate, Hz")
    ap.add_argument("--coffset", type=float, required=True, help="carrier offset of the recording, Hz")
    ap.add_argument("--seconds", type=float, required=True, help="length of the recording")
    ap.add_argument("--seed", type=int, required=True, help="noise seed (64 bits); satellite i draws its data bits from seed + i")
    ap.add_argument("--sigma", type=float, default=12.0, help="noise per component, LSB (default %(default)s)")
    ap.add_argument("--device", type=int, default=0, help="GPU index")
    ap.add_argument("--sat", action="append", default=[], metavar="TRACKER,ITEM,AMP,DOPPLER,CODE0[,PERIODS_PER_BIT]",
                    help="one satellite; may be given up to %d times" % MAX_SATS)
    ap.add_argument("output_filename")
    return ap


def parse(argv):
    """(argparse namespace, [Satellite]) of a command line"""
    a = build_parser().parse_args(_join_sat(list(argv)))
    if not 1 <= len(a.sat) <= MAX_SATS:
        raise SystemExit("need 1..%d --sat options, got %d" % (MAX_SATS, len(a.sat)))
    if not (a.fs > 0.0 and a.seconds > 0.0 and a.sigma >= 0.0):
        raise SystemExit("need --fs > 0, --seconds > 0 and --sigma >= 0")
    return a, [parse_sat(text, i, a.seed, a.seconds) for i, text in enumerate(a.sat)]


def _join_sat(argv):
    """'--sat X' -> '--sat=X', so that a value is never taken for an option"""
    out, i = [], 0
    while i < len(argv):
        if argv[i] == "--sat" and i + 1 < len(argv):
            out.append("--sat=" + argv[i + 1])
            i += 2
        else:
            out.append(argv[i])
            i += 1
    return out


def track_line(sat, path, fs, coffset):
    """The arguments of python -m gnss_dsp_tools_amd.track for this satellite of the file"""
    return "%s %s %r %r %d %r %r" % (sat.tracker, path, float(fs), float(coffset), int(sat.item), float(sat.doppler), float(sat.code0))


def run(argv, out=sys.stdout, piece_bytes=rawfile.PIECE_BYTES):
    a, sats = parse(argv)
    n = int(a.fs * a.seconds)
    piece = max(1, int(piece_bytes) // 2)
    eng = acquire.Engine(a.device)
    try:
        with open(a.output_filename, "wb") as f:
            for j0 in range(0, n, piece):
                x = recording(sats, a.fs, a.coffset, min(piece, n - j0), a.seed, a.sigma, j0, "int8", eng)
                x.cpu().numpy().tofile(f)
    finally:
        eng.close()
    lines = [track_line(s, a.output_filename, a.fs, a.coffset) for s in sats]
    for line in lines:
        print(line, file=out)
    return lines


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    if not argv or argv[0] in ("-h", "--help"):
        print(__doc__)
        return 0
    run(argv)
    return 0


if __name__ == "__main__":
    sys.exit(main())
