"""Jammed antenna-array recordings on the GPU (csrc/gacq_scene.hip, gacq_scene_dev): the satellites of ``simulate`` plus tones, chirps,
gated pulses and broadband noise jammers, each waveform spread over M antennas by complex gains, with independent noise per antenna --
raw int8 I/Q (or complex64) rows that ``nulling`` and ``stap`` take, as an exact function of (scene, seed, antenna, absolute sample
index): the same bytes however the recording is cut into calls or into groups of antennas.

    python -m gnss_dsp_tools_amd.scene --fs FS --coffset HZ --seconds T --seed S [--sigma X] [--element E,N,U ...]
           --sat TRACKER,ITEM,AMP,DOPPLER,CODE0[,PERIODS_PER_BIT][@AZ,EL] ... [--tone AMP,HZ[@AZ,EL]]
           [--chirp AMP,F0,F1,SWEEP_SAMPLES[,tri][@AZ,EL]] [--jammer SIGMA[@AZ,EL]] [--gate ON,PERIOD[,FIRST]] OUT0 [OUT1 ...]

writes one int8 file per antenna element (``--element`` east,north,up in wavelengths; none: one antenna at the origin) and prints
``simulate``'s track lines for OUT0.  ``--sat`` is ``simulate``'s; emitter frequencies are in the recording, in Hz; ``--gate`` applies
to the emitter option before it; a source with ``@AZ,EL`` (degrees) reaches element p under exp(2 pi i element_p . u),
u = (cos el sin az, cos el cos az, sin el), a source without it under gain 1 everywhere.

The definition (fixed-point phases, the chirps' closed form, the Philox counters of every antenna and jammer) is in include/gacq.h;
tests/scene_oracle.py restates it in Python integers and fp64."""
import argparse
import ctypes
import sys
from dataclasses import dataclass

import numpy as np

from . import _native as nat
from . import acquire, rawfile, simulate

MAX_ANTENNAS = 8
MAX_EMITTERS = 8
TONE, SAWTOOTH, TRIANGLE, NOISE = 0, 1, 2, 3


SceneEmitter = nat.struct("gacq_scene_emitter")


def _gate(gate):
    """(on, period, first) or None -> the three gate fields"""
    if gate is None:
        return dict(gate_period=0, gate_on=0, gate_first=0)
    on, period, first = gate
    return dict(gate_period=int(period), gate_on=int(on), gate_first=int(first))


@dataclass
class Tone:
    """A continuous wave: ``amp`` per component (LSB), ``hz`` in the recording, ``phase`` in turns at sample 0, ``gate`` = (on, period,
    first) in samples (None: always on)."""
    amp: float
    hz: float
    phase: float = 0.0
    gate: object = None

    def struct(self):
        return SceneEmitter(kind=TONE, amp=float(self.amp), f0_hz=float(self.hz), f1_hz=float(self.hz), phase=float(self.phase), sweep=0, **_gate(self.gate))


@dataclass
class Chirp:
    """A swept wave: the frequency steps once per sample from ``f0`` towards ``f1`` over ``sweep`` samples and starts again (sawtooth),
    or over sweep / 2 samples and back (``triangle``, sweep even)."""
    amp: float
    f0: float
    f1: float
    sweep: int
    triangle: bool = False
    phase: float = 0.0
    gate: object = None

    def struct(self):
        return SceneEmitter(kind=TRIANGLE if self.triangle else SAWTOOTH, amp=float(self.amp), f0_hz=float(self.f0), f1_hz=float(self.f1),
                            phase=float(self.phase), sweep=int(self.sweep), **_gate(self.gate))


@dataclass
class NoiseJammer:
    """Broadband Gaussian noise of ``sigma`` per component: one waveform common to all antennas, a point source."""
    sigma: float
    gate: object = None

    def struct(self):
        return SceneEmitter(kind=NOISE, amp=float(self.sigma), f0_hz=0.0, f1_hz=0.0, phase=0.0, sweep=0, **_gate(self.gate))


def steering(elements, az_deg, el_deg):
    """exp(2 pi i elements . u), complex128 [M]: ``elements`` [M, 3] in wavelengths (east, north, up), the source at azimuth ``az_deg``
    from north towards east and elevation ``el_deg``, u = (cos el sin az, cos el cos az, sin el)"""
    p = np.asarray(elements, dtype=np.float64).reshape(-1, 3)
    az, el = np.deg2rad(float(az_deg)), np.deg2rad(float(el_deg))
    u = np.array([np.cos(el) * np.sin(az), np.cos(el) * np.cos(az), np.sin(el)])
    return np.exp(2j * np.pi * (p @ u))


def recording(sats, emitters, gains, fs, coffset, n, seed, sigma=12.0, j0=0, dtype="int8", first_antenna=0, engine=None):
    """Samples j0 .. j0 + n - 1 of antennas first_antenna .. first_antenna + M - 1 as one contiguous CUDA tensor, int8 [M, 2 n]
    (interleaved I/Q) or complex64 [M, n]: its rows are what nulling and stap take.  ``sats``: simulate.Satellite objects; ``emitters``:
    Tone, Chirp and NoiseJammer objects; ``gains``: complex [M, len(sats) + len(emitters)], row p for antenna first_antenna + p, the
    satellites' columns first.  Asynchronous on torch's current stream."""
    torch = nat.require_torch()
    eng = engine or acquire.default_engine()
    sats, emitters = list(sats), list(emitters)
    K, I = len(sats), len(emitters)
    n, j0 = int(n), int(j0)
    if dtype not in ("int8", "complex64"):
        raise ValueError("dtype must be 'int8' or 'complex64', not %r" % (dtype,))
    g = np.ascontiguousarray(gains, dtype=np.complex128)
    if g.ndim != 2 or g.shape[1] != K + I or not 1 <= g.shape[0] <= MAX_ANTENNAS:
        raise ValueError("gains must be [M, %d] with 1 <= M <= %d, not %r" % (K + I, MAX_ANTENNAS, g.shape))
    M = g.shape[0]
    pairs = [s.struct(coffset) for s in sats]
    sarr = (simulate.SimSat * max(K, 1))(*[p[0] for p in pairs])
    earr = (SceneEmitter * max(I, 1))(*[e.struct() for e in emitters])
    cplx = dtype == "complex64"
    # nothing is allocated for a call the library refuses; the row addresses are checked below, on the rows themselves
    fake = (ctypes.c_void_p * M)(*([16] * M))
    args = (ctypes.addressof(sarr) if K else None, K, ctypes.addressof(earr) if I else None, I, g.ctypes.data if K + I else None, float(fs), float(sigma))
    tail = (int(first_antenna), M, j0, n, int(cplx))
    nat.check(nat.lib.gacq_scene_check(*args, *tail, ctypes.cast(fake, ctypes.c_void_p)))
    out = torch.empty((M, n) if cplx else (M, 2 * n), dtype=torch.complex64 if cplx else torch.int8, device=torch.device("cuda", eng.device))
    eng.use_torch_stream(out.device)
    ptrs = (ctypes.c_void_p * M)(*[out[p].data_ptr() for p in range(M)])
    nat.check(nat.lib.gacq_scene_dev(eng._ctx, *args, int(seed) & (2 ** 64 - 1), *tail, ctypes.cast(ptrs, ctypes.c_void_p)), eng._ctx)
    del pairs
    return out


# ---- command line

def _direction(text, option):
    """'BODY@AZ,EL' -> (BODY, (az, el)); 'BODY' -> (BODY, None)"""
    body, at, tail = text.partition("@")
    if not at:
        return body, None
    try:
        az, el = (float(v) for v in tail.split(","))
    except ValueError:
        raise SystemExit("%s %s: the direction is @AZ,EL in degrees" % (option, text))
    return body, (az, el)


def _numbers(body, option, text, counts):
    f = body.split(",")
    if len(f) not in counts:
        raise SystemExit("%s: wrong number of fields in %r" % (option, text))
    return f


def parse_emitter(option, text):
    """(emitter, direction or None) of one --tone / --chirp / --jammer value"""
    body, direction = _direction(text, option)
    try:
        if option == "--tone":
            f = _numbers(body, option, text, (2,))
            return Tone(float(f[0]), float(f[1])), direction
        if option == "--chirp":
            f = _numbers(body, option, text, (4, 5))
            if len(f) == 5 and f[4] != "tri":
                raise SystemExit("--chirp %s: the fifth field is 'tri' or absent" % text)
            return Chirp(float(f[0]), float(f[1]), float(f[2]), int(f[3]), triangle=len(f) == 5), direction
        f = _numbers(body, option, text, (1,))
        return NoiseJammer(float(f[0])), direction
    except ValueError:
        raise SystemExit("%s %s: a field is not a number" % (option, text))


def parse_gate(text):
    try:
        f = [int(v) for v in text.split(",")]
    except ValueError:
        f = []
    if len(f) not in (2, 3):
        raise SystemExit("--gate needs ON,PERIOD[,FIRST] in samples, got %r" % text)
    return (f[0], f[1], f[2] if len(f) == 3 else 0)


def build_parser():
    ap = argparse.ArgumentParser(prog="scene", description="Synthesize int8 I/Q recordings of a jammed antenna-array scene on the GPU")
    ap.add_argument("--fs", type=float, required=True, help="sample rate, Hz")
    ap.add_argument("--coffset", type=float, required=True, help="carrier offset of the recording, Hz")
    ap.add_argument("--seconds", type=float, required=True, help="length of the recording")
    ap.add_argument("--seed", type=int, required=True, help="noise seed (64 bits); satellite i draws its data bits from seed + i")
    ap.add_argument("--sigma", type=float, default=12.0, help="noise per component and antenna, LSB (default %(default)s)")
    ap.add_argument("--device", type=int, default=0, help="GPU index")
    ap.add_argument("outputs", nargs="+", metavar="OUT", help="one int8 file per antenna element")
    return ap


SOURCE_OPTIONS = ("--sat", "--tone", "--chirp", "--jammer")


def parse(argv):
    """(argparse namespace, [Satellite], [emitter], elements [M, 3], gains [M, K + I]) of a command line.  The source options, --gate
    and --element are read here in the order given, so that a value that begins with '-' is never taken for an option and a gate binds
    to the emitter before it."""
    argv = list(argv)
    rest, sat_texts, emitters, elements = [], [], [], []
    last, i = None, 0
    while i < len(argv):
        opt, eq, val = argv[i].partition("=")
        if opt in SOURCE_OPTIONS + ("--gate", "--element"):
            if not eq:
                if i + 1 >= len(argv):
                    raise SystemExit("%s needs a value" % opt)
                val, i = argv[i + 1], i + 1
            if opt == "--sat":
                sat_texts.append(_direction(val, opt))
                last = None
            elif opt == "--gate":
                if last is None:
                    raise SystemExit("--gate %s follows no --tone, --chirp or --jammer" % val)
                if last[0].gate is not None:
                    raise SystemExit("--gate %s: the emitter before it has a gate already" % val)
                last[0].gate = parse_gate(val)
            elif opt == "--element":
                try:
                    p = [float(v) for v in val.split(",")]
                except ValueError:
                    p = []
                if len(p) != 3:
                    raise SystemExit("--element needs E,N,U in wavelengths, got %r" % val)
                elements.append(p)
            else:
                last = parse_emitter(opt, val)
                emitters.append(last)
        else:
            rest.append(argv[i])
        i += 1
    a = build_parser().parse_args(rest)
    if not (a.fs > 0.0 and a.seconds > 0.0 and a.sigma >= 0.0):
        raise SystemExit("need --fs > 0, --seconds > 0 and --sigma >= 0")
    if len(sat_texts) > simulate.MAX_SATS or len(emitters) > MAX_EMITTERS or not sat_texts and not emitters:
        raise SystemExit("need at most %d --sat and %d emitter options, and one source at the least" % (simulate.MAX_SATS, MAX_EMITTERS))
    elements = np.asarray(elements or [[0.0, 0.0, 0.0]], dtype=np.float64)
    if len(elements) > MAX_ANTENNAS or len(a.outputs) != len(elements):
        raise SystemExit("need one OUT per --element, %d at the most (%d elements, %d files)" % (MAX_ANTENNAS, len(elements), len(a.outputs)))
    sats = [simulate.parse_sat(text, k, a.seed, a.seconds) for k, (text, _) in enumerate(sat_texts)]
    directions = [d for _, d in sat_texts] + [d for _, d in emitters]
    gains = np.ones((len(elements), len(directions)), dtype=np.complex128)
    for e, d in enumerate(directions):
        if d is not None:
            gains[:, e] = steering(elements, d[0], d[1])
    return a, sats, [e for e, _ in emitters], elements, gains


def run(argv, out=sys.stdout, piece_bytes=rawfile.PIECE_BYTES):
    a, sats, emitters, elements, gains = parse(argv)
    n = int(a.fs * a.seconds)
    piece = max(1, int(piece_bytes) // 2)
    eng = acquire.Engine(a.device)
    files = []
    try:
        for path in a.outputs:
            files.append(open(path, "wb"))
        for j0 in range(0, n, piece):
            x = recording(sats, emitters, gains, a.fs, a.coffset, min(piece, n - j0), a.seed, a.sigma, j0, "int8", 0, eng).cpu().numpy()
            for p, f in enumerate(files):
                x[p].tofile(f)
    finally:
        for f in files:
            f.close()
        eng.close()
    lines = [simulate.track_line(s, a.outputs[0], a.fs, a.coffset) for s in sats]
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
