"""The reference's squaring.py on the GPU: the squaring-loop carrier detector.

    squaring.py:28-40               per chunk of b*n*m samples: carrier-offset wipe-off, squaring, the int16 stream
    gnsstools/squaring.py:14-23     decimate by n (boxcar), square, m incoherent sums
    gnsstools/nco.py:30-41          the fixed-point table NCO

One launch of gacq_squaring_int8_dev (gacq_spectrum.hip) covers every chunk of an upload, in the complex128 arithmetic of the
compiled (numba) program.  The per-chunk NCO start phases are formed here in fp64 with the script's own expressions.

    python -m gnss_dsp_tools_amd.squaring FILE FS COFFSET | baudline -reset -stdin ...        (squaring.py:12)
"""
import ctypes
import sys

import numpy as np

from . import _native as nat
from . import acquire, rawfile

B, N, M = 1000, 16, 100        # squaring.py:22-24


def chunk_phases(nchunks, chunk, fs, coffset, phase=0.0):
    """coffset_phase at the start of each of nchunks chunks of `chunk` samples, and the phase after the last (squaring.py:20,33-35)."""
    out = np.empty(nchunks, dtype=np.float64)
    coffset_phase = phase
    for c in range(nchunks):
        out[c] = coffset_phase
        coffset_phase = coffset_phase - chunk * coffset / fs
        coffset_phase = np.mod(coffset_phase, 1)
    return out, float(coffset_phase)


def squaring_dev(iq_int8, fs, coffset, b=B, n=N, m=M, engine=None, phase=0.0):
    """(r complex128 [chunks, b], int16 stream [chunks, 2 b], clamped count [1] uint64, phase after the last chunk), the arrays as CUDA tensors."""
    torch = nat.require_torch()
    eng = engine or acquire.default_engine()
    b, n, m = int(b), int(n), int(m)
    if b < 1 or n < 1 or m < 1:
        raise ValueError("b, n and m must be positive")
    fs, coffset = float(fs), float(coffset)
    x = rawfile.device_int8(eng, iq_int8)
    chunk = b * n * m
    nchunks = (x.numel() // 2) // chunk         # a trailing partial chunk is dropped (squaring.py:29-31)
    r = torch.empty((nchunks, b), dtype=torch.complex128, device=x.device)
    y = torch.empty((nchunks, 2 * b), dtype=torch.int16, device=x.device)
    clamped = torch.zeros(1, dtype=torch.int64, device=x.device)
    if nchunks == 0:
        return r, y, clamped, float(phase)
    ph, after = chunk_phases(nchunks, chunk, fs, coffset, phase)
    d_ph = torch.from_numpy(ph).to(x.device)
    nat.check(nat.lib.gacq_squaring_int8_dev(eng._ctx, ctypes.c_void_p(x.data_ptr()), nchunks, chunk, n, m, ctypes.c_void_p(d_ph.data_ptr()),
                                             -coffset / fs, ctypes.c_void_p(r.data_ptr()), ctypes.c_void_p(y.data_ptr()),
                                             ctypes.c_void_p(clamped.data_ptr())), eng._ctx)
    return r, y, clamped, after


def squaring(iq_int8, fs, coffset, b=B, n=N, m=M, engine=None, phase=0.0):
    """r (complex128 [chunks, b]), the script's int16 stream (flat: round(20 re), round(20 im) interleaved, chunk after chunk) and the
    number of stream values that had to be clamped to the int16 range.  iq_int8 as for spectrum.psd; phase: coffset_phase at the start."""
    r, y, clamped, _ = squaring_dev(iq_int8, fs, coffset, b, n, m, engine, phase)
    return r.cpu().numpy(), y.cpu().numpy().reshape(-1), int(clamped.item())


def parse(argv):
    """FILE FS COFFSET, read as the script reads sys.argv[1:4] (no option parser: COFFSET may be negative, in any float spelling)"""
    import argparse
    argv = list(argv)
    if len(argv) != 3:
        print("usage: python -m gnss_dsp_tools_amd.squaring FILE FS COFFSET", file=sys.stderr)
        raise SystemExit(2)
    return argparse.Namespace(filename=argv[0], fs=float(argv[1]), coffset=float(argv[2]))


def run(argv, out=None, engine=None):
    """Writes the stream to `out` (a binary file; default: stdout) chunk by chunk; returns (chunks, clamped)."""
    a = parse(argv)
    out = out or sys.stdout.buffer
    phase, chunks, clamped = 0.0, 0, 0
    with open(a.filename, "rb") as fp:
        for piece in rawfile.read_pieces(fp, 2 * B * N * M):
            r, y, c, phase = squaring_dev(piece, a.fs, a.coffset, engine=engine, phase=phase)
            out.write(y.cpu().numpy().tobytes())
            out.flush()
            chunks += r.shape[0]
            clamped += int(c.item())
    if clamped:
        print("squaring: %d values clamped to the int16 range" % clamped, file=sys.stderr)
    return chunks, clamped


if __name__ == "__main__":
    run(sys.argv[1:])
