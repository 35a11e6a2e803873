"""fp64 numpy restatements of the utilities (checkers only): the Welch spectrum of spectrum.py, the squaring detector in the
complex128 arithmetic of the compiled reference, the C/N0 estimate.  Written from the reference's behaviour, vectorised; nothing here
is used by the package."""
import numpy as np

NT = 1024


def psd_fp64(iq_int8, n, ns):
    """dB frames [F, n]: Hann window (symmetric), complex128 FFT, mean of |z|^2 over ns blocks, fftshift, 10 log10"""
    s = np.asarray(iq_int8, dtype=np.int8).reshape(-1, 2).astype(np.float64)
    F = len(s) // (n * ns)
    x = (s[:F * n * ns, 0] + 1j * s[:F * n * ns, 1]).reshape(F, ns, n)
    z = np.fft.fft(x * np.hanning(n), axis=2)
    p = (z.real ** 2 + z.imag ** 2).sum(axis=1) / ns
    with np.errstate(divide="ignore"):
        return 10 * np.log10(np.fft.fftshift(p, axes=1))


def chunk_phase_sequence(nchunks, chunk, fs, coffset):
    """start phase of every chunk: 0, then minus chunk * coffset / fs modulo 1, chunk after chunk"""
    out, p = [], 0.0
    for _ in range(nchunks):
        out.append(p)
        p = np.mod(p - chunk * coffset / fs, 1)
    return np.array(out, dtype=np.float64)


def mix_fixed(x_c64, f, p):
    """table NCO with a 50-bit fixed-point phase in wrapping 64-bit arithmetic; the complex128 product rounded to complex64"""
    tab = np.exp(2 * np.pi * 1j * np.arange(NT) * (1.0 / NT))
    dp = np.uint64(int(np.floor(p * NT * (1 << 50))) % (1 << 64))
    df = np.uint64(int(np.floor(f * NT * (1 << 50))) % (1 << 64))
    with np.errstate(over="ignore"):
        ph = dp + np.arange(len(x_c64), dtype=np.uint64) * df
    idx = ((ph >> np.uint64(50)) & np.uint64(NT - 1)).astype(np.int64)
    return (x_c64.astype(np.complex128) * tab[idx]).astype(np.complex64)


def squaring_fp64(iq_int8, fs, coffset, b, n, m):
    """(r complex128 [chunks, b], int16 stream, values outside the int16 range)"""
    s = np.asarray(iq_int8, dtype=np.int8).reshape(-1, 2)
    chunk = b * n * m
    chunks = len(s) // chunk
    phases = chunk_phase_sequence(chunks, chunk, fs, coffset)
    r = np.empty((chunks, b), dtype=np.complex128)
    for c in range(chunks):
        part = s[c * chunk:(c + 1) * chunk]
        x = np.empty(chunk, dtype=np.complex64)
        x.real, x.imag = part[:, 0], part[:, 1]
        y = mix_fixed(x, -coffset / fs, phases[c]).astype(np.complex128).reshape(b, m, n)
        box = y.sum(axis=2)
        r[c] = (box * box / n).sum(axis=1)
    v = np.empty((chunks, 2 * b))
    v[:, 0::2], v[:, 1::2] = np.round(20 * r.real), np.round(20 * r.imag)
    clamped = int(np.sum((v > 32767) | (v < -32768)))
    return r, np.clip(v, -32768, 32767).astype(np.int16).reshape(-1), clamped


def cn0_lines(lines, time_ms):
    """'%.2f' per whole block of time_ms track lines: 20 log10(mean |I| / (sqrt 2 std Q)) + 30, population standard deviation"""
    cols = np.array([[float(t) for t in ln.split()[1:3]] for ln in lines]).reshape(-1, 2)
    out = []
    for k in range(0, len(cols) - time_ms + 1, time_ms):
        i, q = cols[k:k + time_ms, 0], cols[k:k + time_ms, 1]
        out.append("%.2f" % (20 * np.log10(np.mean(np.abs(i)) / (np.sqrt(2) * np.std(q))) + 30))
    return out
