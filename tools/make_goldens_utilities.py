#!/usr/bin/env python3
"""Generate tests/golden/utilities_cases.json.gz by RUNNING THE REFERENCE, unmodified, on the seeded recordings of
tests/utilities_cases.py (written to a temporary directory, never committed):

  spectrum   `<reference>/spectrum.py FILE FC FS N NS` as a subprocess.  The script only plots, so a stand-in `matplotlib` package
             (written to the temporary directory, first on PYTHONPATH) records every array handed to the plot line's set_ydata: these
             are the expected dB frames.  Stored with them: the deviation of a CPU complex64 transform (scipy.fft on complex64 input,
             fp64 power sums -- the device kernel's arithmetic) from those frames; the GPU test's tolerance is four times it.
  squaring   gnsstools.nco.mix + gnsstools.squaring.squaring imported from the reference and called chunk by chunk for r; for the
             script's own (b, n, m) also `<reference>/squaring.py FILE FS COFFSET` as a subprocess for the int16 stream on its stdout.
             Without numba the reference's inner sum runs in complex64; the device implements the compiled program's complex128, so
             the measured difference to the fp64 restatement (tests/utilities_oracle.py) is stored and bounds the comparison.
  cn0        `<reference>/cn0.py [--time MS]` as a subprocess on the stdout lines of the golden track cases and on a seeded track.

Asserted here, so that the tests can be tight without being unsatisfiable: no 20 r of the restatement within 1e-6 of a half-integer;
nothing clamped; the reference's own stream within the half-integer share the tests allow; no C/N0 value within 1e-6 of a '%.2f'
rounding boundary.  Re-running must leave `git diff tests/golden/` empty.  Needs the reference checkout, scipy and no GPU.
"""
import gzip
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

REF = os.environ.get("GNSS_REFERENCE", "/root/reference")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, REF)

import utilities_cases as C  # noqa: E402
import utilities_oracle as O  # noqa: E402

PLOT_STUB = '''
import os
import numpy as np

class _Any:
    def __call__(self, *a, **k):
        return self
    def __getattr__(self, name):
        return self
    def __iter__(self):
        return iter((self,))
    def set_ydata(self, y):
        with open(os.environ["PLOT_CAPTURE"], "ab") as f:
            f.write(np.ascontiguousarray(y, dtype=np.float64).tobytes())

_any = _Any()

def __getattr__(name):
    return _any
'''


def run_reference(script, args, tmp, stdin=None, env_extra=None):
    """stdout goes to a regular file: under Python 3 squaring.py's y.tofile(sys.stdout) needs a seekable one"""
    env = dict(os.environ, PYTHONPATH=tmp + os.pathsep + REF, PYTHONDONTWRITEBYTECODE="1")
    env.update(env_extra or {})
    path = os.path.join(tmp, "stdout.bin")
    with open(path, "wb") as so:
        p = subprocess.run([sys.executable, os.path.join(REF, script)] + [str(a) for a in args], cwd=tmp, env=env, input=stdin,
                           stdout=so, stderr=subprocess.PIPE, timeout=3600)
    assert p.returncode == 0, (script, p.stderr[-2000:])
    with open(path, "rb") as so:
        return so.read()


def spectrum_case(case, tmp):
    import scipy.fft
    n, ns, frames, fc, fs = C.SPECTRUM[case]
    x = C.spectrum_recording(case)
    path = os.path.join(tmp, "spectrum_%s.iq" % case)
    x.tofile(path)
    cap = os.path.join(tmp, "spectrum_%s.f64" % case)
    run_reference("spectrum.py", [path, repr(fc), repr(fs), n, ns], tmp, env_extra={"PLOT_CAPTURE": cap})
    db = np.fromfile(cap, dtype=np.float64).reshape(-1, n)
    assert db.shape[0] == frames and np.all(np.isfinite(db)), (case, db.shape)
    # complex64 transform on the CPU, power sums in fp64
    s = x.reshape(-1, 2)[:frames * ns * n].astype(np.float64)
    xw = ((s[:, 0] + 1j * s[:, 1]).reshape(frames, ns, n) * np.hanning(n)).astype(np.complex64)
    z = scipy.fft.fft(xw, axis=2)
    assert z.dtype == np.complex64
    z = z.astype(np.complex128)
    p = (z.real ** 2 + z.imag ** 2).sum(axis=1) / ns
    dev32 = float(np.max(np.abs(10 * np.log10(np.fft.fftshift(p, axes=1)) - db)))
    dev64 = float(np.max(np.abs(O.psd_fp64(x, n, ns) - db)))
    assert dev64 < 1e-10, (case, dev64)
    print("spectrum %-7s n %5d ns %3d  complex64 deviation %.3g dB  fp64 restatement %.3g dB" % (case, n, ns, dev32, dev64))
    return {"n": n, "ns": ns, "frames": frames, "fc": fc, "fs": fs, "sha256": C.sha256(x), "db": C.pack(db), "complex64_deviation_db": dev32}


def squaring_case(case, tmp):
    import gnsstools.nco as nco
    import gnsstools.squaring as ref_squaring
    b, n, m, chunks, fs, coffset = C.SQUARING[case]
    x = C.squaring_recording(case)
    s = x.reshape(-1, 2)
    chunk = b * n * m
    phases = O.chunk_phase_sequence(chunks, chunk, fs, coffset)
    r_ref = np.zeros((chunks, b), dtype=np.complex128)
    for c in range(chunks):
        part = s[c * chunk:(c + 1) * chunk]
        xc = np.empty(chunk, dtype="c8")
        xc.real, xc.imag = part[:, 0], part[:, 1]
        nco.mix(xc, -coffset / fs, phases[c])
        ref_squaring.squaring(xc, r_ref[c], n, m)
    stream = np.empty((chunks, 2 * b), dtype=np.int16)
    stream[:, 0::2] = np.round(20 * np.real(r_ref)).astype(np.int16)
    stream[:, 1::2] = np.round(20 * np.imag(r_ref)).astype(np.int16)
    stream = stream.reshape(-1)
    if case == "script":
        path = os.path.join(tmp, "squaring_%s.iq" % case)
        x.tofile(path)
        out = np.frombuffer(run_reference("squaring.py", [path, repr(fs), repr(coffset)], tmp), dtype=np.int16)
        assert np.array_equal(out, stream), "squaring.py's stdout differs from its functions called chunk by chunk"
    r64, stream64, clamped = O.squaring_fp64(x, fs, coffset, b, n, m)
    assert clamped == 0 and np.max(np.abs(20 * r_ref)) < 32000, (case, clamped)
    v = np.concatenate([20 * r64.real.reshape(-1), 20 * r64.imag.reshape(-1)])
    half = float(np.min(np.abs(np.abs(v - np.floor(v)) - 0.5)))
    assert half > 1e-6, (case, half)
    diff = float(np.max(np.abs(20 * r_ref - 20 * r64)))
    ok, share = C.stream_check(stream64, stream, r_ref, C.HALF_FACTOR * diff)
    vr = np.concatenate([20 * r_ref.real.reshape(-1), 20 * r_ref.imag.reshape(-1)])
    near = float(np.mean(np.abs(np.abs(vr - np.floor(vr)) - 0.5) <= C.HALF_FACTOR * diff))
    assert ok and near <= C.HALF_SHARE, (case, ok, share, near)
    print("squaring %-8s max|20 r| %.0f  |20 r_ref - 20 r_fp64| %.3g  closest half-integer %.3g  share near one %.4f  differing %.4f"
          % (case, np.max(np.abs(20 * r_ref)), diff, half, near, share))
    return {"b": b, "n": n, "m": m, "chunks": chunks, "fs": fs, "coffset": coffset, "sha256": C.sha256(x), "r": C.pack(r_ref),
            "stream": C.pack(stream), "max_diff_20r": diff}


def cn0_case(lines, time_ms, tmp):
    argv = [] if time_ms == 300 else ["--time", time_ms]
    text = "".join(ln + "\n" for ln in lines)
    out = run_reference("cn0.py", argv, tmp, stdin=text.encode()).decode().split()
    cols = np.array([[float(t) for t in ln.split()[1:3]] for ln in lines])
    for k, got in enumerate(out):
        i, q = cols[k * time_ms:(k + 1) * time_ms, 0], cols[k * time_ms:(k + 1) * time_ms, 1]
        v = 20 * np.log10(np.mean(np.abs(i)) / (np.sqrt(2) * np.std(q))) + 30
        assert abs(abs(v * 100 - np.floor(v * 100)) - 0.5) > 1e-6 * 100, (time_ms, k, v)
    assert len(out) == len(lines) // time_ms
    return {"time": time_ms, "lines": out}


def main():
    gold = {"generator": "tools/make_goldens_utilities.py", "seed": C.SEED, "spectrum": {}, "squaring": {}, "cn0": {}}
    with open(os.path.join(C.GOLD, "trackloop_cases.json")) as f:
        tracks = json.load(f)["cases"]
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "matplotlib"))
        for name in ("__init__.py", "pyplot.py"):
            with open(os.path.join(tmp, "matplotlib", name), "w") as f:
                f.write(PLOT_STUB)
        for case in C.SPECTRUM:
            gold["spectrum"][case] = spectrum_case(case, tmp)
        for case in C.SQUARING:
            gold["squaring"][case] = squaring_case(case, tmp)
        for case in sorted(tracks):
            gold["cn0"]["track/" + case] = [cn0_case(tracks[case]["stdout_lines"], C.CN0_TRACK_TIME, tmp)]
        synth = C.cn0_synthetic_lines()
        gold["cn0"]["synthetic"] = [cn0_case(synth, t, tmp) for t in C.CN0_SYNTH["times"]]
        gold["cn0_synthetic_sha256"] = C.sha256(np.frombuffer("\n".join(synth).encode(), dtype=np.uint8))
    raw = json.dumps(gold, sort_keys=True, indent=0).encode()
    with open(C.GOLDEN_FILE, "wb") as f:
        with gzip.GzipFile(filename="", mode="wb", fileobj=f, mtime=0) as g:      # mtime 0: the same bytes on every run
            g.write(raw)
    print("wrote %s (%d bytes)" % (C.GOLDEN_FILE, os.path.getsize(C.GOLDEN_FILE)))


if __name__ == "__main__":
    main()
