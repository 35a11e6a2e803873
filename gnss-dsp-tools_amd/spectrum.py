"""The reference's spectrum.py on the GPU: Welch power spectrum of a raw int8 I/Q recording.

    spectrum.py:48-57     per output frame: ns blocks of n samples, np.hanning(n) window, FFT, |z|^2 / ns summed, fftshift, 10 log10
    spectrum.py:18        the frequency axis of the plot

Power-of-two lengths from 64 to 16384 run in the LDS transform kernel of gacq_spectrum.hip (gacq_psd_int8_dev: complex64 transform,
fp64 power sums, bit-reproducible); every other length the script accepts goes through torch.fft in complex128 on the device.

    python -m gnss_dsp_tools_amd.spectrum FILE FC FS N NS [--out FILE] [--plot]
"""
import ctypes
import sys

import numpy as np

from . import _native as nat
from . import acquire, rawfile

KERNEL_LENGTHS = tuple(1 << k for k in range(6, 15))


def freq_axis_mhz(fc, fs, n):
    """x-axis of the script's plot (spectrum.py:18)."""
    return (fc + fs * ((np.arange(n) - (n / 2.0)) / n)) / 1e6


def _psd_torch(x, n, ns, F):
    """any length: complex128 on the device, the script's operations frame by frame"""
    torch = nat.require_torch()
    w = torch.from_numpy(np.hanning(n)).to(x.device)
    out = torch.empty((F, n), dtype=torch.float64, device=x.device)
    for f in range(F):
        s = x[2 * f * n * ns:2 * (f + 1) * n * ns].view(ns, n, 2).to(torch.float64)
        z = torch.fft.fft(torch.complex(s[..., 0] * w, s[..., 1] * w), dim=1)
        p = (z.real * z.real + z.imag * z.imag).sum(dim=0) / ns
        out[f] = 10 * torch.log10(torch.fft.fftshift(p))
    return out


def psd_dev(iq_int8, n, ns, engine=None, split=0):
    """psd() with the result left on the device: torch float64 CUDA tensor [F, n]."""
    torch = nat.require_torch()
    eng = engine or acquire.default_engine()
    n, ns = int(n), int(ns)
    if n < 1 or ns < 1:
        raise ValueError("n and ns must be positive")
    x = rawfile.device_int8(eng, iq_int8)
    F = (x.numel() // 2) // (n * ns)            # a trailing partial group of frames is dropped, as the script's sys.exit() does
    if F == 0:
        return torch.empty((0, n), dtype=torch.float64, device=x.device)
    if n not in KERNEL_LENGTHS:
        return _psd_torch(x, n, ns, F)
    win = torch.from_numpy(np.hanning(n).astype(np.float32)).to(x.device)
    out = torch.empty((F, n), dtype=torch.float64, device=x.device)
    nat.check(nat.lib.gacq_psd_int8_dev(eng._ctx, ctypes.c_void_p(x.data_ptr()), F, n, ns, ctypes.c_void_p(win.data_ptr()), int(split),
                                        ctypes.c_void_p(out.data_ptr())), eng._ctx)
    return out


def psd(iq_int8, n, ns, engine=None, split=0):
    """dB frames [F, n] (float64, what the script plots) of F = len // (n * ns) groups of ns blocks of n samples.  iq_int8: numpy int8
    ([len, 2] or flat interleaved) or a torch int8 CUDA tensor.  split: workgroups per spectrum (0: chosen from F); the result does
    not depend on it."""
    return psd_dev(iq_int8, n, ns, engine, split).cpu().numpy()


USAGE = "usage: python -m gnss_dsp_tools_amd.spectrum FILE FC FS N NS [--out FILE] [--plot]"


def parse(argv):
    """FILE FC FS N NS as the script reads sys.argv[1:6], plus --out FILE (append each frame's n float64 dB values) and --plot (live
    plot, needs matplotlib).  The numbers are not run through an option parser: FC may be negative, in any float spelling."""
    import argparse
    argv, pos, out, plot = list(argv), [], None, False
    while argv:
        t = argv.pop(0)
        if t == "--plot":
            plot = True
        elif t == "--out" and argv:
            out = argv.pop(0)
        elif t.startswith("--out="):
            out = t[6:]
        else:
            pos.append(t)
    try:
        if len(pos) != 5:
            raise ValueError
        a = argparse.Namespace(filename=pos[0], fc=float(pos[1]), fs=float(pos[2]), n=int(pos[3]), ns=int(pos[4]), out=out, plot=plot)
        if a.n < 1 or a.ns < 1:
            raise ValueError
    except ValueError:
        print(USAGE, file=sys.stderr)
        raise SystemExit(2)
    return a


def frame_line(k, x_mhz, y):
    """index, peak frequency (MHz), peak dB, median dB"""
    i = int(np.argmax(y))
    return "%d %.6f %.3f %.3f" % (k, x_mhz[i], y[i], np.median(y))


class _LivePlot:
    """dB against MHz in one matplotlib window, redrawn for every frame"""

    def __init__(self, x_mhz):
        import matplotlib.pyplot as plt
        self.plt = plt
        plt.ion()
        self.fig, self.ax = plt.subplots()
        self.curve = self.ax.plot(x_mhz, np.full(len(x_mhz), np.nan))[0]
        self.ax.set(xlabel="MHz", ylabel="dB", title="Welch power spectrum")
        self.ax.grid(True)

    def show(self, y):
        finite = y[np.isfinite(y)]
        self.curve.set_ydata(y)
        if len(finite):
            self.ax.set_ylim(finite.min() - 1.0, finite.max() + 1.0)
        self.fig.canvas.draw_idle()
        self.plt.pause(0.05)


def run(argv, out=None, engine=None):
    a = parse(argv)
    out = out or sys.stdout
    x_mhz = freq_axis_mhz(a.fc, a.fs, a.n)
    plot = _LivePlot(x_mhz) if a.plot else None
    sink = open(a.out, "ab") if a.out else None
    k = 0
    try:
        with open(a.filename, "rb") as fp:
            for piece in rawfile.read_pieces(fp, 2 * a.n * a.ns):
                for y in psd(piece, a.n, a.ns, engine):
                    if sink:
                        sink.write(y.tobytes())
                    if plot:
                        plot.show(y)
                    if not sink and not plot:
                        print(frame_line(k, x_mhz, y), file=out)
                    k += 1
    finally:
        if sink:
            sink.close()
    return k


if __name__ == "__main__":
    run(sys.argv[1:])
