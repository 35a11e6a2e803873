"""The definition of the recording ingest (gacq_ingest_dev, include/gacq.h) restated in numpy: integers (int64) for the codes, the LUT
and the real-IF filter, which is summed in its plain complex form sum_k g[k] x[2m - k] (-i)^(2m - k); numpy float32 for the one
multiply by the gain.  No GPU, and nothing of the package.

A format is a dict: container 's8' | 'u8' | 's16' | 'f32' | 'packed', bits, msb_first, lut (packed), real, conj."""
import numpy as np

G_ODD = (10382, -3333, 1852, -1175, 774, -506, 320, -188, 97, -40, 9)      # g[1], g[3], .., g[21]
HALF = 21
AUTO_SAMPLES = 65536


def taps():
    """g[-21 .. 21] as int64 [43]"""
    g = np.zeros(2 * HALF + 1, dtype=np.int64)
    g[HALF] = 16384
    for i, v in enumerate(G_ODD):
        g[HALF + 2 * i + 1] = g[HALF - 2 * i - 1] = v
    return g


def taps_from_formula():
    """rint(h / h[23] * 16384) of the 47-tap Hann-windowed sinc with its cutoff at fs/4 (numpy.hanning(47) is zero at both ends, which
    leaves the 45 taps -22 .. 22 and g[+-22] = 0 besides): returned for k = -23 .. 23"""
    k = np.arange(47, dtype=np.float64) - 23.0
    h = 0.5 * np.sinc(0.5 * k) * (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(47) / 46.0))
    return np.rint(h / h[23] * 16384.0).astype(np.int64)


def preset(bits, coding):
    out = []
    for code in range(1 << bits):
        if coding == "sm":
            mag = code & ((1 << (bits - 1)) - 1)
            out.append(-(2 * mag + 1) if code >> (bits - 1) else 2 * mag + 1)
        elif coding == "ob":
            out.append(2 * code - ((1 << bits) - 1))
        elif coding == "tc":
            out.append(2 * (code - (1 << bits) if code >> (bits - 1) else code) + 1)
        else:
            raise ValueError(coding)
    return out


def fmt(name, real=False, conj=False, msb_first=True, lut=None):
    if name in ("s8", "u8", "s16", "f32"):
        return dict(container=name, bits={"s8": 8, "u8": 8, "s16": 16, "f32": 32}[name], msb_first=True, lut=None, real=real, conj=conj)
    bits = int(name[0])
    return dict(container="packed", bits=bits, msb_first=msb_first, lut=list(preset(bits, name[1:]) if lut is None else lut), real=real, conj=conj)


def sample_bits(f):
    return f["bits"] * (1 if f["real"] else 2)


def values(f, data):
    """every whole value of the bytes: int64, or float32 for 'f32'"""
    b = np.frombuffer(bytes(data), dtype=np.uint8)
    c = f["container"]
    if c == "s8":
        return b.view(np.int8).astype(np.int64)
    if c == "u8":
        return b.astype(np.int64) - 128
    if c == "s16":
        return b[:len(b) // 2 * 2].view("<i2").astype(np.int64)
    if c == "f32":
        return b[:len(b) // 4 * 4].view("<f4").copy()
    bits = f["bits"]
    per = 8 // bits
    i = np.arange(per)
    shift = (8 - bits * (i + 1)) if f["msb_first"] else bits * i
    codes = (b[:, None].astype(np.int64) >> shift[None, :]) & ((1 << bits) - 1)
    return np.asarray(f["lut"], dtype=np.int64)[codes.reshape(-1)]


def out_range(f, in_first, in_count):
    """(first, count) of the output samples that input samples in_first .. in_first + in_count - 1 support"""
    if not f["real"]:
        return in_first, in_count
    first = 0 if in_first == 0 else (in_first + HALF + 1) // 2
    last = (in_first + in_count - 1 - HALF) // 2
    return first, max(0, last - first + 1)


def accumulate_real(x_at, out_first, n_out):
    """acc(m) = sum_k g[k] x[2m - k] (-i)^(2m - k), m = out_first .. out_first + n_out - 1, in its plain complex form: (re, im) int64.
    x_at(n) -> int64 values of an int64 index array (0 below index 0)."""
    g = taps()
    m = np.arange(n_out, dtype=np.int64) + out_first
    re = np.zeros(n_out, dtype=np.int64)
    im = np.zeros(n_out, dtype=np.int64)
    rot_re = np.array([1, 0, -1, 0], dtype=np.int64)            # (-i)^p = 1, -i, -1, i
    rot_im = np.array([0, -1, 0, 1], dtype=np.int64)
    for k in range(-HALF, HALF + 1):
        n = 2 * m - k
        t = g[k + HALF] * x_at(n)
        re += t * rot_re[n % 4]
        im += t * rot_im[n % 4]
    return re, im


def closed_form_real(x_at, out_first, n_out):
    """the form the kernel evaluates: Re = (-1)^m 16384 x[2m], Im = (-1)^m sum_{k odd > 0} g[k] s(k) (x[2m - k] - x[2m + k])"""
    g = taps()
    m = np.arange(n_out, dtype=np.int64) + out_first
    sign = 1 - 2 * (m % 2)
    im = np.zeros(n_out, dtype=np.int64)
    for k in range(1, HALF + 1, 2):
        s = 1 if k % 4 == 1 else -1
        im += g[k + HALF] * s * (x_at(2 * m - k) - x_at(2 * m + k))
    return sign * 16384 * x_at(2 * m), sign * im


def unscaled(f, data, in_first=0, out_first=None, n_out=None):
    """u(m) as (re, im) float32 arrays -- exact for every container but f32, where they are the floats themselves"""
    v = values(f, data)
    in_count = len(v) // (1 if f["real"] else 2)
    first, count = out_range(f, in_first, in_count)
    out_first = first if out_first is None else out_first
    n_out = first + count - out_first if n_out is None else n_out
    assert n_out >= 0 and out_first >= first and out_first + n_out <= first + count, "an input that is needed is not present"
    if f["real"]:
        def x_at(n):
            assert np.all((n < 0) | ((n >= in_first) & (n < in_first + in_count)))
            return np.where(n < 0, 0, v[np.clip(n - in_first, 0, len(v) - 1)])
        re, im = accumulate_real(x_at, out_first, n_out)
        assert max(np.max(np.abs(re), initial=0), np.max(np.abs(im), initial=0)) < 2 ** 23
        re = re.astype(np.float32) * np.float32(2.0 ** -14)      # exact: below 2^23, times a power of two
        im = im.astype(np.float32) * np.float32(2.0 ** -14)
    else:
        j = np.arange(n_out, dtype=np.int64) + (out_first - in_first)
        re, im = v[2 * j].astype(np.float32), v[2 * j + 1].astype(np.float32)
    if f["conj"]:
        im = -im
    return re, im


def to_int8(v):
    """interleaved int8 of complex64 values: clip(rint(.), -127, 127), ties to even, NaN to 0"""
    out = np.empty(2 * len(v), dtype=np.int8)
    for k, part in enumerate((np.real(v), np.imag(v))):
        r = np.clip(np.rint(np.where(np.isnan(part), np.float32(0), part)), -127, 127)
        out[k::2] = r.astype(np.int8)
    return out


def evaluate(f, data, gain, in_first=0, out_first=None, n_out=None, dtype="int8"):
    """what gacq_ingest_dev writes: complex64 [n_out], or int8 [2 n_out]"""
    re, im = unscaled(f, data, in_first, out_first, n_out)
    g = np.float32(gain)
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.empty(len(re), dtype=np.complex64)
        v.real = re * g                                          # one float32 multiply per component
        v.imag = im * g
    return v if dtype == "complex64" else to_int8(v)


def auto_gain(f, data, target_rms=32.0):
    """target_rms / sqrt(mean |u(j)|^2, j < P) in float64, P = min(output samples the data supports, 65536)"""
    v = values(f, data)
    _, count = out_range(f, 0, len(v) // (1 if f["real"] else 2))
    re, im = unscaled(f, data, 0, 0, min(count, AUTO_SAMPLES))
    power = float(np.mean(re.astype(np.float64) ** 2 + im.astype(np.float64) ** 2))
    return float(target_rms) / np.sqrt(power)
