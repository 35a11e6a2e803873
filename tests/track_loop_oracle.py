"""numpy restatement of the template track-*.py loop (track-gps-l1.py:33-179), vectorised per block -- a test helper.

It follows the scripts step by step in fp64 with their own evaluation order, and differs from the interpreted reference in two
places only, both as the device kernel does it: the correlator phases are the closed form of tracking_oracle.closed_form_indices
(one rounding of cp0 + incr*i), and each correlator is summed as a dot product rather than sample by sample.  The wipe-off
products are written as separate real multiplies and adds (numpy's complex loops may fuse them) and rounded to complex64 twice,
as the reference's c8 array stores them.  It serves the shapes the interpreted reference is too slow for."""
import numpy as np

from oracle import tracking_oracle

NT = 1024
NCO_TABLE = np.exp(2 * (np.pi) * (1j) * np.arange(NT) * (1.0 / NT))      # gnsstools/nco.py:3-4
_TMBOC = np.array([1, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0], dtype=bool)
_M64 = (1 << 64) - 1


def mix(xr, xi, f, p):
    """nco.mix(x, f, p) on complex64 parts (float32 arrays): the 50-bit fixed-point table NCO (gnsstools/nco.py:30-41)."""
    n = len(xr)
    dp = int(np.floor(p * NT * (1 << 50)))
    df = int(np.floor(f * NT * (1 << 50)))
    ph = np.uint64(dp & _M64) + np.arange(n, dtype=np.uint64) * np.uint64(df & _M64)      # wraps mod 2^64: bits 50..59 are exact
    idx = ((ph >> np.uint64(50)) & np.uint64(NT - 1)).astype(np.int64)
    tr, ti = NCO_TABLE.real[idx], NCO_TABLE.imag[idx]
    a, b = xr.astype(np.float64), xi.astype(np.float64)
    re = a * tr - b * ti
    im = a * ti + b * tr
    return re.astype(np.float32), im.astype(np.float32)


def weights(chips01, kind, frac, incr, n):
    """fp64 chip weights of correlate(x, prn, 0, frac, incr, c[, boc11]) for n samples, closed-form phases."""
    L = len(chips01)
    idx, b1, b6 = tracking_oracle.closed_form_indices(L, 0, frac, incr, n)
    w = 1.0 - 2.0 * chips01[idx].astype(np.float64)
    s1 = 1.0 - 2.0 * b1
    s6 = 1.0 - 2.0 * b6
    if kind == 1:
        w = w * s1
    elif kind == 2:
        w = w * (0.953463 * s1 + 0.301511 * s6)
    elif kind == 3:
        w = w * np.where(_TMBOC[idx % 33], s6, s1)
    elif kind == 4:
        w = w * (b1 == 0)
    elif kind == 5:
        w = w * (b1 == 1)
    return w


def _fll_atan(a, b):
    t = np.pi / 2 if a.real == 0 else np.arctan(a.imag / a.real)
    t1 = np.pi / 2 if b.real == 0 else np.arctan(b.imag / b.real)
    d = t - t1
    if d > np.pi / 2:
        d = np.pi - d
    if d < -np.pi / 2:
        d = -np.pi - d
    return d


def _pll_costas(x):
    return np.arctan2(x.imag, x.real) if x.real > 0 else np.arctan2(-x.imag, -x.real)


def track(spec, chips01, iq, max_records=None, n_bias=0):
    """Records of one channel: spec is trackloop.channel_spec()'s TrackSpec, chips01 the code's {0,1} chips, iq the recording as
    interleaved int8.  Returns a list of dicts with the fields of trackloop.RECORD_DTYPE.
    n_bias: samples added to every block length (a deliberate bug, for the tests that show their bounds reject it)."""
    L = len(chips01)
    fs = spec.fs
    nsamp = len(iq) // 2
    xr_all = iq[0::2][:nsamp].astype(np.float32)
    xi_all = iq[1::2][:nsamp].astype(np.float32)
    code_offset = spec.code_offset
    n = int(fs * spec.period * ((L - code_offset) / L))
    pos = n
    code_p = code_offset + n * spec.rate * L / fs
    code_f, carrier_p, carrier_f = spec.chip_rate, spec.carrier_phase, spec.doppler
    prompt1 = 0 + 0 * (1j)
    carrier_e1 = code_e1 = 0
    carrier_cyc = code_cyc = 0
    mode = 2 if spec.fixed_pll else 0
    block, samp, coffset_phase = 0, 0, 0.0
    out = []
    while True:
        if not spec.fixed_pll:
            if block >= spec.dwell_wide:
                mode = 1
            if block >= spec.dwell_wide + spec.dwell_narrow:
                mode = 2
        if code_p < L / 2:
            n = int(fs * spec.period * (L - code_p) / L)
        else:
            n = int(fs * spec.period * (2 * L - code_p) / L)
        n += n_bias
        if pos + n > nsamp or (max_records is not None and len(out) >= max_records):
            break
        xr, xi = xr_all[pos:pos + n], xi_all[pos:pos + n]
        pos += n
        samp += n
        if spec.glonass:
            fo = spec.fm
            xr, xi = mix(xr, xi, fo, coffset_phase)
            coffset_phase = coffset_phase + n * fo
        else:
            xr, xi = mix(xr, xi, -spec.coffset / fs, coffset_phase)
            coffset_phase = coffset_phase - n * spec.coffset / fs
        coffset_phase = np.mod(coffset_phase, 1)
        for j in range(spec.subs):
            a, b = int(j * n / spec.subs), int((j + 1) * n / spec.subs)
            m = b - a
            yr, yi = mix(xr[a:b], xi[a:b], -carrier_f / fs, carrier_p)
            carrier_p = carrier_p - m * carrier_f / fs
            t = np.mod(carrier_p, 1)
            carrier_cyc += int(round(carrier_p - t))
            carrier_p = t
            cf = (code_f + carrier_f / spec.ratio) / fs
            yr64, yi64 = yr.astype(np.float64), yi.astype(np.float64)
            p = []
            for off in (-spec.spacing, 0.0, spec.spacing):
                w = weights(chips01, spec.kind, code_p + off, cf, m)
                p.append(complex(np.dot(yr64, w), np.dot(yi64, w)))
            p_early, p_prompt, p_late = p
            if mode == 2:
                e = _pll_costas(p_prompt)
                carrier_f = carrier_f + spec.pll_k1 * e + spec.pll_k2 * (e - carrier_e1)
                carrier_e1 = e
            else:
                e = _fll_atan(p_prompt, prompt1)
                carrier_f = carrier_f + (spec.fll_k_wide if mode == 0 else spec.fll_k_narrow) * e
                prompt1 = p_prompt
            early, prompt, late = np.absolute(p_early), np.absolute(p_prompt), np.absolute(p_late)
            e = 0 if (late + early) == 0 else (late - early) / (late + early)
            code_f = code_f + spec.dll_k1 * e + spec.dll_k2 * (e - code_e1)
            code_e1 = e
            code_p = code_p + m * cf
            t = np.mod(code_p, L)
            code_cyc += int(round(code_p - t))
            code_p = t
            out.append(dict(p_re=p_prompt.real, p_im=p_prompt.imag, carrier_f=carrier_f, code_f=code_f, early=early, prompt=prompt,
                            late=late, code_p=code_p, carrier_p=carrier_p, block=block, code_cyc=code_cyc, carrier_cyc=carrier_cyc,
                            samp=samp))
            block += 1
    return out
