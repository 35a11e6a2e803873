"""numpy restatement of track-beidou-b2bi.py / -b2bq.py -- a test helper.

The loop is the template's (tests/track_loop_oracle.py: closed-form correlator phases, dot-product sums, the wipe-offs rounded to
complex64 twice), with one addition between early / prompt / late and the loop update:

    if nframe > accum_after:  nco.accum(x if real(p_prompt) > 0 else -x, code_p, cf, chips, L)

each wiped-off complex64 sample added to a complex128 bin, in sample order.  The bin of sample i is the prompt correlator's
closed-form index floor(fma(cf, i, code_p)) mod L (tracking_oracle.closed_form_indices), as on the device.  `bug` plants one
deliberate mistake, for the tests that show the goldens reject it."""
import numpy as np

from oracle import tracking_oracle
from track_loop_oracle import _fll_atan, _pll_costas, mix, weights

BUGS = (None, "accum_from_200", "ignore_sign", "code_p_after_update", "runs_out_of_order")


def accum(chips, idx, vr, vi):
    """a[idx[i]] += v[i] for i in sample order (np.add.at applies repeated indices in order)."""
    np.add.at(chips.real, idx, vr)
    np.add.at(chips.imag, idx, vi)


def track(spec, chips01, iq, accum_after=200, max_records=None, bug=None, trace=None):
    """(records, bins, signs) of one channel: spec is chiptrack.chip_channel_spec()'s TrackSpec, chips01 the code's {0,1} chips, iq
    the recording as interleaved int8.  records: dicts with the fields of trackloop.RECORD_DTYPE; bins: complex128[L]; signs: the
    sign (+1 / -1) each accumulated frame took, by frame.  trace: a list that receives (code_p, cf, m) of every accumulated frame."""
    assert bug in BUGS
    assert spec.subs == 1 and spec.kind == 0 and not spec.glonass
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
    mode = 0
    block, samp, coffset_phase = 0, 0, 0.0
    bins = np.zeros(L, dtype=np.complex128)
    signs = {}
    out = []
    thr = accum_after - 1 if bug == "accum_from_200" else accum_after
    while True:
        if block >= spec.dwell_wide:
            mode = 1
        if block >= spec.dwell_wide + spec.dwell_narrow:
            mode = 2
        if code_p < L / 2:
            n = int(fs * spec.period * (L - code_p) / L)
        else:
            n = int(fs * spec.period * (2 * L - code_p) / L)
        if pos + n > nsamp or (max_records is not None and len(out) >= max_records):
            break
        xr, xi = xr_all[pos:pos + n], xi_all[pos:pos + n]
        pos += n
        samp += n
        xr, xi = mix(xr, xi, -spec.coffset / fs, coffset_phase)
        coffset_phase = coffset_phase - n * spec.coffset / fs
        coffset_phase = np.mod(coffset_phase, 1)
        m = n
        yr, yi = mix(xr, xi, -carrier_f / fs, carrier_p)
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
        if block > thr:
            sg = 1.0 if (p_prompt.real > 0 or bug == "ignore_sign") else -1.0
            signs[block] = sg
            start = np.mod(code_p + m * cf, L) if bug == "code_p_after_update" else code_p
            idx = tracking_oracle.closed_form_indices(L, 0, start, cf, m)[0]
            if trace is not None:
                trace.append((code_p, cf, m))
            vr, vi = sg * yr64, sg * yi64                          # -x of a complex64 array: exact, then widened
            if bug == "runs_out_of_order":
                accum(bins, idx[::-1], vr[::-1], vi[::-1])
            else:
                accum(bins, idx, vr, vi)
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
    return out, bins, signs
