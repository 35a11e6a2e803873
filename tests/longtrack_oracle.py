"""numpy restatement of the long-code track scripts' loop (track-gps-l2cl.py, track-glonass-l1-p.py / -l2-p.py) -- a test helper.

The loop is the template's (tests/track_loop_oracle.py) with an outer block of 1.5 s or 1 s split into 1500 or 1000 track() calls:
per outer block the mode switches, the block length from code_p and the offset wipe-off over the whole block; per sub-block
x[int(j*n/subs):int((j+1)*n/subs)] the carrier wipe-off, early / prompt / late and the loop update.  Phases are reduced with a plain
np.mod.  As the device kernel, it forms the correlator phases in closed form (one rounding of cp0 + incr*i) and sums each correlator
as a dot product.  `bug` plants one deliberate mistake, for the tests that show their bounds reject it."""
import numpy as np

from track_loop_oracle import _fll_atan, _pll_costas, mix, weights

BUGS = (None, "floor_boundaries", "modes_per_sub_block")


def track(spec, chips01, iq, max_records=None, bug=None, trace=None):
    """Records of one channel: spec is longtrack.long_channel_spec()'s TrackSpec, chips01 the code's {0,1} chips, iq the recording
    as interleaved int8.  Returns a list of dicts with the fields of trackloop.RECORD_DTYPE (the cycle counters as the template
    keeps them; the long-code scripts print neither).  trace: a list that receives (code_p, cf, m) of every sub-block.
    bug: "floor_boundaries" splits an outer block at j*(n//subs); "modes_per_sub_block" checks the mode switches before every call."""
    assert bug in BUGS
    L = len(chips01)
    fs = spec.fs
    subs = spec.subs
    nsamp = len(iq) // 2
    xr_all = iq[0::2][:nsamp]
    xi_all = iq[1::2][:nsamp]
    code_offset = spec.code_offset
    n = int(fs * spec.period * ((L - code_offset) / L))               # alignment with the code boundary
    pos = n
    code_p = code_offset + n * spec.rate * L / fs
    code_f, carrier_p, carrier_f = spec.chip_rate, spec.carrier_phase, spec.doppler
    prompt1 = 0 + 0 * (1j)
    carrier_e1 = code_e1 = 0
    carrier_cyc = code_cyc = 0
    mode = 2 if spec.fixed_pll else 0
    block, samp, coffset_phase = 0, 0, 0.0
    out = []

    def switch(mode, block):
        if not spec.fixed_pll:
            if block >= spec.dwell_wide:
                mode = 1
            if block >= spec.dwell_wide + spec.dwell_narrow:
                mode = 2
        return mode

    while True:
        mode = switch(mode, block)
        if code_p < L / 2:
            n = int(fs * spec.period * (L - code_p) / L)
        else:
            n = int(fs * spec.period * (2 * L - code_p) / L)
        if pos + n > nsamp or (max_records is not None and len(out) + subs > max_records):
            break
        xr, xi = xr_all[pos:pos + n].astype(np.float32), xi_all[pos:pos + n].astype(np.float32)
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
        for j in range(subs):
            if bug == "floor_boundaries":
                a, b = j * (n // subs), (j + 1) * (n // subs)
            else:
                a, b = int(j * n / subs), int((j + 1) * n / subs)
            if bug == "modes_per_sub_block":
                mode = switch(mode, block)
            m = b - a
            yr, yi = mix(xr[a:b], xi[a:b], -carrier_f / fs, carrier_p)
            carrier_p = carrier_p - m * carrier_f / fs
            t = np.mod(carrier_p, 1)
            carrier_cyc += int(round(carrier_p - t))
            carrier_p = t
            cf = (code_f + carrier_f / spec.ratio) / fs
            if trace is not None:
                trace.append((code_p, cf, m))
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
