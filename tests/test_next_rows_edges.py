"""The kernels either side of the acquisition search -- the long-code search (gacq_longcode.hip), the tracking correlators
(gacq_tracking.hip) and the front-end (gacq_frontend.hip) -- against fp64 references at the shapes where their indexing changes:
candidate groups with a partial last group, chunk tails, the finish kernels' grid boundary, phase wraps, FIR tile boundaries, the
resample clamp.  Every output is compared (not only a winner), with bounds derived from the kernels' arithmetic, and each family
shows once that its bound rejects a one-chip / one-tap / one-sample error."""
import ctypes

import numpy as np
import pytest

# ---------------------------------------------------------------------------------------------------------------- long code

LC_MINWG = 1024          # GACQ_LC_MINWG
LC_CHUNK = 4096          # samples per workgroup of longcode_dot_kernel


def lc_kc(K, blocks, n):
    """candidates per workgroup as longcode_run picks them: halve 8 until there are >= GACQ_LC_MINWG workgroups"""
    chunks = -(-n // LC_CHUNK)
    kc = 8
    while kc > 1 and -(-K // kc) * blocks * chunks < LC_MINWG:
        kc >>= 1
    return kc


# (code, prn, fs, K, blocks, n): one shape per candidate-group size, K % kc != 0 wherever kc > 1
LC_SHAPES = [("glonass.p", 0, 16384000.0, 1003, 1, 65536),     # kc 8 (P-code block), 1003 = 125*8 + 3
             ("gps.l2cl", 7, 4096000.0, 75, 16, 3 * 4096 + 17),  # kc 4, four chunks the last 17 samples long
             ("gps.l2cl", 19, 4096000.0, 37, 30, 4097),         # kc 2, one-sample chunk tail
             ("gps.ca", 5, 4092000.0, 5, 3, 1000),              # kc 1, a short code through the generic entry point, n < chunk
             ("gps.ca", 12, 4096000.0, 9, 2, 4096)]             # kc 1, n == one chunk exactly
LC_IDS = ["%s-K%d-B%d-n%d-kc%d" % (c, K, B, n, lc_kc(K, B, n)) for c, _, _, K, B, n in LC_SHAPES]


def lc_phases(rng, K, blocks, L, span, sig_phase):
    """start phases drawn from every range the kernel's index reduction distinguishes: inside [0, L), negative, crossing L inside the
    block, between L and 2L, beyond 2L (the '%=' branch), far beyond it (~1.5e9 chips); candidate 0 follows the signal."""
    kind = rng.integers(0, 7, size=(K, blocks))
    u = rng.uniform(0.0, 1.0, size=(K, blocks))
    ph = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4, kind == 5, kind == 6],
                   [u * L, -u * 3 * L, L - u * span, L + u * L, 2 * L + u * 5 * L, -1.5e9 * u, 1.5e9 * u + 2 * L])
    ph[0] = sig_phase
    return ph


@pytest.mark.gpu
@pytest.mark.parametrize("shape", LC_SHAPES, ids=LC_IDS)
def test_gpu_longcode_every_candidate_matches_fp64(engine, shape):
    """Every q[k], not only the winner, against oracle/longcode_oracle.q_vector (fp64).  The only roundings on the device are the fp32
    table NCO value and the fp32 complex product x*w (longcode_mix_kernel): each sample's x*w is off by at most (2^-23*sqrt(2) +
    2^-24)|x| < 2^-22|x|; the +-1 weights and the fp64 sums (depth < 60) add nothing at that scale, so
        |q_gpu[k] - q[k]| <= sum_b |sum_i d(x w)_i| <= 2^-22 sum |x|,
    asserted with a factor 2 to spare.  The three input paths (host complex64, raw int8 wiped off on the device, device tensor) must
    produce the same bits; one flipped chip of the winning candidate's code must move the oracle outside the bound."""
    import torch
    from gnss_dsp_tools_amd import longcode, synth
    from oracle import codes_oracle, longcode_oracle
    code, prn, fs, K, blocks, n = shape
    L = len(codes_oracle.chips(code, prn))
    incr = longcode_oracle.CHIP_RATE[code] / fs
    seed = 1000 + K
    rng = np.random.default_rng(seed)
    coffset, dop = -2750.5, 1234.0
    start = float(rng.uniform(0, L))
    total = blocks * n
    # the signal follows candidate 0: its code phase at block b is start + incr*n*b
    sig = synth.make_longcode_iq(code, prn, longcode_oracle.CHIP_RATE[code], L, fs, total, seed, 0.8, coffset + dop, start)
    raw = np.empty((total, 2), dtype=np.int8)
    raw[:, 0] = np.clip(np.round(30 * sig.real), -127, 127)
    raw[:, 1] = np.clip(np.round(30 * sig.imag), -127, 127)
    phase0 = lc_phases(rng, K, blocks, L, incr * n, start + incr * n * np.arange(blocks))
    phase0[0] = np.mod(phase0[0], L)
    assert np.all(np.abs(phase0) < 2147483000.0 - incr * n)                       # the kernel's documented range
    x_dev = engine.mix_int8_dev(raw, fs, coffset)
    x = x_dev.cpu().numpy()
    q_int8 = longcode._run(engine, raw, fs, code, prn, dop, phase0, blocks, n, coffset=coffset)
    q_host = longcode._run(engine, x, fs, code, prn, dop, phase0, blocks, n)
    q_dev = longcode._run(engine, x_dev, fs, code, prn, dop, phase0, blocks, n)
    assert q_host.tobytes() == q_int8.tobytes() == q_dev.tobytes()
    want = longcode_oracle.q_vector(x.astype(np.complex128), code, prn, dop, phase0, blocks, n, fs)
    bound = 2.0 ** -21 * float(np.sum(np.abs(x.astype(np.complex128))))
    err = np.abs(q_host - want)
    assert err.max() <= bound, (int(np.argmax(err)), float(err.max()), bound)
    assert int(np.argmax(want)) == 0 and want[0] > 3 * np.median(want)          # the signal is where it was put
    # sensitivity: the chip candidate 0 reads at sample 0 of block 0, flipped
    c01 = codes_oracle.chips(code, prn).copy()
    c01[int(np.floor(phase0[0, 0])) % L] ^= 1
    flipped = longcode_oracle.q_vector(x.astype(np.complex128), code, prn, dop, phase0[:1], blocks, n, fs, chips01=c01)
    assert abs(flipped[0] - q_host[0]) > bound, (float(abs(flipped[0] - q_host[0])), bound)


def test_q_vector_equals_the_per_candidate_loop():
    """q_vector's grouped index tables against the reference's one-candidate-at-a-time form (_code, np.sum of x*c*w), on start phases
    in every range of lc_phases and a candidate count that leaves a partial group."""
    from oracle import acq_oracle, codes_oracle, longcode_oracle
    rng = np.random.default_rng(5)
    fs, n, blocks, K = 4092000.0, 1000, 3, 41
    incr = longcode_oracle.CHIP_RATE["gps.ca"] / fs
    c01 = codes_oracle.chips("gps.ca", 9)
    x = rng.standard_normal(n * blocks) + 1j * rng.standard_normal(n * blocks)
    phase0 = lc_phases(rng, K, blocks, 1023, incr * n, rng.uniform(0, 1023, blocks))
    got = longcode_oracle.q_vector(x, "gps.ca", 9, 777.0, phase0, blocks, n, fs)
    w = acq_oracle.nco(-777.0 / fs, 0, n)
    for k in range(K):
        want = sum(np.absolute(np.sum(x[n * b:n * (b + 1)] * longcode_oracle._code(c01, 0, phase0[k, b], incr, n) * w)) for b in range(blocks))
        assert got[k] == pytest.approx(want, rel=1e-13), k


# ---------------------------------------------------------------------------------------------------------------- tracking

TR_CODES = ["gps.l1cd", "beidou.b1cd", "beidou.b1cp", "galileo.e1b", "galileo.e1c", "gps.l1cp", "gps.l2cm", "gps.l2cl",
            "gps.ca", "gps.l5i", "beidou.b1i"]
TR_NS = [1, 63, 4095, 4096, 4097, 5 * 4096 + 1, 100000]


def tr_bound(kind, x):
    """|x*w| is exact in fp32 for w in {+-1, 0} and the sums are fp64 (depth < 60): 1e-12 of sum|x| is far above what they can lose.
    CBOC's weight 0.953463f*s1 + 0.301511f*s6 and the product with it are fp32 roundings: < 3*2^-24 relative, bound 2^-22."""
    s = float(np.sum(np.abs(np.asarray(x, dtype=np.complex128))))
    return (2.0 ** -22 if kind == 2 else 1e-12) * s


def tr_specs(rng, L, K, rate_chips):
    """(chips, frac, incr) for K correlators: ordinary phases, chips + frac negative or several periods above L, dyadic start phases
    on the half-chip and sixth-chip boundaries with a dyadic rate (exact in every form), incr = 0, incr above one chip per sample."""
    chips = np.zeros(K)
    frac = rng.uniform(0.0, L, K)
    incr = np.full(K, rate_chips) * rng.uniform(0.9, 1.1, K)
    for k in range(K):
        kind = k % 6
        if kind == 1:
            chips[k] = -float(rng.integers(1, 4)) * L
            frac[k] = -rng.uniform(0.0, L)
        elif kind == 2:
            chips[k] = float(rng.integers(1, 5)) * L + 3.0
        elif kind == 3:
            frac[k] = float(rng.integers(0, 4 * L)) / 4.0            # 2s and 12s integers for even quarters, 12s for odd ones
            incr[k] = (0.25, 0.125, 0.0625, 0.5)[k % 4]
        elif kind == 4:
            incr[k] = 0.0
        elif kind == 5:
            incr[k] = rng.uniform(1.05, 3.3)
    return chips, frac, incr


def tr_check_phase_forms(L, chips, frac, incr, n):
    """The oracle (and the kernel) use closed-form phases; the reference advances them by repeated addition.  On the cases used here
    the two index sequences must be identical -- otherwise the case does not pin the reference's semantics and is replaced."""
    from oracle import tracking_oracle
    seq = tracking_oracle.sequential_indices(L, chips, frac, incr, n)
    for k in range(len(chips)):
        closed = tracking_oracle.closed_form_indices(L, chips[k], frac[k], incr[k], n)
        for name, a, b in zip(("cp", "bp", "bp6"), closed, seq):
            assert np.array_equal(a, b[k]), ("closed-form and sequential phases differ", name, k, chips[k], frac[k], incr[k])


def tr_x(rng, n):
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)


@pytest.mark.gpu
@pytest.mark.parametrize("ci", range(len(TR_CODES)), ids=["%s-n%d" % (c, TR_NS[i % len(TR_NS)]) for i, c in enumerate(TR_CODES)])
def test_gpu_correlators_every_kind_match_fp64(engine, ci):
    """Every subcarrier kind and three plain codes, one block length each (all of 1 .. 100 000 samples over the set, the one-chunk,
    chunk-edge and multi-chunk regimes), 12 correlators spanning every phase range of tr_specs, against correlate_many at the
    derived bound; host and device-resident blocks give identical bytes."""
    import torch
    from gnss_dsp_tools_amd import codes, tracking
    from oracle import tracking_oracle
    code = TR_CODES[ci]
    n = TR_NS[ci % len(TR_NS)]
    kind = tracking.KIND.get(code, 0)
    L = codes.code_length(code)
    rng = np.random.default_rng(300 + ci)
    K = 12
    prns = np.array(codes.prns(code))[rng.integers(0, 30, K)]
    chips, frac, incr = tr_specs(rng, L, K, codes.chip_rate(code) / 4.092e6)
    tr_check_phase_forms(L, chips, frac, incr, n)
    x = tr_x(rng, n)
    got = tracking.correlate_batch(code, x, prns, chips, frac, incr, engine=engine)
    dev = tracking.correlate_batch(code, torch.from_numpy(x).cuda(), prns, chips, frac, incr, engine=engine)
    assert got.tobytes() == dev.tobytes()
    want = tracking_oracle.correlate_many(code, x, prns, chips, frac, incr)
    err = np.abs(got - want)
    assert err.max() <= tr_bound(kind, x), (int(np.argmax(err)), float(err.max()), tr_bound(kind, x))


# cases whose first seeds drew a correlator where the reference's repeated additions straddle a chip boundary that the closed form
# does not (tr_check_phase_forms): replaced, as that check requires, by the next seed that passes
TR_RESEEDED = {("gps.l2cl", 5 * 4096 + 1, 127): 2}


@pytest.mark.gpu
@pytest.mark.parametrize("code,n,K", [(c, 5 * 4096 + 1, K) for c in ("galileo.e1b", "gps.l2cl") for K in (1, 127, 128, 129, 300)]
                         + [("gps.l1cp", 100000, 129)])
def test_gpu_correlator_batch_sizes_across_the_finish_grid(engine, code, n, K):
    """K on both sides of the finish kernel's 128-wide groups with a multi-chunk block (6 and 25 chunks, ragged tails), CBOC and the
    767 250-chip RZ code; host and device-resident calls byte-identical.  Includes the one-chip sensitivity check."""
    import torch
    from gnss_dsp_tools_amd import codes, tracking
    from oracle import codes_oracle, tracking_oracle
    kind = tracking.KIND[code]
    L = codes.code_length(code)
    rng = np.random.default_rng(K * 7 + n + TR_RESEEDED.get((code, n, K), 0))
    valid = np.array(codes.prns(code))
    prns = valid[np.arange(K) % 16]                       # 16 distinct tables (the oracle's L2CL generator is slow)
    chips, frac, incr = tr_specs(rng, L, K, codes.chip_rate(code) / 4.092e6)
    tr_check_phase_forms(L, chips, frac, incr, n)
    x = tr_x(rng, n)
    got = tracking.correlate_batch(code, x, prns, chips, frac, incr, engine=engine)
    dev = tracking.correlate_batch(code, torch.from_numpy(x).cuda(), prns, chips, frac, incr, engine=engine)
    assert got.tobytes() == dev.tobytes()
    want = tracking_oracle.correlate_many(code, x, prns, chips, frac, incr)
    bound = tr_bound(kind, x)
    err = np.abs(got - want)
    assert err.max() <= bound, (int(np.argmax(err)), float(err.max()), bound)
    if K == 1:
        # sensitivity: one chip the correlator reads, flipped, moves the oracle far outside the bound
        c01 = codes_oracle.chips(code, int(prns[0])).copy()
        c01[tracking_oracle.closed_form_indices(L, chips[0], frac[0], incr[0], 1)[0][0]] ^= 1
        flipped = tracking_oracle.correlate_many(code, x, prns[:1], chips[:1], frac[:1], incr[:1], chips01=c01)
        assert abs(flipped[0] - got[0]) > bound


@pytest.mark.gpu
def test_gpu_correlator_chip_table_cache_across_code_and_prn_changes(engine):
    """The context keeps the previous call's (code, PRN list) with its chip-table pointers.  A sequence that changes the code under the
    same PRNs, reorders the PRNs, grows the list and goes back to an earlier list must give, call by call, the bytes a fresh engine
    gives -- and match the oracle."""
    from gnss_dsp_tools_amd import acquire, tracking
    from oracle import tracking_oracle
    rng = np.random.default_rng(77)
    n = 5000
    x = tr_x(rng, n)
    seq = [("gps.ca", [1, 2, 3]), ("beidou.b1i", [1, 2, 3]), ("beidou.b1i", [3, 1, 2]), ("gps.ca", [3, 1, 2]), ("gps.ca", [1, 2, 3, 4]),
           ("gps.l1cd", [1, 2, 3, 4]), ("gps.ca", [1, 2, 3]), ("gps.ca", [1, 2, 3])]
    for code, prns in seq:
        frac = np.linspace(10.3, 900.7, len(prns))
        got = tracking.correlate_batch(code, x, prns, 0.0, frac, 0.2553, engine=engine)
        fresh = acquire.Engine(0)
        try:
            ref = tracking.correlate_batch(code, x, prns, 0.0, frac, 0.2553, engine=fresh)
        finally:
            fresh.close()
        assert got.tobytes() == ref.tobytes(), (code, prns)
        want = tracking_oracle.correlate_many(code, x, prns, 0.0, frac, 0.2553)
        assert np.abs(got - want).max() <= tr_bound(tracking.KIND.get(code, 0), x), (code, prns)


# ---------------------------------------------------------------------------------------------------------------- front-end

FE_TILE_GENERIC, FE_TILE_FIXED = 1024, 1280
# (fs_in, carrier offset, fs_out, cut-off as a fraction of fs_in/2): offsets 0, +-, near +-fs/2; down- and upsampling
FE_RATES = [(8.184e6, 0.0, 4.092e6, 0.45), (10.0e6, 1.25e6, 6.0e6, 0.5), (6.0e6, -2.9999e6, 8.0e6, 0.4),
            (16.368e6, 8.18e6, 4.0e6, 0.3), (5.0e6, -0.75e6, 5.5e6, 0.6)]


def fe_lengths(ntaps):
    """n_in just above the pad length, on each side of the generic and fixed kernels' output-tile boundaries (pass 2 tiles n, pass 1
    tiles n + 6 ntaps)"""
    lo = 3 * ntaps + 1
    out = {lo, lo + 1}
    for tile in (FE_TILE_GENERIC, FE_TILE_FIXED):
        for base in (0, 6 * ntaps):                       # n itself, or the extended length L = n + 2p
            m = -(-(lo + 1 + base) // tile)
            for d in (-1, 0, 1):
                if tile * m - base + d >= lo:
                    out.add(tile * m - base + d)
    return sorted(out)


def fe_run(engine, iq, fs_in, coffset, taps, fs_out, nout):
    import torch
    from gnss_dsp_tools_amd import _native as nat
    d = torch.from_numpy(np.ascontiguousarray(iq).reshape(-1)).to("cuda:0")
    engine.use_torch_stream(d.device)
    out = torch.empty(nout, dtype=torch.complex64, device=d.device)
    t = np.ascontiguousarray(taps, dtype=np.float64)
    nat.check(nat.lib.gacq_frontend_dev(engine._ctx, ctypes.c_void_p(d.data_ptr()), len(iq), float(fs_in), float(coffset),
                                        t.ctypes.data_as(nat.c_double_p), len(t), float(fs_out), nout, ctypes.c_void_p(out.data_ptr())),
              engine._ctx)
    torch.cuda.synchronize()
    return out.cpu().numpy().astype(np.complex128)


def fe_err(got, want, ntaps):
    """max error over all outputs, the first 3 ntaps and the last 3 ntaps, each relative to the signal RMS"""
    rms = np.sqrt(np.mean(np.abs(want) ** 2))
    e = np.abs(got - want) / rms
    edge = 3 * ntaps
    return float(e.max()), float(e[:edge].max()), float(e[-edge:].max())


@pytest.mark.gpu
@pytest.mark.parametrize("ntaps,generic", [(3, True), (4, True), (33, True), (160, True), (161, True), (161, False), (162, True), (512, True)],
                         ids=["3", "4", "33", "160", "161-generic", "161-fixed", "162", "512"])
def test_gpu_frontend_filter_lengths_and_tile_edges_match_scipy(engine, ntaps, generic):
    """gacq_frontend_dev at every filter length class (odd, even, tiny, 161 through either kernel, the 512-tap maximum) and at input
    lengths next to the pad length and to both kernels' tile boundaries, against firwin + filtfilt + np.interp (fp64).  Every case
    asks for two outputs past the last input sample (np.interp's clamp).  Criterion: 1e-5 of the signal RMS, over all outputs and
    over the first and last 3 ntaps on their own."""
    from gnss_dsp_tools_amd import acquire
    from oracle import frontend_oracle
    rng = np.random.default_rng(ntaps + 1000 * generic)
    engine.set_option("fe_generic", int(generic and ntaps == 161))
    try:
        for j, n_in in enumerate(fe_lengths(ntaps)):
            fs_in, coffset, fs_out, cut = FE_RATES[j % len(FE_RATES)]
            iq = rng.integers(-90, 90, size=(n_in, 2), dtype=np.int8)
            fsr = fs_out / fs_in
            nout = int((n_in - 1) * fsr) + 3
            assert (1 / fsr) * (nout - 1) > n_in - 1                         # the last outputs lie past the last input sample
            taps = acquire.firwin_hann(ntaps, cut)
            got = fe_run(engine, iq, fs_in, coffset, taps, fs_out, nout)
            want = frontend_oracle.condition_to(frontend_oracle.iq_to_complex(iq), fs_in, coffset, fs_out, cut * fs_in / 2, nout, ntaps)
            e_all, e_head, e_tail = fe_err(got, want, ntaps)
            assert max(e_all, e_head, e_tail) < 1e-5, (n_in, fs_in, coffset, fs_out, e_all, e_head, e_tail)
            if j == 0 and ntaps >= 4:
                # sensitivity: the reference shifted by one output sample, or filtered without its centre tap, is rejected
                shifted = np.concatenate([want[1:], want[-1:]])
                assert fe_err(got, shifted, ntaps)[0] > 1e-5
                h = taps.copy()
                h[ntaps // 2] = 0.0
                import scipy.signal
                y = scipy.signal.filtfilt(h, [1], frontend_oracle.mix_fixed_point(frontend_oracle.iq_to_complex(iq), -coffset / fs_in, 0))
                t = (1 / fsr) * np.arange(nout)
                zeroed = np.interp(t, np.arange(n_in), y.real) + 1j * np.interp(t, np.arange(n_in), y.imag)
                assert fe_err(got, zeroed, ntaps)[0] > 1e-5
    finally:
        engine.set_option("fe_generic", 0)


def test_frontend_lengths_cover_the_tile_edges():
    for ntaps in (3, 4, 33, 160, 161, 162, 512):
        ns = fe_lengths(ntaps)
        assert 3 * ntaps + 1 in ns and 3 * ntaps + 2 in ns
        for tile in (FE_TILE_GENERIC, FE_TILE_FIXED):
            assert any(n % tile == 0 for n in ns) and any(n % tile == tile - 1 for n in ns) and any(n % tile == 1 for n in ns)
            assert any((n + 6 * ntaps) % tile == 0 for n in ns)


def test_longcode_shapes_cover_every_candidate_group():
    kcs = {lc_kc(K, B, n): K % lc_kc(K, B, n) for _, _, _, K, B, n in LC_SHAPES}
    assert set(kcs) == {8, 4, 2, 1} and all(r != 0 for kc, r in kcs.items() if kc > 1)
    assert {1000, 4096, 4097, 3 * 4096 + 17, 65536} <= {n for *_, n in LC_SHAPES}


def test_closed_form_phase_is_the_single_rounded_value():
    """closed_form_indices models the kernel's fma(incr, i, cp0): one rounding of the exact phase.  Checked against exact rational
    arithmetic on decimal rates and start phases whose exact phases land on chip boundaries (where one or two roundings differ)."""
    import math
    from fractions import Fraction
    from oracle import tracking_oracle
    n = 4000
    for a, c in [(0.127875, 0.5999999999999943), (0.25575, 0.6), (2 * 0.127875, (2 * 77.3) % 2), (12 * 0.127875, (12 * 77.3) % 2),
                 (0.25, 0.5), (1.5345, 1022.7), (0.0, 3.0)]:
        got = tracking_oracle._floor_single_rounded(a, c, n)
        want = [math.floor(float(Fraction(a) * i + Fraction(c))) for i in range(n)]
        assert got.tolist() == want, (a, c)
    # the golden gps.l1cd case: sample 3200 is where the twice-rounded form and the reference part
    assert tracking_oracle._floor_single_rounded(2 * 0.127875, (2 * 77.3) % 2, 3201)[3200] == 818
    assert np.floor((2 * 77.3) % 2 + (2 * 0.127875) * 3200.0) == 819
