"""GPU parity: the HIP path (through the C ABI of libgacq.so) against
  (1) outputs of the reference itself (tests/golden/, fp64 numpy/scipy) and
  (2) the CPU oracle on fresh seeded inputs.
Bar (BASELINE.json north_star): identical peak location (code phase, Doppler bin) and metric within
1e-5 relative.  Chips are bit-exact (tests/test_native_cpu.py).  Nothing here reads /root/reference."""
import numpy as np
import pytest

from conftest import case_iq

pytestmark = pytest.mark.gpu

METRIC_RTOL = 1e-5          # the tolerance north_star states for floating point


def _assert_results(got, want, ctx):
    for g, w, item in zip(got, want, ctx["items"]):
        where = (ctx["id"], item, g, w)
        assert float(g[2]) == w[2], ("doppler",) + where
        assert float(g[1]) == pytest.approx(w[1], rel=1e-12, abs=1e-9), ("code",) + where
        assert float(g[0]) == pytest.approx(w[0], rel=METRIC_RTOL), ("metric",) + where


ALL_CASES = ["cfg1_gps_l1_prn1", "cfg2_gps_l1_all32", "gps_l1_ms3", "gps_l1_default_grid", "cfg3_e1b_subset",
             "cfg3_e1c_subset", "e1b_ms12", "cfg4_l5i_subset", "l5q_subset", "cfg4_b2ad_b80", "cfg5_b1i_ms10",
             "b2i_ms2", "cfg5_glonass_l1", "glonass_l2", "gps_l1cd", "bds_b1cp", "gps_l2cm", "gal_e6b", "gal_e5bq",
             "bds_b3i", "bds_b2bi", "glo_l3ocd", "xona_x1", "xona_x5p", "edge_empty_grid", "edge_zero_blocks_l1",
             "edge_zero_blocks_e1b", "edge_fractional_grid", "bds_b1cd", "gps_l1cp", "bds_b2ap", "bds_b2bq", "gal_e5ai", "gal_e5aq",
             "gal_e5bi", "gal_e6c", "glo_l3ocp"]
N4096_CASES = ["cfg1_gps_l1_prn1", "cfg2_gps_l1_all32", "gps_l1_ms3", "gps_l1_default_grid", "xona_x1",
               "edge_fractional_grid"]


@pytest.mark.parametrize("cid", ALL_CASES)
def test_search_matches_reference_golden(engine, golden_cases, cid):
    """Default engine selection (what a user gets)."""
    case = golden_cases[cid]
    x = case_iq(case)
    engine.set_engine(0)
    got = engine.search_all(case["script"], x, case["items"], case["doppler_search"], case["ms"])
    _assert_results(got, case["results"], case)
    from gnss_dsp_tools_amd import acquire
    if case["results"][0][2] != 0 or case["results"][0][0] != 0:
        for item, g, line in zip(case["items"], got, case["lines"]):
            mine = acquire.format_result(case["script"], item, g)
            # printed with 1-2 decimals: identical text unless the fp32 metric sits on a rounding edge
            assert mine.split("metric")[0] == line.split("metric")[0]
            assert mine.split("code_offset")[1] == line.split("code_offset")[1]


@pytest.mark.parametrize("cid", N4096_CASES)
@pytest.mark.parametrize("eng", [1, 2])
def test_both_engines_match_reference_golden(engine, golden_cases, cid, eng):
    """rocFFT pipeline (1) and LDS-resident FFT kernels (2) separately, where both apply (N = 4096)."""
    case = golden_cases[cid]
    x = case_iq(case)
    engine.set_engine(eng)
    try:
        got = engine.search_all(case["script"], x, case["items"], case["doppler_search"], case["ms"])
    finally:
        engine.set_engine(0)
    _assert_results(got, case["results"], case)


def test_single_search_signature_and_types(engine, golden_cases):
    """search(x, prn, doppler_search, ms) -> (np.float64, float, np.float64), like acquire-gps-l1.py:40."""
    from gnss_dsp_tools_amd import acquire
    case = golden_cases["cfg1_gps_l1_prn1"]
    x = case_iq(case)
    search = acquire.make_search("gps-l1", engine)
    m, c, d = search(x.astype(np.complex128), 1, case["doppler_search"], 1)
    assert isinstance(c, float) and isinstance(m, np.float64) and isinstance(d, np.float64)
    _assert_results([(m, c, d)], case["results"], case)
    code, dop, met = acquire.search_north_star(1, x, 4096000.0, case["doppler_search"], engine=engine)
    assert (met, code, dop) == (m, c, d)
    with pytest.raises(ValueError):
        acquire.search_north_star(1, x, 4000000.0, case["doppler_search"], engine=engine)
    # empty grid: the reference's untouched ints come back
    assert search(x, 1, [1000.0, 1000.0, 100.0], 1) == (0, 0, 0)


def test_rows_match_reference_rows(engine, golden_cases, golden_rows):
    """Full accumulated-magnitude rows q vs the reference's (stage-level check, rocFFT pipeline)."""
    from gnss_dsp_tools_amd import signals
    for key, want in golden_rows.items():
        cid, item, dop = key.split("|")
        case = golden_cases[cid]
        sig = signals.get(case["script"])
        q = engine.debug_row(sig, case_iq(case), int(item), float(dop), sig.blocks(case["ms"]))
        assert int(np.argmax(q)) == int(np.argmax(want)), key
        err = np.max(np.abs(q.astype(np.float64) - want)) / np.max(want)
        assert err < 5e-6, (key, err)
        assert np.sum(q.astype(np.float64)) == pytest.approx(np.sum(want), rel=1e-5)


def test_code_spectra_match_oracle(engine):
    from gnss_dsp_tools_amd import signals
    from oracle import acq_oracle, codes_oracle
    for name, prn in [("gps-l1", 7), ("beidou-b1i", 12), ("galileo-e1b", 3), ("gps-l5i", 9)]:
        sig = signals.get(name)
        s = engine.signal(sig, [prn])
        got = s.spectrum(prn).astype(np.complex128)
        want = acq_oracle.code_spectrum(codes_oracle.chips(sig.code, prn), sig.n, sig.pad, sig.boc)
        err = np.max(np.abs(got - want)) / np.max(np.abs(want))
        assert err < 2e-6, (name, err)


@pytest.mark.parametrize("name,items,ds,ms,seed", [
    ("gps-l1", [2, 9, 13, 30], [-3000.0, 3000.0, 250.0], 2, 101),
    ("gps-l1", [5], [-600.0, 650.0, 125.0], 5, 102),
    ("beidou-b1i", [1, 20], [-1000.0, 1000.0, 250.0], 3, 103),
    ("glonass-l1", [-3, 5], [-500.0, 700.0, 200.0], 2, 104),
    ("galileo-e6b", [11], [-400.0, 400.0, 200.0], 2, 105),
    ("galileo-e1c", [8], [1000.0, 2000.0, 250.0], 8, 106),
])
def test_search_matches_oracle_on_fresh_inputs(engine, name, items, ds, ms, seed):
    """Seeded inputs that are NOT in the goldens: HIP path vs the CPU oracle, same samples."""
    from gnss_dsp_tools_amd import signals, synth
    from oracle import acq_oracle
    sig = signals.get(name)
    sats = [(items[0], 0.3, 1537.0 if ds[0] <= 1537.0 < ds[1] else ds[0] + 0.4 * (ds[1] - ds[0]), 1234)]
    x = synth.make_iq(sig, sig.blocks(ms), seed, sats)
    got = engine.search_all(sig, x, items, ds, ms)
    want = [acq_oracle.search_script(name, x.astype(np.complex128), it, ds, ms) for it in items]
    _assert_results(got, [[float(v) for v in w] for w in want], {"id": name, "items": items})


def test_noise_only_near_ties_locate_like_oracle(engine):
    """Noise-only PRNs have near-tied peaks: location must still agree with the fp64 oracle."""
    from gnss_dsp_tools_amd import signals, synth
    from oracle import acq_oracle
    sig = signals.get("gps-l1")
    x = synth.make_iq(sig, 1, 777, [])
    items = list(range(1, 33))
    ds = [-5000.0, 5000.0, 250.0]
    for eng in (1, 2):
        engine.set_engine(eng)
        got = engine.search_all(sig, x, items, ds, 1)
        engine.set_engine(0)
        want = [acq_oracle.search_script("gps-l1", x.astype(np.complex128), it, ds, 1) for it in items]
        _assert_results(got, [[float(v) for v in w] for w in want], {"id": "noise-only/engine%d" % eng, "items": items})


def test_batched_device_path_equals_single_searches(engine):
    """gacq_search_batch_dev over E epochs == E independent gacq_search calls."""
    import torch
    from gnss_dsp_tools_amd import acquire, signals, synth
    sig = signals.get("gps-l1")
    items = list(range(1, 33))
    ds = [-5000.0, 5000.0, 250.0]
    dop = acquire.doppler_grid(ds)
    E = 11                                     # deliberately not a multiple of 8 (XCD mapping tail)
    sats = synth.default_sats(items)
    xs = synth.make_epochs(sig, 1, 4242, sats, E, nsamp=4096)
    xd = torch.from_numpy(xs).to("cuda:0")
    for eng in (1, 2):
        engine.set_engine(eng)
        peaks = engine.search_batch_dev(sig, xd, items, dop, 1)
        torch.cuda.synchronize()
        pk = peaks.cpu().numpy().view(acquire.PEAK_DTYPE).reshape(E, len(items))
        for e in range(E):
            batch = engine.finalize(sig, items, pk[e], dop)
            single = engine.search_all(sig, xs[e], items, ds, 1)
            assert batch == single, (eng, e)
        engine.set_engine(0)


@pytest.mark.parametrize("variant", [16, -1], ids=["radix16", "radix32"])
def test_glonass_fused_16k_kernel_equals_two_kernel_path(engine, variant):
    """One carrier per item (FDMA channels): forward + correlate run in one kernel without the X buffer.  Same arithmetic
    in the same order, so the peak records must be bit-identical to the forward-kernel + correlate-kernel path -- in both forms of the
    N = 16384 transform."""
    import os
    import torch
    from gnss_dsp_tools_amd import acquire, signals, synth
    sig = signals.get("glonass-l1")
    items = [-7, -3, 0, 2, 6]
    dop = acquire.doppler_grid([-3000.0, 3000.0, 500.0])
    B = 3
    xs = synth.make_epochs(sig, B, 99, synth.default_sats(items), 2)
    xd = torch.from_numpy(xs).to("cuda:0")
    try:
        engine.set_option("lds_variant", variant)
        engine.set_profiling(True)
        engine.reset_stage_times()
        fused = engine.search_batch_dev(sig, xd, items, dop, B)
        torch.cuda.synchronize()                                       # the engine launches on its own stream
        fused = fused.cpu().numpy()
        assert engine.stage_times()["mix_nco"][1] == 0                 # no separate forward launch
        engine.set_option("fused_16k", 0)
        engine.reset_stage_times()
        plain = engine.search_batch_dev(sig, xd, items, dop, B)
        torch.cuda.synchronize()
        plain = plain.cpu().numpy()
        assert engine.stage_times()["mix_nco"][1] == 1
    finally:
        engine.set_option("fused_16k", 1)
        engine.set_option("lds_variant", -1)
        engine.set_profiling(False)
    assert fused.tobytes() == plain.tobytes()


def test_streamed_host_batches_equal_resident_batches():
    """EpochStreamer (pinned double buffers, copy stream overlapped with compute) returns, batch by batch, the records of a
    plain device-resident gacq_search_batch_dev call on the same samples -- including after the staging slots wrap around."""
    import torch
    from gnss_dsp_tools_amd import acquire, signals, stream, synth
    sig = signals.get("gps-l1")
    items = [2, 5, 9, 17, 30]
    dop = acquire.doppler_grid([-2000.0, 2000.0, 250.0])
    E = 6
    batches = [synth.make_epochs(sig, 1, 500 + 10 * k, synth.default_sats(items), E, nsamp=4096) for k in range(7)]
    eng = acquire.Engine(0)
    try:
        st = stream.EpochStreamer(eng, sig, items, dop, 1, E, 4096, depth=3)
        got = list(st.run(iter(batches)))
        assert len(got) == len(batches)
        for k, xs in enumerate(batches):
            want = eng.search_batch_dev(sig, torch.from_numpy(xs).to("cuda:0"), items, dop, 1)
            torch.cuda.synchronize()
            want = want.cpu().numpy().view(acquire.PEAK_DTYPE).reshape(E, len(items))
            assert got[k].tobytes() == want.tobytes(), k
    finally:
        eng.close()


@pytest.mark.parametrize("names,items", [
    (("galileo-e1b", "galileo-e1c"), ([1, 11, 19], [11, 4])),
    (("gps-l5i", "gps-l5q"), ([3, 10], [10])),
])
def test_search_family_shares_forward_transforms_and_equals_separate_searches(engine, names, items):
    """E1B + E1C (BASELINE config 3) and friends in one pass: same records as one search_all per signal."""
    from gnss_dsp_tools_amd import signals, synth
    sig = signals.get(names[0])
    ds = [-1000.0, 1000.0, 250.0]
    ms = 8 if "galileo" in names[0] else 1
    B = sig.blocks(ms)
    x = synth.make_iq(sig, B, 4321, [(items[0][1], 0.4, 310.0, 777)])
    fam = engine.search_family(names, x, items, ds, ms)
    assert len(fam) == len(names)
    for name, it, got in zip(names, items, fam):
        want = engine.search_all(name, x, it, ds, ms)
        assert got == want, name
    again = engine.search_family(names, x, items, ds, ms)            # cached family signal
    assert again == fam
    # device-resident batched form (what bench.py --config 3 and sharded family jobs run): same records
    import torch
    from gnss_dsp_tools_amd import acquire
    dop = acquire.doppler_grid(ds)
    xd = torch.from_numpy(np.stack([x[:sig.samples_needed(B)]] * 2)).cuda()
    pk = engine.search_family_batch_dev(names, xd, items, dop, B)
    torch.cuda.synchronize()
    pk = pk.cpu().numpy().view(acquire.PEAK_DTYPE).reshape(2, -1)
    flat = [r for f in fam for r in f]
    for e in range(2):
        assert acquire.finalize(sig, list(range(len(flat))), pk[e], dop) == flat
    with pytest.raises(ValueError):
        engine.search_family(("gps-l1", "gps-l5i"), x, ([1], [1]), ds, 1)


def test_full_size_config3_family_e1b_plus_e1c_72_rows(engine):
    """BASELINE config 3 as it is defined: E1B + E1C, 36 PRNs each, Doppler arange(-4000,4000,125) = 64 bins, ms = 8 (B = 1),
    N = 65536, searched as ONE 72-row family (mix and forward transforms shared by both signals).  Every record equals the
    one of the separate per-signal searches, and the injected satellites of both signals sit at their delays."""
    from gnss_dsp_tools_amd import codes, signals, synth
    names = ("galileo-e1b", "galileo-e1c")
    items = (list(range(1, 37)), list(range(1, 37)))
    ds, ms = [-4000.0, 4000.0, 125.0], 8
    sig = signals.get(names[0])
    B = sig.blocks(ms)
    assert B == 1
    n = sig.n
    x = synth.make_iq(sig, B, 3636, [(5, 0.4, 1537.0, 1201), (30, 0.3, -3262.0, 20077)], nsamp=sig.samples_needed(B)).astype(np.complex128)
    i = np.arange(len(x))
    rep = codes.replica("galileo.e1c", 17, n, True).astype(np.float64)           # an E1C satellite on top of the two E1B ones
    x = (x + 0.35 * rep[(i - 9000) % n] * np.exp(2j * np.pi * 409.0 * i / sig.fs)).astype(np.complex64)
    fam = engine.search_family(names, x, items, ds, ms)
    assert [len(f) for f in fam] == [36, 36]
    for name, it, got in zip(names, items, fam):
        assert got == engine.search_all(name, x, it, ds, ms), name
    L = 4092
    for k, prn, delay in [(0, 5, 1201), (0, 30, 20077), (1, 17, 9000)]:
        code = fam[k][prn - 1][1]
        assert any(abs(code - (L * ((n * m - delay) % (2 * n)) / n) % L) < 1e-9 for m in (1, 2)), (names[k], prn, code)


def test_finalize_shard_merge(engine):
    """Doppler grid cut into shards, searched separately, merged by gacq_finalize == unsharded search.
    This is the cross-GPU exchange step exercised on one device."""
    import torch
    from gnss_dsp_tools_amd import acquire, signals, synth
    sig = signals.get("gps-l1")
    items = list(range(1, 33))
    ds = [-5000.0, 5000.0, 250.0]
    dop = acquire.doppler_grid(ds)
    x = synth.make_iq(sig, 1, 991, synth.default_sats(items))
    full = engine.search_all(sig, x, items, ds, 1)
    xd = torch.from_numpy(x[None, :4096].copy()).to("cuda:0")
    for nshard in (2, 4, 8, 40):
        bounds = [(s * len(dop)) // nshard for s in range(nshard + 1)]
        parts = []
        for s in range(nshard):
            pk = engine.search_batch_dev(sig, xd, items, dop[bounds[s]:bounds[s + 1]], 1)
            torch.cuda.synchronize()
            parts.append(pk.cpu().numpy().view(acquire.PEAK_DTYPE).reshape(len(items)))
        merged = engine.finalize(sig, items, np.stack(parts), dop, shard_d0=bounds[:-1])
        assert merged == full, nshard


def test_error_behaviour(engine):
    from gnss_dsp_tools_amd import _native as nat
    from gnss_dsp_tools_amd import signals
    x = np.zeros(4000, dtype=np.complex64)
    with pytest.raises(ValueError):               # the reference raises numpy's broadcast ValueError here
        engine.search("gps-l1", x, 1, [-500.0, 500.0, 500.0], 1)
    with pytest.raises(nat.GacqError):
        engine.signal(signals.get("gps-l1"), [999])
    with pytest.raises(nat.GacqError) as ei:
        engine.set_engine(2)
        try:
            engine.search("galileo-e6b", np.zeros(4 * 15345, dtype=np.complex64), 1, [0.0, 200.0, 200.0], 1)
        finally:
            engine.set_engine(0)
    assert ei.value.code == -9


def test_c_abi_rejects_bad_arguments_with_codes_not_crashes(engine):
    """Straight through ctypes: NULL pointers, negative counts, out-of-range item indices, short inputs and NaN Doppler values
    come back as negative GACQ_ERR_* codes with a message; the context stays usable afterwards."""
    import ctypes
    from gnss_dsp_tools_amd import _native as nat
    from gnss_dsp_tools_amd import signals, synth
    lib = nat.lib
    sig = signals.get("gps-l1")
    s = engine.signal(sig, [1, 2, 3])
    x = synth.make_iq(sig, 1, 11, [(2, 0.5, 1000.0, 100)], nsamp=4096)
    xp = x.ctypes.data_as(nat.c_float_p)
    items = np.array([0, 1, 2], dtype=np.int32)
    dop = np.array([500.0, 1000.0, 1500.0])
    res = (nat.Result * 3)()

    def call(xptr=xp, nsamp=4096, it=items, nit=3, dp=dop, nd=3, blocks=1, out=res):
        return lib.gacq_search(s._h, xptr, nsamp, it.ctypes.data_as(nat.c_int_p) if it is not None else None, nit,
                               dp.ctypes.data_as(nat.c_double_p) if dp is not None else None, nd, None, blocks, out)

    assert call() == 0
    good = [(r.metric, r.code_chips, r.doppler_hz) for r in res]
    assert call(xptr=None) < 0
    assert call(it=None) < 0
    assert call(dp=None) < 0
    assert call(out=None) < 0
    assert call(nit=-1) < 0
    assert call(nd=-2) < 0
    assert call(blocks=-1) < 0
    assert call(nsamp=4095) == -6                                        # GACQ_ERR_SHORT_INPUT
    assert call(it=np.array([0, 7, 1], dtype=np.int32)) < 0               # item index outside the signal's table
    assert call(it=np.array([0, -1, 1], dtype=np.int32)) < 0
    assert lib.gacq_last_error(engine._ctx)                               # a message is available
    assert lib.gacq_search(None, xp, 4096, items.ctypes.data_as(nat.c_int_p), 3, dop.ctypes.data_as(nat.c_double_p), 3, None, 1, res) < 0
    assert lib.gacq_set_engine(engine._ctx, 9) < 0
    assert lib.gacq_set_workspace_limit(engine._ctx, 10) < 0
    # a frequency whose phase index leaves the 32-bit range is refused, not wrapped
    assert call(dp=np.array([1e30, 0.0, 1.0])) < 0
    assert call(dp=np.array([0.0, float("nan"), 1.0])) < 0
    assert call(dp=np.array([0.0, float("inf"), 1.0])) < 0
    # round-4 entry points: NULL device pointers, bad kinds and counts come back as codes as well
    import torch
    xd = torch.from_numpy(x).cuda()
    q = np.zeros(4)
    ph = np.zeros(4)
    ip, dp_ = items.ctypes.data_as(nat.c_int_p), dop.ctypes.data_as(nat.c_double_p)
    assert lib.gacq_longcode_search_dev(engine._ctx, None, 4096, 4.096e6, b"gps.l2cl", 1, 0.0, ph.ctypes.data_as(nat.c_double_p), 4, 1, 4096,
                                        q.ctypes.data_as(nat.c_double_p)) < 0
    assert lib.gacq_longcode_search_dev(engine._ctx, ctypes.c_void_p(xd.data_ptr()), 4096, 4.096e6, b"gps.nope", 1, 0.0,
                                        ph.ctypes.data_as(nat.c_double_p), 4, 1, 4096, q.ctypes.data_as(nat.c_double_p)) < 0
    assert lib.gacq_correlate_batch_dev(engine._ctx, None, 4096, b"gps.ca", 0, ip, dp_, dp_, dp_, 3, q.ctypes.data_as(nat.c_double_p)) < 0
    assert lib.gacq_correlate_batch_dev(engine._ctx, ctypes.c_void_p(xd.data_ptr()), 4096, b"gps.ca", 9, ip, dp_, dp_, dp_, 3,
                                        q.ctypes.data_as(nat.c_double_p)) < 0
    assert lib.gacq_mix_int8_dev(engine._ctx, None, 4096, 4.096e6, 0.0, ctypes.c_void_p(xd.data_ptr())) < 0
    pk = torch.zeros((2, 1, 3, 2), dtype=torch.float64, device="cuda")
    d0 = np.array([0, 2], dtype=np.int32)
    args = (s._h, ctypes.c_void_p(xd.data_ptr()), 4096, 1, ip, 3, dp_, 3, None, 1)
    assert lib.gacq_merge_peaks_tiesafe_dev(*args, None, 2, d0.ctypes.data_as(nat.c_int_p), ctypes.c_void_p(pk[0].data_ptr())) < 0
    assert lib.gacq_merge_peaks_tiesafe_dev(*args, ctypes.c_void_p(pk.data_ptr()), 0, d0.ctypes.data_as(nat.c_int_p), ctypes.c_void_p(pk[0].data_ptr())) < 0
    assert lib.gacq_merge_peaks_tiesafe_dev(*args, ctypes.c_void_p(pk.data_ptr()), 2, d0.ctypes.data_as(nat.c_int_p), ctypes.c_void_p(pk[0].data_ptr())) == 0
    v = ctypes.c_double()
    assert lib.gacq_stream_probe(engine._ctx, 9, 1 << 24, 2, ctypes.byref(v)) < 0 and lib.gacq_stream_probe(engine._ctx, 0, 1 << 24, 0, ctypes.byref(v)) < 0
    assert lib.gacq_get_tie_stats(engine._ctx, None) < 0 and lib.gacq_get_tie_stats(None, (ctypes.c_longlong * 4)()) < 0
    # the context still works and returns the same answer
    assert call() == 0
    assert [(r.metric, r.code_chips, r.doppler_hz) for r in res] == good


# ---- full BASELINE sizes: size-independent properties ---------------------------------------------
def test_full_size_properties_config2(engine):
    """Config 2 at full size (32 PRNs x 40 bins x 4096 lags, 64 epochs batched):
    (a) circularly shifting x by s samples moves every detected peak by -s lags (unpadded search is circular);
    (b) scaling x leaves the normalised metric unchanged;
    (c) both engines agree on every (epoch, PRN) location."""
    import torch
    from gnss_dsp_tools_amd import acquire, signals, synth
    sig = signals.get("gps-l1")
    items = list(range(1, 33))
    dop = acquire.doppler_grid([-5000.0, 5000.0, 250.0])
    sats = synth.default_sats(items)
    E = 64
    xs = synth.make_epochs(sig, 1, 31337, sats, E, nsamp=4096)
    s = 357
    xd = torch.from_numpy(xs).to("cuda:0")
    xd_shift = torch.roll(xd, s, dims=1).contiguous()
    xd_scale = (xd * 3.0).contiguous()
    torch.cuda.synchronize()            # torch wrote these on its stream; the engine launches on its own (non-blocking) stream

    def run(t, eng):
        engine.set_engine(eng)
        pk = engine.search_batch_dev(sig, t, items, dop, 1)
        torch.cuda.synchronize()
        engine.set_engine(0)
        return pk.cpu().numpy().view(acquire.PEAK_DTYPE).reshape(E, len(items))

    base = run(xd, 2)
    shifted = run(xd_shift, 2)
    scaled = run(xd_scale, 2)
    other = run(xd, 1)
    sat_cols = [items.index(it) for it, *_ in sats]
    for (it, amp, f, delay), c in zip(sats, sat_cols):
        if amp < 0.25:
            continue
        # the NCO phase restarts at the block start, so a circular shift of x only adds a constant carrier
        # phase: the correlation peak moves by exactly -s lags (mod 4096); the injected Dopplers sit between two
        # bins, so the winning bin may flip to its neighbour (different noise after the wrap), never further
        assert np.all((shifted["idx"][:, c] - base["idx"][:, c]) % 4096 == (-s) % 4096), it
        assert np.all(np.abs(shifted["d_index"][:, c] - base["d_index"][:, c]) <= 1), it
    np.testing.assert_array_equal(scaled["idx"], base["idx"])
    np.testing.assert_array_equal(scaled["d_index"], base["d_index"])
    np.testing.assert_allclose(scaled["metric"], base["metric"], rtol=2e-6)
    np.testing.assert_array_equal(other["idx"], base["idx"])
    np.testing.assert_array_equal(other["d_index"], base["d_index"])
    np.testing.assert_allclose(other["metric"], base["metric"], rtol=5e-6)
    # detection sanity at full size: the four injected satellites sit at their delays in every epoch
    for (it, amp, f, delay), c in zip(sats, sat_cols):
        if amp >= 0.25:
            assert np.all(base["idx"][:, c] == (-delay) % 4096), it


FULL_SIZE = [
    # BASELINE configs 3, 4, 5 at their full (P, D, B, N): name, items, doppler_search, ms (None = engine-level B = 1)
    ("galileo-e1b", list(range(1, 37)), [-4000.0, 4000.0, 125.0], 8),
    ("gps-l5i", list(range(1, 33)), [-7000.0, 7000.0, 200.0], 1),
    ("beidou-b2ad", list(range(1, 64)), [-7000.0, 7000.0, 200.0], None),
    ("beidou-b1i", list(range(1, 64)), [-10000.0, 10000.0, 100.0], 10),
    ("glonass-l1", list(range(-7, 8)), [-10000.0, 10000.0, 100.0], 10),
    ("galileo-e1b", list(range(1, 51)), [-10000.0, 10000.0, 100.0], 10),
    ("gps-l1", list(range(1, 33)), [-10000.0, 10000.0, 100.0], 10),              # config 5's GPS L1 leg: P=32, D=200, B=10, max/mean metric
]


@pytest.mark.parametrize("name,items,ds,ms", FULL_SIZE, ids=["cfg3-e1b", "cfg4-l5i", "cfg4-b2ad", "cfg5-b1i", "cfg5-glonass", "cfg5-e1b", "cfg5-gps-l1"])
def test_full_size_properties_configs_3_4_5(engine, name, items, ds, ms):
    """Full BASELINE shapes, too big for the oracle in a test: (a) the hand-written engine and the rocFFT pipeline (two
    independent transform implementations) agree on every item's (lag, Doppler bin) and on the metric to 5e-6;
    (b) linearity: 2.5 x the samples gives the same locations and 2.5 x the raw metric; (c) every injected satellite
    is found at its delay."""
    import torch
    from gnss_dsp_tools_amd import acquire, signals, synth
    sig = signals.get(name)
    B = 1 if ms is None else sig.blocks(ms)
    dop = acquire.doppler_grid(ds)
    sats = synth.default_sats(items)
    x = synth.make_iq(sig, B, 2468, sats, nsamp=sig.samples_needed(B))
    xd = torch.from_numpy(x[None, :]).to("cuda:0")

    def run(t, eng):
        engine.set_engine(eng)
        try:
            pk = engine.search_batch_dev(sig, t, items, dop, B)
            torch.cuda.synchronize()
        finally:
            engine.set_engine(0)
        return pk.cpu().numpy().view(acquire.PEAK_DTYPE).reshape(len(items))

    auto = run(xd, 0)
    ref = run(xd, 1)
    np.testing.assert_array_equal(auto["idx"], ref["idx"])
    np.testing.assert_array_equal(auto["d_index"], ref["d_index"])
    np.testing.assert_allclose(auto["metric"], ref["metric"], rtol=5e-6)
    xs25 = (xd * 2.5).contiguous()
    torch.cuda.synchronize()            # written on torch's stream, read on the engine's own stream: order them
    scaled = run(xs25, 0)
    np.testing.assert_array_equal(scaled["idx"], auto["idx"])
    np.testing.assert_array_equal(scaled["d_index"], auto["d_index"])
    # raw metrics scale with the samples; the normalised max/mean metric (GPS L1) does not change at all
    np.testing.assert_allclose(scaled["metric"], (1.0 if sig.normalised else 2.5) * auto["metric"], rtol=5e-6)
    n = sig.n
    for it, amp, f, delay in sats:
        if amp >= 0.25:
            # padded searches see two code periods in the 2n window: the peak sits at n - d or 2n - d (equal but for noise)
            assert auto["idx"][items.index(it)] % n == (n - delay % n) % n, (it, delay)


@pytest.mark.parametrize("config,extra", [(2, ["--epochs", "8"]), (3, ["--epochs", "1"]), (4, ["--epochs", "1"]), (5, ["--epochs", "1"])])
def test_bench_under_torchrun_single_rank_exercises_rccl_path(config, extra):
    """The driver launches N>1 through torch.distributed.run; with one GPU the same launcher + --force-gather still
    exercises RCCL init, the single all-gather of every signal's peak records on the engine's stream, the device-side
    merge, the shard census and the barrier/max-reduce timing code -- for the headline config and for the multi-signal
    configs 4 and 5 (ShardedSearch.search_jobs_async), i.e. what `bench.py --gpus 8 --config 4` runs on a node."""
    import json
    import os
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--config", str(config), "--force-gather", "--full", "--no-cpu-baseline", "--no-pmc", "--sustained-s", "0.2"] + extra
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=root)
    assert out.returncode == 0, out.stderr[-3000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("{")][-1]
    j = json.loads(line)
    assert j["n_gpus"] == 1 and j["value"] > 1e9 and j["roofline"]["kernel"]
    assert j["roofline"]["bound"] in ("valu", "hbm") and 0.0 < j["roofline"]["frac"] < 1.0        # a fraction of a real ceiling
    assert j["config"]["baseline_config"] == config and j["config"]["shards_seen_by_every_rank"] == 1
    assert j["sustained"]["seconds"] >= 0.2 and len(j["roofline"]["per_rank"]) == 1


def test_bench_torchrun_single_rank_value_equals_the_plain_run():
    """The driver takes the N = 1 point of the scaling curve from a plain `python bench.py --gpus 1` and the N > 1 points from
    torchrun launches: the two launch styles must measure the same thing.  Same steps, sustained region (--full) of 1 s each, the torchrun
    run with its (one-rank) RCCL exchange and merge inside the timed region: the sustained values agree within 3 % (two processes,
    two clock ramps; the kernels are the same)."""
    import json
    import os
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    common = [os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "3", "--full", "--no-cpu-baseline", "--no-pmc",
              "--no-others", "--no-latency", "--sustained-s", "1.0"]
    vals = {}
    for label, cmd in (("plain", [sys.executable] + common),
                       ("torchrun", [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
                                     "--master-port", str(port)] + common)):
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=root)
        assert out.returncode == 0, (label, out.stderr[-3000:])
        j = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
        vals[label] = j["sustained"]["value"]
        assert j["n_gpus"] == 1 and j["config"]["baseline_config"] == 2
    assert abs(vals["torchrun"] / vals["plain"] - 1.0) < 0.03, vals


def test_bench_measures_hbm_traffic_live_with_pmc_child_runs(tmp_path):
    """bench.py's roofline.traffic is measured in the run itself: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE child runs of the same
    command (separate passes).  The fused N = 4096 kernel must read each epoch's samples and write 16-byte peak records: the
    measured bytes per launch lie between the algorithmic floor (x in) and a few times it (code spectra + twiddle re-reads).
    The side runs are checked in the complete record (--details-json); the printed line carries their headline numbers and stays
    short enough for the driver to read."""
    import json
    import os
    import shutil
    import subprocess
    import sys
    if not (shutil.which("rocprofv3") or os.path.exists("/opt/rocm/bin/rocprofv3")):
        pytest.skip("rocprofv3 not installed")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    E = 1024
    details = tmp_path / "details.json"
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--steps", "3", "--warmup", "1", "--epochs", str(E), "--full", "--no-cpu-baseline",
           "--no-latency", "--sustained-s", "0", "--preroll-s", "0", "--details-json", str(details)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=root)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1 and len(lines[0]) < 12 * 1024, [len(l) for l in lines]
    line = json.loads(lines[0])
    j = json.load(open(details))
    assert line["value"] == j["value"] and line["ms_per_step"] == j["ms_per_step"] and line["roofline"] == j["roofline"]
    assert [(c["baseline_config"], c["value"]) for c in line["other_configs"]] == [(c["baseline_config"], c["value"]) for c in j["other_configs"]]
    assert line["reference_precision"]["value"] == j["reference_precision"]["value"]
    assert set(line["next_rows"]) == set(j["next_rows"])
    src = j["roofline"]["traffic_source"]
    assert src["measured_in_this_run"] is True, src
    x_bytes = E * 4096 * 8
    assert x_bytes <= j["roofline"]["traffic"] <= 40 * x_bytes, (j["roofline"]["traffic"], x_bytes)
    assert 0.3 < src["valu_pipe_busy_pmc"] <= 1.0
    assert src["launches_averaged"] >= 3
    # the full single-GPU headline run also carries the other BASELINE configurations and the complex128 leg (round 3)
    others = j["other_configs"]
    assert [c["baseline_config"] for c in others] == [3, 4, 5] and not any("error" in c for c in others), others
    for c in others:
        assert c["value"] > 1e10 and c["seconds_timed"] >= 1.0 and c["bound"] in ("valu", "hbm") and 0.0 < c["frac"] < 1.0, c
        assert c["traffic_measured_in_this_run"] and c["traffic_measured_bytes_per_launch"] >= 0.9 * c["compulsory_hbm_bytes_per_launch"], c
    ref = j["reference_precision"]
    assert ref["dtype"] == "f64" and ref["value"] > 1e9 and ref["seconds_timed"] >= 1.0, ref
    agree = ref["f32_vs_f64_on_the_same_1024_epochs"]
    assert agree["searches"] == 1024 * 32 and agree["peak_location_mismatches"] == 0 and agree["max_rel_metric_error"] < 1e-5, agree
    # round 4: the complex128 leg is one fused kernel per search with its own roofline entry, the fp32 engine timed in the same loop
    rr = ref["roofline"]
    assert rr["kernel"] == "fused4k_c128_kernel" and rr["peak"] == 78.6 and 0.05 < rr["frac"] < 1.0 and rr["avg_kernel_ms"] <= 1.02 * ref["ms_per_step"], rr      # (the events are taken in a short pass after the timed loop: same rate within the clock drift)
    assert ref["value"] > 1.5e11 and ref["f32_same_loop"]["seconds_timed"] >= 1.0, ref
    assert abs(ref["f32_over_f64"] - ref["f32_same_loop"]["value"] / ref["value"]) < 1e-9
    # round 4: the rows either side of the FFT search, the live stream ceilings and the tie-safe counters are in the driver-visible line
    nr = j["next_rows"]
    assert set(nr) == {"frontend", "longcode_l2cl", "longcode_glonass_p", "tracking_epl"}, nr
    assert 0.0 < nr["frontend"]["frac_hbm_8TBps"] < 1.0 and 0.0 < nr["frontend"]["frac_fp32_vector_peak"] < 1.0 and nr["frontend"]["calls_timed"] >= 3
    assert nr["longcode_l2cl"]["k_found"] == nr["longcode_l2cl"]["k_injected"] and nr["longcode_glonass_p"]["k_found"] == nr["longcode_glonass_p"]["k_injected"]
    assert 0.0 < nr["tracking_epl"]["us_resident_block"] < nr["tracking_epl"]["us_host_block"] < 500.0
    assert j["tie_safe"]["enabled"] is True and j["tie_safe"]["kept_fp32"] == 0, j["tie_safe"]
    # round 6: two steps in flight on hardware queues of their own by default; the one-step-in-flight time of the same process is in the
    # line, and the profiling pass (one step in flight) holds the kernel time against its own step time
    assert j["config"]["steps_in_flight"] == 2 and j["config"]["one_step_in_flight"]["steps_in_flight"] == 1
    assert 0.8 < j["config"]["one_step_in_flight"]["ms_per_step"] / j["ms_per_step"] < 1.3, j["config"]["one_step_in_flight"]
    assert set(j["roofline"]["ab"]["steps_in_flight"]) == {"one_ms_per_step", "2_ms_per_step"}
    assert j["roofline"]["profiling_pass"]["kernel_time_within_its_own_step"] is True
    assert all(c["steps_in_flight"] == 2 and c["one_step_in_flight"]["ms_per_step"] > 0 for c in others)
    for c in others:
        if c["bound"] == "hbm":
            sc = c["stream_ceiling"]
            assert sc["measured_in_this_run"] is True and 2000.0 < sc["GBps"] < 8000.0 and (sc.get("exceeded_by_kernel") or 0.0 < sc["frac"] <= 1.0), sc


def test_plain_bench_run_is_the_headline_alone(tmp_path):
    """A plain `bench.py --gpus 1 --steps N --warmup W` sets up, warms up, times the N steps, writes --dump-outputs and prints the line:
    the headline fields, none of what --full adds, and at most 30 s of the process's wall time outside its N + W steps."""
    import json
    import os
    import subprocess
    import sys
    import time
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    details, dump = tmp_path / "details.json", tmp_path / "dump"
    steps, warmup = 20, 3
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
           "--dump-outputs", str(dump), "--details-json", str(details)]
    t0 = time.perf_counter()
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=root)
    wall = time.perf_counter() - t0
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, lines
    j = json.loads(lines[0])
    assert j["unit"] == "cells/s" and j["higher_is_better"] is True and j["dtype"] == "f32" and j["metric"].startswith("acquisition cells/s")
    assert j["steps"] == steps and j["warmup"] == warmup and j["value"] > 1e11
    assert abs(j["value"] * j["ms_per_step"] * 1e-3 - j["config"]["cells_per_step"]) <= 1e-9 * j["config"]["cells_per_step"]
    for k in ("other_configs", "reference_precision", "next_rows", "tie_safe", "cpu_baseline_pool", "gpu_over_cpu", "bench_wall_s"):
        assert k not in j, k
    assert j["roofline"] is None and j["sustained"] is None and j["host_call_latency"] is None and j["cpu_baseline"] is None
    assert j["config"]["one_step_in_flight"] is None and j["pipeline"]["per_signal"] is None
    assert json.load(open(details)) == j                  # nothing cut: the record is the line
    assert sorted(os.listdir(dump)) == ["gps-l1_code_index.npy", "gps-l1_doppler_index.npy", "gps-l1_metric.npy"]
    outside = wall - (steps + warmup) * j["ms_per_step"] * 1e-3
    assert outside < 30.0, (wall, j["ms_per_step"])


def test_alternating_between_more_grids_than_the_cache_holds(engine):
    """The context keeps the device buffers of the last eight (frequency grid, item list) pairs, so that callers alternating between a few
    grids -- several signals per step, a rank's slice and the full grid of the tie-safe merge -- pay no upload / synchronisation per call.
    Ten different grids in rotation (more than the cache holds: hits, swaps and evictions all occur), three rounds, asynchronously on one
    stream: every result equals the one a fresh context computes for that grid alone."""
    import torch
    from gnss_dsp_tools_amd import acquire, signals, synth
    sig = signals.get("gps-l1")
    xs = synth.make_epochs(sig, 1, 4711, synth.default_sats([3, 11, 19, 28]), 2, nsamp=4096)
    xd = torch.from_numpy(xs).cuda()
    grids = [(list(range(1 + k, 9 + k)), acquire.doppler_grid([-2000.0 + 100.0 * k, 2000.0, 250.0 + 10.0 * k])) for k in range(10)]
    want = []
    for items, dop in grids:
        e = acquire.Engine(0)
        try:
            e.use_torch_stream()
            r = e.search_batch_dev(sig, xd, items, dop, 1)
            torch.cuda.synchronize()
            want.append(r.cpu().numpy().tobytes())
        finally:
            e.close()
    engine.use_torch_stream()
    outs = []
    for rnd in range(3):
        order = range(10) if rnd != 1 else [3, 3, 9, 0, 5, 1, 8, 2, 7, 4, 6, 0]
        for k in order:
            outs.append((k, engine.search_batch_dev(sig, xd, grids[k][0], grids[k][1], 1)))      # no synchronisation in between
    torch.cuda.synchronize()
    for k, r in outs:
        assert r.cpu().numpy().tobytes() == want[k], k


def test_stream_probe_measures_plausible_hbm_rates(engine):
    """gacq_stream_probe: a tuned fill / read / copy kernel on this device (what bench.py holds the HBM-bound kernels against): between a
    quarter of and the full 8 TB/s of the data sheet, read >= fill (stores are the slower direction on this part), and bad arguments rejected."""
    from gnss_dsp_tools_amd import _native as nat
    r = {k: engine.stream_probe(k, 1 << 30, 4) for k in ("fill", "read", "copy")}
    assert all(2000.0 < v < 8000.0 for v in r.values()), r
    assert r["read"] > r["fill"] * 0.95, r
    with pytest.raises(nat.GacqError):
        engine.stream_probe("fill", 1000, 4)


def test_bench_rank_slice_projection_mode():
    """bench.py --emulate-ranks N: every rank's Doppler slice of an N-rank job timed on this one GPU, labelled as a projection."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--config", "2", "--epochs", "16", "--emulate-ranks", "4"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=root)
    assert out.returncode == 0, out.stderr[-3000:]
    j = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert j["projection"] is True and "NOT A MEASUREMENT" in j["note"] and j["ranks_emulated"] == 4
    assert [p["doppler_bins"] for p in j["per_rank"]] == [[10]] * 4 and j["epochs_per_step"] == 64
    assert j["slowest_slice_ms"] == max(p["ms_per_step"] for p in j["per_rank"]) and 0.2 < j["projected_efficiency"] < 1.3


R31_CASES = ["cfg4_l5i_subset", "l5q_subset", "cfg4_b2ad_b80", "gal_e6b", "gal_e5bq", "bds_b3i", "bds_b2bi", "glo_l3ocd",
             "xona_x5p", "bds_b2ap", "bds_b2bq", "gal_e5ai", "gal_e5aq", "gal_e5bi", "gal_e6c", "glo_l3ocp"]


# engine 3 at N = 61380 / 30690: the prime-factor form with the DFT-31 on the VALU (default) / on the matrix pipe, and the
# Cooley-Tukey form with rocFFT inner transforms (GACQ_OPT_FUSED_INNER 0) -- next to the rocFFT pipeline four different arithmetic paths
R31_FORMS = {"rocfft-pipeline": (1, 1, 0), "pfa-valu": (3, 1, 0), "pfa-mfma": (3, 1, 1), "ct-rocfft": (3, 0, 0)}


@pytest.mark.parametrize("cid", R31_CASES)
@pytest.mark.parametrize("form", sorted(R31_FORMS))
def test_radix31_split_and_rocfft_match_reference_golden(engine, golden_cases, cid, form):
    """N = 61380 / 30690: rocFFT (Bluestein) pipeline (1) and every form of the radix-31 split engine (3) separately."""
    case = golden_cases[cid]
    x = case_iq(case)
    eng, fused, mfma = R31_FORMS[form]
    engine.set_engine(eng)
    engine.set_option("fused_inner", fused)
    engine.set_option("split_mfma", mfma)
    try:
        got = engine.search_all(case["script"], x, case["items"], case["doppler_search"], case["ms"])
    finally:
        engine.set_engine(0)
        engine.set_option("fused_inner", 1)
        engine.set_option("split_mfma", 0)
    _assert_results(got, case["results"], case)


def test_radix31_rows_match_oracle(engine):
    """Stage-level check of engine 3: full q rows (padded N=61380, B=2; unpadded N=30690, B=3) vs the fp64 oracle."""
    from gnss_dsp_tools_amd import signals, synth
    from oracle import acq_oracle, codes_oracle
    for name, prn, dop, B in [("gps-l5i", 7, 1600.0, 2), ("xona-x5p", 0, -400.0, 3), ("galileo-e6c", 4, 200.0, 1)]:
        sig = signals.get(name)
        x = synth.make_iq(sig, B, 4711, [(prn, 0.3, dop - 63.0, 1201)])
        want = acq_oracle.search_row(x.astype(np.complex128), codes_oracle.chips(sig.code, prn), dop, B, fs=sig.fs, n=sig.n,
                                     pad=sig.pad, boc=sig.boc)
        for mfma in (0, 1):                          # the lag labels of both inverse outer kernels of the prime-factor form
            engine.set_engine(3)
            engine.set_option("split_mfma", mfma)
            try:
                q = engine.debug_row(sig, x, prn, dop, B)
            finally:
                engine.set_engine(0)
                engine.set_option("split_mfma", 0)
            assert int(np.argmax(q)) == int(np.argmax(want)), (name, mfma)
            err = np.max(np.abs(q.astype(np.float64) - want)) / np.max(want)
            assert err < 5e-6, (name, mfma, err)
            assert np.sum(q.astype(np.float64)) == pytest.approx(np.sum(want), rel=1e-5)


def test_radix31_code_spectrum_is_a_permutation_of_the_natural_one(engine):
    """Engine 3 stores spectra in its own order (the prime-factor maps of gacq_pfa.hip, or [k1][k2] with k = k1 + 31 k2 for the
    Cooley-Tukey form); searching with engines 1 and 3 on noise-only input must locate identically (near ties included) -- a wrong
    index map would scramble the correlation."""
    from gnss_dsp_tools_amd import signals, synth
    sig = signals.get("gps-l5i")
    x = synth.make_iq(sig, 1, 2024, [])
    items = [1, 2, 3, 30, 31, 32]
    ds = [-1000.0, 1000.0, 200.0]
    res = {}
    for eng in (1, 3):
        engine.set_engine(eng)
        res[eng] = engine.search_all(sig, x, items, ds, 1)
        engine.set_engine(0)
    for a, b in zip(res[1], res[3]):
        assert a[1] == b[1] and a[2] == b[2]
        assert float(a[0]) == pytest.approx(float(b[0]), rel=5e-6)


def test_default_engines_create_no_rocfft_plan_code_spectra_included():
    """What every run of an acquire-*.py replacement pays once per process: building the signal (code spectra) and the first
    search.  A rocFFT plan for a new length costs 0.5-2 s (runtime-compiled kernels); the default engines -- LDS-resident 4096 /
    16384, split 65536 / 81920, prime-factor 61380 -- take their code spectra from their own forward transforms and the
    tie-safe complex128 spectra from the library's own Stockham transform, so a fresh context gets through signal build and
    search without one.  The rocFFT pipeline (engine 1) and gacq_signal_spectrum make theirs on first use, and agree with the
    default engine's records."""
    from gnss_dsp_tools_amd import acquire, signals, synth
    for name, items, ds, ms in (("gps-l1", [1, 5, 9], [-1000.0, 1000.0, 500.0], 2), ("beidou-b1i", [1, 2], [-500.0, 500.0, 500.0], 2),
                                ("galileo-e1b", [1, 2], [-250.0, 250.0, 250.0], 8), ("gps-l5i", [1, 2], [-200.0, 200.0, 200.0], 1),
                                ("gps-l1cd", [1], [-100.0, 100.0, 100.0], 10)):
        sig = signals.get(name)
        x = synth.make_iq(sig, ms, 99, synth.default_sats(items))
        eng = acquire.Engine(0)
        try:
            assert eng.tie_stats()["ambiguous_pairs"] == 0 and eng.fft_plans() == 0
            got = eng.search_all(sig, x, items, ds, ms)                      # tie-safe locations on (default): complex128 spectra built too
            assert eng.fft_plans() == 0, (name, eng.fft_plans())
            spec = eng._plan(sig, items)[0].spectrum(items[0])               # natural-order spectrum: rocFFT, on first use
            assert eng.fft_plans() >= 1 and np.isfinite(spec).all() and abs(spec).max() > 0
            eng.set_engine(1)
            ref = eng.search_all(sig, x, items, ds, ms)
            for a, b in zip(got, ref):
                assert a[1] == b[1] and a[2] == b[2] and float(a[0]) == pytest.approx(float(b[0]), rel=5e-6), (name, a, b)
        finally:
            eng.close()


SPLIT_LDS_CASES = ["cfg3_e1b_subset", "cfg3_e1c_subset", "e1b_ms12", "cfg5_b1i_ms10", "b2i_ms2", "cfg5_glonass_l1", "glonass_l2",
                   "gps_l1cd", "bds_b1cp", "gps_l2cm", "bds_b1cd", "gps_l1cp"]


LDS16K_CASES = ["cfg5_b1i_ms10", "b2i_ms2", "cfg5_glonass_l1", "glonass_l2"]


@pytest.mark.parametrize("variant", [16, -1], ids=["radix16", "radix32"])
@pytest.mark.parametrize("cid", LDS16K_CASES)
def test_single_workgroup_16384_engine_matches_reference_golden(engine, golden_cases, cid, variant):
    """N = 16384 through engine 2: the whole transform in one workgroup -- 512 threads x 32 points (32 x 32 x 16, gacq_lds16k.hip, the
    default) or 1024 threads x 16 points (16 x 16 x 16 x 4, option lds_variant = 16)."""
    case = golden_cases[cid]
    x = case_iq(case)
    engine.set_engine(2)
    engine.set_option("lds_variant", variant)
    try:
        got = engine.search_all(case["script"], x, case["items"], case["doppler_search"], case["ms"])
    finally:
        engine.set_option("lds_variant", -1)
        engine.set_engine(0)
    _assert_results(got, case["results"], case)


def test_radix32_16384_rows_match_the_radix16_rows(engine):
    """Both forms of the N = 16384 transform compute the same magnitude row (different butterfly order: equal to fp32 rounding, the peak
    on the same lag), for a raw-metric padded signal and a biased-carrier one."""
    from gnss_dsp_tools_amd import signals, synth
    for name, item in (("beidou-b1i", 12), ("glonass-l1", -3)):
        sig = signals.get(name)
        B = 3
        x = synth.make_iq(sig, B, 5, synth.default_sats([item]))
        rows = {}
        for variant in (16, -1):
            engine.set_engine(2)
            engine.set_option("lds_variant", variant)
            try:
                rows[variant] = engine.debug_row(sig, x, item, 1250.0, B)
            finally:
                engine.set_option("lds_variant", -1)
                engine.set_engine(0)
        a, b = rows[16], rows[-1]
        assert int(np.argmax(a)) == int(np.argmax(b))
        assert np.abs(a - b).max() <= 2e-6 * np.abs(a).max(), (name, np.abs(a - b).max(), np.abs(a).max())


@pytest.mark.parametrize("B", [1, 2])
def test_radix16_16384_two_kernel_search_matches_the_radix32_search(engine, B):
    """r16_forward + r16_correlate (gacq_lds16k_r16.hip, code spectra from r16_code_spectra) at their smallest shape -- BeiDou B1I, one
    epoch, two items, three Doppler bins, one block and two -- against the radix-32 form of the same engine: same lag and Doppler bin,
    metric within the project's 1e-5.  Both satellites are strong (0.5 against unit noise, ~30 sigma after one block), so the location
    does not hang on rounding."""
    from gnss_dsp_tools_amd import signals, synth
    sig = signals.get("beidou-b1i")
    items = [12, 30]
    x = synth.make_iq(sig, B, 7, [(12, 0.5, 1537.0, 1201), (30, 0.5, 1000.0, 77)])
    dop = np.array([1000.0, 1500.0, 2000.0])
    got = {}
    for variant in (16, -1):
        engine.set_engine(2)
        engine.set_option("lds_variant", variant)
        try:
            got[variant] = engine.search_blocks(sig, x, items, dop, B)
        finally:
            engine.set_option("lds_variant", -1)
            engine.set_engine(0)
    for item, want_dop, a, b in zip(items, (1500.0, 1000.0), got[16], got[-1]):
        assert float(a[1]) == float(b[1]) and float(a[2]) == float(b[2]) == want_dop, (item, a, b)
        assert float(a[0]) == pytest.approx(float(b[0]), rel=METRIC_RTOL), (item, a, b)


@pytest.mark.parametrize("cid", SPLIT_LDS_CASES)
@pytest.mark.parametrize("eng", [1, 3, 4])
def test_split_engines_match_reference_golden_pow2(engine, golden_cases, cid, eng):
    """N = 65536 / 16384 / 81920 / 163840 (outer radix 16 / 4 / 20 / 40): rocFFT pipeline (1), split with rocFFT inner
    transforms (3), split with fused LDS inner transforms (4)."""
    case = golden_cases[cid]
    x = case_iq(case)
    engine.set_engine(eng)
    try:
        got = engine.search_all(case["script"], x, case["items"], case["doppler_search"], case["ms"])
    finally:
        engine.set_engine(0)
    _assert_results(got, case["results"], case)


def test_split_lds_rows_match_reference_rows(engine, golden_cases, golden_rows):
    """Row-level check of engine 4 against the reference's q rows (B1I N=16384 B=10, GLONASS N=16384 with channel bias)."""
    from gnss_dsp_tools_amd import signals
    for key, want in golden_rows.items():
        cid, item, dop = key.split("|")
        case = golden_cases[cid]
        sig = signals.get(case["script"])
        if sig.nfft != 16384:
            continue
        engine.set_engine(4)
        try:
            q = engine.debug_row(sig, case_iq(case), int(item), float(dop), sig.blocks(case["ms"]))
        finally:
            engine.set_engine(0)
        assert int(np.argmax(q)) == int(np.argmax(want)), key
        assert np.max(np.abs(q.astype(np.float64) - want)) / np.max(want) < 5e-6, key


@pytest.mark.parametrize("name,items,ds,ms", [
    ("gps-l1", [3, 4, 11, 28], [-1500.0, 2000.0, 250.0], 3),            # LDS engine: epochs/items chunking irrelevant, rows buffer only
    ("beidou-b1i", [6, 7, 33], [1000.0, 2000.0, 250.0], 4),              # split + LDS inner, B = 4
    ("gps-l5i", [7, 8], [1200.0, 2000.0, 200.0], 2),                     # split radix 31 + rocFFT inner
    ("galileo-e1b", [5, 24], [1000.0, 1750.0, 250.0], 8),                # split radix 16
])
def test_tiny_workspace_forces_chunking_same_results(name, items, ds, ms):
    """Workspace limit of 1 MiB (< one correlation row for the big lengths): the group / epoch chunk loops must give the
    same answers as one pass."""
    from gnss_dsp_tools_amd import acquire, signals, synth
    sig = signals.get(name)
    x = synth.make_iq(sig, sig.blocks(ms), 606, [(items[0], 0.4, 1537.0, 1201)])
    big = acquire.Engine(0)
    small = acquire.Engine(0, workspace_bytes=1 << 20)
    try:
        want = big.search_all(sig, x, items, ds, ms)
        for eng in (0, 1):
            small.set_engine(eng)
            got = small.search_all(sig, x, items, ds, ms)
            for g, w in zip(got, want):
                assert g[1] == w[1] and g[2] == w[2]
                assert float(g[0]) == pytest.approx(float(w[0]), rel=5e-6)
    finally:
        big.close()
        small.close()


def test_maximum_default_integration_time_gps_l1(engine):
    """The CLI default --time 80 (80 non-coherent blocks, acquire-gps-l1.py:67) on the default Doppler grid, vs the oracle."""
    from gnss_dsp_tools_amd import signals, synth
    from oracle import acq_oracle
    sig = signals.get("gps-l1")
    items = [3, 11, 19, 30]
    ds = [-7000.0, 7000.0, 200.0]
    x = synth.make_iq(sig, 80, 8080, [(11, 0.05, 1537.0, 1201), (19, 0.03, -3262.0, 77)])
    got = engine.search_all(sig, x, items, ds, 80)
    want = [acq_oracle.search_script("gps-l1", x.astype(np.complex128), it, ds, 80) for it in items]
    _assert_results(got, [[float(v) for v in w] for w in want], {"id": "gps-l1 ms=80", "items": items})


def test_multi_constellation_jobs_single_rank(engine):
    """search_jobs (config-5 style: several signals in one sharded pass) on one rank == per-signal search_all."""
    import torch
    from gnss_dsp_tools_amd import acquire, sharded, signals, synth
    specs = [("gps-l1", [3, 11, 28], [-2000.0, 2000.0, 250.0], 2), ("beidou-b1i", [6, 33], [1000.0, 2000.0, 250.0], 2),
             ("glonass-l1", [-7, 3], [1000.0, 2000.0, 250.0], 1)]
    jobs, want = [], []
    for name, items, ds, ms in specs:
        sig = signals.get(name)
        B = sig.blocks(ms)
        x = synth.make_iq(sig, B, 9090, [(items[0], 0.4, 1537.0, 1201)])
        dop = acquire.doppler_grid(ds)
        jobs.append({"name": sig, "x": torch.from_numpy(x[None, :sig.samples_needed(B)].copy()).cuda(), "items": items, "dopplers": dop, "blocks": B})
        want.append(engine.search_all(sig, x, items, ds, ms))
    sh = sharded.ShardedSearch(engine=engine)
    merged = sh.search_jobs(jobs)
    torch.cuda.synchronize()
    for (name, items, ds, ms), m, w in zip(specs, merged, want):
        got = sh.results(name, items, m, acquire.doppler_grid(ds))[0]
        assert got == w, name
    engine.set_stream(None)


@pytest.mark.gpu
@pytest.mark.parametrize("nlanes", [2, 3])
def test_multi_constellation_jobs_on_job_lanes_equal_the_serial_records(engine, nlanes):
    """ShardedSearch.enable_job_lanes: the searches of one job list queued on several contexts, each on a stream with a hardware queue of
    its own -- the records must be the serial ones bit for bit, in the caller's job order, step after step (buffers reused)."""
    import torch
    from gnss_dsp_tools_amd import acquire, sharded, signals, synth
    specs = [("gps-l1", [3, 11, 28], [-2000.0, 2000.0, 250.0], 2), ("galileo-e1b", [5, 24], [-500.0, 500.0, 250.0], 8),
             ("beidou-b1i", [6, 33], [1000.0, 2000.0, 250.0], 2), ("glonass-l1", [-7, 3], [1000.0, 2000.0, 250.0], 1)]
    jobs = []
    for name, items, ds, ms in specs:
        sig = signals.get(name)
        B = sig.blocks(ms)
        x = synth.make_iq(sig, B, 9191, [(items[0], 0.4, 1537.0, 1201)])
        jobs.append({"name": sig, "x": torch.from_numpy(x[None, :sig.samples_needed(B)].copy()).cuda(), "items": items,
                     "dopplers": acquire.doppler_grid(ds), "blocks": B})
    sh = sharded.ShardedSearch(engine=engine)
    want = [t.cpu().numpy().copy() for t in sh.search_jobs(jobs)]
    sh.enable_job_lanes(nlanes)
    try:
        for _ in range(3):
            got = sh.search_jobs(jobs)
            torch.cuda.synchronize()
            for (name, _, _, _), g_, w in zip(specs, got, want):
                assert np.array_equal(g_.cpu().numpy(), w), name
    finally:
        sh.close_job_lanes()
        engine.set_stream(None)


@pytest.mark.gpu
def test_masked_stream_selects_the_cus_it_names_and_a_full_mask_the_whole_device(engine):
    """gacq_stream_create_cu_mask / gacq_cu_census: the low m bits of the mask are m / 8 CUs of every XCD; the full mask (a stream that
    only wants a hardware queue of its own) reaches every CU."""
    import torch
    from gnss_dsp_tools_amd import acquire
    total = torch.cuda.get_device_properties(0).multi_processor_count
    try:
        assert len(engine.cu_census(8192)) == total
        for cus in (32, total):
            ms = acquire.MaskedStream(0, None if cus == total else cus)
            engine.set_stream(ms.handle)
            places = engine.cu_census(8192)
            engine.set_stream(None)
            ms.close()
            per_xcc = {}
            for p_ in places:
                per_xcc[p_[0]] = per_xcc.get(p_[0], 0) + 1
            assert len(places) == cus and set(per_xcc.values()) == {cus // 8} and len(per_xcc) == 8, (cus, per_xcc)
    finally:
        engine.set_stream(None)


def test_caller_supplied_chips_equal_builtin_generators():
    """gacq_signal_create_chips: same spectra / results as the built-in generators; a wrong chip flips the result."""
    from gnss_dsp_tools_amd import acquire, codes, signals, synth
    sig = signals.get("galileo-e1b")               # BOC + padded: the chips path must apply both itself
    prns = [5, 24]
    x = synth.make_iq(sig, 1, 4321, [(5, 0.4, 1537.0, 1201)])
    ds = [1000.0, 2000.0, 125.0]
    a = acquire.Engine(0)
    b = acquire.Engine(0)
    try:
        want = a.search_all(sig, x, prns, ds, 8)
        rows = np.stack([codes.chips(sig.code, p) for p in prns])
        b.signal(sig, prns, chips=rows)
        assert b.search_all(sig, x, prns, ds, 8) == want
        np.testing.assert_array_equal(a.signal(sig, prns).spectrum(5), b.signal(sig, prns).spectrum(5))
        bad = rows.copy()
        bad[0] ^= 1                                 # inverted code: same magnitude spectrum -> same peak location, opposite sign is invisible
        b.signal(sig, prns, chips=bad)
        assert b.search_all(sig, x, prns, ds, 8)[0][1] == want[0][1]
        bad[0, ::2] ^= 1                            # scrambled code: the satellite is no longer found at its delay
        b.signal(sig, prns, chips=bad)
        assert b.search_all(sig, x, prns, ds, 8)[0][1] != want[0][1]
        with pytest.raises(ValueError):
            b.signal(sig, prns, chips=rows[:, :100])
    finally:
        a.close()
        b.close()


def test_epoch_chunking_with_small_workspace():
    """Several epochs with a workspace smaller than one epoch's forward spectra: the epoch loop must chunk correctly."""
    import torch
    from gnss_dsp_tools_amd import acquire, signals, synth
    sig = signals.get("gps-l1")
    items = list(range(1, 9))
    dop = acquire.doppler_grid([-2500.0, 2500.0, 250.0])
    xs = synth.make_epochs(sig, 2, 1717, synth.default_sats(items), 5, nsamp=2 * 4096)
    xd = torch.from_numpy(xs).cuda()
    big = acquire.Engine(0)
    small = acquire.Engine(0, workspace_bytes=1 << 20)
    try:
        for eng_id in (0, 1):
            big.set_engine(eng_id)
            small.set_engine(eng_id)
            a = big.search_batch_dev(sig, xd, items, dop, 2)
            b = small.search_batch_dev(sig, xd, items, dop, 2)
            torch.cuda.synchronize()
            pa = a.cpu().numpy().view(acquire.PEAK_DTYPE)
            pb = b.cpu().numpy().view(acquire.PEAK_DTYPE)
            np.testing.assert_array_equal(pa["idx"], pb["idx"])
            np.testing.assert_array_equal(pa["d_index"], pb["d_index"])
            np.testing.assert_allclose(pa["metric"], pb["metric"], rtol=1e-6)
    finally:
        big.close()
        small.close()


@pytest.mark.parametrize("name,items,B", [("gps-l5i", [7, 8, 9], 1), ("galileo-e6b", [2, 3, 4], 2)])
@pytest.mark.parametrize("dt", [1, 2, 3])
def test_inner_kernel_doppler_tiles_with_group_chunks_not_aligned_to_the_tile(engine, name, items, B, dt):
    """GACQ_OPT_SPLIT_DT: a workgroup of the prime-factor engine's inner kernel serves dt consecutive Doppler bins.  13 bins (not a multiple of 2
    or 3) and a workspace that holds the forward spectra plus a handful of correlation rows, so that the (epoch, item, Doppler)
    group chunks start and end inside a tile: byte-identical records to the roomy single pass with one bin per workgroup."""
    import torch
    from gnss_dsp_tools_amd import acquire, signals, synth
    sig = signals.get(name)
    dop = acquire.doppler_grid([-1200.0, 1400.0, 200.0])
    assert len(dop) == 13
    xs = synth.make_epochs(sig, B, 5151, [(items[0], 0.4, 537.0, 1201), (items[2], 0.3, -871.0, 333)], 2)
    xd = torch.from_numpy(xs).cuda()
    x_bytes = 8 * len(dop) * B * sig.nfft * 2                                 # both epochs' forward spectra
    small = acquire.Engine(0, workspace_bytes=x_bytes + 5 * 8 * B * sig.nfft + (1 << 16))
    try:
        engine.set_option("split_dt", 1)
        want = engine.search_batch_dev(sig, xd, items, dop, B)
        torch.cuda.synchronize()
        for e in (engine, small):
            e.set_option("split_dt", dt)
            got = e.search_batch_dev(sig, xd, items, dop, B)
            torch.cuda.synchronize()
            assert got.cpu().numpy().tobytes() == want.cpu().numpy().tobytes(), (name, dt, e is small)
    finally:
        engine.set_option("split_dt", 0)
        small.close()


@pytest.mark.parametrize("name,ms", [("galileo-e1b", 4), ("gps-l2cm", 20), ("beidou-b1i", 0), ("gps-l1", 0)])
def test_zero_blocks_never_reads_x(engine, name, ms):
    """ms -> B == 0 (galileo-e1b ms < 8, gps-l2cm ms < 40): the reference's block loop is empty, it returns its untouched
    (0, 0, 0) and never looks at x.  Padded signals used to stage (0 + pad) * n samples from the caller's buffer anyway
    (ADVICE r1): here x is ONE sample long, both through the Python mirror and straight through the C ABI."""
    import ctypes
    from gnss_dsp_tools_amd import _native as nat
    from gnss_dsp_tools_amd import acquire, signals
    sig = signals.get(name)
    assert sig.blocks(ms) <= 0
    x = np.ones(1, dtype=np.complex64)
    ds = [-500.0, 500.0, 250.0]
    assert acquire.make_search(name, engine)(x, 1, ds, ms) == (0, 0, 0)
    assert engine.search_all(sig, x, [1, 2], ds, ms) == [(0, 0, 0), (0, 0, 0)]
    s = engine.signal(sig, [1, 2])
    items = np.array([0, 1], dtype=np.int32)
    dop = acquire.doppler_grid(ds)
    res = (nat.Result * 2)()
    rc = nat.lib.gacq_search(s._h, x.ctypes.data_as(nat.c_float_p), 1, items.ctypes.data_as(nat.c_int_p), 2,
                             dop.ctypes.data_as(nat.c_double_p), len(dop), None, 0, res)
    assert rc == 0 and [(r.metric, r.idx, r.d_index) for r in res] == [(0.0, -1, -1)] * 2


@pytest.mark.parametrize("name,ms", [("gps-l1", 1), ("beidou-b1i", 10), ("galileo-e1b", 8)])
def test_empty_doppler_grid_never_reads_x(engine, name, ms):
    """An empty Doppler grid with blocks > 0 (np.arange(1000, 1000, 100)): the reference's loop body never runs, it returns its
    untouched (0, 0, 0) and never looks at x -- so x may be ONE sample long: Python mirror, batched host call, and the
    three C entry points straight through ctypes."""
    import ctypes
    from gnss_dsp_tools_amd import _native as nat
    from gnss_dsp_tools_amd import acquire, signals
    sig = signals.get(name)
    B = sig.blocks(ms)
    assert B > 0
    x = np.ones(1, dtype=np.complex64)
    ds = [1000.0, 1000.0, 100.0]
    assert len(acquire.doppler_grid(ds)) == 0
    assert acquire.make_search(name, engine)(x, 1, ds, ms) == (0, 0, 0)
    assert engine.search_all(sig, x, [1, 2], ds, ms) == [(0, 0, 0), (0, 0, 0)]
    assert engine.search_batch_host(sig, x[None, :], [1, 2], acquire.doppler_grid(ds), B) == [[(0, 0, 0), (0, 0, 0)]]
    s = engine.signal(sig, [1, 2])
    items = np.array([0, 1], dtype=np.int32)
    res = (nat.Result * 2)()
    rc = nat.lib.gacq_search(s._h, x.ctypes.data_as(nat.c_float_p), 1, items.ctypes.data_as(nat.c_int_p), 2, None, 0, None, B, res)
    assert rc == 0 and [(r.metric, r.idx, r.d_index) for r in res] == [(0.0, -1, -1)] * 2
    rc = nat.lib.gacq_search_batch(s._h, x.ctypes.data_as(nat.c_float_p), 1, 1, items.ctypes.data_as(nat.c_int_p), 2, None, 0, None, B, res)
    assert rc == 0 and [(r.metric, r.idx, r.d_index) for r in res] == [(0.0, -1, -1)] * 2


def test_empty_item_list_and_out_buffer_validation(engine):
    """search_all over no items is [] like the reference's map over an empty list; a caller-supplied result buffer of the
    wrong shape / dtype / layout is refused instead of being overwritten by the last kernel."""
    import torch
    from gnss_dsp_tools_amd import acquire, signals, synth
    sig = signals.get("gps-l1")
    x = synth.make_iq(sig, 1, 5, [(3, 0.5, 1000.0, 100)], nsamp=4096)
    assert engine.search_all(sig, x, [], [-500.0, 500.0, 250.0], 1) == []
    xd = torch.from_numpy(x[None]).cuda()
    dop = acquire.doppler_grid([-500.0, 1500.0, 250.0])
    assert tuple(engine.search_batch_dev(sig, xd, [], dop, 1).shape) == (1, 0, 2)
    for bad in (torch.empty((1, 3, 2), dtype=torch.float32, device="cuda"), torch.empty((1, 2, 2), dtype=torch.float64, device="cuda"),
                torch.empty((1, 3, 4), dtype=torch.float64, device="cuda")[:, :, ::2], torch.empty((1, 3, 2), dtype=torch.float64)):
        with pytest.raises(ValueError):
            engine.search_batch_dev(sig, xd, [1, 2, 3], dop, 1, out=bad)
    good = torch.empty((1, 3, 2), dtype=torch.float64, device="cuda")
    assert engine.search_batch_dev(sig, xd, [1, 2, 3], dop, 1, out=good) is good
    torch.cuda.synchronize()
    assert engine.finalize(sig, [1, 2, 3], good.cpu().numpy().view(acquire.PEAK_DTYPE).reshape(3), dop) == engine.search_blocks(sig, x, [1, 2, 3], dop, 1)


def test_signal_handle_outliving_its_engine_is_harmless():
    """Engine.close() destroys every signal created on it (also user-held ones) before the context, so a later close() /
    garbage collection of the AcqSignal cannot touch a freed context."""
    from gnss_dsp_tools_amd import acquire, signals
    eng = acquire.Engine(0)
    held = acquire.AcqSignal(eng, signals.get("gps-l1"), [1, 2, 3])        # not through the engine's cache
    cached = eng.signal("gps-l1", [4, 5])
    eng.close()
    assert held._h is None and cached._h is None
    held.close()
    del held, cached


def test_search_on_a_nearly_full_device_runs_in_smaller_passes():
    """The work buffers follow the device's FREE memory, not just the 32 GiB default limit (plumbing 11 / ADVICE): a context
    created on a device that something else has filled sizes its passes to its share of what is left; one that had sized them while the
    memory was free, and finds it gone, re-runs the search in passes of half the size instead of failing.  E1B, 36 items x 64 bins: 1.2 GB of
    correlation workspace in one pass on an empty device.  Records identical either way (the pass size changes no arithmetic)."""
    import torch
    from gnss_dsp_tools_amd import acquire, signals, synth
    sig = signals.get("galileo-e1b")
    items = list(range(1, 37))
    ds = [-4000.0, 4000.0, 125.0]
    x = synth.make_iq(sig, 1, 11, synth.default_sats(items))
    ref = acquire.Engine(0)
    try:
        want = ref.search_all(sig, x, items, ds, 8)
    finally:
        ref.close()
    torch.cuda.empty_cache()
    late = acquire.Engine(0)                         # sizes its budget NOW, with the device empty (32 GiB binds) ...
    hog = None
    try:
        assert late.search_all(sig, x[:sig.samples_needed(1)], items[:2], [0.0, 500.0, 250.0], 8)
        free, _ = torch.cuda.mem_get_info(0)
        leave = int(2.5 * 2 ** 30)
        hog = torch.empty(free - leave, dtype=torch.uint8, device="cuda:0")
        early = acquire.Engine(0)                    # ... this one with 2.5 GB left: 0.8 x 2.5 GB / 2.25 / (contexts on the device) per buffer
        try:
            assert early.search_all(sig, x, items, ds, 8) == want
        finally:
            early.close()
        del hog
        hog = None
        torch.cuda.empty_cache()
        free, _ = torch.cuda.mem_get_info(0)
        hog = torch.empty(free - 2 ** 30, dtype=torch.uint8, device="cuda:0")      # 1 GB left: the 1.2 GB pass `late` plans cannot be had
        assert late.search_all(sig, x, items, ds, 8) == want
    finally:
        if hog is not None:
            del hog
        torch.cuda.empty_cache()
        late.close()


def test_doppler_slicing_when_one_epoch_exceeds_the_workspace(engine):
    """One epoch's forward spectra [D][B][N] larger than the workspace limit (galileo-e1b --time 200 would be 9 GB): the grid is
    searched in slices and merged with strict '>' in grid order -- same records as the single pass, on every engine that
    buffers X.  1 MiB limit: gps-l1 B=3 -> 10 bins per slice; beidou-b1i B=2 -> 4; galileo-e1b -> 2."""
    import torch
    from gnss_dsp_tools_amd import acquire, signals, synth
    small = acquire.Engine(0, workspace_bytes=1 << 20)
    try:
        for name, items, ds, ms, engines in [("gps-l1", [3, 4, 11, 28], [-5000.0, 5000.0, 250.0], 3, (0, 1)),
                                             ("beidou-b1i", [6, 7, 33], [-2000.0, 2000.0, 250.0], 2, (0, 1, 4)),
                                             ("galileo-e1b", [5, 24], [-1000.0, 1000.0, 125.0], 8, (0,)),
                                             ("gps-l5i", [7, 8], [-1000.0, 1000.0, 200.0], 1, (0,))]:
            sig = signals.get(name)
            B = sig.blocks(ms)
            xs = synth.make_epochs(sig, B, 4242, [(items[0], 0.4, 537.0, 1201)], 2)
            xd = torch.from_numpy(xs).cuda()
            dop = acquire.doppler_grid(ds)
            assert 8 * len(dop) * B * sig.nfft > (1 << 20)
            for e in engines:
                engine.set_engine(e)
                small.set_engine(e)
                a = engine.search_batch_dev(sig, xd, items, dop, B)
                b = small.search_batch_dev(sig, xd, items, dop, B)
                torch.cuda.synchronize()
                assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes(), (name, e)
    finally:
        engine.set_engine(0)
        small.close()


NCO_KERNELS = {            # (fs, N) -> (script, forward kernels that serve this length: 1 mix_nco, 2 LDS, 3 split outer, 4 fused 16K, 5 prime-factor outer)
    (4096000.0, 4096): ("gps-l1", (1, 2)),
    (8192000.0, 65536): ("galileo-e1b", (1, 3)),
    (30690000.0, 61380): ("gps-l5i", (1, 3, 5)),
    (16384000.0, 16384): ("glonass-l1", (1, 2, 3, 4)),
    (8192000.0, 16384): ("beidou-b1i", (1, 2, 3, 4)),
}


def test_device_nco_indices_are_bit_exact(engine, golden_nco):
    """index work is bit-exact.  Every forward kernel evaluates floor((f*i)*1024) mod 1024 itself (fp64 on the
    device); one wrong index in 4096 moves the metric by ~1e-6, inside the 1e-5 tolerance of the search tests, so each kernel
    dumps its index vector and the SHA-256 must equal the reference's (tests/golden/nco_indices.json, produced by
    gnsstools/nco.py:6-10 incl. the GLONASS-biased carriers of acquire-glonass-l1.py:28)."""
    import hashlib
    from gnss_dsp_tools_amd import _native as nat
    from gnss_dsp_tools_amd import signals
    checked = 0
    for v in golden_nco["vectors"]:
        script, kernels = NCO_KERNELS[(v["fs"], v["n"])]
        sig = signals.get(script)
        s = engine.signal(sig, [0] if sig.bias_hz else [1])
        for k in kernels:
            # the LDS forward (2) and fused (4) kernels of N = 16384 exist in two forms: radix-32 (default) and radix-16 (lds_variant = 16)
            for variant in ((-1, 16) if v["n"] == 16384 and k in (2, 4) else (-1,)):
                engine.set_option("lds_variant", variant)
                try:
                    idx = s.nco_indices(k, v["doppler"], v.get("bias", 0.0))
                finally:
                    engine.set_option("lds_variant", -1)
                assert idx.dtype == np.int32 and len(idx) == v["n"]
                assert [int(i) for i in idx[:16]] == v["head"] and [int(i) for i in idx[-16:]] == v["tail"], (script, k, v["doppler"], variant)
                assert hashlib.sha256(idx.tobytes()).hexdigest() == v["sha256"], (script, k, v["doppler"], variant)
                checked += 1
    assert checked == 6 * 2 + 3 * 2 + 3 * 3 + 2 * 4 + 2 * 4 + 2 * 4 + 3 * 2 * 2
    with pytest.raises(nat.GacqError) as ei:             # no LDS forward kernel for N = 65536
        engine.signal("galileo-e1b", [1]).nco_indices(2, 125.0)
    assert ei.value.code == -9


def _shifted_epochs(sig, B, seed, sats, nepoch, nsamp):
    """nepoch distinct epochs from 8 seeded ones: every epoch a different circular shift, so every epoch has its own answer."""
    from gnss_dsp_tools_amd import synth
    base = synth.make_epochs(sig, B, seed, sats, 8, nsamp=nsamp)
    return np.stack([np.roll(base[e % 8], 7 * e + 3) for e in range(nepoch)])


def test_host_batched_entry_point_equals_single_calls(engine):
    """gacq_search_batch (host buffers in, host results out, pinned staging ring in C, no torch): identical to one gacq_search per
    epoch, across more chunks than the ring has slots (GPS L1: 64 epochs per chunk, 3 slots -> 1000 epochs wrap the ring five
    times) and for a signal whose chunks are bounded by bytes (E1B: 42 epochs per 32 MiB chunk)."""
    from gnss_dsp_tools_amd import acquire, signals
    for name, items, ds, ms, E in [("gps-l1", [3, 11, 19, 28], [-2000.0, 2000.0, 250.0], 1, 1000),
                                   ("galileo-e1b", [5, 24], [1000.0, 2000.0, 250.0], 8, 90),
                                   ("glonass-l1", [-7, 0, 3], [1000.0, 2000.0, 250.0], 1, 10)]:
        sig = signals.get(name)
        B = sig.blocks(ms)
        xs = _shifted_epochs(sig, B, 321, [(items[0], 0.4, 1537.0, 1201)], E, sig.samples_needed(B))
        dop = acquire.doppler_grid(ds)
        got = engine.search_batch_host(sig, xs, items, dop, B)
        assert len(got) == E
        for e in list(range(0, E, max(1, E // 40))) + [E - 1]:
            assert got[e] == engine.search_blocks(sig, xs[e], items, dop, B), (name, e)
        assert len({tuple(map(tuple, g)) for g in got}) > E // 2           # the epochs really differ
    assert engine.search_batch_host("gps-l1", np.zeros((3, 1), dtype=np.complex64), [1, 2], acquire.doppler_grid([0.0, 500.0, 250.0]), 0) == [[(0, 0, 0)] * 2] * 3
    with pytest.raises(ValueError):
        engine.search_batch_host("gps-l1", np.zeros((3, 100), dtype=np.complex64), [1], acquire.doppler_grid([0.0, 500.0, 250.0]), 1)


def test_in_library_device_group_equals_one_device(engine):
    """gacq_group_*: several contexts driven from one process (here three on the one GPU of the test box): Doppler-slice
    split, item split for a coarse grid, FDMA biases, raw and normalised metrics -- bit-identical to the one-device batch."""
    from gnss_dsp_tools_amd import acquire, signals
    grp = acquire.DeviceGroup([0, 0, 0])
    try:
        for name, items, ds, ms, E in [("gps-l1", list(range(1, 33)), [-5000.0, 5000.0, 250.0], 1, 300),      # 40 bins -> 13/13/14
                                       ("gps-l1", [3, 11, 19, 28, 30], [-500.0, 750.0, 250.0], 2, 20),        # 5 bins < 12 -> item split 1/2/2
                                       ("glonass-l1", [-7, -2, 0, 3, 6], [1000.0, 2000.0, 500.0], 2, 6),      # item split with per-item bias
                                       ("beidou-b1i", [6, 33], [-3000.0, 3000.0, 250.0], 2, 8),               # raw metric, padded
                                       ("gps-l1", [7], [-500.0, 0.0, 250.0], 1, 4)]:                          # 2 bins, 1 item: an empty shard
            sig = signals.get(name)
            B = sig.blocks(ms)
            xs = _shifted_epochs(sig, B, 654, [(items[0], 0.4, 537.0, 1201)], E, sig.samples_needed(B))
            dop = acquire.doppler_grid(ds)
            assert grp.search_batch_host(sig, xs, items, dop, B) == engine.search_batch_host(sig, xs, items, dop, B), name
        assert grp.search_batch_host("gps-l1", xs, [1], acquire.doppler_grid([0.0, 0.0, 1.0]), 1) == [[(0, 0, 0)]] * len(xs)     # empty grid
        with pytest.raises(Exception):
            acquire.DeviceGroup([0, 4096])
    finally:
        grp.close()


def test_device_group_rccl_exchange_equals_the_host_merge(engine):
    """gacq_group_set_exchange(GACQ_EXCHANGE_RCCL): the members' records stay on the devices, ONE ncclAllGather per chunk (single-
    process communicators, librccl.so loaded on demand) and the tie-safe merge on a member.  The test box has one GPU: the
    collective runs with one rank -- the RCCL call sequence, the stream ordering against the search and the merge, the device-side
    records and the pinned result slot are what is exercised; the merge itself is the one the sharded path uses.  Duplicate
    devices are refused (RCCL needs distinct ones) and leave the group on the host merge."""
    from gnss_dsp_tools_amd import _native as nat
    from gnss_dsp_tools_amd import acquire, signals
    grp = acquire.DeviceGroup([0])
    try:
        grp.set_exchange("rccl")
        for name, items, ds, ms, E in [("gps-l1", list(range(1, 33)), [-5000.0, 5000.0, 250.0], 1, 700),      # three chunks through the ring
                                       ("beidou-b1i", [6, 33], [-3000.0, 3000.0, 250.0], 2, 8),
                                       ("gps-l5i", [1, 2, 3], [-400.0, 400.0, 200.0], 1, 3)]:
            sig = signals.get(name)
            B = sig.blocks(ms)
            xs = _shifted_epochs(sig, B, 655, [(items[0], 0.4, 137.0, 1201)], E, sig.samples_needed(B))
            dop = acquire.doppler_grid(ds)
            assert grp.search_batch_host(sig, xs, items, dop, B) == engine.search_batch_host(sig, xs, items, dop, B), name
        grp.set_exchange("host")
        assert grp.search_batch_host(sig, xs, items, dop, B) == engine.search_batch_host(sig, xs, items, dop, B)
    finally:
        grp.close()
    dup = acquire.DeviceGroup([0, 0])
    try:
        with pytest.raises(nat.GacqError) as ei:
            dup.set_exchange("rccl")
        assert ei.value.code == -9 and "distinct" in str(ei.value)
        sig = signals.get("gps-l1")
        xs = _shifted_epochs(sig, 1, 656, [], 4, sig.n)
        dop = acquire.doppler_grid([-2000.0, 2000.0, 250.0])
        assert dup.search_batch_host(sig, xs, [1, 2], dop, 1) == engine.search_batch_host(sig, xs, [1, 2], dop, 1)
    finally:
        dup.close()


@pytest.mark.parametrize("cid", ALL_CASES)
def test_complex128_verification_engine_matches_reference_to_1e_10(engine, golden_cases, cid):
    """Engine 5 = the pipeline in complex128 on the device (rocFFT double, fp64 NCO table, fp64 magnitudes and metric): the same
    arithmetic type as the reference, so it must agree with the reference's own outputs to rounding (1e-10 relative; the fp32
    engines are held to 1e-5).  It is the tool for bisecting a near-tie disagreement between an fp32 engine and the oracle."""
    case = golden_cases[cid]
    x = case_iq(case)
    engine.set_engine(5)
    try:
        got = engine.search_all(case["script"], x, case["items"], case["doppler_search"], case["ms"])
    finally:
        engine.set_engine(0)
    for g, w, item in zip(got, case["results"], case["items"]):
        assert float(g[2]) == w[2] and float(g[1]) == pytest.approx(w[1], rel=1e-12, abs=1e-9), (cid, item, g, w)
        assert float(g[0]) == pytest.approx(w[0], rel=1e-10), (cid, item, g, w)


def test_fused_complex128_4096_kernel_equals_the_rocfft_double_pipeline(engine):
    """Engine 5 for N = 4096, B = 1 is one kernel per search (fused4k_c128_kernel); option fused_c128 = 0 brings back the five-stage
    rocFFT double-precision pipeline.  Same locations, metrics equal to 1e-12, for several item-chunk regimes (few epochs: small
    chunks; many epochs: 32 items per workgroup) and on noise-only epochs; the stage timers prove which one ran."""
    import torch
    from gnss_dsp_tools_amd import acquire, signals, synth
    sig = signals.get("gps-l1")
    dop = acquire.doppler_grid([-5000.0, 5000.0, 250.0])
    try:
        engine.set_engine(5)
        for E, items, sats in ((1, [7], None), (3, list(range(1, 33)), None), (40, [3, 3, 9, 31, 12], []), (96, list(range(1, 33)), [])):
            xs = synth.make_epochs(sig, 1, 5150 + E, synth.default_sats(items) if sats is None else sats, E, nsamp=4096)
            xd = torch.from_numpy(xs).cuda()
            engine.set_option("fused_c128", 0)
            want = engine.search_batch_dev(sig, xd, items, dop, 1)
            torch.cuda.synchronize()
            want = want.cpu().numpy().view(acquire.PEAK_DTYPE)
            engine.set_option("fused_c128", 1)
            engine.set_profiling(True)
            engine.reset_stage_times()
            got = engine.search_batch_dev(sig, xd, items, dop, 1)
            torch.cuda.synchronize()
            st = engine.stage_times()
            engine.set_profiling(False)
            assert st["lds_correlate"][1] == 1 and st["best_doppler"][1] == 1, st
            got = got.cpu().numpy().view(acquire.PEAK_DTYPE)
            np.testing.assert_array_equal(got["idx"], want["idx"])
            np.testing.assert_array_equal(got["d_index"], want["d_index"])
            np.testing.assert_allclose(got["metric"], want["metric"], rtol=1e-12)
    finally:
        engine.set_profiling(False)
        engine.set_option("fused_c128", 1)
        engine.set_engine(0)


def test_fp32_engines_agree_with_the_complex128_engine_on_near_ties(engine):
    """Noise-only searches (every row a near-tie between thousands of lags): every fp32 engine picks the lag and Doppler bin
    the complex128 engine picks, batched, at three FFT lengths."""
    import torch
    from gnss_dsp_tools_amd import acquire, signals, synth
    for name, items, ds, B, engines in [("gps-l1", list(range(1, 33)), [-5000.0, 5000.0, 250.0], 1, (1, 2)),
                                         ("beidou-b1i", [1, 2, 3, 4], [-1000.0, 1000.0, 250.0], 2, (1, 2, 4)),
                                         ("gps-l5i", [1, 2], [-600.0, 600.0, 200.0], 1, (1, 3))]:
        sig = signals.get(name)
        xs = synth.make_epochs(sig, B, 8642, [], 3, nsamp=sig.samples_needed(B))
        xd = torch.from_numpy(xs).cuda()
        dop = acquire.doppler_grid(ds)
        engine.set_engine(5)
        ref = engine.search_batch_dev(sig, xd, items, dop, B)
        torch.cuda.synchronize()
        ref = ref.cpu().numpy().view(acquire.PEAK_DTYPE)
        for e in engines:
            engine.set_engine(e)
            got = engine.search_batch_dev(sig, xd, items, dop, B)
            torch.cuda.synchronize()
            got = got.cpu().numpy().view(acquire.PEAK_DTYPE)
            np.testing.assert_array_equal(got["idx"], ref["idx"], err_msg="%s engine %d" % (name, e))
            np.testing.assert_array_equal(got["d_index"], ref["d_index"])
            np.testing.assert_allclose(got["metric"], ref["metric"], rtol=METRIC_RTOL)
        engine.set_engine(0)


@pytest.mark.parametrize("name,items,ds,ms,E", [("galileo-e1b", [1, 2, 19, 36], [-500.0, 500.0, 125.0], 8, 2),           # N = 65536, B = 1
                                                ("beidou-b1i", [6, 7, 33], [1000.0, 2000.0, 250.0], 3, 2),               # N = 16384, B = 3, padded
                                                ("glonass-l1", [-7, 0, 3, 6], [1000.0, 2000.0, 500.0], 2, 1),            # a carrier per item
                                                ("gps-l5i", [3, 17, 32], [-400.0, 400.0, 200.0], 2, 2),                 # N = 61380 = 31 x 1980, B = 2
                                                ("galileo-e6b", [1, 50], [0.0, 600.0, 200.0], 3, 1),                    # N = 30690 = 31 x 990
                                                ("gps-l1", [3, 11, 28], [-750.0, 750.0, 250.0], 3, 2)])                 # N = 4096, B = 3: the two-kernel form
def test_complex128_split_form_equals_the_rocfft_double_pipeline(engine, name, items, ds, ms, E):
    """Engine 5 beyond N = 4096 on hand-written kernels (round 6) against the five-stage pipeline on rocFFT's double-precision transforms it
    replaces (option fused_c128 = 0): N = 4096 with several blocks as forward + correlate kernels on the LDS-resident complex128 transform;
    N = 4 x 4096 / 16 x 4096 as the split form -- forward spectra shared by the items, one Z' round trip on
    the LDS-resident complex128 transform, no rocFFT plan --; N = 31 x M with fp64 DFT-31 stages around rocFFT's native length-M transforms (no
    Bluestein).  The same locations and metrics to 1e-12 (both are fp64 throughout; only the butterfly order differs) and the magnitude row of
    one search to float32 resolution."""
    import torch
    from gnss_dsp_tools_amd import acquire, signals, synth
    sig = signals.get(name)
    B = sig.blocks(ms)
    dop = acquire.doppler_grid(ds)
    xs = synth.make_epochs(sig, B, 2468, synth.default_sats(items), E, nsamp=sig.samples_needed(B))
    xd = torch.from_numpy(xs).cuda()
    eng = acquire.Engine(0, engine=5)
    try:
        got = eng.search_batch_dev(sig, xd, items, dop, B)
        torch.cuda.synchronize()
        got = got.cpu().numpy().view(acquire.PEAK_DTYPE)
        assert eng.fft_plans() == (0 if sig.nfft in (4096, 16384, 65536) else 2)    # 31 x M: the length-M forward and inverse plans
        row = eng.debug_row(sig, xs[0], items[1], float(dop[1]), B)
        eng.set_option("fused_c128", 0)
        ref = eng.search_batch_dev(sig, xd, items, dop, B)
        torch.cuda.synchronize()
        ref = ref.cpu().numpy().view(acquire.PEAK_DTYPE)
        row_ref = eng.debug_row(sig, xs[0], items[1], float(dop[1]), B)
    finally:
        eng.close()
    np.testing.assert_array_equal(got["idx"], ref["idx"])
    np.testing.assert_array_equal(got["d_index"], ref["d_index"])
    np.testing.assert_allclose(got["metric"], ref["metric"], rtol=1e-12)
    assert np.abs(row - row_ref).max() <= 2e-7 * np.abs(row_ref).max()          # the row dump is float32


def test_fused_4096_kernel_equals_two_kernel_path(engine):
    """N = 4096, one block, one carrier: forward + correlate in one kernel (option fused_4k) -- same arithmetic in the same
    order as lds_forward_kernel + lds_correlate_kernel, so the peak records are bit-identical, for every item-chunk size."""
    import torch
    from gnss_dsp_tools_amd import acquire, signals, synth
    sig = signals.get("gps-l1")
    items = list(range(1, 33))
    dop = acquire.doppler_grid([-5000.0, 5000.0, 250.0])
    xs = synth.make_epochs(sig, 1, 1357, synth.default_sats(items), 5, nsamp=4096)
    xd = torch.from_numpy(xs).cuda()
    try:
        engine.set_option("fused_4k", 0)
        plain = engine.search_batch_dev(sig, xd, items, dop, 1)
        torch.cuda.synchronize()
        plain = plain.cpu().numpy().tobytes()
        engine.set_option("fused_4k", 2)                                   # 2: also for batches this small
        engine.set_profiling(True)
        for pch in (0, 1, 5, 8, 32):
            engine.set_option("lds_pch", pch)
            engine.reset_stage_times()
            fused = engine.search_batch_dev(sig, xd, items, dop, 1)
            torch.cuda.synchronize()
            assert engine.stage_times()["mix_nco"][1] == 0                 # no separate forward launch
            assert fused.cpu().numpy().tobytes() == plain, pch
        # a single item and a two-block search fall back / stay correct
        one = engine.search_batch_dev(sig, xd, [7], dop, 1)
        torch.cuda.synchronize()
        engine.set_option("fused_4k", 0)
        engine.set_option("lds_pch", 0)
        one_plain = engine.search_batch_dev(sig, xd, [7], dop, 1)
        torch.cuda.synchronize()
        assert one.cpu().numpy().tobytes() == one_plain.cpu().numpy().tobytes()
    finally:
        engine.set_option("fused_4k", 1)
        engine.set_option("lds_pch", 0)
        engine.set_profiling(False)


@pytest.mark.parametrize("cid", ["cfg1_gps_l1_prn1", "cfg2_gps_l1_all32", "edge_fractional_grid"])      # the B = 1 goldens of N = 4096
def test_fused_4096_bench_kernel_matches_reference_golden(engine, golden_cases, cid):
    """The kernel the headline bench line times (lds_fused4k_kernel; auto-selected only for batches of >= 1024 units) held to
    the reference's own outputs directly: option fused_4k = 2 forces it for these single-epoch golden cases, tie-safe locations on as
    in the bench, and the stage timers prove that it ran -- no separate forward launch, one Doppler-scan launch.  (The option search1
    of round 3 -- the scan inside the kernel, no re-evaluation hook -- is retired: accepted and ignored.)"""
    case = golden_cases[cid]
    x = case_iq(case)
    try:
        engine.set_engine(2)
        engine.set_option("fused_4k", 2)
        engine.set_option("search1", 1)                         # retired: must change nothing
        engine.set_profiling(True)
        engine.reset_stage_times()
        got = engine.search_all(case["script"], x, case["items"], case["doppler_search"], case["ms"])
        st = engine.stage_times()
        assert st["mix_nco"][1] == 0 and st["lds_correlate"][1] >= 1, st
        assert st["best_doppler"][1] == 1, st
        assert engine.get_option("tie_safe") == 1
    finally:
        engine.set_profiling(False)
        engine.set_option("fused_4k", 1)
        engine.set_option("search1", 0)
        engine.set_engine(0)
    _assert_results(got, case["results"], case)


FULL_SIZE_JOBS = [  # BASELINE.json configs 2-5: signal, items, Doppler search, blocks
    ("cfg2", "gps-l1", list(range(1, 33)), [-5000.0, 5000.0, 250.0], 1),
    ("cfg3", "galileo-e1b", list(range(1, 37)), [-4000.0, 4000.0, 125.0], 1),
    ("cfg3", "galileo-e1c", list(range(1, 37)), [-4000.0, 4000.0, 125.0], 1),
    ("cfg4", "gps-l5i", list(range(1, 33)), [-7000.0, 7000.0, 200.0], 1),
    ("cfg4", "beidou-b2ad", list(range(1, 64)), [-7000.0, 7000.0, 200.0], 1),
    ("cfg5", "gps-l1", list(range(1, 33)), [-10000.0, 10000.0, 100.0], 10),
    ("cfg5", "galileo-e1b", list(range(1, 51)), [-10000.0, 10000.0, 100.0], 1),
    ("cfg5", "beidou-b1i", list(range(1, 64)), [-10000.0, 10000.0, 100.0], 10),
    ("cfg5", "glonass-l1", list(range(-7, 8)), [-10000.0, 10000.0, 100.0], 10),
]


@pytest.mark.parametrize("cfg,name,items,ds,B", FULL_SIZE_JOBS, ids=["%s-%s" % (j[0], j[1]) for j in FULL_SIZE_JOBS])
def test_full_size_configs_agree_with_the_complex128_pipeline(engine, cfg, name, items, ds, B):
    """Every BASELINE configuration at its FULL size (all items, the whole Doppler grid, every block), two seeded epochs, through
    the default fp32 engines and through engine 5 (complex128 on the device, itself held to the reference's goldens at 1e-10):
    identical peak locations -- no near-tie allowance: candidates fp32 cannot separate are re-evaluated in complex128
    (tests/test_tie_safe.py) -- and metrics within 2e-6 (north_star's bar is 1e-5).  The numpy oracle cannot do these sizes in
    test time."""
    import torch
    from gnss_dsp_tools_amd import acquire, signals, synth
    sig = signals.get(name)
    dop = acquire.doppler_grid(ds)
    xs = synth.make_epochs(sig, B, 31337, synth.default_sats(items), 2, nsamp=sig.samples_needed(B))
    xd = torch.from_numpy(xs).cuda()
    engine.set_engine(0)
    a = engine.search_batch_dev(sig, xd, items, dop, B)
    torch.cuda.synchronize()
    pa = a.cpu().numpy().view(acquire.PEAK_DTYPE).reshape(-1).copy()
    try:
        engine.set_engine(5)
        c = engine.search_batch_dev(sig, xd, items, dop, B)
        torch.cuda.synchronize()
    finally:
        engine.set_engine(0)
    pc = c.cpu().numpy().view(acquire.PEAK_DTYPE).reshape(-1)
    rel = np.abs(pa["metric"] - pc["metric"]) / np.abs(pc["metric"])
    same = (pa["idx"] == pc["idx"]) & (pa["d_index"] == pc["d_index"])
    assert bool(same.all()), (cfg, name, np.flatnonzero(~same)[:8])
    assert float(rel[same].max()) <= 2e-6, (cfg, name, float(rel[same].max()))


@pytest.mark.parametrize("cid", ["cfg4_l5i_subset", "gal_e6b", "bds_b2bq", "xona_x5p"])
@pytest.mark.parametrize("mfma", [0, 1])
def test_prime_factor_inner_kernel_item_chunks_match_reference_golden(engine, golden_cases, cid, mfma):
    """The prime-factor inner kernel with item chunks that do not divide the item count (the tail of a chunk is skipped row by row,
    the code-spectrum prefetch runs past it) and both outer inverse kernels, raw and max/mean metric (xona_x5p), one and several blocks."""
    case = golden_cases[cid]
    x = case_iq(case)
    engine.set_option("split_mfma", mfma)
    try:
        for pch in (0, 3, 1):
            engine.set_option("split_pch", pch)
            got = engine.search_all(case["script"], x, case["items"], case["doppler_search"], case["ms"])
            _assert_results(got, case["results"], case)
    finally:
        engine.set_option("split_mfma", 0)
        engine.set_option("split_pch", 0)


def test_randomised_differential_run_of_all_engines():
    """tools/fuzz_engines.py for 15 s: random signals, item lists (with duplicates), grids (1-24 bins), blocks, epochs, workspace limits
    and tuning switches; the default engine must equal itself under every switch / chunking byte for byte and agree with the
    complex128 verification pipeline (same location, metric within 2e-6).  The long runs are in profiles/r02_fuzz_engines.log."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "fuzz_engines.py"), "15", "77"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
    assert '"failures": 0' in out.stdout


@pytest.mark.parametrize("world,name,items,ds,ms,mode", [
    (2, "gps-l1", [3, 4, 11, 28], [-2000.0, 2500.0, 250.0], 2, ""),                  # 18 bins -> 9 + 9
    (3, "glonass-l1", [-2, 5, 1], [1000.0, 2300.0, 100.0], 1, "GLOO_ASYNC"),         # 13 bins -> 5 + 4 + 4, FDMA biases, async exchange
    (2, "gps-l5i", [7, 8, 9], [1000.0, 2000.0, 100.0], 1, ""),                       # split engine, Doppler tiles inside each slice
    (2, "galileo-e1b", [5, 11, 24], [1000.0, 1375.0, 125.0], 8, ""),                 # 3 bins < 4 per rank -> item split, ragged slices
])
def test_ranks_sharing_the_gpu_with_real_kernels_equal_the_single_process_search(engine, tmp_path, world, name, items, ds, ms, mode):
    """The sharded path with real per-rank compute: `world` processes, each with its own HIP engine on cuda:0, Doppler (or item)
    slices, ONE all-gather of peak records (gloo on host tensors -- RCCL refuses two ranks on one device), tie-exact merge.  The
    tuples must equal what one process returns for the whole grid."""
    import json
    import os
    import socket
    import subprocess
    import sys
    from gnss_dsp_tools_amd import signals, synth
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out = tmp_path / "res.json"
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), GLOO_HIP="1")
        if mode:
            env[mode] = "1"
        procs.append(subprocess.Popen([sys.executable, os.path.join(root, "tests", "_gloo_worker.py"), str(out), name, ",".join(map(str, items)),
                                       ",".join(map(str, ds)), str(ms)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    for p in procs:
        try:
            log, _ = p.communicate(timeout=600)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        assert p.returncode == 0, log.decode()[-2000:]
    res = json.load(open(out))
    sig = signals.get(name)
    xs = synth.make_epochs(sig, sig.blocks(ms), 5150, [(items[0], 0.4, 1537.0, 1201)], 2)        # the worker's seed and satellites
    for e in range(xs.shape[0]):
        want = engine.search_all(sig, xs[e], items, ds, ms)
        for got, w in zip(res[e], want):
            assert (got[0], got[1], got[2]) == (float(w[0]), float(w[1]), float(w[2])), (e, got, w)


@pytest.mark.parametrize("name,fs,coffset,n_in", [("gps-l1", 8184000.0, 1250000.0, 57288), ("gps-l5i", 40.0e6, -1250000.0, 240000),
                                                   ("galileo-e1b", 10.0e6, 250000.0, 1283)])
def test_specialised_161_tap_front_end_kernels_equal_the_generic_ones_bit_for_bit(engine, name, fs, coffset, n_in):
    """acquire-gps-l1.py:78-96 on the GPU: for the reference's 161-tap filter the carrier wipe-off is fused into the forward FIR pass
    and both passes run the fully unrolled five-outputs-per-thread kernel; GACQ_OPT_FE_GENERIC selects the any-length kernels.
    Same products in the same order: the conditioned samples must be identical (incl. a recording only a few tiles long and the
    odd-extension edges, n_in = 1283 > 3 * 161 * ... barely above filtfilt's pad length)."""
    import torch
    from gnss_dsp_tools_amd import signals
    sig = signals.get(name)
    rng = np.random.Generator(np.random.PCG64(4242))
    iq = np.clip(np.round(18.0 * rng.standard_normal((n_in, 2))), -127, 127).astype(np.int8)
    ms_pad = max(1, int(n_in / fs * 1000.0) - 1)
    try:
        engine.set_option("fe_generic", 1)
        want = engine.frontend_dev(sig, iq, fs, coffset, ms_pad)
        torch.cuda.synchronize()
        want = want.cpu().numpy().copy()
        engine.set_option("fe_generic", 0)
        got = engine.frontend_dev(sig, iq, fs, coffset, ms_pad)
        torch.cuda.synchronize()
        got = got.cpu().numpy()
    finally:
        engine.set_option("fe_generic", 0)
    assert got.tobytes() == want.tobytes()
    assert np.isfinite(got.view(np.float32)).all() and float(np.abs(got).max()) > 0.0
