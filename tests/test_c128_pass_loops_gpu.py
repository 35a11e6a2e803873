"""Engine 5 (complex128) under a workspace limit that forces its host loops round more than once: several epoch passes, a ragged
last pass, several Z' passes inside one epoch pass, and the Doppler-slice path.  The pass size changes no arithmetic, so the peak
records of a small-workspace engine are those of a roomy one byte for byte; the stage timers prove that the small run really looped."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DS = [-750.0, 1000.0, 250.0]      # -750 ... 750: D = 7 bins, more than the items of any case, so one epoch pass needs several Z' passes
MIN_WS = 1 << 20                  # gacq_set_workspace_limit takes no less


def _sats(items):
    """Two of synth.default_sats' satellites, their Doppler shifts scaled into the narrow grid (192 and -408 Hz)."""
    from gnss_dsp_tools_amd import synth
    return [(it, amp, hz / 8.0, delay) for it, amp, hz, delay in synth.default_sats(items)[:2]]


# form, signal, items, ms, E, fused_c128, stage of the Z' writer (None: the form has no Z' round trip or records no stages)
CASES = [
    ("rocfft", "gps-l1", [3, 11, 28], 2, 3, 0, None),                   # the rocFFT double pipeline: no stage timers
    ("lds4k", "gps-l1", [3, 11, 28], 2, 3, 1, None),                    # N = 4096, B = 2: epoch passes only
    ("fused4k", "gps-l1", [3, 11, 28], 1, 3, 1, None),                  # N = 4096, B = 1: buffers row records only
    ("split4", "beidou-b1i", [6, 7, 33], 2, 3, 1, "lds_correlate"),     # N = 4 x 4096, B = 2
    ("split4-fdma", "glonass-l1", [-7, 0, 3], 1, 2, 1, "lds_correlate"),  # a carrier per item: one item per writer workgroup
    ("split16", "galileo-e1b", [1, 19, 36], 8, 2, 1, "lds_correlate"),  # N = 16 x 4096, B = 1
    ("r31", "galileo-e6b", [1, 50], 1, 2, 1, "conj_mul"),               # N = 30690 = 31 x 990, B = 1
]


def _records(eng, sig, xd, items, dop, B):
    import torch
    out = eng.search_batch_dev(sig, xd, items, dop, B)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("form,name,items,ms,E,fused,writer", CASES, ids=[c[0] for c in CASES])
def test_complex128_forms_loop_over_epoch_and_correlation_passes_same_records(form, name, items, ms, E, fused, writer):
    """Workspace of one epoch's forward spectra (one epoch per pass, no Doppler slicing) and, where E = 3, of two (passes of 2 and 1).
    Launch counts: mix_nco once per epoch pass, ceil(E / (workspace // one_epoch_bytes)); the Z' writer once per Z' pass, which holds
    workspace // unit_bytes units (split: the P items of an (epoch, bin); radix-31: one (epoch, item, bin) group) -- with one carrier
    that is D // P < D units, so more Z' passes than epoch passes.  With a carrier per item (the FDMA case) one epoch's forward spectra
    [F = P][D][B][N] are exactly the D units of its Z', so the smallest workspace that does not slice the grid holds an epoch pass's Z'
    whole: there the writer count equals the epoch passes, and only the exact count is asserted.  gps-l1's one-epoch spectra are
    smaller than the least workspace limit the library takes (1 MiB); the limit is then 1 MiB, which still holds one epoch only for
    B = 2 and is immaterial for the fused form."""
    import torch
    from gnss_dsp_tools_amd import acquire, signals, synth
    sig = signals.get(name)
    B = sig.blocks(ms)
    dop = acquire.doppler_grid(DS)
    P, D, N = len(items), len(dop), sig.nfft
    F = P if name.startswith("glonass") else 1
    assert D == 7 and P < D
    xs = synth.make_epochs(sig, B, 1357, _sats(items), E, nsamp=sig.samples_needed(B))
    xd = torch.from_numpy(xs).cuda()
    one_epoch = 16 * F * D * B * N
    roomy = acquire.Engine(0, engine=5)
    try:
        roomy.set_option("fused_c128", fused)
        want = _records(roomy, sig, xd, items, dop, B)
    finally:
        roomy.close()
    assert np.any(want.view(acquire.PEAK_DTYPE)["metric"] > 0)
    for ws in sorted({max(k * one_epoch, MIN_WS) for k in ((1, 2) if E == 3 else (1,))}):
        small = acquire.Engine(0, engine=5, workspace_bytes=ws)
        try:
            small.set_option("fused_c128", fused)
            small.set_profiling(True)
            small.reset_stage_times()
            got = _records(small, sig, xd, items, dop, B)
            st = small.stage_times()
        finally:
            small.close()
        assert got.tobytes() == want.tobytes(), (form, ws)
        Ec = min(E, ws // one_epoch)
        passes = [min(Ec, E - e0) for e0 in range(0, E, Ec)]
        assert form == "fused4k" or len(passes) == -(-E // (ws // one_epoch)) > 1
        print(form, "workspace", ws, "epoch passes", passes, {k: v[1] for k, v in st.items()})
        if form == "rocfft":
            assert all(v[1] == 0 for v in st.values()), st
        elif form == "fused4k":
            assert st["mix_nco"][1] == 0 and st["lds_correlate"][1] == 1 and st["best_doppler"][1] == 1, st
        else:
            assert st["mix_nco"][1] == len(passes) and st["best_doppler"][1] == len(passes), st
        if form == "lds4k":
            assert st["lds_correlate"][1] == len(passes), st
        if writer:
            units = [ne * D * (P if form == "r31" else 1) for ne in passes]
            per_pass = max(1, ws // (16 * B * N * (1 if form == "r31" else P)))
            zpasses = sum(-(-u // min(u, per_pass)) for u in units)
            assert st[writer][1] == zpasses and st["mag_peak"][1] == zpasses, (st, zpasses)
            if F == 1:
                assert st[writer][1] > st["mix_nco"][1], st


def test_complex128_doppler_slices_equal_the_single_pass():
    """One epoch's complex128 forward spectra (beidou-b1i, B = 2, 7 bins: 3.5 MiB) against a 1 MiB workspace: the grid is searched in
    slices of two bins and the slice winners are merged.  Same locations; the metric to 1e-12, the tolerance of the complex128
    cross-form tests (the merge may re-evaluate a winner in another butterfly order, so byte equality is not claimed)."""
    import torch
    from gnss_dsp_tools_amd import acquire, signals, synth
    sig = signals.get("beidou-b1i")
    items, B, E = [6, 7, 33], 2, 2
    dop = acquire.doppler_grid(DS)
    assert 16 * B * sig.nfft * len(dop) > MIN_WS >= 16 * B * sig.nfft
    xs = synth.make_epochs(sig, B, 2468, _sats(items), E, nsamp=sig.samples_needed(B))
    xd = torch.from_numpy(xs).cuda()
    roomy = acquire.Engine(0, engine=5)
    small = acquire.Engine(0, engine=5, workspace_bytes=MIN_WS)
    try:
        want = _records(roomy, sig, xd, items, dop, B).view(acquire.PEAK_DTYPE)
        got = _records(small, sig, xd, items, dop, B).view(acquire.PEAK_DTYPE)
    finally:
        roomy.close()
        small.close()
    np.testing.assert_array_equal(got["idx"], want["idx"])
    np.testing.assert_array_equal(got["d_index"], want["d_index"])
    np.testing.assert_allclose(got["metric"], want["metric"], rtol=1e-12)
