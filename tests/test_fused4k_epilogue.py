"""Row epilogue of the fused 4096-point kernel (lds_fused4k_kernel, csrc/gacq_ldsfft.hip): the last radix-4 layer of the inverse
transform leaves (re, re) / (im, im) pairs of lags k and k + 8, the squared magnitudes are packed, and the two wave reductions
combine their four 16-lane rows on DPP and deliver the result in lane 63.

What can go wrong is a renaming -- which register holds which lag, which lane holds the wave's result -- so the inputs put the
peak at a known (register, lane, wave) position: lag 256 k + l lives in register k of lane l & 63 of wave l >> 6.  Every
comparison is byte for byte against the two-kernel path (option fused_4k = 0: lds_forward_kernel + lds_correlate_kernel, which
share none of the changed code), same engine, same input."""
import numpy as np
import pytest

LANES = (0, 15, 16, 63, 64, 255)          # first / last lane of a 16-lane DPP row, of a wave, of the workgroup
LAGS = [256 * k + l for k in range(16) for l in LANES]


@pytest.fixture(scope="module")
def eng():
    from gnss_dsp_tools_amd import acquire
    e = acquire.Engine(0)
    e.use_torch_stream()
    e.set_profiling(True)
    yield e
    e.close()


def _run(eng, sig, xd, items, dop, fused):
    """Peak records of one batch as a host array; the two-kernel path is recognised by its separate forward launch."""
    import torch
    from gnss_dsp_tools_amd import acquire
    eng.set_option("fused_4k", 2 if fused else 0)           # 2: the fused kernel also for batches this small
    eng.set_option("lds_pch", 0)
    eng.reset_stage_times()
    out = eng.search_batch_dev(sig, xd, items, dop, 1)
    torch.cuda.synchronize()
    forward_launches = eng.stage_times()["mix_nco"][1]
    assert (forward_launches == 0) == bool(fused), (fused, forward_launches)
    return out.cpu().numpy().view(acquire.PEAK_DTYPE).reshape(xd.shape[0], len(items))


@pytest.fixture(scope="module")
def placed(eng):
    """96 epochs, one PRN 7 arrival each, at lag 256 k + l for every register k and the edge lanes l; records of the two-kernel path."""
    import torch
    from gnss_dsp_tools_amd import signals, synth
    sig = signals.get("gps-l1")
    xs = np.stack([synth.make_iq(sig, 1, 5000 + lag, [(7, 0.5, 0.0, (4096 - lag) % 4096)], nsamp=4096) for lag in LAGS])
    xd = torch.from_numpy(xs).cuda()
    assert eng.get_option("tie_safe") == 1
    return sig, xd, _run(eng, sig, xd, [7, 7], np.array([0.0]), fused=False)


@pytest.mark.gpu
def test_peak_in_every_register_and_at_the_row_edges_of_every_wave(eng, placed):
    sig, xd, plain = placed
    # the condition that makes the comparison cover every position: the yardstick itself finds each peak at its wanted lag
    for e, lag in enumerate(LAGS):
        assert plain["idx"][e, 0] == lag and plain["idx"][e, 1] == lag, (e, lag, plain[e])
    got = _run(eng, sig, xd, [7, 7], np.array([0.0]), fused=True)
    assert got.tobytes() == plain.tobytes(), np.nonzero(got != plain)


@pytest.mark.gpu
def test_slow_location_path_on_the_renamed_registers(eng, placed):
    """tie_eps_ppb = 10^9 (threshold 0): every wave takes the m[k] == maximum branch of wave_first_max, smallest k first."""
    sig, xd, _ = placed
    eps, cap = eng.get_option("tie_eps_ppb"), eng.get_option("tie_cap")
    try:
        eng.set_option("tie_eps_ppb", 1000000000)
        eng.set_option("tie_cap", 0)
        plain = _run(eng, sig, xd, [7, 7], np.array([0.0]), fused=False)
        got = _run(eng, sig, xd, [7, 7], np.array([0.0]), fused=True)
    finally:
        eng.set_option("tie_eps_ppb", eps)
        eng.set_option("tie_cap", cap)
    assert got.tobytes() == plain.tobytes(), np.nonzero(got != plain)


@pytest.mark.gpu
def test_sums_of_noise_rows_through_the_dpp_reduction(eng):
    """Noise only: every wave and every 16-lane row has a different partial sum, so another combine order changes bits of the metric."""
    import torch
    from gnss_dsp_tools_amd import signals, synth
    sig = signals.get("gps-l1")
    xd = torch.from_numpy(synth.make_epochs(sig, 1, 31, [], 8, nsamp=4096)).cuda()
    items = list(range(1, 33))
    dop = np.array([-500.0, 250.0, 1500.0])
    plain = _run(eng, sig, xd, items, dop, fused=False)
    got = _run(eng, sig, xd, items, dop, fused=True)
    assert got.tobytes() == plain.tobytes(), np.nonzero(got != plain)
