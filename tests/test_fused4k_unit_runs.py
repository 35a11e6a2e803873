"""Work items of the fused 4096-point kernel (lds_fused4k_kernel, csrc/gacq_ldsfft.hip): a workgroup does several work items (epoch,
Doppler bin, item chunk) and pays its set-up once -- a fixed run of `f4k_run` consecutive ones under the static map, or, with
`f4k_claim`, whatever it takes from eight queues with atomic counters (its own XCD's first, then the others'); the forward transform
takes its twiddle powers from the inverse transform's resident ones.

The static map and the queues are host + device functions and are checked on the host through gacq_debug_f4k_map (no GPU).  Every GPU
comparison is byte for byte against the two-kernel path (option fused_4k = 0: lds_forward_kernel + lds_correlate_kernel, which share
none of the changed code), same engine, same input, tie-safe locations on.  In the GPU inputs every (epoch, Doppler bin) carries a
satellite of its own at a delay of its own, so a run that kept the x window or the carrier of its previous work item locates another
peak; that the two-kernel path finds each of them where it was put is asserted before anything is compared.

Both paths write their row records into one buffer that lives as long as the engine, so a fused launch that skipped a work item would
find the right bytes already there.  Every fused run therefore starts from a poisoned buffer (Engine.poison_rows: every record wins any
Doppler scan), and one test shows what a single record left undone does to the results."""
import ctypes
import itertools

import numpy as np
import pytest

BINS3 = np.array([-500.0, 250.0, 1500.0])
ITEMS5 = [1, 2, 3, 4, 5]
ITEMS40 = list(range(1, 33)) + list(range(1, 9))           # 40 rows of work: PRN 1-32, then PRN 1-8 again
DOP2 = np.array([-250.0, 500.0])
CUS = 256


# ---- the map, on the host ------------------------------------------------------------------------------------------------------------

def _walk(E, D, nchunk, run, cus=CUS):
    from gnss_dsp_tools_amd import _native as nat
    info = (ctypes.c_int * 4)()
    cap = E * D * nchunk + 16
    work = np.full((cap, 4), -1, dtype=np.int32)
    n = nat.lib.gacq_debug_f4k_map(E, D, nchunk, run, cus, info, work.ctypes.data_as(nat.c_int_p), cap)
    assert 0 <= n <= cap, (E, D, nchunk, run, n)
    return dict(run=info[0], by_epoch=info[1], nruns=info[2], grid=info[3]), work[:n]


@pytest.mark.parametrize("E", [1, 3, 9, 64, 65, 1024])
def test_map_covers_every_work_item_once_and_keeps_an_epoch_on_one_xcd(E):
    for D, nchunk, U in itertools.product([1, 3, 40], [1, 2, 5], [0, 1, 2, 7, 40]):
        info, w = _walk(E, D, nchunk, U)
        where = (E, D, nchunk, U, info)
        blk, e, d, c = (w[:, k].astype(np.int64) for k in range(4))
        # every (epoch, bin, chunk) exactly once, nothing else
        assert len(w) == E * D * nchunk, where
        assert e.min() >= 0 and e.max() < E and d.min() >= 0 and d.max() < D and c.min() >= 0 and c.max() < nchunk, where
        assert len(np.unique((e * D + d) * nchunk + c)) == len(w), where
        # the run: as forced, capped at the work items of one epoch; no workgroup walks more, and the grid holds every block
        span = D * nchunk if E >= 64 else ((E * D + 7) // 8) * nchunk          # work items one run index counts through
        assert 1 <= info["run"] <= min(D * nchunk, span) and (U == 0 or info["run"] == min(U, D * nchunk, span)), where
        assert blk.max() < info["grid"] and np.bincount(blk).max() <= info["run"], where
        assert np.all(np.diff(blk) >= 0), where                      # block order, each block's items in its walking order
        assert info["by_epoch"] == (1 if E >= 64 else 0), where
        if info["by_epoch"]:
            assert np.array_equal(blk % 8, e % 8), where            # workgroup b runs on XCD b % 8: an epoch stays on one XCD
            assert len(np.unique(np.stack([blk, e], 1), axis=0)) == len(np.unique(blk)), where      # a run never crosses an epoch
        else:
            assert np.array_equal(blk % 8, (e * D + d) % 8), where  # units dealt round-robin: a run walks the units of its own XCD
        # consecutive work items inside a block: the next chunk, else chunk 0 of the next bin (by epoch) / of the XCD's next unit
        same = np.nonzero(np.diff(blk) == 0)[0]
        u = e * D + d
        step_c = (c[same + 1] == c[same] + 1) & (u[same + 1] == u[same])
        step_u = (c[same + 1] == 0) & (c[same] == nchunk - 1) & (u[same + 1] == u[same] + (1 if info["by_epoch"] else 8))
        assert np.all(step_c | step_u), where


@pytest.mark.parametrize("E,D,nchunk", [(1, 1, 1), (3, 3, 1), (9, 40, 2), (64, 2, 1), (65, 3, 5), (1024, 40, 1)])
def test_a_run_of_one_is_the_map_of_one_work_item_per_workgroup(E, D, nchunk):
    """f4k_run = 1 against the map written out: block b on XCD b % 8; by epoch, the D x nchunk blocks of epoch e on XCD e % 8."""
    info, w = _walk(E, D, nchunk, 1)
    want = []
    by_epoch = E >= 64
    grid = 8 * ((E + 7) // 8) * D * nchunk if by_epoch else 8 * ((E * D + 7) // 8) * nchunk
    assert info["run"] == 1 and info["grid"] == grid
    for b in range(grid):
        xcd, j = b & 7, b >> 3
        if by_epoch:
            e8 = (j // (D * nchunk)) * 8 + xcd
            if e8 >= E:
                continue
            u = e8 * D + (j % (D * nchunk)) // nchunk
        else:
            u = (j // nchunk) * 8 + xcd
            if u >= E * D:
                continue
        want.append((b, u // D, u % D, j % nchunk))
    assert np.array_equal(w, np.array(want, dtype=np.int32))


def test_automatic_run_leaves_four_rounds_of_resident_workgroups():
    """Auto: the fewest runs whose grid still has 16 workgroups per compute unit (four rounds of four resident ones), cut to equal lengths."""
    info, _ = _walk(1024, 40, 1, 0)
    assert info["run"] == 10 and info["grid"] == 4096, info         # the headline shape on 256 compute units
    for E, D, nchunk, cus in [(1024, 40, 1, 256), (1024, 40, 2, 256), (1024, 40, 1, 304), (64, 40, 1, 256), (1024, 3, 5, 64), (3, 3, 1, 256), (4096, 40, 1, 256)]:
        info, _ = _walk(E, D, nchunk, 0, cus)
        span = D * nchunk if E >= 64 else ((E * D + 7) // 8) * nchunk
        assert info["run"] == 1 or info["grid"] >= 16 * cus, (E, D, nchunk, cus, info)
        assert info["run"] == -(-span // info["nruns"]), (E, D, nchunk, cus, info)           # runs of equal length
        for longer in range(info["run"] + 1, min(span, D * nchunk) + 1):                     # fewer runs would not leave four rounds
            other, _ = _walk(E, D, nchunk, longer, cus)
            assert other["nruns"] == info["nruns"] or other["grid"] < 16 * cus, (E, D, nchunk, cus, info, other)


def test_map_entry_rejects_bad_arguments_and_the_option_is_declared():
    from gnss_dsp_tools_amd import _native as nat
    info = (ctypes.c_int * 4)()
    for args in [(0, 1, 1, 1, CUS), (1, 0, 1, 1, CUS), (1, 1, 0, 1, CUS), (1, 1, 1, -70000, CUS), (1, 1, 1, 1, 0)]:
        assert nat.lib.gacq_debug_f4k_map(*args, info, None, 0) < 0, args
    assert nat.lib.gacq_debug_f4k_map(3, 3, 2, 2, CUS, info, None, 0) == 18          # counting alone needs no buffer
    assert nat.OPTIONS["f4k_run"] == 18 and nat.OPTIONS["f4k_claim"] == 19


@pytest.mark.parametrize("E", [1, 3, 9, 64, 65, 1024])
def test_queues_of_claimed_work_hold_every_work_item_once_in_the_static_order(E):
    """Queue q is what the static map with runs of 1 gives to the blocks b % 8 == q, in block order; by epoch, epoch e is in queue e % 8."""
    from gnss_dsp_tools_amd import _native as nat
    for D, nchunk in itertools.product([1, 3, 40], [1, 2, 5]):
        _, static = _walk(E, D, nchunk, 1)
        info = (ctypes.c_int * 4)()
        cap = E * D * nchunk
        work = np.full((cap, 4), -1, dtype=np.int32)
        assert nat.lib.gacq_debug_f4k_map(E, D, nchunk, -8, CUS, info, work.ctypes.data_as(nat.c_int_p), cap) == cap, (E, D, nchunk)
        assert info[0] == 1 and info[3] == 8
        order = np.argsort(static[:, 0] % 8, kind="stable")           # the static walk, regrouped by block % 8
        assert np.array_equal(work[:, 1:], static[order, 1:]) and np.array_equal(work[:, 0], static[order, 0] % 8), (E, D, nchunk)
        if E >= 64:
            assert np.array_equal(work[:, 0], work[:, 1] % 8), (E, D, nchunk)


def test_claimed_work_is_automatic_only_with_more_work_than_resident_workgroups():
    from gnss_dsp_tools_amd import _native as nat
    info = (ctypes.c_int * 4)()
    for E, D, nchunk, claim, on, grid in [(1024, 40, 1, 1, 1, 1024), (64, 3, 1, 1, 0, 192), (3, 3, 1, 1, 0, 16), (1024, 40, 1, 0, 0, 40960),
                                         (25, 40, 1, 1, 0, 1000), (26, 40, 1, 1, 1, 1024), (3, 3, 1, 12, 1, 16), (64, 3, 1, 8, 1, 8)]:
        nat.lib.gacq_debug_f4k_map(E, D, nchunk, -claim if claim else 1, CUS, info, None, 0)
        if claim:
            assert (info[0], info[3]) == (on, grid), (E, D, nchunk, claim, list(info))
        else:
            assert info[3] == grid


# ---- on the GPU ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def eng():
    from gnss_dsp_tools_amd import acquire
    e = acquire.Engine(0)
    e.use_torch_stream()
    e.set_profiling(True)
    yield e
    e.close()


def _run(eng, sig, xd, items, dop, fused, pch=0, run=1, claim=0, poison_after=-1):
    """Peak records of one batch as bytes; the two-kernel path is recognised by its separate forward launch."""
    import torch
    eng.set_option("fused_4k", 2 if fused else 0)           # 2: the fused kernel also for batches this small
    eng.set_option("lds_pch", pch)
    eng.set_option("f4k_run", run)
    eng.set_option("f4k_claim", claim)
    if fused:                                               # whatever this launch does not write is seen in the results
        assert eng.poison_rows(poison_after) >= xd.shape[0] * len(items) * len(dop)
    eng.reset_stage_times()
    out = eng.search_batch_dev(sig, xd, items, dop, 1)
    torch.cuda.synchronize()
    forward_launches = eng.stage_times()["mix_nco"][1]
    assert (forward_launches == 0) == bool(fused), (fused, forward_launches)
    return out.cpu().numpy().tobytes()


def _marked_epochs(eng, nepoch, dop, items, seed):
    """Epoch e holds, at Doppler bin k, item items[k] at a delay that no other (epoch, bin) has.  Returns the signal, the device tensor and
    the records of the two-kernel path, after asserting that it finds every one of them at its lag and in its bin."""
    import torch
    from gnss_dsp_tools_amd import acquire, signals, synth
    sig = signals.get("gps-l1")
    delay = lambda e, k: (101 + 37 * e + 1013 * k) % 4096
    xs = np.stack([synth.make_iq(sig, 1, seed + 1000 * e, [(items[k], 0.5, float(dop[k]), delay(e, k)) for k in range(len(dop))], nsamp=4096)
                   for e in range(nepoch)])
    xd = torch.from_numpy(xs).cuda()
    assert eng.get_option("tie_safe") == 1
    plain = _run(eng, sig, xd, items, dop, fused=False)
    rec = np.frombuffer(plain, dtype=acquire.PEAK_DTYPE).reshape(nepoch, len(items))
    for e in range(nepoch):
        for k in range(len(dop)):
            assert rec["idx"][e, k] == (4096 - delay(e, k)) % 4096 and rec["d_index"][e, k] == k, (e, k, rec[e, k])
    return sig, xd, plain


@pytest.fixture(scope="module")
def by_epoch_shape(eng):
    """64 epochs x 3 bins x 5 items: the by-epoch map, one chunk per (epoch, bin), three work items per epoch."""
    return _marked_epochs(eng, 64, BINS3, ITEMS5, 3100)


@pytest.fixture(scope="module")
def round_robin_shape(eng):
    """3 epochs x 3 bins x 5 items: 9 units dealt round-robin over 8 XCDs."""
    return _marked_epochs(eng, 3, BINS3, ITEMS5, 3200)


@pytest.fixture(scope="module")
def shape40(eng):
    """One epoch, two Doppler bins, 40 items (the shape of tests/test_fused4k_item_pipeline.py), and its two-kernel records."""
    import torch
    from gnss_dsp_tools_amd import signals, synth
    sig = signals.get("gps-l1")
    xd = torch.from_numpy(synth.make_epochs(sig, 1, 4242, synth.default_sats(range(1, 33)), 1, nsamp=4096)).cuda()
    assert eng.get_option("tie_safe") == 1
    return sig, xd, _run(eng, sig, xd, ITEMS40, DOP2, fused=False)


@pytest.mark.gpu
@pytest.mark.parametrize("run,claim", [(1, 0), (3, 0), (1, 8)])
def test_one_row_record_left_undone_shows_in_the_results(eng, by_epoch_shape, run, claim):
    """The yardstick of every comparison below: with the buffer poisoned, a single record that the launch leaves as it found it -- here
    epoch 37, item 1, bin 2, not the bin that item's satellite is in -- takes over that (epoch, item)'s result and nothing else."""
    from gnss_dsp_tools_amd import acquire
    sig, xd, plain = by_epoch_shape
    e, p, d = 37, 1, 2
    got = _run(eng, sig, xd, ITEMS5, BINS3, fused=True, run=run, claim=claim, poison_after=(e * len(ITEMS5) + p) * len(BINS3) + d)
    assert got != plain
    want = np.frombuffer(plain, dtype=acquire.PEAK_DTYPE).reshape(64, len(ITEMS5)).copy()
    rec = np.frombuffer(got, dtype=acquire.PEAK_DTYPE).reshape(64, len(ITEMS5))
    assert want["d_index"][e, p] == 1 and rec["d_index"][e, p] == d and rec["idx"][e, p] == 1234, (want[e, p], rec[e, p])
    want[e, p] = rec[e, p]
    assert rec.tobytes() == want.tobytes()
    assert _run(eng, sig, xd, ITEMS5, BINS3, fused=True, run=run, claim=claim) == plain      # the hook is spent: nothing armed


@pytest.mark.gpu
@pytest.mark.parametrize("run", [1, 2, 3, 4])
def test_runs_under_the_by_epoch_map_equal_the_two_kernel_path(eng, by_epoch_shape, run):
    """Three work items per epoch: a run of 2 is cut at the epoch's end (2 + 1), a run of 3 is a whole epoch, a run of 4 is clamped."""
    sig, xd, plain = by_epoch_shape
    assert _run(eng, sig, xd, ITEMS5, BINS3, fused=True, run=run) == plain, run


@pytest.mark.gpu
@pytest.mark.parametrize("run", [1, 2, 5])
def test_runs_under_the_round_robin_map_equal_the_two_kernel_path(eng, round_robin_shape, run):
    """9 units on 8 XCDs: XCD 0 walks units 0 and 8 (another epoch and another bin), the runs of the other XCDs end after one unit
    because their second one does not exist; a run of 5 is clamped."""
    sig, xd, plain = round_robin_shape
    assert _run(eng, sig, xd, ITEMS5, BINS3, fused=True, run=run) == plain, run


@pytest.mark.gpu
@pytest.mark.parametrize("run", [2, 4])
def test_chunks_inside_runs_equal_the_two_kernel_path(eng, shape40, run):
    """Chunks of 33 and 7 items in one run: flush at slot 31, wrap into slot 0, a second flush of one item, then a short last chunk."""
    sig, xd, plain = shape40
    assert _run(eng, sig, xd, ITEMS40, DOP2, fused=True, pch=33, run=run) == plain, run


@pytest.mark.gpu
def test_chunks_then_the_next_bin_inside_one_run(eng):
    """64 epochs x 2 bins x 40 items in chunks of 33 + 7, runs of 3: (bin 0 chunk 0, bin 0 chunk 1, bin 1 chunk 0), then (bin 1 chunk 1) --
    a ring that wrapped, a short chunk, and then a new x window and carrier in the same workgroup."""
    items = ITEMS40
    sig, xd, plain = _marked_epochs(eng, 64, DOP2, items, 3300)
    assert _run(eng, sig, xd, items, DOP2, fused=True, pch=33, run=3) == plain


@pytest.fixture(scope="module")
def uneven_queues_shape(eng):
    """65 epochs x 3 bins x 5 items: queue 0 holds nine epochs, the others eight, so their workgroups end in queue 0."""
    return _marked_epochs(eng, 65, BINS3, ITEMS5, 3400)


@pytest.mark.gpu
@pytest.mark.parametrize("claim", [8, 40, 256])
def test_claimed_work_equals_the_two_kernel_path(eng, uneven_queues_shape, claim):
    """8 workgroups: each walks its whole queue (24 or 27 work items, a new x window every third) and then takes from the queues that are
    not yet empty; 40: five per queue; 256: 32 per queue, more than a queue's 24 or 27 items, so some find nothing and leave at once."""
    sig, xd, plain = uneven_queues_shape
    assert _run(eng, sig, xd, ITEMS5, BINS3, fused=True, claim=claim) == plain, claim


@pytest.mark.gpu
@pytest.mark.parametrize("claim", [8, 16, 4096])
def test_claimed_work_under_the_round_robin_map_equals_the_two_kernel_path(eng, round_robin_shape, claim):
    """9 units: queue 0 holds two, the others one.  8 workgroups: the second unit of queue 0 goes to whichever asks first."""
    sig, xd, plain = round_robin_shape
    assert _run(eng, sig, xd, ITEMS5, BINS3, fused=True, claim=claim) == plain, claim


@pytest.mark.gpu
def test_claimed_work_with_chunks_and_the_slow_location_path(eng, shape40):
    """One epoch x 2 bins x (33 + 7) items handed out to 8 workgroups, rows on the slow path of wave_first_max."""
    sig, xd, plain = shape40
    assert _run(eng, sig, xd, ITEMS40, DOP2, fused=True, pch=33, claim=8) == plain
    eps, cap = eng.get_option("tie_eps_ppb"), eng.get_option("tie_cap")
    try:
        eng.set_option("tie_eps_ppb", 1000000000)
        eng.set_option("tie_cap", len(ITEMS40) * len(DOP2))
        slow = _run(eng, sig, xd, ITEMS40, DOP2, fused=False)
        got = _run(eng, sig, xd, ITEMS40, DOP2, fused=True, pch=33, claim=8)
    finally:
        eng.set_option("tie_eps_ppb", eps)
        eng.set_option("tie_cap", cap)
    assert got == slow


@pytest.mark.gpu
def test_slow_location_path_inside_a_run(eng, shape40):
    """tie_eps_ppb = 10^9 (threshold 0): every wave of every row takes the slow path of wave_first_max; runs of 2, chunks of 33."""
    sig, xd, _ = shape40
    eps, cap = eng.get_option("tie_eps_ppb"), eng.get_option("tie_cap")
    try:
        eng.set_option("tie_eps_ppb", 1000000000)
        eng.set_option("tie_cap", len(ITEMS40) * len(DOP2))
        plain = _run(eng, sig, xd, ITEMS40, DOP2, fused=False)
        got = _run(eng, sig, xd, ITEMS40, DOP2, fused=True, pch=33, run=2)
    finally:
        eng.set_option("tie_eps_ppb", eps)
        eng.set_option("tie_cap", cap)
    assert got == plain


@pytest.mark.gpu
def test_run_option_rejects_values_out_of_range(eng):
    from gnss_dsp_tools_amd import _native as nat
    for bad in (-1, 4097, 1 << 20):
        with pytest.raises(nat.GacqError):
            eng.set_option("f4k_run", bad)
    for bad in (-1, 65537):
        with pytest.raises(nat.GacqError):
            eng.set_option("f4k_claim", bad)
    eng.set_option("f4k_run", 7)
    assert eng.get_option("f4k_run") == 7
    eng.set_option("f4k_run", 1)
    eng.set_option("f4k_claim", 24)
    assert eng.get_option("f4k_claim") == 24
    eng.set_option("f4k_claim", 1)
