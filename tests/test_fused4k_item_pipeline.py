"""Item loop of the fused 4096-point kernel (lds_fused4k_kernel, csrc/gacq_ldsfft.hip): the records of up to 32 items are combined
in one flush from a ring of per-wave partials in LDS instead of after every row.

Every GPU comparison is byte for byte against the two-kernel path (option fused_4k = 0: lds_forward_kernel + lds_correlate_kernel,
which share none of the changed code), same engine, same input, tie-safe locations on.  The shapes are the smallest that reach each
branch of the new loop: a chunk of one item, a flush exactly at slot 31, a wrap into slot 0, a last chunk shorter than the others,
the last item of a middle and of the last chunk, both block-to-work maps (with workgroups that return early), and rows whose waves
all take the ambiguous path of wave_first_max.  The last test reads the compiled kernel's resources (no GPU)."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "gnss-dsp-tools_amd", "lib", "libgacq.so")
LLVM = "/opt/rocm/lib/llvm/bin"
ITEMS40 = list(range(1, 33)) + list(range(1, 9))           # 40 rows of work: PRN 1-32, then PRN 1-8 again
DOP2 = np.array([-250.0, 500.0])


@pytest.fixture(scope="module")
def eng():
    from gnss_dsp_tools_amd import acquire
    e = acquire.Engine(0)
    e.use_torch_stream()
    e.set_profiling(True)
    yield e
    e.close()


def _epochs(nepoch, seed, sats_for):
    import torch
    from gnss_dsp_tools_amd import signals, synth
    sig = signals.get("gps-l1")
    xs = synth.make_epochs(sig, 1, seed, synth.default_sats(sats_for), nepoch, nsamp=4096)
    return sig, torch.from_numpy(xs).cuda()


def _run(eng, sig, xd, items, dop, fused, pch=0):
    """Peak records of one batch as bytes, and whether a separate forward launch was made (the two-kernel path makes one)."""
    import torch
    eng.set_option("fused_4k", 2 if fused else 0)           # 2: the fused kernel also for batches this small
    eng.set_option("lds_pch", pch)
    eng.reset_stage_times()
    out = eng.search_batch_dev(sig, xd, items, dop, 1)
    torch.cuda.synchronize()
    forward_launches = eng.stage_times()["mix_nco"][1]
    assert (forward_launches == 0) == bool(fused), (fused, forward_launches)
    return out.cpu().numpy().tobytes()


@pytest.fixture(scope="module")
def shape40(eng):
    """One epoch, two Doppler bins, 40 items, and its records from the two-kernel path."""
    sig, xd = _epochs(1, 4242, range(1, 33))
    assert eng.get_option("tie_safe") == 1
    return sig, xd, _run(eng, sig, xd, ITEMS40, DOP2, fused=False)


@pytest.mark.gpu
@pytest.mark.parametrize("pch", [1, 2, 31, 32, 33, 40])
def test_ring_wrap_and_flush_edges_equal_the_two_kernel_path(eng, shape40, pch):
    """Chunks of 1 (every row flushes slot 0), 2, 31 (flush below the ring size, last chunk of 9), 32 (flush exactly at slot 31, last
    chunk of 8), 33 (flush at slot 31, wrap into slot 0, second flush of one item, last chunk of 7) and 40 (wrap with 8 items)."""
    sig, xd, plain = shape40
    assert _run(eng, sig, xd, ITEMS40, DOP2, fused=True, pch=pch) == plain, pch


@pytest.mark.gpu
@pytest.mark.parametrize("nepoch,nbins", [(3, 3), (64, 2)], ids=["by_unit_3x3", "by_epoch_64x2"])
def test_both_block_to_work_maps_equal_the_two_kernel_path(eng, nepoch, nbins):
    """3 epochs x 3 bins: units dealt round-robin over the XCDs (by_epoch = 0), 9 units are no multiple of 8, so workgroups return
    before the loop.  64 epochs x 2 bins: all workgroups of an epoch on one XCD (by_epoch = 1).  32 items, automatic chunk size."""
    items = list(range(1, 33))
    dop = np.array([-500.0, 250.0, 1500.0][:nbins])
    sig, xd = _epochs(nepoch, 777, items)
    plain = _run(eng, sig, xd, items, dop, fused=False)
    assert _run(eng, sig, xd, items, dop, fused=True) == plain


@pytest.mark.gpu
def test_ambiguous_rows_through_the_deferred_combine(eng, shape40):
    """tie_eps_ppb = 10^9 (threshold 0): every wave of every row takes the wave-uniform slow path of wave_first_max and every partial
    in the ring carries the tie bit.  The peak records do not show that bit (the Doppler scan consumes it), so it is asserted through
    what it causes: all 40 (epoch, item) pairs are counted ambiguous.  With a re-evaluation list that is too small every pair keeps its
    fp32 record -- the lags located by the slow path and handed through the ring -- and with one that fits they all come from the
    complex128 re-evaluation; both must equal the two-kernel path's under the same settings, at a chunk size that wraps the ring.
    A second, two-item batch isolates the bit: one satellite arrives twice with equal amplitude at two delays, at a Doppler bin whose
    neighbour (1 kHz away, the null of a 1 ms correlation) holds noise only.  With eps = 0.2 the scan finds no second bin within
    reach, so the pair is listed -- with exactly one row -- only because its winning row's record carries the tie bit."""
    import torch
    from gnss_dsp_tools_amd import synth
    sig, xd, _ = shape40
    try:
        eng.set_option("tie_eps_ppb", 1000000000)
        for cap, rows_listed, kept in ((16, 0, 40), (len(ITEMS40) * len(DOP2), 80, 0)):
            eng.set_option("tie_cap", cap)
            got = []
            for fused in (False, True):
                before = eng.tie_stats()
                got.append(_run(eng, sig, xd, ITEMS40, DOP2, fused=fused, pch=33 if fused else 0))
                st = eng.tie_stats()
                delta = {k: st[k] - before[k] for k in st}
                assert delta["rows_reevaluated"] == rows_listed and delta["kept_fp32"] == kept, (cap, fused, delta)
                assert delta["ambiguous_pairs"] + delta["kept_fp32"] >= 40, (cap, fused, delta)
            assert got[1] == got[0], cap
        # the tie bit alone: PRN 5 twice in the row, equal amplitudes, 2000 samples apart, on the grid; the other bin is its null
        sats = [(5, 0.5, 0.0, 100), (5, 0.5, 0.0, 2100)]
        x2 = torch.from_numpy(synth.make_epochs(sig, 1, 99, sats, 1, nsamp=4096)).cuda()
        dop = np.array([0.0, 1000.0])
        eng.set_option("tie_eps_ppb", 200000000)
        eng.set_option("tie_cap", 64)
        got = []
        for fused in (False, True):
            before = eng.tie_stats()
            got.append(_run(eng, sig, x2, [5, 5], dop, fused=fused))
            st = eng.tie_stats()
            delta = {k: st[k] - before[k] for k in st}
            assert delta["ambiguous_pairs"] == 2 and delta["rows_reevaluated"] == 2 and delta["kept_fp32"] == 0, (fused, delta)
        assert got[1] == got[0]
    finally:
        eng.set_option("tie_eps_ppb", 8000)
        eng.set_option("tie_cap", 0)


def _kernel_resources(tmp_path, fragment):
    """Metadata of the one gfx950 kernel whose mangled name contains `fragment`, read from the library's .hip_fatbin section with the
    ROCm LLVM tools, as tests/test_build_guards.py does (plus the LDS size)."""
    tools = [os.path.join(LLVM, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")]
    assert os.path.exists(LIB) and all(os.path.exists(t) for t in tools), "library or ROCm LLVM tools not present"
    fat = tmp_path / "fat.bin"
    subprocess.run([tools[0], "--dump-section", ".hip_fatbin=%s" % fat, LIB], check=True)
    blob = fat.read_bytes()
    starts = [m.start() for m in re.finditer(re.escape(b"__CLANG_OFFLOAD_BUNDLE__"), blob)]
    found = []
    for n, (a, b) in enumerate(zip(starts, starts[1:] + [len(blob)])):
        part = tmp_path / ("bundle%d.bin" % n)
        part.write_bytes(blob[a:b])
        co = tmp_path / ("code%d.elf" % n)
        subprocess.run([tools[1], "--unbundle", "--type=o", "--input=%s" % part, "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=%s" % co],
                       check=True, capture_output=True)
        if not co.exists() or co.stat().st_size == 0:
            continue
        notes = subprocess.run([tools[2], "--notes", str(co)], check=True, capture_output=True, text=True).stdout
        for block in notes.split("- .agpr_count:")[1:]:                     # one block per kernel
            fields = {"agpr_count": block.split()[0]}
            fields.update(re.findall(r"^\s+\.(symbol|vgpr_count|private_segment_fixed_size|vgpr_spill_count|group_segment_fixed_size):\s+(\S+)\s*$",
                                     block, flags=re.M))
            if fragment in fields["symbol"]:
                found.append({k: (v if k == "symbol" else int(v)) for k, v in fields.items()})
    assert len(found) == 1, found
    return found[0]


def test_fused_4096_kernel_resources_keep_four_workgroups_per_cu(tmp_path):
    """lds_fused4k_kernel runs four workgroups per CU, one wave of each per SIMD: at most 128 VGPRs, no accumulator
    registers, no scratch, and four workgroups' LDS (transform buffer + pass-2 twiddle table + record ring) within the CU's 160 KiB."""
    m = _kernel_resources(tmp_path, "lds_fused4k_kernelE")
    assert m["vgpr_count"] <= 128, m
    assert m["agpr_count"] == 0, m
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, m
    assert 4 * m["group_segment_fixed_size"] <= 163840, m
