"""Guards on the compiled kernels of the batched front-end (csrc/gacq_scan.hip), read from lib/libgacq.so without a GPU: six kernels --
mix, the two generic filter passes, the resampler, the 161-tap forward pass and the fused backward pass + resampler -- with no
scratch, no vector or scalar spills and no accumulator registers."""
from test_build_guards import kernel_metadata
from test_simulate_build import _sgpr_spills


def test_scan_kernels_use_no_scratch_spills_or_accumulator_registers(tmp_path):
    kernels = kernel_metadata(tmp_path)
    sgpr = _sgpr_spills(tmp_path)
    hit = sorted(k for k in kernels if "scan_fe_" in k)
    assert len(hit) == 6, hit
    for fragment in ("scan_fe_mix_kernel", "scan_fe_fir_kernelILi1E", "scan_fe_fir_kernelILi2E", "scan_fe_resample_kernel",
                     "scan_fe_fir1_fixed_kernelILi161E", "scan_fe_back_resample_kernelILi161E"):
        assert sum(fragment in k for k in hit) == 1, (fragment, hit)
    for k in hit:
        m = kernels[k]
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["agpr_count"] == 0, (k, m)
        assert sgpr[k] == 0, (k, sgpr[k])
        assert m["vgpr_count"] <= 64, (k, m)                        # eight waves per SIMD as far as registers go
    # the names the other build guards count kernels by stay clear of this file
    assert not any(w in k for k in hit for w in ("fold", "corr_grid", "tie_recheck", "simulate"))
