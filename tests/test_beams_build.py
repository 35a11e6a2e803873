"""Guards on the compiled beams kernels (csrc/gacq_beams.hip), read from lib/libgacq.so without a GPU: the weights kernel and the two forms
of the apply kernel keep their work in architectural registers -- no scratch, no vector or scalar spills, no accumulator registers, at
most 128 VGPRs -- and the covariance kernel is nulling's own: the library holds no second copy of it."""
from test_build_guards import kernel_metadata
from test_simulate_build import _sgpr_spills


def test_beams_kernels_keep_their_work_in_registers(tmp_path):
    kernels = kernel_metadata(tmp_path)
    sgpr = _sgpr_spills(tmp_path)
    hit = sorted(k for k in kernels if "beams_" in k)
    assert sum("beams_weights_kernel" in k for k in hit) == 1 and sum("beams_apply_kernel" in k for k in hit) == 2 and len(hit) == 3, hit
    for k in hit:
        m = kernels[k]
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["agpr_count"] == 0, (k, m)
        assert sgpr[k] == 0, (k, sgpr[k])
        assert m["vgpr_count"] <= 128, (k, m)                       # four waves per SIMD at the least
    # one covariance kernel in the whole library, the one gacq_null.hip compiles
    assert sum("cov_kernel" in k and "stap_" not in k for k in kernels) == 1 and sum("null_cov_kernel" in k for k in kernels) == 1
    # the names the other build guards count kernels by stay clear of this file
    assert not any(w in k for k in hit for w in ("null_", "stap_", "scene_", "bearing_", "aprompt_", "fold", "corr_grid", "tie_recheck", "simulate",
                                                 "scan_fe_", "ingest", "navsym", "viterbi", "psd", "squaring", "mit_", "ddc_", "requant_", "cancel_",
                                                 "r32_correlate_kernel"))
