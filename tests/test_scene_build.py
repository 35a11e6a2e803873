"""Guards on the compiled scene kernels (csrc/gacq_scene.hip), read from lib/libgacq.so without a GPU: sixteen instantiations, one per
antenna count 1..8 and output type, each with its accumulators and the state of the source it walks in architectural registers -- no
scratch, no vector or scalar spills, no accumulator registers, at most 128 VGPRs -- the rule of test_simulate_build.py."""
from test_build_guards import kernel_metadata
from test_simulate_build import _sgpr_spills

# the words the other build guards count kernels by
GUARD_WORDS = ("simulate", "fold", "corr_grid", "tie_recheck", "scan_fe_", "ingest", "navsym", "viterbi", "psd", "squaring", "mit_", "ddc_", "requant_",
               "cancel_", "null_", "stap_", "r32_correlate_kernel")


def test_scene_kernels_keep_their_samples_in_registers(tmp_path):
    kernels = kernel_metadata(tmp_path)
    sgpr = _sgpr_spills(tmp_path)
    hit = sorted(k for k in kernels if "scene_" in k)
    assert len(hit) == 16 and all("scene_kernel" in k for k in hit), hit
    for k in hit:
        m = kernels[k]
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["agpr_count"] == 0, (k, m)
        assert sgpr[k] == 0, (k, sgpr[k])
        assert m["vgpr_count"] <= 128, (k, m)                       # four waves per SIMD at the least
    assert not any(w in k for k in hit for w in GUARD_WORDS), hit
