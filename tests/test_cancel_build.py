"""Guards on the compiled cancellation kernels (csrc/gacq_cancel.hip), read from lib/libgacq.so without a GPU: the two forms of the
projection kernel (int8 and complex64 input) and the four of the subtraction kernel (input form x output form) keep a lane's run and the
segment it walks in architectural registers -- no scratch, no vector or scalar spills, no accumulator registers, at most 128 VGPRs."""
from test_build_guards import kernel_metadata
from test_simulate_build import _sgpr_spills


def test_cancel_kernels_keep_their_runs_in_registers(tmp_path):
    kernels = kernel_metadata(tmp_path)
    sgpr = _sgpr_spills(tmp_path)
    hit = sorted(k for k in kernels if "cancel_" in k)
    assert sum("cancel_project_kernel" in k for k in hit) == 2 and sum("cancel_subtract_kernel" in k for k in hit) == 4 and len(hit) == 6, hit
    for k in hit:
        m = kernels[k]
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["agpr_count"] == 0, (k, m)
        assert sgpr[k] == 0, (k, sgpr[k])
        assert m["vgpr_count"] <= 128, (k, m)                       # four waves per SIMD at the least
    # the names the other build guards count kernels by stay clear of this file
    assert not any(w in k for k in hit for w in ("fold", "corr_grid", "tie_recheck", "simulate", "scan_fe_", "ingest", "navsym", "viterbi", "psd",
                                                 "squaring", "mit_", "ddc_", "r32_correlate_kernel", "requant_"))
