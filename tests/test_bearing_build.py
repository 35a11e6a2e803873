"""Guards on the compiled bearing kernels (csrc/gacq_bearing.hip), read from lib/libgacq.so without a GPU: exactly the factor kernel and
the spectrum kernel, both with their work in architectural registers -- no scratch (the b of a cell is indexed at compile time), no
vector or scalar spills, no accumulator registers, at most 128 VGPRs."""
from test_build_guards import kernel_metadata
from test_simulate_build import _sgpr_spills


def test_bearing_kernels_keep_their_work_in_registers(tmp_path):
    kernels = kernel_metadata(tmp_path)
    sgpr = _sgpr_spills(tmp_path)
    hit = sorted(k for k in kernels if "bearing_" in k)
    assert sum("bearing_factor_kernel" in k for k in hit) == 1 and sum("bearing_spectrum_kernel" in k for k in hit) == 1 and len(hit) == 2, hit
    for k in hit:
        m = kernels[k]
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["agpr_count"] == 0, (k, m)
        assert sgpr[k] == 0, (k, sgpr[k])
        assert m["vgpr_count"] <= 128, (k, m)                       # four waves per SIMD at the least
    # the names the other build guards count kernels by stay clear of this file
    assert not any(w in k for k in hit for w in ("null_", "stap_", "scene_", "scan_fe_", "fold", "mit_", "ddc_", "ingest", "simulate", "cancel_",
                                                 "requant_", "navsym", "viterbi", "psd", "squaring", "corr_grid", "tie_recheck"))
