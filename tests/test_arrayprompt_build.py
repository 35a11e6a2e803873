"""Guards on the compiled array-prompt kernels (csrc/gacq_aprompt.hip), read from lib/libgacq.so without a GPU: exactly the eight forms
of aprompt_project_kernel -- int8 and complex64 input for 1, 2, 4 and 8 antennas; another antenna count runs the next larger form --
with the 2 M + 1 fp64 sums of a lane in architectural registers: no scratch, no vector or scalar spills, no accumulator registers, at
most 128 VGPRs.  The cancellation kernels, which now share the replica through csrc/gacq_cancelcore.h, are still their six."""
from test_build_guards import kernel_metadata
from test_simulate_build import _sgpr_spills

OTHERS = ("cancel_", "null_", "stap_", "scene_", "bearing_", "fold", "mit_", "ddc_", "ingest", "simulate", "requant_", "navsym", "viterbi", "psd",
          "squaring", "corr_grid", "scan_fe_", "tie_recheck")


def test_aprompt_kernels_keep_their_sums_in_registers(tmp_path):
    kernels = kernel_metadata(tmp_path)
    sgpr = _sgpr_spills(tmp_path)
    hit = sorted(k for k in kernels if "aprompt_" in k)
    assert len(hit) == 8 and all("aprompt_project_kernel" in k for k in hit), hit
    for inc in ("Lb0E", "Lb1E"):                                    # the mangled template arguments: <bool INC, int M>
        for m in (1, 2, 4, 8):
            assert sum(("aprompt_project_kernelI%sLi%dEE" % (inc, m)) in k for k in hit) == 1, (inc, m, hit)
    for k in hit:
        m = kernels[k]
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["agpr_count"] == 0, (k, m)
        assert sgpr[k] == 0, (k, sgpr[k])
        assert m["vgpr_count"] <= 128, (k, m)                       # four waves per SIMD at the least
    # the names the other build guards count kernels by stay clear of this file
    assert not any(w in k for k in hit for w in OTHERS)
    # ... and the cancellation kernels are the six they were
    can = sorted(k for k in kernels if "cancel_" in k)
    assert sum("cancel_project_kernel" in k for k in can) == 2 and sum("cancel_subtract_kernel" in k for k in can) == 4 and len(can) == 6, can
