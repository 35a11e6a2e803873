"""Guards on the compiled navigation-data kernels (csrc/gacq_navbits.hip), read from lib/libgacq.so without a GPU: exactly the two
kernels of the file are there, and each keeps its state in architectural registers -- no scratch, no vector or scalar spills, no
accumulator registers, at most 128 vector registers (the Viterbi wave's path metric, branch signs and survivor word; the symbol
former's overlay and running sums)."""
from test_build_guards import kernel_metadata
from test_simulate_build import _sgpr_spills


def test_navdata_kernels_are_the_two_of_the_file_and_keep_their_state_in_registers(tmp_path):
    kernels = kernel_metadata(tmp_path)
    sgpr = _sgpr_spills(tmp_path)
    hit = sorted(k for k in kernels if "navsym" in k or "viterbi" in k)
    assert len(hit) == 2 and sum("navsym_kernel" in k for k in hit) == 1 and sum("viterbi_kernel" in k for k in hit) == 1, hit
    for k in hit:
        m = kernels[k]
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["agpr_count"] == 0, (k, m)
        assert sgpr[k] == 0, (k, sgpr[k])
        assert m["vgpr_count"] <= 128, (k, m)
    # the names the other build guards count kernels by stay clear of this file
    assert not any(w in k for k in hit for w in ("fold", "corr_grid", "tie_recheck", "simulate", "scan_fe_", "ingest", "r32_correlate_kernel"))
