"""Guards on the compiled ingest kernels (csrc/gacq_ingest.hip), read from lib/libgacq.so without a GPU: the values a lane unpacks,
its window of odd-index inputs and its eight outputs must live in architectural registers -- no scratch, no vector or scalar spills,
no accumulator registers -- in every instantiation: seven containers times two output forms of the I/Q kernel, five times two of
the real-IF kernel."""
from test_build_guards import kernel_metadata
from test_simulate_build import _sgpr_spills


def test_ingest_kernels_keep_their_samples_in_registers(tmp_path):
    kernels = kernel_metadata(tmp_path)
    sgpr = _sgpr_spills(tmp_path)
    hit = sorted(k for k in kernels if "ingest" in k)
    assert sum("ingest_iq_kernel" in k for k in hit) == 14 and sum("ingest_real_kernel" in k for k in hit) == 10 and len(hit) == 24, hit
    for k in hit:
        m = kernels[k]
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["agpr_count"] == 0, (k, m)
        assert sgpr[k] == 0, (k, sgpr[k])
        assert m["vgpr_count"] <= 128, (k, m)                       # four waves per SIMD at the least
    # the names the other build guards count kernels by stay clear of this file
    assert not any(w in k for k in hit for w in ("fold", "corr_grid", "tie_recheck", "simulate", "scan_fe_"))
