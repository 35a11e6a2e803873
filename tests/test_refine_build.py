"""Guards on the compiled correlation-grid kernel (csrc/gacq_corrgrid.hip), read from lib/libgacq.so without a GPU: its accumulator
tile must live in architectural registers -- no scratch, no spills, no accumulator registers."""
from test_build_guards import kernel_metadata


def test_corr_grid_kernels_keep_their_tile_in_registers(tmp_path):
    kernels = kernel_metadata(tmp_path)
    hit = sorted(k for k in kernels if "corr_grid" in k)
    assert hit, sorted(kernels)
    for k in hit:
        m = kernels[k]
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["agpr_count"] == 0, (k, m)
        assert m["vgpr_count"] <= 256, (k, m)
