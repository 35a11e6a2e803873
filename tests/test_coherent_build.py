"""Guards on the compiled coherent-fold kernels (csrc/gacq_cohfold.hip), read from lib/libgacq.so without a GPU: the accumulator tile
must live in architectural registers -- no scratch, no spills, no accumulator registers -- in every instantiation (tile of 8, 16, 24 or 32
hypotheses, one or two samples per lane, complex64 or complex128 input)."""
from test_build_guards import kernel_metadata


def test_fold_kernels_keep_their_tile_in_registers(tmp_path):
    kernels = kernel_metadata(tmp_path)
    hit = sorted(k for k in kernels if "fold" in k)
    assert len(hit) == 16 and all("cohfold_kernel" in k for k in hit), hit
    for k in hit:
        m = kernels[k]
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["agpr_count"] == 0, (k, m)
        assert m.get("sgpr_spill_count", 0) == 0 and m["vgpr_count"] <= 168, (k, m)      # 168: three waves per SIMD
