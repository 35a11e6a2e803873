"""Guards on the compiled space-time nulling kernels (csrc/gacq_stap.hip), read from lib/libgacq.so without a GPU: the covariance kernel,
the weights kernel and the sixteen forms of the apply kernel (eight tap counts, int8 and complex64) keep their work in architectural
registers -- no scratch, no vector or scalar spills, no accumulator registers (the integer matrix instruction's tiles stay in VGPRs),
at most 128 VGPRs -- and the covariance kernel holds the 16 x 16 x 64 int8 matrix instruction."""
import os
import subprocess

from test_build_guards import LLVM, kernel_metadata
from test_simulate_build import _sgpr_spills


def test_stap_kernels_keep_their_work_in_registers(tmp_path):
    kernels = kernel_metadata(tmp_path)
    sgpr = _sgpr_spills(tmp_path)
    hit = sorted(k for k in kernels if "stap_" in k)
    assert sum("stap_cov_kernel" in k for k in hit) == 1 and sum("stap_weights_kernel" in k for k in hit) == 1, hit
    assert sum("stap_apply_kernel" in k for k in hit) == 16 and len(hit) == 18, hit
    for k in hit:
        m = kernels[k]
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["agpr_count"] == 0, (k, m)
        assert sgpr[k] == 0, (k, sgpr[k])
        assert m["vgpr_count"] <= 128, (k, m)                       # four waves per SIMD at the least
    # the names the other build guards count kernels by stay clear of this file
    assert not any(w in k for k in hit for w in ("fold", "corr_grid", "tie_recheck", "simulate", "scan_fe_", "ingest", "navsym", "viterbi", "psd",
                                                 "squaring", "mit_", "ddc_", "requant_", "cancel_", "null_", "r32_correlate_kernel"))
    # the instruction itself, where the disassembler is there to show it
    objdump = os.path.join(LLVM, "llvm-objdump")
    if os.path.exists(objdump):
        for co in sorted(tmp_path.glob("code*.elf")):
            if co.stat().st_size == 0:
                continue
            text = subprocess.run([objdump, "-d", "--disassemble-symbols=%s" % [k for k in hit if "stap_cov_kernel" in k][0][:-3], str(co)],
                                  check=True, capture_output=True, text=True).stdout
            if "stap_cov_kernel" in text:
                assert "v_mfma_i32_16x16x64_i8" in text, text[:2000]
                break
        else:
            raise AssertionError("stap_cov_kernel is in no code object")
