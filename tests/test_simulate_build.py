"""Guards on the compiled recording-synthesis kernels (csrc/gacq_simulate.hip), read from lib/libgacq.so without a GPU: the eight
samples a lane owns and the state of the satellite it walks must live in architectural registers -- no scratch, no vector or scalar
spills, no accumulator registers -- in both instantiations (complex64 and int8 output)."""
import os
import re
import subprocess

from test_build_guards import LLVM, kernel_metadata


def _sgpr_spills(tmp_path):
    """symbol -> .sgpr_spill_count from the notes of the code objects kernel_metadata() left in tmp_path"""
    out = {}
    for co in sorted(tmp_path.glob("code*.elf")):
        if co.stat().st_size == 0:
            continue
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", str(co)], check=True, capture_output=True, text=True).stdout
        for block in notes.split("- .agpr_count:")[1:]:
            f = dict(re.findall(r"^\s+\.(symbol|sgpr_spill_count):\s+(\S+)\s*$", block, flags=re.M))
            out[f["symbol"]] = int(f.get("sgpr_spill_count", 0))
    return out


def test_simulate_kernels_keep_their_samples_in_registers(tmp_path):
    kernels = kernel_metadata(tmp_path)
    sgpr = _sgpr_spills(tmp_path)
    hit = sorted(k for k in kernels if "simulate" in k)
    assert len(hit) == 2 and all("simulate_kernel" in k for k in hit), hit
    for k in hit:
        m = kernels[k]
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["agpr_count"] == 0, (k, m)
        assert sgpr[k] == 0, (k, sgpr[k])
        assert m["vgpr_count"] <= 128, (k, m)                       # four waves per SIMD at the least
    # the names the other build guards count kernels by stay clear of this file
    assert not any(w in k for k in hit for w in ("fold", "corr_grid", "tie_recheck"))
