"""Guards on the compiled device code of lib/libgacq.so (no GPU needed): the code objects are pulled out of the library's .hip_fatbin
section once per run and their kernel metadata is read with the ROCm LLVM tools.

* Kernels that carry the LDS-access separators (GACQ_UNPAIR, csrc/gacq_cplx.h: an empty asm statement between LDS accesses) must not
  use accumulator registers: this toolchain produced wrong rows in a kernel that spilled VGPRs to AGPRs around such statements
  (DESIGN 5.2).  The complex128 re-evaluation kernels (gacq_tiesafe.hip) are the only AGPR users and are compiled without separators.
* The hot kernels must not spill to scratch (a spill there is a performance cliff that no parity test would notice).
* Every kernel family of FAMILIES is exactly the kernels its source file instantiates and keeps its work in architectural registers:
  no scratch, no vector or scalar spills, no accumulator registers, and few enough VGPRs for the occupancy it was written for."""
import collections
import os
import re
import subprocess
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "gnss-dsp-tools_amd", "lib", "libgacq.so")
LLVM = "/opt/rocm/lib/llvm/bin"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
FIELDS = ("agpr_count", "vgpr_count", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")


def kernel_metadata(tmp_path):
    """symbol ("<mangled name>.kd") -> FIELDS of every gfx950 kernel in the library; the code objects stay in tmp_path as code<n>.elf"""
    tools = [os.path.join(LLVM, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")]
    if not os.path.exists(LIB) or not all(os.path.exists(t) for t in tools):
        pytest.skip("library or ROCm LLVM tools not present")
    fat = tmp_path / "fat.bin"
    subprocess.run([tools[0], "--dump-section", ".hip_fatbin=%s" % fat, LIB], check=True)
    blob = fat.read_bytes()
    starts = [m.start() for m in re.finditer(re.escape(MAGIC), blob)]
    kernels = {}
    for n, (a, b) in enumerate(zip(starts, starts[1:] + [len(blob)])):
        part = tmp_path / ("bundle%d.bin" % n)
        part.write_bytes(blob[a:b])
        co = tmp_path / ("code%d.elf" % n)
        subprocess.run([tools[1], "--unbundle", "--type=o", "--input=%s" % part, "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=%s" % co],
                       check=True, capture_output=True)
        if not co.exists() or co.stat().st_size == 0:
            continue
        notes = subprocess.run([tools[2], "--notes", str(co)], check=True, capture_output=True, text=True).stdout
        for block in notes.split("- .agpr_count:")[1:]:                     # one block per kernel; .symbol is "<mangled name>.kd"
            fields = {"agpr_count": block.split()[0], "sgpr_spill_count": 0}  # the note leaves a zero scalar spill count out
            fields.update(re.findall(r"^\s+\.(symbol|%s):\s+(\S+)\s*$" % "|".join(FIELDS[1:]), block, flags=re.M))
            kernels[fields["symbol"]] = {k: int(fields[k]) for k in FIELDS}
    return kernels


@pytest.fixture(scope="module")
def library(tmp_path_factory):
    """The library taken apart once for the whole module: .kernels is kernel_metadata(), .code_objects the unbundled ELF files."""
    tmp = tmp_path_factory.mktemp("libgacq")
    kernels = kernel_metadata(tmp)
    return types.SimpleNamespace(kernels=kernels, code_objects=sorted(p for p in tmp.glob("code*.elf") if p.stat().st_size))


def test_kernels_with_lds_separators_use_no_accumulator_registers_and_hot_kernels_do_not_spill(library):
    kernels = library.kernels
    assert len(kernels) > 40, sorted(kernels)
    with_agprs = sorted(k for k, m in kernels.items() if m["agpr_count"])
    assert with_agprs and all("tie_recheck" in k for k in with_agprs), with_agprs
    for fragment in ("lds_fused4k_kernelE", "lds16k_correlate_kernelILb0", "r32_correlate_kernelILb0", "r32_fused_kernelILb0", "fused4k_c128_kernel", "lds_inner_correlate_kernel",
                     "lds_correlate_kernelILb", "pfa_inner_corr_kernelILi1980ELi3E", "pfa_inner_corr_kernelILi990ELi2E",
                     "pfa_outer_inverse_kernelILi1980ELi0E", "pfa_outer_inverse_kernelILi990ELi2E", "pfa_outer_inverse_mfma_kernelILi1980ELi0E"):
        hit = [k for k in kernels if fragment in k]
        assert hit, fragment
        for k in hit:
            if fragment.startswith("r32_correlate_kernel"):
                # 256 registers: the record pointer (two dwords) is stored before the item loop and reloaded in the per-unit tail; nothing
                # is spilled inside the row loop (checked in the ISA: both reloads sit at loop depth 2, once per B rows)
                assert kernels[k]["private_segment_fixed_size"] <= 16 and kernels[k]["vgpr_spill_count"] <= 2, (k, kernels[k])
                continue
            assert kernels[k]["private_segment_fixed_size"] == 0 and kernels[k]["vgpr_spill_count"] == 0, (k, kernels[k])


# One row per kernel family.  To guard a new family add its row here and nothing else: the parametrized test below picks it up under
# the family's name, and the disjointness test takes its words into the set no other family's kernel may match.
#   words     a kernel belongs to the family when its mangled name contains one of them
#   counts    name fragment -> exact number of the family's kernels that contain it
#   total     exact number of kernels in the family (None: at least one)
#   vgprs     most vector registers a kernel may use: 64, 128, 168 and 256 are eight, four, three and two waves per SIMD
#   sgpr      most scalar spills a kernel may have (None: not checked)
#   contains  (name fragment, instruction): the one kernel with that fragment must hold the instruction
Family = collections.namedtuple("Family", "id source words counts total vgprs sgpr contains", defaults=(None,))
MFMA_I8 = "v_mfma_i32_16x16x64_i8"
FAMILIES = (
    # the eight samples a lane owns and the state of the satellite it walks, complex64 and int8 output
    Family("simulate", "gacq_simulate.hip", ("simulate",), {"simulate_kernel": 2}, 2, 128, 0),
    # the accumulator tile: 8, 16, 24 or 32 hypotheses, one or two samples per lane, complex64 or complex128 input
    Family("cohfold", "gacq_cohfold.hip", ("fold",), {"cohfold_kernel": 16}, 16, 168, 0),
    # the accumulator tile of the correlation grid, two workgroups per CU
    Family("corrgrid", "gacq_corrgrid.hip", ("corr_grid",), {}, None, 256, None),
    # mix, the two generic filter passes, the resampler, the 161-tap forward pass and the fused backward pass + resampler
    Family("scan", "gacq_scan.hip", ("scan_fe_",),
           {"scan_fe_mix_kernel": 1, "scan_fe_fir_kernelILi1E": 1, "scan_fe_fir_kernelILi2E": 1, "scan_fe_resample_kernel": 1,
            "scan_fe_fir1_fixed_kernelILi161E": 1, "scan_fe_back_resample_kernelILi161E": 1}, 6, 64, 0),
    # the values a lane unpacks, its window of odd-index inputs and its eight outputs: seven containers x two output forms (I/Q), five x two (real IF)
    Family("ingest", "gacq_ingest.hip", ("ingest",), {"ingest_iq_kernel": 14, "ingest_real_kernel": 10}, 24, 128, 0),
    # the Viterbi wave's path metric, branch signs and survivor word; the symbol former's overlay and running sums
    Family("navbits", "gacq_navbits.hip", ("navsym", "viterbi"), {"navsym_kernel": 1, "viterbi_kernel": 1}, 2, 128, 0),
    # a frame's halves and the kept overlap: seven lengths of the excision kernel, two input x two output forms of the blank-only kernel
    Family("mitigate", "gacq_mitigate.hip", ("mit_",), {"mit_excise_kernel": 7, "mit_blank_kernel": 4}, 11, 128, 0),
    # a lane's eight accumulators and sliding window, two output forms
    Family("ddc", "gacq_ddc.hip", ("ddc_",), {"ddc_kernel": 2}, 2, 128, 0),
    # a lane's run: two block-power kernels, seven output forms x two input widths of the quantize kernel
    Family("requant", "gacq_requant.hip", ("requant_",), {"requant_power_kernel": 2, "requant_quantize_kernel": 14}, 16, 128, 0),
    # a lane's run and the segment it walks: int8 and complex64 projection, input form x output form subtraction
    Family("cancel", "gacq_cancel.hip", ("cancel_",), {"cancel_project_kernel": 2, "cancel_subtract_kernel": 4}, 6, 128, 0),
    # the 2 M + 1 fp64 sums of a lane: <bool INC, int M>, int8 and complex64 input for 1, 2, 4 and 8 antennas
    Family("aprompt", "gacq_aprompt.hip", ("aprompt_",),
           {"aprompt_project_kernel": 8, **{"aprompt_project_kernelI%sLi%dEE" % (inc, m): 1 for inc in ("Lb0E", "Lb1E") for m in (1, 2, 4, 8)}}, 8, 128, 0),
    # covariance, weights, int8 and complex64 apply; the integer matrix instruction's tile stays in VGPRs
    Family("null", "gacq_null.hip", ("null_",), {"null_cov_kernel": 1, "null_weights_kernel": 1, "null_apply_kernel": 2}, 4, 128, 0,
           ("null_cov_kernel", MFMA_I8)),
    # covariance, weights, eight tap counts x int8 and complex64 apply; the integer matrix instruction's tiles stay in VGPRs
    Family("stap", "gacq_stap.hip", ("stap_",), {"stap_cov_kernel": 1, "stap_weights_kernel": 1, "stap_apply_kernel": 16}, 18, 128, 0,
           ("stap_cov_kernel", MFMA_I8)),
    # the accumulators and the state of the source a lane walks: antenna counts 1..8 x output type
    Family("scene", "gacq_scene.hip", ("scene_",), {"scene_kernel": 16}, 16, 128, 0),
    # the factor kernel and the spectrum kernel; the b of a cell is indexed at compile time
    Family("bearing", "gacq_bearing.hip", ("bearing_",), {"bearing_factor_kernel": 1, "bearing_spectrum_kernel": 1}, 2, 128, 0),
    # the weights kernel and the two forms of the apply kernel; the covariance kernel is nulling's own (cross-check below)
    Family("beams", "gacq_beams.hip", ("beams_",), {"beams_weights_kernel": 1, "beams_apply_kernel": 2}, 3, 128, 0),
)
# words that select kernels with no row of their own, which no family's kernel may match either
UNOWNED_WORDS = ("tie_recheck", "r32_correlate_kernel", "psd", "squaring")


def owned(family, kernels):
    return sorted(k for k in kernels if any(w in k for w in family.words))


def assert_holds_instruction(library, symbol, instruction):
    """The instruction itself, where the disassembler is there to show it: only that one symbol is disassembled."""
    objdump = os.path.join(LLVM, "llvm-objdump")
    if not os.path.exists(objdump):
        return
    name = symbol[:-3]                                              # without ".kd"
    for co in library.code_objects:
        text = subprocess.run([objdump, "-d", "--disassemble-symbols=%s" % name, str(co)], check=True, capture_output=True, text=True).stdout
        if name in text:
            assert instruction in text, text[:2000]
            return
    raise AssertionError("%s is in no code object" % name)


def check_family(family, library):
    kernels = library.kernels
    hit = owned(family, kernels)
    assert hit if family.total is None else len(hit) == family.total, (family.source, hit)
    for fragment, count in family.counts.items():
        assert sum(fragment in k for k in hit) == count, (family.source, fragment, hit)
    for k in hit:
        m = kernels[k]
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["agpr_count"] == 0, (k, m)
        assert family.sgpr is None or m["sgpr_spill_count"] <= family.sgpr, (k, m)
        assert m["vgpr_count"] <= family.vgprs, (k, m)
    if family.contains:
        fragment, instruction = family.contains
        assert_holds_instruction(library, [k for k in hit if fragment in k][0], instruction)


@pytest.mark.parametrize("family", FAMILIES, ids=[f.id for f in FAMILIES])
def test_family_is_the_kernels_of_its_file_and_keeps_its_work_in_registers(library, family):
    check_family(family, library)


def test_no_kernel_is_counted_by_two_guards(library):
    words = {w for f in FAMILIES for w in f.words} | set(UNOWNED_WORDS)
    for family in FAMILIES:
        for k in owned(family, library.kernels):
            other = sorted(w for w in words - set(family.words) if w in k)
            assert not other, (family.id, k, other)


def test_the_library_holds_one_single_tap_covariance_kernel_and_it_is_nullings(library):
    """gacq_beams.hip and gacq_aprompt.hip launch gacq_null.hip's covariance kernel: the library holds no second copy of it."""
    cov = sorted(k for k in library.kernels if "cov_kernel" in k and "stap_" not in k)
    assert len(cov) == 1 and "null_cov_kernel" in cov[0], cov


@pytest.mark.parametrize("family,fragment,change", [("scan", "scan_fe_mix_kernel", {"vgpr_count": 65}),
                                                    ("cohfold", "cohfold_kernel", {"sgpr_spill_count": 1}),
                                                    ("stap", "stap_apply_kernel", None)], ids=["vgpr-cap", "sgpr-spill", "count"])
def test_a_guard_fails_with_the_kernels_name_when_one_field_is_off(library, family, fragment, change):
    """check_family against metadata with one kernel's field altered (a cap exceeded, a spill of 1) or one kernel gone (a count off by one)"""
    kernels = dict(library.kernels)
    victim = [k for k in sorted(kernels) if fragment in k][0]
    if change:
        kernels[victim] = dict(kernels[victim], **change)
    else:
        del kernels[victim]
    with pytest.raises(AssertionError, match=re.escape(fragment)):
        check_family([f for f in FAMILIES if f.id == family][0], types.SimpleNamespace(kernels=kernels, code_objects=library.code_objects))
