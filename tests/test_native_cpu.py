"""CPU: host-side parts of libgacq.so -- symbol export, PRN generators (bit-exact), replica sampler,
error paths that need no GPU -- and the host logic of the Python mirror."""
import ctypes
import hashlib
import os
import re

import numpy as np
import pytest

from gnss_dsp_tools_amd import _cabi as cabi
from gnss_dsp_tools_amd import _native as nat
from gnss_dsp_tools_amd import acquire, codes, signals
from oracle import acq_oracle, codes_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    """Every function declared in include/gacq.h is exported by the built .so and bound in _native.py."""
    hdr = open(os.path.join(ROOT, "include", "gacq.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(gacq_[a-z_0-9]+)\s*\(", hdr))
    assert len(declared) >= 129
    assert declared == set(nat.SYMBOLS), declared ^ set(nat.SYMBOLS)
    lib = ctypes.CDLL(nat.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name


def _gcc(tmp_path, name, source, run=False):
    """Compile a C text that includes gacq.h (syntax only, or to a program whose output comes back)"""
    import subprocess
    src = tmp_path / (name + ".c")
    src.write_text(source)
    cmd = ["gcc", "-std=gnu99", "-I", os.path.join(ROOT, "include"), str(src)] + (["-o", str(tmp_path / name)] if run else ["-fsyntax-only"])
    build = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert build.returncode == 0, build.stderr[-4000:]
    if run:
        out = subprocess.run([str(tmp_path / name)], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr[-2000:]
        return out.stdout


def test_parsed_prototypes_are_the_compilers(tmp_path):
    """Every prototype as _cabi read it (return type and parameter types in order, as normalised C text) is compatible with the
    function gcc sees in the header: a dropped, reordered or misread parameter fails the compile.  The ctypes side follows from that
    text by the pointer rule, restated here."""
    assert list(cabi.signatures) == list(cabi.prototypes) == list(nat.SYMBOLS) and len(cabi.signatures) >= 129
    lines = ['#include "gacq.h"']
    for name, (ret, params) in cabi.signatures.items():
        lines.append('_Static_assert(__builtin_types_compatible_p(__typeof__(&%s), %s (*)(%s)), "%s");' % (name, ret, ", ".join(params) or "void", name))
    _gcc(tmp_path, "prototypes", "\n".join(lines) + "\n")

    def bound(ctype):
        if ctype == "void":
            return None
        if ctype.endswith("*"):
            return ctypes.c_char_p if ctype == "const char*" else ctypes.c_void_p
        return cabi.SCALARS[ctype]
    for name, (ret, params) in cabi.signatures.items():
        assert nat.SYMBOLS[name] == (bound(ret), [bound(p) for p in params]), name
        fn = getattr(nat.lib, name)
        assert fn.restype is bound(ret) and list(fn.argtypes) == [bound(p) for p in params], name
    assert cabi.signatures["gacq_get_tie_stats"] == ("int", ["gacq_ctx*", "long long*"])           # the array parameter, decayed
    assert cabi.signatures["gacq_code_name"] == ("const char*", ["int"]) and cabi.signatures["gacq_device_count"] == ("int", [])


def test_scalar_type_table_is_the_compilers(tmp_path):
    """Size, signedness and kind (integer or floating) of every C scalar name of _cabi.SCALARS against the ctypes type it maps to"""
    body = "".join('  printf("%s|%%d %%d %%d\\n", (int)sizeof(%s), (%s)-1 < 0, (%s)0.5 != 0);\n' % (t, t, t, t) for t in cabi.SCALARS)
    out = _gcc(tmp_path, "scalars", '#include <stdio.h>\n#include "gacq.h"\nint main(void) {\n' + body + "  return 0;\n}\n", run=True)
    seen = {}
    for line in out.splitlines():
        name, _, nums = line.partition("|")
        seen[name] = tuple(int(v) for v in nums.split())
    assert set(seen) == set(cabi.SCALARS)
    for name, ct in cabi.SCALARS.items():
        assert seen[name] == (ctypes.sizeof(ct), int(ct(-1).value < 0), int(ct(0.5).value != 0) if ct in (ctypes.c_float, ctypes.c_double) else 0), name


def test_every_struct_layout_is_the_compilers(tmp_path):
    """sizeof of every struct of the header and offsetof / sizeof of every member against the derived ctypes classes: all fields"""
    assert len(cabi.structs) >= 20
    body = []
    for sname, cls in cabi.structs.items():
        body.append('  printf("%s . %%d\\n", (int)sizeof(%s));\n' % (sname, sname))
        for fname, _ in cls._fields_:
            body.append('  printf("%s %s %%d %%d\\n", (int)offsetof(%s, %s), (int)sizeof(((%s*)0)->%s));\n' % (sname, fname, sname, fname, sname, fname))
    out = _gcc(tmp_path, "layouts", '#include <stdio.h>\n#include <stddef.h>\n#include "gacq.h"\nint main(void) {\n' + "".join(body) + "  return 0;\n}\n", run=True)
    fields = 0
    for line in out.splitlines():
        sname, fname, *nums = line.split()
        cls = cabi.structs[sname]
        if fname == ".":
            assert ctypes.sizeof(cls) == int(nums[0]), sname
        else:
            f = getattr(cls, fname)
            assert (f.offset, f.size) == (int(nums[0]), int(nums[1])), (sname, fname)
            fields += 1
    assert fields == sum(len(cls._fields_) for cls in cabi.structs.values()) >= 180
    # the shapes the rule for members names: arrays of arrays, a const char*, another pointer
    beams, spec = cabi.structs["gacq_beams_cfg"], cabi.structs["gacq_grid_spec"]
    assert dict(beams._fields_)["c"] is (ctypes.c_double * 16) * 16
    assert dict(spec._fields_)["code"] is ctypes.c_char_p and dict(spec._fields_)["offsets"] is ctypes.c_void_p
    assert nat.struct("gacq_result") is nat.Result is cabi.structs["gacq_result"]


@pytest.mark.parametrize("text, quoted", [
    ("int gacq_f(gacq_nope* p);", "gacq_nope"),                                         # an unknown type
    ("int gacq_f(short n);", "short"),
    ("int gacq_f(int n, void (*done)(int));", "gacq_f"),                                 # a function pointer
    ("typedef struct gacq_s { int a; void (*done)(int); } gacq_s;", "done"),
    ("typedef struct gacq_s { int a : 3; int b; } gacq_s;", "int a : 3"),                 # a bit-field
    ("typedef struct gacq_s { int a; union { int b; float c; } u; } gacq_s;", "union"),
    ("typedef union gacq_u { int b; float c; } gacq_u;", "gacq_u"),
    ("typedef struct gacq_s { int a; } gacq_s;\nint gacq_f(gacq_s by_value);", "by_value"),
    ("int gacq_f(int);", "gacq_f"),                                                      # a parameter without a name
    ("#define GACQ_X (1 << 3)", "GACQ_X"),
    ("#if 0\nint gacq_f(void);\n#endif", "#if 0"),
])
def test_parser_refuses_what_it_does_not_read(text, quoted):
    with pytest.raises(cabi.CHeaderError) as e:
        cabi.load(text)
    assert quoted in str(e.value), str(e.value)


def test_parser_reads_the_subset():
    protos, sigs, structs, consts = cabi.load("""
        #ifndef X_H
        #define X_H
        #ifdef __cplusplus
        extern "C" {
        #endif
        /* a comment with int gacq_not(void); in it */
        #define GACQ_A (-3)
        #define GACQ_B 7   // seven
        typedef struct gacq_h gacq_h;
        typedef struct gacq_s { const char* name; double a, b[2]; uint8_t m[2][3]; gacq_h* h; } gacq_s;
        const char* gacq_f(const gacq_s* s, const void* const* rows, unsigned long long seed, long long out[4], size_t n);
        void gacq_g(void);
        #ifdef __cplusplus
        }
        #endif
        #endif
    """)
    assert consts == {"GACQ_A": -3, "GACQ_B": 7}
    assert sigs == {"gacq_f": ("const char*", ["const gacq_s*", "const void* const*", "unsigned long long", "long long*", "size_t"]), "gacq_g": ("void", [])}
    assert protos == {"gacq_f": (ctypes.c_char_p, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_ulonglong, ctypes.c_void_p, ctypes.c_size_t]), "gacq_g": (None, [])}
    assert structs["gacq_s"]._fields_ == [("name", ctypes.c_char_p), ("a", ctypes.c_double), ("b", ctypes.c_double * 2), ("m", (ctypes.c_uint8 * 3) * 2),
                                          ("h", ctypes.c_void_p)]


def test_a_package_without_its_header_says_so(tmp_path):
    """_cabi.py looks for <package>/../include/gacq.h: a copy of the module in a tree without one fails to import, plainly"""
    import importlib.util
    import shutil
    (tmp_path / "pkg").mkdir()
    shutil.copy(cabi.__file__, tmp_path / "pkg" / "_cabi.py")
    spec = importlib.util.spec_from_file_location("_cabi_without_header", tmp_path / "pkg" / "_cabi.py")
    with pytest.raises(ImportError, match="gacq.h is missing"):
        spec.loader.exec_module(importlib.util.module_from_spec(spec))


def test_constants_and_dtypes_come_from_the_header():
    from gnss_dsp_tools_amd import cancel, ingest, longtrack, navdata, trackloop
    assert len(cabi.constants) >= 45 and nat.CONSTANTS is cabi.constants
    assert nat.ERRORS[0] == "GACQ_OK" and nat.ERRORS[-9] == "GACQ_ERR_UNSUPPORTED" and len(nat.ERRORS) == 10
    assert (ingest.S8, ingest.U8, ingest.S16, ingest.F32, ingest.PACKED) == (0, 1, 2, 3, 4) and navdata.MAX_R == 20
    assert sorted(trackloop.STATUS) == [0, 1, 2] and sorted(longtrack.STATUS) == [0, 1, 2, 3]
    for dt, sname in [(acquire.PEAK_DTYPE, "gacq_peak"), (acquire.RESULT_DTYPE, "gacq_result"), (cancel.SEG_DTYPE, "gacq_cancel_seg"),
                      (trackloop.RECORD_DTYPE, "gacq_track_record"), (trackloop.STATE_DTYPE, "gacq_track_chstate")]:
        cls = cabi.structs[sname]
        assert dt.names == tuple(f for f, _ in cls._fields_) and dt.itemsize == ctypes.sizeof(cls), sname
        assert [dt.fields[f][1] for f in dt.names] == [getattr(cls, f).offset for f in dt.names], sname
        assert [dt.fields[f][0] for f in dt.names] == [np.dtype(t) for _, t in cls._fields_], sname


def test_struct_layouts_match_header():
    assert ctypes.sizeof(nat.Peak) == 16
    assert ctypes.sizeof(nat.Result) == 32
    assert ctypes.sizeof(nat.SigDesc) == 32
    assert acquire.PEAK_DTYPE.itemsize == 16


def test_native_chips_bit_exact_all_prns(golden_chips):
    """SHA-256 of every PRN of every code family equals the reference's."""
    assert sorted(golden_chips) == sorted(codes.names())
    total = 0
    for code, fam in golden_chips.items():
        assert codes.code_length(code) == fam["code_length"]
        assert codes.chip_rate(code) == fam["chip_rate"]
        assert sorted(map(str, codes.prns(code)), key=int) == sorted(fam["prns"], key=int)
        for prn, g in fam["prns"].items():
            c = codes.chips(code, int(prn))
            assert hashlib.sha256(c.tobytes()).hexdigest() == g["sha256"], (code, prn)
            assert "".join(map(str, c[-24:])) == g["tail"]
            total += 1
    assert total == 2239 + 115 + 1        # + L2CL PRNs + the GLONASS P code


def test_native_chips_equal_oracle_chips():
    for code, prn in [("gps.ca", 17), ("gps.l5i", 101), ("galileo.e1b", 50), ("beidou.b1i", 40), ("beidou.b2ad", 63),
                      ("glonass.ca", 0), ("gps.l1cd", 210), ("beidou.b1cp", 1), ("glonass.l3ocp", 5), ("xona.x5p", 0)]:
        np.testing.assert_array_equal(codes.chips(code, prn), codes_oracle.chips(code, prn))


@pytest.mark.parametrize("code,n,boc", [("gps.ca", 4096, False), ("galileo.e1b", 32768, True), ("gps.l5i", 30690, False),
                                         ("beidou.b1i", 8192, False), ("glonass.ca", 16384, False), ("gps.l1cd", 81920, True),
                                         ("galileo.e6b", 15345, False), ("gps.l2cm", 81920, False)])
def test_replica_sampler_matches_oracle(code, n, boc):
    prn = codes.prns(code)[3 % len(codes.prns(code))]
    chips = codes_oracle.chips(code, prn)
    want = acq_oracle.sample_code(chips, 0, 0, float(len(chips)) / n, n)
    if boc:
        want = want * acq_oracle.boc11(0, 0, float(len(chips)) / n, n)
    got = codes.replica(code, prn, n, boc)
    np.testing.assert_array_equal(got.astype(np.float64), want)


def test_code_errors():
    assert nat.lib.gacq_code_length(b"gps.nope") == -2
    buf = (ctypes.c_uint8 * 2048)()
    assert nat.lib.gacq_code_chips(b"gps.ca", 999, buf, 2048) == -3
    assert nat.lib.gacq_code_chips(b"gps.ca", 1, buf, 10) == -1
    with pytest.raises(nat.GacqError):
        codes.chips("galileo.e1b", 51)


def test_create_without_gpu_fails_loudly():
    if nat.lib.gacq_device_count() > 0:
        pytest.skip("GPU present")
    h = ctypes.c_void_p()
    assert nat.lib.gacq_create(0, ctypes.byref(h)) == -7
    assert b"no HIP device" in nat.lib.gacq_last_error(None)
    with pytest.raises(nat.GacqError):
        acquire.Engine(0)


def test_signal_table_agrees_with_oracle_variants():
    assert set(signals.SIGNALS) == set(acq_oracle.VARIANTS)
    for name, s in signals.SIGNALS.items():
        code, fs, n, pad, boc, norm, fold, blocks, bias = acq_oracle.VARIANTS[name]
        assert (s.code, s.fs, s.n, s.pad, s.boc, s.normalised, s.fold, s.bias_hz) == (code, fs, n, pad, boc, norm, fold, bias), name
        for ms in (0, 1, 4, 8, 10, 20, 39, 40, 80):
            assert s.blocks(ms) == blocks(ms), (name, ms)


def test_result_line_formats(golden_cases):
    for case in golden_cases.values():
        for item, res, line in zip(case["items"], case["results"], case["lines"]):
            m, c, d = res
            assert acquire.format_result(case["script"], item, (m, c, d)) == line


def test_option_parsers():
    assert acquire.parse_list_ranges("1,3,7-9") == [1, 3, 7, 8, 9]
    assert acquire.parse_list_ranges("-7:7", sep=":") == list(range(-7, 8))
    assert acquire.parse_list_floats("-7000,7000,200") == [-7000.0, 7000.0, 200.0]
    np.testing.assert_array_equal(acquire.doppler_grid([-5000, 5000, 500]), np.arange(-5000, 5000, 500))
    assert len(acquire.doppler_grid([-5000.0, 5000.0, 250.0])) == 40      # half-open: max excluded


def test_finalize_merges_shards_in_doppler_order_with_strict_greater():
    """gacq_finalize needs no GPU: shard merge + (metric, code, doppler) conversion."""
    # a gacq_sig cannot be built without a GPU, so this pins the merge RULE the native function
    # implements (tests/test_gpu_parity.py::test_finalize_shard_merge calls the native one)
    peaks = np.zeros((3, 2), dtype=acquire.PEAK_DTYPE)
    peaks["metric"] = [[5.0, 0.0], [5.0, 2.0], [7.0, 2.0]]
    peaks["idx"] = [[10, -1], [11, 20], [12, 21]]
    peaks["d_index"] = [[1, -1], [0, 3], [2, 0]]
    d0 = [0, 4, 8]
    best = []
    for p in range(2):
        m, i, d = 0.0, -1, -1
        for s in range(3):
            if peaks[s, p]["d_index"] >= 0 and peaks[s, p]["metric"] > m:
                m, i, d = peaks[s, p]["metric"], peaks[s, p]["idx"], peaks[s, p]["d_index"] + d0[s]
        best.append((m, i, d))
    assert best == [(7.0, 12, 10), (2.0, 20, 7)]       # ties keep the earlier (lower-Doppler) shard


def test_header_compiles_as_strict_c99_and_a_c_program_links(tmp_path):
    """include/gacq.h is the drop-in boundary for C callers too: a C99 translation unit (-pedantic, no C++) includes it,
    links libgacq.so and gets the ICD's first ten C/A chips of PRN 1 (octal 1440) and a loud error without a GPU."""
    import subprocess
    src = tmp_path / "cabi.c"
    src.write_text(r'''
#include <stdio.h>
#include <stdint.h>
#include "gacq.h"
int main(void) {
  uint8_t chips[1023];
  gacq_ctx* ctx = 0;
  int i, rc;
  if (gacq_code_chips("gps.ca", 1, chips, 1023) < 0) return 1;
  for (i = 0; i < 10; i++) putchar('0' + chips[i]);
  rc = gacq_create(1 << 20, &ctx);                 /* no such device anywhere: must fail, never crash */
  printf(" %d %d\n", rc, ctx == 0);
  return 0;
}
''')
    exe = tmp_path / "cabi"
    libdir = os.path.join(ROOT, "gnss-dsp-tools_amd", "lib")
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
           "-L", libdir, "-lgacq", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"]
    build = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    chips, rc, null = run.stdout.split()
    assert chips == "1100100000" and int(rc) < 0 and null == "1"


def test_new_entry_points_fail_loudly_without_crashing():
    """Round-2 entry points: NULL handles come back as GACQ_ERR_BAD_ARG, a device group cannot be created without a GPU
    (GACQ_ERR_NO_DEVICE, like gacq_create), option numbers are checked -- all without touching a device."""
    lib = nat.lib
    res = (nat.Result * 2)()
    x = np.zeros(8, dtype=np.complex64)
    items = np.zeros(2, dtype=np.int32)
    dop = np.array([0.0, 250.0])
    args = (x.ctypes.data_as(nat.c_float_p), 4, 1, items.ctypes.data_as(nat.c_int_p), 2, dop.ctypes.data_as(nat.c_double_p), 2, None, 1, res)
    assert lib.gacq_search_batch(None, *args) == -1
    assert lib.gacq_group_search_batch(None, *args) == -1
    assert lib.gacq_group_size(None) == -1 and lib.gacq_group_member(None, 0) is None
    assert lib.gacq_group_set_exchange(None, 1) == -1            # round 5: RCCL exchange of a device group, complex128 samples in
    x128 = np.zeros(8, dtype=np.complex128)
    assert lib.gacq_search64(None, x128.ctypes.data_as(ctypes.c_void_p), 4, items.ctypes.data_as(nat.c_int_p), 2, dop.ctypes.data_as(ctypes.c_void_p), 2, None, 1, res) == -1
    assert lib.gacq_search_batch_dev64(None, None, 4, 1, items.ctypes.data_as(nat.c_int_p), 2, dop.ctypes.data_as(nat.c_double_p), 2, None, 1, None) == -1
    assert lib.gacq_merge_peaks_tiesafe_dev64(None, None, 4, 1, items.ctypes.data_as(nat.c_int_p), 2, dop.ctypes.data_as(nat.c_double_p), 2, None, 1, None, 1,
                                              items.ctypes.data_as(nat.c_int_p), None) == -1
    h = ctypes.c_void_p()
    assert lib.gacq_group_create(None, 1, ctypes.byref(h)) == -1
    ids = (ctypes.c_int * 2)(0, 1)
    if lib.gacq_device_count() == 0:
        assert lib.gacq_group_create(ids, 2, ctypes.byref(h)) == -7 and not h.value
        with pytest.raises(nat.GacqError):
            acquire.DeviceGroup([0])
    assert lib.gacq_set_option(None, 0, 1) == -1 and lib.gacq_get_option(None, 0, None) == -1
    assert lib.gacq_debug_nco_indices(None, 1, 0.0, 0.0, None) == -1
    assert lib.gacq_longcode_search_int8(None, None, 0, 1.0, 0.0, b"gps.l2cl", 1, 0.0, None, 1, 1, 1, None) == -1
    assert lib.gacq_debug_fft_plans(None) == -1
    assert lib.gacq_acquire_int8(None, None, 0, 1.0, 0.0, None, 0, 0, None, 0, None, 0, None, 0, None) == -1
    assert set(nat.OPTIONS.values()) == set(range(len(nat.OPTIONS)))          # GACQ_OPT_* numbering is dense
    # round 6: streams with a hardware queue of their own / a CU mask
    sh, mask = ctypes.c_void_p(), (ctypes.c_uint32 * 8)(*([0xffffffff] * 8))
    assert lib.gacq_stream_create_cu_mask(0, mask, 8, None) == -1
    assert lib.gacq_stream_create_cu_mask(-1, mask, 8, ctypes.byref(sh)) == -1 and not sh.value
    assert lib.gacq_stream_create_cu_mask(0, None, 8, ctypes.byref(sh)) == -1 and lib.gacq_stream_create_cu_mask(0, mask, 0, ctypes.byref(sh)) == -1
    if lib.gacq_device_count() > 0:
        assert lib.gacq_stream_create_cu_mask(0, (ctypes.c_uint32 * 8)(), 8, ctypes.byref(sh)) == -1 and not sh.value      # empty mask
    assert lib.gacq_stream_destroy(0, None) == 0
    assert lib.gacq_cu_census(None, 16, None) == -1
    hdr = open(os.path.join(ROOT, "include", "gacq.h")).read()
    for name, num in nat.OPTIONS.items():
        assert re.search(r"#define GACQ_OPT_%s %d\b" % (name.upper(), num), hdr), name
    assert re.search(r"#define GACQ_NOPTS %d\b" % len(nat.OPTIONS), hdr)
    # the one positive return code (a warning, not an error) and its Python mirror
    assert re.search(r"#define GACQ_WARN_TIE_LIST_FULL %d\b" % nat.WARN_TIE_LIST_FULL, hdr) and nat.WARN_TIE_LIST_FULL > 0
    assert nat.check_search(0) == 0
    with pytest.warns(nat.TieListFull):
        assert nat.check_search(nat.WARN_TIE_LIST_FULL) == nat.WARN_TIE_LIST_FULL
    with pytest.raises(nat.GacqError):
        nat.check_search(-1)
