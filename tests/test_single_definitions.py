"""Arithmetic that several tools must share bit for bit has one definition under csrc/, and a copy does not come back: the polynomial
of the replicas' quarter-turn sine / cosine and the TMBOC chip mask (gacq_turn.h), the trace of the diagonal loading in the lane
layout 8 r + c of the array weights kernels (gacq_arraycore.h), and the workgroup reduction of a correlation row to (maximum, first
argmax, sum) -- the fp32 one on Top2 with its runner-up (gacq_common.h), the complex128 one with its record, its per-lane, wave,
cross-wave and LDS-tree steps, the pass-2 twiddle table and the Doppler scan over the records (gacq_fft64.h), the fp64 twiddle table
(gacq_tiesafe.hip).  Each is recognised by a piece of text that only a definition holds.
The same for the C ABI, whose one definition is include/gacq.h (below).  Reads sources only, no GPU."""
import ast
import os
import re

import pytest

PACKAGE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gnss-dsp-tools_amd")
CSRC = os.path.join(PACKAGE, "csrc")


@pytest.mark.parametrize("text, home", [
    ("-4.602163099e-03f", "gacq_turn.h"),             # leading sine coefficient of turn_sincos
    ("(1ull << 29)", "gacq_turn.h"),                  # highest bit of the TMBOC mask
    ("__shfl(Rre, 9 * p, 64)", "gacq_arraycore.h"),   # the trace over lanes 9 p
    # fp32 row reduction: the wave step on shuffles and thread 0's merge of the wave slots
    ("__shfl_down(top.second, off)", "gacq_common.h"),
    ("top.merge(s_peak[", "gacq_common.h"),
    # complex128 row reduction: record, loads / stores, the first-maximum rule per lane (lags in any order), in the shuffle step, in
    # the cross-wave step and in the LDS tree, the lag of the DPP / ballot step, the pass-2 twiddle table, the Doppler scan
    ("struct RowRec64 {", "gacq_fft64.h"),
    ("cd ldc(const double2* p)", "gacq_fft64.h"),
    ("== peak && lag < idx", "gacq_fft64.h"),
    ("const double op = __shfl_down(peak, off)", "gacq_fft64.h"),
    ("&& s_idx[w", "gacq_fft64.h"),
    ("s_sum[t] += s_sum[t + off]", "gacq_fft64.h"),
    ("(t & ~63) + (int)__builtin_ctzll(mk)", "gacq_fft64.h"),
    ("cd pw[15];", "gacq_fft64.h"),
    ("normalised ? r.peak / (r.sum", "gacq_fft64.h"),
    ("sincospi(-2.0 * (double)k", "gacq_tiesafe.hip"),  # W_N^k in fp64: one kernel, one table per context and length
])
def test_one_file_holds_it(text, home):
    hits = []
    for folder, _, names in os.walk(CSRC):
        for name in sorted(names):
            with open(os.path.join(folder, name), encoding="utf-8", errors="replace") as f:
                if text in f.read():
                    hits.append(name)
    assert hits == [home], (text, hits)


# The C ABI has one definition, include/gacq.h: _cabi.py reads it and _native.py binds it.  No other module of the package restates a
# struct (as a ctypes class or as a numpy record dtype) or a prototype.

def abi_copies(source, struct_members):
    """What a module's text restates of the header: ctypes.Structure subclasses, .argtypes / .restype assignments, and np.dtype(...)
    calls on a literal (anything but a name or a call) that spells every member name of a header struct or names one in the comment
    that ends the statement"""
    tree, lines, found = ast.parse(source), source.split("\n"), []
    for node in ast.walk(tree):
        if isinstance(node, ast.ClassDef) and any("Structure" in ast.unparse(b) or "Union" in ast.unparse(b) for b in node.bases):
            found.append("class %s" % node.name)
        if isinstance(node, (ast.Assign, ast.AugAssign, ast.AnnAssign)):
            for t in (node.targets if isinstance(node, ast.Assign) else [node.target]):
                if isinstance(t, ast.Attribute) and t.attr in ("argtypes", "restype"):
                    found.append(ast.unparse(t))
        if isinstance(node, ast.Call) and ast.unparse(node.func).endswith("dtype") and node.args \
                and not isinstance(node.args[0], (ast.Name, ast.Attribute, ast.Call, ast.Constant)):
            words = {c.value for c in ast.walk(node.args[0]) if isinstance(c, ast.Constant) and isinstance(c.value, str)}
            comment = lines[node.end_lineno - 1][node.end_col_offset:].partition("#")[2]
            for sname, members in struct_members.items():
                if set(members) <= words or re.search(r"\b%s\b" % sname, comment):
                    found.append("dtype of %s" % sname)
    return found


def _struct_members():
    from gnss_dsp_tools_amd import _cabi
    return {sname: [f for f, _ in cls._fields_] for sname, cls in _cabi.structs.items()}


def test_the_abi_rule_sees_each_kind_of_copy():
    members = _struct_members()
    text = '''
class Peak(ctypes.Structure):
    _fields_ = []
lib.gacq_search.argtypes = [ctypes.c_void_p]
fn.restype = None
A = np.dtype([("metric", "<f8"), ("idx", "<i4"), ("d_index", "<i4")])
B = np.dtype([(k, "f8") for k in ("s0", "n")] +
             [("x", "i4")])        # gacq_cancel_seg
C = np.dtype([("cell", "<i4"), ("zero", "<i4"), ("q", "<f8")])     # a record of gacq_bearing_run_dev
D = np.dtype(nat.struct("gacq_peak"))
E = np.dtype(np.int8)
'''
    assert abi_copies(text, members) == ["class Peak", "lib.gacq_search.argtypes", "fn.restype", "dtype of gacq_peak", "dtype of gacq_cancel_seg"]


def test_no_module_restates_the_abi():
    members = _struct_members()
    seen = 0
    for name in sorted(os.listdir(PACKAGE)):
        if name.endswith(".py") and name not in ("_cabi.py", "_native.py"):
            with open(os.path.join(PACKAGE, name), encoding="utf-8") as f:
                assert abi_copies(f.read(), members) == [], name
            seen += 1
    assert seen >= 39
