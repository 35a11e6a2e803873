"""ctypes binding of libgacq.so (the C ABI declared in include/gacq.h).

The library is built in-tree by __graft_entry__.build() / `make -C gnss-dsp-tools_amd/csrc`.
There is NO Python/CPU fallback for the engine: if the shared object is missing this module
raises at import, and the engine entry points raise when no GPU is visible.

Nothing here restates the header: prototypes, struct classes and constants are read from include/gacq.h when the package is imported
(_cabi.py).  Adding an entry point, a struct member or a GACQ_* constant means editing the header only; a declaration outside the
subset of C that _cabi.py reads fails the import with the declaration quoted.
"""
import ctypes
import os
import sys

from . import _cabi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libgacq.so")
# Tuning tools only (tools/variant.py): a script that defines GACQ_TUNING_LIB = "<path>" in its __main__ module before
# importing the package loads that build (an A/B or diagnostic variant under build/variants/) instead of the product library.
# lib/libgacq.so itself is never replaced, and nothing reads the environment.
_tuning = getattr(sys.modules.get("__main__"), "GACQ_TUNING_LIB", None)
if _tuning:
    LIB_PATH = os.path.abspath(_tuning)

# One HIP runtime per process: when torch is (or will be) in the process its bundled
# libamdhip64/librocfft (same SONAMEs as /opt/rocm's) must be the ones that get bound, so it
# is imported before libgacq.so is dlopen'ed.  Device buffers are torch tensors anyway.
# A program that never touches a device tensor -- the command-line shim, a stub around search() on numpy samples -- can skip that
# (importing torch is ~0.8 s, most of such a run): it defines GACQ_NO_TORCH = True in its __main__ module before importing the package.
# libgacq.so then binds /opt/rocm's runtime through its rpath, and the entry points that take torch tensors refuse to run (require_torch).
NO_TORCH = bool(getattr(sys.modules.get("__main__"), "GACQ_NO_TORCH", False)) and "torch" not in sys.modules
torch = None
if not NO_TORCH:
    try:
        import torch  # noqa: F401
    except Exception:  # pragma: no cover - torch is part of the image; C-only users do not need it
        torch = None


if NO_TORCH:
    # ... and nothing else in the process may bring torch (a second HIP runtime) in afterwards
    import importlib.abc

    class _NoTorchLater(importlib.abc.MetaPathFinder):
        def find_spec(self, name, path, target=None):
            if name == "torch" or name.startswith("torch."):
                raise ImportError("this process loaded libgacq.so without torch (GACQ_NO_TORCH in __main__): torch and the device-tensor "
                                  "entry points of the package are not available in it")
            return None

    sys.meta_path.insert(0, _NoTorchLater())


def require_torch():
    """For the device-tensor entry points (raises in a GACQ_NO_TORCH process, see above)."""
    import torch as _t
    return _t

if not os.path.exists(LIB_PATH):
    raise ImportError(
        "libgacq.so not built: %s is missing. Run `python -c 'import __graft_entry__ as g; g.build()'` "
        "or `make -C gnss-dsp-tools_amd/csrc` (needs hipcc). There is no CPU fallback." % LIB_PATH)

lib = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)

c_int_p = ctypes.POINTER(ctypes.c_int)
c_double_p = ctypes.POINTER(ctypes.c_double)
c_float_p = ctypes.POINTER(ctypes.c_float)
c_uint8_p = ctypes.POINTER(ctypes.c_uint8)


# Everything below is read from include/gacq.h (_cabi.py).  Pointer parameters are void* to ctypes: the latency path passes plain
# addresses (no ctypes.cast per call), and typed pointer objects, byref(), arrays and None are accepted for a void* parameter as well.
CONSTANTS = _cabi.constants          # "GACQ_TRACK_BAD_BLOCK" -> 1: every integer #define GACQ_*


def struct(name):
    """The ctypes.Structure of a `typedef struct NAME { ... } NAME;` of the header"""
    return _cabi.structs[name]


SigDesc, Result, Peak = struct("gacq_sigdesc"), struct("gacq_result"), struct("gacq_peak")

ERRORS = {v: k for k, v in CONSTANTS.items() if k == "GACQ_OK" or k.startswith("GACQ_ERR_")}
OPTIONS = {k[len("GACQ_OPT_"):].lower(): v for k, v in CONSTANTS.items() if k.startswith("GACQ_OPT_")}      # retired ones included
WARN_TIE_LIST_FULL = CONSTANTS["GACQ_WARN_TIE_LIST_FULL"]

# name -> (restype, argtypes): every symbol include/gacq.h declares
SYMBOLS = _cabi.prototypes

for _name, (_res, _args) in SYMBOLS.items():
    _fn = getattr(lib, _name)          # AttributeError here == the .so does not export a declared symbol
    _fn.restype = _res
    _fn.argtypes = _args


class GacqError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("%s (%d): %s" % (ERRORS.get(code, "GACQ_ERR_?"), code, message))
        self.code = code


class TieListFull(UserWarning):
    """gacq.h GACQ_WARN_TIE_LIST_FULL: the results are valid, but the call's near-ties were NOT re-evaluated in complex128."""


def check(rc, ctx=None):
    if rc < 0:
        msg = lib.gacq_last_error(ctx)
        raise GacqError(rc, msg.decode() if msg else "")
    return rc


def check_search(rc, ctx=None):
    """check() for gacq_search / gacq_search64, whose positive return is a warning (other entry points return counts)."""
    if rc == WARN_TIE_LIST_FULL:
        import warnings
        warnings.warn("tie-safe re-evaluation list full (option tie_cap / workspace limit): every near-tied (epoch, item) of this call kept "
                      "its fp32 location", TieListFull, stacklevel=3)
        return rc
    return check(rc, ctx)
