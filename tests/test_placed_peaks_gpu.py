"""Peak location at every position of every reducer, against the fp64 oracle.

Each kernel family labels lags and reduces maxima in its own way (register k / j / n1, lane, wave, workgroup chunk, the 31 outputs of
the prime-factor reader over its nine padded segments).  The inputs of tests/placed_cases.py put one peak at a chosen lag per epoch --
every label class of every reducer that serves the length -- and every path below must report that lag, Doppler bin 0 and the
oracle's metric: within 1e-5 on the fp32 paths, within 1e-10 on engine 5 and where every row is re-evaluated in complex128 (DESIGN
section 3).  The path taken is checked where stage_times() or tie_stats() can tell.

Items are [p, p]: two records per epoch from one carrier.  A search whose items share a carrier never takes the one-kernel N = 16384
form (that needs one carrier per item), so that form runs with items [p]."""
import contextlib

import numpy as np
import pytest

import placed_cases as pc

pytestmark = pytest.mark.gpu

FP32, FP64 = 1e-5, 1e-10

# stages with launches (best_doppler aside) that tell the forms apart (gacq_engine.hip, launch_search)
FUSED = {"lds_correlate"}
LDS = {"mix_nco", "lds_correlate"}
SPLIT = {"mix_nco", "lds_correlate", "mag_peak"}                      # forms SplitLds and Pfa
CT = {"mix_nco", "conj_mul", "rocfft_inverse"}                         # SplitRocfft
ROCFFT = {"mix_nco", "rocfft_forward", "conj_mul", "rocfft_inverse", "mag_peak"}

# (id, engine, options, stage signature or None, metric bar, items [p] instead of [p, p])
P4096 = [("rocfft", 1, {}, ROCFFT, FP32, False),
         ("lds-two-kernel", 2, {"fused_4k": 0}, LDS, FP32, False),
         ("lds-fused", 2, {"fused_4k": 2}, FUSED, FP32, False),
         ("c128-rocfft", 5, {"fused_c128": 0}, None, FP64, False),
         ("c128-fused", 5, {"fused_c128": 1}, None, FP64, False)]
P16384 = [("rocfft", 1, {}, ROCFFT, FP32, False),
          ("lds-radix32", 2, {"lds_variant": -1}, LDS, FP32, False),
          ("lds-radix16", 2, {"lds_variant": 16}, LDS, FP32, False),
          ("fused-radix32", 2, {"lds_variant": -1, "fused_16k": 1}, FUSED, FP32, True),
          ("fused-radix16", 2, {"lds_variant": 16, "fused_16k": 1}, FUSED, FP32, True),
          ("unfused-radix32-one-item", 2, {"lds_variant": -1, "fused_16k": 0}, LDS, FP32, True),
          ("unfused-radix16-one-item", 2, {"lds_variant": 16, "fused_16k": 0}, LDS, FP32, True),
          ("split-rocfft", 3, {}, CT, FP32, False),
          ("split-lds", 4, {}, SPLIT, FP32, False),
          ("c128", 5, {}, None, FP64, False)]
PSPLIT = [("rocfft", 1, {}, ROCFFT, FP32, False),
          ("split-rocfft", 3, {}, CT, FP32, False),
          ("split-lds", 4, {}, SPLIT, FP32, False),
          ("c128", 5, {}, None, FP64, False)]
# the four forms of tests/test_gpu_parity.py R31_FORMS, and engine 5
PR31 = [("rocfft-pipeline", 1, {"fused_inner": 1, "split_mfma": 0}, ROCFFT, FP32, False),
        ("pfa-valu", 3, {"fused_inner": 1, "split_mfma": 0}, SPLIT, FP32, False),
        ("pfa-mfma", 3, {"fused_inner": 1, "split_mfma": 1}, SPLIT, FP32, False),
        ("ct-rocfft", 3, {"fused_inner": 0, "split_mfma": 0}, CT, FP32, False),
        ("c128", 5, {}, None, FP64, False)]
PATHS = {"gps-l1": P4096, "glonass-l1-ch0": P16384, "glonass-l1-ch-7": P16384, "beidou-b1i": P16384, "galileo-e1b": PSPLIT,
         "gps-l1cd": PSPLIT, "gps-l2cm": PSPLIT, "gps-l5i": PR31, "xona-x5p": PR31, "galileo-e6b": PR31}
# B = 2: the paths with a multi-block branch of their own -- lds_correlate_kernel<B1 = false> and the N = 16384 correlate kernels, the
# accumulating branch of split_outer_inverse_kernel, pfa_outer_inverse_kernel<., 2> and its matrix-pipe form, c128_4k_* and the
# complex128 readers.  With two blocks the N = 4096 search never takes the fused kernels, whatever fused_4k / fused_c128 say.
PATHS_B2 = {"gps-l1": [("lds-two-kernel", 2, {"fused_4k": 2}, LDS, FP32, False), ("c128-4k", 5, {"fused_c128": 1}, None, FP64, False)],
            "glonass-l1-ch0": [p for p in P16384 if p[0].startswith(("lds-", "fused-", "c128"))],
            "beidou-b1i": [p for p in P16384 if p[0].startswith(("lds-", "split-", "c128"))],
            "galileo-e1b": PSPLIT[1:], "gps-l1cd": PSPLIT[1:],
            "gps-l5i": [PR31[1], PR31[2], PR31[4]], "xona-x5p": [PR31[1], PR31[2], PR31[4]]}

CASES = [(key, 1, p) for key in pc.FAMILIES for p in PATHS[key]] + [(key, 2, p) for key in pc.B2_FAMILIES for p in PATHS_B2[key]]
FAMILY_CASES = [(key, 1) for key in pc.FAMILIES] + [(key, 2) for key in pc.B2_FAMILIES]
DOP0 = np.array([0.0])


@pytest.fixture(scope="module")
def uploads(engine):
    """One upload per (family, B) for the whole module, and stage counters on the shared engine while it runs."""
    import torch
    cache = {}

    def get(key, B):
        if (key, B) not in cache:
            cache[(key, B)] = torch.from_numpy(pc.family(key, B)["xs"].copy()).to("cuda:0")      # the shared array is read-only
        return pc.family(key, B), cache[(key, B)]

    engine.set_profiling(True)
    yield get
    engine.set_profiling(False)
    cache.clear()


@contextlib.contextmanager
def _path(engine, eng, opts):
    saved = {k: engine.get_option(k) for k in opts}
    try:
        engine.set_engine(eng)
        for k, v in opts.items():
            engine.set_option(k, v)
        yield
    finally:
        engine.set_engine(0)
        for k, v in saved.items():
            engine.set_option(k, v)


def _search(engine, f, xd, items):
    import torch
    from gnss_dsp_tools_amd import acquire, signals
    engine.reset_stage_times()
    out = engine.search_batch_dev(signals.get(f["name"]), xd, items, DOP0, f["B"])
    torch.cuda.synchronize()                                       # the engine launches on its own stream
    return out.cpu().numpy().view(acquire.PEAK_DTYPE).reshape(xd.shape[0], len(items))


def _launched(engine):
    return {k for k, (_ms, n) in engine.stage_times().items() if n > 0 and k != "best_doppler"}


def _check(f, got, rtol, what):
    for col in range(got.shape[1]):
        bad = np.flatnonzero(got["idx"][:, col] != f["idx"])
        assert bad.size == 0, (what, "lag", [(int(f["idx"][e]), int(got["idx"][e, col])) for e in bad[:8]], bad.size)
        assert (got["d_index"][:, col] == 0).all(), (what, "Doppler bin", got["d_index"][:, col])
        rel = np.abs(got["metric"][:, col] - f["metric"]) / f["metric"]
        assert rel.max() <= rtol, (what, "metric", int(np.argmax(rel)), rel.max())


@pytest.mark.parametrize("key,B,path", CASES, ids=["%s-B%d-%s" % (k, B, p[0]) for k, B, p in CASES])
def test_every_reducer_position_reports_the_oracle_lag(engine, uploads, key, B, path):
    pid, eng, opts, signature, rtol, single = path
    f, xd = uploads(key, B)
    items = [f["item"]] if single else [f["item"], f["item"]]
    with _path(engine, eng, opts):
        got = _search(engine, f, xd, items)
        launched = _launched(engine)
    if signature is not None:
        assert launched == signature, (key, B, pid, launched)
    _check(f, got, rtol, (key, B, pid))


@pytest.mark.parametrize("key,B", FAMILY_CASES, ids=["%s-B%d" % c for c in FAMILY_CASES])
def test_every_row_reevaluated_in_complex128_reports_the_oracle_lag(engine, uploads, key, B):
    """tie_eps_ppb = 10^9: every row is 'ambiguous', the records come from tie_recheck* / tie_resolve_kernel alone."""
    f, xd = uploads(key, B)
    items = [f["item"], f["item"]]
    rows = len(f["lags"]) * len(items)
    before = engine.tie_stats()
    with _path(engine, 0, {"tie_safe": 1, "tie_eps_ppb": 10 ** 9, "tie_cap": max(64, rows)}):
        got = _search(engine, f, xd, items)
    st = engine.tie_stats()
    assert st["rows_reevaluated"] - before["rows_reevaluated"] == rows and st["kept_fp32"] == before["kept_fp32"], (before, st)
    _check(f, got, FP64, (key, B, "re-evaluated"))


@pytest.mark.parametrize("key", list(pc.FAMILIES))
def test_default_path_without_tie_safe_locations_reports_the_oracle_lag(engine, uploads, key):
    """tie_safe = 0: the plain fp32 record of the default engine, nothing listed and nothing re-evaluated."""
    f, xd = uploads(key, 1)
    before = engine.tie_stats()
    with _path(engine, 0, {"tie_safe": 0}):
        got = _search(engine, f, xd, [f["item"], f["item"]])
    assert engine.tie_stats() == before
    _check(f, got, FP32, (key, 1, "tie_safe = 0"))
