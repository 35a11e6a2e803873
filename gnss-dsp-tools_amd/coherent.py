"""Coherent acquisition across the secondary code and the data-bit edge.

The FFT search integrates coherently over one primary-code period and sums magnitudes beyond that.  Here M periods are summed
coherently under every sign hypothesis that the secondary (overlay) code or a data-bit edge allows: correlation is linear, so the
coherent sum of the M per-period correlations under a sign pattern W[h] equals the correlation of the signed, carrier-wiped sum of
the M input periods.  ``fold_dev`` forms those sums on the device (csrc/gacq_cohfold.hip, one launch: every fine Doppler value d and
pattern h gives one row), ``search`` hands the rows as epochs to ``Engine.search_batch_dev`` at Doppler 0 with one block and keeps,
per item, the best (d, h): metric, code offset, Doppler and the label of the pattern -- the secondary-code phase and, with
``data_flip``, the period at which the data bit inverts.

    python -m gnss_dsp_tools_amd.coherent <signal> [--prn 1-32] [--doppler-search MIN,MAX,INCR] --periods M [--data-flip]
                                          [--carrier-hz HZ] FILE FS COFFSET

prints the acquire script's line per item plus `` secondary_phase %d[ flip_at %d]``.
"""
import argparse
import ctypes
import sys

import numpy as np

from . import _native as nat
from . import acquire, cli, codes
from . import signals as _signals
from .secondary import SECONDARY

MAX_M = 128              # gacq_fold_dev
MAX_H = 256


def patterns(secondary, M, data_flip=False):
    """Sign patterns over M periods: (W int8 [H, M], labels).  Row h < S is secondary[(m + h) % S] (secondary=None: all ones, S = 1).
    With data_flip every such row is followed by its variants whose sign inverts from period k on, for each k in 1..M-1 at which a
    data-bit boundary can fall -- where the overlay restarts, (k + h) % S == 0: at most one k per row when M <= S, every k without
    an overlay.  A row that equals an earlier one up to a global sign is dropped.  labels[h] = (secondary_phase, flip_at or None)."""
    M = int(M)
    if M < 1:
        raise ValueError("M = %d: need at least one period" % M)
    sec = np.ones(1, dtype=np.int8) if secondary is None else np.asarray(secondary)
    if sec.ndim != 1 or len(sec) < 1 or not np.all(np.abs(sec) == 1):
        raise ValueError("secondary must be a 1-D array of +-1 chips")
    sec = sec.astype(np.int8)
    S = len(sec)
    m = np.arange(M)
    rows, labels, seen = [], [], set()

    def add(row, label):
        key = (row * row[0]).tobytes()                   # up to a global sign
        if key not in seen:
            seen.add(key)
            rows.append(row)
            labels.append(label)

    for h in range(S):
        base = sec[(m + h) % S]
        add(base, (h, None))
        if data_flip:
            for k in range(1, M):
                if (k + h) % S == 0:
                    add(np.where(m >= k, -base, base).astype(np.int8), (h, k))
    return np.stack(rows).astype(np.int8), labels


def starts(sig, dopplers, M, carrier_hz=None):
    """Start table int64 [D, M] of the M periods in samples: m * sig.n, and with carrier_hz the code-Doppler slip in whole samples,
    -rint(m * sig.n * f_d / carrier_hz), on top (fp64 numpy)."""
    sig = _signals.get(sig) if isinstance(sig, str) else sig
    f = np.atleast_1d(np.asarray(dopplers, dtype=np.float64))
    t = (np.arange(int(M), dtype=np.int64) * int(sig.n))[None, :]
    out = np.broadcast_to(t, (len(f), int(M))).copy()
    if carrier_hz is not None:
        out = out - np.rint(t.astype(np.float64) * f[:, None] / float(carrier_hz)).astype(np.int64)
    return np.ascontiguousarray(out, dtype=np.int64)


def one_block_per_secondary_chip(sig):
    """True when one block of sig.n samples is exactly one period of the primary code, hence one secondary chip:
    code_length / chip_rate == n / fs."""
    sig = _signals.get(sig) if isinstance(sig, str) else sig
    return float(codes.code_length(sig.code)) * float(sig.fs) == float(sig.n) * float(codes.chip_rate(sig.code))


def builtin_secondary(sig):
    """The built-in secondary code of an acquire signal: a +-1 array, or {PRN: array} for the per-PRN tables.  Refuses, by name, a
    signal whose code has none or whose blocks are not one secondary chip long."""
    sig = _signals.get(sig) if isinstance(sig, str) else sig
    if sig.code not in SECONDARY:
        raise ValueError("%s (%s) has no built-in secondary code; pass secondary=<array> or secondary=None" % (sig.name, sig.code))
    if not one_block_per_secondary_chip(sig):
        raise ValueError("%s: a block of %d samples at %g Hz is not one period of %s (%d chips at %g chips/s): the built-in secondary "
                         "code does not apply" % (sig.name, sig.n, sig.fs, sig.code, codes.code_length(sig.code), codes.chip_rate(sig.code)))
    return SECONDARY[sig.code]


def fold_dev(x_dev, n_out, starts, dopplers, fs, W, j0=0, engine=None):
    """gacq_fold_dev: x_dev 1-D complex64 (or complex128, rounded once) CUDA tensor ->
    y[d,h,i] = sum_m W[h,m] x[starts[d,m] + i] exp(-2 pi i frac(dopplers[d] (j0 + starts[d,m] + i) / fs)), complex64 [D, H, n_out].
    Asynchronous on the engine's stream (torch's current one)."""
    torch = nat.require_torch()
    eng = engine or acquire.default_engine()
    if not (torch.is_tensor(x_dev) and x_dev.is_cuda and x_dev.dtype in (torch.complex64, torch.complex128) and x_dev.dim() == 1
            and x_dev.is_contiguous()):
        raise ValueError("x_dev must be a contiguous 1-D complex64 (or complex128) CUDA tensor")
    st = np.ascontiguousarray(starts, dtype=np.int64)
    f = np.ascontiguousarray(np.atleast_1d(dopplers), dtype=np.float64)
    w = np.ascontiguousarray(W, dtype=np.int8)
    if st.ndim != 2 or w.ndim != 2 or st.shape[0] != len(f) or st.shape[1] != w.shape[1]:
        raise ValueError("need starts [D, M], dopplers [D] and W [H, M]; got %r, %r and %r" % (st.shape, f.shape, w.shape))
    D, M = st.shape
    H = w.shape[0]
    n_out = int(n_out)
    # what gacq_fold_dev checks, here too: nothing is allocated for a call it would refuse
    if n_out < 1 or D < 1 or H < 1 or M < 1 or M > MAX_M or H > MAX_H:
        raise ValueError("need n_out >= 1, D >= 1, 1 <= M <= %d, 1 <= H <= %d (n_out %d, D %d, M %d, H %d)" % (MAX_M, MAX_H, n_out, D, M, H))
    if not (np.all(np.isfinite(f)) and np.isfinite(fs) and fs > 0.0):
        raise ValueError("dopplers and fs must be finite, fs > 0")
    if np.any(np.abs(w) > 1):
        raise ValueError("W entries must be -1, 0 or +1")
    if st.min() < 0 or st.max() + n_out > x_dev.numel():
        raise ValueError("samples [%d, %d) needed, %d available" % (st.min(), st.max() + n_out, x_dev.numel()))
    eng.use_torch_stream(x_dev.device)
    y = torch.empty((D, H, n_out), dtype=torch.complex64, device=x_dev.device)
    nat.check(nat.lib.gacq_fold_dev(eng._ctx, ctypes.c_void_p(x_dev.data_ptr()), int(x_dev.dtype == torch.complex128), x_dev.numel(), n_out,
                                    M, D, H, st.ctypes.data_as(ctypes.c_void_p), f.ctypes.data_as(ctypes.c_void_p), float(fs), int(j0),
                                    w.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(y.data_ptr())), eng._ctx)
    return y


def y_budget(x_dev, engine):
    """Bytes one chunk of folded rows may take: the context's workspace limit (32 GiB unless the engine was given one), and no more
    than a third of 80 % of the device's free memory -- the search that follows wants its two workspaces of the same share."""
    torch = nat.require_torch()
    free, _ = torch.cuda.mem_get_info(x_dev.device)
    limit = int(getattr(engine, "workspace_bytes", 0) or (32 << 30))
    return max(min(limit, int(0.8 * free) // 3), 1)


def _search_group(eng, sig, x_dev, items, dop, st, W, labels, n_out, j0, max_bytes):
    H = len(W)
    per_row = H * n_out * 8
    step = max(1, min(len(dop), int(max_bytes) // per_row))
    best_m = np.zeros(len(items), dtype=np.float64)
    best_i = np.full(len(items), -1, dtype=np.int64)
    best_r = np.full(len(items), -1, dtype=np.int64)
    for d0 in range(0, len(dop), step):
        d1 = min(d0 + step, len(dop))
        y = fold_dev(x_dev, n_out, st[d0:d1], dop[d0:d1], sig.fs, W, j0, eng)
        peaks = eng.search_batch_dev(sig, y.view((d1 - d0) * H, n_out), items, [0.0], 1)
        rec = peaks.cpu().numpy().view(acquire.PEAK_DTYPE).reshape((d1 - d0) * H, len(items))
        for k in range(len(items)):
            col = np.where(rec["d_index"][:, k] >= 0, rec["metric"][:, k], 0.0)
            r = int(np.argmax(col))                      # the first maximum in (d, h) row-major order
            if col[r] > best_m[k]:                       # strictly greater across chunks: the earlier row keeps a tie
                best_m[k], best_i[k], best_r[k] = col[r], rec["idx"][r, k], d0 * H + r
    peaks = np.zeros((1, len(items)), dtype=acquire.PEAK_DTYPE)
    peaks["metric"][0], peaks["idx"][0], peaks["d_index"][0] = best_m, np.maximum(best_i, 0), np.where(best_r >= 0, 0, -1)
    fin = acquire.finalize(sig, items, peaks, [0.0])
    out = []
    for k in range(len(items)):
        if best_r[k] < 0:
            out.append((0, 0, 0, None))
        else:
            out.append((fin[k][0], fin[k][1], np.float64(dop[best_r[k] // H]), labels[best_r[k] % H]))
    return out


def search(name, x_dev, items, dopplers, M, secondary="builtin", data_flip=False, carrier_hz=None, j0=0, engine=None, max_bytes=None):
    """Coherent search over M periods.  x_dev: 1-D complex CUDA tensor at the signal's rate; dopplers: the fine grid (Hz, explicit
    values).  secondary: "builtin" (SECONDARY[sig.code]), a +-1 array, {item: array} or None (no overlay).  Returns per item
    (metric, code_offset, doppler, label): the first strictly greatest metric over (d, h) in row-major order, code_offset as
    acquire.finalize reports it, label = (secondary_phase, flip_at or None) of patterns().  The folded rows are produced in chunks of
    Doppler rows of at most max_bytes (default y_budget); the result does not depend on the chunking."""
    sig = _signals.get(name) if isinstance(name, str) else name
    if sig.bias_hz:
        raise ValueError("%s is an FDMA signal (one carrier per item): the coherent search folds the input once for all items and "
                         "does not serve it" % sig.name)
    items = [int(i) for i in items]
    dop = np.ascontiguousarray(np.atleast_1d(dopplers), dtype=np.float64)
    if isinstance(secondary, str):
        if secondary != "builtin":
            raise ValueError("secondary must be 'builtin', an array, a dict or None")
        secondary = builtin_secondary(sig)
    if isinstance(secondary, dict):
        missing = [it for it in items if it not in secondary]
        if missing:
            raise ValueError("%s: no secondary code for item(s) %s" % (sig.name, missing))
        groups = [([it], secondary[it]) for it in items]
    else:
        groups = [(items, secondary)]
    plans = []
    for its, sec in groups:                              # every pattern set is built and checked before any GPU work
        W, labels = patterns(sec, M, data_flip)
        if int(M) > MAX_M or len(W) > MAX_H:
            raise ValueError("M = %d periods, %d hypotheses: at most %d and %d" % (int(M), len(W), MAX_M, MAX_H))
        plans.append((its, W, labels))
    if not items or len(dop) == 0:
        return [(0, 0, 0, None) for _ in items]
    eng = engine or acquire.default_engine()
    n_out = sig.samples_needed(1)
    st = starts(sig, dop, M, carrier_hz)
    budget = y_budget(x_dev, eng) if max_bytes is None else int(max_bytes)
    out = []
    for its, W, labels in plans:
        out += _search_group(eng, sig, x_dev, its, dop, st, W, labels, n_out, j0, budget)
    return out


def format_line(sig, item, result):
    """The acquire script's line plus ` secondary_phase %d[ flip_at %d]`"""
    metric, code, doppler, label = result
    line = acquire.format_result(sig, item, (metric, code, doppler))
    if label is not None:
        line += " secondary_phase %d" % label[0]
        if label[1] is not None:
            line += " flip_at %d" % label[1]
    return line


_VALUE_OPTS = ("--periods", "--carrier-hz")          # on top of the acquire command line's


def build_parser(sig):
    ap = argparse.ArgumentParser(prog="coherent %s" % sig.name, description="Coherent acquisition of %s over several code periods" % sig.name)
    ap.add_argument(sig.item_opt, dest="items", default=sig.default_items, help="items to search, e.g. 1,3,7%s14 (default %%(default)s)" % sig.item_sep)
    ap.add_argument("--doppler-search", metavar="MIN,MAX,INCR", default=",".join("%g" % v for v in sig.default_doppler))
    ap.add_argument("--periods", type=int, required=True, help="code periods summed coherently (M)")
    ap.add_argument("--data-flip", action="store_true", help="also try a data-bit inversion inside the window")
    ap.add_argument("--carrier-hz", type=float, default=None, help="carrier frequency: follow the code Doppler in whole samples")
    ap.add_argument("--device", type=int, default=0, help="GPU index")
    ap.add_argument("input_filename")
    ap.add_argument("sample_rate", type=float)
    ap.add_argument("carrier_offset", type=float)
    return ap


def run(name, argv, out=sys.stdout):
    sig = _signals.get(name)
    if sig.bias_hz:
        raise SystemExit("%s is an FDMA signal: not served by the coherent search" % sig.name)
    a = build_parser(sig).parse_args(cli.join_option_values(list(argv), cli.VALUE_OPTS + _VALUE_OPTS))
    items = acquire.parse_list_ranges(a.items, sep=sig.item_sep) if a.items else codes.prns(sig.code)
    dop = acquire.doppler_grid(acquire.parse_list_floats(a.doppler_search))
    secondary = builtin_secondary(sig) if sig.code in SECONDARY else None
    if a.carrier_hz is not None and not (a.carrier_hz > 0.0):
        raise SystemExit("--carrier-hz must be positive")
    per_ms = int(round(sig.fs * 0.001))
    slip = int(np.max(np.abs(starts(sig, dop, a.periods, a.carrier_hz)[:, -1] - (a.periods - 1) * sig.n))) if len(dop) else 0
    need = (a.periods - 1) * sig.n + sig.samples_needed(1) + slip
    ms_pad = -(-need // per_ms) + 5                      # the acquire scripts' five spare milliseconds
    n_in = int(a.sample_rate * 0.001 * ms_pad)
    raw = np.fromfile(a.input_filename, dtype=np.int8, count=2 * n_in)
    if len(raw) != 2 * n_in:
        raise SystemExit("input file too short: need %d complex int8 samples" % n_in)
    eng = acquire.Engine(a.device)
    try:
        x_dev = eng.frontend_dev(sig, raw, a.sample_rate, a.carrier_offset, ms_pad)
        results = search(sig, x_dev, items, dop, a.periods, secondary, a.data_flip, a.carrier_hz, 0, eng)
    finally:
        eng.close()
    lines = [format_line(sig, it, r) for it, r in zip(items, results)]
    for line in lines:
        print(line, file=out)
    return lines


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    if not argv or argv[0] in ("-h", "--help"):
        print(__doc__)
        print("signals:", ", ".join(s for s in sorted(_signals.SIGNALS) if not _signals.SIGNALS[s].bias_hz))
        return 0
    run(argv[0], argv[1:])
    return 0


if __name__ == "__main__":
    sys.exit(main())
