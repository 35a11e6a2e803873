"""Placed-peak inputs and their fp64 expectations, shared by test_placed_peaks_cpu.py, test_placed_peaks_gpu.py and
test_doppler_scan_gpu.py.  CPU only: everything here comes from the numpy oracle (oracle/acq_oracle.py).

One epoch per wanted lag, built from the oracle's own replica (sample_code, times boc11 where the signal has BOC, zero-padded to 2n
where padded), so that the peak of the correlation row sits at a lag chosen in advance -- one lag for every class of every reducer's
label map (register, lane, wave, chunk, segment; see the table in DESIGN.md section 3):

  B = 1            x = AMP * roll(replica_N, -lag) + unit-variance complex Gaussian noise (seeded per epoch); Doppler 0, where the
                   table NCO is exactly 1
  B = 2 unpadded   np.tile(roll(c, -lag), 2), no noise
  B = 2 padded     two code periods from sample s = (2n - lag) mod 2n on in a 3n buffer: lag 0 and the upper half [n, 2n) only
  GLONASS          the signal term times the channel's bias carrier, as synth.make_iq does

The expectation of an epoch is acq_oracle.search_row in fp64 on the complex64-rounded samples: argmax, max, mean and the relative
margin (max - runner-up) / max.
"""
import functools

import numpy as np

from oracle import acq_oracle, codes_oracle

AMP = 0.5


def _grid(R, stride, ts):
    return [stride * r + t for r in range(R) for t in ts]


def _inv_mod(a, m):
    return next(x for x in range(1, m) if (a * x) % m == 1)


def pfa_time_index(M, pos):
    """Column position of a padded row of the prime-factor reader (nine segments of 11 x Nb columns, each padded to a multiple of 16)
    -> time index t of the column, None for a padding column: the reader's label map, lag = t + M ((q0 + u) mod 31)."""
    Na, Nc, Nb = 11, 9, M // 99
    AB = Na * Nb
    seg = (AB + 15) & ~15
    c, r = divmod(pos, seg)
    if c >= Nc or r >= AB:
        return None
    b, a = divmod(r, Na)
    e = lambda f: (M // f) * _inv_mod(M // f, f)
    return (a * e(Na) + b * e(Nb) + c * e(Nc)) % M


def pfa_extra_lags(M):
    """The table's t values are time indices; the reader's threads are column positions, which the CRT map scatters.  Added: the first
    and last column of each of the nine segments and both sides of every 128-column boundary (wave, tile group and workgroup edges of
    the VALU and the matrix-pipe reader), each at j = 0 and j = 30."""
    AB = 11 * (M // 99)
    seg = (AB + 15) & ~15
    pitch = (9 * seg + 255) & ~255
    pos = {c * seg for c in range(9)} | {c * seg + AB - 1 for c in range(9)}
    pos |= {p for k in range(1, pitch // 128) for p in (128 * k - 1, 128 * k)}
    ts = sorted({pfa_time_index(M, p) for p in pos} - {None})
    return [t + M * j for t in ts for j in (0, 30)]


def paired_extra_lags():
    """Engine 4's reader serves n2 = t + 256 j at position (j >> 1) * 512 + 2 t + (j & 1); the table's n2 values reach j in {0, 1, 2, 15}
    and four of the sixteen 256-position workgroups.  Added: every j with t in {0, 127, 128, 255} (first and last position of every
    workgroup), n1 walking with j."""
    return [4096 * j + 256 * j + t for j in range(16) for t in (0, 127, 128, 255)]


# key -> (signal, item, B = 1 lags of the table, B = 2 lags or None); EXTRA: B = 1 lags added for label classes the table misses
# B = 2 keeps every register index (k, j, n1, the 31 outputs) with t in {0, last}; padded signals keep of those what two periods in a
# 3n buffer can reach (lag 0 and lags >= n)
def _families():
    f = {}
    f["gps-l1"] = ("gps-l1", 7, _grid(16, 256, (0, 15, 16, 63, 64, 255)), _grid(16, 256, (0, 255)))
    t16 = (0, 63, 64, 511)
    f["glonass-l1-ch0"] = ("glonass-l1", 0, _grid(32, 512, t16), _grid(32, 512, (0, 511)))
    f["glonass-l1-ch-7"] = ("glonass-l1", -7, _grid(32, 512, t16), None)
    f["beidou-b1i"] = ("beidou-b1i", 12, _grid(32, 512, t16), _grid(32, 512, (0, 511)))
    f["galileo-e1b"] = ("galileo-e1b", 3, _grid(16, 4096, (0, 1, 255, 256, 511, 512, 4095)), _grid(16, 4096, (0, 4095)))
    f["gps-l1cd"] = ("gps-l1cd", 3, _grid(20, 4096, (0, 255, 256, 4095)), _grid(20, 4096, (0, 4095)))
    f["gps-l2cm"] = ("gps-l2cm", 3, sorted(_grid(40, 4096, (0, 4095)) + [4096 * n1 + n2 for n1 in (0, 39) for n2 in (255, 256)]), None)
    f["gps-l5i"] = ("gps-l5i", 9, _grid(31, 1980, (0, 1, 219, 220, 1979)), _grid(31, 1980, (0, 1979)))
    t990 = (0, 109, 110, 989)
    f["xona-x5p"] = ("xona-x5p", 0, _grid(31, 990, t990), _grid(31, 990, (0, 989)))
    f["galileo-e6b"] = ("galileo-e6b", 11, _grid(31, 990, t990), None)
    return f


FAMILIES = _families()
EXTRA = {"galileo-e1b": paired_extra_lags(), "gps-l5i": pfa_extra_lags(1980), "xona-x5p": pfa_extra_lags(990), "galileo-e6b": pfa_extra_lags(990)}
B2_FAMILIES = [k for k, v in FAMILIES.items() if v[3] is not None]


def variant(name):
    """(code module, fs, n, pad, boc, normalised, bias multiplier) of a signal."""
    code, fs, n, pad, boc, normalised, _fold, _blocks, bias = acq_oracle.VARIANTS[name]
    return code, fs, n, pad, boc, normalised, bias


def chips_of(name, item):
    code, _fs, _n, _pad, _boc, _norm, bias = variant(name)
    return codes_oracle.chips(code, 0 if bias else item)


def replica(name, item):
    """The oracle's time-domain replica of one block: n samples, +-1."""
    _code, _fs, n, _pad, boc, _norm, _bias = variant(name)
    chips = chips_of(name, item)
    incr = float(len(chips)) / n
    c = acq_oracle.sample_code(chips, 0, 0, incr, n)
    if boc:
        c = c * acq_oracle.boc11(0, 0, incr, n)
    return c


def wanted_lags(key, B):
    name, _item, lags1, lags2 = FAMILIES[key]
    if B == 1:
        return list(lags1) + sorted(set(EXTRA.get(key, [])) - set(lags1))
    _code, _fs, n, pad, _boc, _norm, _bias = variant(name)
    return [lag for lag in lags2 if not pad or lag == 0 or lag >= n]


def placed_epochs(name, item, lags, B, seed):
    """xs [len(lags), nsamp] complex64: epoch e peaks at lags[e] (module docstring)."""
    _code, fs, n, pad, _boc, _norm, bias = variant(name)
    c = replica(name, item)
    N = 2 * n if pad else n
    nsamp = (B + (1 if pad else 0)) * n
    carrier = np.exp(2j * np.pi * (bias * item) * np.arange(nsamp) / fs) if bias else None
    xs = np.empty((len(lags), nsamp), dtype=np.complex64)
    for e, lag in enumerate(lags):
        if B == 1:
            rep = np.concatenate((c, np.zeros(n))) if pad else c
            s = AMP * np.roll(rep, -lag)
        elif not pad:
            s = np.tile(np.roll(c, -lag), B)
        else:
            start = (N - lag) % N
            if B != 2 or start > n:
                raise ValueError("B = 2 padded reaches lag 0 and lags >= n only, not %d" % lag)
            s = np.zeros(nsamp)
            s[start:start + 2 * n] = np.tile(c, 2)
        x = s.astype(np.complex128)
        if carrier is not None:
            x = x * carrier
        if B == 1:
            rng = np.random.Generator(np.random.PCG64([seed, lag]))
            x = x + (rng.standard_normal(nsamp) + 1j * rng.standard_normal(nsamp)) / np.sqrt(2.0)
        xs[e] = x.astype(np.complex64)
    return xs


def row_expectation(name, item, x, B, doppler=0.0):
    """(argmax, max, mean, relative margin to the runner-up) of the oracle's fp64 row on the samples as the device gets them."""
    _code, fs, n, pad, boc, _norm, bias = variant(name)
    q = acq_oracle.search_row(x.astype(np.complex128), chips_of(name, item), doppler, B, fs=fs, n=n, pad=pad, boc=boc, bias_hz=bias * item)
    i = int(np.argmax(q))
    top = q[i]
    rest = q.copy()
    rest[i] = -np.inf
    return i, float(top), float(np.mean(q)), float((top - rest.max()) / top)


def seed_of(key, B):
    return 7000 + 10 * sorted(FAMILIES).index(key) + B


@functools.lru_cache(maxsize=None)
def family(key, B):
    """Everything the tests need of one (family, B), computed once per process: name, item, lags, xs, and the oracle's idx / peak /
    mean / margin / metric (max/mean or raw max, as the signal reports it) per epoch.  The arrays are shared: do not write to them."""
    name, item = FAMILIES[key][:2]
    lags = wanted_lags(key, B)
    xs = placed_epochs(name, item, lags, B, seed_of(key, B))
    exp = np.array([row_expectation(name, item, x, B) for x in xs], dtype=np.float64)
    normalised = variant(name)[5]
    out = {"name": name, "item": item, "B": B, "lags": lags, "xs": xs, "idx": exp[:, 0].astype(np.int64), "peak": exp[:, 1],
           "mean": exp[:, 2], "margin": exp[:, 3], "metric": exp[:, 1] / exp[:, 2] if normalised else exp[:, 1].copy()}
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


# ---- Doppler scan: explicit grids (repeated values included), carriers placed on chosen bins, dead epochs ----------------------------

def doppler_epoch(name, item, lag, doppler_hz, seed):
    """One B = 1 epoch: AMP * roll(replica_N, -lag) on a carrier of doppler_hz (plus the GLONASS bias) + unit-variance noise."""
    _code, fs, n, pad, _boc, _norm, bias = variant(name)
    c = replica(name, item)
    rep = np.concatenate((c, np.zeros(n))) if pad else c
    i = np.arange(len(rep))
    rng = np.random.Generator(np.random.PCG64([seed, lag]))
    x = AMP * np.roll(rep, -lag) * np.exp(2j * np.pi * (bias * item + doppler_hz) * i / fs)
    x = x + (rng.standard_normal(len(rep)) + 1j * rng.standard_normal(len(rep))) / np.sqrt(2.0)
    return x.astype(np.complex64)


def grid_search(name, item, x, grid, B=1):
    """The body of acq_oracle.search over explicit grid values (np.arange cannot repeat a value): (metric, lag, Doppler index, relative
    margin of the winning bin over the best other bin), Doppler index -1 and metric 0 when no bin beats the initial 0."""
    _code, fs, n, pad, boc, normalised, bias = variant(name)
    C = acq_oracle.code_spectrum(chips_of(name, item), n, pad, boc)
    x = np.asarray(x).astype(np.complex128)
    m_metric, m_idx, m_d = 0, 0, -1
    metrics = []
    with np.errstate(all="ignore"):
        for d, doppler in enumerate(grid):
            f = -(bias * item + doppler) / fs if bias else -doppler / fs
            q = acq_oracle.accumulate_row(x, C, f, n, pad, B)
            idx = np.argmax(q)
            metric = q[idx] / np.mean(q) if normalised else q[idx]
            metrics.append(metric)
            if metric > m_metric:
                m_metric, m_idx, m_d = metric, int(idx), d
    others = [m for m in metrics if not m == m_metric]
    margin = float((m_metric - max(others)) / m_metric) if (m_d >= 0 and others) else 1.0
    return float(m_metric), m_idx, m_d, margin
