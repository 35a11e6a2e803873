"""CPU ORACLE -- TEST INFRASTRUCTURE ONLY.  numpy (fp64) restatement of the reference's time-domain long-code searches
(acquire-gps-l2cl.py:15-30, acquire-glonass-l1-p.py:15-33, acquire-glonass-l2-p.py:15-33).  Pinned by
tests/golden/longcode_cases.json (tools/make_goldens_longcode.py ran the reference's own search() functions)."""
import numpy as np

from . import acq_oracle, codes_oracle


def _code(chips01, chips, frac, incr, n):
    """<sig>.code(prn, chips, frac, incr, n)   (gnsstools/gps/l2cl.py:57-63, glonass/p.py:27-32)."""
    L = len(chips01)
    idx = (chips % L) + frac + incr * np.arange(n)
    idx = np.mod(np.floor(idx).astype('int'), L)
    return 1.0 - 2.0 * chips01[idx].astype(np.float64)


# chips per second of the codes the long-code searches (and the generic entry point's tests) use (gnsstools/gps/l2cl.py, glonass/p.py,
# gps/ca.py: chip_rate)
CHIP_RATE = {"gps.l2cl": 511500.0, "glonass.p": 5110000.0, "gps.ca": 1023000.0}


def q_vector(x, code, prn, carrier_hz, phase0, blocks, n, fs, chips01=None):
    """Every candidate's sum, fp64, exactly what gacq_longcode_search computes:
        q[k] = sum_b | sum_i x[b*n + i] * code[floor(phase0[k, b] + incr*i) mod L] * nco(-carrier_hz/fs, 0, n)[i] |
    with incr = chip_rate/fs.  The index is the reference's (chips % L) + frac + incr*np.arange(n) with phase0 = (chips % L) + frac,
    floored and np.mod-wrapped (_code).  Candidates go through in groups so that no (group, n) index table exceeds ~4 M entries.
    chips01: a {0,1} code table to use instead of the code's own (a deliberately corrupted one, for sensitivity checks)."""
    c01 = codes_oracle.chips(code, prn) if chips01 is None else np.asarray(chips01)
    L = len(c01)
    sign = 1.0 - 2.0 * c01.astype(np.float64)
    phase0 = np.asarray(phase0, dtype=np.float64).reshape(-1, max(blocks, 0))
    K = phase0.shape[0]
    q = np.zeros(K)
    if blocks <= 0:
        return q
    w = acq_oracle.nco(-carrier_hz / fs, 0, n)
    di = (CHIP_RATE[code] / fs) * np.arange(n)
    rows = max(1, (1 << 22) // n)
    for block in range(blocks):
        xw = np.asarray(x[n * block:n * (block + 1)], dtype=np.complex128) * w
        for k0 in range(0, K, rows):
            idx = np.mod(np.floor(phase0[k0:k0 + rows, block, None] + di[None, :]).astype('int'), L)
            s = sign[idx]
            q[k0:k0 + rows] += np.absolute((s @ xw.real) + 1j * (s @ xw.imag))
    return q


def best(q):
    """The reference's strict '>' scan from (0, 0): the first maximum wins (acquire-gps-l2cl.py:20,27-29)."""
    m_metric, m_k = 0, 0
    for k, v in enumerate(q):
        if v > m_metric:
            m_metric, m_k = v, k
    return m_metric, m_k


def search_l2cl(x, prn, doppler, l2cm_code_phase, ms, fs):
    blocks = ms // 20
    n = int(fs * 0.020)
    # chips = (k + block) * 10230 + l2cm_code_phase, start phase (chips % L) + 0   (acquire-gps-l2cl.py:24, gps/l2cl.py:59)
    phase0 = np.empty((75, max(blocks, 0)))
    for k in range(75):
        for block in range(blocks):
            phase0[k, block] = (((k + block) * 10230 + l2cm_code_phase) % 767250) + 0
    return best(q_vector(x, "gps.l2cl", prn, doppler, phase0, blocks, n, fs))


def search_glonass_p(x, chan, doppler, ca_code_phase, ms, fs, band="l1"):
    spacing = {"l1": 562500, "l2": 437500}[band]
    blocks = ms // 4
    n = int(fs * 0.004)
    incr = 5110000.0 / fs
    # cp = 5110 k + 10 ca_code_phase, advanced by n * incr per block; start phase (0 % L) + cp   (acquire-glonass-l1-p.py:24-31)
    phase0 = np.empty((1000, max(blocks, 0)))
    for k in range(1000):
        cp = 5110 * k + 10 * ca_code_phase
        for block in range(blocks):
            phase0[k, block] = (0 % 5110000) + cp
            cp += n * incr
    return best(q_vector(x, "glonass.p", 0, spacing * chan + doppler, phase0, blocks, n, fs))
