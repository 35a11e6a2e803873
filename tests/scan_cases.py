"""The scene shared by tests/test_scan_cpu.py and tests/test_scan_gpu.py: three GPS L1 satellites with off-grid Dopplers and code
phases at 5 MS/s, 45 ms long, scanned with --time 2 --every 7 (six back-to-back windows of 7 ms), and one PRN that is not there.

Amplitudes 3, 2.5 and 2 LSB per component under noise of sigma 12: 52, 50.5 and 48.5 dB-Hz.  The CPU path (the fp64 recording of
tests/simulate_oracle.py, oracle/frontend_oracle.condition, the numpy search) finds all three at the first and at the last epoch:
tests/test_scan_cpu.py asserts that."""
from gnss_dsp_tools_amd import signals, simulate

SEED = 20261019
FS = 5.0e6
COFFSET = 120000.0
SIGMA = 12.0
N = 225000                                   # 45 ms
MS, EVERY = 2, 7.0
N_IN = int(FS * 0.001 * (MS + 5))            # 35000
DOPPLER_SEARCH = [-4000.0, 4000.0, 200.0]
NOISE_PRN = 30
SATS = [
    simulate.Satellite("gps-l1", 5, 3.0, 1537.3, 200.25, 0.1),
    simulate.Satellite("gps-l1", 12, 2.5, -2210.7, 811.6, 0.7),
    simulate.Satellite("gps-l1", 23, 2.0, 3333.3, 17.9, 0.4),
]
ITEMS = [5, 12, NOISE_PRN, 23]
EPOCHS = 6
L = 1023


def predicted_code(sat, start):
    """code phase (chips, modulo the code length) of `sat` at sample `start` of the recording, code Doppler included"""
    return (sat.code0 + sat.code_rate_hz() * start / FS) % L


def code_error(found, want):
    d = abs(found - want) % L
    return min(d, L - d)


def found(sig_name, sat, start, result):
    """(Doppler error in bins, code error in internal-rate samples) of a (metric, code, doppler) result against the scene"""
    sig = signals.get(sig_name)
    return abs(float(result[2]) - sat.doppler) / DOPPLER_SEARCH[2], code_error(float(result[1]), predicted_code(sat, start)) / (L / sig.n)
