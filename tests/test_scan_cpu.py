"""CPU: the parts of the recording scan (gnss_dsp_tools_amd/scan.py) that need no GPU -- the epoch arithmetic against exact rational
arithmetic, the piece reader with carried overlap against slices of the whole array, the parser, the refusals of the two new entry
points through the raw ABI -- and the statement tests/test_scan_gpu.py relies on: the CPU path finds every satellite of the scene of
tests/scan_cases.py."""
import io
from fractions import Fraction

import numpy as np
import pytest

import scan_cases as S
from gnss_dsp_tools_amd import _native as nat
from gnss_dsp_tools_amd import cli, scan, signals


def _exact_starts(fs, every_ms, total, n_in, skip_ms=0.0, epochs=None):
    """the definition in exact rational arithmetic; it decides what the float products of the definition must give where a position
    is a whole number or lies further than 1e-6 from one, which the cases below keep to (asserted)"""
    step = Fraction(fs) * Fraction(1, 1000) * Fraction(every_ms)
    skip = int(Fraction(fs) * Fraction(1, 1000) * Fraction(skip_ms))
    out, e = [], 0
    while epochs is None or e < epochs:
        pos = step * e
        assert pos == int(pos) or min(pos - int(pos), int(pos) + 1 - pos) > Fraction(1, 10 ** 6), (e, float(pos))
        s = skip + int(pos)
        if s + n_in > total:
            break
        out.append(s)
        e += 1
    return out


@pytest.mark.parametrize("fs,every,total,n_in,skip,epochs", [
    (5000001.0, 7.0, 225000, 35000, 0.0, None),          # fs*0.001*T_MS = 35000.007: the starts are no multiples of anything
    (5000001.0, 2.3, 225000, 35000, 0.0, None),          # overlapping windows
    (5.0e6, 7.0, 225000, 35000, 1.5, None),              # skip
    (5.0e6, 7.0, 225000, 35000, 0.0, 99),                # more epochs asked for than fit
    (5.0e6, 7.0, 225000, 35000, 0.0, 3),
    (69.984e6, 6.0, 3000000, 419904, 0.0, None),
])
def test_window_starts_are_the_definition(fs, every, total, n_in, skip, epochs):
    got = scan.window_starts(fs, every, total, n_in, skip, epochs)
    assert got.dtype == np.int64 and got.tolist() == _exact_starts(fs, every, total, n_in, skip, epochs)
    assert len(got) >= 3 and got[-1] + n_in <= total


def test_a_recording_of_one_window_has_one_epoch_and_one_sample_less_has_none():
    assert scan.window_starts(5.0e6, 7.0, 35000, 35000).tolist() == [0]
    assert scan.window_starts(5.0e6, 7.0, 34999, 35000).tolist() == []
    assert scan.window_starts(5.0e6, 7.0, 70000, 35000).tolist() == [0, 35000]
    assert scan.window_starts(5.0e6, 7.0, 69999, 35000).tolist() == [0]
    assert scan.window_starts(5.0e6, 7.0, 70000, 35000, epochs=0).tolist() == []
    with pytest.raises(ValueError):
        scan.window_starts(5.0e6, 0.0, 70000, 35000)


class _ShortReads(io.BytesIO):
    """a file object that, like a pipe, returns less than it was asked for"""

    def read(self, n=-1):
        return super().read(min(n, 7001) if n is not None and n > 0 else n)


@pytest.mark.parametrize("every,epochs", [(7.0, None), (3.0, None), (9.5, None), (7.0, 4), (0.0003, 5)])
def test_piece_reader_yields_the_windows_of_the_whole_array(every, epochs):
    """pieces of 1.5 windows: back to back (7 ms) every piece is one window, with overlap (3 ms) the shared samples are carried, with
    gaps (9.5 ms) the samples in between are read and dropped; the file object returns short reads"""
    fs, n_in, total = 5.0e6, 35000, 225000 + 1
    rec = np.random.default_rng(5).integers(-128, 128, size=2 * total, dtype=np.int8)
    fp = _ShortReads(rec.tobytes() + b"\x01")                  # an odd byte at the end is nobody's sample
    want = scan.window_starts(fs, every, total, n_in, epochs=epochs)
    got, sizes = [], []
    for e0, starts, base, buf in scan.read_windows(fp, fs, every, n_in, epochs=epochs, piece_bytes=3 * n_in):
        assert e0 == len(got) and buf.dtype == np.int8 and base <= starts[0]
        for s in starts:
            k = int(s - base)
            assert np.array_equal(buf[2 * k:2 * (k + n_in)], rec[2 * s:2 * (s + n_in)]), (e0, s)
        got += starts.tolist()
        sizes.append((len(starts), len(buf)))
    assert got == want.tolist() and len(got) >= 4
    assert all(nbytes <= 2 * max(3 * n_in // 2, n_in) for _, nbytes in sizes)      # a piece never outgrows its size
    if every == 7.0:
        assert all(m == 1 for m, _ in sizes)
    if every == 3.0:
        assert max(m for m, _ in sizes) == 2                   # 15000 + 35000 samples fit 52500


def test_piece_reader_respects_max_windows_and_a_large_piece_holds_everything():
    fs, n_in, total = 5.0e6, 35000, 225000
    rec = np.random.default_rng(6).integers(-128, 128, size=2 * total, dtype=np.int8)
    pieces = list(scan.read_windows(io.BytesIO(rec.tobytes()), fs, 7.0, n_in))
    assert len(pieces) == 1 and pieces[0][1].tolist() == [0, 35000, 70000, 105000, 140000, 175000]
    pieces = list(scan.read_windows(io.BytesIO(rec.tobytes()), fs, 7.0, n_in, max_windows=4))
    assert [len(p[1]) for p in pieces] == [4, 2]


def test_parser_takes_the_acquire_options_and_the_scan_options():
    sig, a = scan.parse("gps-l1", ["--doppler-search", "-7000,7000,200", "--prn", "1,5-7", "--time", "2", "--every", "7.5", "--skip", "1.25",
                                   "--epochs", "9", "--min-metric", "2.5", "--device", "0", "/dev/stdin", "5e6", "-120000"])
    assert sig is signals.get("gps-l1")
    assert (a.doppler_search, a.items, a.time, a.every, a.skip, a.epochs, a.min_metric) == ("-7000,7000,200", "1,5-7", 2, 7.5, 1.25, 9, 2.5)
    assert (a.input_filename, a.sample_rate, a.carrier_offset) == ("/dev/stdin", 5.0e6, -120000.0)
    # defaults: those of the acquire command; --every = --time + 5 (back-to-back windows)
    sig, a = scan.parse("glonass-l1", ["--channel", "-7:7", "f", "10e6", "0"])
    ref = cli.build_parser(sig).parse_args(["f", "10e6", "0"])
    assert (a.time, a.doppler_search, a.device) == (ref.time, ref.doppler_search, ref.device) and a.items == "-7:7"
    assert a.every == ref.time + 5 and a.skip == 0 and a.epochs is None and a.min_metric is None
    with pytest.raises(SystemExit):
        scan.parse("gps-l1", ["--every", "0", "f", "5e6", "0"])


@pytest.mark.parametrize("name", sorted(cli.LONGCODE))
def test_long_code_signals_are_refused_by_name(name):
    with pytest.raises(SystemExit, match=name):
        scan.run(name, ["f", "5e6", "0", "1", "0", "0"])


def test_new_entry_points_refuse_a_null_context():
    lib = nat.lib
    starts = np.zeros(1, dtype=np.int64)
    taps = np.ones(161, dtype=np.float64)
    assert lib.gacq_frontend_batch_dev(None, None, 0, None, 0, 0, 1.0, 0.0, None, 0, 1.0, 0, None) == -1
    assert lib.gacq_frontend_batch_dev(None, 8, 1000, starts.ctypes.data, 1, 1000, 1.0, 0.0, taps.ctypes.data_as(nat.c_double_p), 161, 1.0, 10, 8) == -1
    assert b"ctx is NULL" in lib.gacq_last_error(None)
    assert lib.gacq_scan_int8_dev(None, None, 0, None, 0, 0, 1.0, 0.0, None, 0, 0, None, 0, None, 0, None, 0, None) == -1
    assert b"gacq_scan_int8_dev" in lib.gacq_last_error(None)


def test_the_cpu_path_finds_every_satellite_of_the_scene():
    """first and last epoch of the scene: fp64 recording -> int8 -> front-end oracle -> numpy search"""
    import simulate_cases
    import simulate_oracle as O
    from oracle import acq_oracle, frontend_oracle
    sig = signals.get("gps-l1")
    sats = simulate_cases.oracle_sats(S.SATS, S.COFFSET)
    starts = scan.window_starts(S.FS, S.EVERY, S.N, S.N_IN)
    assert len(starts) == S.EPOCHS
    for start in (int(starts[0]), int(starts[-1])):
        iq = O.to_int8(O.evaluate(sats, S.FS, S.SIGMA, S.SEED, start, S.N_IN))
        x = frontend_oracle.condition(frontend_oracle.iq_to_complex(iq), S.FS, S.COFFSET, sig, S.MS + 5)
        for sat in S.SATS:
            r = acq_oracle.search_script("gps-l1", x, sat.item, S.DOPPLER_SEARCH, S.MS)
            bins, samples = S.found("gps-l1", sat, start, r)
            print("start %6d prn %2d: metric %.2f doppler %.1f (%.2f bins off) code %.2f (%.2f samples off)" % (start, sat.item, r[0], r[2], bins, r[1], samples))
            assert bins <= 1.0 and samples <= 1.0, (start, sat, r)
