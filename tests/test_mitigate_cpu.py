"""CPU: the numpy definition of the mitigation stage (tests/mitigate_oracle.py) against its own properties, the decision margins of
every committed case, the refusals of the raw ABI without a context (gacq_mitigate_check), the command line's parser and report line,
and the interference scene through the oracle and the reference search: the raw recording gives a noise peak, the mitigated one the
satellite."""
import ctypes

import numpy as np
import pytest

import mitigate_cases as C
import mitigate_oracle as O
from gnss_dsp_tools_amd import _native as nat
from gnss_dsp_tools_amd import mitigate
from oracle import acq_oracle, codes_oracle

BAD_ARG, SHORT_INPUT = -1, -6


def _noise_int8(n, seed, sigma=20.0):
    rng = np.random.Generator(np.random.PCG64([C.SEED, seed, n]))
    return np.clip(np.rint(sigma * rng.standard_normal(2 * n)), -127, 127).astype(np.int8)


@pytest.mark.parametrize("n", [64, 128, 1024, 4096])
def test_window_halves_are_power_complementary(n):
    w = O.window(n)
    assert np.max(np.abs(w[:n // 2] ** 2 + w[n // 2:] ** 2 - 1.0)) <= 8 * 2.0 ** -53         # a few fp64 roundings


@pytest.mark.parametrize("n", [64, 1024])
def test_thresholds_that_never_fire_reproduce_the_input(n):
    data = _noise_int8(12 * n + 7, n)
    x, _ = O.samples(data, False)
    r = O.evaluate(O.config(nfft=n, ratio=1e30), data, 1.0)
    assert len(r.y) == (len(x) // (n // 2) - 2 + 1) * (n // 2) and r.bins == 0 and r.blanked == 0 and r.frames == len(r.y) // (n // 2)
    assert np.max(np.abs(r.y - x[:len(r.y)])) <= 1e-12 * 127.0          # block 0, with its zero history, included
    f32 = O.evaluate(O.config(nfft=n, ratio=1e30), data, 1.0, precision="f32")
    assert np.max(np.abs(f32.y - x[:len(r.y)])) <= 2e-5 * 127.0


def test_lower_median_is_the_sorted_middle():
    rng = np.random.Generator(np.random.PCG64(C.SEED))
    for n in (64, 128, 1024):
        p = rng.standard_normal((5, n)) ** 2
        p[2, : n // 2 + 3] = 0.0                                          # ties across the middle
        assert np.array_equal(O.lower_median(p), np.sort(p, axis=1)[:, n // 2 - 1])


def test_blanking_reaches_the_first_and_last_sample_and_across_a_block_edge():
    n, h = 64, 32
    data = np.full(2 * 6 * n, 3, dtype=np.int8)
    for at in (0, 6 * n - 1, 2 * h - 1):                                  # first, last, the last sample of block 1
        data[2 * at] = 120
    cfg = O.config(blank=90.0, hold=3, nfft=0)
    r = O.evaluate(cfg, data, 1.0)
    zero = np.flatnonzero(r.y == 0)
    assert len(r.y) == 6 * n - 3 and zero.tolist() == [0, 1, 2, 3] + list(range(2 * h - 4, 2 * h + 3)) + [6 * n - 4]
    assert r.blanked == len(zero) and r.frames == 0 and r.bins == 0
    assert np.array_equal(r.i8[2 * 4:2 * 8], data[2 * 4:2 * 8])
    # with excision that never fires the blanked samples come back as zeros, the others as they were: the hold crossed the block edge
    both = O.evaluate(O.config(blank=90.0, hold=3, nfft=n, ratio=1e30), data, 1.0)
    x, _ = O.samples(data, False)
    want = np.where(np.isin(np.arange(len(both.y)), zero), 0.0, x[:len(both.y)])
    assert np.max(np.abs(both.y - want)) <= 1e-12 * 127.0 and both.blanked == 4 + 7


def test_a_non_finite_sample_is_blanked_and_counted_with_blanking_off():
    x = (np.arange(1, 401) + 1j * np.arange(400)).astype(np.complex64)
    x[7] = np.nan
    x[300] = complex(1.0, np.inf)
    r = O.evaluate(O.config(nfft=64, ratio=1e30), x, 1.0, True)
    assert r.blanked == 2 and abs(r.y[7]) <= 1e-9 and abs(r.y[300]) <= 1e-9 and np.all(np.isfinite(r.c64))
    assert np.max(np.abs(np.delete(r.y, [7, 300]) - np.delete(x[:len(r.y)].astype(np.complex128), [7, 300]))) <= 1e-10 * 400.0
    r = O.evaluate(O.config(blank=1e6, hold=5, nfft=0), x, 1.0, True)    # no hold around a sanitised sample: it is no hit
    assert r.blanked == 2 and np.flatnonzero(r.y == 0).tolist() == [7, 300]


@pytest.mark.parametrize("cut", [1, 31, 32, 100, 333])
def test_statistics_of_a_two_way_split_sum_to_the_whole(cut):
    c = C.EXCISE_CASES[4]
    cfg = O.config(blank=88.5, hold=1, nfft=c.nfft, ratio=c.ratio, guard=c.guard)
    data, in_first, out_first, n_out = C.case_input(c)
    whole = O.evaluate(cfg, data, C.GAIN, c.in_complex64, in_first, out_first, n_out)
    a = O.evaluate(cfg, data, C.GAIN, c.in_complex64, in_first, out_first, cut)
    b = O.evaluate(cfg, data, C.GAIN, c.in_complex64, in_first, out_first + cut, n_out - cut)
    assert whole.blanked > 0 and whole.bins > 0
    assert (a.blanked + b.blanked, a.frames + b.frames, a.bins + b.bins) == (whole.blanked, whole.frames, whole.bins)
    assert np.array_equal(np.concatenate([a.frame_bins, b.frame_bins]), whole.frame_bins)
    assert np.array_equal(np.concatenate([a.c64, b.c64]), whole.c64)


@pytest.mark.parametrize("c", C.EXCISE_CASES, ids=lambda c: c.name)
def test_decisions_of_every_case_keep_their_distance_from_the_threshold(c):
    ref, bound, top = C.case_reference(c)
    print(c.name, "margin %.3g, float32 deviation %.3g of max |y| = %.3g" % (ref.margin, bound / 4.0, top))
    assert ref.margin >= 1e-4 and ref.bins > 0 and 0 < bound < 1e-4


def _search(i8, chips):
    x = i8[0::2].astype(np.float64) + 1j * i8[1::2].astype(np.float64)
    return acq_oracle.search(x, chips, C.SCENE_DOPPLERS, 3, fs=C.SCENE["fs"], n=4096, normalised=True)


def test_the_scene_is_found_only_after_mitigation():
    s = C.SCENE
    chips = codes_oracle.chips("gps.ca", s["prn"])
    raw = C.scene_int8(chips)
    metric, code, doppler = _search(raw, chips)
    print("raw: metric %.3f code %.2f doppler %.0f" % (metric, code, doppler))
    assert doppler != 1200.0
    cfg = C.scene_cfg()
    gain = O.auto_gain(cfg, raw)
    r = O.evaluate(cfg, raw, gain)
    metric, code, doppler = _search(r.i8, chips)
    print("mitigated (gain %.3f, blanked %.4f, %.1f bins a frame, margin %.3g): metric %.3f code %.2f doppler %.0f"
          % (gain, r.blanked / len(r.c64), r.bins / r.frames, r.margin, metric, code, doppler))
    assert r.margin >= 1e-4
    assert doppler == 1200.0 and abs(code - s["code0"]) <= 1023.0 / 4096.0 and metric >= 5.0


def raw_check(src=1 << 20, dst=1 << 21, blank=0.0, ratio=12.0, hold=2, nfft=64, guard=2, in_c=0, in_first=0, in_count=1000, out_first=0, n_out=100,
              gain=1.0, cplx=0, cfg=True, ctx=None, dev=False, stats=0, frame_bins=0):
    """gacq_mitigate_check (no context), or gacq_mitigate_dev on ctx; the addresses are only looked at by the checks"""
    st = mitigate.MitigateCfg(blank_thr=blank, ratio=ratio, hold=hold, nfft=nfft, guard=guard)
    args = [ctypes.addressof(st) if cfg else None, ctypes.c_void_p(src), in_c, in_first, in_count, out_first, n_out, gain, cplx, ctypes.c_void_p(dst)]
    if dev:
        return nat.lib.gacq_mitigate_dev(ctx, *args, ctypes.c_void_p(stats), ctypes.c_void_p(frame_bins))
    return nat.lib.gacq_mitigate_check(*args)


def bad_calls():
    """(label, expected code, changed arguments)"""
    nan, inf = float("nan"), float("inf")
    out = [("both stages off", BAD_ARG, dict(nfft=0)),
           ("NULL cfg", BAD_ARG, dict(cfg=False)), ("NULL input", BAD_ARG, dict(src=0)), ("NULL output", BAD_ARG, dict(dst=0)),
           ("complex64 input off 8 bytes", BAD_ARG, dict(in_c=1, src=(1 << 20) + 4)), ("complex64 output off 8 bytes", BAD_ARG, dict(cplx=1, dst=(1 << 21) + 4)),
           ("short input", SHORT_INPUT, dict(in_count=5 * 32 + 2 - 1)), ("short input, blanking alone", SHORT_INPUT, dict(nfft=0, blank=5.0, in_count=101)),
           ("input starts too late", SHORT_INPUT, dict(in_first=1, in_count=999)),
           ("input starts too late for block 2", SHORT_INPUT, dict(out_first=64, in_first=32 - 2 + 1, in_count=900))]
    out += [("nfft %d" % v, BAD_ARG, dict(nfft=v)) for v in (32, 63, 96, 8192, -64)]
    out += [("ratio %r" % v, BAD_ARG, dict(ratio=v)) for v in (1.0, 0.5, -3.0, nan, inf)]
    out += [("blank %r" % v, BAD_ARG, dict(blank=v)) for v in (-1.0, nan, inf)]
    out += [("hold %d" % v, BAD_ARG, dict(hold=v)) for v in (-1, 65)] + [("guard %d" % v, BAD_ARG, dict(guard=v)) for v in (-1, 9)]
    out += [("gain %r" % v, BAD_ARG, dict(gain=v)) for v in (0.0, -1.0, nan, inf, 1e39, 1e-46)]
    for k in ("in_first", "in_count", "out_first", "n_out"):
        out += [("%s %s" % (k, v), BAD_ARG, {k: v}) for v in (-1, (1 << 48) + 1)]
    return out


def test_every_refusal_through_the_raw_abi_without_a_context():
    for label, code, change in bad_calls():
        assert raw_check(**change) == code, (label, nat.lib.gacq_last_error(None))
        assert nat.lib.gacq_last_error(None).startswith(b"gacq_mitigate_dev: "), label      # every message names its own tool
    assert raw_check() == 0 and raw_check(in_count=5 * 32 + 2) == 0 and raw_check(n_out=0, in_count=0) == 0
    assert raw_check(out_first=64, in_first=32 - 2, in_count=900) == 0
    assert raw_check(nfft=0, blank=5.0, in_count=102) == 0
    assert raw_check(dev=True) == BAD_ARG                                 # a good call without a context
    assert [nat.lib.gacq_mitigate_tile(n) for n in (64, 128, 1024, 4096, 32, 100, 8192)] == [C.TILE] * 4 + [BAD_ARG] * 3
    assert ctypes.sizeof(mitigate.MitigateCfg) == 32


def test_out_range_of_the_module_is_the_oracles():
    for cfg, ocfg in ((mitigate.Config(blank=50, hold=7, nfft=128), O.config(blank=50, hold=7, nfft=128)), (mitigate.Config(blank=50, hold=64, nfft=0),
                                                                                                               O.config(blank=50, hold=64, nfft=0))):
        for in_first in (0, 1, 63, 64, 65, 500):
            for count in (0, 1, 100, 191, 192, 193, 199, 200, 1000):
                first, n = cfg.out_range(in_first, count)
                assert (first, n) == O.out_range(ocfg, in_first, count)
                if n:
                    lo, hi = O.needed(ocfg, first, n)
                    assert in_first <= lo and hi < in_first + count and cfg.first_needed(first) == lo
                    assert O.needed(ocfg, first, n + 1)[1] >= in_first + count


def test_command_line_parser_and_report_line():
    a, cfg = mitigate.parse(["in.bin", "out.bin"])
    assert (cfg.blank, cfg.hold, cfg.nfft, cfg.ratio, cfg.guard) == (0.0, 2, 1024, 12.0, 2) and a.gain is None and a.target_rms == 32.0
    assert not a.complex64 and not a.in_complex64 and (a.input_filename, a.output_filename) == ("in.bin", "out.bin")
    a, cfg = mitigate.parse(["--blank", "85", "--hold", "4", "--nfft", "256", "--ratio", "9.5", "--guard", "0", "--in-complex64", "--gain", "2.5",
                             "--complex64", "-", "-"])
    assert (cfg.blank, cfg.hold, cfg.nfft, cfg.ratio, cfg.guard) == (85.0, 4, 256, 9.5, 0) and a.gain == 2.5 and a.complex64 and a.in_complex64
    assert mitigate.parse(["--blank", "85", "--no-excise", "a", "b"])[1].nfft == 0
    for bad in (["--no-excise", "a", "b"], ["--nfft", "100", "a", "b"], ["--ratio", "1", "a", "b"], ["--hold", "65", "a", "b"], ["--guard", "9", "a", "b"],
                ["--blank", "-1", "a", "b"], ["--gain", "0", "a", "b"], ["--gain", "2", "--target-rms", "3", "a", "b"]):
        with pytest.raises(SystemExit):
            mitigate.parse(bad)
    line = mitigate.report_line(mitigate.Config(blank=85.0), 4.7, 15360, 338, 30, 2040)
    assert line == "gain 4.7 samples 15360 blanked %r excised %r" % (338 / 15360.0, 2040 / (30 * 1024.0))
    assert mitigate.report_line(mitigate.Config(blank=85.0, nfft=0), 1.0, 0, 0, 0, 0) == "gain 1.0 samples 0 blanked 0.0 excised 0.0"
