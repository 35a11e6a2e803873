"""B2b tracking with the chip accumulator without a GPU: the numpy oracle against the reference's stdout and track-chips.dat, the
tracker table against the scripts, the regenerated recordings against their SHA-256, the command-line parsing, goldens that reject
plausible accumulator bugs, and the kernel's registers and contraction.  Goldens: tools/make_goldens_chiptrack.py."""
import os
import re
import subprocess

import numpy as np
import pytest

import chiptrack_cases as CC
import track_loop_cases as C
from gnss_dsp_tools_amd import chiptrack, codes, longtrack, track, trackloop

GOLDEN = CC.load()
CASES = sorted(GOLDEN["cases"])
_IQ = {}


def _iq(case_id):
    if case_id not in _IQ:
        _IQ[case_id] = CC.recording(GOLDEN["cases"][case_id])
    return _IQ[case_id]


@pytest.mark.parametrize("case_id", CASES)
def test_oracle_reproduces_golden_lines_and_chips(case_id):
    case = GOLDEN["cases"][case_id]
    _, lines, bins, _ = CC.oracle(case, _iq(case_id))
    ok, worst, wabs = C.lines_match(lines, case["stdout_lines"])
    assert ok, (case_id, len(lines), len(case["stdout_lines"]), worst, wabs)
    want = CC.chips_lines(case)
    assert len(want) == 10230 and chiptrack.format_chips(bins) == want


def test_recordings_match_their_sha256():
    for cid in CASES:
        assert len(_iq(cid)) == 2 * GOLDEN["cases"][cid]["nsamp"]        # CC.recording() asserts the stored SHA-256


def test_golden_cases_cover_scripts_modes_signs_and_ends():
    cases = GOLDEN["cases"]
    assert {c["tracker"] for c in cases.values()} == set(chiptrack.CHIP_TRACKERS)
    assert any("--carrier-phase" in c["argv"] for c in cases.values())
    modes = cases["b2bi_modes"]["argv"]
    wide, narrow = map(float, modes[modes.index("--loop-dwells") + 1].split(","))
    assert wide + narrow < 200 and len(cases["b2bi_modes"]["stdout_lines"]) > 201       # FLL_WIDE -> FLL_NARROW -> PLL, then accum
    for c in cases.values():                   # each recording ends before the block after the last printed one could be read
        assert c["nsamp"] < c["fs"] * 0.001 * (len(c["stdout_lines"]) + 2)
    short = cases["b2bi_short"]
    assert len(short["stdout_lines"]) <= 200 and set(CC.chips_lines(short)) == {"0.000000 0.000000"}
    assert any(c["signs"] == [-1.0, 1.0] for c in cases.values())      # both sign branches of nco.accum


def test_chip_trackers_equal_script_parameters():
    params = GOLDEN["params"]
    assert sorted(params) == sorted(chiptrack.CHIP_TRACKERS) == ["beidou-b2bi", "beidou-b2bq"]
    for name, p in params.items():
        t = chiptrack.CHIP_TRACKERS[name]
        mine = dict(code=t.code, kind=t.kind, spacing=t.spacing, ratio=t.ratio, glonass=t.glonass, period=t.period, rate=t.rate,
                    subs=t.subs, pll=[float(v) for v in t.pll], dll=[float(v) for v in t.dll], fll=list(t.fll), cols=t.cols,
                    fixed_pll=t.fixed_pll, carrier_phase=t.carrier_phase, accum_after=chiptrack.ACCUM_AFTER,
                    chips_file=chiptrack.CHIPS_FILE, code_length=codes.code_length(t.code))
        assert mine == p, (name, {k: (mine[k], p[k]) for k in p if mine[k] != p[k]})
    assert len(trackloop.TRACKERS) == 28
    assert not set(chiptrack.CHIP_TRACKERS) & (set(trackloop.TRACKERS) | set(longtrack.LONG_TRACKERS))


def test_cli_parsing_matches_optparse():
    path, ch = chiptrack.parse("beidou-b2bi", ["--carrier-phase", "-0.214", "f.bin", "69984000", "-15498375", "31", "-1200.5", "831.15"])
    assert path == "f.bin" and ch.fs == 69984000.0 and ch.coffset == -15498375.0 and ch.prn == 31
    assert ch.doppler == -1200.5 and ch.code_offset == 831.15 and ch.carrier_phase == -0.214
    spec = chiptrack.chip_channel_spec(ch)
    assert spec.dwell_wide == 0.0 and spec.dwell_narrow == 0.0 and spec.carrier_phase == -0.214
    assert spec.ratio == 118.0 and spec.kind == 0 and spec.subs == 1 and spec.chip_rate == 10230000.0 and spec.prn == 31
    _, ch = chiptrack.parse("beidou-b2bq", ["--loop-dwells", "3,7", "f", "69984000", "15498375", "19", "1200.0", "831.15"])
    assert ch.loop_dwells == (3.0, 7.0) and ch.carrier_phase is None
    _, ch = chiptrack.parse("beidou-b2bq", ["f", "4092000", "0", "31", "1200.0", "831.15", "--carrier-phase", "0.5"])
    assert ch.carrier_phase is None                                    # interspersed arguments off: a positional
    with pytest.raises(SystemExit):
        chiptrack.parse("beidou-b2bi", ["f", "4092000", "0", "31", "1200.0"])
    with pytest.raises(SystemExit):
        chiptrack.parse("gps-l1", ["f", "4092000", "0", "31", "1200.0", "1.0"])
    with pytest.raises(SystemExit):                                     # track.parse keeps refusing the B2b names
        track.parse("beidou-b2bi", ["f", "4092000", "0", "31", "1200.0", "1.0"])
    with pytest.raises(KeyError):
        chiptrack.chip_channel_spec(trackloop.Channel("gps-l1", 4092000.0, 0.0, 3, 0.0, 10.0))
    for name in chiptrack.CHIP_TRACKERS:
        assert name in track.__doc__ and name in chiptrack.__doc__


def test_format_chips_prints_the_scripts_format():
    z = np.array([0.0, 1.5 - 2.25j, -1e-7 + 3.0000005j], dtype=np.complex128)
    assert chiptrack.format_chips(z) == ["0.000000 0.000000", "1.500000 -2.250000", "-0.000000 3.000001"]


@pytest.mark.parametrize("bug", ["accum_from_200", "ignore_sign", "code_p_after_update"])
def test_goldens_reject_plausible_bugs(bug):
    """Each bug changes the printed bins of a case that accumulates (the records are untouched: the bins do not feed the loop)."""
    bad = 0
    for cid in ("b2bi_modes", "b2bq_carrier_phase"):
        case = GOLDEN["cases"][cid]
        _, lines, bins, _ = CC.oracle(case, _iq(cid), bug=bug)
        assert C.lines_match(lines, case["stdout_lines"])[0]
        got, want = chiptrack.format_chips(bins), CC.chips_lines(case)
        bad += sum(a != b for a, b in zip(got, want))
    assert bad >= 100, (bug, bad)


def test_bins_are_sequential_sums_in_sample_order():
    """The closed-form bins of the accumulated frames equal the reference's repeated addition.  Summing a run out of order is not
    visible in the printed bins ('%f' of sums of a few dozen complex64 values) and gives the same bits on the golden recordings; on
    the GPU batch's recording (tests/test_chiptrack_gpu.py, noise-only channel accumulating from frame 1) it changes a bin's bits,
    so the bit-level comparison of the device's bins with the oracle's rejects it there."""
    from chiptrack_oracle import track
    from oracle import tracking_oracle as T
    import longtrack_cases as LC
    case = GOLDEN["cases"]["b2bq_carrier_phase"]
    spec = chiptrack.chip_channel_spec(CC.channel_of(case))
    trace = []
    _, bins, signs = track(spec, codes.chips("beidou.b2bq", spec.prn), _iq("b2bq_carrier_phase"), trace=trace, max_records=205)
    assert len(trace) == 4 and sorted(signs) == [201, 202, 203, 204] and np.count_nonzero(bins) == 10230
    for code_p, cf, m in trace:
        seq = T.sequential_indices(10230, 0, [code_p], cf, m)[0][0]
        assert np.array_equal(seq, T.closed_form_indices(10230, 0, code_p, cf, m)[0])
    # the GPU batch's recording and last channel (tests/test_chiptrack_gpu.py: SATS, CHANNELS[-1], ACCUM_AFTER[-1])
    fs = 69.984e6
    sats = [("beidou.b2bi", 21, 4.0, 1200.0, 831.15), ("beidou.b2bi", 30, 3.0, -2300.0, 5000.5), ("beidou.b2bq", 19, 4.0, 700.0, 9000.25),
            ("beidou.b2bq", 33, 3.0, -400.0, 2222.75), ("beidou.b2bi", 45, 3.0, 3100.0, 7777.0)]
    host = LC.synth_many(fs, 0.045, sats, 5150, noise=12.0)
    spec = chiptrack.chip_channel_spec(trackloop.Channel("beidou-b2bq", fs, 0.0, 40, 500.0, 100.5, (4.0, 6.0)))
    chips01 = codes.chips("beidou.b2bq", 40)
    _, fwd, _ = track(spec, chips01, host, accum_after=0)
    _, rev, _ = track(spec, chips01, host, accum_after=0, bug="runs_out_of_order")
    assert rev.tobytes() != fwd.tobytes()


def _hipcc(*args):
    src = os.path.join(os.path.dirname(C.HERE), "gnss-dsp-tools_amd", "csrc", "gacq_chiptrack.hip")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I/opt/rocm/include"] + list(args) + [src],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return r


def test_chip_track_kernel_has_no_scratch_no_spills_no_agprs():
    r = _hipcc("-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull)
    blocks = re.split(r"remark: [^\n]*Function Name: ", r.stderr)[1:]
    blocks = [b for b in blocks if "chip_track_kernel" in b.split("\n")[0]]
    assert len(blocks) == 1
    b = blocks[0]
    val = lambda k: int(re.search(k + r": (\d+)", b).group(1))
    assert val(r"ScratchSize \[bytes/lane\]") == 0 and val("VGPRs Spill") == 0 and val("SGPRs Spill") == 0 and val("AGPRs") == 0, b


def test_chiptrack_file_is_not_contracted(tmp_path):
    ll = str(tmp_path / "ct.ll")
    _hipcc("--cuda-device-only", "-S", "-emit-llvm", "-o", ll)
    ir = open(ll).read()
    assert "chip_track_kernel" in ir
    contracted = re.findall(r"= (?:fmul|fadd|fsub) contract", ir)
    assert not contracted and "llvm.fmuladd" not in ir, contracted[:5]
    src = open(os.path.join(os.path.dirname(C.HERE), "gnss-dsp-tools_amd", "csrc", "gacq_chiptrack.hip")).read()
    assert [l for l in src.split("\n") if l.startswith("#")][0] == "#pragma clang fp contract(off)"
