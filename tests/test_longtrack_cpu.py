"""Long-code tracking loops without a GPU: the numpy oracle against the reference's own output lines, the tracker table against the
scripts, the regenerated recordings against their SHA-256, the command-line parsing, bounds that reject plausible bugs, and the
kernel's registers and contraction.  Goldens: tools/make_goldens_longtrack.py."""
import ctypes
import os
import re
import subprocess

import pytest

import longtrack_cases as LC
import track_loop_cases as C
from gnss_dsp_tools_amd import codes, longtrack, track, trackloop

GOLDEN = LC.load()
CASES = sorted(GOLDEN["cases"])
_IQ = {}


def _iq(case_id):
    if case_id not in _IQ:
        _IQ[case_id] = LC.recording(GOLDEN["cases"][case_id])
    return _IQ[case_id]


def _oracle(case_id, spec=None, **kw):
    case = GOLDEN["cases"][case_id]
    ch = LC.channel_of(case)
    spec = spec or longtrack.long_channel_spec(ch)
    chips = codes.chips(longtrack.LONG_TRACKERS[ch.name].code, spec.prn)
    return LC.oracle_lines(ch.name, spec, chips, _iq(case_id), **kw)[1]


@pytest.mark.parametrize("case_id", CASES)
def test_oracle_reproduces_golden_lines(case_id):
    """Every line of the reference's stdout: integer columns exact, floats within track_loop_cases' bound."""
    want = GOLDEN["cases"][case_id]["stdout_lines"]
    got = _oracle(case_id)
    ok, worst, wabs = C.lines_match(got, want)
    assert ok, (case_id, len(got), len(want), worst, wabs, got[:2], want[:2])
    assert len(want) >= 1000


def test_recordings_match_their_sha256():
    for cid in CASES:
        iq = _iq(cid)                                            # LC.recording() asserts the stored SHA-256
        assert len(iq) == 2 * GOLDEN["cases"][cid]["nsamp"]


def test_long_trackers_equal_script_parameters():
    """LONG_TRACKERS holds the three long-code scripts, with the constants read off each script's source."""
    params = GOLDEN["params"]
    assert sorted(params) == sorted(longtrack.LONG_TRACKERS) == ["glonass-l1-p", "glonass-l2-p", "gps-l2cl"]
    for name, p in params.items():
        t = longtrack.LONG_TRACKERS[name]
        mine = dict(code=t.code, kind=t.kind, spacing=t.spacing, ratio=t.ratio, glonass=list(t.glonass) if t.glonass else None,
                    period=t.period, rate=t.rate, subs=t.subs, pll=[float(v) for v in t.pll], dll=[float(v) for v in t.dll],
                    fll=list(t.fll), cols=t.cols, fixed_pll=t.fixed_pll, carrier_phase=t.carrier_phase)
        assert mine == p, (name, {k: (mine[k], p[k]) for k in p if mine[k] != p[k]})
    assert longtrack.LONG_TRACKERS["gps-l2cl"].rate == 1.0 / 1.500
    assert not set(longtrack.LONG_TRACKERS) & set(trackloop.TRACKERS)


def _modes(case):
    """the mode of each outer block, as the script switches it against the record counter"""
    argv = case["argv"]
    wide, narrow = (0.0, 0.0) if "--carrier-phase" in argv else map(float, argv[argv.index("--loop-dwells") + 1].split(","))
    subs = longtrack.LONG_TRACKERS[case["tracker"]].subs
    out = []
    for b in range(len(case["stdout_lines"]) // subs):
        r = b * subs
        out.append("PLL" if r >= wide + narrow else ("FLL_NARROW" if r >= wide else "FLL_WIDE"))
    return out


def test_golden_cases_cover_scripts_modes_and_partial_block():
    cases = GOLDEN["cases"]
    assert {c["tracker"] for c in cases.values()} == set(longtrack.LONG_TRACKERS)
    assert any("--carrier-phase" in c["argv"] for c in cases.values())
    assert any(c["prn"] < 0 for c in cases.values() if c["tracker"].startswith("glonass"))
    modes = set()
    for code in ("gps.l2cl", "glonass.p"):
        two = [c for c in cases.values() if longtrack.LONG_TRACKERS[c["tracker"]].code == code
               and len(c["stdout_lines"]) == 2 * longtrack.LONG_TRACKERS[c["tracker"]].subs]
        assert two, code
        assert any(len(set(_modes(c))) == 2 for c in two), code             # the mode switches between the two outer blocks
    for c in cases.values():
        modes |= set(_modes(c))
        assert all(len(l.split()) == 9 for l in c["stdout_lines"])
    assert modes == {"FLL_WIDE", "FLL_NARROW", "PLL"}
    # the L2CL recording ends inside its third outer block: the reference prints nothing for it
    c = cases["gps_l2cl"]
    assert c["nsamp"] > c["fs"] * (3.0 + 0.5)


def test_cli_parsing_matches_optparse():
    """Interspersed arguments off, as the scripts have it: negative positionals are values, and so is a negative option value."""
    path, ch = track.parse("glonass-l1-p", ["--carrier-phase", "-0.214", "f.bin", "69984000", "17245125", "-7", "-1200.5", "1841430.6"])
    assert path == "f.bin" and ch.fs == 69984000.0 and ch.coffset == 17245125.0 and ch.prn == -7
    assert ch.doppler == -1200.5 and ch.code_offset == 1841430.6 and ch.carrier_phase == -0.214
    spec = longtrack.long_channel_spec(ch)
    assert spec.dwell_wide == 0.0 and spec.dwell_narrow == 0.0 and spec.carrier_phase == -0.214
    assert spec.ratio == (1602.0 + 0.5625 * -7) / 5.11 and spec.fm == -(17245125.0 + 562500 * -7) / 69984000.0 and spec.prn == 0
    _, ch = track.parse("glonass-l2-p", ["f", "69984000", "18272874", "4", "1200.0", "4220621.7"])
    spec = longtrack.long_channel_spec(ch)
    assert ch.loop_dwells == (500.0, 500.0) and ch.carrier_phase is None
    assert spec.ratio == (1246.0 + 0.4375 * 4) / 5.11 and spec.fm == -(18272874.0 + 437500 * 4) / 69984000.0
    assert spec.subs == 1000 and spec.period == 1.0 and spec.rate == 1.0 and spec.glonass == 1
    _, ch = track.parse("gps-l2cl", ["--loop-dwells", "3,7", "f", "4092000", "-1", "31", "-1", "831.15"])
    spec = longtrack.long_channel_spec(ch)
    assert ch.loop_dwells == (3.0, 7.0) and ch.coffset == -1.0 and ch.doppler == -1.0 and spec.prn == 31
    assert spec.kind == 5 and spec.ratio == 2400.0 and spec.subs == 1500 and spec.rate == 1.0 / 1.500 and spec.chip_rate == 511500.0
    # interspersed arguments off: an option after the first positional is a positional
    _, ch = track.parse("gps-l2cl", ["f", "4092000", "0", "31", "1200.0", "831.15", "--carrier-phase", "0.5"])
    assert ch.carrier_phase is None
    with pytest.raises(SystemExit):
        track.parse("glonass-l1-p", ["f", "4092000", "0", "3", "1200.0"])
    with pytest.raises(SystemExit):
        track.parse("beidou-b2bi", ["f", "4092000", "0", "31", "1200.0", "1.0"])
    with pytest.raises(KeyError):
        trackloop.channel_spec(trackloop.Channel("gps-l2cl", 4092000.0, 0.0, 3, 0.0, 10.0))
    with pytest.raises(KeyError):
        longtrack.long_channel_spec(trackloop.Channel("gps-l1", 4092000.0, 0.0, 3, 0.0, 10.0))
    for name in longtrack.LONG_TRACKERS:
        assert name in track.names() and name in track.__doc__


def _spec_with(case_id, **fields):
    spec = longtrack.long_channel_spec(LC.channel_of(GOLDEN["cases"][case_id]))
    out = trackloop.TrackSpec()
    ctypes.memmove(ctypes.byref(out), ctypes.byref(spec), ctypes.sizeof(spec))
    for k, v in fields.items():
        setattr(out, k, v(getattr(spec, k)) if callable(v) else v)
    return out


@pytest.mark.parametrize("case_id,bug", [("glonass_l1_p", "floor_boundaries"), ("glonass_l1_p", "divisor_0.511"),
                                         ("glonass_l1_p", "early_late_swapped"), ("glonass_l1_p", "modes_per_sub_block"),
                                         ("gps_l2cl", "floor_boundaries"), ("gps_l2cl", "modes_per_sub_block")])
def test_bounds_reject_plausible_bugs(case_id, bug):
    """Each plausible bug moves some printed column by at least 1e-3, far outside the bound."""
    want = GOLDEN["cases"][case_id]["stdout_lines"]
    if bug == "divisor_0.511":
        ch = LC.channel_of(GOLDEN["cases"][case_id])
        base, step, _, _ = longtrack.LONG_TRACKERS[ch.name].glonass
        got = _oracle(case_id, spec=_spec_with(case_id, ratio=(base + step * ch.prn) / 0.511))
    elif bug == "early_late_swapped":
        got = _oracle(case_id, spec=_spec_with(case_id, spacing=lambda s: -s))
    else:
        got = _oracle(case_id, bug=bug)
    ok, worst, wabs = C.lines_match(got, want)
    assert not ok and wabs >= 1e-3, (bug, worst, wabs)


def _hipcc(*args):
    src = os.path.join(os.path.dirname(C.HERE), "gnss-dsp-tools_amd", "csrc", "gacq_longtrack.hip")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I/opt/rocm/include"] + list(args) + [src],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return r


def test_longtrack_kernel_has_no_scratch_no_spills_no_agprs():
    r = _hipcc("-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull)
    blocks = re.split(r"remark: [^\n]*Function Name: ", r.stderr)[1:]
    blocks = [b for b in blocks if "longtrack_kernel" in b.split("\n")[0]]
    assert len(blocks) == 1
    b = blocks[0]
    val = lambda k: int(re.search(k + r": (\d+)", b).group(1))
    assert val(r"ScratchSize \[bytes/lane\]") == 0 and val("VGPRs Spill") == 0 and val("SGPRs Spill") == 0 and val("AGPRs") == 0, b


def test_longtrack_file_is_not_contracted(tmp_path):
    """No floating-point multiply, add or subtract of the file's device code carries the `contract` flag, and nothing is a fmuladd:
    each wipe-off product and correlator term is rounded on its own."""
    ll = str(tmp_path / "lt.ll")
    _hipcc("--cuda-device-only", "-S", "-emit-llvm", "-o", ll)
    ir = open(ll).read()
    assert "longtrack_kernel" in ir
    contracted = re.findall(r"= (?:fmul|fadd|fsub) contract", ir)
    assert not contracted and "llvm.fmuladd" not in ir, contracted[:5]
    src = open(os.path.join(os.path.dirname(C.HERE), "gnss-dsp-tools_amd", "csrc", "gacq_longtrack.hip")).read()
    first = [l for l in src.split("\n") if l.startswith("#")][0]
    assert first == "#pragma clang fp contract(off)"
