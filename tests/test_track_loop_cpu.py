"""Tracking loops without a GPU: the numpy oracle against the reference's own output lines, the tracker table against the scripts,
the command-line parsing, and bounds that reject plausible bugs.  Goldens: tools/make_goldens_trackloop.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import track_loop_cases as C
from gnss_dsp_tools_amd import codes, track, trackloop

GOLDEN = C.load()
CASES = sorted(GOLDEN["cases"])


def _oracle(case_id, **kw):
    case = GOLDEN["cases"][case_id]
    ch = C.channel_of(case)
    spec = kw.pop("spec", None) or trackloop.channel_spec(ch)
    chips = codes.chips(trackloop.TRACKERS[ch.name].code, spec.prn)
    return C.oracle_lines(ch.name, spec, chips, C.recording(case), **kw)[1]


@pytest.mark.parametrize("case_id", CASES)
def test_oracle_reproduces_golden_lines(case_id):
    """Every line of the reference's stdout: integer columns exact, floats within the bound of track_loop_cases (half a printed digit
    plus 1e-9 relative); measured: every line of every case prints identically."""
    want = GOLDEN["cases"][case_id]["stdout_lines"]
    got = _oracle(case_id)
    ok, worst, wabs = C.lines_match(got, want)
    assert ok, (case_id, worst, wabs, got[:2], want[:2])
    assert len(want) >= 10


def test_golden_cases_cover_modes_columns_and_partial_block():
    cases = GOLDEN["cases"]
    names = {c["tracker"] for c in cases.values()}
    assert {"gps-l1", "xona-x1d", "galileo-e1b", "gps-l1cp", "beidou-b1cd", "gps-l2cm", "glonass-l1", "gps-l5i"} <= names
    assert any("--carrier-phase" in c["argv"] for c in cases.values())
    assert any(c["prn"] < 0 for c in cases.values() if c["tracker"].startswith("glonass"))
    for cid, c in cases.items():
        t = trackloop.TRACKERS[c["tracker"]]
        assert all(len(l.split()) == t.cols for l in c["stdout_lines"]), cid
        if "--loop-dwells" in c["argv"] and not t.fixed_pll:
            wide, narrow = map(float, c["argv"][c["argv"].index("--loop-dwells") + 1].split(","))
            assert len(c["stdout_lines"]) > wide + narrow, cid          # all three modes occur
    # the B1C recording ends inside a block: the reference stops there, with samples left over
    b = cases["beidou_b1cd"]
    assert b["nsamp"] > 30 * int(b["fs"] * 0.001) + int(b["fs"] * 0.01 * (10230 - b["code_offset"]) / 10230)


def test_trackers_equal_script_parameters():
    """TRACKERS holds exactly the 28 template scripts, with the constants read off each script's source."""
    params = GOLDEN["params"]
    assert sorted(params) == sorted(trackloop.TRACKERS) and len(params) == 28
    for name, p in params.items():
        t = trackloop.TRACKERS[name]
        mine = dict(code=t.code, kind=t.kind, spacing=t.spacing, ratio=t.ratio, glonass=list(t.glonass) if t.glonass else None,
                    period=t.period, rate=t.rate, subs=t.subs, pll=[float(v) for v in t.pll], dll=[float(v) for v in t.dll],
                    fll=list(t.fll), cols=t.cols, fixed_pll=t.fixed_pll, carrier_phase=t.carrier_phase)
        assert mine == p, (name, {k: (mine[k], p[k]) for k in p if mine[k] != p[k]})
        assert codes.code_length(t.code) <= 10240


def test_cli_parsing_matches_optparse():
    """Interspersed arguments off, as the scripts have it: negative positionals are values, and so is a negative option value."""
    path, ch = track.parse("glonass-l1", ["--carrier-phase", "-0.214", "f.bin", "69984000", "-9334875", "-7", "-1200.5", "381.1"])
    assert path == "f.bin" and ch.fs == 69984000.0 and ch.coffset == -9334875.0 and ch.prn == -7
    assert ch.doppler == -1200.5 and ch.code_offset == 381.1 and ch.carrier_phase == -0.214
    _, ch = track.parse("gps-l1", ["f", "4092000", "0", "31", "1200.0", "831.15"])
    assert ch.loop_dwells == (500.0, 500.0) and ch.carrier_phase is None
    _, ch = track.parse("gps-l1", ["--loop-dwells", "3,7", "f", "4092000", "-1", "31", "-1", "831.15"])
    assert ch.loop_dwells == (3.0, 7.0) and ch.coffset == -1.0 and ch.doppler == -1.0
    with pytest.raises(SystemExit):
        track.parse("gps-l1", ["f", "4092000", "0", "31", "1200.0"])
    with pytest.raises(SystemExit):
        track.parse("beidou-b2bi", ["f", "4092000", "0", "31", "1200.0", "1.0"])
    spec = trackloop.channel_spec(track.parse("glonass-l1", ["--carrier-phase", "0.25", "f", "2.5e6", "180000", "-3", "0", "1"])[1])
    assert spec.dwell_wide == 0.0 and spec.dwell_narrow == 0.0 and spec.carrier_phase == 0.25
    assert spec.ratio == (1602.0 + 0.5625 * -3) / 0.511 and spec.fm == -(180000.0 + 562500 * -3) / 2.5e6
    spec = trackloop.channel_spec(track.parse("glonass-l3ocd", ["--carrier-phase", "0.25", "f", "2.5e6", "0", "3", "0", "1"])[1])
    assert spec.carrier_phase == 0.0 and spec.dwell_wide == 0.0       # carrier_p=0 in the script, dwells still zeroed


def _spec_with(case_id, **fields):
    spec = trackloop.channel_spec(C.channel_of(GOLDEN["cases"][case_id]))
    out = trackloop.TrackSpec()
    ctypes.memmove(ctypes.byref(out), ctypes.byref(spec), ctypes.sizeof(spec))
    for k, v in fields.items():
        setattr(out, k, v(getattr(spec, k)) if callable(v) else v)
    return out


@pytest.mark.parametrize("bug", ["block_length", "early_late_swapped", "carrier_ratio", "mode_switch_late"])
@pytest.mark.parametrize("case_id", ["gps_l1", "galileo_e1b"])
def test_bounds_reject_plausible_bugs(case_id, bug):
    want = GOLDEN["cases"][case_id]["stdout_lines"]
    if bug == "block_length":
        got = _oracle(case_id, n_bias=1)
    elif bug == "early_late_swapped":
        got = _oracle(case_id, spec=_spec_with(case_id, spacing=lambda s: -s))
    elif bug == "carrier_ratio":
        got = _oracle(case_id, spec=_spec_with(case_id, ratio=lambda r: 1557.5))
    else:
        subs = trackloop.TRACKERS[GOLDEN["cases"][case_id]["tracker"]].subs          # modes switch once per outer block
        got = _oracle(case_id, spec=_spec_with(case_id, dwell_wide=lambda w: w + subs, dwell_narrow=lambda n: n - subs))
    ok, worst, _ = C.lines_match(got, want)
    assert not ok and worst > 100, (bug, worst)


def _hipcc(*args):
    src = os.path.join(os.path.dirname(C.HERE), "gnss-dsp-tools_amd", "csrc", "gacq_trackloop.hip")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I/opt/rocm/include"] + list(args) + [src],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return r


def test_track_loop_kernel_has_no_scratch_no_spills_no_agprs():
    """The new kernel keeps everything in registers and LDS: no private segment, no VGPR or SGPR spills, no accumulator registers."""
    r = _hipcc("-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull)
    blocks = re.split(r"remark: [^\n]*Function Name: ", r.stderr)[1:]
    blocks = [b for b in blocks if "track_loop_kernel" in b.split("\n")[0]]
    assert len(blocks) == 1
    b = blocks[0]
    val = lambda k: int(re.search(k + r": (\d+)", b).group(1))
    assert val(r"ScratchSize \[bytes/lane\]") == 0 and val("VGPRs Spill") == 0 and val("SGPRs Spill") == 0 and val("AGPRs") == 0, b


def test_wipe_off_and_correlator_sums_are_not_contracted(tmp_path):
    """Each wipe-off product and each correlator term is rounded on its own, as the reference computes them: no floating-point
    multiply, add or subtract of the device code may carry the `contract` flag (which lets the backend fuse it into v_fma_f64), and the
    per-sample loop of track_loop_kernel holds no fused multiply-add beyond the nine intended closed-form phases (three per
    correlator).  The other v_fmac_f64 there multiply by the literal -2^32 (0xc1f00000): the backend's exact split of an fp64 value
    into the two halves of an int64 conversion."""
    ll = str(tmp_path / "tl.ll")
    _hipcc("--cuda-device-only", "-S", "-emit-llvm", "-o", ll)
    ir = open(ll).read()
    contracted = re.findall(r"= (?:fmul|fadd|fsub) contract", ir)
    assert not contracted and "llvm.fmuladd" not in ir, contracted[:5]
    asm_path = str(tmp_path / "tl.s")
    _hipcc("--cuda-device-only", "-S", "-o", asm_path)
    asm = open(asm_path).read()
    kernel = asm[asm.index("track_loop_kernel"):]
    kernel = kernel[:kernel.index("s_endpgm")]
    blocks, cur = [], None
    for line in kernel.split("\n"):
        if re.match(r"^\.LBB\d+_\d+:", line):
            m = re.search(r"Depth=(\d+)", line)
            cur = []
            blocks.append((int(m.group(1)) if m else 0, cur))
        elif cur is not None and line.startswith("\t") and not line.startswith("\t."):
            cur.append(line.strip())
    depth = max(d for d, _ in blocks)
    assert depth == 3                                   # outer blocks > sub-blocks > samples
    loop = [i for d, b in blocks if d == depth for i in b]
    fused = [i for i in loop if re.match(r"v_fmac?_f64", i)]
    phases = [i for i in fused if "0xc1f00000" not in i]
    assert 3 <= len(phases) <= 9, phases
    muls = [i for i in loop if i.startswith("v_mul_f64")]
    assert len(muls) >= 8 + 6, muls                  # two complex products (8) and the six correlator terms
