"""The correlation-grid kernel (csrc/gacq_corrgrid.hip) against the numpy fp64 oracle, its argument checks through the raw ABI, its
bit-identity across batching, and refine() on the device against the same estimator on the oracle's grid.

Grid bound: max |C_dev - C_oracle| <= 1e-5 max |C_oracle| per candidate (the project's fp32 parity bar; with 64-bit phase reduction
the expected error is below 1e-6 of the peak).  refine() bounds: |dc| <= 1e-3 of the code step and |df| <= 0.05 Hz, which follow from
the grid bound (a triangle peak's parabola denominator is about twice the code step times the peak; the differential angle moves by a
few 1e-5 rad) with an order of magnitude to spare, for inputs whose oracle argmax leads its runner-up by more than 1e-4 relative."""
import ctypes

import numpy as np
import pytest

import handoff_cases as H
import refine_oracle as O
from gnss_dsp_tools_amd import _native as nat
from gnss_dsp_tools_amd import acquire, codes, refine, trackloop

MS = 70
COFFSET = 250000.0
# one satellite per correlator kind, so that every kind's grid has a peak and not only noise
SATS = [dict(tracker="gps-l1", item=7, amp=3.0, doppler=1234.5, code0=417.37),
        dict(tracker="gps-l1cd", item=4, amp=3.0, doppler=-820.0, code0=9800.6),
        dict(tracker="galileo-e1b", item=11, amp=3.0, doppler=2210.3, code0=2999.63),
        dict(tracker="gps-l1cp", item=9, amp=3.0, doppler=-1500.0, code0=5000.2),
        dict(tracker="gps-l2cm", item=5, amp=3.0, doppler=640.0, code0=3.4),
        dict(tracker="glonass-l1", item=-5, amp=3.0, doppler=777.7, code0=301.81)]
FS = (6.0e6, 5.9995e6)                     # n = 6000 and n = 5999: not a multiple of the wave or of any vector width


def _grid(tracker, item, fs, D, P, M, s0, doppler0, code0, df=50.0, dc=0.05, offsets=None):
    t = trackloop.TRACKERS[tracker]
    off = (np.arange(P) - (P - 1) / 2.0) * dc if offsets is None else np.asarray(offsets, dtype=np.float64)
    return refine.Grid(code=t.code, prn=0 if t.glonass else item, kind=t.kind, n=int(fs * 0.001), M=M, D=D, fs=fs,
                       carrier_hz=H.carrier_hz(tracker, item, COFFSET), chip_rate=float(codes.chip_rate(t.code)), ratio=t.scale(item),
                       doppler0=doppler0, code0=code0, df=df, s0=s0, offsets=off)


def _cases():
    """(label, recording index, Grid).  Kinds 0-4 x the four (D, P) shapes, cycling over the two sample rates, odd and even first
    samples, M = 1 and 3; then the code-phase and carrier edge cases."""
    out = []
    shapes = ((1, 1), (5, 10), (7, 13), (33, 33))
    k = 0
    for sat in SATS[:5]:
        for D, P in shapes:
            r = k % 2
            s0 = (1001, 2500, 37, 14)[k % 4] + 13 * k
            out.append(("%s D%d P%d" % (sat["tracker"], D, P), r,
                        _grid(sat["tracker"], sat["item"], FS[r], D, P, (1, 3)[(k // 2) % 2], s0, sat["doppler"] + 30.0, sat["code0"] + 0.03)))
            k += 1
    # gps.ca (1023 chips, 1 ms) wraps inside every block; gps.l1cd (10230 chips, 10 ms) does not from code0 = 100 over 3 ms, and does
    # from 9800.6 + cf s0 on
    out.append(("l1cd no wrap", 0, _grid("gps-l1cd", 4, FS[0], 5, 10, 3, 1000, -820.0, 100.0)))
    out.append(("l1cd wraps", 0, _grid("gps-l1cd", 4, FS[0], 5, 10, 3, 2221, -820.0, 9800.6)))
    # code0 + off negative, and beyond L
    out.append(("negative code phase", 1, _grid("gps-l1", 7, FS[1], 5, 10, 3, 777, 1234.5, 0.11, offsets=np.linspace(-2.5, 0.5, 10))))
    out.append(("code phase beyond L", 0, _grid("gps-l1", 7, FS[0], 5, 10, 1, 778, 1234.5, 1022.7, offsets=np.linspace(-0.5, 1500.25, 10))))
    out.append(("negative start phase", 0, _grid("galileo-e1b", 11, FS[0], 5, 10, 1, 4001, 2210.3, -7.25)))
    # GLONASS channel -5: the carrier is 250000 - 2812500 Hz
    out.append(("glonass -5", 0, _grid("glonass-l1", -5, FS[0], 7, 13, 3, 3333, 777.7 - 40.0, 301.81 + 0.1)))
    out.append(("glonass -5 odd n", 1, _grid("glonass-l1", -5, FS[1], 5, 10, 3, 10001, 777.7 + 20.0, 301.81)))
    return out


CASES = _cases()


def _chips(g):
    return codes.chips(g.code, g.prn)


@pytest.fixture(scope="module")
def setup():
    torch = nat.require_torch()
    eng = acquire.default_engine()
    host = [H.recording(21 + r, fs, int(fs * MS * 0.001), COFFSET, SATS) for r, fs in enumerate(FS)]
    dev = [torch.from_numpy(x).to("cuda:%d" % eng.device) for x in host]
    got = refine.corr_grid([g for _, _, g in CASES], [dev[r] for _, r, _ in CASES], eng)
    want = [O.grid(g, _chips(g), host[r]) for _, r, g in CASES]
    return dict(eng=eng, host=host, dev=dev, got=got, want=want)


@pytest.mark.gpu
def test_grid_matches_oracle(setup):
    assert {g.kind for _, _, g in CASES} == {0, 1, 2, 3, 4} and {g.n for _, _, g in CASES} == {6000, 5999}
    assert {g.s0 % 2 for _, _, g in CASES} == {0, 1} and {g.M for _, _, g in CASES} == {1, 3}
    assert {(g.D, g.P) for _, _, g in CASES} >= {(1, 1), (5, 10), (7, 13), (33, 33)}
    worst = 0.0
    for (label, _, g), got, want in zip(CASES, setup["got"], setup["want"]):
        assert got.shape == want.shape == (g.M, g.D, g.P)
        rel = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
        print("%-28s max |dC| / max |C| = %.3g" % (label, rel))
        worst = max(worst, rel)
    print("worst ratio over %d candidates: %.3g" % (len(CASES), worst))
    for (label, _, g), got, want in zip(CASES, setup["got"], setup["want"]):
        assert np.max(np.abs(got - want)) <= 1e-5 * np.max(np.abs(want)), label


def _raw(eng, grids, tensors, out=None):
    """gacq_corr_grid_dev through the raw ABI: (return code, output buffer)"""
    K = len(grids)
    specs = (refine.GridSpec * K)()
    ptrs = (ctypes.c_void_p * K)()
    avail = np.zeros(K, dtype=np.int64)
    keep = []
    for k, (g, x) in enumerate(zip(grids, tensors)):
        off = np.ascontiguousarray(g.offsets, dtype=np.float64)
        keep.append(off)
        specs[k] = refine.GridSpec(code=g.code.encode(), prn=g.prn, kind=g.kind, n=g.n, M=g.M, D=g.D, P=getattr(g, "P_raw", len(off)), fs=g.fs,
                                   carrier_hz=g.carrier_hz, chip_rate=g.chip_rate, ratio=g.ratio, doppler0=g.doppler0, code0=g.code0, df=g.df,
                                   s0=g.s0, offsets=off.ctypes.data)
        ptrs[k] = x.data_ptr()
        avail[k] = x.numel() // 2
    if out is None:
        out = np.full(sum(max(g.M, 1) * 33 * 33 for g in grids), np.nan + 0j, dtype=np.complex128)
    eng.use_torch_stream()
    rc = nat.lib.gacq_corr_grid_dev(eng._ctx, specs, K, ptrs, avail.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p))
    return rc, out


@pytest.mark.gpu
def test_recording_end_and_short_recording(setup):
    torch = nat.require_torch()
    eng = setup["eng"]
    g = _grid("gps-l1", 7, FS[1], 5, 10, 3, 1001, 1234.5, 417.4)
    need = g.s0 + g.M * g.n
    exact = torch.from_numpy(setup["host"][1][:2 * need].copy()).to("cuda:%d" % eng.device)        # its last block ends on the last sample
    assert exact.numel() == 2 * need
    got = refine.corr_grid([g], [exact], eng)[0]
    want = O.grid(g, _chips(g), setup["host"][1])
    assert np.max(np.abs(got - want)) <= 1e-5 * np.max(np.abs(want))
    short = torch.from_numpy(setup["host"][1][:2 * (need - 1)].copy()).to("cuda:%d" % eng.device)
    rc, out = _raw(eng, [g], [short])
    assert rc == -6 and nat.ERRORS[rc] == "GACQ_ERR_SHORT_INPUT"
    assert np.all(np.isnan(out.real)), "the output was written"
    with pytest.raises(nat.GacqError, match="SHORT_INPUT"):
        refine.corr_grid([g], [short], eng)
    # a short candidate among good ones stops the whole call
    rc, out = _raw(eng, [g, g], [exact, short])
    assert rc == -6 and np.all(np.isnan(out.real))


@pytest.mark.gpu
def test_arguments_checked_before_launch(setup):
    eng = setup["eng"]
    x = setup["dev"][0]
    good = _grid("gps-l1", 7, FS[0], 5, 10, 3, 1001, 1234.5, 417.4)
    rc, _ = _raw(eng, [good], [x])
    assert rc == 0
    nan, inf = float("nan"), float("inf")
    bad = [dict(n=0), dict(n=-5), dict(M=0), dict(D=0), dict(D=34), dict(P_raw=0), dict(P_raw=34), dict(fs=nan), dict(fs=inf), dict(fs=0.0),
           dict(df=nan), dict(df=inf), dict(doppler0=nan), dict(doppler0=-inf), dict(code0=nan), dict(code0=inf), dict(ratio=0.0),
           dict(ratio=nan), dict(kind=6), dict(s0=-1), dict(offsets=np.array([0.0, nan] + [0.0] * 8))]
    for change in bad:
        g = refine.Grid(**{**good.__dict__, **{k: v for k, v in change.items() if k != "P_raw"}})
        if "P_raw" in change:
            g.P_raw = change["P_raw"]
        rc, out = _raw(eng, [good, g], [x, x])
        assert rc == -1, (change, rc)
        assert np.all(np.isnan(out.real)), change
    rc, _ = _raw(eng, [refine.Grid(**{**good.__dict__, "code": "gps.nope"})], [x])
    assert rc == -2
    rc, _ = _raw(eng, [refine.Grid(**{**good.__dict__, "prn": 1000})], [x])
    assert rc < 0 and nat.ERRORS[rc] in ("GACQ_ERR_BAD_PRN", "GACQ_ERR_BAD_ARG")
    assert nat.lib.gacq_corr_grid_dev(eng._ctx, None, 0, None, None, None) == -1


@pytest.mark.gpu
def test_bit_identity(setup):
    eng = setup["eng"]
    pick = [5, 3, 14, 20, 25]                        # l1cd (5, 10), gps-l1 (33, 33), l1cp (7, 13), l1cd no wrap, glonass
    grids = [CASES[k][2] for k in pick]
    tens = [setup["dev"][CASES[k][1]] for k in pick]
    among = refine.corr_grid(grids, tens, eng)
    for k, a in zip(pick, among):
        assert a.tobytes() == setup["got"][k].tobytes(), CASES[k][0]                 # among five == among all
    alone = refine.corr_grid([grids[2]], [tens[2]], eng)[0]
    assert alone.tobytes() == among[2].tobytes()
    # two candidates on one tensor == each on a private copy
    a, b = CASES[1][2], CASES[9][2]                  # gps-l1 and galileo-e1b (5, 10), both on recording 1
    assert CASES[1][1] == CASES[9][1] == 1
    shared = refine.corr_grid([a, b], [setup["dev"][1], setup["dev"][1]], eng)
    private = refine.corr_grid([a, b], [setup["dev"][1].clone(), setup["dev"][1].clone()], eng)
    assert shared[0].tobytes() == private[0].tobytes() and shared[1].tobytes() == private[1].tobytes()
    again = refine.corr_grid(grids, tens, eng)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(again, among))


@pytest.mark.gpu
def test_refine_on_device_matches_estimator_on_oracle_grid(setup):
    eng = setup["eng"]
    x, xd, fs = setup["host"][0], setup["dev"][0], FS[0]
    cands = [refine.Candidate("gps-l1", 7, fs, COFFSET, 1234.5 + 80.0, 417.37 - 0.12, 200.0, 0.25),
             refine.Candidate("galileo-e1b", 11, fs, COFFSET, 2210.3 - 20.0, 2999.63 + 0.03, 50.0, 1.023e6 / 8.192e6),
             refine.Candidate("glonass-l1", -5, fs, COFFSET, 777.7 + 60.0, 301.81 - 0.01, 200.0, 0.511e6 / 16.384e6),
             refine.Candidate("gps-l2cm", 5, fs, COFFSET, 640.0 - 70.0, 3.4 + 0.1, 200.0, 0.25)]
    chips = [codes.chips(g.code, g.prn) for g in (refine.default_grid(c) for c in cands)]

    def oracle_fn(grids):
        return [O.grid(g, ch, x) for g, ch in zip(grids, chips)]

    # precondition: the oracle's argmax leads its runner-up by more than 1e-4 relative
    for C in oracle_fn([refine.default_grid(c) for c in cands]):
        S = np.sort(np.abs(C).sum(axis=0)[:, :-1].ravel())
        assert S[-1] - S[-2] > 1e-4 * S[-1]
    want = refine.estimate(cands, oracle_fn, [len(x) // 2] * len(cands))
    got = refine.refine(cands, xd, engine=eng)
    for c, g, w in zip(cands, got, want):
        dc = c.code_res / 4.0
        print("%s: dc %.3g of the code step, df %.3g Hz (ratio %.1f)" % (c, abs(g.code_offset - w.code_offset) / dc, abs(g.doppler - w.doppler), g.ratio))
        assert (g.d_index, g.p_index, g.edge) == (w.d_index, w.p_index, w.edge)
        assert abs(g.code_offset - w.code_offset) <= 1e-3 * dc
        assert abs(g.doppler - w.doppler) <= 0.05
        assert abs(g.ratio - w.ratio) <= 1e-4 * w.ratio
    with pytest.raises(ValueError, match="gps-l1 7"):
        refine.refine(cands[:1], xd[:2 * 30000], engine=eng)
