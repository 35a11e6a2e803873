"""GPU: the coherent fold kernel (csrc/gacq_cohfold.hip) against the fp64 oracle, its bit-identity across batching, its argument checks
through the raw ABI, the existing search on the device's own folded rows against oracle.acq_oracle, and coherent.search end to end.

Fold bound, per case: four times the deviation of a numpy complex64 evaluation of the same formula (tests/coherent_oracle.fold32)
from the fp64 one, relative to max |y|; both figures and the device's are printed before the assertion (DESIGN 5.16 has the table)."""
import ctypes
import io

import numpy as np
import pytest

import coherent_cases as C
import coherent_oracle as O
from gnss_dsp_tools_amd import _native as nat
from gnss_dsp_tools_amd import acquire, codes, coherent, signals
from oracle import codes_oracle


def _dev(engine, a):
    torch = nat.require_torch()
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:%d" % engine.device)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(C.FOLD_CASES))
def test_fold_matches_the_fp64_oracle(engine, name):
    x, n_out, st, f, fs, W, j0 = C.fold_case(name)
    got = coherent.fold_dev(_dev(engine, x), n_out, st, f, fs, W, j0, engine).cpu().numpy()
    want = O.fold64(x, n_out, st, f, fs, W, j0)
    assert got.shape == want.shape == (len(f), len(W), n_out) and got.dtype == np.complex64
    scale = float(np.max(np.abs(want)))
    dev32 = float(np.max(np.abs(O.fold32(x, n_out, st, f, fs, W, j0) - want))) / scale
    err = float(np.max(np.abs(got - want))) / scale
    print("%-20s D %d  numpy complex64 deviation %.3g  bound %.3g  device %.3g" % (name, len(f), dev32, 4 * dev32, err))
    assert err <= 4 * dev32


def test_fold_cases_cover_the_shapes_and_variations():
    shapes = {(c["n_out"], c["M"], c["H"]) for c in C.FOLD_CASES.values()}
    assert shapes == {(4096, 1, 1), (4096, 20, 33), (4096, 10, 40), (61380, 5, 5), (16384, 100, 100), (1000, 3, 2)}
    assert {len(c["f"]) for c in C.FOLD_CASES.values()} == {1, 7}
    assert min(C.F7) < 0 and max(C.F7) > 0 and 0.0 in C.F7
    assert any(c.get("j0") == 2 ** 40 + 12345 for c in C.FOLD_CASES.values())
    assert any(c.get("wide") for c in C.FOLD_CASES.values()) and any(c.get("odd") for c in C.FOLD_CASES.values())
    x, n_out, st, f, fs, W, j0 = C.fold_case("4096x10x40 zeros")
    assert np.any(W == 0) and np.all(W[3] == 0) and np.any(st[0] != st[-1])      # zero weights; a start table that differs by row
    assert np.any(C.fold_case("1000x3x2 odd")[2] % 2 == 1)


@pytest.mark.gpu
def test_fold_bits_do_not_depend_on_the_batch(engine):
    torch = nat.require_torch()
    for name, d, h in (("4096x10x40 zeros", 3, 35), ("61380x5x5", 5, 2), ("1000x3x2 odd", 6, 1)):
        x, n_out, st, f, fs, W, j0 = C.fold_case(name)
        xd = _dev(engine, x)
        y = coherent.fold_dev(xd, n_out, st, f, fs, W, j0, engine)
        again = coherent.fold_dev(xd, n_out, st, f, fs, W, j0, engine)
        assert torch.equal(y.view(torch.int64), again.view(torch.int64)), name                        # a second run
        row = coherent.fold_dev(xd, n_out, st[d:d + 1], f[d:d + 1], fs, W, j0, engine)
        assert torch.equal(row[0].view(torch.int64), y[d].view(torch.int64)), name                    # row d alone / among seven
        one = coherent.fold_dev(xd, n_out, st, f, fs, W[h:h + 1], j0, engine)
        assert torch.equal(one[:, 0].view(torch.int64), y[:, h].view(torch.int64)), name              # hypothesis h alone / in the batch
        assert float(y.abs().max()) > 0.0


@pytest.mark.gpu
def test_search_does_not_depend_on_the_chunking(engine):
    rec = C.RECORDINGS["nh20"]
    sig = signals.get(rec["signal"])
    xd = _dev(engine, C.recording("nh20", rec["seeds"][0]))
    items = [rec["sats"][0]["item"], 5]
    whole = coherent.search(sig, xd, items, rec["dopplers"], rec["M"], engine=engine)
    row = 20 * sig.samples_needed(1) * 8
    for max_bytes in (row, 2 * row + 1):                                          # one and two Doppler rows per chunk
        assert coherent.search(sig, xd, items, rec["dopplers"], rec["M"], engine=engine, max_bytes=max_bytes) == whole


def _raw(engine, xd, avail, n_out, M, D, H, st, f, fs, j0, W, y, wide=0):
    engine.use_torch_stream()
    keep = [np.ascontiguousarray(st, dtype=np.int64), np.ascontiguousarray(f, dtype=np.float64), np.ascontiguousarray(W, dtype=np.int8)]
    return nat.lib.gacq_fold_dev(engine._ctx, ctypes.c_void_p(xd.data_ptr()), wide, avail, n_out, M, D, H, keep[0].ctypes.data_as(ctypes.c_void_p),
                                 keep[1].ctypes.data_as(ctypes.c_void_p), fs, j0, keep[2].ctypes.data_as(ctypes.c_void_p),
                                 ctypes.c_void_p(y.data_ptr() if y is not None else None))


@pytest.mark.gpu
def test_every_argument_check_through_the_raw_abi(engine):
    torch = nat.require_torch()
    n_out, M, D, H, fs = 1000, 3, 2, 2, 4096000.0
    rng = np.random.Generator(np.random.PCG64(77))
    nsamp = 2 * 1001 + 5 + n_out                                                  # exactly what the last period of row 1 needs
    x = (rng.standard_normal(nsamp) + 1j * rng.standard_normal(nsamp)).astype(np.complex64)
    xd = _dev(engine, x)
    st = np.array([[0, 1001, 2002], [5, 1006, 2007]], dtype=np.int64)
    f = np.array([-250.0, 1000.0])
    W = np.array([[1, -1, 1], [1, 0, -1]], dtype=np.int8)
    y = torch.full((D, H, n_out), float("nan"), dtype=torch.complex64, device=xd.device)
    big_w = np.ones((257, 129), dtype=np.int8)
    BAD, SHORT = -1, -6
    bad = [("n_out 0", dict(n_out=0)), ("M 0", dict(M=0)), ("D 0", dict(D=0)), ("H 0", dict(H=0)), ("n_out -1", dict(n_out=-1)),
           ("M 129", dict(M=129, W=big_w, st=np.zeros((2, 129), dtype=np.int64))), ("H 257", dict(H=257, W=big_w)),
           ("f nan", dict(f=np.array([0.0, np.nan]))), ("f inf", dict(f=np.array([np.inf, 0.0]))), ("fs nan", dict(fs=float("nan"))),
           ("fs inf", dict(fs=float("inf"))), ("fs 0", dict(fs=0.0)), ("fs < 0", dict(fs=-4096000.0)),
           ("j0 > 2^62", dict(j0=2 ** 62 + 1)), ("j0 < -2^62", dict(j0=-2 ** 62 - 1)),
           ("more than 2^31 - 1 workgroups", dict(D=2 ** 29)),                    # 4 workgroups per row; refused before row 2 is read
           ("W 2", dict(W=np.array([[1, -1, 1], [1, 2, -1]], dtype=np.int8))), ("W -2", dict(W=np.array([[-2, -1, 1], [1, 0, -1]], dtype=np.int8)))]
    short = [("start < 0", dict(st=np.array([[0, 1001, 2002], [-1, 1006, 2007]]))),
             ("one sample short", dict(avail=nsamp - 1)),
             ("start past the end", dict(st=np.array([[0, 1001, 2002], [5, 1006, 2008]])))]
    base = dict(avail=nsamp, n_out=n_out, M=M, D=D, H=H, st=st, f=f, fs=fs, j0=0, W=W)
    for want, cases in ((BAD, bad), (SHORT, short)):
        for label, change in cases:
            a = dict(base, **change)
            rc = _raw(engine, xd, a["avail"], a["n_out"], a["M"], a["D"], a["H"], a["st"], a["f"], a["fs"], a["j0"], a["W"], y)
            assert rc == want, (label, rc)
            assert nat.ERRORS[rc] in ("GACQ_ERR_BAD_ARG", "GACQ_ERR_SHORT_INPUT") and nat.lib.gacq_last_error(engine._ctx)
    assert nat.lib.gacq_fold_dev(None, None, 0, 0, 1, 1, 1, 1, None, None, 1.0, 0, None, None) == BAD
    assert _raw(engine, xd, nsamp, n_out, M, D, H, st, f, fs, 0, W, None) == BAD      # NULL output
    torch.cuda.synchronize()
    assert bool(torch.isnan(y.real).all()), "a refused call wrote to the output"
    # the exact-length input runs and is right
    assert _raw(engine, xd, nsamp, n_out, M, D, H, st, f, fs, 0, W, y) == 0
    torch.cuda.synchronize()
    want = O.fold64(x, n_out, st, f, fs, W)
    assert np.max(np.abs(y.cpu().numpy() - want)) <= 1e-5 * np.max(np.abs(want))


@pytest.mark.gpu
@pytest.mark.parametrize("name,item,delay", [("gps-l1", 7, 301), ("beidou-b1i", 11, 5003), ("gps-l5i", 3, 20001)])
def test_search_on_the_devices_own_folded_rows(engine, name, item, delay):
    """Engine.search_batch_dev on y as the device folded it against acq_oracle on the downloaded rows at [0.0], B = 1: equal
    location, metric within 1e-5."""
    sig = signals.get(name)
    M = 3
    n_out = sig.samples_needed(1)
    rng = np.random.Generator(np.random.PCG64(91))
    nsamp = (M - 1) * sig.n + n_out
    x = rng.standard_normal(nsamp) + 1j * rng.standard_normal(nsamp)
    i = np.arange(nsamp)
    rep = codes.replica(sig.code, item, sig.n, sig.boc).astype(np.float64)
    sec = np.array([1, 1, -1])
    x += 0.3 * sec[((i - delay) // sig.n) % 3] * rep[(i - delay) % sig.n] * np.exp(2j * np.pi * 750.0 * i / sig.fs)
    x = x.astype(np.complex64)
    f = np.array([700.0, 750.0])
    W, _ = coherent.patterns(sec, M)
    y = coherent.fold_dev(_dev(engine, x), n_out, coherent.starts(sig, f, M), f, sig.fs, W, 0, engine)
    rows = y.view(len(f) * len(W), n_out)
    items = [item, item + 1]
    peaks = engine.search_batch_dev(sig, rows, items, [0.0], 1).cpu().numpy().view(acquire.PEAK_DTYPE).reshape(len(rows), len(items))
    host = rows.cpu().numpy()
    worst = 0.0
    for k, it in enumerate(items):
        chips = codes_oracle.chips(sig.code, it)
        for r in range(len(rows)):
            metric, idx = O.best(sig, chips, host[r])
            assert int(peaks["idx"][r, k]) == idx and int(peaks["d_index"][r, k]) == 0, (name, it, r)
            worst = max(worst, abs(float(peaks["metric"][r, k]) - metric) / metric)
    print("%s: worst metric deviation %.3g over %d rows x %d items" % (name, worst, len(rows), len(items)))
    assert worst <= 1e-5
    d, h = np.unravel_index(int(np.argmax(peaks["metric"][:, 0])), (len(f), len(W)))
    assert (d, h) == (1, 0)                                                       # the satellite: 750 Hz, overlay phase 0


@pytest.mark.gpu
@pytest.mark.parametrize("key", sorted(C.RECORDINGS))
def test_search_end_to_end_returns_the_oracle_chains_answer(engine, key):
    """The CPU test's recordings (supplied overlay; built-in NH20; GPS L1 with a bit edge inside the window; a per-PRN table with two
    items), every seed, through coherent.search: the (d, h, code_offset) that tests/test_coherent_cpu.py shows the oracle chain to return."""
    rec = C.RECORDINGS[key]
    sig = signals.get(rec["signal"])
    items = [s["item"] for s in rec["sats"]]
    for seed in rec["seeds"]:
        x = C.recording(key, seed)
        got = coherent.search(sig, _dev(engine, x), items, rec["dopplers"], rec["M"], rec["secondary"], rec["data_flip"], engine=engine)
        assert len(got) == len(items)
        for sat, (metric, code, doppler, label) in zip(rec["sats"], got):
            td, th, tc = C.truth(key, sat)
            W, labels = coherent.patterns(C.secondary_of(rec, sat["item"]), rec["M"], rec["data_flip"])
            assert (float(doppler), label, float(code)) == (float(rec["dopplers"][td]), labels[th], tc), (key, seed, sat["item"], got)
            assert label == (sat["h0"], sat["flip_at"])
            if key != "table" and seed == rec["seeds"][0]:           # the chain's metric too, where the oracle is cheap
                y = O.fold64(x.astype(np.complex128), sig.samples_needed(1), coherent.starts(sig, rec["dopplers"], rec["M"]), rec["dopplers"], sig.fs, W)
                met, idx, d, h = O.chain(sig, codes_oracle.chips(sig.code, sat["item"]), y)
                assert (d, h) == (td, th) and abs(float(metric) - met[d, h]) <= 1e-5 * met[d, h], (key, metric, met[d, h])


@pytest.mark.gpu
def test_command_line_on_an_int8_file(engine, tmp_path):
    """beidou-b1i from a 10 MS/s int8 file: the line is the acquire script's plus the label, and equals what the interface returns
    on the same front-end output; the satellite's Doppler and overlay phase come back."""
    name, item, fs, coffset, M, h0, f_true = "beidou-b1i", 11, 10.0e6, 250000.0, 20, 13, -1975.0
    sig = signals.get(name)
    nh = coherent.SECONDARY["beidou.b1i"]
    ms_pad = M + 1 + 5
    nsamp = int(fs * 0.001 * ms_pad)
    rng = np.random.Generator(np.random.PCG64(2024))
    t = np.arange(nsamp) / fs - 0.0006                                            # the code starts 0.6 ms into the file
    chips = 1.0 - 2.0 * codes.chips(sig.code, item)
    a = 4.0 * nh[(np.floor(t / 0.001).astype(np.int64) + h0) % 20] * chips[np.floor(t * 2.046e6).astype(np.int64) % 2046]
    ang = 2 * np.pi * np.mod((coffset + f_true) * (np.arange(nsamp) / fs), 1.0)
    iq = np.stack([a * np.cos(ang), a * np.sin(ang)], axis=1) + rng.normal(0.0, 12.0, size=(nsamp, 2))
    raw = np.clip(np.round(iq), -127, 127).astype(np.int8).ravel()
    path = tmp_path / "b1i.iq"
    raw.tofile(str(path))
    out = io.StringIO()
    lines = coherent.run(name, ["--prn", "%d,5" % item, "--doppler-search", "-2050,-1900,25", "--periods", str(M), str(path), repr(fs), repr(coffset)],
                         out=out)
    assert out.getvalue().splitlines() == lines and len(lines) == 2
    dop = acquire.doppler_grid([-2050.0, -1900.0, 25.0])
    res = coherent.search(sig, engine.frontend_dev(sig, raw, fs, coffset, ms_pad), [item, 5], dop, M, engine=engine)
    assert lines == [coherent.format_line(sig, it, r) for it, r in zip([item, 5], res)]
    metric, code, doppler, label = res[0]
    assert lines[0] == acquire.format_result(sig, item, (metric, code, doppler)) + " secondary_phase %d" % h0
    assert float(doppler) == f_true and label == (h0, None)
    # minus the delay, in chips; the front-end's 161-tap filter may add up to its group delay, 80 samples at 10 MS/s = 16.4 chips
    want_code = (2046 * (1.0 - 0.6)) % 2046
    assert abs(code - want_code) <= 20.0
    assert metric > 2.0 * res[1][0]                                               # PRN 5 is not in the file
