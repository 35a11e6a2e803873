"""GPU: the symbol former and the Viterbi decoder (csrc/gacq_navbits.hip) bit for bit against tests/navdata_oracle.py -- soft symbols,
alignment, E, A, decoded bits and final metrics -- the frames of gnss_dsp_tools_amd.navdata.decode field for field against the
oracle's framing, and one end-to-end run: encode, simulate, track, decode."""
import numpy as np
import pytest

import navdata_cases as C
import navdata_oracle as O
from gnss_dsp_tools_amd import navdata, simulate, trackloop

pytestmark = pytest.mark.gpu


def _same_symbols(got, want, label):
    a, E, A, q = got
    wa, wE, wA, wq = want
    assert a == wa, (label, a, wa, E, wE)
    assert E.dtype == np.int64 and np.array_equal(E, wE), (label, E, wE)
    assert A == wA, (label, A, wA)                                 # the same double
    assert q.dtype == np.int8 and np.array_equal(q, wq), (label, np.nonzero(q != wq)[0][:8])


@pytest.mark.parametrize("with_overlay", [False, True])
@pytest.mark.parametrize("R", [1, 4, 10, 20])
def test_symbols_bit_for_bit(engine, R, with_overlay):
    """33 channels of one R: n cycles over 2R - 1, 2R, 7R + 3 and 3001, the true alignment over 0, 1 and R - 1; the first one, the
    first three and all 33 in one launch each"""
    o = C.overlays(R)[int(with_overlay)]
    ns = [2 * R - 1, 2 * R, 7 * R + 3, 3001]
    chans = [C.symbol_prompts(k, R, o, ns[k % 4], [0, 1 % R, R - 1][(k // 4) % 3]) for k in range(33)]
    want = [O.symbols(p, R, o) for p in chans]
    for k in (3, 7, 11):                                           # n = 3001: the search finds the alignment the case was built with
        assert want[k][0] == [0, 1 % R, R - 1][(k // 4) % 3], (k, want[k][0])
    for K in (1, 3, 33):
        got = navdata.symbols_many(chans[:K], [R] * K, [o] * K, engine=engine)
        for k in range(K):
            _same_symbols(got[k], want[k], (R, with_overlay, K, k))


def test_symbols_edge_values(engine):
    R, name = 10, "gps-l5i"
    o = navdata.overlay(name)
    base = C.symbol_prompts(50, R, o, 407, 3)
    chans, aligns = [], []
    chans.append(np.zeros(407))                                    # a tie of all alignments: a = 0, q = 0
    out = base.copy()
    out[123] = 1.0e6 * 1000.0                                      # one outlier 10^6 times the rest
    chans.append(out)
    bad = base.copy()
    bad[57], bad[201] = np.nan, np.inf                             # erasures: every symbol either touches, in every alignment
    chans.append(bad)
    chans.append(base * 1.0e-6)                                    # amplitude 1e-3
    chans.append(base * 1.0e6)                                     # amplitude 1e9
    chans.append(np.full(407, -np.inf))                            # nothing finite at all: M = 0, A = 0, q = 0
    aligns = [None] * len(chans)
    chans.append(base)                                             # the alignment given: not the one a search finds
    aligns.append(7)
    chans.append(base)
    aligns.append(None)
    want = [O.symbols(p, R, o, a) for p, a in zip(chans, aligns)]
    got = navdata.symbols_many(chans, [R] * len(chans), [o] * len(chans), aligns, engine=engine)
    for k in range(len(chans)):
        _same_symbols(got[k], want[k], k)
    assert got[0][0] == 0 and not got[0][3].any() and got[0][2] == 0.0 and not got[0][1].any()
    assert got[2][0] == 3 and got[2][3][5] == 0 and got[2][3][19] == 0 and np.count_nonzero(got[2][3] == 0) == 2
    assert got[3][0] == got[4][0] == 3 and int(np.max(np.abs(got[3][3].astype(int) - got[4][3]))) <= 1          # the scale drops out
    assert got[5][2] == 0.0 and not got[5][3].any()
    assert got[6][0] == 7 and got[7][0] == 3 and np.array_equal(got[6][1], got[7][1])
    _same_symbols(navdata.symbols(base, name, align=7, engine=engine), want[6], "symbols(align=7)")
    _same_symbols(navdata.symbols(base, name, engine=engine), want[7], "symbols()")


BLOCK_SHAPES = [(7, None), (120, None), (120, (8, 30)), (121, None)]


@pytest.mark.parametrize("g2_inverted", [False, True])
@pytest.mark.parametrize("steps,gather", BLOCK_SHAPES)
def test_block_jobs_bit_for_bit(engine, steps, gather, g2_inverted):
    """67 terminated jobs cycling over the six kinds of input; the first one, the first five and all 67 in one launch each"""
    made = [C.block(C.BLOCK_KINDS[k % 6], steps, k, gather, g2_inverted) for k in range(67)]
    rx = np.stack([m[0] for m in made])
    rows, cols = gather or (0, 0)
    want = [O.viterbi(r, steps, rows, cols, 0, 0, g2_inverted) for r in rx]
    for k, (_, sent) in enumerate(made):
        if sent is not None and steps >= 120:                      # clean, 12 negated, 20 erased, full scale: the code corrects them
            assert np.array_equal(want[k][0], sent), (k, C.BLOCK_KINDS[k % 6])
    for J in (1, 5, 67):
        bits, met = navdata.viterbi_blocks(rx[:J], gather, g2_inverted, engine=engine)
        assert bits.shape == (J, steps) and bits.dtype == np.uint8 and met.dtype == np.int32
        for k in range(J):
            assert np.array_equal(bits[k], want[k][0]) and int(met[k]) == want[k][1], (J, k, C.BLOCK_KINDS[k % 6], int(met[k]), want[k][1])


def test_jobs_of_mixed_shapes_and_free_end_states_in_one_launch(engine):
    """lengths 7, 120 (gathered and not), 121, the LDS / workspace threshold 1536 / 1537 and 1700 in one launch; every start / end rule;
    partial bit ranges"""
    shapes = [(7, None), (120, (8, 30)), (120, None), (121, None), (1536, None), (1537, None), (1700, None), (240, (16, 30))]
    pieces, jobs, want, nsym, nbits = [], [], [], 0, 0
    for k in range(24):
        steps, gather = shapes[k % len(shapes)]
        rx, _ = C.block(C.BLOCK_KINDS[(k // 2) % 6], steps, 100 + k, gather, bool(k & 1))
        rows, cols = gather or (0, 0)
        start, end = [(0, 0), (-1, -1), (21, -1), (-1, 42)][(k // 8 + k) % 4]
        first = [0, steps // 3, steps - 1][k % 3]
        count = [steps - first, (steps - first + 1) // 2, 1][(k // 3) % 3]
        b, m = O.viterbi(rx, steps, rows, cols, start, end, bool(k & 1))
        want.append((b[first:first + count], m))
        jobs.append(navdata.job(nsym, steps, nbits, rows, cols, start, end, first, count, bool(k & 1)))
        pieces.append(rx)
        nsym += len(rx)
        nbits += count
    bits, met = navdata.viterbi_jobs(np.concatenate(pieces), jobs, nbits + 5, engine)
    assert not bits[nbits:].any()
    for k, (j, (b, m)) in enumerate(zip(jobs, want)):
        assert np.array_equal(bits[j.bit_base:j.bit_base + j.nbits], b) and int(met[k]) == m, (k, j.steps, int(met[k]), m)


@pytest.mark.parametrize("L,W", [(32, 16), (1024, 96)])
def test_streams_bit_for_bit(engine, L, W):
    for T in (1, L - 1, L, L + 1, 3 * L + 5):
        for offset in (0, 1):                                      # both pair alignments of the same symbols
            q, sent = C.noisy_stream(7 * T + offset, T, 0.6, offset)
            for a in (0, 1):
                s = q[a:a + (len(q) - a) // 2 * 2]
                if len(s) < 2:
                    continue
                want, wm = O.stream(s, L, W)
                bits, met = navdata.viterbi_stream(s, L, W, engine=engine)
                assert np.array_equal(bits, want) and np.array_equal(met, wm), (L, W, T, offset, a, int(np.sum(bits != want)))
    # how the jobs are grouped into launches does not change the bits
    q, _ = C.noisy_stream(99, 3 * L + 5, 0.8)
    one, m1 = navdata.viterbi_stream(q, L, W, engine=engine)
    two, m2 = navdata.viterbi_stream(q, L, W, engine=engine, max_jobs=2)
    assert np.array_equal(one, two) and np.array_equal(m1, m2)
    assert np.array_equal(one, O.stream(q, L, W)[0])


def test_one_job_of_2_to_the_20_steps_at_full_scale(engine):
    """the int32 bound: 254 per step for 2^20 steps.  The expected bits and metric come from the encoder."""
    T = 1 << 20
    sent = np.random.Generator(np.random.PCG64(C.SEED)).integers(0, 2, size=T).astype(np.uint8)
    q = (127 * (1 - 2 * navdata.conv_encode(sent).astype(np.int16))).astype(np.int8)
    bits, met = navdata.viterbi_jobs(q, [navdata.job(0, T, 0, start=0, end=-1)], T, engine)
    assert int(met[0]) == 254 * T
    assert np.array_equal(bits, sent)


def _keys(frames):
    return [f.key() if isinstance(f, navdata.Frame) else O.frame_key(f) for f in frames]


@pytest.mark.parametrize("name", sorted(navdata.FORMATS))
def test_frames_field_for_field(engine, name):
    f = navdata.get_format(name)
    # LNAV parity passes in either polarity, so random payload that resembles a TLM and a HOW at a word boundary is a frame to any decoder of
    # these rules (seed 3 draws one); the planted preamble sits inside a word, where the parity of the words around it rejects it
    for seed, kw in ((1, {}), (2, dict(invert=True)), (13, dict(preamble_inside=True)), (4, dict(corrupt=True)), (5, dict(lead=5 * f.R + 1, corrupt=True, invert=True))):
        p, what, lead = C.frame_prompts(name, seed, **kw)
        for everything in (False, True):
            got = navdata.decode(p, name, all_candidates=everything, engine=engine)
            want = O.decode(p, name, everything)
            assert _keys(got) == _keys(want), (name, seed, kw, everything, [(g.record, g.ok) for g in got], [(w["record"], w["ok"]) for w in want])
        got = navdata.decode(p, name, engine=engine)
        full = navdata.decode(p, name, all_candidates=True, engine=engine)
        n_frames = {"lnav": 2, "cnav": 3, "inav": 2}[f.message]
        starts = [lead + i * {"lnav": 6000, "cnav": 600 * f.R, "inav": 500 * f.R}[f.message] for i in range(n_frames)]
        assert all(g.inverted == bool(kw.get("invert")) for g in got)
        if kw.get("corrupt"):
            # LNAV reports the subframe with the failed word; a CNAV message or an I/NAV page whose CRC fails is a candidate like any false hit
            failed = [g for g in full if g.record in starts and not g.ok and g.inverted == bool(kw.get("invert"))]
            assert len(failed) == 1, [(g.record, g.ok) for g in full]
            if f.message == "lnav":
                assert [g.record for g in got] == starts and [g.ok for g in got] == [False, True] and got[0].fields["words"] == "1111011111"
            else:
                assert [g.record for g in got] == [s for s in starts if s != failed[0].record] and all(g.ok for g in got)
        else:
            # a preamble inside the payload starts no frame of its own
            assert [g.record for g in got] == starts and all(g.ok for g in got), (name, seed, [(g.record, g.ok) for g in got])


def test_32_channels_of_mixed_trackers_in_one_call(engine):
    names = sorted(navdata.FORMATS)
    chans = []
    for k in range(32):
        name = names[k % 5]
        p, _, _ = C.frame_prompts(name, 40 + k, invert=bool(k & 2), corrupt=(k % 7 == 3))
        chans.append((p, name, 1 + k))
    many = navdata.decode_many(chans, engine=engine)
    assert len(many) == 32
    for k, (p, name, item) in enumerate(chans):
        single = navdata.decode(p, name, item, engine=engine)
        assert _keys(many[k]) == _keys(single) and len(single) >= 1, (k, name)


def test_end_to_end_galileo_e1b_page_through_simulate_track_decode(engine):
    """Two I/NAV pages, encoded, carried by a simulated galileo-e1b satellite at the rate and amplitude of the E1B simulate / hand-off
    tests, tracked with the default dwells and decoded: a complete page comes back with its CRC passing and the payload that was
    encoded, whichever way round the Costas loop settled.  The stream is rotated so that the second page starts 1.4 s in, behind the
    tracker's pull-in; frames that start in the first 1.2 s are discarded, nothing else."""
    fs, coffset, seconds, prn, doppler, code0 = 10.0e6, -150000.0, 3.5, 11, -1377.3, 2500.42
    rng = C.rng_of(9)
    pages = [navdata.inav_page(1 + i, rng) for i in range(2)]
    stream = navdata.encode_inav(np.concatenate([np.concatenate(p) for p in pages]), "galileo-e1b")
    assert len(stream) == 1000
    sym = np.roll(stream, 350 - 500)                               # page 2 from symbol 350 = 1.4 s to 3.4 s
    sat = simulate.Satellite("galileo-e1b", prn, 3.0, doppler, code0, symbols=sym, periods_per_symbol=1)
    x = simulate.recording([sat], fs, coffset, int(fs * seconds), 31, 12.0, engine=engine)
    loop = trackloop.TrackLoop([trackloop.Channel("galileo-e1b", fs, coffset, prn, doppler, code0)], engine)
    try:
        recs = loop.run([x])[0]
        assert list(loop.status) == [0]
    finally:
        loop.close()
    assert len(recs) >= 3400
    frames = [fr for fr in navdata.decode(recs, "galileo-e1b", prn, engine=engine) if fr.record >= 1200]
    print([navdata.format_frame("galileo-e1b", prn, fr) for fr in frames], "mean prompt", float(np.mean(np.abs(recs["p_re"][1200:]))))
    assert frames and all(fr.ok for fr in frames)
    want = bytes(np.concatenate(pages[1]))
    assert any(bytes(fr.bits) == want and fr.fields["word_type"] == 2 for fr in frames), [fr.fields for fr in frames]
    # the same records with the sign the Costas loop did not settle on: the same payload, reported as inverted the other way
    flipped = [fr for fr in navdata.decode(-recs["p_re"], "galileo-e1b", prn, engine=engine) if fr.record >= 1200]
    assert [(fr.record, bytes(fr.bits), fr.ok, not fr.inverted) for fr in flipped] == [(fr.record, bytes(fr.bits), fr.ok, fr.inverted) for fr in frames]


def test_handoff_nav_flag_adds_lines_and_changes_none(engine, tmp_path):
    """handoff on a short simulated gps-l1 recording: with --nav the lines of the plain run come first, unchanged, and only nav lines
    follow (a quarter of a second holds no subframe, so none here)"""
    import io
    from gnss_dsp_tools_amd import handoff
    fs, coffset = 6.0e6, 250000.0
    sat = simulate.Satellite("gps-l1", 7, 3.0, 1234.5, 417.37, symbols=simulate.symbols("gps-l1", 7, 13, 20, 100))
    path = str(tmp_path / "scene.bin")
    simulate.recording([sat], fs, coffset, int(fs * 0.25), 31, 12.0, engine=engine).cpu().numpy().tofile(path)
    argv = ["--prn", "7", "--loop-dwells", "20,20", path, repr(fs), repr(coffset)]
    plain, with_nav = io.StringIO(), io.StringIO()
    a = handoff.run("gps-l1", argv, plain)
    b = handoff.run("gps-l1", ["--nav"] + argv, with_nav)
    assert plain.getvalue().splitlines() == a and with_nav.getvalue().splitlines() == b
    assert b[:len(a)] == a and any(line.startswith("handoff gps-l1 7 ") for line in a)
    assert all(line.startswith("nav gps-l1 ") for line in b[len(a):])
