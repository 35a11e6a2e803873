"""CPU: the fixed points of the navigation-data formats (CRC-24Q check value, the impulse responses of the code, the interleaver, the
LNAV parity equations), the encoders against the numpy definition of the decoder (tests/navdata_oracle.py) for all five trackers, the
chunking rule of the stream decoder on the definition alone, every refusal of gacq_navsym and gacq_viterbi_dev that is made before a
launch, and the command line's input and output lines."""
import ctypes
import io

import numpy as np
import pytest

import navdata_cases as C
import navdata_oracle as O
from gnss_dsp_tools_amd import _native as nat
from gnss_dsp_tools_amd import navdata, secondary, trackloop


def test_crc24q_check_value():
    bits = np.unpackbits(np.frombuffer(b"123456789", dtype=np.uint8))
    assert navdata.crc24q(bits) == 0xCDE703 and O.crc24q(bits.tolist()) == 0xCDE703
    assert navdata.crc24q([]) == 0 and navdata.CRC24Q_POLY == 0x1864CFB


def test_impulse_responses_of_the_code():
    for enc in (navdata.conv_encode, O.encode):
        c = np.asarray(enc([1, 0, 0, 0, 0, 0, 0])).reshape(7, 2)
        assert c[:, 0].tolist() == [1, 1, 1, 1, 0, 0, 1] and c[:, 1].tolist() == [1, 0, 1, 1, 0, 1, 1]
        c = np.asarray(enc([1, 0, 0, 0, 0, 0, 0], True)).reshape(7, 2)
        assert c[:, 0].tolist() == [1, 1, 1, 1, 0, 0, 1] and c[:, 1].tolist() == [0, 1, 0, 0, 1, 0, 0]
    bits = C.rng_of(0).integers(0, 2, size=300)
    for inv in (False, True):
        assert np.array_equal(navdata.conv_encode(bits, inv), O.encode(bits, inv))


def test_interleaver_against_the_literal_matrix():
    # 30 columns of 8 rows, filled column by column with 0..239 and read row by row
    matrix = [[8 * col + row for col in range(30)] for row in range(8)]
    want = [v for row in matrix for v in row]
    got = navdata.interleave(np.arange(240))
    assert got.tolist() == want
    # the decoder's gather undoes it: coded[i] = rx[(i mod rows) cols + i div rows]
    assert [int(got[(i % 8) * 30 + i // 8]) for i in range(240)] == list(range(240))


def test_lnav_word_against_the_six_equations():
    d = [None, 1, 0, 0, 0, 1, 0, 1, 1, 0, 1, 1, 0, 1, 0, 0, 1, 1, 1, 0, 1, 0, 0, 1, 0]        # d[1..24]
    for d29s, d30s in ((0, 0), (0, 1), (1, 0), (1, 1)):
        D25 = d29s ^ d[1] ^ d[2] ^ d[3] ^ d[5] ^ d[6] ^ d[10] ^ d[11] ^ d[12] ^ d[13] ^ d[14] ^ d[17] ^ d[18] ^ d[20] ^ d[23]
        D26 = d30s ^ d[2] ^ d[3] ^ d[4] ^ d[6] ^ d[7] ^ d[11] ^ d[12] ^ d[13] ^ d[14] ^ d[15] ^ d[18] ^ d[19] ^ d[21] ^ d[24]
        D27 = d29s ^ d[1] ^ d[3] ^ d[4] ^ d[5] ^ d[7] ^ d[8] ^ d[12] ^ d[13] ^ d[14] ^ d[15] ^ d[16] ^ d[19] ^ d[20] ^ d[22]
        D28 = d30s ^ d[2] ^ d[4] ^ d[5] ^ d[6] ^ d[8] ^ d[9] ^ d[13] ^ d[14] ^ d[15] ^ d[16] ^ d[17] ^ d[20] ^ d[21] ^ d[23]
        D29 = d30s ^ d[1] ^ d[3] ^ d[5] ^ d[6] ^ d[7] ^ d[9] ^ d[10] ^ d[14] ^ d[15] ^ d[16] ^ d[17] ^ d[18] ^ d[21] ^ d[22] ^ d[24]
        D30 = d29s ^ d[3] ^ d[5] ^ d[6] ^ d[8] ^ d[9] ^ d[10] ^ d[11] ^ d[13] ^ d[15] ^ d[19] ^ d[22] ^ d[23] ^ d[24]
        want = [v ^ d30s for v in d[1:]] + [D25, D26, D27, D28, D29, D30]
        word = navdata.lnav_word(d[1:], d29s, d30s)
        assert word.tolist() == want
        assert O.lnav_parity(d, d29s, d30s) == want[24:]
        ok, src = navdata.lnav_check(word, d29s, d30s)
        assert ok and src.tolist() == d[1:]
        bad = word.copy()
        bad[7] ^= 1
        assert not navdata.lnav_check(bad, d29s, d30s)[0]


def test_lnav_encoder_solves_the_last_bits_of_words_2_and_10():
    pl = C.lnav_payloads(3, 2)
    for prev in ((0, 0), (1, 1), (0, 1)):
        bits = (navdata.encode_lnav(pl, prev)[::20] < 0).astype(int)
        assert len(bits) == 600
        for sf in range(2):
            for w in (1, 9):
                assert bits[300 * sf + 30 * w + 28] == 0 and bits[300 * sf + 30 * w + 29] == 0


def test_format_table():
    assert sorted(navdata.FORMATS) == sorted(O.FORMATS) == ["galileo-e1b", "galileo-e5bi", "gps-l1", "gps-l2cm", "gps-l5i"]
    for name, f in navdata.FORMATS.items():
        message, R, _, fec, inv = O.FORMATS[name]
        assert (f.message, f.R, f.fec, f.g2_inverted) == (message, R, fec, inv)
        assert np.array_equal(navdata.overlay(name), O.overlay(name)) and len(navdata.overlay(name)) == R
        # a record is one 1 ms track() call: R = code periods per symbol times the tracker's calls per period
        t = trackloop.TRACKERS[name]
        assert f.R == f.periods * t.subs and f.message in navdata.FRAMERS
    assert np.array_equal(navdata.overlay("gps-l5i"), secondary.SECONDARY["gps.l5i"])
    with pytest.raises(KeyError):
        navdata.get_format("beidou-b1i")


@pytest.mark.parametrize("name", sorted(navdata.FORMATS))
@pytest.mark.parametrize("invert", [False, True])
def test_encoder_to_oracle_round_trip(name, invert):
    p, what, lead = C.frame_prompts(name, 7, invert=invert)
    frames = O.decode(p, name)
    f = navdata.get_format(name)
    assert frames and all(fr["ok"] and fr["inverted"] == invert for fr in frames), frames
    assert frames[0]["record"] == lead
    if f.message == "lnav":
        assert [(fr["fields"]["subframe"], fr["fields"]["tow"]) for fr in frames] == [(1, 1000), (2, 1001)]
        sent = (navdata.encode_lnav(what)[::20] < 0).astype(np.uint8)
        assert b"".join(fr["bits"] for fr in frames) == bytes(sent)
        assert [fr["record"] for fr in frames] == [lead, lead + 6000]
    elif f.message == "cnav":
        assert [fr["bits"] for fr in frames] == [bytes(m) for m in what]
        assert [(fr["fields"]["prn"], fr["fields"]["type"], fr["fields"]["tow"]) for fr in frames] == [(3, 10, 500), (4, 11, 501), (5, 12, 502)]
        assert [fr["record"] for fr in frames] == [lead + 600 * f.R * i for i in range(3)]
    else:
        assert [fr["bits"] for fr in frames] == [bytes(np.concatenate(pg)) for pg in what]
        assert [(fr["fields"]["word_type"], fr["fields"]["page_type"], fr["fields"]["even_odd"]) for fr in frames] == [(2, 0, (0, 1)), (3, 0, (0, 1))]
        assert [fr["record"] for fr in frames] == [lead, lead + 500 * f.R]


def test_lnav_round_trip_with_the_preceding_d30_set():
    pl = C.lnav_payloads(5, 2)
    for prev in ((0, 1), (1, 1), (1, 0)):
        v = navdata.encode_lnav(pl, prev)
        lead = np.repeat(1 - 2 * np.array([0, 1, 0, prev[0], prev[1]]), 20)
        p = 500.0 * np.concatenate([np.ones(3), lead, v, np.ones(45)])
        for sign in (1.0, -1.0):
            frames = O.decode(sign * p, "gps-l1")
            assert [(fr["record"], fr["ok"], fr["inverted"], fr["fields"]["tow"]) for fr in frames] == [(103, True, sign < 0, 1000), (6103, True, sign < 0, 1001)]
            if prev[1]:                                             # the preamble is transmitted inverted
                assert frames[0]["bits"][:8] == bytes(1 - navdata.PREAMBLE)


@pytest.mark.parametrize("sigma", [0.6, 0.8])
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_chunked_stream_decode_of_the_oracle_equals_its_whole_stream_decode(seed, sigma):
    q, bits = C.noisy_stream(seed, 5000, sigma)
    raw = float(np.mean((q < 0) != (navdata.conv_encode(bits) == 1)))
    whole = O.viterbi(q, 5000, start=-1, end=-1)[0]
    chunked = O.stream(q)[0]
    print("seed %d sigma %.1f: raw symbol error rate %.3f, chunked vs whole %d bits, whole vs sent %d bits" %
          (seed, sigma, raw, int(np.sum(whole != chunked)), int(np.sum(whole != bits))))
    assert np.array_equal(whole, chunked)
    assert 0.03 <= raw <= 0.13


def _navsym_check(p=None, n=None, R=None, o=None, align=None, K=1, null=None):
    p = np.ones(64) if p is None else np.asarray(p, dtype=np.float64)
    n = np.array([40] * max(K, 1) if n is None else n, dtype=np.int32)
    R = np.array([20] * max(K, 1) if R is None else R, dtype=np.int32)
    o = np.ones((max(K, 1), navdata.MAX_R), dtype=np.int8) if o is None else np.asarray(o, dtype=np.int8)
    al = None if align is None else np.array(align, dtype=np.int32)
    outs = [np.zeros(max(K, 1), dtype=np.int32), np.zeros((max(K, 1), 20), dtype=np.int64), np.zeros(max(K, 1)), np.zeros(64, dtype=np.int8),
            np.zeros(max(K, 1), dtype=np.int32)]
    args = [p, n, R, o, al] + outs
    ptr = [None if (a is None or i == null) else a.ctypes.data_as(ctypes.c_void_p) for i, a in enumerate(args)]
    rc = nat.lib.gacq_navsym_check(ptr[0], ptr[1], ptr[2], ptr[3], ptr[4], K, *ptr[5:])
    # the entry point makes the same refusal before it looks at the context (a NULL context is itself refused, with everything else in order)
    rc2 = nat.lib.gacq_navsym(None, ptr[0], ptr[1], ptr[2], ptr[3], ptr[4], K, *ptr[5:])
    assert rc2 == (rc if rc < 0 else -1) and not any(a.any() for a in outs)
    return rc


def test_every_refusal_of_navsym_before_a_launch():
    BAD, SHORT = -1, -6
    assert _navsym_check() == 0
    assert _navsym_check(K=0) == BAD and _navsym_check(K=-3) == BAD
    assert _navsym_check(R=[0]) == BAD and _navsym_check(R=[21]) == BAD and _navsym_check(R=[-1]) == BAD
    assert _navsym_check(R=[1], n=[1]) == 0 and _navsym_check(R=[20], n=[39]) == 0
    o = np.ones((1, 20), dtype=np.int8)
    for v in (0, 2, -2, 127):
        o2 = o.copy()
        o2[0, 19] = v
        assert _navsym_check(o=o2) == BAD
        assert _navsym_check(o=o2, R=[19], n=[40]) == 0         # beyond R nothing is read
    for i in (0, 1, 2, 3, 5, 6, 7, 8, 9):                       # every pointer but the optional alignments
        assert _navsym_check(null=i) == BAD, i
    assert _navsym_check(n=[(1 << 24) + 1]) == BAD
    assert _navsym_check(align=[20]) == BAD and _navsym_check(align=[-2]) == BAD and _navsym_check(align=[19]) == 0 and _navsym_check(align=[-1]) == 0
    assert _navsym_check(n=[38]) == SHORT and _navsym_check(R=[1], n=[0]) == SHORT and _navsym_check(R=[4], n=[6]) == SHORT
    assert _navsym_check(K=2, n=[40, 38], R=[20, 20], o=np.ones((2, 20))) == SHORT
    assert _navsym_check(K=2, n=[40, 7], R=[20, 4], o=np.ones((2, 20))) == 0
    with pytest.raises(ValueError):
        navdata.symbols_many([np.ones(40)], [20], [np.ones(19)])


def _vit_check(nsym=240, nbits=120, J=1, jobs="default", **kw):
    j = navdata.job(0, 120, 0, **kw) if jobs == "default" else jobs
    arr = (navdata.VitJob * 1)(j) if j is not None else None
    rc = nat.lib.gacq_viterbi_check(None if arr is None else ctypes.addressof(arr), J, nsym, nbits)
    buf = np.zeros(256, dtype=np.int8)
    rc2 = nat.lib.gacq_viterbi_dev(None, buf.ctypes.data_as(ctypes.c_void_p), nsym, None if arr is None else ctypes.addressof(arr), J,
                                   buf.ctypes.data_as(ctypes.c_void_p), nbits, buf.ctypes.data_as(ctypes.c_void_p))
    assert rc2 == (rc if rc < 0 else -1) and not buf.any()
    return rc


def test_every_refusal_of_the_viterbi_entry_before_a_launch():
    BAD, SHORT = -1, -6
    J = navdata.job
    assert ctypes.sizeof(navdata.VitJob) == 48
    assert _vit_check() == 0 and _vit_check(rows=8, cols=30) == 0 and _vit_check(start=-1, end=-1, g2_inverted=True) == 0
    assert _vit_check(J=0) == BAD and _vit_check(jobs=None) == BAD and _vit_check(nsym=-1) == BAD and _vit_check(nbits=-1) == BAD
    assert _vit_check(jobs=J(0, 0)) == BAD and _vit_check(jobs=J(0, (1 << 20) + 1), nsym=1 << 22, nbits=1 << 21) == BAD
    assert _vit_check(jobs=J(0, 1 << 20), nsym=1 << 21, nbits=1 << 20) == 0
    assert _vit_check(nsym=239) == SHORT and _vit_check(jobs=J(1, 120)) == SHORT and _vit_check(jobs=J(-1, 120)) == SHORT
    assert _vit_check(rows=8, cols=29) == BAD and _vit_check(rows=-8, cols=-30) == BAD and _vit_check(rows=16, cols=30) == BAD
    assert _vit_check(rows=0, cols=30) == 0
    for s in (-2, 64):
        assert _vit_check(start=s) == BAD and _vit_check(end=s) == BAD
    assert _vit_check(start=63, end=63) == 0
    assert _vit_check(jobs=J(0, 120, first_bit=-1, nbits=10)) == BAD and _vit_check(jobs=J(0, 120, first_bit=100, nbits=21)) == BAD
    assert _vit_check(jobs=J(0, 120, first_bit=100, nbits=-1)) == BAD and _vit_check(jobs=J(0, 120, first_bit=100, nbits=20)) == 0
    assert _vit_check(nbits=119) == BAD and _vit_check(jobs=J(0, 120, bit_base=1)) == BAD and _vit_check(jobs=J(0, 120, bit_base=-1)) == BAD
    assert _vit_check(jobs=J(0, 120, bit_base=100, first_bit=100, nbits=20)) == 0
    with pytest.raises(ValueError):
        navdata.stream_jobs(100, chunk_bits=0)
    with pytest.raises(ValueError):
        navdata.viterbi_blocks(np.zeros((3, 7), dtype=np.int8))


def test_stream_jobs_follow_the_fixed_rule():
    for T, L, W in ((1, 32, 16), (31, 32, 16), (32, 32, 16), (33, 32, 16), (101, 32, 16), (3077, 1024, 96), (5000, 1024, 96)):
        jobs = navdata.stream_jobs(T, 10, 5, L, W)
        assert len(jobs) == -(-T // L)
        for c, j in enumerate(jobs):
            lo, hi = max(0, c * L - W), min(T, (c + 1) * L + W)
            assert (j.sym_base, j.steps, j.bit_base, j.first_bit, j.nbits) == (10 + 2 * lo, hi - lo, 5 + c * L, c * L - lo, min(T, (c + 1) * L) - c * L)
            assert (j.start_state, j.end_state, j.rows, j.cols, j.g2_inverted) == (-1, -1, 0, 0, 0)
        assert sum(j.nbits for j in jobs) == T


def test_command_line_reads_the_track_lines_and_prints_one_line_per_frame():
    text = "0 812.5 -3.25 1200.0 0.1 -0.2 10.0 12.0 9.0\n\n1 -790.125 4.0 1200.5 0.1 179.7 10.0 12.0 9.0\n2 1e3 0 0 0 0 0 0 0\n"
    assert navdata.read_prompts(io.StringIO(text)).tolist() == [812.5, -790.125, 1000.0]
    with pytest.raises(ValueError):
        navdata.read_prompts(["17"])
    recs = np.zeros(3, dtype=trackloop.RECORD_DTYPE)
    recs["p_re"] = [1.5, -2.5, 3.0]
    assert navdata._prompts(recs).tolist() == [1.5, -2.5, 3.0]
    lines = trackloop.format_lines("galileo-e1b", recs)
    assert navdata.read_prompts(lines).tolist() == [1.5, -2.5, 3.0]
    fr = navdata.Frame("lnav", 147, 7, True, False, np.zeros(300, dtype=np.uint8), dict(subframe=3, tow=1234, words="1111011111"))
    assert navdata.format_frame("gps-l1", 11, fr) == "nav gps-l1 11 lnav record 147 FAIL inverted subframe 3 tow 1234 words 1111011111"
    fr = navdata.Frame("inav", 40, 10, False, True, np.zeros(228, dtype=np.uint8), dict(even_odd=(0, 1), page_type=0, word_type=4))
    assert navdata.format_frame("galileo-e1b", 5, fr) == "nav galileo-e1b 5 inav record 40 ok even_odd 01 page_type 0 word_type 4"
    fr = navdata.Frame("cnav", 0, 0, False, True, np.zeros(300, dtype=np.uint8), dict(prn=3, type=10, tow=500))
    assert navdata.format_frame("gps-l5i", None, fr) == "nav gps-l5i 0 cnav record 0 ok prn 3 type 10 tow 500"
    a = navdata.parse(["gps-l2cm", "--prn", "7", "--all-candidates", "-"])
    assert (a.tracker, a.prn, a.all_candidates, a.input_filename) == ("gps-l2cm", 7, True, "-")
    with pytest.raises(SystemExit):
        navdata.parse(["beidou-b1i", "x.txt"])


def test_handoff_takes_the_nav_flag_and_defaults_to_off():
    from gnss_dsp_tools_amd import handoff
    _, a = handoff.parse("galileo-e1b", ["--prn", "11", "x.bin", "10e6", "-150000"])
    assert a.nav is False
    _, a = handoff.parse("galileo-e1b", ["--prn", "11", "--nav", "x.bin", "10e6", "-150000"])
    assert a.nav is True and a.out_dir is None
