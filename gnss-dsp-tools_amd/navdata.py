"""Navigation frames from tracked prompts: symbol forming and bit synchronisation (gacq_navsym) and the batched K = 7 Viterbi decoder
(gacq_viterbi_dev) on the GPU (csrc/gacq_navbits.hip), framing on the host.

    python -m gnss_dsp_tools_amd.navdata <tracker> [--prn N] [--all-candidates] FILE|-

reads the output lines of ``python -m gnss_dsp_tools_amd.track <tracker>`` (column 1 is the prompt's real part, one line per 1 ms
record) and prints one line per frame:

    nav <tracker> <prn> <message> record <first record> <ok|FAIL>[ inverted] <field> <value> ...

FORMATS has one row per tracker: the message family, the records per symbol R, the overlay over the R records of a symbol and whether
the symbols are convolutionally coded.  A new format is a row plus a framing function in FRAMERS (and, for tests, an encoder).

    gps-l1        LNAV   R = 20                   (32,26) parity per 30-bit word, no FEC
    gps-l2cm      CNAV   R = 20                   K = 7 rate 1/2, continuous
    gps-l5i       CNAV   R = 10, NH10 overlay     the same
    galileo-e1b   I/NAV  R = 4                    K = 7 rate 1/2, G2 inverted, terminated page parts, 30 x 8 interleaver
    galileo-e5bi  I/NAV  R = 4, CS4 overlay       the same

Not covered: BeiDou D1 / D2 (BCH), GLONASS strings (meander), B1C / L1C (LDPC), F/NAV, and the contents of the frames (ephemerides).
The definitions of the two kernels are in include/gacq.h; tests/navdata_oracle.py restates them, and the framing, in plain numpy."""
import argparse
import ctypes
import sys
from dataclasses import dataclass, field

import numpy as np

from . import _native as nat
from . import secondary

MAX_R = nat.CONSTANTS["GACQ_NAV_MAX_R"]
MAX_STEPS = 1 << 20
CHUNK_BITS, WARM = 1024, 96

PREAMBLE = np.array([1, 0, 0, 0, 1, 0, 1, 1], dtype=np.uint8)               # LNAV TLM and CNAV
INAV_SYNC = np.array([0, 1, 0, 1, 1, 0, 0, 0, 0, 0], dtype=np.uint8)
INAV_ROWS, INAV_COLS = 8, 30                 # the interleaver: filled column-wise, read row-wise
INAV_PART_BITS, INAV_PART_SYMBOLS = 120, 250
CRC24Q_POLY = 0x1864CFB

# IS-GPS-200 table 20-XIV: the source bits d1..d24 (1-based) under each parity bit, and which of D29*, D30* it starts from
LNAV_PARITY = (
    (29, (1, 2, 3, 5, 6, 10, 11, 12, 13, 14, 17, 18, 20, 23)),
    (30, (2, 3, 4, 6, 7, 11, 12, 13, 14, 15, 18, 19, 21, 24)),
    (29, (1, 3, 4, 5, 7, 8, 12, 13, 14, 15, 16, 19, 20, 22)),
    (30, (2, 4, 5, 6, 8, 9, 13, 14, 15, 16, 17, 20, 21, 23)),
    (30, (1, 3, 5, 6, 7, 9, 10, 14, 15, 16, 17, 18, 21, 22, 24)),
    (29, (3, 5, 6, 8, 9, 10, 11, 13, 15, 19, 22, 23, 24)),
)


@dataclass(frozen=True)
class Format:
    message: str               # key of FRAMERS: "lnav", "cnav", "inav"
    R: int                     # 1 ms records per symbol
    overlay: str = None        # key of secondary.SECONDARY: the overlay over the R records of a symbol
    periods: int = 1           # code periods per symbol (what the encoders emit per symbol)
    fec: str = None            # None, "stream" (continuous) or "block" (terminated page parts)
    g2_inverted: bool = False


FORMATS = {
    "gps-l1": Format("lnav", 20, periods=20),
    "gps-l2cm": Format("cnav", 20, fec="stream"),
    "gps-l5i": Format("cnav", 10, "gps.l5i", 10, fec="stream"),
    "galileo-e1b": Format("inav", 4, fec="block", g2_inverted=True),
    "galileo-e5bi": Format("inav", 4, "galileo.e5bi", 4, fec="block", g2_inverted=True),
}


def get_format(name):
    if name not in FORMATS:
        raise KeyError("no navigation message format for tracker %r (the formats: %s)" % (name, ", ".join(sorted(FORMATS))))
    return FORMATS[name]


def overlay(name):
    """The +-1 overlay over the R records of a symbol of the tracker (int8 [R])"""
    f = get_format(name)
    if f.overlay is None:
        return np.ones(f.R, dtype=np.int8)
    o = np.asarray(secondary.SECONDARY[f.overlay], dtype=np.int8)
    return np.repeat(o, f.R // len(o)).astype(np.int8)


@dataclass
class Frame:
    """One frame: ``record`` the first 1 ms record of the frame in the prompts, ``symbol`` its first symbol among the soft symbols,
    ``bits`` the frame as transmitted (polarity removed; LNAV: the 300 bits D1..D30 of ten words; CNAV: the 300-bit message; I/NAV:
    the even then the odd page part without their tails, 228 bits), ``ok`` every check passed, ``fields`` what the framing read."""
    message: str
    record: int
    symbol: int
    inverted: bool
    ok: bool
    bits: np.ndarray
    fields: dict = field(default_factory=dict)

    def key(self):
        return (self.message, int(self.record), int(self.symbol), bool(self.inverted), bool(self.ok), bytes(np.asarray(self.bits, dtype=np.uint8)),
                tuple(sorted((k, tuple(v) if isinstance(v, (list, tuple, np.ndarray)) else v) for k, v in self.fields.items())))


# ------------------------------------------------------------------------------------------------ bits and codes

def crc24q(bits):
    """CRC-24Q (polynomial 0x1864CFB, initial value 0) of a bit sequence, first bit first"""
    crc = 0
    for b in np.asarray(bits, dtype=np.uint8).tolist():
        crc = ((crc ^ (b << 23)) << 1)
        if crc & 0x1000000:
            crc ^= CRC24Q_POLY
    return crc


def bits_of(value, n):
    """n bits of an integer, most significant first (uint8)"""
    return np.array([(int(value) >> (n - 1 - i)) & 1 for i in range(n)], dtype=np.uint8)


def int_of(bits):
    v = 0
    for b in np.asarray(bits).tolist():
        v = (v << 1) | int(b)
    return v


def conv_encode(bits, g2_inverted=False):
    """The K = 7 rate 1/2 code from the all-zero register: G1 = 171 (taps r0 r1 r2 r3 r6) then G2 = 133 (r0 r2 r3 r5 r6) per input
    bit, r[k] the input k steps before; uint8 [2 len(bits)]"""
    b = np.asarray(bits, dtype=np.uint8)
    r = np.concatenate([np.zeros(6, dtype=np.uint8), b])
    n = len(b)
    tap = lambda k: r[6 - k:6 - k + n]
    g1 = tap(0) ^ tap(1) ^ tap(2) ^ tap(3) ^ tap(6)
    g2 = tap(0) ^ tap(2) ^ tap(3) ^ tap(5) ^ tap(6)
    if g2_inverted:
        g2 = g2 ^ 1
    return np.stack([g1, g2], axis=1).reshape(-1).astype(np.uint8)


def interleave(coded, rows=INAV_ROWS, cols=INAV_COLS):
    """Block interleaver filled column-wise and read row-wise: tx[(i mod rows) cols + i div rows] = coded[i]"""
    c = np.asarray(coded)
    return c.reshape(cols, rows).T.reshape(-1).copy()


def lnav_word(d, d29, d30):
    """The 30 transmitted bits of a word from its source bits d1..d24 and D29*, D30* of the word before"""
    d = np.asarray(d, dtype=np.uint8)
    prev = {29: int(d29), 30: int(d30)}
    par = [(prev[s] + sum(int(d[i - 1]) for i in idx)) & 1 for s, idx in LNAV_PARITY]
    return np.concatenate([d ^ np.uint8(d30), np.array(par, dtype=np.uint8)])


def lnav_check(word, d29, d30):
    """(passes, source bits d1..d24) of 30 received bits"""
    w = np.asarray(word, dtype=np.uint8)
    d = w[:24] ^ np.uint8(d30)
    return bool(np.array_equal(lnav_word(d, d29, d30)[24:], w[24:])), d


def _periods(sym_bits, name):
    """+-1 per code period (int8) of the symbol bits of a tracker: 1 - 2 bit, repeated over the symbol's periods, times the overlay"""
    f = get_format(name)
    v = np.repeat(1 - 2 * np.asarray(sym_bits, dtype=np.int8), f.periods).astype(np.int8)
    if f.overlay is not None:
        v = (v * np.resize(np.asarray(secondary.SECONDARY[f.overlay], dtype=np.int8), len(v))).astype(np.int8)
    return v


def encode_lnav(payload, prev=(0, 0), name="gps-l1"):
    """payload: 240 source bits per subframe (24 per word, ten words), any number of subframes.  Bits 23 and 24 of words 2 and 10 are
    replaced by the solution of D29 = D30 = 0.  prev: (D29*, D30*) before the first word.  Returns the +-1 value per code period."""
    p = np.array(payload, dtype=np.uint8).reshape(-1)
    if len(p) % 240:
        raise ValueError("LNAV payload: 240 source bits per subframe")
    d29, d30 = int(prev[0]), int(prev[1])
    out = []
    for w in range(len(p) // 24):
        d = p[24 * w:24 * w + 24].copy()
        if w % 10 in (1, 9):
            d[22] = d[23] = 0
            d[23] = lnav_word(d, d29, d30)[28]            # d24 enters D29 alone of the two
            d[22] = lnav_word(d, d29, d30)[29]            # then d23 settles D30
        word = lnav_word(d, d29, d30)
        d29, d30 = int(word[28]), int(word[29])
        out.append(word)
    return _periods(np.concatenate(out), name)


def lnav_payload(tow, subframe_id, rng):
    """240 source bits of a subframe: the preamble, a HOW with the TOW count and the subframe id, random bits elsewhere"""
    p = rng.integers(0, 2, size=240).astype(np.uint8)
    p[:8] = PREAMBLE
    p[24:41] = bits_of(tow, 17)
    p[43:46] = bits_of(subframe_id, 3)
    p[46:48] = 0
    return p


def cnav_message(prn, msg_type, tow, rng):
    """A 300-bit CNAV message: preamble, PRN, type, TOW count, alert, 238 random bits, CRC-24Q"""
    m = np.concatenate([PREAMBLE, bits_of(prn, 6), bits_of(msg_type, 6), bits_of(tow, 17), rng.integers(0, 2, size=239).astype(np.uint8)])
    return np.concatenate([m, bits_of(crc24q(m), 24)])


def encode_cnav(bits, name="gps-l2cm"):
    """bits: whole 300-bit messages, encoded as one continuous stream from the all-zero register.  +-1 per code period."""
    if get_format(name).message != "cnav":
        raise ValueError("%s does not carry CNAV" % name)
    return _periods(conv_encode(np.asarray(bits, dtype=np.uint8).reshape(-1)), name)


def inav_page(word_type, rng, page_type=0):
    """(even, odd): the two 114-bit page parts of a nominal page (without their six tail bits) with random contents and its CRC"""
    even = np.concatenate([[0, page_type], bits_of(word_type, 6), rng.integers(0, 2, size=106)]).astype(np.uint8)
    odd = np.concatenate([[1, page_type], rng.integers(0, 2, size=80)]).astype(np.uint8)
    crc = bits_of(crc24q(np.concatenate([even, odd])), 24)
    return even, np.concatenate([odd, crc, rng.integers(0, 2, size=8).astype(np.uint8)])


def encode_inav(parts, name="galileo-e1b"):
    """parts: 114 bits per page part.  Each gets six tail bits, the code (G2 inverted) from the all-zero register, the 30 x 8
    interleaver and the ten sync symbols in front.  +-1 per code period."""
    if get_format(name).message != "inav":
        raise ValueError("%s does not carry I/NAV" % name)
    p = np.asarray(parts, dtype=np.uint8).reshape(-1, 114)
    out = []
    for part in p:
        coded = conv_encode(np.concatenate([part, np.zeros(6, dtype=np.uint8)]), g2_inverted=True)
        out += [INAV_SYNC, interleave(coded)]
    return _periods(np.concatenate(out), name)


def records_of(periods, name):
    """The encoders' value per code period repeated over the 1 ms records of a period (gps-l2cm: 20, galileo-e1b: 4, else 1)"""
    f = get_format(name)
    return np.repeat(np.asarray(periods), f.R // f.periods)


# ------------------------------------------------------------------------------------------------ the two device entry points

VitJob = nat.struct("gacq_vit_job")


def _engine(engine):
    from . import acquire
    return engine or acquire.default_engine()


def _prompts(x):
    """float64 prompt real parts of a record array (trackloop.RECORD_DTYPE) or of anything array-like"""
    a = np.asarray(x)
    if a.dtype.names and "p_re" in a.dtype.names:
        a = a["p_re"]
    return np.ascontiguousarray(a, dtype=np.float64).reshape(-1)


def navsym_arrays(prompts, R, overlays, align=None):
    """The flat arrays gacq_navsym takes, from one prompt array, R and overlay per channel"""
    K = len(prompts)
    p = [_prompts(x) for x in prompts]
    n = np.array([len(x) for x in p], dtype=np.int32)
    Rv = np.array([int(r) for r in R], dtype=np.int32)
    o = np.zeros((max(K, 1), MAX_R), dtype=np.int8)
    for k, ov in enumerate(overlays):
        ov = np.asarray(ov, dtype=np.int8).reshape(-1)
        o[k, :min(len(ov), MAX_R)] = ov[:MAX_R]
    al = None if align is None else np.array([-1 if a is None else int(a) for a in align], dtype=np.int32)
    flat = np.concatenate(p) if p else np.zeros(0)
    return np.ascontiguousarray(flat, dtype=np.float64), n, Rv, o, al


def symbols_many(prompts, R, overlays, align=None, engine=None):
    """gacq_navsym on K channels in one launch: a list of (alignment, E int64 [R], A, q int8) per channel"""
    K = len(prompts)
    flat, n, Rv, o, al = navsym_arrays(prompts, R, overlays, align)
    if len(overlays) != K or len(Rv) != K or (al is not None and len(al) != K):
        raise ValueError("need one R, one overlay and one alignment per channel")
    for k in range(K):
        if 1 <= Rv[k] <= MAX_R and len(np.asarray(overlays[k]).reshape(-1)) != Rv[k]:
            raise ValueError("channel %d: the overlay needs R = %d values" % (k, Rv[k]))
    qoff = np.concatenate([[0], np.cumsum(n // np.maximum(Rv, 1))]).astype(np.int64)
    eng = _engine(engine)
    a_out = np.zeros(max(K, 1), dtype=np.int32)
    e_out = np.zeros((max(K, 1), MAX_R), dtype=np.int64)
    A_out = np.zeros(max(K, 1), dtype=np.float64)
    q_out = np.zeros(int(qoff[-1]) + 1, dtype=np.int8)
    nq = np.zeros(max(K, 1), dtype=np.int32)
    if flat.size == 0:
        flat = np.zeros(1)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    nat.check(nat.lib.gacq_navsym(eng._ctx, ptr(flat), ptr(n), ptr(Rv), ptr(o), None if al is None else ptr(al), K, ptr(a_out), ptr(e_out), ptr(A_out),
                                  ptr(q_out), ptr(nq)), eng._ctx)
    return [(int(a_out[k]), e_out[k, :Rv[k]].copy(), float(A_out[k]), q_out[qoff[k]:qoff[k] + nq[k]].copy()) for k in range(K)]


def symbols(prompts, name, item=None, align=None, engine=None):
    """Soft symbols of one channel of tracker ``name`` (``item``: its PRN, for overlays that depend on it -- none of the table's do):
    (alignment, E, A, q).  ``align`` skips the search."""
    f = get_format(name)
    return symbols_many([prompts], [f.R], [overlay(name)], None if align is None else [align], engine)[0]


def job(sym_base, steps, bit_base=0, rows=0, cols=0, start=0, end=0, first_bit=0, nbits=None, g2_inverted=False):
    return VitJob(int(sym_base), int(bit_base), int(steps), int(rows), int(cols), int(start), int(end), int(first_bit),
                  int(steps - first_bit if nbits is None else nbits), int(bool(g2_inverted)))


def viterbi_jobs(sym, jobs, nbits, engine=None):
    """gacq_viterbi_dev: one launch for all jobs (VitJob) on the int8 soft symbols ``sym``; (bits uint8 [nbits], metrics int32 [J])"""
    torch = nat.require_torch()
    eng = _engine(engine)
    q = np.ascontiguousarray(sym, dtype=np.int8).reshape(-1)
    J = len(jobs)
    arr = (VitJob * max(J, 1))(*jobs)
    rc = nat.lib.gacq_viterbi_check(ctypes.addressof(arr), J, len(q), int(nbits))
    if rc < 0:
        nat.check(rc, None)
    dev = torch.device("cuda", eng.device)
    eng.use_torch_stream(dev)
    d_q = torch.from_numpy(q).to(dev)
    d_bits = torch.zeros(max(int(nbits), 1), dtype=torch.uint8, device=dev)
    d_met = torch.zeros(J, dtype=torch.int32, device=dev)
    nat.check(nat.lib.gacq_viterbi_dev(eng._ctx, ctypes.c_void_p(d_q.data_ptr()), len(q), ctypes.addressof(arr), J, ctypes.c_void_p(d_bits.data_ptr()),
                                       int(nbits), ctypes.c_void_p(d_met.data_ptr())), eng._ctx)
    return d_bits.cpu().numpy()[:int(nbits)], d_met.cpu().numpy()


def viterbi_blocks(blocks, gather=None, g2_inverted=False, start=0, end=0, engine=None):
    """J terminated decodes of equal length in one launch: ``blocks`` int8 [J, 2 steps] as received, ``gather`` = (rows, cols) of the
    de-interleaver or None, start / end state (-1: every state starts at 0 / the best end state).  (bits uint8 [J, steps], metrics)."""
    b = np.ascontiguousarray(blocks, dtype=np.int8)
    if b.ndim != 2 or b.shape[1] % 2 or b.shape[1] < 2:
        raise ValueError("blocks must be [J, 2 steps]")
    J, steps = b.shape[0], b.shape[1] // 2
    rows, cols = gather or (0, 0)
    jobs = [job(i * 2 * steps, steps, i * steps, rows, cols, start, end, 0, steps, g2_inverted) for i in range(J)]
    bits, met = viterbi_jobs(b, jobs, J * steps, engine)
    return bits.reshape(J, steps), met


def stream_jobs(T, sym_base=0, bit_base=0, chunk_bits=CHUNK_BITS, warm=WARM, g2_inverted=False):
    """The jobs of a stream of T steps: job c writes bits [c L, (c + 1) L) and runs the trellis from max(0, c L - W) to
    min(T, (c + 1) L + W), every state starting at 0, ending in the best state"""
    L, W = int(chunk_bits), int(warm)
    if L < 1 or W < 0 or L + 2 * W > MAX_STEPS:
        raise ValueError("need chunk_bits >= 1, warm >= 0 and chunk_bits + 2 warm <= 2^20")
    out = []
    for c in range(-(-int(T) // L)):
        lo, hi = max(0, c * L - W), min(T, (c + 1) * L + W)
        out.append(job(sym_base + 2 * lo, hi - lo, bit_base + c * L, 0, 0, -1, -1, c * L - lo, min(T, (c + 1) * L) - c * L, g2_inverted))
    return out


def viterbi_stream(q, chunk_bits=CHUNK_BITS, warm=WARM, g2_inverted=False, engine=None, max_jobs=None):
    """A continuous stream: q int8, symbol pairs from q[0]; (bits uint8 [len(q) div 2], metric of each chunk).  The bits are a function
    of (q, chunk_bits, warm) alone; max_jobs splits the jobs over several launches."""
    q = np.ascontiguousarray(q, dtype=np.int8).reshape(-1)
    T = len(q) // 2
    if T < 1:
        return np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.int32)
    jobs = stream_jobs(T, 0, 0, chunk_bits, warm, g2_inverted)
    step = len(jobs) if not max_jobs else int(max_jobs)
    bits, mets = np.zeros(T, dtype=np.uint8), []
    for i in range(0, len(jobs), step):
        part = jobs[i:i + step]
        lo, hi = part[0].bit_base, part[-1].bit_base + part[-1].nbits
        for j in part:
            j.bit_base -= lo
        b, m = viterbi_jobs(q, part, hi - lo, engine)
        bits[lo:hi] = b
        mets.append(m)
    return bits, np.concatenate(mets)


# ------------------------------------------------------------------------------------------------ framing

def hard(q):
    """Hard bits of soft symbols: positive means 0, and so does an erasure"""
    return (np.asarray(q) < 0).astype(np.uint8)


def find(bits, pattern):
    """Every offset at which ``pattern`` occurs in ``bits``"""
    b, p = np.asarray(bits, dtype=np.uint8), np.asarray(pattern, dtype=np.uint8)
    if len(b) < len(p):
        return np.zeros(0, dtype=np.int64)
    hit = np.ones(len(b) - len(p) + 1, dtype=bool)
    for i, v in enumerate(p):
        hit &= b[i:len(b) - len(p) + 1 + i] == v
    return np.nonzero(hit)[0]


def frame_lnav(q, f, align, all_candidates=False):
    """Subframes: at every offset >= 2 where, in either polarity, the eight bits after removing D30* are the preamble, ten words are
    checked.  Reported: those whose TLM and HOW pass with the HOW's D29 = D30 = 0 and a subframe id 1..5 (all_candidates: every one)."""
    h = hard(q)
    out = []
    for i in range(2, len(h) - 299):
        for pol in (0, 1):
            b = h[i - 2:i + 300] ^ np.uint8(pol)
            if not np.array_equal(b[2:10] ^ b[1], PREAMBLE):
                continue
            d29, d30 = int(b[0]), int(b[1])
            ok, src = [], []
            for w in range(10):
                word = b[2 + 30 * w:32 + 30 * w]
                good, d = lnav_check(word, d29, d30)
                ok.append(good)
                src.append(d)
                d29, d30 = int(word[28]), int(word[29])
            how = b[32:62]
            sfid = int_of(src[1][19:22])
            if not all_candidates and not (ok[0] and ok[1] and how[28] == 0 and how[29] == 0 and 1 <= sfid <= 5):
                continue
            out.append(Frame("lnav", align + i * f.R, i, bool(pol), all(ok), b[2:].copy(),
                             dict(subframe=sfid, tow=int_of(src[1][:17]), words="".join("1" if g else "0" for g in ok))))
    return out


def cnav_streams(q):
    """The two symbol-pair alignments of a CNAV stream: [(offset, symbols)], each with at least one pair"""
    return [(a, q[a:a + (len(q) - a) // 2 * 2]) for a in (0, 1) if len(q) - a >= 2]


def frame_cnav(decoded, f, align, all_candidates=False):
    """decoded: [(pair alignment, bits)].  Messages: wherever the preamble or its inverse starts 300 decoded bits; reported: those
    whose CRC-24Q passes (all_candidates: every one)."""
    out = []
    for a, bits in decoded:
        for pol in (0, 1):
            b = np.asarray(bits, dtype=np.uint8) ^ np.uint8(pol)
            for i in find(b[:max(0, len(b) - 292)], PREAMBLE):
                m = b[i:i + 300]
                if len(m) < 300:
                    continue
                ok = crc24q(m[:276]) == int_of(m[276:])
                if ok or all_candidates:
                    sym = a + 2 * int(i)
                    out.append(Frame("cnav", align + sym * f.R, sym, bool(pol), ok, m.copy(),
                                     dict(prn=int_of(m[8:14]), type=int_of(m[14:20]), tow=int_of(m[20:37]))))
    out.sort(key=lambda fr: (fr.symbol, fr.inverted))
    return out


def inav_candidates(q):
    """[(offset of the sync pattern, polarity)] of every page part that fits: the hard symbols equal the pattern or its inverse"""
    h = hard(q)[:max(0, len(q) - INAV_PART_SYMBOLS + len(INAV_SYNC))]
    c = [(int(i), 0) for i in find(h, INAV_SYNC)] + [(int(i), 1) for i in find(h, INAV_SYNC ^ 1)]
    return sorted(c)


def inav_blocks(q, cands):
    """int8 [J, 240]: the symbols after each candidate's sync pattern with its polarity applied"""
    q = np.asarray(q, dtype=np.int8)
    out = np.zeros((len(cands), 240), dtype=np.int8)
    for k, (i, pol) in enumerate(cands):
        out[k] = q[i + 10:i + 250] * (-1 if pol else 1)
    return out


def frame_inav(cands, parts, f, align, all_candidates=False):
    """cands: inav_candidates; parts: their decoded 120 bits.  Pages: a candidate and the one 250 symbols later in the same polarity,
    the first an even part, the second an odd one; CRC-24Q over the even part without its tail and the first 82 bits of the odd part.
    Reported: the pages whose CRC passes (all_candidates: every pair of candidates 250 symbols apart)."""
    at = {c: k for k, c in enumerate(cands)}
    out = []
    for k, (i, pol) in enumerate(cands):
        k2 = at.get((i + INAV_PART_SYMBOLS, pol))
        if k2 is None:
            continue
        even, odd = np.asarray(parts[k], dtype=np.uint8), np.asarray(parts[k2], dtype=np.uint8)
        shaped = even[0] == 0 and odd[0] == 1
        ok = bool(shaped and crc24q(np.concatenate([even[:114], odd[:82]])) == int_of(odd[82:106]))
        if ok or all_candidates:
            out.append(Frame("inav", align + i * f.R, i, bool(pol), ok, np.concatenate([even[:114], odd[:114]]),
                             dict(even_odd=(int(even[0]), int(odd[0])), page_type=int(even[1]), word_type=int_of(even[2:8]))))
    return out


FRAMERS = {"lnav": frame_lnav, "cnav": frame_cnav, "inav": frame_inav}


def decode_many(channels, all_candidates=False, chunk_bits=CHUNK_BITS, warm=WARM, engine=None):
    """channels: (records or prompts, tracker name, item) each.  One gacq_navsym launch forms the symbols of all channels, one
    gacq_viterbi_dev launch decodes every page part and every stream chunk of all of them; the framing runs on the host.
    Returns one list of Frame per channel."""
    channels = list(channels)
    if not channels:
        return []
    fmts = [get_format(name) for _, name, _ in channels]
    syms = symbols_many([c[0] for c in channels], [f.R for f in fmts], [overlay(c[1]) for c in channels], None, engine)
    pieces, jobs, plan, nsym, nbits = [], [], [], 0, 0
    for f, (align, _, _, q) in zip(fmts, syms):
        if f.fec == "block":
            cands = inav_candidates(q)
            blocks = inav_blocks(q, cands)
            plan.append((cands, nbits))
            for k in range(len(cands)):
                jobs.append(job(nsym + 240 * k, INAV_PART_BITS, nbits + INAV_PART_BITS * k, INAV_ROWS, INAV_COLS, 0, 0, 0, INAV_PART_BITS, f.g2_inverted))
            pieces.append(blocks.reshape(-1))
            nsym += blocks.size
            nbits += INAV_PART_BITS * len(cands)
        elif f.fec == "stream":
            streams = []
            for a, s in cnav_streams(q):
                T = len(s) // 2
                jobs += stream_jobs(T, nsym, nbits, chunk_bits, warm, f.g2_inverted)
                streams.append((a, nbits, T))
                pieces.append(s)
                nsym += len(s)
                nbits += T
            plan.append(streams)
        else:
            plan.append(None)
    bits = viterbi_jobs(np.concatenate(pieces), jobs, nbits, engine)[0] if jobs else np.zeros(0, dtype=np.uint8)
    out = []
    for f, (align, _, _, q), p in zip(fmts, syms, plan):
        if f.fec == "block":
            cands, base = p
            parts = bits[base:base + INAV_PART_BITS * len(cands)].reshape(len(cands), INAV_PART_BITS)
            out.append(frame_inav(cands, parts, f, align, all_candidates))
        elif f.fec == "stream":
            out.append(frame_cnav([(a, bits[base:base + T]) for a, base, T in p], f, align, all_candidates))
        else:
            out.append(FRAMERS[f.message](q, f, align, all_candidates))
    return out


def decode(records_or_prompts, name, item=None, all_candidates=False, engine=None, **kw):
    """The frames of one channel: records (trackloop.RECORD_DTYPE) or prompt real parts of tracker ``name``"""
    return decode_many([(records_or_prompts, name, item)], all_candidates, engine=engine, **kw)[0]


# ------------------------------------------------------------------------------------------------ command line

def format_frame(name, item, fr):
    fields = " ".join("%s %s" % (k, "".join(str(x) for x in v) if isinstance(v, (tuple, list)) else v) for k, v in fr.fields.items())
    return "nav %s %d %s record %d %s%s %s" % (name, int(item or 0), fr.message, fr.record, "ok" if fr.ok else "FAIL", " inverted" if fr.inverted else "",
                                               fields)


def read_prompts(lines):
    """Column 1 of the track scripts' output lines (the prompt's real part); empty lines are skipped"""
    out = []
    for n, line in enumerate(lines):
        f = line.split()
        if not f:
            continue
        if len(f) < 2:
            raise ValueError("line %d: no prompt column" % (n + 1))
        out.append(float(f[1]))
    return np.array(out, dtype=np.float64)


def build_parser():
    ap = argparse.ArgumentParser(prog="navdata", description="Decode navigation frames from a tracker's output lines on the GPU")
    ap.add_argument("tracker", help="one of: %s" % " ".join(sorted(FORMATS)))
    ap.add_argument("--prn", type=int, default=0, help="PRN, printed on every line")
    ap.add_argument("--all-candidates", action="store_true", help="also print the sync hits whose checks fail")
    ap.add_argument("--device", type=int, default=0, help="GPU index")
    ap.add_argument("input_filename", help="the tracker's output, or - for stdin")
    return ap


def parse(argv):
    a = build_parser().parse_args(list(argv))
    if a.tracker not in FORMATS:
        raise SystemExit("navdata: no navigation message format for tracker %r (the formats: %s)" % (a.tracker, ", ".join(sorted(FORMATS))))
    return a


def run(argv, out=None):
    a = parse(argv)
    out = sys.stdout if out is None else out
    if a.input_filename == "-":
        p = read_prompts(sys.stdin)
    else:
        with open(a.input_filename) as f:
            p = read_prompts(f)
    from . import acquire
    eng = acquire.Engine(a.device)
    try:
        frames = decode(p, a.tracker, a.prn, a.all_candidates, engine=eng)
    finally:
        eng.close()
    lines = [format_frame(a.tracker, a.prn, fr) for fr in frames]
    for line in lines:
        print(line, file=out)
    return lines


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    if not argv or argv[0] in ("-h", "--help"):
        print(__doc__)
        return 0
    run(argv)
    return 0


if __name__ == "__main__":
    sys.exit(main())
