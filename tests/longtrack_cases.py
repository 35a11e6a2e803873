"""Shared helpers of the long-code tracking tests: the golden cases of tools/make_goldens_longtrack.py, their synthetic recordings
(regenerated from a seed, not stored: each is several MB) and the oracle's output lines.  numpy and codes.chips only."""
import gzip
import hashlib
import json
import os

import numpy as np

from gnss_dsp_tools_amd import codes, longtrack, track

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
NOISE = 18.0
CHUNK = 1 << 22


def load():
    with gzip.open(os.path.join(GOLD, "longtrack_cases.json.gz"), "rt") as f:
        return json.load(f)


def synth(tracker, fs, coffset, prn, doppler, code_offset, seconds, amp, seed):
    """Interleaved int8 I/Q: noise (sigma NOISE per component) + amp * code(code_offset + chip_rate/fs * i) [* RZ gate] *
    exp(2 pi i f i / fs), f = coffset [+ offset_step * chan] + doppler.  Built in chunks of CHUNK samples from one PCG64 stream."""
    t = longtrack.LONG_TRACKERS[tracker]
    c = codes.chips(t.code, 0 if t.glonass else prn)
    L = len(c)
    rate = codes.chip_rate(t.code) / fs
    f = coffset + doppler + (t.glonass[3] * prn if t.glonass else 0)
    n = int(round(fs * seconds))
    rng = np.random.Generator(np.random.PCG64(seed))
    out = np.empty((n, 2), dtype=np.int8)
    for s in range(0, n, CHUNK):
        e = min(n, s + CHUNK)
        i = np.arange(s, e, dtype=np.float64)
        noise = NOISE * rng.standard_normal((e - s, 2))
        ph = code_offset + rate * i
        w = 1.0 - 2.0 * c[np.mod(np.floor(ph).astype(np.int64), L)]
        if t.kind == 5:
            w = w * ((np.floor(2 * ph).astype(np.int64) & 1) == 1)
        ang = 2 * np.pi * np.mod(f / fs * i, 1.0)
        out[s:e, 0] = np.clip(np.round(noise[:, 0] + amp * w * np.cos(ang)), -127, 127)
        out[s:e, 1] = np.clip(np.round(noise[:, 1] + amp * w * np.sin(ang)), -127, 127)
    return out.ravel()


def recording(case):
    """The case's recording, regenerated; checked against its stored SHA-256."""
    iq = synth(case["tracker"], case["fs"], case["coffset"], case["prn"], case["doppler"], case["code_offset"], case["seconds"],
               case["amp"], case["seed"])
    got = hashlib.sha256(iq.tobytes()).hexdigest()
    assert got == case["sha256"], (case["tracker"], case["seed"], got)
    return iq


def argv_of(case, path):
    return list(case["argv"]) + [path, repr(case["fs"]), repr(case["coffset"]), str(case["prn"]), repr(case["doppler"]),
                                 repr(case["code_offset"])]


def channel_of(case, path="recording.iq"):
    """trackloop.Channel of a golden case, parsed from its stored command line by the CLI's parser."""
    _, ch = track.parse(case["tracker"], argv_of(case, path))
    return ch


def oracle_lines(name, spec, chips01, iq, **kw):
    from longtrack_oracle import track as oracle_track
    recs = oracle_track(spec, chips01, iq, **kw)
    arr = np.zeros(len(recs), dtype=longtrack.RECORD_DTYPE)
    for i, r in enumerate(recs):
        for k, v in r.items():
            arr[i][k] = v
    return arr, longtrack.format_lines(name, arr)


def synth_many(fs, seconds, sats, seed, noise=12.0):
    """Interleaved int8 I/Q of several satellites (code, prn, amp, f Hz, code phase at sample 0), each with the RZ gate where its code
    has one (gps.l2cl), over noise of sigma `noise` per component; chunked, so that 16 MS/s recordings of a few seconds fit easily."""
    n = int(round(fs * seconds))
    tabs = [(codes.chips(code, prn), codes.chip_rate(code) / fs, code == "gps.l2cl", amp, f, ph0) for code, prn, amp, f, ph0 in sats]
    rng = np.random.Generator(np.random.PCG64(seed))
    out = np.empty((n, 2), dtype=np.int8)
    for s in range(0, n, CHUNK):
        e = min(n, s + CHUNK)
        i = np.arange(s, e, dtype=np.float64)
        x = noise * rng.standard_normal((e - s, 2))
        for c, rate, rz, amp, f, ph0 in tabs:
            ph = ph0 + rate * i
            w = amp * (1.0 - 2.0 * c[np.mod(np.floor(ph).astype(np.int64), len(c))])
            if rz:
                w = w * ((np.floor(2 * ph).astype(np.int64) & 1) == 1)
            ang = 2 * np.pi * np.mod(f / fs * i, 1.0)
            x[:, 0] += w * np.cos(ang)
            x[:, 1] += w * np.sin(ang)
        out[s:e] = np.clip(np.round(x), -127, 127)
    return out.ravel()
