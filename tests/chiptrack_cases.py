"""Shared helpers of the chip-accumulator tracking tests: the golden cases of tools/make_goldens_chiptrack.py, their synthetic
recordings (regenerated from a seed, not stored: each is several MB) and the oracle's lines and bins.  numpy and codes.chips only."""
import gzip
import hashlib
import json
import os

import numpy as np

from gnss_dsp_tools_amd import chiptrack, codes

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
NOISE = 18.0
CHUNK = 1 << 22


def load():
    with gzip.open(os.path.join(GOLD, "chiptrack_cases.json.gz"), "rt") as f:
        return json.load(f)


def synth(tracker, fs, coffset, prn, doppler, code_offset, seconds, amp, seed, noise=NOISE):
    """Interleaved int8 I/Q: noise (sigma `noise` per component) + amp * code(code_offset + chip_rate/fs * i) *
    exp(2 pi i f i / fs), f = coffset + doppler.  Built in chunks of CHUNK samples from one PCG64 stream."""
    code = chiptrack.CHIP_TRACKERS[tracker].code
    c = codes.chips(code, prn)
    L = len(c)
    rate = codes.chip_rate(code) / fs
    f = coffset + doppler
    n = int(round(fs * seconds))
    rng = np.random.Generator(np.random.PCG64(seed))
    out = np.empty((n, 2), dtype=np.int8)
    for s in range(0, n, CHUNK):
        e = min(n, s + CHUNK)
        i = np.arange(s, e, dtype=np.float64)
        x = noise * rng.standard_normal((e - s, 2))
        w = amp * (1.0 - 2.0 * c[np.mod(np.floor(code_offset + rate * i).astype(np.int64), L)])
        ang = 2 * np.pi * np.mod(f / fs * i, 1.0)
        out[s:e, 0] = np.clip(np.round(x[:, 0] + w * np.cos(ang)), -127, 127)
        out[s:e, 1] = np.clip(np.round(x[:, 1] + w * np.sin(ang)), -127, 127)
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
    _, ch = chiptrack.parse(case["tracker"], argv_of(case, path))
    return ch


def chips_lines(case):
    return gzip.decompress(bytes.fromhex(case["chips_gz"])).decode().splitlines()


def oracle(case, iq, **kw):
    """(records, stdout lines, bins, signs) of the oracle on a golden case."""
    from chiptrack_oracle import track as oracle_track
    ch = channel_of(case)
    spec = chiptrack.chip_channel_spec(ch)
    chips01 = codes.chips(chiptrack.CHIP_TRACKERS[ch.name].code, spec.prn)
    recs, bins, signs = oracle_track(spec, chips01, iq, **kw)
    arr = np.zeros(len(recs), dtype=chiptrack.RECORD_DTYPE)
    for i, r in enumerate(recs):
        for k, v in r.items():
            arr[i][k] = v
    return arr, chiptrack.format_lines(ch.name, arr), bins, signs
