"""Seeded inputs shared by tests/test_coherent_cpu.py and tests/test_coherent_gpu.py.

RECORDINGS: noise (sigma 1 per component) plus satellites that carry a secondary code or a data-bit edge, a Doppler on the fine grid
and a known delay, at an amplitude where one period alone does not show them.  A satellite's period p = floor((i - delay) / n) carries
the chip secondary[(p + h0) % S], negated from period flip_at on; the search windows start at multiples of n, so window m holds period
m from sample `delay` on (an unpadded signal's circular correlation also sees the tail of period m - 1 in its first `delay` samples,
hence the short delays for gps-l1).  Amplitudes and seeds were fixed on the CPU by the rule of the coherent-search issue: the oracle
chain (fp64 fold + oracle.acq_oracle) finds the true (d, h, code_offset) for every seed listed; DESIGN 5.16 has the margins.

FOLD_CASES: the shapes of the device fold test."""
import numpy as np

from gnss_dsp_tools_amd import codes, coherent, signals

NH10 = np.array([1, 1, 1, 1, -1, -1, 1, -1, 1, -1], dtype=np.int8)

# key -> signal, M, secondary argument of coherent.search, data_flip, fine Doppler grid, satellites, seeds
RECORDINGS = {
    "supplied": dict(signal="gps-l1", M=10, secondary=NH10, data_flip=False, dopplers=1000.0 + 50.0 * np.arange(-2, 3),
                     sats=[dict(item=7, amp=0.05, d=3, delay=301, h0=4, flip_at=None)], seeds=(1, 2, 3, 4, 5, 6)),
    "nh20": dict(signal="beidou-b1i", M=20, secondary="builtin", data_flip=False, dopplers=-2000.0 + 25.0 * np.arange(-2, 3),
                 sats=[dict(item=11, amp=0.025, d=1, delay=5003, h0=13, flip_at=None)], seeds=(1, 2, 3, 4, 5, 6)),
    "flip": dict(signal="gps-l1", M=20, secondary=None, data_flip=True, dopplers=-500.0 + 25.0 * np.arange(-2, 3),
                 sats=[dict(item=19, amp=0.05, d=2, delay=77, h0=0, flip_at=7)], seeds=(3, 6, 7, 8, 11, 12)),
    "table": dict(signal="galileo-e6c", M=12, secondary="builtin", data_flip=False, dopplers=750.0 + 50.0 * np.arange(-1, 2),
                  sats=[dict(item=3, amp=0.03, d=1, delay=9001, h0=42, flip_at=None),
                        dict(item=24, amp=0.03, d=1, delay=6000, h0=60, flip_at=None)], seeds=(1, 2, 3, 4, 5, 6)),
}


def secondary_of(rec, item):
    """the +-1 chips the satellite `item` of a recording carries (None: no overlay)"""
    sec = rec["secondary"]
    if isinstance(sec, str):
        sec = coherent.builtin_secondary(rec["signal"])
    if isinstance(sec, dict):
        sec = sec[item]
    return sec


def samples(rec):
    sig = signals.get(rec["signal"])
    return (rec["M"] - 1) * sig.n + sig.samples_needed(1) + sig.n


def recording(key, seed):
    """complex64 at the signal's rate; sample 0 is absolute sample 0"""
    rec = RECORDINGS[key]
    sig = signals.get(rec["signal"])
    nsamp = samples(rec)
    rng = np.random.Generator(np.random.PCG64([seed, sum(key.encode())]))
    x = rng.standard_normal(nsamp) + 1j * rng.standard_normal(nsamp)
    i = np.arange(nsamp)
    for s in rec["sats"]:
        rep = codes.replica(sig.code, s["item"], sig.n, sig.boc).astype(np.float64)
        p = (i - s["delay"]) // sig.n
        sec = secondary_of(rec, s["item"])
        sign = np.ones(nsamp) if sec is None else np.asarray(sec, dtype=np.float64)[(p + s["h0"]) % len(sec)]
        if s["flip_at"] is not None:
            sign = np.where(p >= s["flip_at"], -sign, sign)
        x += s["amp"] * sign * rep[(i - s["delay"]) % sig.n] * np.exp(2j * np.pi * rec["dopplers"][s["d"]] * i / sig.fs)
    return x.astype(np.complex64)


def truth(key, sat):
    """(d, h, code_offset) the search has to return for satellite `sat` of a recording: h is the row of patterns() that equals the
    satellite's signs over the M windows up to a global sign"""
    rec = RECORDINGS[key]
    sig = signals.get(rec["signal"])
    W, labels = coherent.patterns(secondary_of(rec, sat["item"]), rec["M"], rec["data_flip"])
    m = np.arange(rec["M"])
    sec = secondary_of(rec, sat["item"])
    want = np.ones(rec["M"]) if sec is None else np.asarray(sec)[(m + sat["h0"]) % len(sec)]
    if sat["flip_at"] is not None:
        want = np.where(m >= sat["flip_at"], -want, want)
    hit = [h for h in range(len(W)) if np.array_equal(W[h] * W[h][0], want * want[0])]
    assert len(hit) == 1, (key, hit)
    L = codes.code_length(sig.code)
    c = L * (float((sig.nfft - sat["delay"]) % sig.nfft) / sig.n)       # r = ifft(C conj(fft(x))) peaks at minus the delay
    return sat["d"], hit[0], (c % L if sig.fold else c)


# --- device fold cases: (n_out, M, H) of the issue, D = 1 and 7, and the variations spread over them ---------------------------------
FS = 4096000.0
F7 = np.array([-5012.5, -1000.0, -25.0, 0.0, 25.0, 1537.0, 6999.0])
FOLD_CASES = {
    "4096x1x1": dict(n_out=4096, M=1, H=1, f=[1537.0], period=4096),
    "4096x20x33": dict(n_out=4096, M=20, H=33, f=F7, period=4096, j0=2 ** 40 + 12345),
    "4096x10x40 zeros": dict(n_out=4096, M=10, H=40, f=F7, period=4096, zeros=True, carrier_hz=1575.42e6 / 4000.0),
    "61380x5x5": dict(n_out=61380, M=5, H=5, f=F7, period=30690, fs=30690000.0),
    "16384x100x100": dict(n_out=16384, M=100, H=100, f=[-3262.0], period=8192, fs=8192000.0),
    "1000x3x2 odd wide": dict(n_out=1000, M=3, H=2, f=[-409.0], period=1001, odd=True, wide=True),
    "1000x3x2 odd": dict(n_out=1000, M=3, H=2, f=F7, period=777, odd=True, j0=-3),
}


def fold_case(name):
    """(x, n_out, starts [D, M], f [D], fs, W [H, M], j0) of a fold case; x complex64, or complex128 for a `wide` case"""
    c = FOLD_CASES[name]
    n_out, M, H = c["n_out"], c["M"], c["H"]
    f = np.asarray(c["f"], dtype=np.float64)
    fs = c.get("fs", FS)
    rng = np.random.Generator(np.random.PCG64([20261018, sum(name.encode())]))
    st = (np.arange(M, dtype=np.int64) * c["period"])[None, :].repeat(len(f), axis=0)
    if "carrier_hz" in c:                                # the code-Doppler slip of coherent.starts, scaled up to reach whole samples
        st = st - np.rint(st * f[:, None] / c["carrier_hz"]).astype(np.int64)
    if c.get("odd"):
        st = st + 1 + 2 * np.arange(len(f), dtype=np.int64)[:, None]
    nsamp = int(st.max()) + n_out
    x = rng.standard_normal(nsamp) + 1j * rng.standard_normal(nsamp)
    x = x if c.get("wide") else x.astype(np.complex64)
    W = rng.integers(0, 2, size=(H, M)).astype(np.int8) * 2 - 1
    if c.get("zeros"):
        W[rng.random(size=(H, M)) < 0.3] = 0
        W[3, :] = 0                                      # a whole pattern of zeros
    return x, n_out, np.ascontiguousarray(st), f, fs, W, c.get("j0", 0)
