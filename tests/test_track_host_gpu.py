"""The host side of the three tracking handles through the C ABI alone: which error each bad spec or launch argument gets from
gacq_track_open / gacq_longtrack_open / gacq_chiptrack_open and their *_run_dev (the exact return code, the channel named in the
message, no handle), and the state gacq_chiptrack_open starts a channel from -- the bytes gacq_track_open gives the same spec."""
import ctypes

import numpy as np
import pytest

from gnss_dsp_tools_amd import _native as nat
from gnss_dsp_tools_amd import acquire
from gnss_dsp_tools_amd.trackloop import RECORD_DTYPE, STATE_DTYPE, TrackSpec

BAD_ARG, UNKNOWN_CODE, BAD_PRN, UNSUPPORTED = -1, -2, -3, -9       # GACQ_ERR_* of include/gacq.h
NAN = float("nan")
FS = 4.092e6
L_CA = 1023
WIN_CHIPS = 16384            # the long-code kernel's chip window


def spec(**fields):
    """A good gps.ca channel (kind 0: every entry point takes it), with some fields replaced."""
    s = dict(code=b"gps.ca", prn=3, kind=0, subs=1, fixed_pll=0, glonass=0, pad=0, fs=FS, period=0.001, rate=1000.0, ratio=1540.0,
             spacing=0.05, chip_rate=1.023e6, fll_k_wide=3.0, fll_k_narrow=0.8, pll_k1=0.1, pll_k2=3.5, dll_k1=0.00002, dll_k2=0.2,
             coffset=0.0, fm=0.0, code_offset=10.0, doppler=0.0, carrier_phase=0.0, dwell_wide=500.0, dwell_narrow=500.0)
    s.update(fields)
    return TrackSpec(**s)


# bad fields of channel 1 and the code every entry point returns for them
COMMON = [(dict(fs=0.0), BAD_ARG), (dict(fs=NAN), BAD_ARG), (dict(fs=-FS), BAD_ARG),
          (dict(code_offset=float(L_CA)), BAD_ARG), (dict(code_offset=-0.5), BAD_ARG), (dict(code_offset=NAN), BAD_ARG),
          (dict(prn=1000), BAD_PRN), (dict(code=b"no.such"), UNKNOWN_CODE), (dict(subs=0), BAD_ARG), (dict(ratio=0.0), BAD_ARG),
          (dict(spacing=-0.5), BAD_ARG), (dict(carrier_phase=7.0), BAD_ARG)]
# ... and those of one entry point: a kind outside its set, one sub-block more than it takes, a code too long for it
OPEN_CASES = {
    "gacq_track": COMMON + [(dict(kind=6), BAD_ARG), (dict(kind=-1), BAD_ARG), (dict(subs=65), BAD_ARG),
                            (dict(code=b"gps.l2cl"), UNSUPPORTED)],
    # any length goes; the early/late spacing must stay below a quarter of the chip window
    "gacq_longtrack": COMMON + [(dict(kind=2), BAD_ARG), (dict(subs=1501), BAD_ARG), (dict(spacing=0.25 * WIN_CHIPS), BAD_ARG)],
    "gacq_chiptrack": COMMON + [(dict(kind=1), UNSUPPORTED), (dict(subs=65), BAD_ARG), (dict(code=b"gps.l2cl"), UNSUPPORTED),
                                (dict(glonass=1), UNSUPPORTED)],
}
ENTRIES = sorted(OPEN_CASES)


def _open(eng, entry, specs, h, thr="default"):
    fn = getattr(nat.lib, entry + "_open")
    if entry != "gacq_chiptrack":
        return fn(eng._ctx, specs, len(specs), ctypes.byref(h))
    if thr == "default":
        thr = np.full(len(specs), 200, dtype=np.int64)
    return fn(eng._ctx, specs, len(specs), None if thr is None else thr.ctypes.data_as(ctypes.c_void_p), ctypes.byref(h))


def _message(eng):
    return (nat.lib.gacq_last_error(eng._ctx) or b"").decode()


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ENTRIES)
def test_open_reports_the_bad_channel(entry):
    eng = acquire.default_engine()
    for fields, want in OPEN_CASES[entry]:
        specs = (TrackSpec * 2)(spec(), spec(**fields))
        h = ctypes.c_void_p(1)
        rc = _open(eng, entry, specs, h)
        print(entry, fields, rc, _message(eng))
        assert rc == want and "channel 1" in _message(eng) and not h.value, (entry, fields, rc, _message(eng))


@pytest.mark.gpu
def test_chiptrack_open_needs_its_thresholds():
    """No channel is at fault here: the message names the missing threshold array"""
    eng = acquire.default_engine()
    h = ctypes.c_void_p(1)
    rc = _open(eng, "gacq_chiptrack", (TrackSpec * 2)(spec(), spec()), h, thr=None)
    print(rc, _message(eng))
    assert rc == BAD_ARG and "threshold" in _message(eng) and not h.value


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ENTRIES)
def test_run_dev_rejects_bad_launch_arguments(entry):
    torch = nat.require_torch()
    eng = acquire.default_engine()
    eng.use_torch_stream(torch.device("cuda", eng.device))
    subs = 2
    specs = (TrackSpec * 2)(spec(), spec(subs=subs, period=0.002, rate=500.0))
    n0 = int(FS * 0.002 * ((L_CA - 10.0) / L_CA))                # where channel 1's first block starts
    h = ctypes.c_void_p()
    nat.check(_open(eng, entry, specs, h), eng._ctx)
    try:
        x = torch.zeros(2 * 4092, dtype=torch.int8, device="cuda:%d" % eng.device)
        recs = np.zeros((2, 4), dtype=RECORD_DTYPE)
        counts = np.zeros(2, dtype=np.int32)
        status = np.zeros(2, dtype=np.int32)

        def run(max_records=4, rec_cap=4, ptr1=x.data_ptr(), base1=0):
            ptrs = (ctypes.c_void_p * 2)(x.data_ptr(), ptr1)
            base = np.array([0, base1], dtype=np.int64)
            avail = np.full(2, x.numel() // 2, dtype=np.int64)
            rc = getattr(nat.lib, entry + "_run_dev")(h, ptrs, base.ctypes.data_as(ctypes.c_void_p), avail.ctypes.data_as(ctypes.c_void_p),
                                                      max_records, recs.ctypes.data_as(ctypes.c_void_p), rec_cap,
                                                      counts.ctypes.data_as(nat.c_int_p), status.ctypes.data_as(nat.c_int_p))
            print(entry, max_records, rec_cap, ptr1 is None, base1, rc, _message(eng))
            return rc, _message(eng)

        for kw, part in ((dict(max_records=subs - 1), "max_records"), (dict(max_records=4, rec_cap=3), "max_records"),
                         (dict(ptr1=None), "channel 1"), (dict(base1=-1), "channel 1"), (dict(base1=n0 + 1), "channel 1")):
            rc, msg = run(**kw)
            assert rc == BAD_ARG and msg.startswith(entry + "_run_dev:") and part in msg, (entry, kw, rc, msg)
        assert not counts.any() and not recs.tobytes().strip(b"\0")      # nothing was launched or written
    finally:
        getattr(nat.lib, entry + "_close")(h)


@pytest.mark.gpu
def test_chiptrack_starts_from_the_template_state():
    """Right after open, before any launch: one channel aligned with the code boundary already, one a fraction of a chip into the code"""
    eng = acquire.default_engine()
    b2b = dict(code=b"beidou.b2bi", prn=21, fs=69.984e6, ratio=118.0, spacing=0.5, chip_rate=10.23e6, doppler=1200.0, carrier_phase=0.1)
    specs = (TrackSpec * 2)(spec(code_offset=0.0, **b2b), spec(code_offset=831.15, **b2b))
    states = {}
    for entry in ("gacq_track", "gacq_chiptrack"):
        h = ctypes.c_void_p()
        nat.check(_open(eng, entry, specs, h), eng._ctx)
        try:
            st = np.zeros(2, dtype=STATE_DTYPE)
            for k in range(2):
                nat.check(getattr(nat.lib, entry + "_state")(h, k, st[k:].ctypes.data_as(ctypes.c_void_p)), eng._ctx)
            states[entry] = st
        finally:
            getattr(nat.lib, entry + "_close")(h)
    got, want = states["gacq_chiptrack"], states["gacq_track"]
    assert got.tobytes() == want.tobytes(), (got, want)
    # the alignment of the scripts: n = int(fs*period*((L-code_offset)/L)) samples skipped, code_offset += n*rate*L/fs
    n = [int(69.984e6 * 0.001 * ((10230 - off) / 10230)) for off in (0.0, 831.15)]
    assert [int(p) for p in want["pos"]] == n
    assert [float(c) for c in want["code_p"]] == [off + m * 1000.0 * 10230.0 / 69.984e6 for off, m in zip((0.0, 831.15), n)]
