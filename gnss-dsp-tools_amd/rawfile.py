"""Bounded reading of raw int8 I/Q recordings for the utilities (spectrum, squaring): the reference's scripts read one frame or one
chunk at a time with gnsstools/io.py:3-12 and stop at the first short read; here a piece is many such units, so that one upload feeds
one launch, and a long recording (or /dev/stdin) never has to fit in memory."""
import numpy as np

PIECE_BYTES = 1 << 26


def read_pieces(fp, unit_bytes, piece_bytes=PIECE_BYTES):
    """Yield int8 arrays holding whole units of unit_bytes bytes, at most max(1, piece_bytes // unit_bytes) units each, until the
    file ends; a trailing partial unit is dropped (io.get_samples_complex returns None on a short read and the scripts stop)."""
    unit_bytes = int(unit_bytes)
    if unit_bytes <= 0:
        raise ValueError("unit must be at least one byte")
    want = max(1, int(piece_bytes) // unit_bytes) * unit_bytes
    while True:
        z = fp.read(want)
        # a pipe may return less than asked for before its end: keep reading until the piece is full or the file is over
        while 0 < len(z) < want:
            more = fp.read(want - len(z))
            if not more:
                break
            z += more
        whole = (len(z) // unit_bytes) * unit_bytes
        if whole:
            yield np.frombuffer(z, dtype=np.int8, count=whole)
        if len(z) < want:
            return


def device_int8(eng, iq_int8):
    """numpy int8 ([n, 2] or flat interleaved) or a torch int8 CUDA tensor -> flat, contiguous, 16-byte aligned CUDA tensor"""
    from . import _native as nat
    torch = nat.require_torch()
    if not torch.is_tensor(iq_int8):
        iq_int8 = torch.from_numpy(np.array(iq_int8, dtype=np.int8, copy=True).reshape(-1)).to("cuda:%d" % eng.device)
    if iq_int8.dtype != torch.int8 or not iq_int8.is_cuda:
        raise ValueError("samples must be int8: a numpy array or a CUDA tensor")
    eng.use_torch_stream(iq_int8.device)        # as Engine.mix_int8_dev: torch-owned temporaries and the context's stream
    iq_int8 = iq_int8.contiguous().view(-1)
    if iq_int8.data_ptr() % 16:
        iq_int8 = iq_int8.clone()
    return iq_int8
