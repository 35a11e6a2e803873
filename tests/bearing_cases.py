"""Cases shared by the bearing tests (test_bearing_cpu.py, test_bearing_gpu.py): arrays, direction tables, covariances and their oracle
results (computed once, never changed).  Everything here was chosen on the CPU; the end-to-end table at the bottom was recorded from
tests/scene_oracle.py and tests/bearing_oracle.py before any device run."""
import functools

import numpy as np

import bearing_oracle as B
import nulling_cases as NC
from gnss_dsp_tools_amd import bearing

LB, W, SHIFT = 256, 2, 10                           # of the covariances of the shape cases
N_BLOCKS, K = 5, 4
# one cell, a wave edge, a workgroup edge, the 5 degree grid; then one cell past what LDS holds in doubles, and the cap
SHAPES = [(M, G) for M in (2, 3, 5, 8) for G in (1, 63, 64, 65, 257, 1368)] + [(8, 20481), (2, 32768)]
COS_SEP = float(np.cos(np.deg2rad(20.0)))


def ring(M, radius=0.5):
    """M elements in wavelengths: one at the origin, the others on a ring in the horizontal plane"""
    ang = 2.0 * np.pi * np.arange(M - 1) / max(M - 1, 1)
    return np.concatenate([np.zeros((1, 3)), np.stack([radius * np.cos(ang), radius * np.sin(ang), np.zeros(M - 1)], axis=1)])


def spiral(G):
    """G (az, el) cells over the upper hemisphere, no two alike; the 5 degree grid where that has G cells"""
    if G == 1368:
        return bearing.grid(5.0)
    i = np.arange(G, dtype=np.float64)
    return np.stack([(i * 137.50776405) % 360.0, 90.0 * (i + 0.5) / G], axis=1)


@functools.lru_cache(maxsize=None)
def table(M, G):
    """(a [G, M], u [G, 3]) of the ring of M elements over spiral(G)"""
    a, u = bearing.tables(ring(M), spiral(G))
    a.setflags(write=False)
    u.setflags(write=False)
    return a, u


@functools.lru_cache(maxsize=None)
def covariances(M, n=N_BLOCKS, seed=None):
    """(re, im) int64 [n][M][M]: the window sums of blocks W + 1 .. W + n of nulling_cases.recording, every one another matrix"""
    xs = NC.recording(M, (W + n + 1) * LB, 7000 + M if seed is None else seed)
    Rre, Rim = B.window_sums(xs, LB, W, list(range(W + 1, W + 1 + n)))
    Rre.setflags(write=False)
    Rim.setflags(write=False)
    return Rre, Rim


def stacked(Rre, Rim):
    """the int64 array [n][M][M][2] of gacq_null_run_dev's d_cov"""
    return np.ascontiguousarray(np.stack([Rre, Rim], axis=3), dtype=np.int64)


@functools.lru_cache(maxsize=None)
def reference(M, G):
    """(records, floor, q) of the shape case, K = 4, 20 degrees apart"""
    a, u = table(M, G)
    out = B.run(*covariances(M), SHIFT, a, u, K, COS_SEP)
    for x in out:
        x.setflags(write=False)
    return out


# ---- exact ties: two elements on the east axis see a source and its mirror image in the axis alike, so on the 5 degree grid the cells
# (az, el) and (180 - az, el) have bit-equal a (checked by the CPU tests on the table itself) and bit-equal q
TIE_ELEMENTS = np.array([[0.0, 0.0, 0.0], [0.5, 0.0, 0.0]])


def tie_covariances(n=3):
    return covariances(2, n, 4242)


# ---- ineligible cells: an arbitrary int64 "covariance" whose second pivot is negative; one whose loaded diagonal is 0 (t = -1 at
# load_shift 0 gives d = 0: 0 / 0 in every cell); the all-zero matrix
def negative_pivot(M=3):
    R = np.zeros((1, M, M, 2), dtype=np.int64)
    for p in range(M):
        R[0, p, p, 0] = 1000 * (p + 1)
    R[0, 0, 1, 0] = R[0, 1, 0, 0] = 5000                      # 2000 - 5000^2 / 1000 < 0
    R[0, 0, 2] = (300, 700)
    R[0, 2, 0] = (300, -700)
    return R


def all_nan(M=3):
    R = np.zeros((1, M, M, 2), dtype=np.int64)
    R[0, 1, 1, 0] = -1                                        # trace -1, load_shift 0: d = 0; A = diag(0, -1, 0): piv_0 = 0, m = 0 / 0
    return R


# ---- the end-to-end scene: 8 elements, ring(8); a noise jammer of sigma 42 at (az 70, el 20), a tone of amplitude 30 at (250, 50),
# antenna noise of sigma 6; block 4096, window 8, load_shift 10, the 5 degree grid (1368 cells), K = 3, 20 degrees apart.
# Recorded on the CPU before any device run: tests/scene_oracle.py (fp64, seed 311, the tone at 151234.5 Hz) rounded to int8 (about 800
# of 114688 components of an antenna clip), the window sums of tests/nulling_oracle.py, tests/bearing_oracle.py.  Blocks 0 .. 14:
#   rank 0 (70, 20) 24.1 dB   rank 1 (250, 50) 18.3 dB   rank 2 (70, 0) 18.0 dB (a sidelobe)     in every block, the warm-up included;
#   the relative gap between the smallest and the second smallest q of a block: 0.59 .. 0.60 (cells 302 and 770 are the sources).
E2E = dict(fs=4.092e6, seed=311, sigma=6.0, jammer=(42.0, 70.0, 20.0), tone=(30.0, 151234.5, 250.0, 50.0), block=4096, window=8, load_shift=10,
           step=5.0, peaks=3, sep=20.0, blocks=14)


def e2e_scene():
    """(emitters, elements [8, 3], gains [8, 2]) of the end-to-end scene, as scene.recording takes them"""
    from gnss_dsp_tools_amd import scene
    el = ring(8)
    gains = np.stack([scene.steering(el, E2E["jammer"][1], E2E["jammer"][2]), scene.steering(el, E2E["tone"][2], E2E["tone"][3])], axis=1)
    return [scene.NoiseJammer(E2E["jammer"][0]), scene.Tone(E2E["tone"][0], E2E["tone"][1])], el, gains


def e2e_cells():
    """the grid and the indices of the two sources' cells"""
    cells = bearing.grid(E2E["step"])
    find = lambda az, el: int(np.flatnonzero((cells[:, 0] == az) & (cells[:, 1] == el))[0])
    return cells, find(E2E["jammer"][1], E2E["jammer"][2]), find(E2E["tone"][2], E2E["tone"][3])
