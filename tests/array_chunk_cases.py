"""Cases shared by the multi-chunk tests of the antenna-array tools (test_array_chunks_cpu.py, test_array_chunks_gpu.py): recordings long
enough that one gacq_null_run_dev / gacq_stap_run_dev call is cut by ar_run_dev (csrc/gacq_arrayhost.h) into several triples of launches.
Only a chunk after the first runs with pb0 = b0 - W > 0, p_off = W and warm = 0, shares an apply tile with the launch before it, indexes
the side outputs by b - own_first across launches and adds to stats[1] a second time; every other device test of both tools is one
chunk.  All recordings are nulling_cases.recording(M, n, seed) at Lb = 64, the shortest block: the fewest samples that cross a chunk.

  case  tool     M  T  W  chunk K  n (samples)                    seed  margin   chunks  compared with the oracle
  A     nulling  2  -  1  2^14     (2^14 + 3) 64 + 37             9001  1.14e-5  2       bytes, weights, cov, counts
  B     nulling  2  -  3  2^14     (2^14 + 5) 64 + 37             9002  1.81e-5  2       bytes, weights, cov, counts
  C     stap     1  3  2  2^14     (2^14 + 4) 64 + 37 + 1         9101  3.18e-6  2       bytes, weights, cov, counts
  D     stap     8  7  1  2627     (2 2627 + 3) 64 + 37 + 3       9103  2.72e-6  3       bytes, weights, counts (cov: 264 MB, left out)
  S     stap     1  3  2  2^14     (2^14 + 133) 64 + 37 + 1       9101  1.14e-5  2       the stream test alone

For stap n includes t_c extra samples; the outputs are 0 .. n - 1 - t_c.  Case D has a middle chunk, neither first nor last; its seeds
9102 and 9104 leave margins of 5.1e-7 and 9.9e-7 and are not used.  Case S is case C's configuration on a longer recording: after one
piece of more than K blocks, case C has 223 samples left, too few for the pieces of 4097 samples its stream test feeds next.  The seeds
were chosen on the CPU so that the oracle alone keeps MARGIN from a rounding tie in every block; test_array_chunks_cpu.py asserts it, and
there is no exemption for tied blocks.  K is read from the library there, so that a constant that moves fails the tests instead of
quietly putting every call back into one chunk.

Every oracle result is computed once and cached.  A call that starts past sample 0 and runs to the end of the recording is a slice of
the whole-recording result: the output is a function of the absolute index, the side outputs are those of the blocks that begin in the
range, and the clip count is the whole recording's less that of the outputs before the call, which a short oracle run counts.

Named findings: none -- every case passed on the kernels as they were.  DESIGN.md 5.25 and 5.27 have the mutations that these tests
were shown to catch."""
import functools

import numpy as np

import nulling_cases as NC
import nulling_oracle as NO
import stap_oracle as SO

MARGIN = NC.MARGIN
Lb = 64
LOAD_SHIFT = 10
GAIN_INT8, GAIN_C64 = 2.5, 1.0                    # int8 at a gain that clips, so that the count sums over launches; complex64 at gain 1
FAR_SHIFT = (1 << 32) - (1 << 19)                 # case A: the first chunk of the shifted call straddles 2^32, the second lies above it

# name -> (tool, M, T, W, K, blocks, seed, cov): the recording holds `blocks` whole blocks, 37 samples and t_c more
CASES = {
    "A": ("nulling", 2, 1, 1, 1 << 14, (1 << 14) + 3, 9001, True),
    "B": ("nulling", 2, 1, 3, 1 << 14, (1 << 14) + 5, 9002, True),
    "C": ("stap", 1, 3, 2, 1 << 14, (1 << 14) + 4, 9101, True),
    "D": ("stap", 8, 7, 1, 2627, 2 * 2627 + 3, 9103, False),
    "S": ("stap", 1, 3, 2, 1 << 14, (1 << 14) + 133, 9101, False),
}
TABLE = ("A", "B", "C", "D")                      # the cases every test runs; S is the stream test's
EDGE_CASES = ("A", "D")
MIN_CHUNKS = {"A": 2, "B": 2, "C": 2, "D": 3, "S": 2}


def tc(name):
    return SO.centre(CASES[name][2])


def samples(name):
    return CASES[name][5] * Lb + 37 + tc(name)


def outputs(name):
    """the outputs the recording supports: all but the last t_c"""
    return samples(name) - tc(name)


@functools.lru_cache(maxsize=None)
def data(name):
    tool, M, T, W, K, blocks, seed, cov = CASES[name]
    return tuple(NC.recording(M, samples(name), seed))


def needed(name, out_first, n_out):
    """(first, end) of the input samples a call needs"""
    tool, M, T, W = CASES[name][:4]
    return SO.needed(Lb, W, T, out_first, n_out) if tool == "stap" else NO.needed(Lb, W, out_first, n_out)


def oracle(name, xs, in_first, out_first, n_out, complex64=False, gain=GAIN_INT8):
    tool, M, T, W = CASES[name][:4]
    if tool == "stap":
        return SO.run(list(xs), in_first, out_first, n_out, Lb, W, T, LOAD_SHIFT, None, gain, complex64)
    return NO.run(list(xs), in_first, out_first, n_out, Lb, W, LOAD_SHIFT, None, gain, complex64)


def cut(name, lo, end):
    """input samples lo .. end - 1 of every antenna"""
    return [x[2 * lo:2 * end] for x in data(name)]


@functools.lru_cache(maxsize=None)
def reference(name, complex64=False):
    """the oracle on the whole recording, from output 0: int8 at GAIN_INT8 or complex64 at GAIN_C64.  Where the device's d_cov is left
    out the oracle's window sums are not kept either (case D: 264 MB a result)."""
    res = oracle(name, data(name), 0, 0, outputs(name), complex64, GAIN_C64 if complex64 else GAIN_INT8)
    if not CASES[name][7]:
        res["cov"] = None
    return res


@functools.lru_cache(maxsize=None)
def reference_call(name, out_first, n_out, complex64=False):
    """the oracle on one call, handed the input the call needs"""
    lo, end = needed(name, out_first, n_out)
    res = oracle(name, cut(name, lo, end), lo, out_first, n_out, complex64, GAIN_C64 if complex64 else GAIN_INT8)
    if not CASES[name][7]:
        res["cov"] = None
    return res


def mid_first(name):
    """mid-block, past the warm-up, b0 Lb no multiple of the apply tile: the second chunk starts inside a tile that the first chunk's
    launch also wrote, and own_first = b0 + 1"""
    return (CASES[name][3] + 1) * Lb + 5


@functools.lru_cache(maxsize=None)
def reference_from(name, out_first, complex64=False):
    """the oracle's result of the call from out_first to the end of the recording, as the slice of reference() that it is"""
    whole = reference(name, complex64)
    per = 1 if complex64 else 2
    own = -(-out_first // Lb)
    head = reference_call(name, 0, out_first, complex64)
    res = {"out": whole["out"][per * out_first:], "wq": whole["wq"][own:], "cov": None if whole["cov"] is None else whole["cov"][own:], "owned": whole["owned"] - own,
           "clipped": whole["clipped"] - head["clipped"]}
    assert head["owned"] == own and head["out"].tobytes() == whole["out"][:per * out_first].tobytes() and np.array_equal(head["wq"], whole["wq"][:own])
    return res


def edge(name):
    """the end of the first chunk of a call from output 0: (b0 + K) Lb with b0 = 0"""
    return CASES[name][4] * Lb


def calls(name):
    """label -> (in_first, in_count, out_first, n_out) of every call test_array_chunks_gpu.py makes on the case, each on exactly the input
    it needs"""
    n, o = outputs(name), mid_first(name)
    out = {"whole": (0, n), "mid": (o, n - o)}
    if name in EDGE_CASES:
        out["edge"] = (0, edge(name))
        out["edge + 1"] = (0, edge(name) + 1)
    got = {}
    for label, (first, count) in out.items():
        lo, end = needed(name, first, count)
        got[label] = (lo, end - lo, first, count)
    if name == "A":
        lo, cnt, first, count = got["mid"]
        got["far"] = (lo + FAR_SHIFT, cnt, first + FAR_SHIFT, count)
    return got


def chunks_of(name, out_first, n_out):
    """the triples of launches ar_run_dev cuts a call into: chunk K blocks from the block of its first output"""
    K = CASES[name][4]
    return -(-((out_first + n_out - 1) // Lb + 1 - out_first // Lb) // K)


def margins():
    """name -> margin, after asserting the margin of every case"""
    out = {}
    for name in CASES:
        out[name] = reference(name)["margin"]
        assert out[name] >= MARGIN, (name, out[name])
    return out
