"""The chunk state machine and the block / window algebra of streaming.py, on CPU tensors with a fake launch: no device, no library call.

The fake filter: output m needs input samples m D - H .. m D + H (those below 0 do not exist and count as absent, as in ddc and
ingest's real mode) and is the sum of the bytes of that support as int64, so every expected value comes straight from the whole
recording.  A sample is 2 bytes; the recording holds 257 samples, which is no multiple of anything the cuts use."""
import numpy as np
import pytest
import torch

from gnss_dsp_tools_amd import streaming

N, UNIT = 257, 2
FILTERS = [(1, 0), (1, 2), (3, 4)]


def recording(seed=1, n=N):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, n * UNIT, dtype=np.uint8))


def support(m, D, H):
    return max(0, m * D - H), m * D + H


def whole_result(recs, D, H, first=0):
    """every output that the whole recordings (input samples first ..) support, from output `first` on"""
    n = recs[0].numel() // UNIT
    sums = sum(r.to(torch.int64).reshape(-1, UNIT).sum(1) for r in recs)
    return torch.stack([sums[lo - first:hi - first + 1].sum() for lo, hi in (support(m, D, H) for m in range(first, first + (n - 1 - H) // D + 1))])


class Fake:
    """the three callables of a fake filter with one (D, H) per output; the launch asserts that it is asked only for what is present"""

    def __init__(self, filters):
        self.filters, self.calls = list(filters), 0

    def supported(self, in_first, in_count):
        ends = [(in_first + in_count - 1 - H) // D + 1 for D, H in self.filters]
        return ends if len(ends) > 1 else ends[0]

    def needed(self, next_out):
        nexts = next_out if isinstance(next_out, list) else [next_out]
        return min(support(m, D, H)[0] for m, (D, H) in zip(nexts, self.filters))

    def launch(self, ds, in_first, in_count, out_first, n_out, k):
        D, H = self.filters[k]
        self.calls += 1
        assert all(d.dtype == torch.uint8 and d.numel() == in_count * UNIT for d in ds)             # whole samples, nothing else
        out = torch.zeros(n_out, dtype=torch.int64)
        for i in range(n_out):
            lo, hi = support(out_first + i, D, H)
            assert in_first <= lo and hi < in_first + in_count, "output %d needs %d .. %d, present are %d .. %d" % (
                out_first + i, lo, hi, in_first, in_first + in_count - 1)
            out[i] = sum(int(d[(lo - in_first) * UNIT:(hi + 1 - in_first) * UNIT].to(torch.int64).sum()) for d in ds)
        return out


def cuts(nbytes):
    """the five ways to cut a recording of nbytes bytes into chunks: lists of chunk lengths"""
    rest = nbytes - 72
    return {"bytes": [1] * nbytes, "threes": [3] * (nbytes // 3) + [nbytes % 3], "7-64-1-rest": [7, 64, 1, rest],
            "with empty chunks": [0, 7, 0, 0, 64, 1, 0, rest, 0], "one chunk": [nbytes]}


def pieces(rec, lengths):
    at = 0
    for n in lengths:
        yield rec[at:at + n]
        at += n
    assert at == rec.numel()


@pytest.mark.parametrize("D,H", FILTERS)
@pytest.mark.parametrize("cut", list(cuts(N * UNIT)))
def test_every_cut_gives_the_whole_buffer_result(D, H, cut):
    rec, fake = recording(), Fake([(D, H)])
    c = streaming.Chunks(8 * UNIT, fake.supported, fake.launch, fake.needed)
    got = []
    for p in pieces(rec, cuts(N * UNIT)[cut]):
        got.append(c.feed_all([p]))
        # the tail: the supports of the outputs still to come reach back 2 H + D samples at most, plus the bytes of a cut sample
        assert c._tails[0].numel() <= (2 * H + D) * UNIT + (UNIT - 1)
        assert c.in_first <= fake.needed(c.next_out)
    want = whole_result([rec], D, H)
    assert torch.equal(torch.cat(got), want)
    assert c.next_out == (N - 1 - H) // D + 1 == want.numel()
    assert fake.calls == len(cuts(N * UNIT)[cut])


def test_two_outputs_on_one_input_keep_the_smaller_need():
    rec, filters = recording(2), [(1, 2), (3, 4)]
    for cut, lengths in cuts(N * UNIT).items():
        fake = Fake(filters)
        c = streaming.Chunks(8 * UNIT, fake.supported, fake.launch, fake.needed, outputs=2)
        got, fed = [[], []], 0
        for p in pieces(rec, lengths):
            before = c.in_first
            for k, out in enumerate(c.feed_all([p])):
                got[k].append(out)
            fed += p.numel()
            needs = [support(m, D, H)[0] for m, (D, H) in zip(c.next_out, filters)]
            assert c.in_first == max(before, min(min(needs), fed // UNIT)), cut
        for k, (D, H) in enumerate(filters):
            assert torch.equal(torch.cat(got[k]), whole_result([rec], D, H)), (cut, k)
        assert c.next_out == [(N - 1 - H) // D + 1 for D, H in filters]


def test_three_inputs_in_lockstep():
    recs = [recording(seed) for seed in (3, 4, 5)]
    for cut, lengths in cuts(N * UNIT).items():
        fake = Fake([(3, 4)])
        c = streaming.Chunks(8 * UNIT, fake.supported, fake.launch, fake.needed)
        got = [c.feed_all(list(ps)) for ps in zip(*[pieces(r, lengths) for r in recs])]
        assert torch.equal(torch.cat(got), whole_result(recs, 3, 4)), cut
        assert len(c._tails) == 3 and len(set(t.numel() for t in c._tails)) == 1


def test_a_start_at_absolute_index_1000():
    rec = recording(6)
    for cut, lengths in cuts(N * UNIT).items():
        fake = Fake([(1, 0)])
        c = streaming.Chunks(8 * UNIT, fake.supported, fake.launch, fake.needed, start=1000)
        assert (c.in_first, c.next_out) == (1000, 1000)
        got = [c.feed_all([p]) for p in pieces(rec, lengths)]
        assert torch.equal(torch.cat(got), whole_result([rec], 1, 0, first=1000)), cut
        assert c.next_out == c.in_first == 1000 + N


def test_bit_granular_samples_keep_a_tail_on_a_byte_boundary():
    """samples of 2 bits, D = 2, H = 21, the tail kept from a multiple of 16 samples, as ingest's real mode does"""
    bits, D, H, n = 2, 2, 21, 1000
    rec = recording(7, n * bits // 8 // UNIT)

    def launch(ds, in_first, in_count, out_first, n_out, k):
        assert in_first % 16 == 0 and ds[0].numel() * 8 == in_count * bits
        for m in range(out_first, out_first + n_out):
            assert in_first <= max(0, m * D - H) and m * D + H < in_first + in_count
        return torch.arange(out_first, out_first + n_out)

    c = streaming.Chunks(bits, lambda in_first, in_count: (in_first + in_count - 1 - H) // D + 1, launch, lambda out: (D * out - H) // 16 * 16)
    got = torch.cat([c.feed_all([p]) for p in pieces(rec, [1] * 50 + [3] * 50 + [50])])
    assert torch.equal(got, torch.arange((n - 1 - H) // D + 1)) and c.in_first % 16 == 0 and c.in_first <= D * c.next_out - H


LB, W = 16, 3


def block_support(j):
    """output j of block b needs j itself and the blocks max(b - W, 0) .. max(b, W) - 1 whole"""
    b = j // LB
    return min(j, max(b - W, 0) * LB), max(j, max(b, W) * LB - 1)


def block_machine():
    def launch(ds, in_first, in_count, out_first, n_out, k):
        for j in range(out_first, out_first + n_out):
            lo, hi = block_support(j)
            assert in_first <= lo and hi < in_first + in_count, (j, lo, hi, in_first, in_count)
        return torch.arange(out_first, out_first + n_out)
    return streaming.Chunks(8 * UNIT, lambda in_first, in_count: streaming.out_end(LB, W, in_first + in_count), launch,
                            lambda out: streaming.first_needed(LB, W, out))


def test_block_window_rule_through_the_machine():
    rec = recording(8, 100)
    for cut in (47, 48, 49):
        c = block_machine()
        first = c.feed_all([rec[:cut * UNIT]])
        # no output before W Lb inputs have arrived, all of them after that
        assert first.numel() == (0 if cut < W * LB else cut) and c.next_out == first.numel()
        assert c.in_first == streaming.first_needed(LB, W, c.next_out) == 0
        rest = c.feed_all([rec[cut * UNIT:]])
        assert torch.equal(torch.cat([first, rest]), torch.arange(100)) and c.next_out == 100
        assert c.in_first == streaming.first_needed(LB, W, 100) == 48 and c._tails[0].numel() == 52 * UNIT
    c = block_machine()                       # sample by sample: the outputs come with the 48th sample and then one by one
    counts = [c.feed_all([rec[i * UNIT:(i + 1) * UNIT]]).numel() for i in range(100)]
    assert counts == [0] * 47 + [48] + [1] * 52


def test_block_window_algebra_agrees_with_its_definitions():
    ends = {}                                 # in_end -> the outputs 0 .. j - 1 whose supports a recording of in_end samples holds
    for in_end in range(141):
        ends[in_end] = next(j for j in range(in_end + 1) if j == in_end or block_support(j)[1] >= in_end)
    for out_first in range(71):
        lo = min(block_support(j)[0] for j in range(out_first, out_first + 71))
        assert streaming.first_needed(LB, W, out_first) == lo == block_support(out_first)[0]
        for n_out in range(71):
            begin = [b for b in range(10) if out_first <= b * LB < out_first + n_out]
            assert streaming.owned_blocks(LB, out_first, n_out) == len(begin)
            in_end = out_first + n_out
            assert streaming.out_end(LB, W, in_end) == ends[in_end]
            for unit in (2, 4):
                assert streaming.out_end(LB, W, in_end, unit) == ends[in_end] // unit * unit
