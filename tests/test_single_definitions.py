"""Arithmetic that several tools must share bit for bit has one definition under csrc/, and a copy does not come back: the polynomial
of the replicas' quarter-turn sine / cosine and the TMBOC chip mask (gacq_turn.h), the trace of the diagonal loading in the lane
layout 8 r + c of the array weights kernels (gacq_arraycore.h).  Each is recognised by a piece of text that only a definition holds;
reads sources only, no library and no GPU."""
import os

import pytest

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gnss-dsp-tools_amd", "csrc")


@pytest.mark.parametrize("text, home", [
    ("-4.602163099e-03f", "gacq_turn.h"),             # leading sine coefficient of turn_sincos
    ("(1ull << 29)", "gacq_turn.h"),                  # highest bit of the TMBOC mask
    ("__shfl(Rre, 9 * p, 64)", "gacq_arraycore.h"),   # the trace over lanes 9 p
])
def test_one_file_holds_it(text, home):
    hits = []
    for folder, _, names in os.walk(CSRC):
        for name in sorted(names):
            with open(os.path.join(folder, name), encoding="utf-8", errors="replace") as f:
                if text in f.read():
                    hits.append(name)
    assert hits == [home], (text, hits)
