"""CPU test of the crafted block of test_gpu_backhalf.py: from the float64
oracle alone, the block must keep every decision of the back half far enough
from its threshold that float32 rounding on the GPU cannot flip it.  These
are conditions on the input, not measurements: if one drifts, change the
block in backhalf_block.py, not the limits here."""

import numpy as np
import pytest

import backhalf_block as bb


@pytest.mark.parametrize("S", [16, 8])
def test_block_margins(S):
    o = bb.oracle(bb.make_block(S), S)
    sk, lo, hi = o["sk"], o["sk_lo"], o["sk_hi"]
    print("S", S, "SK", np.round(sk, 3), "lo'", lo, "hi'", hi)
    assert set(np.nonzero(o["flags"])[0]) == {bb.CHIRP_ROW, bb.tone_row(S)}
    assert sk[bb.CHIRP_ROW] < lo and sk[bb.tone_row(S)] > hi
    assert np.abs(sk - lo).min() >= 0.04 and np.abs(sk - hi).min() >= 0.04
    r = o["rfi_ratio"]
    near = np.abs(r / bb.RFI_THRESHOLD - 1.0) <= 0.05
    print("bins above the RFI threshold", int((r > bb.RFI_THRESHOLD).sum()),
          "within 5 % of it", int(near.sum()))
    assert r[bb.CW_BIN] > bb.RFI_THRESHOLD
    assert near.sum() <= 4
    print("counts", o["counts"])
    assert sorted(o["counts"]) == [1, 2, 4, 8, 16]
    assert all(c > 0 for c in o["counts"].values())


def test_windowed_block_margins():
    """Hamming window, noise only: sk_threshold = 4 sits in the largest gap of
    the rows' de-applied SK, which flags some rows and not all."""
    S = 16
    o = bb.oracle(bb.make_noise_block(), S, window="hamming",
                  sk_threshold=bb.WINDOWED_SK_THRESHOLD)
    sk = np.sort(o["sk"])
    print("SK", np.round(sk, 3), "hi'", o["sk_hi"])
    gaps = np.diff(sk)
    g = int(np.argmax(gaps))
    assert sk[g] < o["sk_hi"] < sk[g + 1]
    assert min(o["sk_hi"] - sk[g], sk[g + 1] - o["sk_hi"]) >= 0.04
    assert (sk > o["sk_lo"] + 0.04).all()
    assert 0 < o["flags"].sum() < S
