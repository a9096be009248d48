"""The premise of the integer distance order of csrc/gma_nn.hip: float32 sqrt is strictly
increasing on the integers up to 2^22 (and one beyond), so ordering keys by the integer
squared distance and by its float32 square root picks the same key."""
import numpy as np


def test_float32_sqrt_is_strictly_increasing_up_to_2_pow_22():
    n = np.arange(2 ** 22 + 2).astype(np.float32)
    assert np.array_equal(n.astype(np.int64), np.arange(2 ** 22 + 2))      # all exact in float32
    r = np.sqrt(n)
    assert r.dtype == np.float32
    assert (np.diff(r) > 0).all()
