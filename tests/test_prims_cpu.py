"""Arithmetic behind the device's numpy primitives that needs no device.

The LDS plan of wave_pw_sum (csrc/vmp_np_sum.h) lists the leaves of numpy's
reduction of n elements: one pairwise recursion per buffer of 8192 elements.
The carve (csrc/vmp_carve.h) sizes the leaf arrays for pw_worst(m).leaves + 8,
the most leaves of ONE recursion over any n <= m. The buffered reduction must
never need more."""
import numpy as np


def test_buffered_reduction_fits_the_leaf_arrays_of_the_carve():
    M = 65533  # the largest P a handle takes (V goes to 10240)
    leaves = np.ones(M + 1, np.int64)  # of one recursion over n
    for n in range(129, M + 1):
        n2 = n // 2 - (n // 2) % 8
        leaves[n] = leaves[n2] + leaves[n - n2]
    worst = np.maximum.accumulate(leaves)  # pw_worst(m).leaves
    n = np.arange(M + 1)
    buffered = 64 * (n // 8192) + np.where(n % 8192 > 0, leaves[n % 8192], 0)
    assert leaves[8192] == 64
    assert (np.maximum.accumulate(buffered) <= worst).all()
    # every size the plan is used at: no n needs more than the carve of ITS size holds
    assert (buffered[1929:] <= worst[1929:] + 8).all()
