"""The order in which the cull builds take a launch's blocks (bt_cull.hpp block_order), through
bt_debug_block_order on the host: a stable partition of the block indices -- non-zero masks first, each part ascending --
and the two counts.  tests/test_gpu_block_order.py holds the kernel to the same arrays."""
import numpy as np
import pytest

from block_order_cases import FILLS, LENGTHS, check_order, mask_array


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("n", LENGTHS)
def test_host_order(bendy, n, fill):
    masks = mask_array(n, fill)
    order, header = bendy.Tracer.block_order(masks)
    check_order(masks, order, header)


def test_the_arrays_are_what_they_claim():
    for n in LENGTHS:
        assert (mask_array(n, "zero") == 0).all() and (mask_array(n, "nonzero") != 0).all()
        if n >= 255:
            for d in (0.1, 0.5, 0.9):
                assert abs(float((mask_array(n, f"random-{d}") != 0).mean()) - d) < 0.1


def test_null_and_empty_arguments_are_refused(bendy):
    with pytest.raises(bendy.BendyError):
        bendy.Tracer.block_order(np.zeros(0, np.uint64))
