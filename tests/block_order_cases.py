"""Mask arrays for the block-order tests (test_block_order.py, test_gpu_block_order.py) and what every order of them must
satisfy (test infrastructure)."""
import numpy as np

# 255 .. 257 and 1023 .. 1025: a wave's and a workgroup's worth of masks; 4095 .. 4097 and 8193: the order kernel's chunk
# (BT_ORDER_CHUNK = 4096 masks) and the first mask of its third chunk
LENGTHS = [1, 2, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 4099, 8193]
FILLS = ["zero", "nonzero", "alternating", "alternating-from-1", "random-0.1", "random-0.5", "random-0.9"]


def mask_array(n, fill):
    """`n` masks: zeros, non-zero values (any bit, the top one included), every other one, or seeded random at a density."""
    some = (np.uint64(1) << (np.arange(n, dtype=np.uint64) % np.uint64(64))) | np.uint64(1 << 63 if n % 2 else 0)
    if fill == "zero":
        live = np.zeros(n, bool)
    elif fill == "nonzero":
        live = np.ones(n, bool)
    elif fill.startswith("alternating"):
        live = (np.arange(n) + (1 if fill.endswith("1") else 0)) % 2 == 0
    else:
        density = float(fill.split("-")[1])
        live = np.random.default_rng([n, int(density * 10)]).uniform(size=n) < density
    return np.where(live, some, np.uint64(0)).astype(np.uint64)


def check_order(masks, order, header):
    n = masks.size
    n_live, n_empty = header
    assert n_live + n_empty == n
    assert order.shape == (n,)
    assert np.array_equal(np.sort(order), np.arange(n, dtype=np.uint32)), "not a permutation"
    assert np.array_equal(order[:n_live], np.flatnonzero(masks != 0).astype(np.uint32))
    assert np.array_equal(order[n_live:], np.flatnonzero(masks == 0).astype(np.uint32))
