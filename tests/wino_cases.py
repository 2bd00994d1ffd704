"""Constructed inputs of the Winograd conv2 tests (test_wino_pack_cpu.py, test_wino_conv2_gpu.py)."""
import numpy as np


def random_weights(seed: int):
    """A [9, 128, 128] kernel at the scale of a BN-folded layer (unit-variance outputs for unit-variance inputs) and a bias."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((9, 128, 128)) / np.sqrt(9 * 128), 0.1 * rng.standard_normal(128)


def random_case(B: int, H: int, W: int, seed: int):
    """x = LeakyReLU_0.3(normal), as conv1's output is, float32; weights of random_weights(seed)."""
    rng = np.random.default_rng(seed + 1000)
    x = rng.standard_normal((B, H, W, 128))
    x = np.where(x > 0, x, 0.3 * x).astype(np.float32)
    k9, b = random_weights(seed)
    return x, k9, b


def hot_pixel_positions(H: int, W: int):
    """Every border and corner position of an H x W map, and the pixels on both sides of every 4x32 tile seam near the map's corners
    and centre."""
    pos = {(y, x) for y in range(H) for x in (0, W - 1)} | {(y, x) for y in (0, H - 1) for x in range(W)}
    ys = sorted({y for s in range(4, H, 4) for y in (s - 1, s)})
    xs = sorted({x for s in range(32, W, 32) for x in (s - 1, s)})
    pos |= {(y, x) for y in ys for x in (1, W // 2, W - 2)}
    pos |= {(y, x) for y in (1, H // 2, H - 2) for x in xs}
    pos |= {(y, x) for y in ys for x in xs}
    return sorted(pos)
