"""Constructed inputs of the 25-product transposed-conv tests (test_wino_convt_pack_cpu.py, test_wino_convt_gpu.py)."""
import numpy as np


def random_weights(cin: int, seed: int):
    """A [9, cin, 64] transposed kernel at the scale of a BN-folded layer (an output sums at most 4 taps x cin products) and a bias that
    is nowhere zero."""
    rng = np.random.default_rng(seed)
    b = 0.1 * rng.standard_normal(64)
    return rng.standard_normal((9, cin, 64)) / np.sqrt(4 * cin), np.where(np.abs(b) < 0.01, 0.05, b)


def random_case(B: int, H: int, W: int, cin: int, seed: int):
    """x = LeakyReLU_0.3(normal), as the layers' inputs are, float32; weights of random_weights(cin, seed)."""
    rng = np.random.default_rng(seed + 1000)
    x = rng.standard_normal((B, H, W, cin))
    x = np.where(x > 0, x, 0.3 * x).astype(np.float32)
    k9, b = random_weights(cin, seed)
    return x, k9, b
