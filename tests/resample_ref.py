"""The definition every layer of the sample-rate converter computes, in float64 numpy, with the quantities its error bound needs:

    y[m] = sum_j h[m q + L - p j] x[j],  0 <= j < len, tap index in [0, 2 L],  0 <= m < n_out = ceil(len p / q)

(the zero-stuffed direct form, centred: scipy.signal.resample_poly(x, p, q, window=h / p)), plus the ratios, lengths and random
inputs the CPU and GPU tests share."""
import numpy as np

# (p, q) the issue lists for the definition and the design check, and the lengths they are checked at
RATIOS = [(1, 2), (2, 1), (1, 3), (6, 1), (80, 441), (441, 80), (160, 441), (320, 441)]
LENGTHS = [1, 37, 1000]
# element-bound test on the device: ratios, one batch of B = 3 mixed lengths (T = the longest), S = 2
BOUND_RATIOS = [(1, 2), (2, 1), (1, 3), (6, 1), (80, 441), (441, 80), (320, 441)]
BOUND_LENGTHS = [[1, 37, 1000], [9000, 1000, 37]]


def n_out(n, p, q):
    return -((-n * p) // q)


def terms(n, p, q, L):
    """(sample index j [n_out, K], tap index [n_out, K], valid [n_out, K]) of every product of every output"""
    m = np.arange(n_out(n, p, q), dtype=np.int64)
    K = (2 * L + p) // p
    c = m * q + L
    j = (c // p)[:, None] - np.arange(K, dtype=np.int64)[None, :]
    tap = c[:, None] - p * j
    ok = (j >= 0) & (j < n) & (tap >= 0) & (tap <= 2 * L)
    return j, tap, ok


def direct(x, p, q, h, full=False):
    """float64 y [n_out] of the definition; full=True: (y, sum_j |h x| per output, number of products per output).  A zero
    result is +0.0 (the device starts its sums from +0.0)."""
    x = np.asarray(x, dtype=np.float64)
    h = np.asarray(h, dtype=np.float64)
    assert x.ndim == 1 and h.ndim == 1 and h.size % 2 == 1
    L = (h.size - 1) // 2
    j, tap, ok = terms(x.size, p, q, L)
    prod = np.where(ok, h[np.clip(tap, 0, 2 * L)] * x[np.clip(j, 0, max(x.size - 1, 0))], 0.0)
    y = prod.sum(axis=1) + 0.0
    if not full:
        return y
    return y, np.abs(prod).sum(axis=1), ok.sum(axis=1)


def bound64(sabs, count):
    """|y - direct| allowed for float64 output: the summation-error bound of K products in any order, applied to both sides"""
    return 2.0 * (count + 2) * 2.0 ** -53 * sabs


def bound32(sabs, count, y):
    """... for float32 output: plus the one rounding to float32 (half an ulp, and the smallest subnormal)"""
    return bound64(sabs, count) + 2.0 ** -24 * np.abs(y) + 2.0 ** -149


def random_rows(seed, shape):
    """float32 samples of a few magnitudes (unit-variance noise times 1, 1e-3 or 30 per row)"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape)
    scale = np.array([1.0, 1e-3, 30.0])[rng.integers(0, 3, shape[:-1])]
    return (x * scale[..., None]).astype(np.float32)
