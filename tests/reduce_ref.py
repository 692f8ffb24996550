"""The fixed-order float64 block reduction of csrc/reduce_device.h restated in numpy, and the two cases that hold the library
to it bit for bit (tests/test_reduce_order_gpu.py; tests/test_reduce_ref_cpu.py shows that other orders give other bits).

The contract: thread t of an n-thread block adds its addends t, t + n, ... in order (from +0.0); the 64 lanes of a wave run the
butterfly v = v + v[lane ^ o], o = 32 .. 1; the n / 64 wave totals are folded first to last.  The addends of both cases are
products of two float32 values, exact in float64: only the additions round."""
import numpy as np

import longform_ref as R

LF_BLOCKS = 16  # kLfBlocks of csrc/longform.hip: contiguous shares (= block partials) per overlap


def fold_first_to_last(w):
    r = w[..., 0]
    for i in range(1, w.shape[-1]):
        r = r + w[..., i]
    return r


def fold_last_to_first(w):
    return fold_first_to_last(w[..., ::-1])


def fold_pairwise(w):
    while w.shape[-1] > 1:
        w = w[..., 0::2] + w[..., 1::2]
    return w[..., 0]


def block_total(addends, n, fold=fold_first_to_last):
    """addends float64 [..., L] -> [...]: what an n-thread block makes of them (fold: how the wave totals are combined)"""
    a = np.asarray(addends, np.float64)
    L = a.shape[-1]
    rows = max(1, -(-L // n))
    a = np.concatenate([a, np.zeros(a.shape[:-1] + (rows * n - L,))], axis=-1).reshape(a.shape[:-1] + (rows, n))
    v = np.zeros(a.shape[:-2] + (n,))
    for r in range(rows):  # a thread past the end adds +0.0: the same bits as not adding
        v = v + a[..., r, :]
    v = v.reshape(v.shape[:-1] + (n // 64, 64))
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ o]
    return fold(v[..., 0])


def sequential_total(addends, n=None, fold=None):
    a = np.asarray(addends, np.float64)
    r = np.zeros(a.shape[:-1])
    for i in range(a.shape[-1]):
        r = r + a[..., i]
    return r


# ---------------------------------------------------------------------------------------------------------------- the cases
def gram_case():
    """ref, est [3, 2, 3000] float32 for ops.gram: 1024 threads (16 waves) hold 2 or 3 addends each"""
    g = np.random.default_rng(20240611)
    return g.standard_normal((3, 2, 3000)).astype(np.float32), g.standard_normal((3, 2, 3000)).astype(np.float32)


def gram_expected(ref, est, total=block_total, fold=fold_first_to_last):
    """[B, 3, S, S] = (ref ref^T, ref est^T, est est^T) as gram_kernel sums them"""
    r, e = ref.astype(np.float64), est.astype(np.float64)
    prod = np.stack([r[:, :, None, :] * r[:, None, :, :], r[:, :, None, :] * e[:, None, :, :], e[:, :, None, :] * e[:, None, :, :]], axis=1)
    return total(prod, 1024, fold)


LF_CASE = dict(S=3, Tw=1024, Tv=256, T=5000)


def longform_case():
    """win [7, 3, 1024] float32: the cross-Gram case of tests/test_longform_gpu.py"""
    return R.reassembly_case(LF_CASE["S"], LF_CASE["T"], LF_CASE["Tw"], LF_CASE["Tv"], seed=1)[1]


def longform_expected(win, total=block_total, fold=fold_first_to_last):
    """[K - 1, S, S]: every overlap in 16 contiguous shares of ceil(ov / 16) samples (lf_gram_kernel, 256 threads a block), the
    16 block partials then added in block order from +0.0 (lf_perm_kernel)"""
    starts = R.plan(LF_CASE["T"], LF_CASE["Tw"], LF_CASE["Tv"])
    out = []
    for k, (b, ov) in enumerate(R.overlaps(starts, LF_CASE["Tw"])):
        a = win[k][:, b - starts[k]:b - starts[k] + ov].astype(np.float64)
        c = win[k + 1][:, :ov].astype(np.float64)
        prod = a[:, None, :] * c[None, :, :]
        share = -(-ov // LF_BLOCKS)
        s = np.zeros(prod.shape[:2])
        for blk in range(LF_BLOCKS):
            s = s + total(prod[..., blk * share:min(ov, (blk + 1) * share)], 256, fold)
        out.append(s)
    return np.stack(out)
