"""tests/reduce_ref.py is a statement about ORDER: on the very inputs tests/test_reduce_order_gpu.py compares bit for bit, the
emulated totals differ from the same sums formed in three other orders, so the equality on the device has content."""
import numpy as np

import reduce_ref as RR

MIN_DIFFER = 4  # entries that must differ per alternative; a seed that gives fewer is replaced, never this number


def differing(a, b):
    return int(np.count_nonzero(a.view(np.uint64) != b.view(np.uint64)))


def test_block_total_is_the_stated_order():
    # one wave, hand-made: the butterfly pairs lane l with l ^ 32 first, a sequential sum would lose the small terms
    v = np.zeros(64)
    v[0], v[32], v[1], v[33] = 1.0, -1.0, 2.0 ** -60, 2.0 ** -60
    assert RR.block_total(v, 64) == 2.0 ** -59 and RR.sequential_total(v) == 2.0 ** -60
    # thread t takes t, t + n, ...; the wave totals first to last
    w = np.zeros(256)
    w[0], w[64], w[128], w[192] = 1.0, 2.0 ** -53, 2.0 ** -53, -1.0
    assert RR.block_total(w, 256) == 0.0 and RR.block_total(w, 256, RR.fold_last_to_first) == 2.0 ** -52
    assert RR.block_total(w, 256, RR.fold_pairwise) == 2.0 ** -53
    x = np.arange(1, 301, dtype=np.float64)
    assert RR.block_total(x, 256) == x.sum() and RR.block_total(x[:0], 256) == 0.0


def test_other_orders_give_other_bits():
    ref, est = RR.gram_case()
    win = RR.longform_case()
    g = RR.gram_expected(ref, est)
    lf = RR.longform_expected(win)
    assert g.shape == (3, 3, 2, 2) and lf.shape == (6, 3, 3)
    exact = np.einsum("bit,bjt->bij", ref.astype(np.float64), est.astype(np.float64))
    assert np.allclose(g[:, 1], exact, rtol=1e-12, atol=1e-9)  # (the emulation sums the right things)
    others = {
        "sequential": dict(total=RR.sequential_total),
        "waves last to first": dict(fold=RR.fold_last_to_first),
        "waves pairwise": dict(fold=RR.fold_pairwise),
    }
    for name, kw in others.items():
        dg = differing(g, RR.gram_expected(ref, est, **kw))
        dl = differing(lf, RR.longform_expected(win, **kw))
        print(f"{name}: gram {dg} of {g.size} entries differ, longform cross-Gram {dl} of {lf.size}")
        assert dg + dl >= MIN_DIFFER, (name, dg, dl)
        # the Gram case alone carries each alternative: its blocks fill all 16 waves.  The shares of the long-recording case
        # are 16 and 56 samples, inside one wave: there only the order within the wave (the butterfly) can show.
        assert dg >= MIN_DIFFER, (name, dg)
    assert differing(lf, RR.longform_expected(win, total=RR.sequential_total)) >= MIN_DIFFER
