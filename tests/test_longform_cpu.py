"""Long-recording windows (csrc/longform.hip) — what can be checked without a GPU: the window plan through the C-ABI against
the numpy restatement (tests/longform_ref.py), the plan's properties, the kernel's sample-to-window arithmetic
(diffsep_longform_locate: the host copy of what the blend kernel computes per sample), the refusals, and the restatement's
own exact reassembly — the precondition of the GPU exactness test."""
import ctypes as C

import numpy as np
import pytest

import longform_ref as R
from diffsep_amd import _lib, ops


def c_plan(T, Tw, Tv, cap=None):
    l = _lib.lib()
    K = l.diffsep_longform_plan(T, Tw, Tv, None, 0)
    if K < 0:
        return K, None
    cap = K if cap is None else cap
    buf = (C.c_int64 * max(cap, 1))()
    K2 = l.diffsep_longform_plan(T, Tw, Tv, buf, cap)
    return K2, list(buf[:K]) if K2 >= 0 else None


def check_properties(T, Tw, Tv, starts):
    K = len(starts)
    if T <= Tw:
        assert starts == [0]
        return
    assert all(b > a for a, b in zip(starts, starts[1:]))
    assert starts[0] == 0 and starts[-1] + Tw == T
    ov = R.overlaps(starts, Tw)
    sm = R.seams(starts, Tw, Tv)
    assert all(n >= Tv for _, n in ov)
    assert all(n == Tv for _, n in ov[:-1])  # longer only for the last pair
    for (ob, on), (sb, sn) in zip(ov, sm):
        assert sn == Tv and ob <= sb and sb + sn <= ob + on  # seam inside its overlap
    assert all(sm[i][0] + sm[i][1] <= sm[i + 1][0] for i in range(K - 2))  # pairwise disjoint, in order
    # every sample: in exactly one seam, or outside all seams inside the window that owns the stretch between two seams
    cover = np.zeros(T, np.int64)
    edge = 0
    for w, (sb, sn) in enumerate(sm):
        assert starts[w] <= edge and sb <= starts[w] + Tw  # the stretch [edge, sb) lies inside window w
        cover[edge:sb] += 1
        cover[sb:sb + sn] += 1
        edge = sb + sn
    assert starts[-1] <= edge
    cover[edge:] += 1
    assert np.all(cover == 1)


@pytest.mark.parametrize("Tw,Tv", R.SWEEPS)
def test_plan_equals_restatement_and_has_its_properties(Tw, Tv):
    for T in range(1, 6 * Tw + 1):
        K, starts = c_plan(T, Tw, Tv)
        assert starts == R.plan(T, Tw, Tv) and K == len(starts), (T, Tw, Tv)
        check_properties(T, Tw, Tv, starts)


def test_plan_real_window_shape():
    Tw, Tv = R.REAL
    for T in R.REAL_T:
        K, starts = c_plan(T, Tw, Tv)
        assert starts == R.plan(T, Tw, Tv) and K == len(starts), T
        check_properties(T, Tw, Tv, starts)
    assert len(R.plan(480000, Tw, Tv)) == 17  # a 60 s file at 8 kHz: two engine calls of 16 windows
    assert ops.longform_plan(100001, Tw, Tv) == R.plan(100001, Tw, Tv)


@pytest.mark.parametrize("Tw,Tv", [(96, 32), (30, 10), (3, 1), (1024, 341)])
def test_kernel_sample_arithmetic_equals_restatement(Tw, Tv):
    """diffsep_longform_locate is the function the blend kernel calls per sample, compiled for the host"""
    l = _lib.lib()
    k, j, n = C.c_int32(), C.c_int64(), C.c_int64()
    Ts = range(1, 6 * Tw + 1) if Tw <= 96 else (1, Tw, Tw + 1, 2 * Tw - Tv, 2 * Tw - Tv + 1, 3 * Tw, 5000, 6 * Tw)
    for T in Ts:
        rk, rj, rn = R.owners(T, Tw, Tv)
        for t in range(T):
            assert l.diffsep_longform_locate(T, Tw, Tv, t, C.byref(k), C.byref(j), C.byref(n)) == 0
            assert (k.value, j.value, n.value) == (rk[t], rj[t], rn[t]), (T, t)
    assert l.diffsep_longform_locate(10, Tw, Tv, 10, C.byref(k), C.byref(j), C.byref(n)) != 0
    assert b"outside" in l.diffsep_last_error()


def test_kernel_sample_arithmetic_real_window_shape():
    l = _lib.lib()
    Tw, Tv = R.REAL
    k, j, n = C.c_int32(), C.c_int64(), C.c_int64()
    for T in (32001, 59999, 60000, 60001, 100001, 480000):
        rk, rj, rn = R.owners(T, Tw, Tv)
        edges = np.flatnonzero((np.diff(rk) != 0) | (np.diff(rn) != 0))
        ts = sorted({0, T - 1, *[int(e + d) for e in edges for d in (0, 1)], *range(0, T, 997)})
        for t in ts:
            assert l.diffsep_longform_locate(T, Tw, Tv, t, C.byref(k), C.byref(j), C.byref(n)) == 0
            assert (k.value, j.value, n.value) == (rk[t], rj[t], rn[t]), (T, t)


def test_plan_edge_cases():
    Tw, Tv = 1024, 256
    assert c_plan(1, Tw, Tv) == (1, [0])
    assert c_plan(Tw, Tw, Tv) == (1, [0])
    K, starts = c_plan(Tw + 1, Tw, Tv)
    assert (K, starts) == (2, [0, 1]) and R.overlaps(starts, Tw) == [(1, Tw - 1)]
    assert R.seams(starts, Tw, Tv) == [(1 + (Tw - 1 - Tv) // 2, Tv)]
    K, starts = c_plan(2 * Tw - Tv, Tw, Tv)
    assert (K, starts) == (2, [0, Tw - Tv]) and R.overlaps(starts, Tw) == [(Tw - Tv, Tv)]
    assert c_plan(2 * Tw - Tv + 1, Tw, Tv)[0] == 3


def test_refusals_name_their_cause():
    l = _lib.lib()
    for (T, Tw, Tv), word in (((5000, 1024, 0), b"Tv"), ((5000, 1024, 342), b"3 Tv > Tw"), ((0, 1024, 256), b"T = 0"),
                              ((-3, 1024, 256), b"T = -3")):
        assert l.diffsep_longform_plan(T, Tw, Tv, None, 0) == -1
        assert word in l.diffsep_last_error(), l.diffsep_last_error()
        with pytest.raises(ValueError):
            R.plan(T, Tw, Tv)
        with pytest.raises(_lib.DiffsepError):
            ops.longform_plan(T, Tw, Tv)
    buf = (C.c_int64 * 8)(*([-7] * 8))
    assert l.diffsep_longform_plan(5000, 1024, 256, None, 0) == 7
    assert l.diffsep_longform_plan(5000, 1024, 256, buf, 6) == -1
    assert b"cap" in l.diffsep_last_error() and list(buf) == [-7] * 8
    assert l.diffsep_longform_plan(5000, 1024, 256, buf, 7) == 7 and list(buf)[:7] == R.plan(5000, 1024, 256)
    # the stitch validates before its first device call: these return non-zero with a message without a GPU
    p = C.c_void_p(4096)
    assert l.diffsep_longform_workspace_bytes(7, 4) == -1 and l.diffsep_longform_workspace_bytes(0, 2) == -1
    need = l.diffsep_longform_workspace_bytes(7, 2)
    assert need > 0
    assert l.diffsep_longform_stitch(p, 7, 4, 1024, 5000, 256, p, p, None, p, 1 << 20, None) != 0
    assert b"sources" in l.diffsep_last_error()
    assert l.diffsep_longform_stitch(p, 6, 2, 1024, 5000, 256, p, p, None, p, 1 << 20, None) != 0
    assert b"windows" in l.diffsep_last_error()
    assert l.diffsep_longform_stitch(p, 7, 2, 1024, 5000, 342, p, p, None, p, 1 << 20, None) != 0
    assert b"3 Tv > Tw" in l.diffsep_last_error()
    assert l.diffsep_longform_stitch(p, 7, 2, 1024, 5000, 256, p, p, None, p, need - 1, None) != 0
    assert b"workspace too small" in l.diffsep_last_error()
    assert l.diffsep_longform_stitch(None, 7, 2, 1024, 5000, 256, p, p, None, p, need, None) != 0
    assert b"null" in l.diffsep_last_error()


@pytest.mark.parametrize("S", [1, 2, 3])
def test_restatement_reassembles_its_own_windows(S):
    T, Tw, Tv = 5000, 1024, 256
    x, win, q = R.reassembly_case(S, T, Tw, Tv)
    assert win.shape == (7, S, Tw)
    if S == 3:  # the walk really contains two permutations that do not commute
        P = [np.asarray(p) for p in q]
        assert any(not np.array_equal(a[b], b[a]) for a in P for b in P)
    perm, grams, margins = R.global_perms(win, T, Tv, want_margins=True)
    out = R.blend(win, T, Tv, perm)
    assert out.dtype == np.float32 and np.array_equal(out.view(np.uint32), x[list(q[0])].view(np.uint32))
    # perm[k][i] is the row of window k that holds x[q_0[i]]
    for k in range(7):
        assert [q[k][r] for r in perm[k]] == list(q[0])
    if S > 1:
        print(f"S={S}: smallest margin of the winning permutation {min(margins):.3f}")
        assert min(margins) >= 0.05
    c, _ = R.cross_gram_exact(win[0][:, Tw - Tv:], win[1][:, :Tv])
    assert np.allclose(grams[0], c, rtol=0, atol=1e-9)


def test_restatement_tie_is_the_identity():
    C0 = np.zeros((3, 3))
    assert R.best_permutation(C0)[0] == (0, 1, 2)
    assert R.best_permutation(np.ones((2, 2)))[0] == (0, 1)
    assert R.best_permutation(np.array([[0.0, 1.0], [1.0, 0.0]]))[0] == (1, 0)
