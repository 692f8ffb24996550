"""Long-recording windows and their stitch (csrc/longform.hip) restated in numpy, independent of the library: the plan, the
seams, the permutation rule and the blend as include/diffsep_hip.h defines them, written from the definitions (a table of
owners per sample, not the kernel's closed form), plus the inputs the CPU and GPU tests share (tests/test_longform_cpu.py,
tests/test_longform_gpu.py)."""
import itertools
import math

import numpy as np

# (Tw, Tv) swept over every T up to 6 Tw, and the real window shape at chosen lengths
SWEEPS = [(1024, 256), (1024, 341), (96, 32), (30, 10), (3, 1)]
REAL = (32000, 4000)
REAL_T = list(range(31990, 32010)) + list(range(59990, 60010)) + [100001, 480000]


def plan(T, Tw, Tv):
    """-> list of window starts (K = its length), or ValueError for a refused request"""
    if T < 1 or Tv < 1 or 3 * Tv > Tw:
        raise ValueError(f"refused: T={T} Tw={Tw} Tv={Tv}")
    if T <= Tw:
        return [0]
    hop = Tw - Tv
    K = 1 + -((T - Tw) // -hop)
    return [k * hop for k in range(K - 1)] + [T - Tw]


def window_length(T, Tw):
    return min(T, Tw)


def overlaps(starts, Tw):
    """[(begin, length)] of the overlap of windows k and k + 1"""
    return [(starts[k + 1], starts[k] + Tw - starts[k + 1]) for k in range(len(starts) - 1)]


def seams(starts, Tw, Tv):
    """[(begin, n)] of the seam of windows k and k + 1: the n = min(Tv, overlap) samples at the centre of the overlap"""
    out = []
    for b, ov in overlaps(starts, Tw):
        n = min(Tv, ov)
        out.append((b + (ov - n) // 2, n))
    return out


def owners(T, Tw, Tv):
    """(k [T], j [T], n [T]): sample t comes from window k[t] alone (n[t] = 0) or from offset j[t] of the n[t]-sample seam of
    windows k[t] and k[t] + 1.  Built by painting: the stretches between seams first, then the seams."""
    starts = plan(T, Tw, Tv)
    sm = seams(starts, Tw, Tv)
    k = np.zeros(T, np.int64)
    j = np.zeros(T, np.int64)
    n = np.zeros(T, np.int64)
    edge = 0
    for w, (b, m) in enumerate(sm):
        k[edge:b] = w
        k[b:b + m] = w
        j[b:b + m] = np.arange(m)
        n[b:b + m] = m
        edge = b + m
    k[edge:] = len(starts) - 1
    return k, j, n


def permutations(S):
    return list(itertools.permutations(range(S)))  # lexicographic


def cross_gram(a, b):
    """C[i][j] = sum_t a[i][t] b[j][t] in float64 (a, b [S, n] float32)"""
    return a.astype(np.float64) @ b.astype(np.float64).T


def cross_gram_exact(a, b):
    """the same from the exact float64 products with math.fsum (correctly rounded), and sum |a b| per entry"""
    S = a.shape[0]
    c, m = np.zeros((S, S)), np.zeros((S, S))
    for i in range(S):
        for q in range(S):
            pr = a[i].astype(np.float64) * b[q].astype(np.float64)
            c[i, q] = math.fsum(pr)
            m[i, q] = math.fsum(np.abs(pr))
    return c, m


def best_permutation(C):
    """(r, scores): the first permutation, in lexicographic order, of strictly largest sum_i C[i][r(i)]"""
    S = C.shape[0]
    best, bv, scores = None, None, []
    for r in permutations(S):
        v = 0.0
        for i in range(S):
            v += C[i, r[i]]
        scores.append(v)
        if best is None or v > bv:
            best, bv = r, v
    return best, scores


def global_perms(win, T, Tv, want_margins=False):
    """perm [K, S] int32 (g_0 = identity, g_{k+1}[i] = r_k[g_k[i]]), the pairs' cross-Grams and, on request, every pair's margin:
    (best score - runner-up) as a fraction of the sum over the overlap of (sum_i |a_i[t]|) (sum_j |b_j[t]|), the largest value
    any entry sum of the cross-Gram could reach"""
    K, S, Tw = win.shape
    starts = plan(T, Tw, Tv)
    assert len(starts) == K
    g = [tuple(range(S))]
    grams, margins = [], []
    for k, (b, ov) in enumerate(overlaps(starts, Tw)):
        a_ = win[k][:, b - starts[k]:b - starts[k] + ov]
        b_ = win[k + 1][:, :ov]
        C = cross_gram(a_, b_)
        r, scores = best_permutation(C)
        grams.append(C)
        if S > 1:
            top = sorted(scores, reverse=True)
            scale = float(np.sum(np.abs(a_.astype(np.float64)).sum(0) * np.abs(b_.astype(np.float64)).sum(0)))
            margins.append((top[0] - top[1]) / scale if scale > 0 else 0.0)
        g.append(tuple(r[g[-1][i]] for i in range(S)))
    perm = np.asarray(g, dtype=np.int32)
    return (perm, grams, margins) if want_margins else (perm, grams)


def blend(win, T, Tv, perm):
    """out [S, T] float32: the owning window's row perm[k][i], or inside a seam a + (b - a) * r with r = (j + 0.5) / n, every
    operation rounded to float32"""
    K, S, Tw = win.shape
    starts = np.asarray(plan(T, Tw, Tv))
    k, j, n = owners(T, Tw, Tv)
    t = np.arange(T)
    out = np.empty((S, T), np.float32)
    seam = n > 0
    for i in range(S):
        a = win[k, perm[k, i], t - starts[k]]
        out[i] = a
        ks = k[seam]
        b = win[ks + 1, perm[ks + 1, i], t[seam] - starts[ks + 1]]
        r = (j[seam].astype(np.float32) + np.float32(0.5)) / n[seam].astype(np.float32)
        out[i, seam] = a[seam] + (b - a[seam]) * r
    return out


def blend_f64(win, T, Tv):
    """float64 evaluation of the blend of S = 1 windows (no permutation): (ref [T], |a| + |b| [T] (0 outside seams), seam mask)"""
    K, S, Tw = win.shape
    assert S == 1
    starts = np.asarray(plan(T, Tw, Tv))
    k, j, n = owners(T, Tw, Tv)
    t = np.arange(T)
    seam = n > 0
    a = win[k, 0, t - starts[k]].astype(np.float64)
    ref, mag = a.copy(), np.zeros(T)
    ks = k[seam]
    b = win[ks + 1, 0, t[seam] - starts[ks + 1]].astype(np.float64)
    ref[seam] = a[seam] + (b - a[seam]) * (j[seam] + 0.5) / n[seam]
    mag[seam] = np.abs(a[seam]) + np.abs(b)
    return ref, mag, seam


def stitch(win, T, Tv):
    """(out [S, T] float32, perm [K, S] int32, grams)"""
    perm, grams = global_perms(win, T, Tv)
    return blend(win, T, Tv, perm), perm, grams


def cut(x, Tw, Tv, perms=None):
    """x [S, T] -> win [K, S, Tw'] (Tw' = min(T, Tw)): window k holds x[perms[k]] over its stretch (perms None: x itself)"""
    S, T = x.shape
    starts = plan(T, Tw, Tv)
    L = window_length(T, Tw)
    win = np.empty((len(starts), S, L), np.float32)
    for k, s in enumerate(starts):
        rows = list(perms[k]) if perms is not None else list(range(S))
        win[k] = x[rows, s:s + L]
    return win


def reassembly_case(S, T=5000, Tw=1024, Tv=256, seed=0):
    """The exactness case: x [S, T] standard-normal float32; window k's rows are x permuted by the ((5 k + 1) mod S!)-th
    permutation q_k (for S = 3 that walks through non-commuting ones).  -> (x, win, q): a correct stitch returns x[q_0]."""
    x = np.random.default_rng(1000 * S + seed).standard_normal((S, T)).astype(np.float32)
    P = permutations(S)
    K = len(plan(T, Tw, Tv))
    q = [P[(5 * k + 1) % len(P)] for k in range(K)]
    return x, cut(x, Tw, Tv, q), q
