"""NumPy restatement of diffsep_ensemble (csrc/ensemble.hip; the arithmetic is stated in include/diffsep_hip.h): K posterior draws
of every utterance of a zero-padded batch aligned to an anchor by the permutation rule of perm_search.h, then the mean, the
population spread, every draw's squared distance to the mean and the medoid, all in float64.  Sums here are numpy's (pairwise,
another order than the device's blocks): equal to the device bit for bit only where every sum is exact, within the summation
bounds otherwise.  The mean's add chain IS in the device's order (k ascending, one division), so it is bit-equal always."""
import itertools

import numpy as np


def perms(S):
    """the permutations of 0 .. S - 1 in lexicographic order (itertools' order for a sorted input)"""
    return list(itertools.permutations(range(S)))


def best_perm(c):
    """the permutation r of largest sum_i c[i][r(i)]: candidates in lexicographic order, strict >, so a tie keeps the earliest"""
    S = c.shape[0]
    best, bestv = None, 0.0
    for p in perms(S):
        v = 0.0
        for i in range(S):
            v += c[i, p[i]]
        if best is None or v > bestv:
            best, bestv = p, v
    return best


def best_perm_brute(c):
    """the same by brute force: the largest total, and among equal totals the lexicographically smallest permutation"""
    S = c.shape[0]
    tot = {p: sum(c[i, p[i]] for i in range(S)) for p in perms(S)}
    top = max(tot.values())
    return min(p for p, v in tot.items() if v == top)


def cross_gram(a, d):
    """a [S,n], d [S,n] float32 -> (C [S,S] float64 = a d^T as exactly as float64 sums get, M [S,S] = sum |products|)"""
    a64, d64 = a.astype(np.float64), d.astype(np.float64)
    prod = a64[:, None, :] * d64[None, :, :]  # exact: 24-bit x 24-bit significands
    return np.sum(prod, axis=-1), np.sum(np.abs(prod), axis=-1)


def cross_gram_int(a, d):
    """integer-valued rows: the Gram in int64, exact"""
    return a.astype(np.int64) @ d.astype(np.int64).T


def ensemble_one(draws, anchor=None):
    """draws [K,S,n] float32 (one utterance, its n samples only), anchor [S,n] or None (draw 0) -> dict of
    gram [K,S,S], gram_mag [K,S,S], perm [K,S] int32, mean64 / mean [S,n], std64 / std [S,n], dist [K], dist_terms [K] (number
    of terms), medoid, pick [S,n], aligned [K,S,n]"""
    K, S, n = draws.shape
    a = draws[0] if anchor is None else anchor
    gram, mag, perm = np.zeros((K, S, S)), np.zeros((K, S, S)), np.zeros((K, S), np.int32)
    for k in range(K):
        gram[k], mag[k] = cross_gram(a, draws[k])
        perm[k] = range(S) if (anchor is None and k == 0) else best_perm(gram[k])
    v = np.stack([draws[k][perm[k]] for k in range(K)])  # [K,S,n]
    m = v[0].astype(np.float64)
    for k in range(1, K):
        m = m + v[k].astype(np.float64)
    m = m / float(K)
    dev2 = (v.astype(np.float64) - m[None]) ** 2
    ss = dev2[0].copy()
    for k in range(1, K):
        ss = ss + dev2[k]
    std64 = np.sqrt(ss / float(K))
    dist = np.array([np.sum(dev2[k]) for k in range(K)])
    medoid = 0
    for k in range(1, K):
        if dist[k] < dist[medoid]:
            medoid = k
    return dict(gram=gram, gram_mag=mag, perm=perm, mean64=m, mean=m.astype(np.float32), std64=std64, var64=ss / float(K),
                std=std64.astype(np.float32), dist=dist, medoid=medoid, pick=v[medoid].copy(), aligned=v)


def ensemble(draws, lengths=None, anchor=None):
    """draws [B,K,S,T] -> per utterance ensemble_one over its first lengths[b] samples (nothing beyond them is looked at)"""
    B, K, S, T = draws.shape
    lengths = [T] * B if lengths is None else lengths
    return [ensemble_one(draws[b][:, :, :lengths[b]], None if anchor is None else anchor[b][:, :lengths[b]]) for b in range(B)]


def ulp32(x):
    """the spacing of float32 at |x| (float64 in, float64 out)"""
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)
