"""Float64 references for the warm start (csrc/warm_start.hip, ops.warm_start) in the notation of tests/sdecheck.py:
U = 2^-24, bound = U (k A + sum_c rho_c A_c), k counted in the kernel source, function accuracies from sdecheck's table.  Nothing
below is fitted to device output.

PERTURB.  The kernel (warm_apply_kernel; `#pragma clang fp contract(off)`: every operation rounds on its own), per sample:
    x0_i = (gf_i * e_i - mu) / sd             3 roundings; gf_i = (float) g_i is one more, relative, on g_i e_i (rho_g = 1)
    m    = mixn / S                            1           (mean_from mix)
         = (x0_0 + .. + x0_{S-1}) / S          S           (mean_from estimate), on top of the 3 of x0
    mean = m + d * (x0_i - m)                  3: the difference, the product, the sum;   d = expf(-t lam): rho_d = 4 + t lam
    lz   = ca * mz + cp * (z_i - mz)           mz: S;  z_i - mz, cp * (..), ca * mz, the sum: longest path S + 3
           ca = a * sm, cp = p * sm            rho_a, rho_p of sdecheck.mix_coef, + 1 for the product with sigma_mix
    x    = mean + lz                           1
Longest path: mean_from mix: max(3 + 3, S + 3) + 1 = max(7, S + 4); mean_from estimate: 3 + S + 3 + 1 = S + 7.
A: the expression on absolute values, |v - w| -> |v| + |w|.

GAIN FIT.  fit(est, mix, n): Gram matrix and right-hand side as exactly rounded sums (math.fsum), then the kernel's Cholesky with its
pivot rule (pivot <= 2^-40 trace / S -> gains 1, fallback) in float64.  fit_device_order restates the kernel's summation order
(32 shares of warm_share(n) samples, 256 threads taking groups of 4 samples, reduce_ref.block_total) for a bit-level look.
gain_bound: with E the [n, S] matrix of the estimates, G = E^T E, r = E^T y and y = E g up to a small residual:
    every entry of G and r is a float64 sum of n exact products: |dG_ij| <= n 2^-53 sqrt(G_ii G_jj), so ||dG||_2 <= n 2^-53 trace(G)
    <= n 2^-53 S ||G||_2, and ||dr||_2 <= n 2^-53 sqrt(trace G) ||y|| <= n 2^-53 sqrt(S) ||G||_2 ||g||_2.
    (G + dG)(g + dg) = r + dr  =>  ||dg|| / ||g|| <= cond(G) (||dG|| / ||G|| + ||dr|| / (||G|| ||g||)) <= cond(G) n 2^-53 (S + sqrt S)
    to first order; the S x S Cholesky solve adds at most 8 S^2 2^-53 cond(G) (Higham, Accuracy and Stability, Thm 10.4 with
    gamma_{3S+1} <= 8 S 2^-53 and the factor S of the norm change).  The float64 reference (numpy.linalg.lstsq on E, cond(E) =
    sqrt(cond G)) is itself no closer than the same order, so the bound is doubled:
    |dg|_inf <= 2 ||g||_2 cond(G) 2^-53 (n (S + sqrt S) + 8 S^2).
"""
import math

import numpy as np

import reduce_ref
import sdecheck as K

PARTS = 32  # kWarmParts


def share(n):
    """warm_share(n) of csrc/warm_start.hip"""
    return ((n + PARTS - 1) // PARTS + 3) // 4 * 4


def cholesky_gains(G, r):
    """(gains [S], fallback) of the kernel's warm_solve on float64 sums G [S,S], r [S]"""
    S = len(r)
    tr = 0.0
    for i in range(S):
        tr += G[i, i]
    thr = 2.0 ** -40 * tr / S
    L = np.zeros((S, S))
    for j in range(S):
        d = G[j, j]
        for k in range(j):
            d -= L[j, k] * L[j, k]
        if not d > thr:
            return np.ones(S), 1
        L[j, j] = math.sqrt(d)
        for i in range(j + 1, S):
            s = G[i, j]
            for k in range(j):
                s -= L[i, k] * L[j, k]
            L[i, j] = s / L[j, j]
    y, g = np.zeros(S), np.zeros(S)
    for i in range(S):
        s = r[i]
        for k in range(i):
            s -= L[i, k] * y[k]
        y[i] = s / L[i, i]
    for i in range(S - 1, -1, -1):
        s = y[i]
        for k in range(i + 1, S):
            s -= L[k, i] * g[k]
        g[i] = s / L[i, i]
    return g, 0


def sums_exact(est, mix, n):
    """(G [S,S], r [S]) over the first n samples, every entry an exactly rounded sum"""
    e, y = K.f64(est)[:, :n], K.f64(mix).reshape(-1)[:n]
    S = e.shape[0]
    G = np.array([[math.fsum(e[i] * e[j]) for j in range(S)] for i in range(S)])
    return G, np.array([math.fsum(e[i] * y) for i in range(S)])


def sums_device_order(est, mix, n):
    """the same sums in the kernel's order: share p = samples [p sh, min(n, (p + 1) sh)), thread q of 256 adds the samples of its
    groups 4 q + 1024 r + (0 .. 3) in order, block totals by reduce_ref.block_total, the 32 partials folded in share order"""
    e, y = K.f64(est)[:, :n], K.f64(mix).reshape(-1)[:n]
    S = e.shape[0]
    prod = np.concatenate([(e[:, None, :] * e[None, :, :]).reshape(S * S, n), e * y[None]], 0)  # [S S + S, n]
    sh = share(n)
    tot = None
    for p in range(PARTS):
        seg = prod[:, p * sh:min(n, (p + 1) * sh)]
        rows = max(1, -(-seg.shape[1] // 1024))
        pad = np.zeros((seg.shape[0], rows * 1024))
        pad[:, :seg.shape[1]] = seg
        # element (r, q, k) -> addend index (4 r + k) * 256 + q of thread q
        a = pad.reshape(-1, rows, 256, 4).transpose(0, 1, 3, 2).reshape(seg.shape[0], rows * 4 * 256)
        part = reduce_ref.block_total(a, 256)
        tot = part if tot is None else tot + part
    return tot[:S * S].reshape(S, S), tot[S * S:]


def fit(est, mix, n=None, sums=sums_exact):
    """est [S,T], mix [T] or [1,T] float32, the first n samples -> (gains float64 [S], fallback 0 | 1, cond(G) or inf)"""
    n = est.shape[-1] if n is None else int(n)
    G, r = sums(est, mix, n)
    g, fb = cholesky_gains(G, r)
    with np.errstate(all="ignore"):
        cond = float(np.linalg.cond(G)) if np.isfinite(G).all() and G.any() else float("inf")
    return g, fb, cond


def gain_bound(g, cond, n):
    S = len(g)
    return 2.0 * float(np.linalg.norm(g)) * cond * 2.0 ** -53 * (n * (S + math.sqrt(S)) + 8.0 * S * S)


def perturb(sde, est, mixn, mean, std, t, z, gains=None, smix=None, mean_from="mix", lengths=None):
    """(x_init, bound) float64 [B,S,T] of ops.warm_start's second pass.  est, z [B,S,T], mixn [B,1,T], smix [B,T] | None: stored
    float32; mean, std, t [B] float32; gains [B,S] float64 (None: exactly 1, and then gf * e is exact)."""
    e, zz = K.f64(est), K.f64(z)
    B, S, T = e.shape
    mu, sd, tt = (K._b(K._tt(v)) for v in (mean, std, t))
    _, _, lam, _, _ = K._sde_scalars(sde)
    c = K.mix_coef(sde, t)
    sm, one = K._sm(smix, B, T)
    a, p = K._b(c.a) * sm, K._b(c.p) * sm
    ra, rp = K._b(c.ra) + one, K._b(c.rp) + one
    d, rd = np.exp(-tt * lam), K.fu("expf") + tt * lam
    g = np.ones((B, S, 1)) if gains is None else np.asarray(gains, np.float64).reshape(B, S, 1)
    rho_g = 0.0 if gains is None else 1.0
    ge = g * e
    x0 = (ge - mu) / sd
    A0 = (np.abs(ge) + np.abs(mu)) / sd
    Ag = np.abs(ge) / sd  # the part of A0 that carries the narrowed gain
    if mean_from == "mix":
        m = K.f64(mixn).reshape(B, 1, T) / S
        Am, Amg, k = np.abs(m), 0.0, max(7, S + 4)
    else:
        m, Am, Amg, k = K._ms(x0), K._ms(A0), K._ms(Ag), S + 7
    mz, amz = K._ms(zz), K._ams(zz)
    ref = m + d * (x0 - m) + (a * mz + p * (zz - mz))
    Ad = d * (A0 + Am)
    Aa, Ap = a * amz, p * (np.abs(zz) + amz)
    bound = K.U * (k * (Am + Ad + Aa + Ap) + rd * Ad + ra * Aa + rp * Ap + rho_g * (Amg + d * (Ag + Amg)))
    if lengths is not None:
        for b, L in enumerate(lengths):
            ref[b, :, L:], bound[b, :, L:] = 0.0, 0.0
    return ref, bound
