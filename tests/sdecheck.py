"""Float64 references and per-element bounds for the kernels of csrc/sde.hip (sampler state updates, the SDE object surface,
noise, time-domain reductions, time embedding, the wide Dense_0 projection), on the pattern of tests/convcheck.py, whose
assert_elementwise is the gate.  Everything is float64 numpy, computed from the STORED fp32 inputs and the fp32 scalars the
kernel is given (t, snr, the SDE parameters, f_scale / g_scale); nothing below is fitted to device output.

NOTATION.  U = 2^-24: the relative error of one correctly rounded fp32 operation (+, -, *, /, an FMA, a narrowing cast).  Every
bound has the form

    bound = U * (k * A + sum_c rho_c * A_c)

A: the kernel's expression evaluated on the absolute values of its terms (|v_i - mean_s v| -> |v_i| + mean_s |v|); k: the
fp32 roundings on the longest path from an input to the output, counted in the kernel source (an a * b + c that hipcc's default
-ffp-contract=fast turns into an FMA is ONE rounding; a product by 2.0f or 0.5f none); rho_c: the relative error, in units of
U, of a per-utterance coefficient c, and A_c the part of A that carries c.

DEVICE MATH FUNCTIONS (ULP below).  The HIP math-API accuracy tables are not part of the ROCm install this suite runs on (only
the runtime API's doxygen index is), so every function is ASSUMED to be within 2 ulp = 4 U of its result: logf, expf, powf,
sqrtf, sinf, cosf, sincosf.  The assumption is this table and nothing else; a ratio above 1 on the device is a finding about
the kernel or about this table, never a reason to raise it silently.

PER-UTTERANCE COEFFICIENTS (mix_coef, g_coef; common.h mix_eig / sde_g_of_t), all relative errors in units of U:
    r = smax / smin: 1.      srp = powf(r, 2t) (2t exact): 4 + 2t (the error of r, amplified by the exponent).
    mult = smin * smin: 1.   ev1 = mult * (srp - 1): absolute  mult * srp * (4 + 2t) + 3 |ev1|  (mult, the subtraction, the
    product) — the cancellation r^{2t} - 1 divides the first term by srp - 1, 34 U at t = 0.03, r = 10.
    ex = expf(-2 lam t): 4 + 2 lam t (one rounding of the argument).   logf(r): 4 + 1 / ln r (the error of r).
    denom = 1 + lam / logf(r): q (5 + 1 / ln r) / denom + 1, q = lam / ln r.
    ev2 = mult * (srp - ex) / denom: absolute  mult / denom * (srp (4 + 2t) + ex (4 + 2 lam t)) + (4 + rho_denom) |ev2|.
    a = sqrtf(ev1), p = sqrtf(ev2): half the relative error of the argument + 4.      A product with sigma_mix: + 1.
    g = smin * powf(r, t) * sqrtf(2 logf(r)): (4 + t) + 1 + (0.5 (4 + 1 / ln r) + 4) + 1.
    G = g [* sigma_mix] * sqrtf(dt), dt = 1.0f / N: rho_g [+ 1] + 1 + (0.5 + 4).

MEAN OVER SOURCES  m = (v_0 + .. + v_{S-1}) / S: S - 1 additions and a division, S roundings, |dm| <= S U mean_s |v|.

THE BOUNDS, kernel by kernel (k, then where its roundings are):
  prior              x = c y + (a m + p (z_i - m)):  k = S + 4: m (S), z_i - m, a * m, the FMA with p, the sum with c y (c = 1.0f / S
                     and c * y are two roundings on a shorter path).  Coefficients: rho_a on a mean|z|, rho_p on p (|z_i| + mean|z|).
  corrector (0 / 1)  u = a mg + p (g_i - mg); llg = a (a mg) + p (u - a mg); mean = x + step llg; xo = mean + (a2 mn + p2 (n_i - mn)),
                     step = 2 snr snr, a2 = 2 snr a.  k(mean) = S + 8: mg (S), g_i - mg, a * mg, FMA (u), u - a mg, a * (a mg), FMA (llg),
                     step (1) folded with the FMA into x (1).  k(xo) = S + 9.  Every term of llg carries two coefficients (2 rho), the
                     noise term one; variant 1 sets p = a.
  predictor          mean = x_i - (f - G G s h), f = (-lam (x_i - mx)) dt;  xo = mean + G z.  k(mean) = S + 6: mx (S), the difference, * lam,
                     * dt, dt itself, f - (..), x_i - rev_f; the score path G * G, * s, (* h exact) is shorter.  2 rho_G on G^2 |s| h;
                     k(xo) = S + 7, rho_G on G |z|.  probability flow: h = 0.5, no noise, xo == mean bit for bit.
  sde_coefficients   drift = (-lam (x_i - mx)) fs: k = S + 3.  diffusion = g [* sigma_mix] * gs: (rho_g [+ 1] + 1) U |ref|.
  sde_mean           out = mx + d (x_i - mx), d = expf(-t lam): k = S + 2 (mx, the difference, one FMA); rho_d = 4 + t lam on d (..).
  sde_std            L = (a inv + p (delta - inv)) sm, inv = 1.0f / S: k = 5 (inv, delta - inv, a * inv, FMA, * sm).
  sde_mult_std       S FMAs: k = S on sum_d |L| |x|.
  sde_reverse_drift  out = f - g g s h: k = 3 on |f| + g^2 |s| h.
  sigma_mix          n FMAs over the n in-range samples of the window, / k, clamp, sqrtf, * 0.5: all terms positive, so relative:
                     (0.5 (n + 1) + 4) U.  The floor value is 0.5 sqrt(fp32(1e-4)).
  normalize_batch    fp64 sums: d_mean = 2^-53 (sum|m| + |mean|); rel(var) = (T + 2) 2^-53 + 2 sum|d| d_mean / sum d^2;
                     rel(std) = 0.5 rel(var) + 2^-53 + U (the narrowing).  mean_o: d_mean + U |mean| (the narrowing).  The kernel
                     subtracts the NARROWED mean: out = (m - mu) / sd, |d out| <= (d_mean + U |mean| + |m - mean| (2 U + rel(std))) / std
                     — U |mean| / std per element is what an offset of 1000 on a deviation of 1e-3 costs.
  scale_output       num, den in fp64 (products exact): d_num = T 2^-53 sum|m x|, rel(den) = (T + 1) 2^-53; alpha narrowed (U);
                     out = alpha x (U).
  gram               fp64 sums of exact products: T 2^-53 sum |r_a e_c| per entry; the reference sums with math.fsum.
  langevin           norms in fp64 (rho_64 = (n + 4) 2^-29 in units of U), r = snr * (float) zn / (float) gn: 4 + 2 rho_64; step = r r 2:
                     rho_step = 2 rho_r + 1 — ONE scalar, so its error multiplies every element of the batch; sq = sqrtf(2 step):
                     0.5 rho_step + 4.  mean = x + step g (FMA): k = 1; xo = mean + z sq (FMA): k = 2.
  time embedding     lt = logf(t) (4); xp = ((lt W) 2) pi (2 roundings; the constant is fp32(pi), which the reference uses as it is):
                     |d xp| <= 6 U |xp| — |xp| reaches 10^3, an ulp of logf(t) moves the argument by |xp| 2^-23; sinf / cosf: + 4 U.
                     linear_kernel: ceil(K / 64) FMAs per lane, 6 butterfly additions, the bias: k = ceil(K / 64) + 7, on
                     sum |x| |W| + |b|, plus the input errors through |W|.  SiLU (silu_t<float>): expf of an exact argument (4 sigma(-v)),
                     1 + e, the division: (4 sigma(-v) + 2) U |silu(v)|; an input error passes with |silu'| <= 1.1.
  dense projection   linear_t16_kernel<K / 16> (K = 64, 128, 256, 512): K / 16 FMAs, 16 LDS partial sums, the bias: k = K / 16 + 17;
                     linear_t_kernel (every other K): K FMAs and the bias: k = K + 1; SiLU as above.

THE INSTRUMENTS, what each sees and cannot see:
  Philox reference (philox4x32_10, randn_ref, randn_batch_ref): Philox4x32-10 on uint32 words, counter (q lo, q hi, stream-id lo,
    stream-id hi), key (seed lo, seed hi), u = ((c >> 8) + 0.5f) 2^-24 in float32 arithmetic (bit-identical, u == 1.0 for
    c >> 8 == 0xffffff included: radius 0), angle = the single fp32 product 6.28318530718f * u, then sqrt(-2 ln u), cos, sin in
    float64.  Bound c 2^-23 |ref| with c = 0.5 ulp(logf) + ulp(sqrtf) + ulp(sincosf) + 0.5 = 5.5: half the logarithm's error passes
    the square root, one rounding for the product.  Sees: a wrong round constant, multiplier, counter or key word, bump, pairing,
    output order, tail handling, batch layout.  Cannot see: the counter's high word (needs n > 2^34).
  Closed forms with bounds: see any element off by more than its rounding budget — a coefficient of the wrong utterance on one
    element, a mean over the wrong number of sources, a missing term.  Cannot see: errors below that budget; the `lens` arguments of
    the three sampler updates, which have no unit entry (the engine's batch-equals-single tests cover them).
  Exact integers (dense projection): x, W in -3 .. 3, integer bias, no SiLU: every partial sum is an integer below 2^24 in any
    order, torch.equal.  Sees: a wrong row, column, tail, offset.  Cannot see: rounding, the SiLU.

MEASURED below: worst err / bound per family on the MI355X, copied from the output of tests/test_sde_gpu.py.  Records, not gates;
the gate is 1.  Near 1, and why: sde_mult_std at S = 1 (0.98) is ONE FMA against a bound of one rounding, so the ratio is the
rounding error itself in units of half an ulp, which reaches 1 just above a power of two; scale_output (0.89) has two roundings
(alpha narrowed, the product) against 2 U |ref| less the fp64 terms; the Langevin step (0.86 at 1025 samples) and normalize_batch
(0.71 .. 0.80) are one or two roundings on top of a narrowed fp64 scalar.  Far from 1: the time embedding (0.003 .. 0.02), whose
bound sums the worst-case argument error 6 U |xp| of every Fourier feature through two dense layers, and the dense projection at
large K (K + 1 roundings in the worst order): those see a wrong row, column or feature, not a wrong low-order bit.
"""
import math

import numpy as np

U = 2.0 ** -24
# assumed accuracy of the device math functions, in ulp of the result (see the docstring: not documented in the local install)
ULP = {"logf": 2, "expf": 2, "powf": 2, "sqrtf": 2, "sinf": 2, "cosf": 2, "sincosf": 2}
NOISE_C = 0.5 * ULP["logf"] + ULP["sqrtf"] + ULP["sincosf"] + 0.5
PI32 = float(np.float32(3.14159265358979323846))
TWO_PI_F32 = np.float32(6.28318530718)
SIGMA_FLOOR = float(np.float32(1e-4))
STD_FLOOR = float(np.float32(1e-5))

# case family -> worst err / bound on the MI355X (copied from the output of tests/test_sde_gpu.py; records, not gates)
MEASURED = {
    "randn, seeds 0 / 123 / 2^40 + 5 / 2^64 - 1": (0.356, 0.300, 0.317, 0.352),
    # (prior, corrector, predictor) per S = 1 .. 4
    "updates MixSDE": ((0.164, 0.178, 0.171), (0.119, 0.144, 0.244), (0.159, 0.140, 0.312), (0.091, 0.128, 0.238)),
    "updates PriorMixSDE": ((0.176, 0.174, 0.193), (0.134, 0.157, 0.256), (0.102, 0.147, 0.319), (0.089, 0.136, 0.293)),
    # (coefficients, mean, std, mult_std, reverse_drift) per S = 1 .. 4
    "surface MixSDE": ((0.065, 0.000, 0.101, 0.978, 0.682), (0.343, 0.257, 0.118, 0.780, 0.663), (0.401, 0.234, 0.044, 0.687, 0.681),
                       (0.323, 0.211, 0.067, 0.603, 0.713)),
    "surface PriorMixSDE": ((0.158, 0.000, 0.135, 0.974, 0.773), (0.331, 0.263, 0.152, 0.746, 0.609), (0.377, 0.245, 0.078, 0.662, 0.739),
                            (0.322, 0.184, 0.100, 0.560, 0.728)),
    "sigma_mix": 0.264,
    # (out, mean, std) per T = 2, 1023, 1024, 1025, 3000
    "normalize_batch": ((0.325, 0.507, 0.077), (0.714, 0.145, 0.797), (0.467, 0.476, 0.254), (0.479, 0.359, 0.296), (0.603, 0.221, 0.603)),
    "scale_output S = 1 .. 4": (0.886, 0.854, 0.869, 0.854), "gram S = 1 .. 4": (0.002, 0.002, 0.002, 0.002),
    "langevin (B, n) = (1, 1), (1, 1025), (3, 1), (3, 1025)": (0.145, 0.787, 0.283, 0.859),
    "time embedding nf = 8, 16, 24, 32, 64": (0.018, 0.009, 0.008, 0.004, 0.003),
    "dense linear_t16 K = 64, 128, 256, 512 at (O, B) = (65, 17)": (0.086, 0.053, 0.030, 0.016),
    "dense generic K = 4, 20, 32, 96, 1024 at (O, B) = (65, 17)": (0.345, 0.154, 0.075, 0.026, 0.004),
    "dense tails, K = 128 / 96, worst over O, B and the two-block placement": (0.062, 0.039),
}


def fu(name):
    """error of a device math function in units of U"""
    return 2.0 * ULP[name]


def f32(v):
    return float(np.float32(v))


def f64(a):
    """a stored fp32 tensor (numpy or torch) as float64 numpy"""
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    a = np.asarray(a)
    assert a.dtype == np.float32, a.dtype
    return a.astype(np.float64)


def _tt(t):
    """times [B] (tensor, array or list) as the fp32 values the kernel reads, in float64"""
    return f64(t) if hasattr(t, "detach") else f64(np.asarray(t, np.float32))


def rel_rms(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(np.mean((a - b) ** 2)) / (np.sqrt(np.mean(b ** 2)) + 1e-30))


def ratio(out, ref, bound):
    """worst err / bound without asserting (the self-test's planted errors)"""
    err = np.abs(np.asarray(out, np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / np.maximum(bound, 1e-300), np.where(err > 0, np.inf, 0.0))
    return float(r.max())


def check(y, ref_bound, what):
    """convcheck.assert_elementwise on a (ref, bound) pair of numpy arrays; returns the worst err / bound"""
    import torch
    from convcheck import assert_elementwise
    ref, bound = ref_bound
    assert ref.dtype == np.float64 and bound.dtype == np.float64
    y = y.detach().cpu() if hasattr(y, "detach") else torch.as_tensor(np.asarray(y))
    assert tuple(y.shape) == ref.shape, (what, tuple(y.shape), ref.shape)
    return assert_elementwise(y, torch.from_numpy(ref), torch.from_numpy(bound), what)


# ------------------------------------------------------------------------------------------------ Philox4x32-10 + Box-Muller
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr [..., 4], key (k0, k1): uint32 words -> uint32 [..., 4] (Random123's philox4x32-10)"""
    c = [np.asarray(ctr[..., i]).astype(np.uint64) for i in range(4)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & _MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & _MASK]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return np.stack(c, -1).astype(np.uint32)


def uniform_f32(c):
    """u = ((c >> 8) + 0.5f) * 2^-24 in float32 arithmetic, as the kernels compute it (1.0 for c >> 8 == 0xffffff)"""
    x = (np.asarray(c, np.uint32) >> np.uint32(8)).astype(np.float32)
    u = (x + np.float32(0.5)) * np.float32(1.0 / 16777216.0)
    assert u.dtype == np.float32
    return u


def stream_words(nq, seed, sid):
    """the Philox outputs of counters q = 0 .. nq - 1 of stream (seed, sid): uint32 [nq, 4]"""
    q = np.arange(nq, dtype=np.uint64)
    ctr = np.stack([q & _MASK, q >> np.uint64(32), np.full(nq, sid & 0xFFFFFFFF, np.uint64), np.full(nq, (sid >> 32) & 0xFFFFFFFF, np.uint64)], -1)
    return philox4x32_10(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))


def box_muller(u0, u1, u2, u3):
    """float32 uniforms -> float64 [n, 4] = (r0 cos, r0 sin, r1 cos, r1 sin), r0 = sqrt(-2 ln u0) on angle 2 pi u1, r1 from u2 on u3"""
    out = []
    for ur, ua in ((u0, u1), (u2, u3)):
        ang = TWO_PI_F32 * ua
        assert ang.dtype == np.float32
        r = np.sqrt(-2.0 * np.log(ur.astype(np.float64)))
        out += [r * np.cos(ang.astype(np.float64)), r * np.sin(ang.astype(np.float64))]
    return np.stack(out, -1)


def randn_ref(n, seed, sid):
    """(ref, bound) float64 [n] of diffsep_randn(n, seed, stream id)"""
    w = stream_words((n + 3) // 4, seed, sid)
    u = uniform_f32(w)
    ref = box_muller(u[:, 0], u[:, 1], u[:, 2], u[:, 3]).reshape(-1)[:n]
    return ref, NOISE_C * 2.0 ** -23 * np.abs(ref)


def randn_batch_ref(S, T, seeds, lens, sid):
    """(ref, bound) [B, S, T] of diffsep_randn_batch: element (s, t) of utterance b is value s * len_b + t of its stream, zero tail"""
    B = len(seeds)
    ref, bound = np.zeros((B, S, T)), np.zeros((B, S, T))
    for b in range(B):
        L = int(lens[b])
        assert 0 <= L <= T
        r, e = randn_ref(S * L, int(seeds[b]), sid)
        ref[b, :, :L], bound[b, :, :L] = r.reshape(S, L), e.reshape(S, L)
    return ref, bound


# ------------------------------------------------------------------------------------------------ per-utterance coefficients
class Coef:
    pass


def _sde_scalars(sde):
    smin, smax, lam = f32(sde["sigma_min"]), f32(sde["sigma_max"]), f32(sde["d_lambda"])
    r = smax / smin
    return smin, smax, lam, r, math.log(r)


def mix_coef(sde, t, variant=0):
    """a = sqrt(ev1), p = sqrt(ev2) [B] of mix_eig at fp32 times t, and their relative errors ra, rp in units of U"""
    t = _tt(t)
    smin, _, lam, r, lnr = _sde_scalars(sde)
    c = Coef()
    srp = r ** (2.0 * t)
    e_srp = srp * (fu("powf") + 2.0 * t)
    mult = smin * smin
    ev1 = mult * (srp - 1.0)
    e_ev1 = mult * e_srp + 3.0 * np.abs(ev1)
    arg = 2.0 * lam * t
    ex = np.exp(-arg)
    e_ex = ex * (fu("expf") + arg)
    q = lam / lnr
    rel_ln = fu("logf") + 1.0 / lnr
    denom = 1.0 + q
    rel_den = q * (rel_ln + 1.0) / denom + 1.0
    ev2 = mult * (srp - ex) / denom
    e_ev2 = mult / denom * (e_srp + e_ex) + (4.0 + rel_den) * np.abs(ev2)
    assert (ev1 > 0).all() and (ev2 > 0).all()
    c.ev1, c.ev2 = ev1, ev2
    c.a, c.ra = np.sqrt(ev1), 0.5 * e_ev1 / ev1 + fu("sqrtf")
    c.p, c.rp = np.sqrt(ev2), 0.5 * e_ev2 / ev2 + fu("sqrtf")
    if variant == 1:
        c.p, c.rp = c.a, c.ra
    return c


def g_coef(sde, t):
    """g(t) = smin r^t sqrt(2 ln r) [B] and its relative error in units of U"""
    t = _tt(t)
    smin, _, _, r, lnr = _sde_scalars(sde)
    g = smin * r ** t * math.sqrt(2.0 * lnr)
    rg = (fu("powf") + t) + 1.0 + (0.5 * (fu("logf") + 1.0 / lnr) + fu("sqrtf")) + 1.0
    return g, rg


def _ms(v):
    """mean over sources [B, 1, T]"""
    return v.mean(1, keepdims=True)


def _ams(v):
    return np.abs(v).mean(1, keepdims=True)


def _b(v):
    """[B] -> [B, 1, 1]"""
    return np.asarray(v, np.float64).reshape(-1, 1, 1)


def _sm(smix, B, T):
    """sigma_mix [B, T] -> ([B, 1, T] | 1.0, 1 | 0: the extra rounding of the product)"""
    if smix is None:
        return 1.0, 0.0
    s = f64(smix).reshape(B, 1, T)
    return s, 1.0


# ------------------------------------------------------------------------------------------------ sampler state updates
def prior(sde, y, z, smix=None):
    z = f64(z)
    B, S, T = z.shape
    y = f64(y).reshape(B, 1, T)
    c = mix_coef(sde, np.ones(B, np.float32))
    sm, one = _sm(smix, B, T)
    a, p = _b(c.a) * sm, _b(c.p) * sm
    ra, rp = _b(c.ra) + one, _b(c.rp) + one
    cf = 0.5 if (S == 2 or smix is not None) else 1.0 / S
    mz, amz = _ms(z), _ams(z)
    ref = cf * y + (a * mz + p * (z - mz))
    Aa, Ap = a * amz, p * (np.abs(z) + amz)
    A = np.abs(cf * y) + Aa + Ap
    return ref, U * ((S + 4) * A + ra * Aa + rp * Ap)


def corrector(sde, snr, x, t, score, z, smix=None, variant=0):
    """((x_out, bound), (x_mean, bound)) of the ald2 (variant 0) / ald (variant 1) corrector step"""
    x, g, n = f64(x), f64(score), f64(z)
    B, S, T = x.shape
    snr = f32(snr)
    c = mix_coef(sde, t, variant)
    sm, one = _sm(smix, B, T)
    a, p = _b(c.a) * sm, _b(c.p) * sm
    rho = np.maximum(_b(c.ra), _b(c.rp)) + one
    step = 2.0 * snr * snr
    mg, amg, mn, amn = _ms(g), _ams(g), _ms(n), _ams(n)
    u = a * mg + p * (g - mg)
    llg = a * (a * mg) + p * (u - a * mg)
    mean = x + step * llg
    noise = 2.0 * snr * (a * mn + p * (n - mn))
    Au = a * amg + p * (np.abs(g) + amg)
    Allg = a * a * amg + p * (Au + a * amg)
    Amean = np.abs(x) + step * Allg
    Anoise = 2.0 * snr * (a * amn + p * (np.abs(n) + amn))
    bm = U * ((S + 8) * Amean + 2.0 * rho * step * Allg)
    bx = U * ((S + 9) * (Amean + Anoise) + 2.0 * rho * step * Allg + rho * Anoise)
    return (mean + noise, bx), (mean, bm)


def predictor(sde, N, x, t, score, z, smix=None, pflow=False):
    """((x_out, bound), (x_mean, bound)) of the reverse-diffusion predictor step; pflow: the probability-flow variant"""
    x, s = f64(x), f64(score)
    B, S, T = x.shape
    _, _, lam, _, _ = _sde_scalars(sde)
    g, rg = g_coef(sde, t)
    sm, one = _sm(smix, B, T)
    dt = 1.0 / N
    G = _b(g) * sm * math.sqrt(dt)
    rG = _b(rg) + one + 1.0 + (0.5 + fu("sqrtf"))
    h = 0.5 if pflow else 1.0
    mx, amx = _ms(x), _ams(x)
    f = -lam * (x - mx) * dt
    mean = x - (f - G * G * s * h)
    Asc = G * G * np.abs(s) * h
    Amean = np.abs(x) + lam * dt * (np.abs(x) + amx) + Asc
    bm = U * ((S + 6) * Amean + 2.0 * rG * Asc)
    if pflow:
        return (mean, bm), (mean, bm)
    zz = f64(z)
    An = G * np.abs(zz)
    return (mean + G * zz, U * ((S + 7) * (Amean + An) + 2.0 * rG * Asc + rG * An)), (mean, bm)


# ------------------------------------------------------------------------------------------------ the SDE object surface
def sde_coefficients(sde, x, t, smix=None, f_scale=1.0, g_scale=1.0):
    """((drift, bound) [B,S,T], (diffusion, bound) [B] or [B,S,T])"""
    x = f64(x)
    B, S, T = x.shape
    _, _, lam, _, _ = _sde_scalars(sde)
    fs, gs = f32(f_scale), f32(g_scale)
    mx, amx = _ms(x), _ams(x)
    drift = -lam * (x - mx) * fs
    bd = U * (S + 3) * lam * abs(fs) * (np.abs(x) + amx)
    g, rg = g_coef(sde, t)
    if smix is None:
        diff = g * gs
        return (drift, bd), (diff, U * (rg + 1.0) * np.abs(diff))
    diff = np.broadcast_to(_b(g) * f64(smix).reshape(B, 1, T) * gs, (B, S, T)).copy()
    return (drift, bd), (diff, U * (_b(rg) + 2.0) * np.abs(diff))


def sde_mean(sde, x0, t):
    x = f64(x0)
    B, S, T = x.shape
    _, _, lam, _, _ = _sde_scalars(sde)
    tt = _tt(t)
    d, rd = _b(np.exp(-tt * lam)), _b(fu("expf") + tt * lam)
    mx, amx = _ms(x), _ams(x)
    Ad = d * (np.abs(x) + amx)
    return mx + d * (x - mx), U * ((S + 2) * (amx + Ad) + rd * Ad)


def sde_std(sde, t, S, smix=None, T=1):
    """(L, bound): [B,S,S] or, with sigma_mix [B,T], [B,S,S,T]"""
    c = mix_coef(sde, t)
    B = c.a.shape[0]
    inv = 1.0 / S
    Pn = np.eye(S) - inv
    a, p, ra, rp = (v.reshape(B, 1, 1) for v in (c.a, c.p, c.ra, c.rp))
    L = a * inv + p * Pn[None]
    Aa, Ap = a * inv + 0.0 * Pn[None], p * np.abs(Pn)[None]
    bound = U * (5.0 * (Aa + Ap) + ra * Aa + rp * Ap)
    if smix is None:
        return L, bound
    s = f64(smix).reshape(B, 1, 1, T)
    return L[..., None] * s, bound[..., None] * s


def sde_mult_std(std, x):
    L, x = f64(std), f64(x)
    S = x.shape[1]
    eq = "bcdt,bdt->bct" if L.ndim == 4 else "bcd,bdt->bct"
    return np.einsum(eq, L, x), U * S * np.einsum(eq, np.abs(L), np.abs(x))


def sde_reverse_drift(f, G, score, pflow=False):
    f, G, s = f64(f), f64(G), f64(score)
    if G.ndim == 1:
        G = G.reshape((-1,) + (1,) * (f.ndim - 1))
    h = 0.5 if pflow else 1.0
    return f - G * G * s * h, U * 3.0 * (np.abs(f) + G * G * np.abs(s) * h)


def sigma_mix(mix, k):
    """(ref, bound) [B, T] of PriorMixSDE's per-sample noise scale for mix [B, T] (or [B, 1, T]) and window k"""
    m = f64(mix)
    m = m.reshape(m.shape[0], m.shape[-1])
    B, T = m.shape
    pad = np.zeros((B, k))
    sq = np.concatenate([pad, m * m, pad], 1)  # sq[:, k + i] = m[i]^2
    win = np.lib.stride_tricks.sliding_window_view(sq, k, axis=1)  # win[:, j] = sq[j : j + k]
    tt = np.arange(T)
    v = win[:, k + tt - k // 2].sum(-1) / k  # window of output t: samples t - k/2 .. t - k/2 + k - 1, zeros outside
    n_in = np.minimum(T, tt - k // 2 + k) - np.maximum(0, tt - k // 2)
    ref = 0.5 * np.sqrt(np.maximum(v, SIGMA_FLOOR))
    return ref, U * (0.5 * (n_in[None] + 1.0) + fu("sqrtf")) * ref


# ------------------------------------------------------------------------------------------------ fp64 reductions
def _fsum(a):
    """exactly rounded sums over the last axis"""
    a = np.asarray(a, np.float64)
    return np.array([math.fsum(r) for r in a.reshape(-1, a.shape[-1])]).reshape(a.shape[:-1])


E53 = 2.0 ** -53


def normalize_batch(mix):
    """dict(out, mean, std -> (ref, bound)) for mix [B, 1, T]"""
    m = f64(mix)
    B, T = m.shape[0], m.shape[-1]
    m = m.reshape(B, T)
    mean = _fsum(m) / T
    d = m - mean[:, None]
    ssq = _fsum(d * d)
    std_raw = np.sqrt(ssq / max(T - 1, 1))
    std = np.maximum(std_raw, STD_FLOOR)
    d_mean = E53 * (np.abs(m).sum(-1) + np.abs(mean))
    rel_var = (T + 2) * E53 + np.where(ssq > 0, 2.0 * np.abs(d).sum(-1) * d_mean / np.where(ssq > 0, ssq, 1.0), 0.0)
    rel_std = 0.5 * rel_var + E53 + U
    b_mean = d_mean + U * np.abs(mean)
    out = d / std[:, None]
    b_out = (b_mean[:, None] + np.abs(d) * (2.0 * U + rel_std[:, None])) / std[:, None] * (1.0 + 4.0 * U)
    return dict(out=(out.reshape(B, 1, T), b_out.reshape(B, 1, T)), mean=(mean, b_mean), std=(std, rel_std * std))


def scale_output(mix, sep):
    x = f64(sep)
    B, S, T = x.shape
    m = f64(mix).reshape(B, 1, T)
    num = _fsum(m * x)
    den = _fsum(x * x) + T * 1e-10
    alpha = num / den
    d_alpha = T * E53 * np.abs(m * x).sum(-1) / den + np.abs(alpha) * ((T + 2) * E53 + U)
    ref = alpha[..., None] * x
    return ref, np.abs(x) * d_alpha[..., None] + U * np.abs(ref)


def gram(ref, est):
    """(G, bound) float64 [B, 3, S, S] = (ref ref^T, ref est^T, est est^T)"""
    r, e = f64(ref), f64(est)
    B, S, T = r.shape
    out, bound = np.zeros((B, 3, S, S)), np.zeros((B, 3, S, S))
    for k, (p, q) in enumerate(((r, r), (r, e), (e, e))):
        prod = p[:, :, None, :] * q[:, None, :, :]
        out[:, k] = _fsum(prod)
        bound[:, k] = T * E53 * np.abs(prod).sum(-1)
    return out, bound


def langevin(snr, x, score, z):
    """((x_out, bound), (x_mean, bound), step) of the Langevin corrector; the step size is one scalar for the whole batch"""
    x, g, n = f64(x), f64(score), f64(z)
    B = x.shape[0]
    npb = x[0].size
    snr = f32(snr)
    gn = np.sqrt(_fsum((g * g).reshape(B, -1))).mean()
    zn = np.sqrt(_fsum((n * n).reshape(B, -1))).mean()
    r = snr * zn / gn
    step = 2.0 * r * r
    rho64 = (npb + 4) * 2.0 ** -29
    rho_step = 2.0 * (4.0 + 2.0 * rho64) + 1.0
    sq = math.sqrt(2.0 * step)
    rho_sq = 0.5 * rho_step + fu("sqrtf")
    mean = x + step * g
    Am = np.abs(x) + step * np.abs(g)
    An = sq * np.abs(n)
    bm = U * (Am + rho_step * step * np.abs(g))
    bx = U * (2.0 * (Am + An) + rho_step * step * np.abs(g) + rho_sq * An)
    return (mean + sq * n, bx), (mean, bm), step


# ------------------------------------------------------------------------------------------------ time embedding, dense projection
def _sig(v):
    return 1.0 / (1.0 + np.exp(-v))


def silu(v):
    """(silu(v), its own error in units of U): silu_t<float> on an exactly given argument"""
    s = v * _sig(v)
    return s, (fu("expf") * _sig(-v) + 2.0) * np.abs(s)


def _linear(x, ex, W, b, k):
    """y = x W^T + b with input errors ex (units of U) and k roundings: (y, error in units of U)"""
    aw = np.abs(W)
    ab = np.abs(b)[None] if b is not None else 0.0
    y = x @ W.T + (b[None] if b is not None else 0.0)
    return y, ex @ aw.T + k * (np.abs(x) @ aw.T + ab)


def time_embedding(t, fourier_w, w1, b1, w2, b2):
    """(temb, bound) [B, 4 nf] of diffsep_time_embedding"""
    t, Wf, w1, b1, w2, b2 = (f64(v) for v in (t, fourier_w, w1, b1, w2, b2))
    nf = Wf.shape[0]
    xp = np.log(t)[:, None] * Wf[None] * 2.0 * PI32
    e_xp = np.abs(xp) * (fu("logf") + 2.0)
    emb = np.concatenate([np.sin(xp), np.cos(xp)], -1)
    e_emb = np.concatenate([e_xp, e_xp], -1) + fu("sinf") * np.abs(emb)
    y1, e1 = _linear(emb, e_emb, w1, b1, math.ceil(2 * nf / 64) + 7)
    v, ev = silu(y1)
    y2, e2 = _linear(v, ev + 1.1 * e1, w2, b2, math.ceil(4 * nf / 64) + 7)
    return y2, U * e2


def dense_roundings(K):
    """roundings of ds_launch_linear_t's route for this K: linear_t16_kernel<K / 16> or the generic linear_t_kernel"""
    return K // 16 + 17 if K in (64, 128, 256, 512) else K + 1


def dense_projection(x, weights, biases=None, silu_in=True):
    """(y, bound) [B, sum O_i] of y = act(x) W^T + b for nn.Linear weight blocks [O_i, K] side by side"""
    x = f64(x)
    W = np.concatenate([f64(w) for w in weights], 0)
    b = np.concatenate([f64(v) for v in biases]) if biases is not None else None
    act, ea = silu(x) if silu_in else (x, np.zeros_like(x))
    y, e = _linear(act, ea, W, b, dense_roundings(x.shape[1]))
    return y, U * e


# ------------------------------------------------------------------------------------------------ inputs shared by the CPU and GPU tests
MIX = dict(kind=0, ndim=2, d_lambda=2.0, sigma_min=0.05, sigma_max=0.5)
PMIX = dict(kind=1, ndim=2, d_lambda=2.0, sigma_min=0.05, sigma_max=0.5, avg_len=510)
T_CASES = np.array([1.0, 0.5, 0.03], np.float32)


def noise(tag, shape, scale=1.0):
    """float32 N(0, 1) * scale, every element its own draw (synth.synth_noise keyed by tag)"""
    from diffsep_amd import synth
    return (synth.synth_noise("sdecheck." + tag, shape) * np.float32(scale)).astype(np.float32)


def sigma_mix_signals(T=700, silent=600):
    """[2, T] float32: an ordinary signal, and one with `silent` exact zeros from sample 50 on"""
    m = noise("smix.m", (2, T), 0.5)
    m[1, 50:50 + silent] = 0.0
    return m


def state_case(tag, B, S, T, pmix):
    """the inputs of one row of the per-index case table: dict of float32 arrays (x, score, z, y [B,1,T], smix [B,T] | None)"""
    c = dict(x=noise(tag + ".x", (B, S, T), 0.5), score=noise(tag + ".s", (B, S, T), 2.0), z=noise(tag + ".z", (B, S, T)),
             y=noise(tag + ".y", (B, 1, T)), smix=None)
    if pmix:  # from the float64 reference rounded to fp32: the kernels under test do not feed each other
        c["smix"] = sigma_mix(c["y"], 5)[0].astype(np.float32)
    return c


def int_case(tag, B, K, outs):
    """exact-integer operands of the dense projection: x [B,K], weights [O_i,K] in -3 .. 3, biases in -8 .. 8 (float32)"""
    from diffsep_amd import synth

    def ints(t, shape, lo, hi):
        n = int(np.prod(shape))
        return (np.floor(synth.uniform01("sdecheck." + t, n) * (hi - lo + 1)) + lo).astype(np.float32).reshape(shape)
    return (ints(tag + ".x", (B, K), -3, 3), [ints(f"{tag}.w{i}", (o, K), -3, 3) for i, o in enumerate(outs)],
            [ints(f"{tag}.b{i}", (o,), -8, 8) for i, o in enumerate(outs)])


def rand_case(tag, B, K, outs):
    return (noise(tag + ".x", (B, K), 1.5), [noise(f"{tag}.w{i}", (o, K), 1.0 / math.sqrt(K)) for i, o in enumerate(outs)],
            [noise(f"{tag}.b{i}", (o,), 0.3) for i, o in enumerate(outs)])


# (K, O blocks, B) of the dense projection: every K with (O, B) = (65, 17) and (1, 1); every O and every B once on each route
DENSE_K16 = (64, 128, 256, 512)
DENSE_KGEN = (4, 20, 32, 96, 1024)
DENSE_O = (1, 15, 16, 17, 63, 64, 65, 200)
DENSE_B = (1, 15, 16, 17, 33)


def dense_cases():
    cases = []
    for K in DENSE_K16 + DENSE_KGEN:
        cases += [(K, (65,), 17), (K, (1,), 1)]
    for K in (128, 96):  # one K of each route
        cases += [(K, (o,), 5) for o in DENSE_O if o not in (1, 65)]
        cases += [(K, (33,), b) for b in DENSE_B if b not in (1, 17)]
        cases += [(K, (17, 48), 18)]  # two weight blocks side by side (offset / ldo placement)
    return cases
