"""Instruments for the STFT / iSTFT front end of csrc/stft.hip (ops.stft_pack, ops.istft_unpack; n_fft = 510, hop = 128), on the
pattern of tests/convcheck.py and tests/gncheck.py: float64 references of the two operations, a derived per-element error bound for
every route, and fp32 / bfloat16-split simulations of the two fused kernels that validate the bounds without a GPU
(tests/test_stftcheck_cpu.py).  Nothing here imports the device library; nothing is fitted to device output.

REFERENCES (torch float64, the DFT as a dense matrix product; exponent and factor are taken at their float32 values, which is what
the C entry points receive):
  stft_ref   frame f, tap n reads sample 128 f - 255 + n of cat(xt, mix) (zero outside [0, T)); periodic Hann window
             w_n = (1 - cos(2 pi n / 510)) / 2; z_k = sum_n w_n x_n exp(-2 pi i k n / 510), k < 256; y = z |z|^(e-1) factor;
             channels [re x (S+1) | im x (S+1)], NHWC [B, 256, W, 8]; frames [F, W) are 0; then 2 y - 1 on the 2 (S+1) channels.
  istft_ref  v = (ow x) / t[b] + ob (or the first 2 S channels), z = (v_s + i v_{S+s}) / |factor|, U = z |z|^(1/e - 1);
             frame_f[n] = sum_K U_K inv[n, K], inv[n, k] = w_n c_k cos(2 pi k n / 510) / 510, inv[n, 256 + k] = -w_n c_k sin(.) / 510,
             c_0 = c_255 = 1 (their imaginary columns are 0), c_k = 2 otherwise; out[t] = sum_f frame_f[t + 255 - 128 f] / env[t],
             env[t] = sum_f w^2[t + 255 - 128 f], t < T.  (128 (F - 1) > T always: tests/test_stftcheck_cpu.py.)

BOUNDS.  u = 2^-24 (one fp32 rounding to nearest; a format of p significand bits rounds with relative error <= 2^-p: bfloat16
2^-8, half 2^-11).  A term that passes through d fp32 additions on its way into a sum contributes at most d u (1 + d u) of its
magnitude to the sum's error, whatever the order: sequential summation of n terms has d <= n, a blocked one the block depth.

Forward, |got - ref| per stored number:
  operands   fused and split routes keep each operand as hi + lo, hi = bf16(v), lo = bf16(v - hi): |v - hi - lo| <= 2^-16 |v| (two
             roundings to 8 significand bits: 16 kept), and drop lo_a lo_b <= 2^-16 |a b|: three relative terms of 2^-16, with their
             cross terms 3 * 2^-16 (1 + 2^-7).  The fused table entry fl32(w_n cos) carries one u; the three-launch routes form
             fl32(fl32(w_n) x_n) and read fl32(cos): 3 u.    eps_op = 3 * 2^-16 (1 + 2^-7) + u (fused) | + 3 u (split) | 3 u (fp32)
  sum        the fused kernels chain 3 x 32 MFMAs on one accumulator, each adding a block of 16 exact bfloat16 products: a product
             passes through at most 16 additions inside its block, in whatever order the matrix unit takes them, and at most 96 of
             the chain: n_acc = 112.  The generic GEMM of the three-launch routes is taken in any order and grouping: n_acc = 512
             products (fp32, an fmaf chain) or 3 x 512 (split).  n_acc u (1 + 2^-7) of sum |terms| (the lo products add 2^-7 to
             the sum of magnitudes).
  so         |d Re z| <= c A_re, |d Im z| <= c A_im, c = eps_op + n_acc u (1 + 2^-7), A_re = sum_n |w_n x_n cos|, A_im = sum_n |w_n x_n sin|
             (each <= the A = sum |w_n x_n| of the plain form), |dz| <= sqrt(d Re^2 + d Im^2).
  compress   g(z) = z |z|^(e-1) has the Jacobian norm |z|^(e-1) for e <= 1 (tangential; radial e |z|^(e-1)), decreasing in |z|:
             |g(z + dz) - g(z)| <= (|z| - |dz|)^(e-1) |dz| for |dz| < |z| (mean value along the segment: first order plus its
             remainder), and g is Hoelder: |g(a) - g(b)| <= 2^(1-e) |a - b|^e.  |dy| <= factor * the smaller of the two: finite and
             valid where |z| << A.  e = 1: factor |dz|.
  scale      m2 = fma(re, re, im im) (2 u), sqrt and rsq at 1 ulp = 2 u each on the e = 0.5 path (sqrtf + powf at <= 2 ulp, with the
             exactly representable exponent e - 1, on the general one), sc * factor, re * sc: <= 12 u |y|.
  shift      fmaf(2, v, -1) or 2 v - 1: the error so far doubles, + u (|2 y| + |2 y - 1|).
  storage    rounding to the output type: u_st (|ref| + error so far), u_st = 2^-8 (bfloat16) | 2^-11 (half, + 2^-25 absolute for
             subnormals) | 0 (fp32): half an ulp of a number just above a power of two.
  Frames [F, W) and channels [2 (S+1), 8) are compared exactly by the tests, and the bound is 0 there and wherever the input is silent.

Inverse, |got - ref| per output sample (the input is exact: the reference reads the same 16-bit or fp32 numbers):
  layer      a = fmaf chain over ow_cin terms, then fmaf(a, fl(1/t), b) or a / t + b:
             |dv| <= (ow_cin + 2) u sum_k |ow_ck x_k| / t + 2 u |v|; without ow the chain is 1 * x + 0: exact.
  decompress h(z) = z |z|^p, p = 1/e - 1 >= 0, Jacobian norm (1 + p) |z|^p increasing in |z|:
             |dU| <= (1/e) (|z| + |dz|)^p |dz|, |dz| = |dv| / |factor|, plus the arithmetic fl(1/|factor|), the product, m2, sqrt at 1 ulp,
             re * sc: 10 u |U|; general exponent: p itself is fl(fl(1/e) - 1), relative error <= (1 / (1 - e) + 1) u, which moves
             |z|^p by p |ln |z|| times that: (12 + 4 |ln |z||) u |U|.
  product    P[f, n] = sum_K |U_K inv[n, K]|; the same eps_op (U split hi / lo, the table fl32 of double then split; fp32 route: u)
             and n_acc u (1 + 2^-7) as forward, and dU enters through |inv|: E[f, n] = sum_K |dU_K| |inv[n, K]| (both components
             of a bin are given the modulus bound |dU|: at most sqrt 2 loose).
  overlap    up to 4 contributions added in a fixed order (3 u of sum_f P), den = up to 4 fl32(w)^2 summed (6 u), fl(1 / den) and the
             product, or num / den (2 u): 11 u of sum_f P / env.
  so         bound[t] = ((eps_op + n_acc u (1 + 2^-7) + 11 u) sum_f P[f, n_f(t)] + (1 + 2^-10) sum_f E[f, n_f(t)]) / env[t].

Sees: any element off by more than its rounding budget: a frame at a tile edge that reads the neighbouring hop, a swapped bin at the
row-half boundary, a dropped lo plane, a segment that misses its predecessor's last frame, a stale overlap-add copy, a missing bias
(tests/test_stftcheck_cpu.py shows each passes a relative-RMS gate of the older tests).  Cannot see: an error below the accumulation
budget, which is the worst case over signs and orders, well above what random data produces (the simulated ratios below).

MEASURED: worst |got - ref| / bound per case family: the simulated fused kernels (tests/test_stftcheck_cpu.py prints them) and the
MI355X (tests/test_stft_gpu.py prints them).  Records, not gates; the gate is 1.
"""
import functools
import math

import numpy as np
import torch

from convcheck import BF, HF, F32, rel_rms, round_dt  # noqa: F401
from diffsep_amd import synth

N_FFT, HOP, BINS, SEG = 510, 128, 256, 29 * 128
U = 2.0 ** -24
U_ST = {BF: 2.0 ** -8, HF: 2.0 ** -11, F32: 0.0}
SPLIT_EPS = 3 * 2.0 ** -16 * (1 + 2.0 ** -7)
ROUTES = ("fused", "split", "f32")
N_ACC = {"fused": 112, "split": 1536, "f32": 512}
EPS_FWD = {"fused": SPLIT_EPS + U, "split": SPLIT_EPS + 3 * U, "f32": 3 * U}
EPS_INV = {"fused": SPLIT_EPS + U, "split": SPLIT_EPS + U, "f32": U}

# case family -> worst err / bound: (simulated fused kernel, bf16 | f16 build) and the MI355X per route, in the order
# (fused-bf16, fused-f16, f32, f32-split, thin-bf16, thin-f16) of tests/test_stft_gpu.py; None: the family does not run there.
# 16-bit forward outputs sit just under 1: a value just above a power of two is stored with nearly the whole u_st |ref| of error, and
# the transform's own error adds to it (the fp32 routes show what the transform spends: a few percent of its worst case).  The
# inverse figures are the distance between the worst case over all signs and what one signal does.
MEASURED = {
    "stft noise (all lengths, S, exponents, factors, shift)": ((0.968, 0.849), (0.968, 0.849, 0.007, 0.022, 0.976, 0.894)),
    "stft cancelling tone": ((0.970, 0.798), (0.970, 0.798, 0.019, 0.058, 0.976, 0.843)),
    "stft impulses across the tile edge": ((0.935, 0.816), (0.935, 0.816, 0.005, None, None, None)),
    "stft B = 3, silent entry": (None, (0.931, 0.733, 0.004, 0.012, 0.948, 0.801)),
    "istft noise (all lengths, S, exponents, factors)": ((0.022, 0.018), (0.021, 0.022, 0.007, 0.008, 0.007, 0.005)),
    "istft fused output layer": ((0.022, 0.020), (0.021, 0.020, 0.006, 0.009, 0.006, 0.005)),
    "istft large (+-300, half precision)": ((None, 0.017), (None, 0.017, None, None, None, 0.003)),
    "istft one-hot pixels": ((0.183, 0.183), (0.183, 0.183, 0.008, None, None, None)),
    "round trip fused -> fused": ((0.029, 0.012), (0.029, 0.012, None, None, None, None)),
}


def f32(v):
    return float(np.float32(v))


def n_frames(T):
    return 1 + (T + N_FFT - HOP) // HOP


def width(T, mult=32):
    return (n_frames(T) + mult - 1) // mult * mult


def rnd(tag, shape, scale=1.0):
    return torch.from_numpy(synth.synth_noise(tag, shape)) * scale


@functools.lru_cache(None)
def tables():
    """w [510], C [256, 510] = cos(2 pi k n / 510), Sn = sin(.), IR / II [510, 256] = the inverse matrix's Re / Im columns (float64)"""
    n = torch.arange(N_FFT, dtype=torch.float64)
    k = torch.arange(BINS, dtype=torch.int64)
    w = 0.5 * (1.0 - torch.cos(2.0 * math.pi * n / N_FFT))
    ang = 2.0 * math.pi * ((k[:, None] * torch.arange(N_FFT)[None, :]) % N_FFT).double() / N_FFT
    C, Sn = torch.cos(ang), torch.sin(ang)
    Sn[0] = 0.0
    Sn[BINS - 1] = 0.0                                                   # sin(pi n): exactly 0, not the 1e-16 of the evaluation
    cj = torch.full((BINS,), 2.0, dtype=torch.float64)
    cj[0] = cj[BINS - 1] = 1.0
    IR = (w[:, None] / N_FFT) * cj[None, :] * C.T
    II = -(w[:, None] / N_FFT) * cj[None, :] * Sn.T
    II[:, 0] = 0.0
    II[:, BINS - 1] = 0.0
    return w, C, Sn, IR, II


def frame_index(T):
    """idx [F, 510] int64 = 128 f - 255 + n and its validity mask (inside [0, T))"""
    F_ = n_frames(T)
    idx = HOP * torch.arange(F_)[:, None] - N_FFT // 2 + torch.arange(N_FFT)[None, :]
    return idx, (idx >= 0) & (idx < T)


def gather_frames(x):
    """x [..., T] -> [..., F, 510], zeros outside the signal"""
    idx, ok = frame_index(x.shape[-1])
    return x[..., idx.clamp(0, x.shape[-1] - 1)] * ok.to(x.dtype)


def ola(fr, T):
    """fr [..., F, 510] -> [..., T]: out[t] = sum_f fr[f, t + 255 - 128 f]"""
    F_ = fr.shape[-2]
    buf = torch.zeros(fr.shape[:-2] + (HOP * (F_ - 1) + N_FFT,), dtype=fr.dtype)
    for f in range(F_):
        buf[..., HOP * f:HOP * f + N_FFT] += fr[..., f, :]
    return buf[..., N_FFT // 2:N_FFT // 2 + T]


# ------------------------------------------------------------------------------------------------ forward
def _pack(re, im, W, shift_val=None):
    """re / im [B, NC, F, 256] -> NHWC [B, 256, W, 8]: channels [re x NC | im x NC], zeros elsewhere"""
    B, NC, F_, _ = re.shape
    y = torch.zeros((B, BINS, W, 8), dtype=re.dtype)
    y[:, :, :F_, :NC] = re.permute(0, 3, 2, 1)
    y[:, :, :F_, NC:2 * NC] = im.permute(0, 3, 2, 1)
    return y


def stft_ref(xt, mix, W, exponent=0.5, factor=0.33, shift=False):
    """float64 reference of ops.stft_pack.  Returns a dict: y [B, 256, W, 8] (NHWC, what the kernels store), and for the bound, in
    the same layout with 2 (S+1) channels' worth of frames [B, 256, F, S+1]: z_re, z_im (uncompressed), A_re, A_im."""
    w, C, Sn, _, _ = tables()
    x = torch.cat([xt, mix], 1).double()
    B, NC, T = x.shape
    F_ = n_frames(T)
    assert W >= F_ and 2 * NC <= 8
    e, fac = f32(exponent), f32(factor)
    fr = gather_frames(x) * w
    re, im = fr @ C.T, -(fr @ Sn.T)
    A_re, A_im = fr.abs() @ C.abs().T, fr.abs() @ Sn.abs().T
    mag = torch.sqrt(re * re + im * im)
    sc = torch.where(mag > 0, mag.clamp(min=1e-300) ** (e - 1.0), torch.zeros_like(mag)) * fac
    y = _pack(re * sc, im * sc, W)
    if shift:
        y[..., :2 * NC] = 2.0 * y[..., :2 * NC] - 1.0
    nhwc = lambda t: t.permute(0, 3, 2, 1).contiguous()
    return dict(y=y, z_re=nhwc(re), z_im=nhwc(im), A_re=nhwc(A_re), A_im=nhwc(A_im), S=NC - 1, F=F_, W=W, e=e, fac=fac,
                shift=bool(shift))


def compress_bound(mag, dz, e):
    """|g(z + dz) - g(z)| for g(z) = z |z|^(e-1), e <= 1, given |z| = mag and |dz| <= dz"""
    if e == 1.0:
        return dz
    assert 0.0 < e < 1.0, "the compression bound is derived for 0 < e <= 1"
    first = torch.where(dz < mag, (mag - dz).clamp(min=1e-300) ** (e - 1.0) * dz, torch.full_like(dz, float("inf")))
    return torch.minimum(first, 2.0 ** (1.0 - e) * dz ** e)


def stft_bound(ref, route, out_dt):
    """per-element bound [B, 256, W, 8] on |got - ref['y']| for a kernel of `route` storing `out_dt` (module docstring)"""
    assert route in ROUTES
    NC, F_, e, fac = ref["S"] + 1, ref["F"], ref["e"], ref["fac"]
    c = EPS_FWD[route] + N_ACC[route] * U * (1 + 2.0 ** -7)
    d_re, d_im = c * ref["A_re"], c * ref["A_im"]
    dz = torch.sqrt(d_re * d_re + d_im * d_im)
    mag = torch.sqrt(ref["z_re"] ** 2 + ref["z_im"] ** 2)
    dy = fac * compress_bound(mag, dz, e)                               # [B, 256, F, NC], the modulus
    yv = ref["y"][:, :, :F_, :2 * NC]
    yy = (yv + 1.0) / 2.0 if ref["shift"] else yv                       # the compressed value before the shift
    pre = torch.cat([dy, dy], -1) + 12 * U * yy.abs()
    if ref["shift"]:
        pre = 2.0 * pre + U * ((2.0 * yy).abs() + yv.abs())
    b = pre + U_ST[out_dt] * (yv.abs() + pre)
    if out_dt == HF:
        b = b + 2.0 ** -25
    live = torch.cat([ref["A_re"] + ref["A_im"]] * 2, -1) > 0             # a silent input is transformed exactly
    out = torch.zeros_like(ref["y"])
    out[:, :, :F_, :2 * NC] = torch.where(live, b, torch.zeros_like(b))
    return out


# ------------------------------------------------------------------------------------------------ inverse
def output_layer(x, ow, ob, tdiv):
    """x [B, 256, F, >= ow_cin] float64 -> (v [B, 256, F, 2S], sum_k |ow x| / t)"""
    cin = ow.shape[1]
    t = tdiv.double()[:, None, None, None]
    lin = torch.einsum("ck,bhfk->bhfc", ow.double(), x[..., :cin])
    absl = torch.einsum("ck,bhfk->bhfc", ow.double().abs(), x[..., :cin].abs())
    return lin / t + ob.double(), absl / t


def istft_ref(x, S, T, exponent=0.5, factor=0.33, ow=None, ob=None, tdiv=None, dx=None):
    """float64 reference of ops.istft_unpack on the stored values x [B, 256, W, ld].  dx (optional, [B, 256, >= F, >= 2S]): a bound
    on an error already in the first 2 S channels (the round trip).  Returns a dict: out [B, S, T]; Pola = sum_f P[f, n_f(t)] and
    Eola = sum_f E[f, n_f(t)] (module docstring), env [T]."""
    w, _, _, IR, II = tables()
    F_ = n_frames(T)
    assert x.shape[1] == BINS and x.shape[2] >= F_
    xd = x.double()[:, :, :F_]
    e, fac = f32(exponent), abs(f32(factor))
    p = 1.0 / e - 1.0
    if ow is not None:
        v, absl = output_layer(xd, ow, ob, tdiv)
        dv = (ow.shape[1] + 2) * U * absl + 2 * U * v.abs()
    else:
        v = xd[..., :2 * S]
        dv = torch.zeros_like(v)
    if dx is not None:
        dv = dv + dx.double()[:, :, :F_, :2 * S]
    zr, zi = v[..., :S] / fac, v[..., S:2 * S] / fac                     # [B, 256, F, S]
    mag = torch.sqrt(zr * zr + zi * zi)
    sc = mag ** p if p != 0.0 else torch.ones_like(mag)
    Ur, Ui = zr * sc, zi * sc
    Um = mag * sc
    dzv = torch.sqrt(dv[..., :S] ** 2 + dv[..., S:2 * S] ** 2) / fac
    c_dec = 10.0 if e in (0.5, 1.0) else 12.0 + 4.0 * torch.where(mag > 0, mag.clamp(min=1e-300).log().abs(), torch.zeros_like(mag))
    dU = (1.0 / e) * (mag + dzv) ** p * dzv + c_dec * U * Um
    rows = lambda t: t.permute(0, 3, 2, 1)                               # -> [B, S, F, 256]
    fr = rows(Ur) @ IR.T + rows(Ui) @ II.T                               # [B, S, F, 510]
    P = rows(Ur).abs() @ IR.abs().T + rows(Ui).abs() @ II.abs().T
    E = rows(dU) @ (IR.abs() + II.abs()).T
    env = ola((w * w).expand(F_, N_FFT), T)
    return dict(out=ola(fr, T) / env, Pola=ola(P, T), Eola=ola(E, T), env=env, S=S, T=T, F=F_)


def istft_bound(ref, route):
    """per-sample bound [B, S, T] on |got - ref['out']| for a kernel of `route` (module docstring)"""
    assert route in ROUTES
    c = EPS_INV[route] + N_ACC[route] * U * (1 + 2.0 ** -7) + 11 * U
    return (c * ref["Pola"] + (1 + 2.0 ** -10) * ref["Eola"]) / ref["env"]


def support(f, T):
    """the samples [lo, hi) a pixel of frame f can reach: [128 f - 255, 128 f + 255) within [0, T)"""
    return max(0, HOP * f - N_FFT // 2), max(0, min(T, HOP * f + N_FFT // 2))


# ------------------------------------------------------------------------------------------------ comparison
def worst_ratio(got, ref, bound):
    """max over elements of |got - ref| / bound; an element with bound 0 must be exact (inf otherwise)"""
    got = got.detach().double().cpu() if isinstance(got, torch.Tensor) else torch.as_tensor(got, dtype=torch.float64)
    err = (got - ref).abs()
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    r = torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(r.max())


# ------------------------------------------------------------------------------------------------ inputs
def signal(tag, B, S, T, scale=0.3):
    """(xt [B, S, T], mix [B, 1, T]) float32 noise at the older tests' scale"""
    x = rnd(tag, (B, S + 1, T), scale)
    return x[:, :S].contiguous(), x[:, S:].contiguous()


def cancelling_signal(tag, B, S, T, k0=37, amp=0.3):
    """channel 0 of xt: a pure tone at the exact frequency of bin k0 plus noise 1e-4 below it: its interior frames are nearly
    orthogonal to every bin but k0 and k0 +- 1, so |z| << A there (the Hoelder branch of the bound); the other channels are noise"""
    xt, mix = signal(tag, B, S, T)
    t = torch.arange(T, dtype=torch.float64)
    tone = amp * torch.cos(2.0 * math.pi * k0 * t / N_FFT + 0.3)
    xt[:, 0] = (tone[None, :] + 1e-4 * amp * rnd(tag + ".n", (B, T)).double()).float()
    return xt, mix


def pixels(tag, B, S, T, dt, ld=8, W=None, scale=0.2, fill=0.0):
    """spectrogram pixels [B, 256, W, ld] in the storage type dt: noise at `scale` in the first 2 S channels (all ld with
    fill=None), `fill` in the others.  W: the frame count rounded up to 64, as the engine pads it"""
    W = W or width(T, 64)
    x = rnd(tag, (B, BINS, W, ld), scale)
    if fill is not None:
        x[..., 2 * S:] = fill
    return x.to(dt)


def large_pixels(tag, B, S, T, W=None):
    """half-precision pixels up to +-300: the decompressed |z|^2 reaches 1e6"""
    W = W or width(T, 64)
    x = (rnd(tag, (B, BINS, W, 8), 120.0)).clamp(-300.0, 300.0)
    x[..., 2 * S:] = 0.0
    return x.to(HF)


def layer(tag, B, S):
    """(ow [2S, 2 (S+1)] at 0.5, ob [2S] at 0.1, tdiv [B] in [0.03, 1], different per entry) float32"""
    ow = rnd(tag + ".ow", (2 * S, 2 * (S + 1)), 0.5)
    ob = rnd(tag + ".ob", (2 * S,), 0.1)
    tdiv = torch.tensor([(0.03, 1.0, 0.4, 0.11)[b % 4] for b in range(B)], dtype=torch.float32)
    return ow.contiguous(), ob.contiguous(), tdiv


# ------------------------------------------------------------------------------------------------ simulated fused kernels
def _bf(t):
    return t.to(torch.bfloat16).float()


def _split(t):
    hi = _bf(t)
    return hi, _bf(t - hi)


def _fma(a, b, c):
    """fl32(a b + c) of float32 tensors (the product is exact in float64)"""
    return (a.double() * b.double() + c.double()).float()


def split_gemm(Ah, Al, Bh, Bl, gen):
    """acc[i, j] = sum_K A[i, K] B[j, K] as the fused kernels form it: 32 k-steps of 16, three matrix products per k-step (hi hi,
    lo hi, hi lo), each an fp32 accumulation of 16 exact bfloat16 products in an order drawn from `gen`, added to the fp32
    accumulator.  A: the operand named first in the kernel's mfma calls (table forward, U inverse)."""
    K = Ah.shape[1]
    assert K == 512 and Bh.shape[1] == 512
    acc = torch.zeros((Ah.shape[0], Bh.shape[0]), dtype=torch.float32)
    for ks in range(32):
        for a, b in ((Ah, Bh), (Al, Bh), (Ah, Bl)):
            idx = 16 * ks + torch.randperm(16, generator=gen)
            acc = acc + a[:, idx] @ b[:, idx].T
    return acc


def _pad512(t):
    return torch.nn.functional.pad(t, (0, 512 - t.shape[-1]))


def sim_stft_fused(xt, mix, W, exponent=0.5, factor=0.33, shift=False, out_dt=BF, seed=0, fault=None):
    """stft_fused_kernel in fp32 / bfloat16-split arithmetic, rounding where the kernel rounds.  fault (test_stftcheck_cpu.py):
    ("hop", b, c, f, ks): frame f of channel c takes the 16 taps of k-step ks one hop early;
    ("swap", b, c, f, k): Re and Im of one bin change places;  ("lo", b, c, tile): the samples' lo plane is dropped in one tile."""
    w, C, Sn, _, _ = tables()
    gen = torch.Generator().manual_seed(seed)
    x = torch.cat([xt, mix], 1).float()
    B, NC, T = x.shape
    F_ = n_frames(T)
    e, fac = np.float32(exponent), np.float32(factor)
    xh, xl = _split(x)
    fh, fl = gather_frames(xh), gather_frames(xl)                       # [B, NC, F, 510]: frame r, tap n is sample 128 r + n
    if fault and fault[0] == "hop":
        _, b, c, f, ks = fault
        fh[b, c, f, 16 * ks:16 * ks + 16] = fh[b, c, f - 1, 16 * ks:16 * ks + 16]
        fl[b, c, f, 16 * ks:16 * ks + 16] = fl[b, c, f - 1, 16 * ks:16 * ks + 16]
    if fault and fault[0] == "lo":
        _, b, c, tile = fault
        fl[b, c, 32 * tile:32 * tile + 32] = 0.0
    tab = torch.cat([(w * C).float(), (-(w * Sn)).float()], 0)          # [512, 510]: rows Re k | Im k, the window folded in
    th, tl = _split(_pad512(tab))
    acc = split_gemm(th, tl, _pad512(fh.reshape(-1, N_FFT)), _pad512(fl.reshape(-1, N_FFT)), gen)  # [512, B NC F]
    acc = acc.reshape(2, BINS, B, NC, F_)
    re, im = acc[0].permute(1, 2, 3, 0).clone(), acc[1].permute(1, 2, 3, 0).clone()  # [B, NC, F, 256]
    if fault and fault[0] == "swap":
        _, b, c, f, k = fault
        re[b, c, f, k], im[b, c, f, k] = im[b, c, f, k].clone(), re[b, c, f, k].clone()
    m2 = _fma(re, re, im * im)
    one = torch.ones_like(m2)
    if e == np.float32(0.5):
        sc = torch.where(m2 > 0, one / torch.sqrt(torch.sqrt(m2)), torch.zeros_like(m2))
    elif e == np.float32(1.0):
        sc = one
    else:
        sc = torch.where(m2 > 0, torch.pow(torch.sqrt(m2), float(e - np.float32(1.0))), torch.zeros_like(m2))
    sc = sc * float(fac)
    vr, vi = re * sc, im * sc
    if shift:
        vr, vi = _fma(torch.full_like(vr, 2.0), vr, -one), _fma(torch.full_like(vi, 2.0), vi, -one)
    y = _pack(vr, vi, W)
    if shift:
        y[:, :, F_:, :2 * NC] = -1.0
    return y.to(out_dt)


def sim_istft_fused(x, S, T, exponent=0.5, factor=0.33, ow=None, ob=None, tdiv=None, seed=0, fault=None):
    """istft_fused_kernel in fp32 / bfloat16-split arithmetic.  x [B, 256, W, ld] in a 16-bit type.  fault:
    ("miss_prev", b, s, seg): the first 128 samples of segment seg miss frame 29 seg - 1;
    ("stale", b, s, t0, w): overlap-add copy w is read one sample early at sample t0."""
    wd, _, _, IR, II = tables()
    gen = torch.Generator().manual_seed(seed)
    F_ = n_frames(T)
    B = x.shape[0]
    v = x.float()[:, :, :F_, :8]
    e, fac = np.float32(exponent), np.float32(factor)
    if ow is not None:
        w8 = torch.zeros((2 * S, 8), dtype=torch.float32)
        w8[:, :ow.shape[1]] = ow
        inv_td = (torch.ones_like(tdiv) / tdiv)[:, None, None]
        cols = []
        for c in range(2 * S):
            a = torch.zeros_like(v[..., 0])
            for k in range(8):
                a = _fma(w8[c, k].expand_as(a), v[..., k], a)
            cols.append(_fma(a, inv_td.expand_as(a), ob[c].expand_as(a)))
        v = torch.stack(cols, -1)
    inv_fac = float(np.float32(1.0) / np.float32(abs(fac)))
    vr, vi = v[..., :S] * inv_fac, v[..., S:2 * S] * inv_fac
    m2 = _fma(vr, vr, vi * vi)
    if e == np.float32(0.5):
        sc = torch.sqrt(m2)
    elif e == np.float32(1.0):
        sc = torch.ones_like(m2)
    else:
        sc = torch.where(m2 > 0, torch.pow(torch.sqrt(m2), float(np.float32(1.0) / e - np.float32(1.0))), torch.zeros_like(m2))
    re, im = vr * sc, vi * sc                                            # [B, 256, F, S]
    Umat = torch.cat([re.permute(0, 3, 2, 1), im.permute(0, 3, 2, 1)], -1).reshape(-1, 512)  # rows (b, s, f), [Re 256 | Im 256]
    uh, ul = _split(Umat)
    inv = torch.zeros((512, 512), dtype=torch.float32)                   # [tap n][K]
    inv[:N_FFT, :BINS], inv[:N_FFT, BINS:] = IR.float(), II.float()
    th, tl = _split(inv)
    fr = split_gemm(uh, ul, th, tl, gen).reshape(B, S, F_, 512)
    # overlap-add: copy w holds taps 128 w .. 128 w + 127; summed w = 0 .. 3; then times fl(1 / den)
    t = torch.arange(T)
    q = t + N_FFT // 2
    w32 = wd.float()
    w2 = torch.zeros(512, dtype=torch.float32)
    w2[:N_FFT] = w32 * w32
    num = torch.zeros((B, S, T), dtype=torch.float32)
    den = torch.zeros(T, dtype=torch.float32)
    contrib = []
    for wv in range(4):
        n = HOP * wv + (q % HOP)
        f = q // HOP - wv
        ok = (n < N_FFT) & (f >= 0) & (f < F_)
        cw = fr[:, :, f.clamp(0, F_ - 1), n.clamp(0, 511)] * ok.float()
        if fault and fault[0] == "miss_prev":
            _, b, s, seg = fault
            drop = (f == 29 * seg - 1) & (t >= SEG * seg) & (t < SEG * seg + HOP)
            cw[b, s] = cw[b, s] * (~drop).float()
        if fault and fault[0] == "stale" and fault[4] == wv:
            _, b, s, t0, _ = fault
            cw[b, s, t0] = cw[b, s, t0 - 1]
        contrib.append((cw, n, ok))
    for cw, n, ok in contrib:
        num = num + cw
    for cw, n, ok in reversed(contrib):                                  # den: f ascending = taps descending
        den = den + w2[n.clamp(0, 511)] * ok.float()
    return num * (torch.ones_like(den) / den)


# ------------------------------------------------------------------------------------------------ the cases of both test modules
FWD_W = {300: 32, 3713: 32, 3714: 64, 4000: 128, 4500: 64}


def fwd_cases():
    """(id, dict(T, S, B, exponent, factor, shift, kind)): the forward cases of tests/test_stft_gpu.py, simulated in
    tests/test_stftcheck_cpu.py.  kind: 'noise' | 'cancel'"""
    out = []
    for T in (300, 3713, 3714, 4000):
        out.append((f"T{T}", dict(T=T, S=2, exponent=0.5, factor=0.33, shift=False)))
    for S in (1, 3):
        out.append((f"T3714-S{S}", dict(T=3714, S=S, exponent=0.5, factor=0.33, shift=True)))
    for e in (0.5, 1.0, 0.7):
        for fac, shift in ((0.33, False), (0.15, True)):
            if (e, fac) != (0.5, 0.33):
                out.append((f"T3714-e{e}-f{fac}-shift{int(shift)}", dict(T=3714, S=2, exponent=e, factor=fac, shift=shift)))
    for e in (0.5, 0.7):
        out.append((f"T3714-cancel-e{e}", dict(T=3714, S=2, exponent=e, factor=0.33, shift=False, kind="cancel")))
    return [(i, dict(dict(B=2, kind="noise"), **c)) for i, c in out]


def fwd_input(cid, c):
    make = cancelling_signal if c["kind"] == "cancel" else signal
    return make("stft." + cid, c["B"], c["S"], c["T"])


def inv_cases():
    """(id, dict(T, S, B, exponent, factor, ld, layer, kind)): kind 'noise' | 'large' (half precision only)"""
    out = []
    for T in (300, 3712, 3713, 7425):
        out.append((f"T{T}", dict(T=T, S=2)))
    for S in (1, 3):
        out.append((f"T3713-S{S}", dict(T=3713, S=S)))
    for e, fac in ((1.0, 0.33), (0.7, 0.33), (0.5, 0.15), (0.7, 0.15)):
        out.append((f"T3713-e{e}-f{fac}", dict(T=3713, S=2, exponent=e, factor=fac)))
    for S in (1, 3):
        for e in (1.0, 0.7):
            out.append((f"T300-S{S}-e{e}", dict(T=300, S=S, exponent=e)))          # every (NS, EM) instantiation
    for S in (1, 2, 3):
        for ld in (8, 16):
            out.append((f"T3713-S{S}-layer-ld{ld}", dict(T=3713, S=S, ld=ld, layer=True)))
    out.append(("T3713-layer-e0.7", dict(T=3713, S=2, layer=True, exponent=0.7)))
    out.append(("T3713-large", dict(T=3713, S=2, kind="large")))
    return [(i, dict(dict(B=2, exponent=0.5, factor=0.33, ld=8, layer=False, kind="noise"), **c)) for i, c in out]


def inv_input(cid, c, dt):
    """(x [B, 256, W, ld] in dt, (ow, ob, tdiv) | (None, None, None)).  With a layer every one of the ld channels is noise (the
    first 2 (S+1) are read), without one the channels beyond 2 S are zero."""
    if c["kind"] == "large":
        return large_pixels("istft." + cid, c["B"], c["S"], c["T"]), (None, None, None)
    x = pixels("istft." + cid, c["B"], c["S"], c["T"], dt, ld=c["ld"], fill=None if c["layer"] else 0.0)
    return x, (layer("istft." + cid, c["B"], c["S"]) if c["layer"] else (None, None, None))


IMPULSE_T, IMPULSES = 4500, (3840, 3841, 3968, 4096, 4350)


def impulse_input():
    """(xt [5, 2, 4500], mix): entry b holds a unit impulse at sample IMPULSES[b] of source 0 and nothing else: across the edge of the
    first 32-frame tile (F = 39, W = 64)"""
    xt = torch.zeros((len(IMPULSES), 2, IMPULSE_T))
    for b, n0 in enumerate(IMPULSES):
        xt[b, 0, n0] = 1.0
    return xt, torch.zeros((len(IMPULSES), 1, IMPULSE_T))


def impulse_frames(n0, T=IMPULSE_T):
    """the frames an impulse at n0 reaches: tap n0 - (128 f - 255) in [1, 509] (the window is exactly 0 at tap 0)"""
    return [f for f in range(n_frames(T)) if 1 <= n0 - (HOP * f - N_FFT // 2) <= N_FFT - 1]


ONEHOT_T, ONEHOT_K = 7425, (0, 1, 127, 128, 254, 255)
ONEHOT_F = (0, 28, 29, 30, n_frames(ONEHOT_T) - 1)


def onehot_input(f, dt, S=2):
    """(x [12, 256, W, 8] in dt, probes): entry j holds ONE non-zero pixel, 0.25 at bin ONEHOT_K[j // 2], frame f, source (j // 2) % S,
    the real (j even) or imaginary (j odd) channel.  probes[j] = (k, source, imaginary)"""
    W = width(ONEHOT_T, 64)
    x = torch.zeros((2 * len(ONEHOT_K), BINS, W, 8))
    probes = []
    for j in range(x.shape[0]):
        k, s, part = ONEHOT_K[j // 2], (j // 2) % S, j % 2
        x[j, k, f, s + part * S] = 0.25
        probes.append((k, s, part))
    return x.to(dt), probes
