"""The two instruments of tests/convcheck.py for the TAPS = 1 half of csrc/conv_mfma.hip (1x1 convolutions, the batched NT GEMMs
of the unfused attention path) and for the attention chain built on it (attention_core in engine.hip: scores, softmax_kernel in
norm.hip, P V).  The generators, the representability conditions, check_exact, assert_elementwise and the staging error model are
convcheck's; this module adds what the path has of its own.  Nothing here touches the GPU.

1. EXACT INTEGERS.
   1x1 through ops.conv2d_fused: convcheck.exact_case(ksize=1) — x in 0..3 (times 32 raw, through 32 x + 32 otherwise), weights
   -1 / 0 / +1 with min(32, real input channels) non-zeros per output channel, bias / bias_b / residual multiples of 32,
   out_scale 0.5: torch.equal on the output and both int64 statistics, padding channels zero.
   GEMM through ops.gemm_nt (exact_gemm): the same numbers with what only this entry reaches — a row bias (multiples of 32), a
   shared left operand, a batched Bt that DIFFERS per sample (a launch that reads sample 0's matrix for everyone is wrong on every
   element of sample 1), and div_b = a power of two per sample, different per sample.  The left operand is ints 0..3 times
   16 max|div_b| / out_scale (32 without a divisor at out_scale 0.5, 128 with div_b = (2, 4) or with out_scale = 1 / 8), so that the
   output stays a multiple of 16: the division and the scale only move the exponent.
   Attention through ops.attention (exact_attention), C = 64 / 256 (C^-0.5 = 1 / 8, 1 / 16): q row i = sqrt(C) (e_c + e_{c + C/2}),
   k[j, c] = a[j, c], k[j, c + C/2] = S_c[j] - a[j, c] with integers |a| <= 64, so score[i, j] = S_c[j], an integer pattern of
   magnitude <= 128 (exact in every storage type) built as (a) one key leads by >= 128 -> exp of every other key is exactly 0 in
   fp32 (exp(-104) is below the smallest subnormal; v_exp_f32 flushes earlier) and the row of P is an exact one-hot; (b) two keys tie
   for the lead, the rest >= 128 below -> 0.5 / 0.5; (c) all L scores equal, L a power of two -> 1 / L.  v = ints 0..3 times L (L a
   power of two) or times 2, so the mean of two rows and of L rows is an integer <= 192.  V^T's padding columns [L, Lp) hold 100.
   Sees: a wrong operand, sample, row / column block, chunk, padding column, bias direction, divisor, anywhere, on one element.
   Cannot see: rounding (nothing rounds), the exponential away from 0 and -inf, the reciprocal away from powers of two.

2. PER-ELEMENT BOUND on ordinary random data, reference in float64 from the STORED operands.
   1x1 through ops.conv2d_fused: convcheck.ConvCheck as it is (one tap: K = Cin + 6).
   GEMM (GemmCheck), a raw launch (no input term):
       bound = |out_scale| (K 2^-23 A_all [+ 2^-16 A in split mode]) / |div_b| + u_out |ref|    K = Cin + 6
       A = sum_k |a| |bt|,  A_all = A + |bias| + |res|
   The quotient, the two additions and the scale of the general epilogue (conv_mfma.hip: v / dvs; v + rowb; (v + bv + rv) *
   out_scale) are five roundings of at most 2^-24 (A / |div_b| + |bias| + |res|); with |div_b| <= 4 (asserted) and Cin >= 8 the
   term above leaves 28 * 2^-24 / 4 = 7 * 2^-24 (|bias| + |res|) and Cin 2^-23 A / |div_b| for them and for the accumulation.
   Attention (AttnCheck), counting the roundings of attention_core / softmax_kernel:
       s   scores: one-tap GEMM with out_scale C^-0.5, stored.  |ds| <= (C + 6) 2^-23 As [+ 2^-16 As] + u/2 (|s| + that) =: D_j
           (As = C^-0.5 sum |q| |k|; u/2: round to nearest of the storage type, u = convcheck.ulp_of)
       p   softmax of the stored scores.  Scores off by at most D = max_j D_j move every probability of the row by a factor within
           e^(+-2 D): relative e^(2 D) - 1 (2 D to first order).  x = s_j - max in fp32: exact up to 2^-24 |x|;
           exp_t<float> = expf (2 ulp, the assumption of tests/sdecheck.py), exp_t<bf16_t> = __expf = v_exp_f32(x log2 e): the
           product and the constant 1.5 |x| 2^-24 (convcheck's count), the instruction 2 ulp: relative (2.5 |x| + 4) 2^-24 =: E_j;
           the sum: ceil(L / 64) + 6 additions (lane loop + wave_sum butterfly) and sum_j p_j E_j; 1.0f / sum: 2 ulp assumed;
           e * inv: 2^-24; stored: u/2 (+ 2^-24 absolute in half precision: subnormals; 2^-120 else: flushed exponentials).
           R_j = (1 + e^(2D) - 1)(1 + E_j + sum_j p_j E_j + (ceil(L / 64) + 6 + 4 + 1) 2^-24)(1 + u/2) - 1,  |dp_j| <= p_j R_j + abs
       o   P V: one-tap GEMM with K = Lp (padding columns of P are exact zeros: softmax_kernel writes them), stored:
           |do| <= sum_j |dp_j| |v_j| + (Lp + 6) 2^-23 Ao (1 + max R) [+ 2^-16 Ao] + u |o|,  Ao = sum_j p_j |v_j|
   Sees: any element of o or P off by more than its own rounding budget: a dropped channel tail, a wrong sample's matrix, a row
   block written from its neighbour, padding columns that carry weight, a missing maximum.  Cannot see: an error below one storage
   ulp of the inputs it sums (instrument 1), and in fp32 a wrong low-order bit (K roundings in the worst order are most of the bound).

MEASURED: worst err / bound per family on the MI355X, copied from the tests' output; nothing above was fitted to it.
"""
import math

import numpy as np
import torch

import convcheck as CC
import sdecheck
from convcheck import BF, F32, HF
from diffsep_amd import synth

# family -> worst err / bound on the MI355X as (bfloat16, half, fp32, split); tests/test_gemm_gpu.py prints them
MEASURED = {
    "1x1 N64 raw": (0.495, 0.488, 0.030, 0.223), "1x1 N64 affine": (0.229, 0.216, 0.033, 0.142), "1x1 N64 silu": (0.277, 0.288, 0.031, 0.148),
    "1x1 N64 gn_acc": (0.270, 0.279, 0.015, 0.065),
    "1x1 N32 raw": (0.496, 0.491, 0.086, 0.787), "1x1 N32 affine": (0.347, 0.361, 0.066, 0.393), "1x1 N32 silu": (0.418, 0.418, 0.074, 0.498),
    "1x1 8X8 raw": (0.497, 0.487, 0.099, 0.868), "1x1 8X8 affine": (0.382, 0.346, 0.108, 0.433), "1x1 8X8 silu": (0.416, 0.412, 0.103, 0.402),
    "gemm_nt V^T L20": (0.484, 0.459, 0.017, 0.149), "gemm_nt V^T L20 wide ldy": (0.485, 0.469, 0.016, 0.177),
    "gemm_nt V^T L272": (0.497, 0.481, 0.030, 0.171), "gemm_nt QK^T 20": (0.474, 0.448, 0.024, 0.104),
    "gemm_nt QK^T 68": (0.492, 0.468, 0.029, 0.174), "gemm_nt PV K24": (0.491, 0.486, 0.050, 0.272),
    "gemm_nt output layer": (0.491, 0.495, 0.108, 0.561),
    "attention scores": (0.965, 0.891, 0.015, 0.094), "attention P": (0.494, 0.465, 0.006, 0.045), "attention o": (0.279, 0.264, 0.002, 0.025),
    "attention P gain 30": (0.596, 0.548, 0.008, 0.044), "attention o gain 30": (0.463, 0.441, 0.004, 0.026),
}
# Near the limit, by construction rather than by accident: the stored scores (0.97 / 0.89) — their bound is the half ulp of round
# to nearest plus an accumulation term of 2^-16 of it, so a score just above a power of two, rounded by almost half an ulp, sits at 1;
# and the split mode's raw launches on 8 input channels (0.79 / 0.87; 0.22 on 72 .. 128): the per-product 2^-16 is the dropped
# lo * lo term plus both operands' hi + lo residuals, and eight products leave little room for cancellation.  Raw 16-bit launches sit
# at 0.45 .. 0.50 as in convcheck (u_out is twice the half ulp the output rounding can cost).  The simulated kernels of
# tests/test_gemmcheck_cpu.py reach 0.41 (1x1), 0.50 (GEMM), 0.60 / 0.46 (P / o at gain 30).

STORAGE = [("bf16", BF, False), ("f16", HF, False), ("f32", F32, False), ("split", F32, True)]
KC1 = {"bf16": 64, "f16": 64, "f32": 32, "split": 32}   # launch_typed of conv_mfma.hip: K-chunk of the TAPS = 1 tiles
# ds_conv_plan's three TAPS = 1 tiles as template arguments <T, TAPS, TH, TW, BN, WM, WN, KC, ...> of conv_mfma_kernel (launch_typed)
TILES = {"N64": "1,8,32,64,2,2,", "N32": "1,8,32,32,2,1,", "8X8": "1,8,8,64,1,1,"}


def plan_class(M, N):
    """ds_conv_plan for taps = 1 (the last lines of the function)"""
    if M >= 1024 or (M >= 256 and N >= 1024):
        return "N32" if N <= 32 else "N64"
    return "8X8"


def assert_kernel(name, cls, kind):
    """the launch ran conv_mfma_kernel in the expected TAPS = 1 tile with the storage type's chunk width and split flag"""
    assert name.startswith("conv_mfma_kernel<") and name.endswith(">"), name
    args = name[len("conv_mfma_kernel<"):-1].split(",")
    assert ",".join(args[1:7]) + "," == TILES[cls], f"{name}: not the {cls} tile"
    assert int(args[7]) == KC1[kind] and int(args[10]) == (1 if kind == "split" else 0), name
    assert args[0] == {"bf16": "bf16", "f16": "f16", "f32": "float", "split": "float"}[kind], name


def rnd(tag, shape, scale=1.0):
    return torch.from_numpy(synth.synth_noise(tag, shape)) * scale


def rup8(n):
    return (n + 7) // 8 * 8


# ------------------------------------------------------------------------------------------------ 1. exact integers
class ExactGemm:
    pass


def exact_gemm(tag, B, M, N, K, a_batched=True, bt_batched=True, bias_mode=None, div=None, res=False, out_scale=0.5):
    """a [B | 1, M, K], bt [B | 1, N, K], bias [N] | [M] | None, div [B] | None, res [B, M, rup8(N)] | None: float32 tensors on the
    CPU holding integers; ref [B, M, N] float64, the value before storage"""
    c = ExactGemm()
    dmax = max(div) if div is not None else 1.0
    unit = 16.0 * dmax / out_scale          # the left operand's step: the output is then a multiple of 16
    bunit = max(32.0, 16.0 / out_scale)     # bias and residual: multiples of 32 that stay multiples of 16 behind the scale
    assert unit == round(unit) and unit % 32 == 0 and bunit % 32 == 0
    if div is not None:
        assert all(math.log2(abs(d)) == round(math.log2(abs(d))) for d in div) and len(set(div)) == len(div) == B
    na, nb = (B if a_batched else 1), (B if bt_batched else 1)
    c.a = CC._ints(tag + ".a", (na, M, K), 0, 3) * unit
    c.bt = torch.stack([CC.sparse_signs(f"{tag}.bt{b}", N, K, min(32, K)) for b in range(nb)])
    if nb > 1:
        assert not torch.equal(c.bt[0], c.bt[1])
    c.bias = None if bias_mode is None else CC._ints(tag + ".bias", (M if bias_mode else N,), -2, 2) * bunit
    c.bias_mode = bias_mode or 0
    c.div = None if div is None else torch.tensor(div, dtype=torch.float32)
    ref = torch.einsum("bmk,bnk->bmn", c.a.double().expand(B, M, K), c.bt.double().expand(B, N, K))
    if div is not None:
        ref = ref / c.div.double()[:, None, None]
    if c.bias is not None:
        ref = ref + (c.bias.double()[None, :, None] if bias_mode else c.bias.double()[None, None, :])
    c.res = None
    if res:
        c.res = torch.zeros(B, M, rup8(N))
        c.res[..., :N] = CC._ints(tag + ".r", (B, M, N), -2, 2) * bunit
        ref = ref + c.res[..., :N].double()
    c.ref = (ref * out_scale)[:, None]  # [B, 1, M, N]: check_exact's NHWC
    c.B, c.M, c.N, c.CO, c.K, c.out_scale = B, M, N, N, K, out_scale
    CC.assert_representable(c.ref)
    return c


def check_exact_gemm(c, y, dt, what, sentinel=None):
    """torch.equal on columns [0, N); [N, rup8(N)) exactly zero; columns beyond keep the caller's sentinel (the contract stated at
    diffsep_gemm_nt and in conv_mfma.hip's epilogue: whole 8-column groups up to cout8 are stored, nothing else)"""
    n8 = rup8(c.N)
    CC.check_exact(c, y[:, None, :, :n8], None, dt, what)
    if y.shape[-1] > n8:
        assert sentinel is not None and bool((y[..., n8:].detach().cpu().float() == sentinel).all()), f"{what}: columns past {n8} written"


def pow2(n):
    return n & (n - 1) == 0


class ExactAttention:
    pass


def exact_attention(tag, B, L, C):
    """q, k, v [B, L, C], vt [B, C, Lp] (padding 100), pattern [B, L, L] (the exact probabilities), kinds [B, L] in "abc",
    o [B, L, C] float64: see the module docstring.  Every property is asserted here, on the float64 reference."""
    assert C in (64, 256)
    half, g, Lp = C // 2, math.sqrt(C), rup8(L)
    c = ExactAttention()
    q, k = torch.zeros(B, L, C), torch.zeros(B, L, C)
    pattern = torch.zeros(B, L, L, dtype=torch.float64)
    kinds = [["?"] * L for _ in range(B)]
    u = synth.uniform01(tag + ".u", B * half * (3 + L)).reshape(B, half, 3 + L)
    a = CC._ints(tag + ".ka", (B, L, half), -64, 64)
    S = torch.zeros(B, half, L)
    kind_of = []
    for b in range(B):
        kb = []
        for ch in range(half):
            kd = "abc"[(ch + b) % 3]
            if kd == "c" and not pow2(L):
                kd = "a"
            if kd == "b" and L < 2:
                kd = "a"
            lead = 64 + int(u[b, ch, 0] * 65)                          # 64 .. 128
            rest = np.floor(u[b, ch, 3:] * (lead + 1)) - 128              # -128 .. lead - 128
            j0 = int(u[b, ch, 1] * L)
            if kd == "c":
                S[b, ch] = float(int(u[b, ch, 0] * 257) - 128)
            else:
                S[b, ch] = torch.from_numpy(rest.astype(np.float32))
                S[b, ch, j0] = lead
                if kd == "b":
                    j1 = (j0 + 1 + int(u[b, ch, 2] * (L - 1))) % L
                    S[b, ch, j1] = lead
            kb.append(kd)
        kind_of.append(kb)
    k[:, :, :half] = a
    k[:, :, half:] = S.transpose(1, 2) - a
    for b in range(B):
        for i in range(L):
            ch = (i + 5 * b) % half
            q[b, i, ch] = g
            q[b, i, ch + half] = g
            kinds[b][i] = kind_of[b][ch]
    mult = float(L) if pow2(L) else 2.0
    v = CC._ints(tag + ".v", (B, L, C), 0, 3) * mult
    # ---- the properties, on the float64 reference
    s = torch.einsum("bic,bjc->bij", q.double(), k.double()) * C ** -0.5
    assert torch.equal(s, s.round()) and float(s.abs().max()) <= 256 and float(k.abs().max()) <= 256
    top = s.max(-1, keepdim=True).values
    lead = s == top
    gap = torch.where(lead, torch.full_like(s, float("inf")), top - s).min(-1).values
    for b in range(B):
        for i in range(L):
            n = int(lead[b, i].sum())
            kd = kinds[b][i]
            assert n == {"a": 1, "b": 2, "c": L}[kd], (b, i, kd, n)
            assert kd == "c" or float(gap[b, i]) >= 128
    pattern = lead.double() / lead.double().sum(-1, keepdim=True)
    p64 = torch.softmax(s, -1)
    assert float((p64 - pattern).abs().max()) < 1e-50
    # exp(-128) is exactly 0 in fp32 (and so in half): below half the smallest subnormal
    assert float(torch.tensor(-128.0).exp()) == 0.0 and math.exp(-128.0) < 2.0 ** -150
    o = torch.einsum("bij,bjc->bic", pattern, v.double())
    for dt in (BF, HF):
        assert torch.equal(o.float().to(dt).double(), o) and torch.equal(pattern.float().to(dt).double(), pattern)
        assert all(torch.equal(t.to(dt).float(), t) for t in (q, k, v))
    assert torch.equal(o, o.round()) and float(o.max()) <= 192
    vt = torch.full((B, C, Lp), 100.0)
    vt[:, :, :L] = v.transpose(1, 2)
    c.q, c.k, c.v, c.vt, c.pattern, c.kinds, c.o, c.scores = q, k, v, vt, pattern, kinds, o, s
    c.B, c.L, c.Lp, c.C = B, L, Lp, C
    return c


def check_exact_attention(c, o, scores, probs, dt, what):
    L = c.L
    oc, sc, pc = (t.detach().cpu().double() for t in (o, scores, probs))
    assert torch.equal(sc[..., :L], c.scores), f"{what}: {int((sc[..., :L] != c.scores).sum())} scores differ"
    bad = (pc[..., :L] != c.pattern).nonzero()
    assert len(bad) == 0, (f"{what}: {len(bad)} probabilities differ; first at (b, i, j) = {bad[0].tolist()}, row kind "
                           f"{c.kinds[int(bad[0][0])][int(bad[0][1])]}: kernel {float(pc[tuple(bad[0])])}, exact {float(c.pattern[tuple(bad[0])])}")
    assert not bool(pc[..., L:].any()), f"{what}: probability padding columns [L, Lp) not zero"
    bad = (oc != c.o).nonzero()
    assert len(bad) == 0, (f"{what}: {len(bad)} of {oc.numel()} outputs differ; first at (b, i, c) = {bad[0].tolist()}, row kind "
                           f"{c.kinds[int(bad[0][0])][int(bad[0][1])]}: kernel {float(oc[tuple(bad[0])])}, exact {float(c.o[tuple(bad[0])])}")


# ------------------------------------------------------------------------------------------------ 2. the per-element bound
class GemmCheck:
    """Reference and per-element bound of one ops.gemm_nt case on stored operands (see the module docstring); call it on the
    output [B, M, >= N]."""

    def __init__(self, a, bt, dt, B=None, bias=None, bias_mode=0, div=None, res=None, out_scale=1.0, split=False):
        a, bt = a.detach().cpu().double(), bt.detach().cpu().double()
        B = B or (a.shape[0] if a.dim() == 3 else bt.shape[0] if bt.dim() == 3 else 1)
        M, K = a.shape[-2:]
        N = bt.shape[-2]
        a, bt = a.expand(B, M, K), bt.expand(B, N, K)
        u = CC.ulp_of(dt)
        ref = torch.einsum("bmk,bnk->bmn", a, bt)
        A = torch.einsum("bmk,bnk->bmn", a.abs(), bt.abs())
        dv = torch.ones(B, dtype=torch.float64) if div is None else div.detach().cpu().double()
        assert float(dv.abs().max()) <= 4.0 and float(dv.abs().min()) >= 1.0 and K >= 8
        ref = ref / dv[:, None, None]
        A_all = A.clone()
        if bias is not None:
            bd = bias.detach().cpu().double()
            bd = bd[None, :, None] if bias_mode else bd[None, None, :]
            ref, A_all = ref + bd, A_all + bd.abs()
        if res is not None:
            rd = res.detach().cpu().double()[..., :N]
            ref, A_all = ref + rd, A_all + rd.abs()
        self.ref = ref * out_scale
        inner = (K + 6) * 2.0 ** -23 * A_all + (2.0 ** -16 * A if split else 0.0)
        self.bound = abs(out_scale) * inner / dv.abs()[:, None, None] + u * self.ref.abs() + (2.0 ** -24 if dt == HF else 0.0)
        self.N = N

    def __call__(self, y, what):
        return CC.assert_elementwise(y[..., :self.N], self.ref, self.bound, what)


EXP_ULP = 2.0 * sdecheck.ULP["expf"]   # in units of 2^-24
RCP_ULP = 2.0 * sdecheck.ULP["expf"]   # the reciprocal under the same 2-ulp assumption


class AttnCheck:
    """float64 reference and per-element bounds of scores, probabilities and output of ops.attention on stored q, k, v [B, L, C]"""

    def __init__(self, q, k, v, dt, split=False):
        q, k, v = (t.detach().cpu().double() for t in (q, k, v))
        B, L, C = q.shape
        Lp, u = rup8(L), CC.ulp_of(dt)
        e24 = 2.0 ** -24
        sc = C ** -0.5
        s = torch.einsum("bic,bjc->bij", q, k) * sc
        As = torch.einsum("bic,bjc->bij", q.abs(), k.abs()) * sc
        acc = (C + 6) * 2.0 ** -23 * As + (2.0 ** -16 * As if split else 0.0)
        Dj = acc + 0.5 * u * (s.abs() + acc) + (e24 if dt == HF else 0.0)
        self.s, self.s_bound = s, Dj
        D = Dj.max(-1, keepdim=True).values
        p = torch.softmax(s, -1)
        x = (s.max(-1, keepdim=True).values - s) + 2.0 * D       # |argument of the exponential|, of the stored scores
        E = ((2.5 * x + EXP_ULP) if dt != F32 else (x + EXP_ULP)) * e24   # (exp_t<float>: expf on the fp32 difference)
        nsum = math.ceil(L / 64) + 6
        fp = E + (p * E).sum(-1, keepdim=True) + (nsum + RCP_ULP + 1) * e24
        R = torch.exp(2.0 * D) * (1.0 + fp) * (1.0 + 0.5 * u) - 1.0
        self.p, self.R = p, R
        abs_p = e24 if dt == HF else 2.0 ** -120
        self.p_bound = p * R + abs_p
        o = torch.einsum("bij,bjc->bic", p, v)
        Ao = torch.einsum("bij,bjc->bic", p, v.abs())
        din = torch.einsum("bij,bjc->bic", self.p_bound, v.abs())
        Rmax = R.max(-1).values[..., None]
        self.o = o
        self.o_bound = din + (Lp + 6) * 2.0 ** -23 * Ao * (1.0 + Rmax) + (2.0 ** -16 * Ao if split else 0.0) + u * o.abs() + \
            (e24 if dt == HF else 0.0)
        self.L = L

    def __call__(self, o, probs, what):
        """(worst err / bound of the output, of the probabilities); the probability padding columns must be exact zeros"""
        pc = probs.detach().cpu()
        assert not bool(pc[..., self.L:].any()), f"{what}: probability padding columns [L, Lp) not zero"
        rp = CC.assert_elementwise(pc[..., :self.L], self.p, self.p_bound, what + " P")
        ro = CC.assert_elementwise(o, self.o, self.o_bound, what + " o")
        return ro, rp
