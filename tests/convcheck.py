"""Two instruments for the 3x3 convolution kernels, both against a CPU reference of the same operation, and what each can see.
(tests/gemmcheck.py carries both to the 1x1 / GEMM instantiations of conv_mfma.hip and the unfused attention chain, on these pieces.)

1. EXACT INTEGERS (exact_case / check_exact): bit for bit, no tolerance.  x holds integers 0..3 (times 32 in a raw launch, through
   the affine 32 x + 32 otherwise), weights are -1 / 0 / +1 with exactly 32 non-zero (tap, cin) positions per output channel, every
   bias, residual and skip input is a multiple of 32, skip weights have 8 non-zero positions per output channel, out_scale = 0.5.
   Every product, every partial sum in any order, the output (a multiple of 16, at most 255 * 16) and both statistics are then
   exact in fp32, bfloat16 and half alike (assert_representable states the conditions ON THE REFERENCE before anything is
   compared), so torch.equal must hold on y and on the int64 accumulators.  SiLU is the identity on 32, 64, 96, 128 in fp32
   (1 + exp(-32) == 1) and in packed half precision (the exponential underflows), so the activated staging path has an exact
   test too — where the kernel stages silu(v) itself.  The register-weight and streamed kernels stage silu(v) / -ln 2 and leave
   the factor to the epilogue whenever no raw skip / residual chunk shares the accumulators (FOLD in conv3x3_rw / sw / sws.hip):
   such launches round a non-integer and cannot be bit exact by construction; their activated exact cases therefore carry a
   residual or a skip (rw: ops.conv3x3_regweight, the unit entry with the folded skip).  Both make NSK > 0: a folded 1x1 skip is sCin / KC raw chunks, and all three kernels carry a residual as
   Cout / KC identity-weight skip chunks (conv3x3_rw.hip: nsk = a.res ? a.Cout / KC; conv3x3_sw / sws.hip: res + ident_frag).
   Sees: a wrong tap, halo, seam, sample, channel block, tile share, padding, statistic, anywhere, on one element.  Cannot see: rounding behaviour (nothing rounds), the SiLU at ordinary arguments.

2. PER-ELEMENT BOUND (ConvCheck / assert_elementwise) on ordinary random data.  Reference in float64 from the STORED operands:
   h = round_dtype(silu64(x * sc + sh)), ref = out_scale * (conv(h, w) + bias + bias_b + res + skip).  Per element

       bound = out_scale * (u_in * A + d_abs * Wsum + K * 2^-23 * A_all) + u_out * |ref|
       A = conv(|h|, |w|),  A_all = A + |skip products| + |bias| + |bias_b| + |res|,  Wsum = conv(1, |w|) with zero padding
       u_in = u_out = 2^-7 (bfloat16) | 2^-10 (half, + 2^-24 absolute for subnormals) | 0 (float32)

   u_in: the kernel rounds its own fp32 silu, the reference rounds the float64 one; each is within half an ulp of its argument and
   the arguments differ by at most d_abs, so |dh| <= ulp(h) + d_abs <= u_in |h| (1 + u_in) + d_abs.  A raw launch has neither term.
   u_out: half a storage ulp is u_out / 2 |ref|; the other half covers the rounding of a value that is itself off by the rest.
   K = 9 Cin + skip channels + 6: one fp32 rounding of at most one ulp (2^-23; the MFMA's internal adds need not round to
   nearest) per accumulation step, bias / residual / scale / folded factor in the epilogue.  Doubled when the reference itself
   is computed in float32 (the largest cases).

   d_abs = 2^-16, on the domain |x sc| + |sh| <= 32 (asserted), from the instruction chain of gn8 / silu_t<bf16_t>
   (conv_device.h, common.h): v = x * sc + sh in one or two fp32 roundings, |dv| <= 2^-24 (|x sc| + |v|) <= 2^-18, times
   |silu'| <= 1.1; t = -v * log2(e) (one rounding + the constant's: 1.5 |t| 2^-24 absolute, i.e. 1.5 |v| 2^-24 relative on e);
   v_exp_f32 1 ulp, 1 + e one rounding, v_rcp_f32 1 ulp, the product one rounding: relative
   (sigma(-v) (1.5 |v| + 2) + 4) 2^-24 on silu, at most 130 * 2^-24 absolute for |v| <= 32.  With the folded factor two more
   roundings of the table entries (2^-24 * 32 * 1.1).  Sum 1.4e-5 < 2^-16.  silu_t<float> (accurate expf, IEEE division) is inside.

   Packed-half staging of the half-precision build (gn8<., true> in conv3x3_ws.hip; the rw / sw kernels): the table is rounded to
   half, the reference uses those stored entries, z = round_half(x a + b) carries 2^-11 |z| and the rest c(z) half-ulps of |h|:
       |dh| <= |z silu'(z)| 2^-11 + z^2 2^-23 + c(z) 2^-11 |h| + 2^-24
       c(z) = 4 + sigma(-z) (1.44 |z| + 2):  product with -log2(e) (one rounding + 0.44 for the constant 0xbdc5, together a
       relative 1.44 |z| 2^-11 on e), v_exp_f16 1 ulp = 2, 1 + e: 1, v_rcp_f16 1 ulp = 2, product: 1.
       folded (rw / sw without skip): the factor sits in the table, c(z) = 4 + 2 sigma(-z), the reference is silu of -ln 2 times
       the stored affine.  Below z = -11 the half-precision exponential overflows and the staged value is -0: |dh| <= |h|.
   Split mode (fp32 tensors as hi + lo bfloat16, 2^-17 per operand): u_in = u_out = 0 and 2^-16 * A per product.
   Plain fp32 (gn4 / silu_t<float> of the generic kernel: fmaf or two roundings, the accurate expf at 1 ulp, 1 + e one rounding,
   correctly rounded division): no storage rounding, so the chain's own error is the whole input term, per element
   |dh| <= 1.1 * 2^-24 (|x sc| + |v|) + (2 sigma(-v) + 2) * 2^-24 |silu(v)|  (the argument's rounding through
   |silu'| <= 1.1; expf's argument is exact, its result within 2^-23, the sum and the quotient 2^-24 each); 2^-16 would be
   a hundred times that.  The split kernel (conv3x3_sws.hip) stages through v_exp_f32 / v_rcp_f32 and keeps d_abs.

   Sees: any element off by more than its own rounding budget — a missing tap on one tile row, a halo from the wrong sample, one
   stale pixel (tests/test_convcheck_cpu.py shows all three pass the relative-RMS gates).  Cannot see: an error smaller than one
   storage ulp of the inputs it sums; that is what instrument 1 is for.

Worst err / bound measured on the MI355X (MEASURED below; printed by the tests, nothing above was fitted to them).  Activated
launches on random data sit at 0.12 .. 0.23 in bfloat16 (rw 0.23, rw 128 -> 128 0.17, ws 0.21, small 0.19, heads 0.19, wide tile
0.22, sw 0.14) and 0.05 .. 0.19 in half (sw packed 0.09, sw packed + folded 0.05, ws packed 0.09, generic 0.18); the simulated
kernel of tests/test_convcheck_cpu.py (one-ulp input flips on a quarter of the inputs) reaches 0.25 and the injected faults 11 ..
54, so a fault of the size shown there is caught on every family with a factor of at least four to spare.  Raw launches sit at
0.44 .. 0.50 whatever the kernel: they have no input term and u_out is twice the half ulp the output rounding can cost.  Near the
limit: the bfloat16 probes with a residual (0.59 .. 0.74: one-hot weights leave the input term alone, and a one-ulp flip of the
staged value is most of it), and the packed-half probes at 1.00 — the elements below z = -11, where the staged value is -0 and
the bound IS |h|; ConvCheck prints the worst ratio without them as well.  Slack: the split kernel (0.03 .. 0.05) and plain fp32
(0.03), where K, one ulp for each of 9 Cin accumulation steps in the worst order, is most of the bound: there the bound sees a
missing tap or a foreign halo (errors of the size of A / 9) but not a single wrong low-order bit.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from diffsep_amd import ops, synth

BF, HF, F32 = torch.bfloat16, torch.float16, torch.float32
D_ABS = 2.0 ** -16
DOMAIN = 32.0
LOG2E_F32 = float(np.float32(-1.4426950408889634))
LN2 = math.log(2.0)

# family -> worst err / bound of the per-element check on the MI355X (copied from the tests' output)
MEASURED = {
    "rw 64 / cat -> 64 activated": 0.226, "rw 64 / cat -> 64 raw": 0.476, "rw 128 -> 128 activated": 0.165, "rw 128 -> 128 raw": 0.442,
    "rw probe, residual / folded": (0.588, 0.492), "ws activated": 0.211, "ws affine": 0.175, "ws raw": 0.474, "ws probe bf16": 0.594,
    "ws probe f16 (packed half)": 1.000, "small activated": 0.187, "small raw": 0.455, "small head": 0.122, "small probe": 0.000,
    "pyramid head (thin out)": 0.191, "thin out probe": 0.000, "first layer (raw)": 0.497, "wide tile": 0.215, "generic probe": 0.000,
    "sw bf16 activated": 0.138, "sw bf16 raw": 0.473, "sw f16 packed": 0.089, "sw f16 packed + folded": 0.051, "sw f16 raw": 0.373,
    "streamed probe bf16, residual / folded": (0.738, 0.490), "streamed probe f16, residual / folded": (1.000, 0.998),
    "streamed probe split, residual / folded": (0.048, 0.049), "sws": 0.031, "split generic": 0.122, "fp32 generic": 0.029,
    "f16 build: ws / small / generic / first layer": (0.093, 0.060, 0.184, 0.481),
}


def rel_rms(a, b):
    a = a.detach().double().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, np.float64)
    b = b.detach().double().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b, np.float64)
    return float(np.sqrt(np.mean((a - b) ** 2)) / (np.sqrt(np.mean(b ** 2)) + 1e-30))


def ulp_of(dt):
    return {BF: 2.0 ** -7, HF: 2.0 ** -10, F32: 0.0}[dt]


def round_dt(t, dt):
    """float64 -> the storage format and back"""
    return t.double() if dt == F32 else t.float().to(dt).double()


def silu64(v):
    return v / (1.0 + torch.exp(-v))


def dsilu64(v):
    s = torch.sigmoid(v)
    return s * (1.0 + v * (1.0 - s))


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _conv(h, w, big):
    """3x3 (or 1x1) convolution of NHWC h with OIHW w, zero padding; float64, or float32 where `big`"""
    dt = torch.float32 if big else torch.float64
    return F.conv2d(_nchw(h).to(dt), w.to(dt), None, padding=w.shape[-1] // 2).permute(0, 2, 3, 1).double()


# ------------------------------------------------------------------------------------------------ 1. exact integers
def _ints(tag, shape, lo, hi):
    n = int(np.prod(shape))
    return torch.from_numpy(np.floor(synth.uniform01(tag, n) * (hi - lo + 1)).astype(np.float32) + lo).reshape(shape)


def sparse_signs(tag, cout, npos, nnz):
    """[cout, npos] of -1 / 0 / +1 with exactly nnz non-zero positions per row, every row different"""
    u = synth.uniform01(tag, cout * npos).reshape(cout, npos)
    idx = np.argsort(u, axis=1, kind="stable")[:, :nnz]
    sgn = np.where(synth.uniform01(tag + ".s", cout * nnz).reshape(cout, nnz) < 0.5, -1.0, 1.0).astype(np.float32)
    w = np.zeros((cout, npos), np.float32)
    np.put_along_axis(w, idx, sgn, axis=1)
    return torch.from_numpy(w)


class ExactCase:
    pass


def exact_case(tag, B, H, W, C1, C2, CO, mode, res=False, skip=None, cin_real=None, big=False, out_scale=0.5, with_bb=True, ksize=3):
    """mode "raw": x = 32 * ints, no table; "affine" / "silu": x = ints through scale 32, shift 32 (padding stays 0).
    Tensors are float32 on the CPU with integer values; ref [B,H,W,CO] is the value before storage.  out_scale = 1 and
    with_bb=False (c.bb None): the first-layer and pyramid-head kernels, which take neither a scale nor a per-sample bias.
    ksize = 1 (tests/gemmcheck.py): min(32, real input channels) non-zero weights per output channel."""
    assert mode in ("raw", "affine", "silu") and ksize in (1, 3)
    c = ExactCase()
    C = C1 + C2
    kk = ksize * ksize
    big = big or B * H * W * CO * C * 9 > 1e9  # (float32 on the CPU is exact on these numbers too: tests/test_convcheck_cpu.py)
    cr = cin_real or C
    xi = _ints(tag + ".x", (B, H, W, C), 0, 3)
    xi[..., cr:] = 0
    c.mode, c.C1, c.C2, c.CO, c.out_scale = mode, C1, C2, CO, out_scale
    x = xi * 32.0 if mode == "raw" else xi
    c.a, c.b = x[..., :C1].contiguous(), (x[..., C1:].contiguous() if C2 else None)
    c.sc, c.sh = torch.full((B, C), 32.0), torch.full((B, C), 32.0)
    h = x if mode == "raw" else xi * 32.0 + 32.0
    w = torch.zeros(CO, C, ksize, ksize)
    w[:, :cr] = sparse_signs(tag + ".w", CO, kk * cr, min(32, kk * cr)).reshape(CO, ksize, ksize, cr).permute(0, 3, 1, 2)
    c.w = w
    c.bias, c.bb = _ints(tag + ".bias", (CO,), -2, 2) * 32.0, _ints(tag + ".bb", (B, CO), -2, 2) * 32.0
    ref = _conv(h, w, big) + c.bias.double()
    if with_bb:
        ref = ref + c.bb.double()[:, None, None, :]
    else:
        c.bb = None
    c.res = None
    if res:
        c.res = _ints(tag + ".r", (B, H, W, CO), -2, 2) * 32.0
        ref = ref + c.res.double()
    c.skip = None
    if skip:
        s1, s2 = skip
        sx = _ints(tag + ".sx", (B, H, W, s1 + s2), 0, 3) * 32.0
        sw = sparse_signs(tag + ".sw", CO, s1 + s2, 8).reshape(CO, s1 + s2, 1, 1)
        c.skip = (sx[..., :s1].contiguous(), sx[..., s1:].contiguous() if s2 else None, sw)
        ref = ref + _conv(sx, sw, big)
    c.ref = ref * out_scale
    assert_representable(c.ref)
    if mode == "silu":
        v = torch.tensor([32.0, 64.0, 96.0, 128.0])
        assert torch.equal(F.silu(v), v), "the CPU's float32 SiLU is not the identity at 32, 64, 96, 128"
    return c


def assert_representable(ref):
    """the conditions under which every number of the exact cases is exact in fp32, bfloat16 and half (ref: float64)"""
    q = ref / 16.0
    assert torch.equal(q, q.round()) and float(q.abs().max()) <= 255.0, "output not a multiple of 16 within 255 * 16"
    assert float(ref.abs().sum((1, 2)).max()) < 2.0 ** 24 * 16, "a channel sum could round in fp32"
    assert float((ref * ref).sum((1, 2)).max()) / 256.0 < 2.0 ** 24, "a channel sum of squares could round in fp32"


def check_exact(c, y, st, dt, what):
    """torch.equal on the output and on both int64 accumulators (st None: a launch without statistics)"""
    yc = y.detach().cpu()
    want = c.ref.to(dt) if dt != F32 else c.ref.float()
    CO = c.CO
    if not torch.equal(yc[..., :CO], want):
        bad = (yc[..., :CO].double() != c.ref).nonzero()
        b, i, j, k = (int(v) for v in bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {want.numel()} output elements differ; first at (b, h, w, c) = ({b}, {i}, {j}, {k}): "
                             f"kernel {float(yc[b, i, j, k])}, reference {float(c.ref[b, i, j, k])}; samples {sorted(set(bad[:, 0].tolist()))[:8]}, "
                             f"rows {int(bad[:, 1].min())}..{int(bad[:, 1].max())}, columns {int(bad[:, 2].min())}..{int(bad[:, 2].max())}, "
                             f"channels {int(bad[:, 3].min())}..{int(bad[:, 3].max())}")
    if yc.shape[-1] > CO:
        assert not bool(yc[..., CO:].any()), f"{what}: padding channels written"
    if st is not None:
        s0 = (c.ref.sum((1, 2)) * ops.STAT_SUM_SCALE).to(torch.int64)
        s1 = ((c.ref * c.ref).sum((1, 2)) * ops.STAT_SQ_SCALE).to(torch.int64)
        sc = st.detach().cpu()
        assert torch.equal(sc[..., 0], s0), f"{what}: channel sums differ at (b, c) = {(sc[..., 0] != s0).nonzero()[:4].tolist()}"
        assert torch.equal(sc[..., 1], s1), f"{what}: sums of squares differ at (b, c) = {(sc[..., 1] != s1).nonzero()[:4].tolist()}"


def multi_tile_batch(H, W, th, tw, cus, blocks_per_cu=1, couts_blocks=1):
    """smallest B at which the persistent kernels (blocks per image = min(tiles, blocks_per_cu * (CUs // (B * couts_blocks))), at
    least 1) give one block two tiles and another one: blocks < tiles < 2 * blocks"""
    tiles = (H // th) * (W // tw)
    for B in range(1, 4 * cus):
        g = min(tiles, max(1, cus // (B * couts_blocks)) * blocks_per_cu)
        if g < tiles < 2 * g:
            return B
    raise AssertionError("no such batch")


def device_cus():
    from golden.gen_conv_routes import device_cus as cus  # (tests/golden: the one query of the compute-unit count)
    return cus()


# ------------------------------------------------------------------------------------------------ 2. the per-element bound
def assert_elementwise(y, ref, bound, what):
    """fails if any element of y is further from ref than its bound; prints the worst err / bound otherwise and returns it"""
    err = (y.detach().double().cpu() - ref).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    worst = float(ratio.max())
    if not worst <= 1.0:
        k = int(ratio.argmax())
        idx = tuple(int(v) for v in np.unravel_index(k, tuple(ratio.shape)))
        over = int((ratio > 1.0).sum())
        raise AssertionError(f"{what}: {over} elements over their bound; worst at (b, h, w, c) = {idx}: err {float(err[idx]):.4e}, "
                             f"bound {float(bound[idx]):.4e}, err / bound {worst:.2f}, reference {float(ref[idx]):.5f}")
    print(f"[convcheck {what}] worst err / bound {worst:.3f}")
    return worst


def packed_half_reference(x, sc, sh, fold):
    """(h, dh) float64 of the packed-half staging (see the module docstring); x [B,H,W,C] stored half values, sc / sh [B,C]"""
    x = x.double()
    if fold:
        a = (sc.float() * LOG2E_F32).to(HF).double()[:, None, None, :]
        b = (sh.float() * LOG2E_F32).to(HF).double()[:, None, None, :]
        z = -(x * a + b) * LN2   # (in units of the SiLU's argument)
    else:
        z = x * sc.float().to(HF).double()[:, None, None, :] + sh.float().to(HF).double()[:, None, None, :]
    h = silu64(z)
    sg = torch.sigmoid(-z)
    c = 4.0 + sg * (2.0 if fold else 1.44 * z.abs() + 2.0)
    dh = (z * dsilu64(z)).abs() * 2.0 ** -11 + z * z * 2.0 ** -23 + c * 2.0 ** -11 * h.abs() + 2.0 ** -24
    dh = torch.where(z < -11.0, h.abs() + 2.0 ** -24, dh)
    return h, dh


class ConvCheck:
    """Reference and per-element bound of one convolution case, computed once; call it on every output of the case.
    x: (a, b | None) stored tensors [B,H,W,C*]; gn: None (raw) or (sc, sh, act); w OIHW float32 (rounded to dt here, as
    pack_conv_weight / pack_frag_weight do); skip: (sa, sb | None, sw OIHW 1x1); dt: storage type, F32 with split=True for the
    split mode; packed: "pk" | "pk_fold" for the packed-half staging of the half-precision build; exact_out: the output is a stored
    value times one (the activation probe on a kernel that does not fold), no output rounding."""

    def __init__(self, x, gn, w, dt, bias=None, bb=None, res=None, skip=None, out_scale=1.0, split=False, packed=None,
                 exact_out=False, cout=None):
        a, b = x
        self.overflow = None
        xc = (torch.cat([a, b], -1) if b is not None else a).detach().cpu().double()
        B, H, W, C = xc.shape
        CO = w.shape[0]
        big = B * H * W * CO * C * w.shape[-1] ** 2 > 1e9
        wq = round_dt(w.double(), dt)
        if split:  # hi + lo bfloat16 of the fp32 weight: within 2^-17, inside the per-product term
            wq = w.double()
        u = ulp_of(dt)
        dh = None
        if gn is None:
            h = xc
        else:
            sc, sh, act = (t.detach().cpu() if isinstance(t, torch.Tensor) else t for t in gn)
            dom = (xc.abs() * sc.double().abs()[:, None, None, :] + sh.double().abs()[:, None, None, :]).max()
            assert float(dom) <= DOMAIN, f"|x sc| + |sh| = {float(dom)} leaves the domain of d_abs"
            if packed:
                assert dt == HF and act
                h, dh = packed_half_reference(xc, sc, sh, packed == "pk_fold")
                self.overflow = (dh >= h.abs()) & (h.abs() > 2.0 ** -20)  # (the z < -11 branch: staged -0, bound = |h|)
            else:
                xs = xc * sc.double()[:, None, None, :]
                v = xs + sh.double()[:, None, None, :]
                h = round_dt(silu64(v) if act else v, dt)
                if dt == F32 and not split:  # the accurate chain of gn4 / silu_t<float>
                    dh = 1.1 * 2.0 ** -24 * (xs.abs() + v.abs())
                    if act:
                        dh = dh + (2.0 * torch.sigmoid(-v) + 2.0) * 2.0 ** -24 * h.abs()
                else:
                    dh = u * (1.0 + u) * h.abs() + D_ABS
        ref = _conv(h, wq, big)
        aw = wq.abs()
        A = _conv(h.abs(), aw, big)
        A_all = A.clone()
        for t, shape in ((bias, (1, 1, 1, CO)), (bb, (B, 1, 1, CO)), (res, None)):
            if t is not None:
                td = t.detach().cpu().double()[..., :CO]
                td = td.reshape(shape) if shape else td
                ref = ref + td
                A_all = A_all + td.abs()
        n_skip = 0
        if skip is not None:
            sa, sb, sw = skip
            sx = (torch.cat([sa, sb], -1) if sb is not None else sa).detach().cpu().double()
            swq = round_dt(sw.double(), dt) if not split else sw.double()
            ref = ref + _conv(sx, swq, big)
            A_skip = _conv(sx.abs(), swq.abs(), big)
            A_all = A_all + A_skip
            n_skip = sx.shape[-1]
        else:
            A_skip = 0.0
        self.ref = ref * out_scale
        K = (w.shape[-1] ** 2 * C + n_skip + 6) * (2 if big else 1)  # (9 Cin for the 3x3 kernels, Cin for the 1x1 / GEMM route)
        inner = K * 2.0 ** -23 * A_all
        if dh is not None:
            inner = inner + _conv(dh, aw, big)
        if self.overflow is not None:  # outputs that sum such an input
            self.overflow = _conv(self.overflow.double(), aw, big) > 0
        if split:
            inner = inner + 2.0 ** -16 * (A + A_skip)
        bound = abs(out_scale) * inner
        if not exact_out:
            bound = bound + u * self.ref.abs() + (2.0 ** -24 if dt == HF else 0.0)
        self.bound = bound
        self.CO = CO if cout is None else cout
        self.worst = 0.0

    def __call__(self, y, what):
        r = assert_elementwise(y[..., :self.CO], self.ref[..., :self.CO], self.bound[..., :self.CO], what)
        if self.overflow is not None and bool(self.overflow.any()):  # where the bound is |h| by definition the ratio says nothing
            keep = ~self.overflow[..., :self.CO]
            e = (y[..., :self.CO].detach().double().cpu() - self.ref[..., :self.CO]).abs() / self.bound[..., :self.CO]
            print(f"[convcheck {what}, half-precision exp overflow excluded] worst err / bound {float(e[keep].max()):.3f}")
        self.worst = max(self.worst, r)
        return r


def probe_inputs(tag, B, H, W, C):
    """x [B,H,W,C], sc, sh [B,C] float32 with arguments x sc + sh over [-12, 12]; channels 0..7 run sc = 1, sh = 0 on
    arguments near zero (+- 2^-1 .. 2^-14 and 0), one-hot weights [C, C, 3, 3] (cout c reads cin c at the centre tap)"""
    n = B * H * W * C
    x = torch.from_numpy((synth.uniform01(tag + ".x", n) * 16.0 - 8.0).astype(np.float32)).reshape(B, H, W, C)
    sc = torch.from_numpy((synth.uniform01(tag + ".sc", B * C) * 0.5 + 0.75).astype(np.float32)).reshape(B, C)
    sh = torch.from_numpy((synth.uniform01(tag + ".sh", B * C) * 4.0 - 2.0).astype(np.float32)).reshape(B, C)
    sc[:, :8], sh[:, :8] = 1.0, 0.0
    e = torch.from_numpy(np.floor(synth.uniform01(tag + ".e", B * H * W * 8) * 16.0).astype(np.float32)).reshape(B, H, W, 8)
    sg = torch.where(x[..., :8] < 0, -1.0, 1.0)
    x[..., :8] = torch.where(e >= 15.0, torch.zeros_like(e), sg * torch.exp2(-e - 1.0))
    w = torch.zeros(C, C, 3, 3)
    w[torch.arange(C), torch.arange(C), 1, 1] = 1.0
    return x, sc, sh, w
