"""GPU parity of the register-weight 3x3 kernel (conv3x3_rw.hip: 64 / cat(64, 64) -> 64 couts at >= 32-row images, bf16)
through the C-ABI against torch fp32 on the CPU (same bf16-rounded operands) and, for whole residual blocks with the
folded 1x1 skip, against the CPU oracle.  Tolerance: 4e-3 relative RMS per convolution (bf16 storage of the activated
input and of the output), 1.5e-2 per residual block.

Next to the relative-RMS gates stand the two instruments of tests/convcheck.py.  (1) Exact integers (test_rw_exact_integers):
torch.equal on the output and the int64 statistics, raw launches in both weight layouts and GroupNorm + SiLU launches with a
residual; sees any wrong tap, halo, seam, tile share or statistic on a single element, cannot see rounding or the SiLU at ordinary
arguments; activated launches WITHOUT a residual or skip fold -1 / ln 2 into the staged value and cannot be bit exact; the folded
1x1 skip on 64 / 128 / 192 raw channels runs through the kernel's unit entry (test_rw_exact_integers_folded_skip).  (2) The per-element bound (ConvCheck in both
matches-torch tests, test_rw_activation_probe): every output element within its own derived rounding budget of a float64
reference; sees a local fault of more than about one storage ulp of the summed inputs, cannot see less than that."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import convcheck as CC
import diffsep_oracle as O
from diffsep_amd import ops, synth

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


@pytest.fixture(autouse=True, scope="module")
def _every_eligible_launch_on_the_rw_kernel():
    """The dispatch keeps small images (64-channel launches at <= 128^2, 128-cout launches with fewer tiles than CUs) on
    the weight-stationary / generic kernels (faster there); this module tests the register-weight kernel on them too."""
    from diffsep_amd import _lib
    libs = [_lib.lib(k) for k in ("bf16", "f16")]
    for l in libs:
        _lib.check(l.diffsep_set_option(b"rw_small", 1), l)
    yield
    for l in libs:
        _lib.check(l.diffsep_set_option(b"rw_small", 0), l)
DEV = "cuda"
DT = torch.bfloat16


def rel_rms(a, b):
    a = a.detach().double().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, np.float64)
    b = b.detach().double().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b, np.float64)
    return float(np.sqrt(np.mean((a - b) ** 2)) / (np.sqrt(np.mean(b ** 2)) + 1e-30))


def rnd(tag, shape, scale=1.0):
    return torch.from_numpy(synth.synth_noise(tag, shape)) * scale


# (B, H, W): one tile per block, several tiles per block (B >= 64 on 256 CUs), 8-row tiles (H % 16 != 0), wide images
SHAPES = [(2, 32, 32), (3, 64, 96), (64, 64, 64), (256, 32, 64), (2, 40, 64), (130, 24 + 16, 32), (1, 128, 256)]


@pytest.mark.parametrize("B,H,W", SHAPES)
@pytest.mark.parametrize("C1,C2", [(64, 0), (64, 64), (128, 0)])
@pytest.mark.parametrize("act", [1, None])
def test_rw_conv3x3_matches_torch(B, H, W, C1, C2, act):
    if B * H * W * (C1 + C2) > 40e6 and act is None:
        pytest.skip("large case covered with the activation")
    C = C1 + C2
    a = (rnd(f"rw.a{B}{H}{C1}", (B, H, W, C1), 1.2) + 0.1).to(DEV, DT)
    bt = (rnd(f"rw.b{B}{H}{C2}", (B, H, W, C2), 0.9) - 0.2).to(DEV, DT) if C2 else None
    w = rnd(f"rw.w{C}", (64, C, 3, 3), 1.0 / math.sqrt(9 * C))
    bias, bb = rnd("rw.bias", (64,), 0.1).to(DEV), rnd(f"rw.bb{B}", (B, 64), 0.1).to(DEV)
    # (a residual rides through the kernel as identity-weight skip chunks; no 128-channel layer of the network has one)
    res = rnd(f"rw.r{B}{H}", (B, H, W, 64)).to(DEV, DT) if C == 64 else None
    sc = (1.0 + rnd(f"rw.sc{B}{C}", (B, C), 0.2)).to(DEV)
    sh = rnd(f"rw.sh{B}{C}", (B, C), 0.2).to(DEV)
    xf = torch.cat([a.float(), bt.float()], -1) if C2 else a.float()
    if act is not None:
        xf = F.silu(xf * sc[:, None, None, :] + sh[:, None, None, :]).to(DT).float()
    wq = w.to(DT).float()
    ref = F.conv2d(xf.cpu().permute(0, 3, 1, 2), wq, bias.cpu(), padding=1).permute(0, 2, 3, 1)
    ref = (ref + bb.cpu()[:, None, None, :] + (res.float().cpu() if res is not None else 0.0)) * 0.70710678
    chk = CC.ConvCheck((a, bt), None if act is None else (sc, sh, 1), w, DT, bias=bias, bb=bb, res=res, out_scale=0.70710678)
    for chunk in (0, ops.conv2d_chunk(3, DT)):
        wp = ops.pack_conv_weight(w, DT, chunk=chunk).to(DEV) if chunk else ops.pack_conv_weight(w, DT).to(DEV)
        y, st = ops.conv2d_fused(a, wp, bias, 64, 3, x2=bt, gn=None if act is None else (sc, sh), gn_act=act or 0,
                                 bias_b=bb, res=res, out_scale=0.70710678, stats=True, w_chunk=chunk)
        assert rel_rms(y.float(), ref) < 4e-3
        chk(y, f"rw {C1}+{C2}->64 {B}x{H}x{W} act {act} chunk {chunk}")
        s = ops.stats_to_float(st)
        assert torch.allclose(s[..., 0].cpu(), ref.double().sum((1, 2)), rtol=2e-3, atol=2e-3 * H * W)
        assert torch.allclose(s[..., 1].cpu(), (ref.double() ** 2).sum((1, 2)), rtol=2e-3, atol=2e-3 * H * W)
    # plain launch: no bias / residual / statistics / GroupNorm
    y2 = ops.conv2d_fused(a, ops.pack_conv_weight(w, DT).to(DEV), None, 64, 3, x2=bt)
    xr = torch.cat([a.float(), bt.float()], -1) if C2 else a.float()
    ref2 = F.conv2d(xr.cpu().permute(0, 3, 1, 2), wq, None, padding=1).permute(0, 2, 3, 1)
    assert rel_rms(y2.float(), ref2) < 4e-3
    CC.ConvCheck((a, bt), None, w, DT)(y2, f"rw {C1}+{C2}->64 {B}x{H}x{W} plain")


# ---- 128 -> 128 couts: 4 cout groups on one 4 x 32 pixel group (tiles of 4 rows), skip / residual fragments in LDS
@pytest.mark.parametrize("B,H,W", [(2, 32, 32), (3, 64, 96), (16, 64, 64), (2, 40, 64), (1, 128, 256), (130, 32, 32)])
@pytest.mark.parametrize("C1,C2", [(128, 0), (64, 64)])
@pytest.mark.parametrize("extra", ["none", "res"])  # (the folded skips: test_rw128_resblock_vs_oracle)
def test_rw128_conv3x3_matches_torch(B, H, W, C1, C2, extra):
    C, CO = C1 + C2, 128
    if extra != "none" and (B, H, W) in ((1, 128, 256), (130, 32, 32)) and C2:
        pytest.skip("covered by the single-tensor input")
    a = (rnd(f"rw8.a{B}{H}{C1}", (B, H, W, C1), 1.2) + 0.1).to(DEV, DT)
    bt = (rnd(f"rw8.b{B}{H}{C2}", (B, H, W, C2), 0.9) - 0.2).to(DEV, DT) if C2 else None
    w = rnd(f"rw8.w{C}", (CO, C, 3, 3), 1.0 / math.sqrt(9 * C))
    bias, bb = rnd("rw8.bias", (CO,), 0.1).to(DEV), rnd(f"rw8.bb{B}", (B, CO), 0.1).to(DEV)
    sc = (1.0 + rnd(f"rw8.sc{B}{C}", (B, C), 0.2)).to(DEV)
    sh = rnd(f"rw8.sh{B}{C}", (B, C), 0.2).to(DEV)
    xf = torch.cat([a.float(), bt.float()], -1) if C2 else a.float()
    xa = F.silu(xf * sc[:, None, None, :] + sh[:, None, None, :]).to(DT).float()
    wq = w.to(DT).float()
    ref = F.conv2d(xa.cpu().permute(0, 3, 1, 2), wq, bias.cpu(), padding=1).permute(0, 2, 3, 1) + bb.cpu()[:, None, None, :]
    kw = {}
    if extra == "res":
        res = rnd(f"rw8.r{B}{H}", (B, H, W, CO)).to(DEV, DT)
        ref = ref + res.float().cpu()
        kw = dict(res=res)
    ref = ref * 0.70710678
    chk = CC.ConvCheck((a, bt), (sc, sh, 1), w, DT, bias=bias, bb=bb, res=kw.get("res"), out_scale=0.70710678)
    for chunk in (0, ops.conv2d_chunk(3, DT)):
        wp = ops.pack_conv_weight(w, DT, chunk=chunk).to(DEV) if chunk else ops.pack_conv_weight(w, DT).to(DEV)
        y, st = ops.conv2d_fused(a, wp, bias, CO, 3, x2=bt, gn=(sc, sh), gn_act=1, bias_b=bb, out_scale=0.70710678, stats=True,
                                 w_chunk=chunk, **kw)
        assert rel_rms(y.float(), ref) < 4e-3
        chk(y, f"rw128 {C1}+{C2} {B}x{H}x{W} {extra} chunk {chunk}")
        s = ops.stats_to_float(st)
        assert torch.allclose(s[..., 0].cpu(), ref.double().sum((1, 2)), rtol=2e-3, atol=2e-3 * H * W)
        assert torch.allclose(s[..., 1].cpu(), (ref.double() ** 2).sum((1, 2)), rtol=2e-3, atol=2e-3 * H * W)
    if extra == "none":  # raw input (the launch behind a FIR resampling kernel): no GroupNorm, no bias, no statistics
        y2 = ops.conv2d_fused(a, ops.pack_conv_weight(w, DT).to(DEV), None, CO, 3, x2=bt)
        ref2 = F.conv2d(xf.cpu().permute(0, 3, 1, 2), wq, None, padding=1).permute(0, 2, 3, 1)
        assert rel_rms(y2.float(), ref2) < 4e-3
        CC.ConvCheck((a, bt), None, w, DT)(y2, f"rw128 {C1}+{C2} {B}x{H}x{W} raw")


# ---- exact integers (tests/convcheck.py): bit for bit on the output and on the statistics
# (C1, C2, Cout, tile rows, multi-tile image); tile rows = (4 / NCG) * RPW of the instantiation ds_launch_conv_rw picks (RPW = 4
# always: 8 rows at 64 couts, 4 rows at 128), asserted below from the name of the kernel that ran
RW_EXACT = [(64, 0, 64, 8, (64, 96)), (64, 64, 64, 8, (64, 96)), (128, 0, 128, 4, (32, 32))]


@pytest.mark.parametrize("shape", [(2, 32, 32), (2, 40, 64), (3, 64, 96), "multi"], ids=str)
@pytest.mark.parametrize("C1,C2,CO,th,mimg", RW_EXACT)
def test_rw_exact_integers(C1, C2, CO, th, mimg, shape):
    """raw launches (both weight layouts) and, where the kernel takes a residual, GroupNorm + SiLU + residual launches on integer
    data: torch.equal on y and on both accumulators.  "multi": the smallest batch at which one block of an image gets two tiles
    and another one (from the tile size and the device's compute-unit count)."""
    if shape == "multi":
        H, W = mimg
        B = CC.multi_tile_batch(H, W, th, 32, CC.device_cus())
        print(f"\n[rw exact {C1}+{C2}->{CO}] multi-tile batch B = {B} at {H} x {W} on {CC.device_cus()} compute units")
        if B * H * W * CO > 2e7:
            pytest.skip(f"multi-tile batch B = {B}: more than 2e7 output elements")
    else:
        B, H, W = shape
    modes = [("raw", False)] + ([("silu", True)] if (C1 + C2 == 64 or CO == 128) else [])
    for mode, with_res in modes:
        c = CC.exact_case(f"rwx{C1}{C2}{CO}{B}{H}{W}{mode}", B, H, W, C1, C2, CO, mode, res=with_res, big=B > 8)
        a, bt = c.a.to(DEV, DT), (c.b.to(DEV, DT) if C2 else None)
        gn = None if mode == "raw" else (c.sc.to(DEV), c.sh.to(DEV))
        res = c.res.to(DEV, DT) if with_res else None
        for chunk in (0, ops.conv2d_chunk(3, DT)):
            wp = ops.pack_conv_weight(c.w, DT, chunk=chunk).to(DEV)
            y, st = ops.conv2d_fused(a, wp, c.bias.to(DEV), CO, 3, x2=bt, gn=gn, gn_act=1 if gn else 0, bias_b=c.bb.to(DEV), res=res,
                                     out_scale=0.5, stats=True, w_chunk=chunk)
            name = ops.last_conv_kernel()
            assert name.startswith("conv3x3_rw_kernel<"), name
            if shape == "multi":  # the tile height the batch was worked out from is the one that ran: <NCH,RPW,NSK,MODE,NCG>,
                t = name[name.index("<") + 1:-1].split(",")  # rows = (4 / NCG) * RPW (RwGeom in conv3x3_rw.hip)
                assert (4 // int(t[4])) * int(t[1]) == th, name
            CC.check_exact(c, y, st, DT, f"rw {C1}+{C2}->{CO} {B}x{H}x{W} {mode} chunk {chunk}")


# the folded 1x1 skip (raw channels through the centre tap; NSK = 1, 2, 3 skip chunks with real weights) through the kernel's
# unit entry: (Cin, Cout, skip channels (first, second))
RW_SKIP = [(64, 64, (64, 0)), (64, 64, (64, 64)), (64, 64, (64, 128)), (128, 128, (128, 0)), (128, 128, (64, 64))]


@pytest.mark.parametrize("B,H,W", [(2, 32, 32), (2, 40, 64)])
@pytest.mark.parametrize("C,CO,skip", RW_SKIP)
def test_rw_exact_integers_folded_skip(C, CO, skip, B, H, W):
    """GroupNorm + SiLU launch with a folded skip on 64 / 128 / 192 raw channels (one tensor or the concat of two), both weight
    layouts: torch.equal on y and on both accumulators; the skip keeps the staged value silu(v) itself"""
    c = CC.exact_case(f"rwk{C}{CO}{skip}{B}{H}{W}", B, H, W, C, 0, CO, "silu", skip=skip)
    a = c.a.to(DEV, DT)
    sa, sb, sw = c.skip
    sk = (sa.to(DEV, DT), sb.to(DEV, DT) if sb is not None else None, sw.reshape(CO, -1).to(DEV, DT).contiguous())
    for chunk in (0, ops.conv2d_chunk(3, DT)):
        wp = ops.pack_conv_weight(c.w, DT, chunk=chunk).to(DEV)
        y, st = ops.conv3x3_regweight(a, wp, CO, gn=(c.sc.to(DEV), c.sh.to(DEV)), bias=c.bias.to(DEV), bias_b=c.bb.to(DEV), skip=sk,
                                      out_scale=0.5, stats=True, w_chunk=chunk)
        name = ops.last_conv_kernel()
        assert name.startswith("conv3x3_rw_kernel<") and name.split(",")[2] == str(sum(skip) // 64), name
        CC.check_exact(c, y, st, DT, f"{name} skip {skip} {B}x{H}x{W} chunk {chunk}")


@pytest.mark.parametrize("C,CO,with_res", [(64, 64, True), (64, 64, False), (128, 128, True)])
def test_rw_activation_probe(C, CO, with_res):
    """one-hot weights: the kernel outputs its activated input; arguments over [-12, 12] and near zero against the input-error
    model of the bound (u_in, d_abs).  With a (zero) residual the staged value is silu(v) itself and the output is exactly it;
    without, the folded factor adds the output rounding."""
    B, H, W = 2, 32, 32
    x, sc, sh, w = CC.probe_inputs(f"rwp{C}", B, H, W, C)
    a = x.to(DEV, DT)
    res = torch.zeros(B, H, W, CO).to(DEV, DT) if with_res else None
    y = ops.conv2d_fused(a, ops.pack_conv_weight(w, DT).to(DEV), None, CO, 3, gn=(sc.to(DEV), sh.to(DEV)), gn_act=1, res=res)
    assert ops.last_conv_kernel().startswith("conv3x3_rw_kernel<")
    CC.ConvCheck((a, None), (sc, sh, 1), w, DT, exact_out=with_res)(y, f"rw probe {C} residual {with_res}")


def test_rw_conv3x3_zero_padding_is_exact():
    # an all-ones image through GroupNorm + SiLU with shift: every border pixel must see ZERO padding (not silu(shift))
    B, H, W, C = 2, 32, 64, 64
    x = torch.ones((B, H, W, C)).to(DEV, DT)
    w = torch.ones((64, C, 3, 3)) / 64.0
    sc, sh = torch.ones((B, C)).to(DEV), torch.full((B, C), 0.5).to(DEV)
    y = ops.conv2d_fused(x, ops.pack_conv_weight(w, DT).to(DEV), None, 64, 3, gn=(sc, sh), gn_act=1)
    v = float(F.silu(torch.tensor(1.5)).to(DT))
    cnt = F.conv2d(torch.ones(1, 1, H, W), torch.ones(1, 1, 3, 3), padding=1)[0, 0]  # taps inside the image: 4 / 6 / 9
    ref = (cnt * v)[None, :, :, None].expand(B, H, W, 64)
    assert rel_rms(y.float(), ref) < 4e-3  # (one bf16 rounding of the output)
    assert float((y.float().cpu() - ref).abs().max()) < 0.05


@pytest.mark.parametrize("dt,kind", [(torch.bfloat16, "bf16"), (torch.float16, "f16")])
def test_rw_refuses_one_kilobyte_output_pitch(dt, kind):
    """The kernel marks "no tile" with the constant pixel index 0x3fffff, which is safe only while every pixel pitch stays under
    1 KB (halo_addressing_ok in conv3x3_halo.h): at cout_pad = 512 (a 1024-byte output pitch) the epilogue of the "previous tile"
    of a block's first tile would store INTO the image.  So the launch must not reach the kernel: under rw_small (a) another
    kernel runs, (b) the lanes 64 .. 511 of every pixel keep the marker they were prefilled with, (c) lanes 0 .. 63 equal, bit for
    bit, the same call with rw_small off, which runs the same fallback kernel.  The dense launch of the same shape still runs on
    conv3x3_rw_kernel<1,4,0,0,2>: the refusal is the pitch and nothing else."""
    from diffsep_amd import _lib
    L = _lib.lib(kind)
    B, H, W, C, MARK = 2, 32, 32, 64, 3.0
    x = rnd("rwpitch.x", (B, H, W, C)).to(DEV, dt)
    wp = ops.pack_conv_weight(rnd("rwpitch.w", (64, C, 3, 3), 1.0 / math.sqrt(9 * C)), dt).to(DEV)
    try:
        _lib.check(L.diffsep_set_option(b"rw_small", 1), L)
        ops.conv2d_fused(x, wp, None, 64, 3, gn_act=0)
        assert ops.last_conv_kernel(kind) == "conv3x3_rw_kernel<1,4,0,0,2>"
        y_on = torch.full((B, H, W, 512), MARK, dtype=dt, device=DEV)
        ops.conv2d_fused(x, wp, None, 64, 3, gn_act=0, cout_pad=512, out=y_on)
        name_on = ops.last_conv_kernel(kind)
        _lib.check(L.diffsep_set_option(b"rw_small", 0), L)
        y_off = torch.full((B, H, W, 512), MARK, dtype=dt, device=DEV)
        ops.conv2d_fused(x, wp, None, 64, 3, gn_act=0, cout_pad=512, out=y_off)
        name_off = ops.last_conv_kernel(kind)
    finally:
        _lib.check(L.diffsep_set_option(b"rw_small", 1), L)  # (this module's setting: the fixture at the top)
    assert not name_on.startswith("conv3x3_rw_kernel"), name_on
    assert name_on == name_off
    assert bool((y_on[..., 64:] == MARK).all()), "lanes past Cout were written"
    assert torch.equal(y_on[..., :64], y_off[..., :64])
    assert bool(y_on[..., :64].float().abs().max() > 0)


@pytest.mark.parametrize("C1,C2", [(64, 0), (64, 64)])
def test_rw_conv3x3_groupnorm_from_producer_accumulators(C1, C2):
    B, H, W = 3, 32, 64
    C = C1 + C2
    groups = min(C // 4, 32)
    g, be = (1.0 + rnd(f"rwa.g{C}", (C,), 0.2)).to(DEV), rnd(f"rwa.be{C}", (C,), 0.1).to(DEV)

    def produce(tag, Cp):
        xi = rnd(f"rwa.x{tag}{Cp}", (B, H, W, 16)).to(DEV, DT)
        wi = ops.pack_conv_weight(rnd(f"rwa.w{tag}{Cp}", (Cp, 16, 3, 3), 1.0 / 12.0), DT).to(DEV)
        return ops.conv2d_fused(xi, wi, rnd(f"rwa.b{tag}{Cp}", (Cp,), 0.3).to(DEV), Cp, 3, stats=True)

    a, sa = produce("a", C1)
    (bt, sb) = produce("b", C2) if C2 else (None, None)
    w = rnd(f"rwa.w{C}", (64, C, 3, 3), 1.0 / math.sqrt(9 * C))
    wp = ops.pack_conv_weight(w, DT).to(DEV)
    y = ops.conv2d_fused(a, wp, None, 64, 3, x2=bt, gn_acc=(sa, sb, g, be, groups), gn_act=1)
    # reference on the CPU in fp32 (torch CPU ops, not MIOpen on the GPU), on the same 16-bit-rounded operands
    xcat = (torch.cat([a.float(), bt.float()], -1) if C2 else a.float()).cpu()
    hn = F.silu(F.group_norm(xcat.permute(0, 3, 1, 2), groups, g.cpu(), be.cpu(), eps=1e-6)).to(DT).float()
    ref = F.conv2d(hn, w.to(DT).float(), None, padding=1).permute(0, 2, 3, 1)
    assert rel_rms(y.float(), ref) < 1e-2


RB = [("GroupNorm_0.weight", "cin"), ("GroupNorm_0.bias", "cin"), ("Conv_0.weight", "w0"), ("Conv_0.bias", "cout"),
      ("Dense_0.weight", "d"), ("Dense_0.bias", "cout"), ("GroupNorm_1.weight", "cout"), ("GroupNorm_1.bias", "cout"),
      ("Conv_1.weight", "w1"), ("Conv_1.bias", "cout"), ("Conv_2.weight", "w2"), ("Conv_2.bias", "cout")]


@pytest.mark.parametrize("cin,B,H,W,up,down", [(128, 3, 32, 64, False, False), (64, 2, 64, 32, False, False),
                                               (128, 2, 32, 32, True, False), (128, 2, 64, 128, False, True), (256, 2, 32, 64, False, False)])
def test_rw128_resblock_vs_oracle(cin, B, H, W, up, down):
    # 128-cout residual blocks: plain (Conv_1 + residual), widening 64 -> 128 (Conv_1 + folded 64-channel skip), FIR up /
    # down (raw-input Conv_0, Conv_1 + folded 128-channel skip), 256 -> 128 (Conv_0 and the 256-channel skip stay on the
    # generic tile)
    cout = 128
    shp = dict(cin=(cin,), cout=(cout,), w0=(cout, cin, 3, 3), w1=(cout, cout, 3, 3), w2=(cout, cin, 1, 1), d=(cout, 64))
    tbl = [(n, shp[k]) for n, k in RB if not (n.startswith("Conv_2") and cin == cout and not up and not down)]
    sd = synth.synth_state_dict(tbl, 33)
    if "Conv_2.weight" in sd:
        sd["Conv_2.weight"] = (sd["Conv_2.weight"] * 3.0).astype(np.float32)
    x, temb = rnd(f"rw8rb.x{cin}{H}{W}{B}", (B, cin, H, W)), rnd("rw8rb.t", (B, 64))
    ref = O._res_block(O.to_torch(sd), "", x, temb, up=up, down=down)
    yb = ops.resblock_forward([sd[n] for n, _ in tbl], ops.to_nhwc(x).to(DT).to(DEV), temb.to(DEV), cout, up=up, down=down)
    assert rel_rms(ops.to_nchw(yb).float(), ref) < 1.5e-2


@pytest.mark.parametrize("cin,B,H,W,up,down", [(128, 3, 32, 64, False, False), (128, 2, 40, 32, False, False),
                                               (64, 3, 32, 32, True, False), (64, 2, 64, 128, False, True),
                                               (128, 70, 64, 64, False, False), (64, 2, 24, 32, True, False),
                                               (192, 2, 32, 64, False, False), (192, 33, 32, 32, False, False)])
def test_rw_resblock_with_folded_skip_vs_oracle(cin, B, H, W, up, down):
    # 64-cout residual blocks whose Conv_0 (cat(64, 64) -> 64, GroupNorm + SiLU on the concat) and Conv_1 + folded Conv_2
    # (64, 128 or — the cat(64, 128) block of the 128^2 up path — 192 raw channels through the centre tap) run on the
    # register-weight kernel: 16-row and 8-row tiles, one and
    # several tiles per block, FIR up / down in front (raw-input mode of Conv_0)
    cout = 64
    shp = dict(cin=(cin,), cout=(cout,), w0=(cout, cin, 3, 3), w1=(cout, cout, 3, 3), w2=(cout, cin, 1, 1), d=(cout, 64))
    tbl = [(n, shp[k]) for n, k in RB]
    sd = synth.synth_state_dict(tbl, 31)
    sd["Conv_2.weight"] = (sd["Conv_2.weight"] * 3.0).astype(np.float32)  # a wrong skip product cannot hide
    x, temb = rnd(f"rwrb.x{cin}{H}{W}{B}", (B, cin, H, W)), rnd("rwrb.t", (B, 64))
    ref = O._res_block(O.to_torch(sd), "", x, temb, up=up, down=down)
    yb = ops.resblock_forward([sd[n] for n, _ in tbl], ops.to_nhwc(x).to(DT).to(DEV), temb.to(DEV), cout, up=up, down=down)
    assert rel_rms(ops.to_nchw(yb).float(), ref) < 1.5e-2
