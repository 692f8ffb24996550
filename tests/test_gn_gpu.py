"""The GroupNorm-apply / FIR x2 resampling kernels of csrc/norm.hip, one kernel at a time, under the two instruments of
tests/gncheck.py: exact integer inputs (torch.equal on y, on xr and on the NaN-filled extra lanes of padded buffers) and the
per-element bound on random data, each with dense buffers and with leading dimensions C + (8, 16, 8).  Every case names its kernel:
a forced route of ops.gn_apply (the kernel's shape preconditions hold, only the dispatch's size thresholds are lifted) and
ops.last_conv_kernel() afterwards; one case per route lets the dispatch choose, on a shape just over the route's threshold, and
holds the name against the route query.  Shapes are the smallest with every edge the kernel distinguishes: odd sizes, one whole
strip / a ragged one / a single row left over, one and three column pairs, halo columns inside and outside the image, images
shorter than a strip, one and two 64-channel blocks.  The statistics pass (gn_stats_kernel + gn_finalize_kernel) runs on exact
integers against float64 from exact sums, under the rounding budget of its four fp32 operations."""
import pytest
import torch

import convcheck as CC
import gncheck as G
from diffsep_amd import ops, synth

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda"
BF, HF, F32 = G.BF, G.HF, G.F32
KIND = {BF: "bf16", HF: "f16", F32: "bf16"}  # the library ops.gn_apply runs a tensor type in
TN = {BF: "bf16", HF: "f16", F32: "f32"}
PADS = [(0, 0, 0), (8, 16, 8)]
WORST = {}


def _note(family, r):
    WORST[family] = max(WORST.get(family, 0.0), r)
    print(f"[gncheck family {family}] worst err / bound so far {WORST[family]:.3f}")


def _table(B, C, sc, sh):
    return torch.full((B, C), sc, device=DEV), torch.full((B, C), sh, device=DEV)


def run_exact(dt, mode, B, H, W, C, route, name, tables, pads=PADS, big=False):
    """exact inputs through one kernel: tables = [(scale, shift, act)] or None for the pyramid's pure FIR"""
    x = G.exact_inputs(f"gn{mode}{H}{W}{C}", B, H, W, C)
    xd = x.to(DEV, dt)
    for tab in (tables or [None]):
        ry, rx = G.exact_reference(x, tab[:2] if tab else None, mode, big=big)
        for pad in pads:
            sc, sh = _table(B, C, tab[0], tab[1]) if tab else (None, None)
            y, xr, yb, xrb = ops.gn_apply(xd, sc, sh, tab[2] if tab else 0, mode, want_y=tab is not None, want_xr=mode != 0,
                                          route=route, pad=pad)
            got = ops.last_conv_kernel(KIND[dt])
            assert got == name, f"{got} ran, {name} expected"
            what = f"{name} {TN[dt]} {B}x{H}x{W}x{C} table {tab} pad {pad}"
            if tab:
                G.check_exact(y, yb, ry, dt, what + " y")
            if mode != 0:
                G.check_exact(xr, xrb, rx, dt, what + " xr")


def run_random(dt, mode, B, H, W, C, route, name, family, table=True, pre_round=False, pads=PADS):
    x, sc, sh = G.random_inputs(f"gnr{mode}{H}{W}{C}", B, H, W, C, dt)
    chk = G.GnCheck(x, (sc, sh) if table else None, 1, mode, dt, pre_round=pre_round)
    for pad in pads:
        y, xr, yb, xrb = ops.gn_apply(x.to(DEV), sc.to(DEV) if table else None, sh.to(DEV) if table else None, 1, mode,
                                      want_y=table, want_xr=mode != 0, route=route, pad=pad)
        got = ops.last_conv_kernel(KIND[dt])
        assert got == name, f"{got} ran, {name} expected"
        what = f"{name} {TN[dt]} {B}x{H}x{W}x{C} pad {pad}"
        if table:
            _note(family + " y", chk.y(y, what))
            G.check_lanes(yb, C, dt, what + " y")
        if mode != 0:
            _note(family + " xr", chk.xr(xr, what))
            G.check_lanes(xrb, C, dt, what + " xr")


E32 = [(32.0, 32.0, 1), (32.0, 32.0, 0)]  # the exact table with and without SiLU


# ------------------------------------------------------------------------------------------------ gn_apply_kernel
@pytest.mark.parametrize("dt", [F32, BF, HF])
@pytest.mark.parametrize("C", [8, 192])
def test_apply_mode0(dt, C):
    name = "gn_apply_kernel<0,affine>"
    run_exact(dt, 0, 2, 5, 7, C, "apply", name, E32 + [(2.0, -1.0, 0)])
    run_random(dt, 0, 2, 5, 7, C, "apply", name, f"apply mode 0 {TN[dt]}")


@pytest.mark.parametrize("dt", [F32, BF, HF])
@pytest.mark.parametrize("mode", [1, 2])
def test_apply_pyramid_without_table(dt, mode):
    name = f"gn_apply_kernel<{mode},raw>"
    run_exact(dt, mode, 2, 6, 10, 8, "apply", name, None)
    run_random(dt, mode, 2, 6, 10, 8, "apply", name, f"pyramid mode {mode} {TN[dt]}", table=False)
    run_exact(dt, mode, 2, 6, 10, 8, None, name, None)  # the dispatch's choice, whatever the size (tests/test_gncheck_cpu.py)


@pytest.mark.parametrize("dt", [F32, BF, HF])
@pytest.mark.parametrize("mode,H,W", [(2, 6, 10), (1, 5, 7)])
def test_apply_resampling_with_table(dt, mode, H, W):
    # mode 2: W % 4 == 2, no other kernel runs it; mode 1: an instantiation the dispatch never reaches
    name = f"gn_apply_kernel<{mode},affine>"
    for C in (8, 16):
        run_exact(dt, mode, 2, H, W, C, "apply", name, E32)
        run_random(dt, mode, 2, H, W, C, "apply", name, f"apply mode {mode} {TN[dt]}")
    if mode == 2:
        run_exact(dt, 2, 2, H, W, 8, None, name, E32)


# ------------------------------------------------------------------------------------------------ gn_resample2x2_kernel
@pytest.mark.parametrize("dt", [F32, BF, HF])
@pytest.mark.parametrize("mode,H,W", [(1, 5, 7), (2, 8, 12)])
def test_block2x2(dt, mode, H, W):
    # <., 2> is reachable from the dispatch for fp32 tensors only (the strips' condition is weaker); forced here in all three
    name = f"gn_resample2x2_kernel<{TN[dt]},{mode}>"
    run_exact(dt, mode, 2, H, W, 16, "block2x2", name, E32)
    run_random(dt, mode, 2, H, W, 16, "block2x2", name, f"2x2 blocks mode {mode} {TN[dt]}")
    if mode == 1:
        run_exact(dt, 1, 2, H, W, 16, None, name, E32)


# ------------------------------------------------------------------------------------------------ gn_fir_down_strip_kernel
@pytest.mark.parametrize("dt", [BF, HF])
@pytest.mark.parametrize("W", [4, 12])
@pytest.mark.parametrize("rs,H", [(rs, h) for rs in (4, 8) for h in (2 * rs, 2 * rs + 2, 4 * rs - 2)])
def test_fir_down_strips(dt, rs, H, W):
    # one whole strip, a ragged one with a single row in the last strip, one row short of two strips; one and three column pairs;
    # C = 16: a shape the half-precision build's row-tile kernel refuses
    name = f"gn_fir_down_strip_kernel<{rs}>"
    run_exact(dt, 2, 2, H, W, 16, f"down_strip{rs}", name, E32)
    run_random(dt, 2, 2, H, W, 16, f"down_strip{rs}", name, f"strips<{rs}> {TN[dt]}")


# ------------------------------------------------------------------------------------------------ gn_fir_down_tiled_kernel
@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("W", [32, 96])
@pytest.mark.parametrize("rs,H", [(rs, h) for rs in (4, 8) for h in (2 * rs, 2 * rs + 2, 6)])
def test_fir_down_row_tiles(rs, H, W, C):
    # W = 32: both halo columns outside the image; H = 6: shorter than one strip
    name = f"gn_fir_down_tiled_kernel<{rs}>"
    run_exact(HF, 2, 2, H, W, C, f"down_tiled{rs}", name, E32)
    run_random(HF, 2, 2, H, W, C, f"down_tiled{rs}", name, f"row tiles<{rs}>", pre_round=True)


def test_row_tiles_exist_in_the_half_build_only_and_forced_routes_check_shapes():
    from diffsep_amd._lib import DiffsepError
    x = torch.zeros(2, 8, 32, 64, device=DEV)
    sc, sh = _table(2, 64, 1.0, 0.0)
    for dt, route in ((BF, "down_tiled4"), (F32, "down_strip4"), (F32, "down_tiled8")):
        with pytest.raises(DiffsepError, match="shape preconditions"):
            ops.gn_apply(x.to(dt), sc, sh, 1, 2, want_xr=True, route=route)
    for args, route in (((2, 8, 30, 64), "down_strip4"), ((2, 6, 32, 64), "block2x2"), ((2, 8, 32, 72), "down_tiled4"),
                        ((2, 8, 48, 64), "down_tiled8")):
        with pytest.raises(DiffsepError, match="shape preconditions"):
            ops.gn_apply(torch.zeros(*args, device=DEV, dtype=HF), *_table(2, args[3], 1.0, 0.0), 1, 2, want_xr=True, route=route)
    with pytest.raises(DiffsepError, match="shape preconditions"):
        ops.gn_apply(torch.zeros(2, 4, 8, 72, device=DEV, dtype=HF), *_table(2, 72, 1.0, 0.0), 1, 1, want_xr=True, route="up_tiled")
    with pytest.raises(DiffsepError, match="shape preconditions"):
        ops.gn_apply(x.to(HF), sc, sh, 1, 2, want_xr=True, route="up_tiled")


# ------------------------------------------------------------------------------------------------ gn_resample_up_tiled_kernel
@pytest.mark.parametrize("dt", [F32, BF, HF])
@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("H,W", [(4, 8), (5, 9), (3, 20)])
def test_up_tiles(dt, C, H, W):
    name = f"gn_resample_up_tiled_kernel<{TN[dt]}>"
    run_exact(dt, 1, 2, H, W, C, "up_tiled", name, E32)
    run_random(dt, 1, 2, H, W, C, "up_tiled", name, f"up tiles {TN[dt]}")


# ------------------------------------------------------------------------------------------------ the dispatch arrives there too
# (tensor type, mode, B, H, W, C, kernel): shapes just over each route's threshold; the small routes' dispatch cases sit with
# their forced ones above.  Exact inputs only where the threshold makes the tensor large.
OVER = [(BF, 2, 2, 256, 512, 64, "gn_fir_down_strip_kernel<4>"), (BF, 2, 16, 256, 256, 64, "gn_fir_down_strip_kernel<8>"),
        (HF, 2, 2, 256, 520, 64, "gn_fir_down_strip_kernel<4>"), (F32, 2, 2, 256, 512, 64, "gn_resample2x2_kernel<f32,2>"),
        (HF, 2, 2, 64, 256, 64, "gn_fir_down_tiled_kernel<4>"), (HF, 2, 2, 256, 512, 64, "gn_fir_down_tiled_kernel<8>"),
        (BF, 1, 2, 128, 128, 64, "gn_resample_up_tiled_kernel<bf16>"), (HF, 1, 2, 128, 128, 64, "gn_resample_up_tiled_kernel<f16>"),
        (F32, 1, 2, 128, 128, 64, "gn_resample_up_tiled_kernel<f32>")]


@pytest.mark.parametrize("dt,mode,B,H,W,C,name", OVER)
def test_dispatch_reaches_each_route(dt, mode, B, H, W, C, name):
    cus = CC.device_cus()
    want = ops.gn_route_name(KIND[dt], mode, True, dt, B, H, W, C, cus=cus)
    assert want == name or (cus != 256 and "tiled_kernel<" in name), f"the route query names {want}"
    run_exact(dt, mode, B, H, W, C, None, want, E32[:1], pads=PADS[:1], big=True)
    if B * H * W * C <= 1 << 21 and mode == 2:
        run_random(dt, mode, B, H, W, C, None, want, "row tiles<4> by dispatch", pre_round="tiled" in want, pads=PADS[:1])


# ------------------------------------------------------------------------------------------------ the statistics pass
NPIX = [(1, 1), (7, 9), (8, 8), (5, 13), (37, 109), (57, 73)]  # 1, 63, 64, 65, 4033, 4161 pixels: one block .. 64 blocks, ragged shares


@pytest.mark.parametrize("dt", [F32, BF, HF])
@pytest.mark.parametrize("C1,C2,groups", [(8, 0, 2), (24, 0, 6), (136, 0, 34), (1024, 0, 32), (64, 72, 34)])
def test_groupnorm_statistics_on_exact_integers(dt, C1, C2, groups):
    # C = 8: one channel octet, 256 pixel lanes; 24: 255 active threads; 136: 17 octets, 15 lanes; 1024: the LDS limit; 64 + 72: the
    # concat read in place.  Values 0..3 (+ 1000): every sum is an exact integer in the kernel's float64 and in the reference.
    C, B = C1 + C2, 2
    gamma = (1.0 + torch.from_numpy(synth.synth_noise(f"gs.g{C}", (C,))) * 0.2).float()
    beta = (torch.from_numpy(synth.synth_noise(f"gs.b{C}", (C,))) * 0.1).float()
    for H, W in NPIX:
        for off in (0.0, 1000.0):
            x = (G._ints(f"gs.x{C}{H}", (B, H, W, C), 0, 3) + off).to(dt)  # (bfloat16 rounds 1001..1003: the STORED integers count)
            xa, xb = x[..., :C1].contiguous(), (x[..., C1:].contiguous() if C2 else None)
            sc, sh = ops.groupnorm_stats(xa.to(DEV), gamma.to(DEV), beta.to(DEV), groups, 1e-6, x2=xb.to(DEV) if C2 else None)
            rs, rh, ts, th = G.stats_reference(xa.float(), xb.float() if C2 else None, gamma, beta, groups)
            es, eh = (sc.double().cpu() - rs).abs(), (sh.double().cpu() - rh).abs()
            what = f"{TN[dt]} C {C1}+{C2} {H}x{W} offset {off}"
            print(f"[gn statistics {what}] worst dscale / tol {float((es / ts).max()):.3f}, dshift / tol {float((eh / th.clamp_min(1e-300)).max()):.3f}")
            assert bool((es <= ts).all()), f"{what}: scale off by {float((es / ts).max()):.2f} of its tolerance at {(es > ts).nonzero()[:4].tolist()}"
            assert bool((eh <= th).all()), f"{what}: shift off by {float((eh / th).max()):.2f} of its tolerance at {(eh > th).nonzero()[:4].tolist()}"
