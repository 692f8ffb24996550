"""CPU self-test of tests/convcheck.py: the per-element bound passes a simulated correct kernel (reference + storage rounding +
random one-ulp flips of the activated input) with room to spare, and catches three local faults that the relative-RMS gate of
4e-3 lets through; the exact-integer generator meets its representability conditions at every channel count it is used with, and
one swapped tap breaks the bit equality."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import convcheck as CC
from diffsep_amd import synth

torch.set_grad_enabled(False)
DT = torch.bfloat16
B, H, W, C = 256, 32, 64, 64
SCALE = 0.70710678


def rnd(tag, shape, scale=1.0):
    return torch.from_numpy(synth.synth_noise(tag, shape)) * scale


def conv32(h, w):
    return F.conv2d(h.float().permute(0, 3, 1, 2), w.float(), None, padding=1).permute(0, 2, 3, 1).double()


@pytest.fixture(scope="module")
def case():
    """the 256 x 32 x 64 x 64 case of test_rw_conv3x3_matches_torch, and a simulated kernel output before storage"""
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    a = (rnd(f"rw.a{B}{H}{C}", (B, H, W, C), 1.2) + 0.1).to(DT)
    w = rnd(f"rw.w{C}", (64, C, 3, 3), 1.0 / math.sqrt(9 * C))
    bias, bb = rnd("rw.bias", (64,), 0.1), rnd(f"rw.bb{B}", (B, 64), 0.1)
    res = rnd(f"rw.r{B}{H}", (B, H, W, 64)).to(DT)
    sc, sh = 1.0 + rnd(f"rw.sc{B}{C}", (B, C), 0.2), rnd(f"rw.sh{B}{C}", (B, C), 0.2)
    chk = CC.ConvCheck((a, None), (sc, sh, 1), w, DT, bias=bias, bb=bb, res=res, out_scale=SCALE)
    v = a.double() * sc.double()[:, None, None, :] + sh.double()[:, None, None, :]
    h = CC.silu64(v).float().to(DT)
    # one-ulp flips (either direction) on a quarter of the activated inputs: what a kernel's own fp32 SiLU may round to
    u = torch.from_numpy(synth.uniform01("cc.flip", h.numel())).reshape(h.shape)
    bits = h.view(torch.int16)
    step = torch.where(u < 0.125, 1, torch.where(u < 0.25, -1, 0)).to(torch.int16)
    step = torch.where((bits & 0x7fff) == 0, torch.zeros_like(step), step)
    hk = (bits + step).view(DT)
    wq = w.to(DT)
    add = bias.double() + bb.double()[:, None, None, :] + res.double()
    pre = (conv32(hk, wq) + add) * SCALE
    return dict(chk=chk, hk=hk.double(), wq=wq.double(), pre=pre)


def test_bound_passes_a_correct_kernel_with_input_flips(case):
    y = case["pre"].float().to(DT)
    assert CC.rel_rms(y, case["chk"].ref) < 4e-3
    assert CC.assert_elementwise(y, case["chk"].ref, case["chk"].bound, "simulated rw 256x32x64") < 0.5


def _fault(case, name):
    """(faulty output before storage, the damaged region as (b, rows, columns))"""
    pre, hk, wq = case["pre"].clone(), case["hk"], case["wq"]
    if name == "missing tap":  # tap (0, 1) of output row 16, columns 32..63 of sample 7: the row above, same column
        b, r = 7, 16
        pre[b, r, 32:64] -= SCALE * torch.einsum("wc,oc->wo", hk[b, r - 1, 32:64], wq[:, :, 0, 1])
        return pre, (b, (r, r), (32, 63))
    if name == "halo from the neighbouring sample":  # the tile at rows 16..31, columns 32..63 of sample 100 reads its left halo
        b = 100                                      # column (column 31, rows 15..32) from sample 101
        d = (hk[b + 1, 15:32, 31] - hk[b, 15:32, 31])[None, :, None]  # [1, 17, 1, C]; row 32 is padding in both
        d = F.pad(d.permute(0, 3, 1, 2), (0, 0, 0, 1))                  # -> rows 15..32
        pre[b, 16:32, 32] += SCALE * F.conv2d(d, wq[:, :, :, 0:1]).permute(0, 2, 3, 1)[0, :, 0]
        return pre, (b, (16, 31), (32, 32))
    assert name == "stale pixel"  # one pixel keeps what the previous launch left there (the neighbouring sample's value)
    pre[200, 9, 41] = pre[199, 9, 41]
    return pre, (200, (9, 9), (41, 41))


@pytest.mark.parametrize("name", ["missing tap", "halo from the neighbouring sample", "stale pixel"])
def test_local_faults_pass_the_rms_gate_and_fail_the_bound(case, name):
    pre, (b, rows, cols) = _fault(case, name)
    y = pre.float().to(DT)
    assert not torch.equal(y, case["pre"].float().to(DT))
    r = CC.rel_rms(y, case["chk"].ref)
    print(f"\n[{name}] relative RMS {r:.3e} (gate 4e-3)")
    assert r < 4e-3
    with pytest.raises(AssertionError) as e:
        CC.assert_elementwise(y, case["chk"].ref, case["chk"].bound, name)
    msg = str(e.value)
    print(msg)
    at = tuple(int(v) for v in msg.split("(b, h, w, c) = (")[1].split(")")[0].split(","))
    assert at[0] == b and rows[0] <= at[1] <= rows[1] and cols[0] <= at[2] <= cols[1]


# (C1, C2, Cout, B, H, W, mode, residual, skip channels): every channel count of the exact GPU cases, at their largest images
USES = [(64, 0, 64, 3, 64, 96, "raw", False, None), (64, 0, 64, 3, 64, 96, "silu", True, None),
        (64, 64, 64, 3, 64, 96, "raw", False, None), (128, 0, 128, 2, 40, 64, "silu", True, None),
        (128, 64, 128, 3, 64, 96, "silu", False, (128, 64)), (128, 128, 256, 3, 12, 64, "silu", False, None),
        (256, 256, 256, 2, 8, 32, "silu", False, None), (256, 0, 256, 2, 8, 32, "silu", False, (256, 256)),
        (64, 192, 48, 3, 16, 12, "affine", True, None), (256, 256, 256, 3, 4, 1, "affine", True, None),
        (128, 0, 6, 3, 8, 8, "silu", True, None), (192, 0, 128, 1, 9, 33, "affine", True, None)]


@pytest.mark.parametrize("C1,C2,CO,Bn,Hn,Wn,mode,res,skip", USES)
def test_exact_generator_is_representable(C1, C2, CO, Bn, Hn, Wn, mode, res, skip):
    c = CC.exact_case("t", Bn, Hn, Wn, C1, C2, CO, mode, res=res, skip=skip)  # (asserts the conditions on its reference)
    assert int((c.w != 0).sum()) == 32 * CO and set(c.w.unique().tolist()) <= {-1.0, 0.0, 1.0}
    assert float(c.ref.abs().max()) > 0
    x = torch.cat([c.a, c.b], -1) if c.b is not None else c.a
    assert len({tuple(x[b, :, :, ch].flatten().tolist()) for b in range(Bn) for ch in (0, 1, C1 + C2 - 1)}) == 3 * Bn
    c32 = CC.exact_case("t", Bn, Hn, Wn, C1, C2, CO, mode, res=res, skip=skip, big=True)  # the float32 reference of the big cases
    assert torch.equal(c.ref, c32.ref)


def test_thin_input_generator_keeps_the_padding_channels_zero():
    c = CC.exact_case("t", 3, 8, 96, 8, 0, 64, "raw", cin_real=6)
    assert not bool(c.a[..., 6:].any()) and not bool(c.w[:, 6:].any()) and int((c.w != 0).sum()) == 32 * 64


def test_one_swapped_tap_breaks_bit_equality():
    c = CC.exact_case("t", 2, 32, 32, 64, 0, 64, "raw")
    st = torch.stack([(c.ref.sum((1, 2)) * 2.0 ** 24).to(torch.int64), ((c.ref ** 2).sum((1, 2)) * 2.0 ** 16).to(torch.int64)], -1)
    CC.check_exact(c, c.ref.to(DT), st, DT, "the reference itself")
    st[1, 7, 1] += 1  # one unit of 2^-16 in one sum of squares
    with pytest.raises(AssertionError, match="sums of squares differ"):
        CC.check_exact(c, c.ref.to(DT), st, DT, "one statistic off by one unit")
    w = c.w.clone()
    o, i = 5, int(((w[5, :, 0, 0] != w[5, :, 2, 2])).nonzero()[0])
    w[o, i, 0, 0], w[o, i, 2, 2] = c.w[o, i, 2, 2], c.w[o, i, 0, 0]
    y = ((CC._conv(c.a, w, False) + c.bias.double() + c.bb.double()[:, None, None, :]) * 0.5).to(DT)
    with pytest.raises(AssertionError, match="output elements differ"):
        CC.check_exact(c, y, None, DT, "swapped tap")
    assert not torch.equal(y, c.ref.to(DT))


def test_multi_tile_batch_against_the_launchers():
    """multi_tile_batch restates the launchers' grid sizing (blocks per image = CUs / B, at least 1, at most the image's tiles; tiles
    handed out in contiguous shares): the lines it restates are read from the .hip sources, then its result is checked against them"""
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "diffusion-separation_amd", "csrc")
    rw, ws, halo = (open(os.path.join(csrc, f)).read() for f in ("conv3x3_rw.hip", "conv3x3_ws.hip", "conv3x3_halo.h"))
    # (the register-weight launcher takes its start value, its tile count and the clamp from the halo-tile kernels' shared launch tail)
    body = re.search(r"int rw_blocks_per_image\(.*?\n}", rw, re.S).group(0)
    assert "int g = halo_blocks_wanted(a, 1);" in body and "rw_blocks_per_image(a, halo_tiles(a, G::TH))" in rw
    body = re.search(r"inline int halo_blocks_wanted\(.*?\n}", halo, re.S).group(0)
    assert "const int g = ds_num_cus() / (a.B * ncb);" in body
    assert "inline int halo_tiles(const ConvArgs& a, int tile_h) { return (a.H / tile_h) * (a.W / TW); }" in halo
    body = re.search(r"\nint halo_launch\(.*?\n}", halo, re.S).group(0)
    assert "const int tiles = halo_tiles(a, tile_h);" in body and "k.G = g < 1 ? 1 : (g > tiles ? tiles : g);" in body
    assert "static constexpr int TH = PGN * RPW" in rw
    body = re.search(r"int ws_blocks_per_image\(.*?\n}", ws, re.S).group(0)
    assert "int g = ds_num_cus() / a.B;" in body and "if (g < 1) g = 1;" in body and "if (g > tiles) g = tiles;" in body
    assert "constexpr int TH = 8, TW = 32;" in ws and "const int tiles = (a.H / TH) * (a.W / TW);" in body
    assert "constexpr int TW = 32" in halo

    def blocks(Bn, tiles, cus):  # the launchers' lines
        g = cus // Bn
        g = 1 if g < 1 else g
        return tiles if g > tiles else g
    for (Hn, Wn, th, cus) in [(64, 96, 8, 256), (32, 32, 4, 256), (16, 96, 8, 256), (64, 96, 8, 304), (16, 96, 8, 64)]:
        Bn = CC.multi_tile_batch(Hn, Wn, th, 32, cus)
        tiles = (Hn // th) * (Wn // 32)
        g = blocks(Bn, tiles, cus)
        shares = {(tiles * (i + 1)) // g - (tiles * i) // g for i in range(g)}  # any contiguous split into g shares
        assert shares == {1, 2}, (Bn, tiles, g)
        assert all(not (blocks(b, tiles, cus) < tiles < 2 * blocks(b, tiles, cus)) for b in range(1, Bn))
