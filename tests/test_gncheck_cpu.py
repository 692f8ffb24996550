"""CPU self-test of tests/gncheck.py, the instruments of tests/test_gn_gpu.py.  The per-element bound passes a simulated correct
kernel (reference arithmetic in fp32, storage rounding, one-ulp flips of a quarter of the activated values in the precision the
kernel holds them in) below ratio 0.5, for FIR up, FIR down and FIR down behind the row-tile kernel's rounding of the activated
value; three local faults of the FIR-down kernels' geometry pass the relative-RMS gates of the existing tests (1e-2 bfloat16,
1.5e-3 half) and exceed ratio 1; on the exact inputs an activated padding pixel and a tap shifted by one column each break
torch.equal.  The route query (diffsep_gn_route_name: host arithmetic, no device) returns, for a table of launches, the kernels
that the thresholds of gn_apply_typed named before it was split into ds_gn_route and a launch function."""
import os
import re

import pytest
import torch

import diffsep_oracle as O
import gncheck as G
from diffsep_amd import _lib, ops, synth

torch.set_grad_enabled(False)
BF, HF, F32 = G.BF, G.HF, G.F32


# ------------------------------------------------------------------------------------------------ the filter and the exact cases
@pytest.mark.parametrize("mode", [1, 2])
def test_filter_is_the_oracles(mode):
    x = torch.from_numpy(synth.synth_noise("gc.fir", (2, 3, 6, 10)))  # NCHW for the oracle (pinned to the reference's golden vectors)
    want = (O.fir_up2 if mode == 1 else O.fir_down2)(x)
    got = G.fir(x.permute(0, 2, 3, 1).double(), mode).permute(0, 3, 1, 2)
    assert float((got - want.double()).abs().max()) < 1e-6


@pytest.mark.parametrize("mode,H,W", [(0, 5, 7), (0, 6, 10), (1, 5, 7), (1, 6, 10), (1, 18, 12), (2, 6, 10), (2, 18, 12), (2, 2, 4)])
def test_exact_reference_is_representable(mode, H, W):
    x = G.exact_inputs("t", 2, H, W, 16)
    ry, rx = G.exact_reference(x, (32.0, 32.0), mode)  # (asserts the conditions on its references)
    assert float(ry.max()) <= 128.0 and (mode == 0 or float(rx.max()) <= 3.0)
    step = {0: 32.0, 1: 2.0, 2: 0.5}[mode]
    assert torch.equal(ry / step, (ry / step).round())
    assert len({tuple(x[b, :, :, c].flatten().tolist()) for b in range(2) for c in (0, 1, 15)}) == 6
    if mode == 0:
        r2, _ = G.exact_reference(x, (2.0, -1.0), 0)
        assert set(r2.unique().tolist()) == {-1.0, 1.0, 3.0, 5.0}


@pytest.mark.parametrize("dt", [BF, HF, F32])
@pytest.mark.parametrize("mode", [1, 2])
def test_exact_faults_break_bit_equality(mode, dt):
    x = G.exact_inputs("t", 2, 8, 12, 16)
    ry, rx = G.exact_reference(x, (32.0, 32.0), mode)
    G.check_exact(ry.to(dt), None, ry, dt, "the reference itself")
    a = x.double() * 32.0 + 32.0
    # (1) the padding is activated: SiLU(shift) = 32 outside the image instead of 0
    big = torch.nn.functional.pad(a.permute(0, 3, 1, 2), (2, 2, 2, 2), value=32.0).permute(0, 2, 3, 1)
    yb = G.fir(big, mode)
    k = 1 if mode == 2 else 4
    y1 = yb[:, k:yb.shape[1] - k, k:yb.shape[2] - k]
    assert y1.shape == ry.shape and torch.equal(y1[:, 2:-2, 2:-2], ry[:, 2:-2, 2:-2])
    assert float((y1 - ry).abs().max()) >= 4.0
    with pytest.raises(AssertionError, match="elements differ"):
        G.check_exact(y1.to(dt), None, ry, dt, "activated padding")
    # (2) every tap one column to the right
    y2 = G.fir(torch.cat([a[:, :, 1:], torch.zeros_like(a[:, :, :1])], 2), mode)
    with pytest.raises(AssertionError, match="elements differ"):
        G.check_exact(y2.to(dt), None, ry, dt, "shifted tap")
    # a written pad lane
    buf = torch.full(tuple(ry.shape[:3]) + (24,), float("nan"), dtype=dt)
    buf[..., :16] = ry.to(dt)
    G.check_exact(buf[..., :16], buf, ry, dt, "padded buffer")
    buf[1, 2, 3, 17] = 0.0
    with pytest.raises(AssertionError, match="lanes beyond C"):
        G.check_exact(buf[..., :16], buf, ry, dt, "padded buffer, one lane written")


# ------------------------------------------------------------------------------------------------ the bound: simulated kernels
def _flip(t, tag):
    """one-ulp flips, either direction, on a quarter of the elements of a float32 / 16-bit tensor"""
    u = torch.from_numpy(synth.uniform01(tag, t.numel())).reshape(t.shape)
    it = torch.int32 if t.dtype == torch.float32 else torch.int16
    bits = t.view(it)
    step = torch.where(u < 0.125, 1, torch.where(u < 0.25, -1, 0)).to(it)
    step = torch.where((bits & (0x7fffffff if it == torch.int32 else 0x7fff)) == 0, torch.zeros_like(step), step)
    return (bits + step).view(t.dtype)


def simulate(chk, dt, pre_round, tag):
    """(activated values as the kernel holds them, its y before storage): the activated value in fp32 — or rounded to the storage
    type, for the row-tile kernel — with one-ulp flips in THAT precision on a quarter of them; the filter in fp32"""
    ak = chk.a.float()
    if not pre_round:
        ak = _flip(ak, tag)
    else:
        # The kernel rounds ITS fp32 value, which is within d_k = 2^-16 of the exact one: on a quarter of the elements the value is
        # moved by the full d_k, either way, in front of the rounding, so the stored value flips to the neighbouring one wherever a
        # correct kernel's can.  (A flip of the rounded value itself by one ulp in a random direction lands up to 1.5 ulp from the
        # exact value, which no rounding of a value that near does: it gives ratio 0.84 on the case below, and 0.62 when every
        # flip goes towards the exact value's side — inside the bound, above the 0.5 asked of a correct kernel.)
        u = torch.from_numpy(synth.uniform01(tag, ak.numel())).reshape(ak.shape)
        d = torch.where(u < 0.125, G.D_ABS, torch.where(u < 0.25, -G.D_ABS, 0.0))
        ak = (chk.a + d).float().to(dt).float()
    return ak, G.fir(ak, chk.mode)


@pytest.fixture(scope="module")
def down():
    """FIR down at [8, 132, 256, 128] (66 output rows: a ragged last strip of 8- or 4-row strips): x holds values that are exact in
    bfloat16 AND half, so one float64 reference serves both types; (GnCheck, kernel's activated values, y before storage) for the
    strip kernel in bfloat16 and the row-tile kernel (activated value rounded first) in half"""
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    x, sc, sh = G.random_inputs("gc.down", 8, 132, 256, 128, BF)
    x = torch.where(x.float().abs() < 2.0 ** -10, torch.zeros_like(x), x)
    assert torch.equal(x.float().to(HF).float(), x.float())
    out = {}
    for dt, pre in ((BF, False), (HF, True)):
        chk = G.GnCheck(x.float().to(dt), (sc, sh), 1, 2, dt, pre_round=pre)
        out[dt] = (chk,) + simulate(chk, dt, pre, f"gc.flip{pre}")
    out["x"] = x
    return out


@pytest.mark.parametrize("dt", [BF, HF])
def test_bound_passes_a_correct_fir_down(down, dt):
    chk, _, pre = down[dt]
    y = pre.to(dt)
    assert G.rel_rms(y, chk.ref_y) < G.RMS_GATE[dt]
    assert chk.y(y, f"simulated down {dt}") < 0.5
    chk.xr(G.fir(down["x"].float(), 2).to(dt), f"simulated down {dt}")


def test_bound_passes_a_correct_fir_down_without_pre_rounding_in_half():
    x, sc, sh = G.random_inputs("gc.down2", 2, 20, 64, 64, HF)
    chk = G.GnCheck(x, (sc, sh), 1, 2, HF)
    _, pre = simulate(chk, HF, False, "gc.flip2")
    assert chk.y(pre.to(HF), "simulated down half, fp32 activation") < 0.5


@pytest.mark.parametrize("dt", [BF, HF, F32])
def test_bound_passes_a_correct_fir_up(dt):
    x, sc, sh = G.random_inputs("gc.up", 2, 21, 40, 64, dt)
    chk = G.GnCheck(x, (sc, sh), 1, 1, dt)
    _, pre = simulate(chk, dt, False, "gc.flipu")
    y = pre.to(dt)
    # (fp32 tensors: a flipped fp32 ulp on top of the reference's own rounding is 1.5 of the 2 units d_k allows the SiLU: 0.60)
    assert chk.y(y, f"simulated up {dt}") < (0.5 if dt != F32 else 1.0)
    chk.xr(G.fir(x.float(), 1).to(dt), f"simulated up {dt}")


RS, TILE_COLS = 8, 32  # strips of 8 output rows; the row-tile kernel's tiles of 32 input columns (16 output columns)


def _fault(name, ak, pre):
    """(faulty y before storage, damaged region (b, rows, columns, channels)) — each fault as small as the kernels' geometry makes
    it: one thread's 8 channels"""
    pre = pre.clone()
    ch = slice(40, 48)
    if name in ("seam: halo column reads 0", "seam: halo column of the neighbouring sample"):
        # tile 3 of sample 5, strip 2: its left halo (input column 95) feeds output column 48 through the horizontal tap 1/8
        b, tx, st = 5, 3, 2
        col = TILE_COLS * tx - 1
        have = ak[b, :, col, ch]
        got = torch.zeros_like(have) if name.endswith("reads 0") else ak[b + 1, :, col, ch]
        d = G._fir_axis(got - have, 0, 2) / 8.0  # [Ho, 8]
        rows = slice(st * RS, st * RS + RS)
        pre[b, rows, 16 * tx, ch] += d[rows]
        return pre, (b, (st * RS, st * RS + RS - 1), (16 * tx, 16 * tx), (40, 47))
    assert name == "stale row at the ragged strip end"  # the last output row (65 = 8 * 8 + 1) keeps what the neighbouring sample left there
    oy = pre.shape[1] - 1
    assert oy % RS != RS - 1
    pre[6, oy, 77, ch] = pre[7, oy, 77, ch]
    return pre, (6, (oy, oy), (77, 77), (40, 47))


@pytest.mark.parametrize("dt", [BF, HF])
@pytest.mark.parametrize("name", ["seam: halo column reads 0", "seam: halo column of the neighbouring sample",
                                  "stale row at the ragged strip end"])
def test_local_faults_pass_the_rms_gate_and_fail_the_bound(down, name, dt):
    chk, ak, pre = down[dt]
    bad, (b, rows, cols, chans) = _fault(name, ak, pre)
    y = bad.to(dt)
    assert not torch.equal(y, pre.to(dt))
    r = G.rel_rms(y, chk.ref_y)
    worst = G.ratio(y, chk.ref_y, chk.bound_y)
    print(f"\n[{name}, {dt}] relative RMS {r:.3e} (gate {G.RMS_GATE[dt]:.1e}), worst err / bound {worst:.1f}")
    assert r < G.RMS_GATE[dt]
    assert worst > 1.0
    with pytest.raises(AssertionError) as e:
        chk.y(y, name)
    at = tuple(int(v) for v in str(e.value).split("(b, h, w, c) = (")[1].split(")")[0].split(","))
    assert at[0] == b and rows[0] <= at[1] <= rows[1] and cols[0] <= at[2] <= cols[1] and chans[0] <= at[3] <= chans[1]


# ------------------------------------------------------------------------------------------------ the route table
A, R = True, False  # with a table / the pyramid's raw FIR
# (library, tensor type, mode, table, B, H, W, C, compute units) -> kernel; read off the thresholds of gn_apply_typed:
#   up tiles: table, C % 64 == 0, B H W C / 8 >= 262144;  row tiles (half build, 16-bit): W % 32 == 0, C % 64 == 0, B H W C >= 2^21,
#   strips of 8 halved to 4 while B (W / 32) ceil(H / 2 / rs) (C / 64) < 2 CUs;  strips (16-bit): W % 4 == 0, B (H/4) (W/4) C / 8 >= 131072,
#   <8> where B (W/4) (C/8) ceil(H / 2 / 8) >= 131072;  2 x 2 blocks: up always, down with H % 4 == W % 4 == 0 over the same 131072
ROUTES = [
    ("bf16", BF, 2, A, 2, 256, 520, 128, 256, "gn_fir_down_strip_kernel<4>"),   # the largest down case of test_groupnorm_silu_resample
    ("bf16", BF, 2, A, 16, 256, 256, 64, 256, "gn_fir_down_strip_kernel<8>"),   # the 256-row level at a production batch: exactly 131072
    ("bf16", BF, 2, A, 16, 256, 252, 64, 256, "gn_fir_down_strip_kernel<4>"),   # ... and 129024
    ("bf16", BF, 2, A, 2, 256, 512, 64, 256, "gn_fir_down_strip_kernel<4>"),    # B (H/4) (W/4) C/8 = 131072
    ("bf16", BF, 2, A, 2, 256, 508, 64, 256, "gn_apply_kernel<2,affine>"),      # 130048
    ("bf16", BF, 2, A, 2, 256, 256, 64, 256, "gn_apply_kernel<2,affine>"),      # (65536: test_groupnorm_silu_resample's 256 x 256)
    ("bf16", BF, 2, A, 2, 258, 512, 64, 256, "gn_fir_down_strip_kernel<4>"),    # H % 4 == 2: strips need even H only
    ("bf16", BF, 2, A, 2, 256, 514, 64, 256, "gn_apply_kernel<2,affine>"),      # W % 4 == 2
    ("bf16", F32, 2, A, 2, 256, 512, 64, 256, "gn_resample2x2_kernel<f32,2>"),
    ("bf16", F32, 2, A, 2, 256, 508, 64, 256, "gn_apply_kernel<2,affine>"),
    ("bf16", F32, 2, A, 2, 258, 512, 64, 256, "gn_apply_kernel<2,affine>"),     # 2 x 2 blocks need H % 4 == 0
    ("bf16", F32, 2, A, 2, 256, 520, 128, 256, "gn_resample2x2_kernel<f32,2>"),
    ("bf16", BF, 1, A, 2, 128, 128, 64, 256, "gn_resample_up_tiled_kernel<bf16>"),  # exactly 262144
    ("bf16", BF, 1, A, 2, 128, 127, 64, 256, "gn_resample2x2_kernel<bf16,1>"),      # 260096
    ("bf16", F32, 1, A, 2, 128, 128, 64, 256, "gn_resample_up_tiled_kernel<f32>"),
    ("bf16", F32, 1, A, 2, 128, 127, 64, 256, "gn_resample2x2_kernel<f32,1>"),
    ("bf16", BF, 1, A, 2, 128, 128, 72, 256, "gn_resample2x2_kernel<bf16,1>"),      # C % 64 != 0
    ("bf16", BF, 1, A, 1, 3, 5, 8, 256, "gn_resample2x2_kernel<bf16,1>"),           # up with a table: never gn_apply_kernel<1,affine>
    ("bf16", BF, 0, A, 2, 32, 64, 64, 256, "gn_apply_kernel<0,affine>"),
    ("bf16", BF, 1, R, 2, 128, 128, 64, 256, "gn_apply_kernel<1,raw>"),             # the pyramid: no table, whatever the size
    ("bf16", BF, 2, R, 16, 256, 256, 64, 256, "gn_apply_kernel<2,raw>"),
    ("f16", HF, 2, A, 2, 64, 256, 64, 256, "gn_fir_down_tiled_kernel<4>"),          # exactly 2^21 elements; 64 blocks of 8-row strips
    ("f16", HF, 2, A, 2, 62, 256, 64, 256, "gn_apply_kernel<2,affine>"),            # 2031616
    ("f16", HF, 2, A, 16, 256, 256, 64, 256, "gn_fir_down_tiled_kernel<8>"),        # 2048 blocks
    ("f16", HF, 2, A, 16, 256, 256, 64, 1024, "gn_fir_down_tiled_kernel<8>"),       # ... = 2 CUs
    ("f16", HF, 2, A, 16, 256, 256, 64, 1025, "gn_fir_down_tiled_kernel<4>"),
    ("f16", HF, 2, A, 2, 256, 256, 64, 256, "gn_fir_down_tiled_kernel<4>"),         # (test_f16_fir_down_row_tiles: 256 blocks < 512)
    ("f16", HF, 2, A, 2, 256, 520, 128, 256, "gn_fir_down_strip_kernel<4>"),        # W % 32 != 0: the strips, as in the bfloat16 build
    ("f16", HF, 2, A, 16, 256, 264, 64, 256, "gn_fir_down_strip_kernel<8>"),
    ("f16", HF, 2, A, 16, 256, 256, 72, 256, "gn_fir_down_strip_kernel<8>"),        # C % 64 != 0
    ("f16", F32, 2, A, 16, 256, 256, 64, 256, "gn_resample2x2_kernel<f32,2>"),      # fp32 tensors never take the 16-bit kernels
    ("f16", HF, 1, A, 2, 128, 128, 64, 256, "gn_resample_up_tiled_kernel<f16>"),
    ("f16", HF, 1, A, 2, 128, 127, 64, 256, "gn_resample2x2_kernel<f16,1>"),
    ("bf16", BF, 2, A, 16, 256, 256, 64, 1025, "gn_fir_down_strip_kernel<8>"),      # (the strips do not weigh compute units)
]


@pytest.mark.parametrize("kind,dt,mode,aff,B,H,W,C,cus,want", ROUTES)
def test_route_query_matches_the_thresholds(kind, dt, mode, aff, B, H, W, C, cus, want):
    assert ops.gn_route_name(kind, mode, aff, dt, B, H, W, C, has_xr=mode != 0, cus=cus) == want
    if mode != 0 and aff:  # the route does not depend on whether xr is wanted, nor on padded leading dimensions
        assert ops.gn_route_name(kind, mode, aff, dt, B, H, W, C, pad=(8, 16, 8), has_xr=False, cus=cus) == want


def test_route_query_refuses_bad_shapes_and_route_codes_mirror_the_header():
    with pytest.raises(_lib.DiffsepError, match="even H, W"):
        ops.gn_route_name("bf16", 2, True, BF, 2, 5, 8, 16)
    with pytest.raises(_lib.DiffsepError, match="multiple of 8"):
        ops.gn_route_name("bf16", 0, True, BF, 2, 4, 8, 12)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "diffsep_hip.h")).read()
    codes = {n.lower(): int(v) for n, v in re.findall(r"#define DIFFSEP_GN_(\w+)\s+(\d+)", hdr)}
    assert codes == _lib.GN_ROUTES
