"""CPU self-test of tests/gemmcheck.py, after the pattern of tests/test_convcheck_cpu.py.  A "simulated kernel" is the honest
computation in float32 on the stored operands (its own summation order and roundings where the kernels round; one-ulp flips on a
quarter of the activated inputs where the launch activates) — it must stay within the element bound on every family, which is a
condition on the reference and the derivation alone.  The same simulation with one injected fault must (1) fail the element
bound, (2) differ on the exact-integer case, and (3) pass or fail the relative-RMS gate of the corresponding GPU test as RMS_PASSES
states.  At the shapes of tests/test_gemm_gpu.py (the smallest at which each edge exists) every listed fault damages 10 % or more
of a small output and fails the RMS gates as well (0.09 .. 1.0 against 1.5e-2; an overflowing softmax gives nan) — the existing
GPU tests just do not run these shapes and operands.  Confined to the 32-row overhang tile of one sample the same faults measure
1.2e-2 .. 0.17: one wrong column group passes the gate, a dropped channel tail misses it by a factor of 1.7, and a full-size
layer (256 x 256 pixels, 62 times the rows) dilutes each of them a further eight-fold.  The element bound and the exact case see all of them at any
size.  The generators' representability conditions are asserted at every shape the GPU tests use."""
import math

import numpy as np
import pytest
import torch

import convcheck as CC
import gemmcheck as GC
from convcheck import BF, HF
from diffsep_amd import synth

torch.set_grad_enabled(False)
DT = BF
B, H, W = 2, 33, 32          # 1056 pixels: four 256-row tiles and a 32-row overhang tile
M = H * W
rnd = GC.rnd

# fault -> does the relative-RMS gate of the corresponding GPU test pass it (bfloat16 tolerances: test_conv1x1 1.5e-2,
# test_attention / test_attention_ragged_key_count 2e-2)?  What the simulation shows, asserted below.
RMS_GATE = {"conv": 1.5e-2, "gemm": 1.5e-2, "attn": 2e-2}
RMS_PASSES = {
    "channel tail dropped": False, "tail read across the seam": False, "overhang rows from the previous tile": False,
    "column 64 with column 0's weights": False, "sample 1 times sample 0's Bt": False, "row bias along n": False,
    "div_b[0] for every sample": False, "softmax padding columns carry weight": False, "softmax without the maximum": False,
}
# the same convolution faults confined to the 32-row overhang tile of sample 1 (1.5 % of the output)
LOCAL = " (overhang tile of sample 1 only)"
RMS_PASSES.update({"channel tail dropped" + LOCAL: False, "tail read across the seam" + LOCAL: False,
                   "overhang rows from the previous tile" + LOCAL: False, "column 64 with column 0's weights" + LOCAL: True})


def flip_quarter(h, tag):
    """one-ulp flips (either direction) on a quarter of a bfloat16 tensor: what a kernel's own fp32 activation may round to"""
    u = torch.from_numpy(synth.uniform01(tag, h.numel())).reshape(h.shape)
    bits = h.view(torch.int16)
    step = torch.where(u < 0.125, 1, torch.where(u < 0.25, -1, 0)).to(torch.int16)
    step = torch.where((bits & 0x7fff) == 0, torch.zeros_like(step), step)
    return (bits + step).view(h.dtype)


# ------------------------------------------------------------------------------------------------ 1x1 convolution (conv2d_fused)
def conv_inputs(C1, C2, CO, exact):
    """operands of one activated 1x1 launch with residual, both biases, out_scale 0.5: random, or convcheck's exact case"""
    if exact:
        c = CC.exact_case(f"gc{C1}{C2}{CO}", B, H, W, C1, C2, CO, "silu", res=True, ksize=1)
        x = torch.cat([c.a, c.b], -1) if C2 else c.a
        return dict(x=x, sc=c.sc, sh=c.sh, w=c.w, bias=c.bias, bb=c.bb, res=c.res, ref=c.ref, C1=C1, exact=True)
    C = C1 + C2
    x = (rnd(f"gc.x{C}", (B, H, W, C), 1.2) + 0.1).to(DT)
    w = rnd(f"gc.w{C}{CO}", (CO, C, 1, 1), 1.0 / math.sqrt(C))
    bias, bb = rnd("gc.bias", (CO,), 0.1), rnd("gc.bb", (B, CO), 0.1)
    res = rnd(f"gc.r{CO}", (B, H, W, CO)).to(DT)
    sc, sh = 1.0 + rnd(f"gc.sc{C}", (B, C), 0.2), rnd(f"gc.sh{C}", (B, C), 0.2)
    chk = CC.ConvCheck((x, None), (sc, sh, 1), w, DT, bias=bias, bb=bb, res=res, out_scale=0.5)
    return dict(x=x, sc=sc, sh=sh, w=w, bias=bias, bb=bb, res=res, chk=chk, ref=chk.ref, C1=C1, exact=False)


def sim_conv(d, fault=None):
    """the simulated kernel's output in the storage type"""
    if fault and fault.endswith(LOCAL):
        y, yf = sim_conv(d).reshape(B, M, -1).clone(), sim_conv(d, fault[:-len(LOCAL)]).reshape(B, M, -1)
        y[1, 1024:] = yf[1, 1024:]
        return y.reshape(B, H, W, -1)
    x, C1 = d["x"], d["C1"]
    v = x.double() * d["sc"].double()[:, None, None, :] + d["sh"].double()[:, None, None, :]
    h = CC.silu64(v).float().to(DT)
    if not d["exact"]:
        h = flip_quarter(h, "gc.flip")
    h = h.float()
    wq = d["w"].to(DT).float()[:, :, 0, 0]
    if fault == "channel tail dropped":          # Cin = 72: the K chunk that holds channels 64..71 contributes nothing
        h = h.clone()
        h[..., 64:] = 0
    if fault == "tail read across the seam":     # 40 + 24: the tail of source 1 (channels 32..39) read from source 2's start
        h = h.clone()
        h[..., 32:C1] = h[..., C1:C1 + (C1 - 32)]
    # float32 accumulation, channels in two halves (another order than the reference's)
    k2 = h.shape[-1] // 2
    acc = torch.einsum("bhwc,oc->bhwo", h[..., :k2], wq[:, :k2]) + torch.einsum("bhwc,oc->bhwo", h[..., k2:], wq[:, k2:])
    if fault == "column 64 with column 0's weights":
        acc[..., 64] = acc[..., 0]
    y = (acc + (d["bias"] + d["bb"][:, None, None, :]).float() + d["res"].float()) * 0.5
    if fault == "overhang rows from the previous tile":   # rows 1024..1055 of every sample come from rows 768..799
        y = y.reshape(B, M, -1).clone()
        y[:, 1024:1056] = y[:, 768:800]
        y = y.reshape(B, H, W, -1)
    return y.to(DT)


CONV_FAULTS = [("channel tail dropped", 72, 0, 72), ("tail read across the seam", 40, 24, 64),
               ("overhang rows from the previous tile", 72, 0, 72), ("column 64 with column 0's weights", 72, 0, 72)]


@pytest.fixture(scope="module")
def conv_cases():
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    return {(C1, C2, CO, ex): conv_inputs(C1, C2, CO, ex) for (C1, C2, CO) in {c[1:] for c in CONV_FAULTS} for ex in (False, True)}


@pytest.mark.parametrize("C1,C2,CO", sorted({c[1:] for c in CONV_FAULTS}))
def test_honest_conv1x1_is_within_the_bound_and_exact(conv_cases, C1, C2, CO):
    d = conv_cases[(C1, C2, CO, False)]
    assert d["chk"](sim_conv(d), f"simulated 1x1 {C1}+{C2}->{CO}") <= 1.0
    e = conv_cases[(C1, C2, CO, True)]
    assert torch.equal(sim_conv(e).double(), e["ref"])


def _judge(name, family, y, ref, check, y_exact, ref_exact):
    r = CC.rel_rms(y, ref)
    print(f"\n[{name}] relative RMS {r:.3e} (gate {RMS_GATE[family]:g}: {'passes' if r < RMS_GATE[family] else 'fails'})")
    assert (r < RMS_GATE[family]) == RMS_PASSES[name]
    with pytest.raises(AssertionError, match="over their bound"):
        check(y)
    assert not torch.equal(y_exact.double(), ref_exact.double()), f"{name}: the exact case does not see the fault"


@pytest.mark.parametrize("name,C1,C2,CO", CONV_FAULTS + [(c[0] + LOCAL,) + c[1:] for c in CONV_FAULTS])
def test_conv1x1_faults(conv_cases, name, C1, C2, CO):
    d, e = conv_cases[(C1, C2, CO, False)], conv_cases[(C1, C2, CO, True)]
    _judge(name, "conv", sim_conv(d, name), d["ref"], lambda y: CC.assert_elementwise(y, d["ref"], d["chk"].bound, name),
           sim_conv(e, name), e["ref"].float().to(DT))


# ------------------------------------------------------------------------------------------------ GEMM (gemm_nt)
def sim_gemm(a, bt, Bn, bias, bias_mode, div, res, out_scale, fault=None):
    """float32, K in two halves, the general epilogue's order of operations"""
    a, bt = a.float(), bt.float()
    Mn, K = a.shape[-2:]
    N = bt.shape[-2]
    a, bt = a.expand(Bn, Mn, K), bt.expand(Bn, N, K)
    if fault == "sample 1 times sample 0's Bt":
        bt = bt[:1].expand(Bn, N, K)
    k2 = K // 2
    v = torch.einsum("bmk,bnk->bmn", a[..., :k2], bt[..., :k2]) + torch.einsum("bmk,bnk->bmn", a[..., k2:], bt[..., k2:])
    if div is not None:
        dv = div.float()
        if fault == "div_b[0] for every sample":
            dv = dv[:1].expand(Bn)
        v = v / dv[:, None, None]
    if bias is not None:
        if fault == "row bias along n":
            v = v + bias.float()[None, None, :N]
        else:
            v = v + (bias.float()[None, :, None] if bias_mode else bias.float()[None, None, :])
    if res is not None:
        v = v + res.float()[..., :N]
    return (v * out_scale).to(DT)


# (fault, M, N, K, a_batched, bias_mode, div, out_scale)
GEMM_FAULTS = [("sample 1 times sample 0's Bt", 68, 68, 64, True, None, None, 0.125),
               ("row bias along n", 64, 20, 64, False, 1, None, 0.5),
               ("div_b[0] for every sample", 1056, 6, 8, True, 0, (2.0, 4.0), 0.5)]


def gemm_pair(Mn, N, K, a_b, bias_mode, div, out_scale):
    tag = f"gg{Mn}{N}{K}"
    e = GC.exact_gemm(tag, 2, Mn, N, K, a_batched=a_b, bias_mode=bias_mode, div=div, out_scale=out_scale)
    a = rnd(tag + ".a", (2, Mn, K) if a_b else (Mn, K)).to(DT)
    bt = rnd(tag + ".bt", (2, N, K), 1.0 / math.sqrt(K)).to(DT)
    bias = None if bias_mode is None else rnd(tag + ".bias", (Mn if bias_mode else N,), 0.5)
    dv = None if div is None else torch.tensor(div)
    chk = GC.GemmCheck(a, bt, DT, bias=bias, bias_mode=bias_mode or 0, div=dv, out_scale=out_scale)
    return e, (a, bt, bias, dv, chk)


@pytest.mark.parametrize("name,Mn,N,K,a_b,bias_mode,div,out_scale", GEMM_FAULTS)
def test_gemm_faults_and_the_honest_kernel(name, Mn, N, K, a_b, bias_mode, div, out_scale):
    e, (a, bt, bias, dv, chk) = gemm_pair(Mn, N, K, a_b, bias_mode, div, out_scale)
    bm = bias_mode or 0
    assert chk(sim_gemm(a, bt, 2, bias, bm, dv, None, out_scale), f"simulated gemm {Mn}x{N}x{K}") <= 1.0
    assert torch.equal(sim_gemm(e.a, e.bt, 2, e.bias, bm, e.div, None, out_scale).double(), e.ref[:, 0])
    _judge(name, "gemm", sim_gemm(a, bt, 2, bias, bm, dv, None, out_scale, name), chk.ref, lambda y: chk(y, name),
           sim_gemm(e.a, e.bt, 2, e.bias, bm, e.div, None, out_scale, name), e.ref[:, 0].float().to(DT))


# ------------------------------------------------------------------------------------------------ attention chain
def sim_attention(q, k, vt, L, dt, fault=None):
    """scores -> storage -> softmax_kernel's arithmetic in float32 -> storage -> P V over Lp columns -> storage"""
    Bn, _, C = q.shape
    Lp = vt.shape[-1]
    s = torch.zeros(Bn, L, Lp)
    s[..., :L] = torch.einsum("bic,bjc->bij", q.float(), k.float()) * np.float32(1.0 / math.sqrt(C))
    s = s.to(dt).float()                                   # (the score GEMM writes its padding columns as zeros)
    mx = s[..., :L].max(-1, keepdim=True).values
    if fault == "softmax without the maximum":
        mx = torch.zeros_like(mx)
    e = torch.exp(s - mx)
    inv = 1.0 / e[..., :L].sum(-1, keepdim=True)
    p = e * inv
    if fault != "softmax padding columns carry weight":
        p[..., L:] = 0
    p = p.to(dt).float()
    return torch.einsum("bij,bcj->bic", p, vt.float()).to(dt), p.to(dt)


def attn_random(Bn, L, gain, dt):
    C = 128
    q, k, v = (rnd(f"atr.{n}{L}.{Bn}", (Bn, L, C)) for n in "qkv")   # the operands of test_attention_ragged_key_count
    q, k, v = (q * gain).to(dt), k.to(dt), v.to(dt)
    vt = torch.full((Bn, C, GC.rup8(L)), 100.0)
    vt[:, :, :L] = v.float().transpose(1, 2)
    return q, k, v, vt.to(dt)


@pytest.mark.parametrize("dt", [BF, HF], ids=["bf16", "f16"])
@pytest.mark.parametrize("Bn,L,gain", [(2, 4, 1.0), (2, 12, 1.0), (2, 20, 1.0), (2, 64, 1.0), (2, 68, 1.0), (16, 20, 30.0), (1, 13, 1.0)])
def test_honest_attention_is_within_the_bound(dt, Bn, L, gain):
    q, k, v, vt = attn_random(Bn, L, gain, dt)
    o, p = sim_attention(q, k, vt, L, dt)
    ro, rp = GC.AttnCheck(q, k, v, dt)(o, p, f"simulated attention {Bn}x{L} x{gain:g}")
    assert ro <= 1.0 and rp <= 1.0


@pytest.mark.parametrize("L,C", [(L, C) for L in (4, 12, 20, 64, 68) for C in (64, 256)])
def test_exact_attention_generator_and_the_honest_kernel(L, C):
    c = GC.exact_attention(f"xa{L}{C}", 2, L, C)   # (asserts its own properties)
    assert {kd for row in c.kinds for kd in row} == ({"a", "b", "c"} if GC.pow2(L) else {"a", "b"})
    for dt in (BF, HF):
        o, p = sim_attention(c.q.to(dt), c.k.to(dt), c.vt.to(dt), L, dt)
        s = torch.zeros(2, L, c.Lp)
        s[..., :L] = c.scores.float()
        GC.check_exact_attention(c, o, s, p, dt, f"simulated exact attention L{L} C{C}")


@pytest.mark.parametrize("name,Bn,L,gain", [("softmax padding columns carry weight", 2, 20, 1.0), ("softmax without the maximum", 16, 20, 30.0)])
def test_attention_faults(name, Bn, L, gain):
    q, k, v, vt = attn_random(Bn, L, gain, DT)
    chk = GC.AttnCheck(q, k, v, DT)
    o, p = sim_attention(q, k, vt, L, DT, name)
    r = CC.rel_rms(o, chk.o)
    print(f"\n[{name}] relative RMS {r:.3e} (gate {RMS_GATE['attn']:g})")
    assert (r < RMS_GATE["attn"]) == RMS_PASSES[name]   # (nan compares false: an overflowing softmax fails the gate)
    with pytest.raises(AssertionError):
        chk(o, p, name)
    c = GC.exact_attention("xaf", 2, 20, 64)
    oe, pe = sim_attention(c.q.to(DT), c.k.to(DT), c.vt.to(DT), 20, DT, name)
    s = torch.zeros(2, 20, c.Lp)
    s[..., :20] = c.scores.float()
    with pytest.raises(AssertionError):
        GC.check_exact_attention(c, oe, s, pe, DT, name)


# ------------------------------------------------------------------------------------------------ generators at the GPU shapes
CONV_SHAPES = [(2, 33, 32, 72, 0, 72), (2, 33, 32, 40, 24, 64), (2, 33, 32, 64, 64, 128), (2, 33, 32, 8, 0, 6), (2, 33, 32, 64, 0, 24),
               (3, 7, 9, 8, 0, 64), (3, 5, 13, 8, 0, 64), (1, 16, 16, 192, 0, 136)]


@pytest.mark.parametrize("Bn,Hn,Wn,C1,C2,CO", CONV_SHAPES)
@pytest.mark.parametrize("mode", ["raw", "affine", "silu"])
def test_exact_1x1_generator_is_representable(Bn, Hn, Wn, C1, C2, CO, mode):
    c = CC.exact_case("t", Bn, Hn, Wn, C1, C2, CO, mode, res=True, ksize=1)   # (asserts the conditions on its reference)
    assert tuple(c.w.shape) == (CO, C1 + C2, 1, 1) and set(c.w.unique().tolist()) <= {-1.0, 0.0, 1.0}
    assert int((c.w != 0).sum()) == min(32, C1 + C2) * CO and float(c.ref.abs().max()) > 0


def test_3x3_generator_is_unchanged():
    """the kernel-size argument leaves the 3x3 cases what they were: 32 non-zero taps per output channel, the same draws"""
    c = CC.exact_case("t", 2, 8, 8, 64, 0, 64, "raw")
    assert tuple(c.w.shape) == (64, 64, 3, 3) and int((c.w != 0).sum()) == 32 * 64
    w = CC.sparse_signs("t.w", 64, 9 * 64, 32).reshape(64, 3, 3, 64).permute(0, 3, 1, 2)
    assert torch.equal(c.w, w)


def test_kernel_name_check():
    GC.assert_kernel("conv_mfma_kernel<bf16,1,8,32,64,2,2,64,1,2,0,256>", "N64", "bf16")
    GC.assert_kernel("conv_mfma_kernel<float,1,8,8,64,1,1,32,1,2,1,256>", "8X8", "split")
    with pytest.raises(AssertionError):
        GC.assert_kernel("conv_mfma_kernel<float,1,8,32,32,2,1,32,1,2,0,256>", "N64", "f32")
    with pytest.raises(AssertionError):
        GC.assert_kernel("conv_mfma_kernel<float,9,8,32,64,2,2,16,1,2,0,256>", "N64", "f32")
    assert [GC.plan_class(m, n) for m, n in ((1056, 72), (1056, 6), (1056, 32), (63, 64), (256, 136), (512, 1024))] == \
        ["N64", "N32", "N32", "8X8", "8X8", "N64"]
