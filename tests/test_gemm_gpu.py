"""The TAPS = 1 half of csrc/conv_mfma.hip (1x1 convolutions, batched NT GEMMs) and the unfused attention chain on it, with the two
instruments of tests/gemmcheck.py: exact integers (torch.equal on outputs, statistics, scores, probabilities, padding) and the
per-element bound against float64 references, for bfloat16, half (the f16 library), fp32 and fp32 split, at the smallest shapes
at which each edge of the code exists (tile classes N64 / N32 / 8X8, channel tails, the concat seam, M and N overhang, both
weight layouts, GroupNorm from accumulators, row bias, shared operand, batched Bt, div_b, K = Lp below a chunk, the softmax zero
fill).  Every launch asserts the ds_conv_plan class it reached through the kernel name.  tests/test_gemmcheck_cpu.py shows what
the instruments see; the worst err / bound per family is printed and kept in gemmcheck.MEASURED."""
import math
import time

import pytest
import torch
import torch.nn.functional as F

import convcheck as CC
import gemmcheck as GC
from convcheck import BF, F32, HF
from diffsep_amd import ops

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda"
KINDS = [pytest.param(k, dt, sp, id=k) for k, dt, sp in GC.STORAGE]
WORST = {}
rnd = GC.rnd


@pytest.fixture(autouse=True)
def wall_time(request):
    t0 = time.perf_counter()
    yield
    torch.cuda.synchronize()
    print(f"\n[gemm wall] {request.node.name}: {time.perf_counter() - t0:.2f} s")


@pytest.fixture(scope="module", autouse=True)
def measured_table():
    yield
    print("\n[gemmcheck MEASURED] family -> worst err / bound as (bf16, f16, f32, split)")
    for fam in sorted({f for f, _ in WORST}):
        print(f'    "{fam}": ({", ".join(format(WORST.get((fam, k), float("nan")), ".3f") for k, _, _ in GC.STORAGE)}),')


def note(family, kind, ratio):
    WORST[(family, kind)] = max(WORST.get((family, kind), 0.0), ratio)


def lib_kind(kind):
    return "f16" if kind == "f16" else "bf16"


def last_kernel(kind, cls):
    GC.assert_kernel(ops.last_conv_kernel(lib_kind(kind)), cls, kind)


# ------------------------------------------------------------------------------------------------ ops.conv2d_fused(ksize=1)
# (class, (B, H, W), C1, C2, Cout, note)
CONV = [
    ("N64", (2, 33, 32), 72, 0, 72, "K tail of 8 in both chunk widths, N overhang of one 8-column group"),
    ("N64", (2, 33, 32), 40, 24, 64, "seam inside a chunk, both sources end in a tail"),
    ("N64", (2, 33, 32), 64, 64, 128, "both weight layouts"),
    ("N32", (2, 33, 32), 8, 0, 6, "the output-layer shape: padding stays zero"),
    ("N32", (2, 33, 32), 64, 0, 24, ""),
    ("8X8", (3, 7, 9), 8, 0, 64, "the Combine shape, one tile one row short"),
    ("8X8", (3, 5, 13), 8, 0, 64, "the Combine shape, one pixel into a second tile"),
    ("8X8", (1, 16, 16), 192, 0, 136, "three N blocks, the last 8 wide"),
]
CONV_IDS = [f"{c[0]}-{'x'.join(map(str, c[1]))}-{c[2]}+{c[3]}-{c[4]}" for c in CONV]
MODES = ("raw", "affine", "silu")


def conv_layouts(C1, C2, dt):
    kc = ops.conv2d_chunk(1, dt)
    return (0, kc) if (C1 + C2) % kc == 0 and C1 % kc == 0 else (0,)


@pytest.mark.parametrize("kind,dt,split", KINDS)
@pytest.mark.parametrize("cls,shape,C1,C2,CO,why", CONV, ids=CONV_IDS)
def test_conv1x1_exact_integers(cls, shape, C1, C2, CO, why, kind, dt, split):
    """bit for bit on the output, both int64 statistics and the zero padding channels, in every mode and weight layout"""
    B, H, W = shape
    assert GC.plan_class(H * W, CO) == cls
    cp = GC.rup8(CO)
    for mode in MODES:
        c = CC.exact_case(f"g1{C1}{C2}{CO}{B}{H}{W}{mode}", B, H, W, C1, C2, CO, mode, res=True, ksize=1)
        a, bt = c.a.to(DEV, dt), (c.b.to(DEV, dt) if C2 else None)
        gn = None if mode == "raw" else (c.sc.to(DEV), c.sh.to(DEV))
        res = F.pad(c.res, (0, cp - CO)).to(DEV, dt)
        for chunk in conv_layouts(C1, C2, dt):
            wp = ops.pack_conv_weight(c.w, dt, chunk=chunk).to(DEV)
            y, st = ops.conv2d_fused(a, wp, c.bias.to(DEV), CO, 1, x2=bt, gn=gn, gn_act=1 if mode == "silu" else 0, bias_b=c.bb.to(DEV),
                                     res=res, out_scale=0.5, cout_pad=cp, stats=True, w_chunk=chunk, split=split)
            last_kernel(kind, cls)
            CC.check_exact(c, y, st, dt, f"1x1 {kind} {C1}+{C2}->{CO} {B}x{H}x{W} {mode} chunk {chunk}")


def conv_random(tag, B, H, W, C1, C2, CO, dt):
    C = C1 + C2
    x = (rnd(f"{tag}.x", (B, H, W, C), 1.2) + 0.1).to(dt)
    d = dict(a=x[..., :C1].contiguous().to(DEV), b=x[..., C1:].contiguous().to(DEV) if C2 else None)
    d["w"] = rnd(f"{tag}.w", (CO, C, 1, 1), 1.0 / math.sqrt(C))
    d["bias"], d["bb"] = rnd(f"{tag}.bias", (CO,), 0.1).to(DEV), rnd(f"{tag}.bb", (B, CO), 0.1).to(DEV)
    d["res"] = F.pad(rnd(f"{tag}.r", (B, H, W, CO)), (0, GC.rup8(CO) - CO)).to(DEV, dt)
    d["sc"], d["sh"] = (1.0 + rnd(f"{tag}.sc", (B, C), 0.2)).to(DEV), rnd(f"{tag}.sh", (B, C), 0.2).to(DEV)
    return d


@pytest.mark.parametrize("kind,dt,split", KINDS)
@pytest.mark.parametrize("cls,shape,C1,C2,CO,why", CONV, ids=CONV_IDS)
def test_conv1x1_element_bound(cls, shape, C1, C2, CO, why, kind, dt, split):
    B, H, W = shape
    cp = GC.rup8(CO)
    d = conv_random(f"gb{C1}{C2}{CO}{H}", B, H, W, C1, C2, CO, dt)
    kw = dict(bias=d["bias"], bb=d["bb"], res=d["res"], out_scale=0.5)
    for mode in MODES:
        gn = None if mode == "raw" else (d["sc"], d["sh"])
        chk = CC.ConvCheck((d["a"], d["b"]), None if gn is None else (d["sc"], d["sh"], int(mode == "silu")), d["w"], dt, split=split, cout=CO, **kw)
        for chunk in conv_layouts(C1, C2, dt):
            wp = ops.pack_conv_weight(d["w"], dt, chunk=chunk).to(DEV)
            y = ops.conv2d_fused(d["a"], wp, d["bias"], CO, 1, x2=d["b"], gn=gn, gn_act=int(mode == "silu"), bias_b=d["bb"], res=d["res"],
                                 out_scale=0.5, cout_pad=cp, w_chunk=chunk, split=split)
            last_kernel(kind, cls)
            note(f"1x1 {cls} {mode}", kind, chk(y, f"1x1 {kind} {cls} {C1}+{C2}->{CO} {mode} chunk {chunk}"))
            assert not bool(y[..., CO:].any())


@pytest.mark.parametrize("kind,dt,split", KINDS)
def test_conv1x1_groupnorm_from_accumulators(kind, dt, split):
    """64 + 64 -> 128 at 1056 pixels with the GroupNorm table built in the kernel's prologue from the producers' accumulators: the
    output and the statistics equal, bit for bit, those of the launch that is handed the finalize launch's table (the path the
    exact cases go through), and the output is within the element bound of the float64 reference on that table"""
    B, H, W, C1, C2, CO = 2, 33, 32, 64, 64, 128
    d = conv_random("gacc", B, H, W, C1, C2, CO, dt)
    acc = []
    for t in (d["a"], d["b"]):  # any accumulators are legitimate input; these are the stored tensors' own sums
        td = t.double()
        acc.append(torch.stack([(td.sum((1, 2)) * ops.STAT_SUM_SCALE).round().to(torch.int64),
                                ((td * td).sum((1, 2)) * ops.STAT_SQ_SCALE).round().to(torch.int64)], -1).contiguous())
    groups = 32
    g, be = (1.0 + rnd("gacc.g", (C1 + C2,), 0.2)).to(DEV), rnd("gacc.be", (C1 + C2,), 0.1).to(DEV)
    sc, sh = ops.groupnorm_from_acc(acc[0], acc[1], g, be, groups, H * W)
    chk = CC.ConvCheck((d["a"], d["b"]), (sc, sh, 1), d["w"], dt, bias=d["bias"], bb=d["bb"], res=d["res"], out_scale=0.5, split=split)
    for chunk in conv_layouts(C1, C2, dt):
        wp = ops.pack_conv_weight(d["w"], dt, chunk=chunk).to(DEV)
        kw = dict(x2=d["b"], gn_act=1, bias_b=d["bb"], res=d["res"], out_scale=0.5, stats=True, w_chunk=chunk, split=split)
        y, st = ops.conv2d_fused(d["a"], wp, d["bias"], CO, 1, gn_acc=(acc[0], acc[1], g, be, groups), **kw)
        last_kernel(kind, "N64")
        y0, st0 = ops.conv2d_fused(d["a"], wp, d["bias"], CO, 1, gn=(sc, sh), **kw)
        last_kernel(kind, "N64")
        assert torch.equal(y, y0) and torch.equal(st, st0)
        note("1x1 N64 gn_acc", kind, chk(y, f"1x1 {kind} gn_acc chunk {chunk}"))


# ------------------------------------------------------------------------------------------------ ops.gemm_nt
# (name, class, M, N, K, ldy, a_batched, bias_mode, div, out_scale, residual)
GEMM = [
    ("V^T L20", "8X8", 64, 20, 64, 24, False, 1, None, 0.5, False),
    ("V^T L20 wide ldy", "8X8", 64, 20, 64, 32, False, 1, None, 0.5, False),
    ("V^T L272", "8X8", 64, 272, 64, 272, False, 1, None, 0.5, False),
    ("QK^T 20", "8X8", 20, 20, 64, 24, True, None, None, 0.125, False),
    ("QK^T 68", "8X8", 68, 68, 64, 72, True, None, None, 0.125, False),
    ("PV K24", "8X8", 20, 64, 24, 64, True, None, None, 0.5, True),
    ("output layer", "N32", 1056, 6, 8, 8, True, 0, (2.0, 4.0), 0.5, False),
]
SENTINEL = 7.0


@pytest.mark.parametrize("kind,dt,split", KINDS)
@pytest.mark.parametrize("name,cls,M,N,K,ldy,a_b,bias_mode,div,out_scale,with_res", GEMM, ids=[g[0].replace(" ", "_") for g in GEMM])
def test_gemm_nt(name, cls, M, N, K, ldy, a_b, bias_mode, div, out_scale, with_res, kind, dt, split):
    """exact integers, then the element bound on random data, through the unit entry of the general TAPS = 1 launch.  Contract of
    the output columns (conv_mfma.hip's epilogue stores whole 8-column groups below cout8 = N rounded up to 8): [N, cout8) are
    written as zeros, [cout8, ldy) keep what the caller put there."""
    B = 2
    assert GC.plan_class(M, N) == cls
    bm = bias_mode or 0

    def run(a, bt, bias, dv, res):
        out = torch.full((B, M, ldy), SENTINEL, dtype=dt, device=DEV)
        y = ops.gemm_nt(a.to(DEV, dt), bt.to(DEV, dt), N, B=B, bias=None if bias is None else bias.to(DEV), bias_mode=bm,
                        div_b=None if dv is None else dv.to(DEV), res=None if res is None else res.to(DEV, dt), out_scale=out_scale,
                        out=out, split=split)
        last_kernel(kind, cls)
        return y

    c = GC.exact_gemm(f"gx{name}", B, M, N, K, a_batched=a_b, bias_mode=bias_mode, div=div, res=with_res, out_scale=out_scale)
    y = run(c.a if a_b else c.a[0], c.bt, c.bias, c.div, c.res)
    GC.check_exact_gemm(c, y, dt, f"gemm_nt {kind} {name}", sentinel=SENTINEL)

    tag = f"gr{name}"
    a = rnd(tag + ".a", (B, M, K) if a_b else (M, K)).to(dt)
    bt = rnd(tag + ".bt", (B, N, K), 1.0 / math.sqrt(K)).to(dt)
    bias = None if bias_mode is None else rnd(tag + ".bias", (M if bm else N,), 0.5)
    dv = None if div is None else torch.tensor(div)
    res = F.pad(rnd(tag + ".r", (B, M, N)), (0, GC.rup8(N) - N)).to(dt) if with_res else None
    chk = GC.GemmCheck(a, bt, dt, B=B, bias=bias, bias_mode=bm, div=dv, res=res, out_scale=out_scale, split=split)
    y = run(a, bt, bias, dv, res)
    note(f"gemm_nt {name}", kind, chk(y, f"gemm_nt {kind} {name}"))
    n8 = GC.rup8(N)
    assert not bool(y[..., N:n8].any()) and bool((y[..., n8:].float() == SENTINEL).all())


def test_gemm_nt_refuses_bad_arguments():
    """every out-of-range leading dimension is a DS_CHECK refusal, not a launch"""
    a, bt = torch.zeros(2, 16, 64, device=DEV), torch.zeros(2, 20, 64, device=DEV)
    for kw in (dict(out=torch.zeros(2, 16, 16, device=DEV)),                      # ldy below N rounded up to 8
               dict(res=torch.zeros(2, 16, 20, device=DEV)),                      # ldr no multiple of 8
               dict(bias_mode=2)):
        with pytest.raises((ops._lib.DiffsepError, ValueError)):
            ops.gemm_nt(a, bt, 20, **kw)
    with pytest.raises((ops._lib.DiffsepError, ValueError)):
        ops.gemm_nt(torch.zeros(2, 16, 12, device=DEV), torch.zeros(2, 20, 12, device=DEV), 20)   # K no multiple of 8


# ------------------------------------------------------------------------------------------------ ops.attention
def attn_run(q, k, vt, dt, split, workspace=None):
    return ops.attention(q.to(DEV, dt), k.to(DEV, dt), vt.to(DEV, dt), split=split, return_workspace=True, workspace=workspace)


@pytest.mark.parametrize("kind,dt,split", KINDS)
@pytest.mark.parametrize("C", [64, 256])
@pytest.mark.parametrize("L", [4, 12, 20, 64, 68])
def test_attention_exact_rows(L, C, kind, dt, split):
    """one-hot, two-way tie and uniform rows: scores, probabilities, their zero padding and the output bit for bit"""
    c = GC.exact_attention(f"xa{L}{C}", 2, L, C)
    o, scores, probs = attn_run(c.q, c.k, c.vt, dt, split)
    last_kernel(kind, "8X8")
    GC.check_exact_attention(c, o, scores, probs, dt, f"attention {kind} L{L} C{C}")


def attn_random(B, L, gain, dt):
    C = 128
    q, k, v = (rnd(f"atr.{n}{L}.{B}", (B, L, C)) for n in "qkv")   # (the operands of test_attention_ragged_key_count)
    q, k, v = (q * gain).to(dt), k.to(dt), v.to(dt)
    vt = torch.full((B, C, GC.rup8(L)), 100.0)
    vt[:, :, :L] = v.float().transpose(1, 2)
    return q, k, v, vt.to(dt)


@pytest.mark.parametrize("kind,dt,split", KINDS)
@pytest.mark.parametrize("B,L,gain", [(2, 4, 1.0), (2, 12, 1.0), (2, 20, 1.0), (2, 64, 1.0), (2, 68, 1.0), (16, 20, 30.0)])
def test_attention_element_bound(B, L, gain, kind, dt, split):
    q, k, v, vt = attn_random(B, L, gain, dt)
    o, scores, probs = attn_run(q, k, vt, dt, split)
    last_kernel(kind, "8X8")
    chk = GC.AttnCheck(q, k, v, dt, split=split)
    note("attention scores", kind, CC.assert_elementwise(scores[..., :L], chk.s, chk.s_bound, f"attention {kind} B{B} L{L} x{gain:g} scores"))
    ro, rp = chk(o, probs, f"attention {kind} B{B} L{L} x{gain:g}")
    note("attention o" + (" gain 30" if gain != 1.0 else ""), kind, ro)
    note("attention P" + (" gain 30" if gain != 1.0 else ""), kind, rp)


@pytest.mark.parametrize("kind,dt,split", KINDS)
def test_attention_partial_softmax_block_stays_inside_its_workspace(kind, dt, split):
    """B L = 13 rows: the last softmax block (4 rows, one wave each) has one row; nothing is written past B L Lp elements of
    either workspace region, nor past the workspace"""
    B, L = 1, 13
    q, k, v, vt = attn_random(B, L, 1.0, dt)
    esz = torch.empty(0, dtype=dt).element_size()
    one, both = ops.attention_workspace_bytes(B, L, esz)
    n = B * L * GC.rup8(L) * esz
    assert n < one
    ws = torch.full((both + 4096,), 0xA5, dtype=torch.uint8, device=DEV)
    o, scores, probs = attn_run(q, k, vt, dt, split, workspace=ws)
    ro, rp = GC.AttnCheck(q, k, v, dt, split=split)(o, probs, f"attention {kind} B1 L13")
    note("attention o", kind, ro)
    note("attention P", kind, rp)
    wc = ws.cpu()
    assert bool((wc[n:one] == 0xA5).all()) and bool((wc[one + n:2 * one] == 0xA5).all()) and bool((wc[both:] == 0xA5).all())


# ------------------------------------------------------------------------------------------------ batch independence
@pytest.mark.parametrize("kind,dt,split", KINDS)
@pytest.mark.parametrize("cls,shape,C1,C2,CO", [(c[0], c[1], c[2], c[3], c[4]) for c in (CONV[1], CONV[4], CONV[5])], ids=["N64", "N32", "8X8"])
def test_conv1x1_sample_0_does_not_depend_on_the_batch(cls, shape, C1, C2, CO, kind, dt, split):
    B, H, W = shape
    d = conv_random(f"gi{cls}", B, H, W, C1, C2, CO, dt)
    wp = ops.pack_conv_weight(d["w"], dt).to(DEV)

    def run(n):
        y, st = ops.conv2d_fused(d["a"][:n].contiguous(), wp, d["bias"], CO, 1, x2=d["b"][:n].contiguous() if C2 else None,
                                 gn=(d["sc"][:n].contiguous(), d["sh"][:n].contiguous()), gn_act=1, bias_b=d["bb"][:n].contiguous(),
                                 res=d["res"][:n].contiguous(), out_scale=0.5, cout_pad=GC.rup8(CO), stats=True, split=split)
        last_kernel(kind, cls)
        return y, st
    (y2, s2), (y1, s1) = run(B), run(1)
    assert torch.equal(y2[:1], y1) and torch.equal(s2[:1], s1)


@pytest.mark.parametrize("kind,dt,split", KINDS)
def test_attention_sample_0_does_not_depend_on_the_batch(kind, dt, split):
    q, k, v, vt = attn_random(2, 20, 1.0, dt)
    o2, s2, p2 = attn_run(q, k, vt, dt, split)
    o1, s1, p1 = attn_run(q[:1], k[:1], vt[:1], dt, split)
    assert torch.equal(o2[:1], o1) and torch.equal(s2[:1], s1) and torch.equal(p2[:1], p1)
