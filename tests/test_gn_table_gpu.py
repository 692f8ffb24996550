"""One GroupNorm table, whoever builds it.  On every convolution route and in the fused attention block, a launch that builds
its scale / shift table itself from the producers' channel-sum accumulators (gn_acc=) gives the SAME BITS (torch.equal) as the
same launch given gn=(scale, shift) from the finalize launch (ops.groupnorm_from_acc) on the same accumulators: the engine
hands a consumer either form (DESIGN.md sections 4 and 8).  Each case also checks, from diffsep_last_conv_kernel(), that it
ran on the route it names.  Shapes: the smallest each kernel accepts; B = 2, SiLU after the affine,
min(C / 4, 32) groups.  The 16-bit cases run in both libraries (bfloat16 and half-precision storage)."""
import contextlib
import math

import pytest
import torch

from diffsep_amd import _lib, ops, synth

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda"
B = 2
BF, HF, F32 = torch.bfloat16, torch.float16, torch.float32


def rnd(tag, shape, scale=1.0):
    return torch.from_numpy(synth.synth_noise(tag, shape)) * scale


@contextlib.contextmanager
def rw_small(on):
    """the register-weight kernel also for launches with fewer tiles than compute units (as tests/test_rw_gpu.py)"""
    libs = [_lib.lib(k) for k in ("bf16", "f16")] if on else []
    for l in libs:
        _lib.check(l.diffsep_set_option(b"rw_small", 1), l)
    try:
        yield
    finally:
        for l in libs:
            _lib.check(l.diffsep_set_option(b"rw_small", 0), l)


def case_id(route, dt):
    return f"{route}-{str(dt).replace('torch.', '')}".replace(" ", "_")


def producers(tag, C1, C2, H, W, dt):
    """x (+ x2) with their accumulators, out of small conv2d_fused(..., stats=True) launches; gamma, beta, groups"""
    def produce(t, Cp):
        xi = rnd(f"gnt.x{tag}{t}", (B, H, W, 16)).to(DEV, dt)
        wi = ops.pack_conv_weight(rnd(f"gnt.w{tag}{t}", (Cp, 16, 3, 3), 1.0 / 12.0), dt).to(DEV)
        return ops.conv2d_fused(xi, wi, rnd(f"gnt.b{tag}{t}", (Cp,), 0.3).to(DEV), Cp, 3, stats=True)
    a, sa = produce("a", C1)
    bt, sb = produce("b", C2) if C2 else (None, None)
    C = C1 + C2
    g, be = (1.0 + rnd(f"gnt.g{tag}", (C,), 0.2)).to(DEV), rnd(f"gnt.be{tag}", (C,), 0.1).to(DEV)
    return a, sa, bt, sb, g, be, min(C // 4, 32)


def kind_of(dt):
    return "f16" if dt == HF else "bf16"


def check_pair(run, dt, kernel_prefix):
    """run(gn=..., gn_acc=...) -> y for both forms; bit equality, finite and non-trivial output, the route's kernel both times"""
    y_acc, k_acc = run(True)
    y_tab, k_tab = run(False)
    assert k_acc.startswith(kernel_prefix) and k_tab.startswith(kernel_prefix), (k_acc, k_tab)
    assert bool(torch.isfinite(y_acc.float()).all()) and float(y_acc.float().abs().max()) > 0
    assert torch.equal(y_acc, y_tab)


# route, kernel, C1, C2, Cout, H, W, ksize, storage types
FUSED = [
    ("GENERIC 3x3", "conv_mfma_kernel", 16, 16, 24, 8, 8, 3, (F32, BF, HF)),
    ("GENERIC 1x1", "conv_mfma_kernel", 64, 64, 64, 16, 32, 1, (BF, HF)),
    ("WS", "conv3x3_ws1_kernel", 64, 0, 64, 8, 32, 3, (BF, HF)),
    ("THIN_OUT", "conv3x3_thin_out_kernel", 128, 0, 6, 8, 32, 3, (BF, HF)),
    ("SMALL", "conv3x3_small_kernel", 128, 0, 128, 4, 4, 3, (BF, HF)),
    ("SMALL seam", "conv3x3_small_kernel", 64, 192, 48, 16, 12, 3, (BF, HF)),  # the group seam crosses the concat
    ("RW", "conv3x3_rw_kernel", 128, 0, 64, 32, 32, 3, (BF, HF)),
    ("RW cat", "conv3x3_rw_kernel", 64, 64, 64, 32, 32, 3, (BF, HF)),
]


@pytest.mark.parametrize("route,kernel,C1,C2,CO,H,W,k,dt", [c[:8] + (dt,) for c in FUSED for dt in c[8]],
                         ids=[case_id(c[0], dt) for c in FUSED for dt in c[8]])
def test_conv_table_from_accumulators_equals_finalize_table(route, kernel, C1, C2, CO, H, W, k, dt):
    a, sa, bt, sb, g, be, groups = producers(f"{route}{dt}", C1, C2, H, W, dt)
    C = C1 + C2
    wp = ops.pack_conv_weight(rnd(f"gnt.W{route}", (CO, C, k, k), 1.0 / math.sqrt(k * k * C)), dt).to(DEV)
    sc, sh = ops.groupnorm_from_acc(sa, sb, g, be, groups, H * W)

    def run(acc):
        y = ops.conv2d_fused(a, wp, None, CO, k, x2=bt, gn_act=1, cout_pad=(CO + 7) // 8 * 8,
                             **(dict(gn_acc=(sa, sb, g, be, groups)) if acc else dict(gn=(sc, sh))))
        return y, ops.last_conv_kernel(kind_of(dt))
    with rw_small(route.startswith("RW")):
        check_pair(run, dt, kernel)


# route, kernel, Cin, Cout, storage types (8 x 32 images; fragment-major weights; fp32 = split mode)
STREAMED = [
    ("SW", "conv3x3_sw_kernel", 64, 128, (BF, HF)),
    ("SW 512", "conv3x3_sw_kernel", 512, 128, (BF, HF)),  # two table entries per thread, 16 channels per group
    ("SWS", "conv3x3_sws_kernel", 64, 64, (F32,)),
]


@pytest.mark.parametrize("route,kernel,C,CO,dt", [c[:4] + (dt,) for c in STREAMED for dt in c[4]],
                         ids=[case_id(c[0], dt) for c in STREAMED for dt in c[4]])
def test_streamed_conv_table_from_accumulators_equals_finalize_table(route, kernel, C, CO, dt):
    H, W = 8, 32
    a, sa, _, _, g, be, groups = producers(f"{route}{dt}", C, 0, H, W, dt)
    w = rnd(f"gnt.W{route}", (CO, C, 3, 3), 1.0 / math.sqrt(9 * C))
    wf = (ops.pack_frag_weight_split(w) if dt == F32 else ops.pack_frag_weight(w, dt)).to(DEV)
    sc, sh = ops.groupnorm_from_acc(sa, None, g, be, groups, H * W)

    def run(acc):
        y = ops.conv3x3_streamed(a, wf, CO, **(dict(gn_acc=(sa, None, g, be, groups)) if acc else dict(gn=(sc, sh))))
        return y, ops.last_conv_kernel(kind_of(dt))
    check_pair(run, dt, kernel)


@pytest.mark.parametrize("dt", [BF, HF], ids=["bfloat16", "float16"])
def test_fused_attention_table_from_accumulators_equals_finalize_table(dt):
    L, C = 16, 128
    x, sa, _, _, g, be, groups = producers(f"attn{dt}", C, 0, 4, 4, dt)
    x = x.reshape(B, L, C)
    ws = [ops.pack_frag_weight(rnd(f"gnt.attn.w{i}", (C, C, 1, 1), 1.0 / math.sqrt(C)), dt).to(DEV) for i in range(3)]
    bs = [rnd(f"gnt.attn.b{i}", (C,), 0.1).to(DEV) for i in range(3)]
    sc, sh = ops.groupnorm_from_acc(sa, None, g, be, groups, L)
    y_acc = ops.attn_fused(x, *ws, *bs, gn_acc=(sa, g, be, groups))
    k_acc = ops.last_conv_kernel(kind_of(dt))
    y_tab = ops.attn_fused(x, *ws, *bs, gn=(sc, sh))
    assert k_acc.startswith("attn_fused_kernel") and ops.last_conv_kernel(kind_of(dt)).startswith("attn_fused_kernel")
    assert bool(torch.isfinite(y_acc.float()).all()) and float((y_acc.float() - x.float()).abs().max()) > 0
    assert torch.equal(y_acc, y_tab)
