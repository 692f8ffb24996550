"""Unit-op wrappers over the C-ABI (parity tests call the kernels through these).
Activations are NHWC torch tensors on the GPU; bf16 is torch.bfloat16 storage."""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from ._lib import (F32_SPLIT, F32, BF16, GN_ROUTES, ODE_WORKSPACE_BYTES, LossConfig, _ptr, _stream_ptr, call, check, host_array, lib,
                   sde_config)


def _dt_of(dtype):
    if dtype == torch.float32:
        return F32
    if dtype in (torch.bfloat16, torch.float16):  # the 16-bit storage format of the library _L(t) picks
        return BF16
    raise TypeError("float32, bfloat16 or float16 expected")


def _dt(t):
    return _dt_of(t.dtype)


def _L(t):
    """the library build whose 16-bit storage format is t's: half-precision tensors go to libdiffsep_hip_f16.so"""
    return lib("f16" if (t is not None and t.dtype == torch.float16) else "bf16")


def _dts(t, split):
    """dtype code of a matrix-product launch: split=True asks for bf16x3 products on fp32 tensors."""
    if split and t.dtype != torch.float32:
        raise TypeError("split products are a mode of fp32 tensors")
    return F32_SPLIT if split else _dt(t)


def _stats_arg(stats, B, C, device):
    """stats= of a launch: False -> None, True -> zeroed int64 accumulators [B,C,2], a tensor -> itself (the launch adds into it)"""
    if stats is True:
        return torch.zeros((B, C, 2), dtype=torch.int64, device=device)
    return None if stats is False else stats


def _gn_arg(gn):
    """gn = (scale, shift) | None"""
    return gn if gn is not None else (None, None)


def _gn_acc_arg(gn_acc, n):
    """gn_acc = (acc1[, acc2 | None], gamma, beta, groups) | None: n = 5 / 4 elements"""
    return gn_acc if gn_acc is not None else (None,) * (n - 1) + (0,)


def _skip_arg(skip):
    """skip = (sx, sx2 | None, weights) | None -> (sx, sx2, weights, channels of sx, channels of both)"""
    sx, sx2, sw = skip if skip is not None else (None, None, None)
    sC1 = sx.shape[-1] if sx is not None else 0
    return sx, sx2, sw, sC1, sC1 + (sx2.shape[-1] if sx2 is not None else 0)


def _resampled(mode, H, W):
    """output size of resample mode 0 / 1 / 2 = none / x2 up / x2 down"""
    return {0: (H, W), 1: (2 * H, 2 * W), 2: (H // 2, W // 2)}[mode]


def _params_blob(params):
    """a list of parameter arrays as one flat float32 host blob"""
    return np.ascontiguousarray(np.concatenate([np.asarray(p, np.float32).reshape(-1) for p in params]))


def to_nhwc(x, cpad=None):
    """NCHW torch tensor -> contiguous NHWC (optionally zero-padded to cpad channels)."""
    y = x.permute(0, 2, 3, 1).contiguous()
    if cpad is not None and cpad > y.shape[-1]:
        y = torch.nn.functional.pad(y, (0, cpad - y.shape[-1]))
    return y.contiguous()


def to_nchw(y, c=None):
    y = y.permute(0, 3, 1, 2)
    return (y if c is None else y[:, :c]).contiguous()


def pack_conv_weight(w, dtype, chunk=0):
    """OIHW float32 -> [O][taps][Ipad] in `dtype` (Ipad = roundup(I, 8)); chunk = kc > 0: chunk-major
    [Ipad/kc][taps][O][kc] (kc = conv2d_chunk(ksize, dtype); needs Ipad % kc == 0)."""
    O, I, kh, kw = w.shape
    wp = w.permute(0, 2, 3, 1).reshape(O, kh * kw, I)
    ipad = (I + 7) // 8 * 8
    if ipad != I:
        wp = torch.nn.functional.pad(wp, (0, ipad - I))
    if chunk:
        assert ipad % chunk == 0
        wp = wp.reshape(O, kh * kw, ipad // chunk, chunk).permute(2, 1, 0, 3)
    return wp.contiguous().to(dtype)


def pack_frag_weight(w, dtype):
    """OIHW float32 -> the fragment-major order of the register-weight / streamed-weight kernels (include/diffsep_hip.h,
    diffsep_frag_index): element (o, tap, i) at ((((i // 64 * taps + tap) * 4 + i % 64 // 16) * (O // 32) + o // 32) * 64
    + (i % 16 // 8) * 32 + o % 32) * 8 + i % 8.  I % 64 == 0, O % 32 == 0."""
    O, I, kh, kw = w.shape
    taps = kh * kw
    assert I % 64 == 0 and O % 32 == 0
    o, t, i = torch.meshgrid(torch.arange(O), torch.arange(taps), torch.arange(I), indexing="ij")
    idx = ((((i // 64 * taps + t) * 4 + (i % 64) // 16) * (O // 32) + o // 32) * 64 + ((i % 16) // 8) * 32 + o % 32) * 8 + i % 8
    out = torch.empty(O * taps * I, dtype=torch.float32)
    out[idx.reshape(-1)] = w.permute(0, 2, 3, 1).reshape(-1).float()
    return out.to(dtype)


def pack_frag_weight_split(w):
    """OIHW float32 -> the split mode's fragment copy (diffsep_frag_index_split): bfloat16 planes hi = bf16(w), lo = bf16(w - hi);
    element (o, tap, i, plane) at ((((i // 32 * taps + tap) * 2 + i % 32 // 16) * 2 + plane) * (O // 32) + o // 32) * 64
    + (i % 16 // 8) * 32 + o % 32) * 8 + i % 8.  I % 32 == 0, O % 32 == 0.  Returns a bfloat16 tensor of 2 O taps I elements."""
    O, I, kh, kw = w.shape
    taps = kh * kw
    assert I % 32 == 0 and O % 32 == 0
    o, t, i = torch.meshgrid(torch.arange(O), torch.arange(taps), torch.arange(I), indexing="ij")
    base = (((i // 32 * taps + t) * 2 + (i % 32) // 16) * 2) * (O // 32)
    tail = (o // 32) * 64 + ((i % 16) // 8) * 32 + o % 32
    wf = w.permute(0, 2, 3, 1).reshape(-1).float()
    hi = wf.to(torch.bfloat16)
    lo = (wf - hi.float()).to(torch.bfloat16)
    out = torch.empty(2 * O * taps * I, dtype=torch.bfloat16)
    out[((base * 64 + tail) * 8 + i % 8).reshape(-1)] = hi
    out[(((base + O // 32) * 64 + tail) * 8 + i % 8).reshape(-1)] = lo
    return out


def conv3x3_streamed(x, w_frag, cout, x2=None, gn=None, bias=None, bias_b=None, skip=None, out_scale=1.0, stats=False, out=None,
                     res=None, ident_frag=None, gn_acc=None):
    """The streamed-weight 3x3 kernels as units (diffsep_conv3x3_streamed).  x [B,H,W,C1] (+ x2 [B,H,W,C2]) dense; 16-bit tensors:
    conv3x3_sw.hip with pack_frag_weight copies; float32 tensors: the split mode's conv3x3_sws.hip with pack_frag_weight_split
    copies (res + ident_frag: residual against the identity copy).  gn = (scale, shift) [B,Cin] f32 -> SiLU(GroupNorm(.)) on the
    fly, or gn_acc = (acc1, acc2 | None, gamma, beta, groups): the same from the producers' accumulators, as conv2d_fused;
    skip = (sx, sx2 | None, sw_frag): folded 1x1 on raw channels."""
    B, H, W, C1 = x.shape
    Cin = C1 + (x2.shape[-1] if x2 is not None else 0)
    y = torch.zeros((B, H, W, cout), dtype=x.dtype, device=x.device) if out is None else out
    sc, sh = _gn_arg(gn)
    st = _stats_arg(stats, B, cout, x.device)
    sx, sx2, swf, sC1, sCin = _skip_arg(skip)
    a1, a2, gam, bet, grp = _gn_acc_arg(gn_acc, 5)
    split = x.dtype == torch.float32
    L = lib("bf16") if split else _L(x)
    call(L, "diffsep_conv3x3_streamed", _ptr(x), _ptr(x2), C1, _ptr(sc), _ptr(sh), _ptr(w_frag), _ptr(bias), _ptr(bias_b),
         _ptr(sx), _ptr(sx2), sC1, sCin, _ptr(swf), _ptr(y), B, H, W, Cin, cout, out_scale, F32_SPLIT if split else _dt(x),
         _ptr(st), _ptr(res), _ptr(ident_frag), _ptr(a1), _ptr(a2), _ptr(gam), _ptr(bet), grp, _stream_ptr())
    return (y, st) if stats is not False else y


def conv3x3_regweight(x, wpacked, cout, x2=None, gn=None, bias=None, bias_b=None, skip=None, res=None, out_scale=1.0, stats=False,
                      w_chunk=0):
    """The register-weight 3x3 kernel as a unit (diffsep_conv3x3_regweight), with its folded 1x1 skip: x (+ x2) dense 16-bit,
    wpacked from pack_conv_weight; gn = (scale, shift) -> SiLU(GroupNorm(.)) on the fly; skip = (sx, sx2 | None, sw [cout, sCin]
    in x's type): raw channels through the centre tap; res: residual (no skip beside it)."""
    B, H, W, C1 = x.shape
    Cin = C1 + (x2.shape[-1] if x2 is not None else 0)
    y = torch.zeros((B, H, W, cout), dtype=x.dtype, device=x.device)
    sc, sh = _gn_arg(gn)
    st = torch.zeros((B, cout, 2), dtype=torch.int64, device=x.device) if stats else None
    sx, sx2, sw, sC1, sCin = _skip_arg(skip)
    call(_L(x), "diffsep_conv3x3_regweight", _ptr(x), _ptr(x2), C1, _ptr(sc), _ptr(sh), _ptr(wpacked), w_chunk, _ptr(bias),
         _ptr(bias_b), _ptr(sx), _ptr(sx2), sC1, sCin, _ptr(sw), _ptr(res), _ptr(y), B, H, W, Cin, cout, out_scale, _dt(x),
         _ptr(st), _stream_ptr())
    return (y, st) if stats else y


def conv2d_chunk(ksize, dtype):
    return lib().diffsep_conv2d_chunk(ksize, _dt_of(dtype))  # (the same in both builds)


def upfirdn2d(x, up):
    B, H, W, Cc = x.shape
    Ho, Wo = _resampled(1 if up else 2, H, W)
    y = torch.empty((B, Ho, Wo, Cc), dtype=x.dtype, device=x.device)
    call(_L(x), "diffsep_upfirdn2d", _ptr(x), _ptr(y), B, H, W, Cc, Cc, Cc, int(up), _dt(x), _stream_ptr())
    return y


def groupnorm_act(x, gamma, beta, groups, eps=1e-6, act=1, resample=0, want_xr=False):
    B, H, W, Cc = x.shape
    Ho, Wo = _resampled(resample, H, W)
    y = torch.empty((B, Ho, Wo, Cc), dtype=x.dtype, device=x.device)
    xr = torch.empty_like(y) if want_xr else None
    ws = torch.empty(B * 64 * Cc * 16 + 2 * B * Cc * 4 + 4096, dtype=torch.uint8, device=x.device)
    call(_L(x), "diffsep_groupnorm_act", _ptr(x), _ptr(gamma), _ptr(beta), _ptr(y), _ptr(xr), B, H, W, Cc, Cc, Cc, Cc, groups,
         eps, act, resample, _dt(x), _ptr(ws), ws.numel(), _stream_ptr())
    return (y, xr) if want_xr else y


def gn_apply(x, scale, shift, act, resample, want_y=True, want_xr=False, route=None, pad=(0, 0, 0)):
    """The GroupNorm-apply / FIR kernels as units on a caller's table (diffsep_gn_apply): y = FIR(act(x * scale + shift)), xr =
    FIR(x); x [B,H,W,C], scale / shift [B,C] f32 or None (the pyramid's pure FIR: want_y=False, want_xr=True).  resample 0 / 1 /
    2 = none / x2 up / x2 down.  route: None = the dispatch's choice, or a key of _lib.GN_ROUTES to force that kernel (an error
    where its shape preconditions do not hold).  pad = extra lanes (ldx, ldy, ldxr) - C of the buffers this wrapper allocates; all
    of x's buffer but x itself, and both outputs entirely, are prefilled with NaN.  Returns (y, xr, ybuf, xrbuf): views of the
    first C lanes and the full buffers (None where not wanted)."""
    B, H, W, Cc = x.shape
    Ho, Wo = _resampled(resample, H, W)
    nan = float("nan")
    xb = torch.full((B, H, W, Cc + pad[0]), nan, dtype=x.dtype, device=x.device)
    xb[..., :Cc] = x
    yb = torch.full((B, Ho, Wo, Cc + pad[1]), nan, dtype=x.dtype, device=x.device) if want_y else None
    xrb = torch.full((B, Ho, Wo, Cc + pad[2]), nan, dtype=x.dtype, device=x.device) if want_xr else None
    call(_L(x), "diffsep_gn_apply", _ptr(xb), _ptr(scale), _ptr(shift), _ptr(yb), _ptr(xrb), B, H, W, Cc, Cc + pad[0],
         Cc + pad[1], Cc + pad[2], int(act), resample, _dt(x), GN_ROUTES[route or "auto"], _stream_ptr())
    return (yb[..., :Cc] if want_y else None, xrb[..., :Cc] if want_xr else None, yb, xrb)


def gn_route_name(kind, resample, affine, dtype, B, H, W, C, pad=(0, 0, 0), has_xr=True, cus=256):
    """name of the kernel the dispatch picks for a GroupNorm-apply / FIR launch in library `kind` on a device of `cus` compute
    units (diffsep_gn_route_name: host arithmetic, nothing is launched and no device is needed); dtype: torch type of the tensors"""
    l = lib(kind)
    name = l.diffsep_gn_route_name(resample, int(affine), _dt_of(dtype), B, H, W, C, C + pad[0], C + pad[1], C + pad[2],
                                   int(has_xr), cus)
    if name is None:
        check(1, l)
    return name.decode()


def conv2d(x, wpacked, bias, cout, ksize, bias_b=None, res=None, out_scale=1.0, cout_pad=None):
    B, H, W, Cin = x.shape
    cp = cout if cout_pad is None else cout_pad
    y = torch.zeros((B, H, W, cp), dtype=x.dtype, device=x.device)
    call(_L(x), "diffsep_conv2d", _ptr(x), _ptr(wpacked), _ptr(bias), _ptr(bias_b), _ptr(res), _ptr(y), B, H, W, Cin, cout,
         ksize, Cin, res.shape[-1] if res is not None else 0, cp, out_scale, _dt(x), _stream_ptr())
    return y


def groupnorm_stats(x, gamma, beta, groups, eps=1e-6, x2=None):
    """scale, shift [B,C] fp32 of GroupNorm over x (or over cat([x, x2], channel) read in place)."""
    B, H, W, C1 = x.shape
    Cc = C1 + (x2.shape[-1] if x2 is not None else 0)
    scale = torch.empty((B, Cc), dtype=torch.float32, device=x.device)
    shift = torch.empty_like(scale)
    ws = torch.empty(B * 64 * Cc * 16 + 4096, dtype=torch.uint8, device=x.device)
    call(_L(x), "diffsep_groupnorm_stats", _ptr(x), _ptr(x2), C1, _ptr(gamma), _ptr(beta), _ptr(scale), _ptr(shift), B, H, W,
         Cc, C1, x2.shape[-1] if x2 is not None else 0, groups, eps, _dt(x), _ptr(ws), ws.numel(), _stream_ptr())
    return scale, shift


STAT_SUM_SCALE, STAT_SQ_SCALE = 2.0 ** 24, 2.0 ** 16  # fixed-point scales of the GroupNorm accumulators


def conv2d_fused(x, wpacked, bias, cout, ksize, x2=None, gn=None, gn_act=1, bias_b=None, res=None, out_scale=1.0,
                 cout_pad=None, out=None, stats=False, w_chunk=0, gn_acc=None, split=False):
    """stats=True additionally returns the int64 channel-sum accumulators [B,cout,2] of the output (sum * 2^24,
    sum of squares * 2^16); stats=<tensor> adds into it.  gn_acc=(acc1, acc2|None, gamma, beta, groups): GroupNorm of
    the input from such accumulators instead of gn=(scale, shift)."""
    B, H, W, C1 = x.shape
    Cin = C1 + (x2.shape[-1] if x2 is not None else 0)
    cp = cout if cout_pad is None else cout_pad
    y = torch.zeros((B, H, W, cp), dtype=x.dtype, device=x.device) if out is None else out
    sc, sh = _gn_arg(gn)
    st = _stats_arg(stats, B, cout, x.device)
    a1, a2, gam, bet, grp = _gn_acc_arg(gn_acc, 5)
    call(_L(x), "diffsep_conv2d_fused", _ptr(x), _ptr(x2), C1, _ptr(sc), _ptr(sh), gn_act, _ptr(wpacked), _ptr(bias),
         _ptr(bias_b), _ptr(res), _ptr(y), B, H, W, Cin, cout, ksize, C1, x2.shape[-1] if x2 is not None else 0,
         res.shape[-1] if res is not None else 0, cp, out_scale, _dts(x, split), _ptr(st), w_chunk, _ptr(a1), _ptr(a2), _ptr(gam),
         _ptr(bet), grp, _stream_ptr())
    return (y, st) if stats is not False else y


def stats_to_float(st):
    """int64 accumulators [B,C,2] -> float64 (sum, sum of squares)."""
    out = st.double()
    out[..., 0] /= STAT_SUM_SCALE
    out[..., 1] /= STAT_SQ_SCALE
    return out


def groupnorm_from_acc(sa, sb, gamma, beta, groups, npix, eps=1e-6):
    """scale, shift [B,C] fp32 from the int64 accumulators sa [B,C1,2] (+ sb [B,C2,2] | None: the concat of two tensors of npix
    pixels) through the finalize launch: the table a convolution given gn_acc=... builds in its own prologue, bit for bit
    (tests/test_gn_table_gpu.py)."""
    B, C1 = sa.shape[:2]
    C2 = sb.shape[1] if sb is not None else 0
    scale = torch.empty((B, C1 + C2), dtype=torch.float32, device=sa.device)
    shift = torch.empty_like(scale)
    call(lib(), "diffsep_gn_finalize_acc", _ptr(sa), C1, _ptr(sb), C2, B, npix, groups, eps, _ptr(gamma), _ptr(beta),
         _ptr(scale), _ptr(shift), _stream_ptr())
    return scale, shift


def attn_fused(x, wqk, wv, wo, bqk, bv, bo, gn=None, gn_acc=None, stats=False, out=None):
    """The fused attention block's kernel as a unit (diffsep_attn_fused): x [B,L,128] 16-bit, wqk / wv / wo [128*128] in the
    fragment-major order of pack_frag_weight (1x1), biases [128] f32; gn = (scale, shift) [B,128] or gn_acc = (acc, gamma, beta,
    groups).  stats=True additionally returns the int64 accumulators [B,128,2] of the output, stats=<tensor> adds into it, as
    conv2d_fused; out=<tensor>: the output buffer (dense, x's type, at least B samples of [L,128]: the first B are written)."""
    B, L, Cc = x.shape
    if out is not None and (out.dtype != x.dtype or out.device != x.device or not out.is_contiguous() or out.dim() != 3
                            or out.shape[0] < B or tuple(out.shape[1:]) != (L, Cc)):
        raise ValueError("attn_fused: out must be a dense [>= B, L, C] tensor of x's type on x's device")
    y = torch.empty_like(x) if out is None else out
    st = _stats_arg(stats, B, Cc, x.device)
    if stats is not True and stats is not False and (st.dtype != torch.int64 or not st.is_contiguous() or st.dim() != 3
                                                     or st.shape[0] < B or tuple(st.shape[1:]) != (Cc, 2)):
        raise ValueError("attn_fused: stats must be a dense int64 [>= B, C, 2] tensor")
    sc, sh = _gn_arg(gn)
    acc, gam, bet, grp = _gn_acc_arg(gn_acc, 4)
    call(_L(x), "diffsep_attn_fused", _ptr(x), _ptr(acc), _ptr(gam), _ptr(bet), grp, _ptr(sc), _ptr(sh), _ptr(wqk), _ptr(wv),
         _ptr(wo), _ptr(bqk), _ptr(bv), _ptr(bo), _ptr(y), _ptr(st), B, L, Cc, _stream_ptr())
    return (y, st) if stats is not False else y


def last_conv_kernel(kind="bf16"):
    """name of the kernel instantiation the calling thread's last convolution launch ran in library `kind`"""
    return lib(kind).diffsep_last_conv_kernel().decode()


def gemm_nt(a, bt, N, B=None, bias=None, bias_mode=0, div_b=None, res=None, out_scale=1.0, out=None, split=False):
    """The general one-tap launch of conv_mfma.hip (diffsep_gemm_nt): y[b, m, n] = ((sum_k a[b | shared, m, k] bt[b | shared, n, k])
    / div_b[b] + bias + res[b, m, n]) * out_scale.  a [B,M,lda] or [M,lda] (shared by the batch), bt dense [B,N,K] or [N,K] (shared;
    K <= lda), bias f32 [N] (bias_mode 0) or [M] (bias_mode 1), div_b f32 [B], res [B,M,ldr].  out=<tensor> [B,M,ldy]: the output
    buffer (ldy >= N rounded up to 8: the launch writes columns [0, that) and nothing else); default zeros of that width.
    B: the batch size when both operands are shared."""
    a_b, bt_b = a.dim() == 3, bt.dim() == 3
    if B is None:
        B = a.shape[0] if a_b else (bt.shape[0] if bt_b else 1)
    M, lda = a.shape[-2:]
    K = bt.shape[-1]
    if bt.shape[-2] != N or not (a.is_contiguous() and bt.is_contiguous()) or (a_b and a.shape[0] != B) or (bt_b and bt.shape[0] != B):
        raise ValueError("gemm_nt: a [B,M,lda] | [M,lda] and bt [B,N,K] | [N,K] dense, with one batch size")
    y = torch.zeros((B, M, (N + 7) // 8 * 8), dtype=a.dtype, device=a.device) if out is None else out
    if tuple(y.shape[:2]) != (B, M) or not y.is_contiguous() or (res is not None and (tuple(res.shape[:2]) != (B, M) or not res.is_contiguous())):
        raise ValueError("gemm_nt: out and res must be dense [B,M,ld] tensors")
    if (bias is not None and bias.numel() != (M if bias_mode else N)) or (div_b is not None and div_b.numel() != B):
        raise ValueError("gemm_nt: bias is [N] (bias_mode 0) or [M] (bias_mode 1), div_b [B]")
    call(_L(a), "diffsep_gemm_nt", _ptr(a), _ptr(bt), _ptr(bias), _ptr(div_b), _ptr(res), _ptr(y), B, M, N, K, lda,
         res.shape[-1] if res is not None else 0, y.shape[-1], int(a_b), int(bt_b), bias_mode, out_scale, _dts(a, split), _stream_ptr())
    return y


def attention_workspace_bytes(B, L, element_size):
    """(bytes of one of the two regions of diffsep_attention's workspace — scores, then probabilities —, bytes of both)"""
    one = (B * L * ((L + 7) // 8 * 8) * element_size + 255) // 256 * 256
    return one, 2 * one


def attention(q, k, vt, split=False, return_workspace=False, workspace=None):
    """split=True (fp32 tensors only): both GEMMs with bf16x3 products (DIFFSEP_F32_SPLIT).  return_workspace=True additionally
    returns the scores and the probabilities [B,L,Lp] (q's type) as views of the workspace; workspace=<uint8 tensor>: the caller's
    buffer of at least attention_workspace_bytes(...)[1] bytes."""
    B, L, Cc = q.shape
    Lp = (L + 7) // 8 * 8
    assert vt.shape == (B, Cc, Lp)
    o = torch.empty_like(q)
    one, both = attention_workspace_bytes(B, L, q.element_size())
    ws = torch.empty(both, dtype=torch.uint8, device=q.device) if workspace is None else workspace
    if ws.dtype != torch.uint8 or not ws.is_contiguous() or ws.numel() < both or ws.data_ptr() % 16:
        raise ValueError("attention: workspace must be a dense 16-byte aligned uint8 tensor of attention_workspace_bytes(...)[1] bytes")
    call(_L(q), "diffsep_attention", _ptr(q), _ptr(k), _ptr(vt), _ptr(o), B, L, Cc, Cc, _dts(q, split), _ptr(ws), ws.numel(),
         _stream_ptr())
    if not return_workspace:
        return o
    n = B * L * Lp * q.element_size()
    scores, probs = (ws[i * one:i * one + n].view(q.dtype).view(B, L, Lp) for i in (0, 1))
    return o, scores, probs


def resblock_forward(params, x, temb, out_ch, up=False, down=False):
    """ResnetBlockBigGANpp through the engine's block code.  params: list of float32 arrays in reference state_dict
    order; x [B,H,W,Cin] NHWC, temb [B,D] f32 -> [B,H',W',out_ch]."""
    B, H, W, cin = x.shape
    blob = _params_blob(params)
    Ho, Wo = _resampled(1 if up else (2 if down else 0), H, W)
    y = torch.empty((B, Ho, Wo, out_ch), dtype=x.dtype, device=x.device)
    call(_L(x), "diffsep_resblock_forward", cin, out_ch, int(up), int(down), temb.shape[1], _dt(x),
         blob.ctypes.data_as(C.c_void_p), blob.size, _ptr(x.contiguous()), _ptr(temb.contiguous()), _ptr(y), B, H, W,
         _stream_ptr())
    return y


def attnblock_forward(params, x):
    """AttnBlockpp through the engine's block code.  params: GroupNorm_0.{weight,bias}, NIN_0..3.{W,b}."""
    B, H, W, Cc = x.shape
    blob = _params_blob(params)
    y = torch.empty_like(x)
    call(_L(x), "diffsep_attnblock_forward", Cc, _dt(x), blob.ctypes.data_as(C.c_void_p), blob.size, _ptr(x.contiguous()),
         _ptr(y), B, H, W, _stream_ptr())
    return y


def stft_pack(xt, mix, W, cpad, n_fft=510, hop=128, exponent=0.5, factor=0.33, shift=False, dtype=torch.float32, split=False):
    """diffsep_stft_pack_ex.  split=True: the DFT matrix product of the three-launch route with bf16x3 products (the fused kernel of
    the 16-bit types ignores it).  last_conv_kernel() names the kernel afterwards."""
    B, S, T = xt.shape
    y = torch.empty((B, n_fft // 2 + 1, W, cpad), dtype=dtype, device=xt.device)
    F_ = 1 + (T + n_fft - hop) // hop
    ws = torch.empty(2 * ((B * (S + 1) * F_ + 8) * 512 + 64), dtype=torch.float32, device=xt.device)
    call(_L(y), "diffsep_stft_pack_ex", _ptr(xt), _ptr(mix), _ptr(y), B, S, T, n_fft, hop, exponent, factor, W, cpad,
         int(shift), _dt_of(dtype), _ptr(ws), ws.numel() * 4, _stream_ptr(), int(bool(split)))
    return y


def istft_unpack(x, S, T, n_fft=510, hop=128, exponent=0.5, factor=0.33, split=False, ow=None, ob=None, tdiv=None, out=None):
    """diffsep_istft_unpack_ex.  ow [2S, ow_cin], ob [2S], tdiv [B] (float32, on x's device): the network's output layer
    v = (ow x) / tdiv[b] + ob applied to every pixel first; all three or none.  out: a float32 [>= B, S, T] tensor to write into."""
    B, H, W, cpad = x.shape
    F_ = 1 + (T + n_fft - hop) // hop
    if out is None:
        out = torch.empty((B, S, T), dtype=torch.float32, device=x.device)
    elif out.dtype != torch.float32 or not out.is_contiguous() or out.shape[0] < B or tuple(out.shape[1:]) != (S, T):
        raise ValueError("istft_unpack: out must be a dense float32 [>= B, S, T] tensor")
    ws = torch.empty(2 * (B * S * F_ * 512 + 64), dtype=torch.float32, device=x.device)
    ow_cin = 0
    if ow is not None:
        if ob is None or tdiv is None:
            raise ValueError("istft_unpack: ow, ob and tdiv come together")
        for t_, shp in ((ow, (2 * S, ow.shape[-1])), (ob, (2 * S,)), (tdiv, (B,))):
            if t_.dtype != torch.float32 or not t_.is_contiguous() or tuple(t_.shape) != shp or t_.device != x.device:
                raise ValueError("istft_unpack: ow [2S, ow_cin], ob [2S], tdiv [B] must be dense float32 tensors on x's device")
        ow_cin = ow.shape[1]
    call(_L(x), "diffsep_istft_unpack_ex", _ptr(x), _ptr(out), B, S, T, n_fft, hop, exponent, factor, W, cpad, _dt(x), _ptr(ws),
         ws.numel() * 4, _stream_ptr(), int(bool(split)), _ptr(ow), _ptr(ob), _ptr(tdiv), ow_cin)
    return out


def sde_sigma_mix(mix, avg_len=510):
    """PriorMixSDE per-sample noise scale: mix [B,1,T] -> [B,T]."""
    B, _, T = mix.shape
    out = torch.empty((B, T), dtype=torch.float32, device=mix.device)
    call(lib(), "diffsep_sde_sigma_mix", _ptr(mix), _ptr(out), B, T, avg_len, _stream_ptr())
    return out


def sde_prior(sde, y, z, sigma_mix=None):
    B, S, T = z.shape
    x = torch.empty_like(z)
    call(lib(), "diffsep_sde_prior", C.byref(sde_config(sde)), _ptr(y), _ptr(z), _ptr(x), B, S, T, _ptr(sigma_mix),
         _stream_ptr())
    return x


def sde_corrector_update(sde, snr, x, t, score, z, sigma_mix=None, variant=0):
    """variant 0: ald2, 1: ald."""
    B, S, T = x.shape
    xo, xm = torch.empty_like(x), torch.empty_like(x)
    call(lib(), "diffsep_sde_corrector_update", C.byref(sde_config(sde)), snr, _ptr(x), _ptr(t), _ptr(score), _ptr(z), _ptr(xo),
         _ptr(xm), B, S, T, _ptr(sigma_mix), variant, _stream_ptr())
    return xo, xm


def sde_predictor_update(sde, N, x, t, score, z, sigma_mix=None, probability_flow=False):
    B, S, T = x.shape
    xo, xm = torch.empty_like(x), torch.empty_like(x)
    call(lib(), "diffsep_sde_predictor_update", C.byref(sde_config(sde)), N, _ptr(x), _ptr(t), _ptr(score), _ptr(z), _ptr(xo),
         _ptr(xm), B, S, T, _ptr(sigma_mix), int(bool(probability_flow)), _stream_ptr())
    return xo, xm


def sde_coefficients(sde, x, t, sigma_mix=None, f_scale=1.0, g_scale=1.0):
    """(f_scale * drift [B,S,T], g_scale * diffusion): diffusion is [B] for MixSDE, [B,S,T] for PriorMixSDE."""
    B, S, T = x.shape
    drift = torch.empty_like(x)
    diff = torch.empty_like(x) if sigma_mix is not None else torch.empty(B, dtype=torch.float32, device=x.device)
    call(lib(), "diffsep_sde_coefficients", C.byref(sde_config(sde)), _ptr(x), _ptr(t), _ptr(sigma_mix), _ptr(drift),
         _ptr(diff), B, S, T, f_scale, g_scale, _stream_ptr())
    return drift, diff


def sde_mean(sde, x0, t):
    B, S, T = x0.shape
    out = torch.empty_like(x0)
    call(lib(), "diffsep_sde_mean", C.byref(sde_config(sde)), _ptr(x0), _ptr(t), _ptr(out), B, S, T, _stream_ptr())
    return out


def sde_std(sde, t, S, T=1, sigma_mix=None):
    """Dense matrix square root of the perturbation covariance: [B,S,S], or [B,S,S,T] with sigma_mix [B,T]."""
    B = t.shape[0]
    shape = (B, S, S, T) if sigma_mix is not None else (B, S, S)
    out = torch.empty(shape, dtype=torch.float32, device=t.device)
    call(lib(), "diffsep_sde_std", C.byref(sde_config(sde)), _ptr(t), _ptr(sigma_mix), _ptr(out), B, S, T, _stream_ptr())
    return out


def sde_mult_std(std, x):
    """std [B,S,S] or [B,S,S,T] applied to x [B,S,T]."""
    B, S, T = x.shape
    per = std.dim() == 4
    assert std.shape == ((B, S, S, T) if per else (B, S, S)), "std must be [B,S,S] or [B,S,S,T]"
    out = torch.empty_like(x)
    call(lib(), "diffsep_sde_mult_std", _ptr(std.contiguous()), _ptr(x), _ptr(out), B, S, T, int(per), _stream_ptr())
    return out


def sde_mult_std_inv(std, x):
    """std^-1 x for a dense std [B,S,S] or [B,S,S,T] and x [B,S,T] (MixSDE / PriorMixSDE.mult_std_inv)."""
    B, S, T = x.shape
    per = std.dim() == 4
    assert std.shape == ((B, S, S, T) if per else (B, S, S)), "std must be [B,S,S] or [B,S,S,T]"
    out = torch.empty_like(x)
    call(lib(), "diffsep_sde_mult_std_inv", _ptr(std.contiguous()), _ptr(x), _ptr(out), B, S, T, int(per), _stream_ptr())
    return out


def sde_reverse_drift(f, G, score, probability_flow=False):
    """rev_f = f - G^2 score (x 0.5 for the probability-flow ODE); G [B] or the shape of f."""
    B = f.shape[0]
    n = f.numel() // B
    full = G.numel() != B
    assert (not full) or G.shape == f.shape
    out = torch.empty_like(f)
    call(lib(), "diffsep_sde_reverse_drift", _ptr(f), _ptr(G.contiguous()), _ptr(score), _ptr(out), B, n, int(full),
         int(bool(probability_flow)), _stream_ptr())
    return out


def sde_langevin_update(snr, x, score, z):
    B = x.shape[0]
    n = x.numel() // B
    xo, xm = torch.empty_like(x), torch.empty_like(x)
    ws = torch.empty(16 * B + 64, dtype=torch.uint8, device=x.device)
    call(lib(), "diffsep_sde_langevin_update", snr, _ptr(x), _ptr(score), _ptr(z), _ptr(xo), _ptr(xm), B, n, _ptr(ws),
         ws.numel(), _stream_ptr())
    return xo, xm


def normalize_batch(mix):
    B, _, T = mix.shape
    out = torch.empty_like(mix)
    mean = torch.empty(B, dtype=torch.float32, device=mix.device)
    std = torch.empty(B, dtype=torch.float32, device=mix.device)
    call(lib(), "diffsep_normalize_batch", _ptr(mix), _ptr(out), _ptr(mean), _ptr(std), B, T, _stream_ptr())
    return out, mean.view(B, 1, 1), std.view(B, 1, 1)


def scale_output(mix, sep):
    B, S, T = sep.shape
    out = sep.clone()
    call(lib(), "diffsep_scale_output", _ptr(mix), _ptr(out), B, S, T, _stream_ptr())
    return out


def time_embedding(t, fourier_w, w1, b1, w2, b2):
    """NCSNpp's time embedding (ncsnpp.py:324-343): t [B] -> temb [B, 4 nf]; all float32 device tensors."""
    B, nf = t.shape[0], fourier_w.shape[0]
    ts = [x.contiguous().float() for x in (t, fourier_w, w1, b1, w2, b2)]
    out = torch.empty((B, 4 * nf), dtype=torch.float32, device=t.device)
    ws = torch.empty(B * 6 * nf, dtype=torch.float32, device=t.device)
    call(lib(), "diffsep_time_embedding", *[_ptr(x) for x in ts], _ptr(out), B, nf, _ptr(ws), ws.numel() * 4, _stream_ptr())
    return out


def dense_projection(x, weights, biases=None, silu_in=True):
    """y [B, sum O_i] = act(x) W_i^T + b_i for nn.Linear weights [O_i, K] side by side (the engine's Dense_0 projection of the
    time embedding: diffsep_dense_projection); x [B, K] float32, biases: one [O_i] per block, or None for no bias at all."""
    B, K = x.shape
    outs = [int(w.shape[0]) for w in weights]
    assert all(w.shape == (o, K) for w, o in zip(weights, outs)) and (biases is None or [int(b.shape[0]) for b in biases] == outs)
    total = sum(outs)
    w = torch.cat([wi.contiguous().float() for wi in weights], 0)
    b = torch.cat([bi.contiguous().float() for bi in biases]) if biases is not None else None
    y = torch.empty((B, total), dtype=torch.float32, device=x.device)
    ws = torch.empty(max(1, K * total), dtype=torch.float32, device=x.device)
    oc, ocp = host_array(outs, np.int32, len(outs), "out_ch")
    call(lib(), "diffsep_dense_projection", _ptr(x.contiguous()), _ptr(w), _ptr(b), ocp, len(outs), _ptr(y), B, K,
         int(bool(silu_in)), _ptr(ws), ws.numel() * 4, _stream_ptr())
    return y


def convert(src, dst_dtype, kind="bf16"):
    """diffsep_convert of the library build `kind` ("bf16" | "f16": what dtype code 1 stores): a flat float32 or 16-bit tensor
    to float32 or that build's 16-bit type, round to nearest even."""
    half = torch.bfloat16 if kind == "bf16" else torch.float16
    if src.dtype not in (torch.float32, half) or dst_dtype not in (torch.float32, half):
        raise TypeError(f"float32 or {half} expected in the {kind} build")
    src = src.contiguous()
    dst = torch.empty(src.shape, dtype=dst_dtype, device=src.device)
    call(lib(kind), "diffsep_convert", _ptr(src), _ptr(dst), src.numel(), _dt_of(src.dtype), _dt_of(dst_dtype), _stream_ptr())
    return dst


def randn(n, seed, stream_id, device="cuda"):
    out = torch.empty(n, dtype=torch.float32, device=device)
    call(lib(), "diffsep_randn", _ptr(out), n, seed, stream_id, _stream_ptr())
    return out


def randn_batch(B, S, T, seeds, lengths, stream_id, device="cuda"):
    """[B,S,T] draws: row (b, s) = values s*len_b .. of randn(S*len_b, seeds[b], stream_id), zero beyond len_b."""
    out = torch.empty((B, S, T), dtype=torch.float32, device=device)
    sd = torch.as_tensor(np.asarray(seeds, dtype=np.uint64).view(np.int64), device=device)
    ln = torch.as_tensor(np.asarray(lengths, dtype=np.int32), device=device)
    call(lib(), "diffsep_randn_batch", _ptr(out), B, S, T, _ptr(sd), _ptr(ln), stream_id, _stream_ptr())
    return out


def gram(ref, est):
    """[B,S,T] x2 -> float64 [B,3,S,S] = (ref ref^T, ref est^T, est est^T)."""
    B, S, T = ref.shape
    out = torch.empty((B, 3, S, S), dtype=torch.float64, device=ref.device)
    call(lib(), "diffsep_gram", _ptr(ref.contiguous()), _ptr(est.contiguous()), _ptr(out), B, S, T, _stream_ptr())
    return out


def longform_plan(T, Tw, Tv):
    """Window starts of a T-sample file cut into windows of Tw samples with a nominal overlap of Tv (diffsep_longform_plan:
    host arithmetic, no device needed; raises for a request it refuses: T < 1, Tv < 1 or 3 Tv > Tw).  T <= Tw: [0]."""
    l = lib()
    K = l.diffsep_longform_plan(int(T), int(Tw), int(Tv), None, 0)
    check(0 if K >= 1 else 1, l)
    starts = (C.c_int64 * K)()
    if l.diffsep_longform_plan(int(T), int(Tw), int(Tv), starts, K) != K:
        check(1, l)
    return list(starts)


def longform_stitch(win, T, Tv, want_gram=False, out=None):
    """diffsep_longform_stitch: win [K,S,Tw] float32 device tensor, the K windows of longform_plan(T, Tw, Tv) -> (out [S,T]
    float32, perm [K,S] int32[, gram [K-1,S,S] float64]): windows aligned by the source permutation of least squared distance
    over each overlap (perm[k][i] = the row of window k that is output source i), cross-faded over the seams.  Asynchronous on
    the current stream, no readback.  out: a dense float32 [S,T] tensor to write into (every element is written)."""
    if win.dim() != 3 or win.dtype != torch.float32 or not win.is_cuda:
        raise ValueError("longform_stitch: win must be a float32 [K,S,Tw] device tensor")
    win = win.contiguous()
    K, S, Tw = win.shape
    l = lib()
    nbytes = _workspace_bytes(l.diffsep_longform_workspace_bytes, K, S)
    if out is None:
        out = torch.empty((S, int(T)), dtype=torch.float32, device=win.device)
    elif out.dtype != torch.float32 or not out.is_contiguous() or tuple(out.shape) != (S, int(T)) or out.device != win.device:
        raise ValueError("longform_stitch: out must be a dense float32 [S,T] tensor on win's device")
    perm = torch.empty((K, S), dtype=torch.int32, device=win.device)
    gram_ = torch.empty((max(K - 1, 0), S, S), dtype=torch.float64, device=win.device) if want_gram else None
    ws = torch.empty(nbytes, dtype=torch.uint8, device=win.device)
    call(l, "diffsep_longform_stitch", _ptr(win), K, S, Tw, int(T), int(Tv), _ptr(out), _ptr(perm), _ptr(gram_) if (want_gram
         and K > 1) else None, _ptr(ws), nbytes, _stream_ptr())
    return (out, perm, gram_) if want_gram else (out, perm)


class EnsembleResult:
    """what ops.ensemble leaves on the device: mean [B,S,T] float32, std / pick [B,S,T] float32 or None, perm [B,K,S] int32
    (aligned source i of draw k is its row perm[b,k,i]), dist [B,K] float64, medoid [B] int32, gram [B,K,S,S] float64 or None"""
    __slots__ = ("mean", "std", "pick", "perm", "dist", "medoid", "gram")

    def __init__(self, mean, std, pick, perm, dist, medoid, gram):
        self.mean, self.std, self.pick, self.perm, self.dist, self.medoid, self.gram = mean, std, pick, perm, dist, medoid, gram

    def aligned(self, draws):
        """draws [B,K,S,T] with every draw's sources in the common order (a gather by perm)"""
        return torch.gather(draws, 2, self.perm.long()[..., None].expand_as(draws))


def ensemble_workspace_bytes(B, K, S):
    """bytes of workspace diffsep_ensemble needs (host arithmetic; raises for a shape it refuses)"""
    return _workspace_bytes(lib().diffsep_ensemble_workspace_bytes, B, K, S)


def ensemble(draws, lengths=None, anchor=None, want_std=False, want_pick=False, want_gram=False, out=None):
    """diffsep_ensemble: draws [B,K,S,T] float32 device tensor, K posterior draws of each of B zero-padded utterances of
    lengths[b] (default T) samples -> EnsembleResult.  Every draw's sources are permuted to the order of least squared distance
    to anchor [B,S,T] (default: draw 0 of the utterance), then reduced over the draws in float64: the mean, with want_std the
    population standard deviation, every draw's squared distance to the mean, the medoid (the draw nearest to the mean) and with
    want_pick that draw itself, aligned; want_gram: the cross-Grams the permutations were chosen from.  Samples beyond a length
    are never read and come out as zeros.  Asynchronous on the current stream, no readback, no synchronisation.  out: a dense
    float32 [B,S,T] tensor for the mean (every element is written)."""
    if draws.dim() != 4 or draws.dtype != torch.float32 or not draws.is_cuda:
        raise ValueError("ensemble: draws must be a float32 [B,K,S,T] device tensor")
    draws = draws.contiguous()
    B, K, S, T = draws.shape
    dev = draws.device
    if anchor is not None:
        if tuple(anchor.shape) != (B, S, T) or anchor.dtype != torch.float32 or anchor.device != dev:
            raise ValueError("ensemble: anchor must be a float32 [B,S,T] tensor on draws' device")
        anchor = anchor.contiguous()
    ln = None if lengths is None else _dev_i32(lengths, dev)
    if ln is not None and ln.numel() != B:
        raise ValueError("ensemble: lengths must have B entries")
    nbytes = ensemble_workspace_bytes(B, K, S)
    if out is None:
        out = torch.empty((B, S, T), dtype=torch.float32, device=dev)
    elif out.dtype != torch.float32 or not out.is_contiguous() or tuple(out.shape) != (B, S, T) or out.device != dev:
        raise ValueError("ensemble: out must be a dense float32 [B,S,T] tensor on draws' device")
    std = torch.empty((B, S, T), dtype=torch.float32, device=dev) if want_std else None
    pick = torch.empty((B, S, T), dtype=torch.float32, device=dev) if want_pick else None
    perm = torch.empty((B, K, S), dtype=torch.int32, device=dev)
    dist = torch.empty((B, K), dtype=torch.float64, device=dev)
    medoid = torch.empty((B,), dtype=torch.int32, device=dev)
    gram_ = torch.empty((B, K, S, S), dtype=torch.float64, device=dev) if want_gram else None
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    call(lib(), "diffsep_ensemble", _ptr(draws), _ptr(anchor), _ptr(ln), B, K, S, T, _ptr(out), _ptr(std), _ptr(pick), _ptr(perm),
         _ptr(dist), _ptr(medoid), _ptr(gram_), _ptr(ws), nbytes, _stream_ptr())
    return EnsembleResult(out, std, pick, perm, dist, medoid, gram_)


def _dev_i32(v, device):
    """host list / array or tensor -> contiguous int32 device tensor (host values through pinned memory on the current
    stream: a pageable copy would stall every other stream's work)"""
    if isinstance(v, torch.Tensor) and v.is_cuda:
        return v.to(torch.int32).contiguous()
    h = torch.as_tensor(np.ascontiguousarray(np.asarray(v.cpu() if isinstance(v, torch.Tensor) else v, dtype=np.int32)))
    return h.pin_memory().to(device, non_blocking=True)


def _workspace_bytes(fn, *shape):
    """what a *_workspace_bytes entry of the library answers for the shape, or the error it raises"""
    n = fn(*(int(v) for v in shape))
    check(0 if n >= 0 else 1)
    return int(n)


def _pair_call(name, ref, est, lengths, perm):
    """a [B,S,T] pair call (estimate row perm[b][i] against reference row i over lengths[b] samples) validated:
    -> (ref, est, B, S, T, lengths_dev, perm_dev), float32 contiguous / int32 device tensors or None"""
    if ref.shape != est.shape or ref.dim() != 3:
        raise ValueError(f"{name}: ref and est must be [B,S,T] tensors of one shape")
    B, S, T = ref.shape
    ref, est = ref.float().contiguous(), est.float().contiguous()
    ln = None if lengths is None else _dev_i32(lengths, ref.device)
    pm = None if perm is None else _dev_i32(perm, ref.device)
    if ln is not None and ln.numel() != B:
        raise ValueError(f"{name}: lengths must have B entries")
    if pm is not None and tuple(pm.shape) != (B, S):
        raise ValueError(f"{name}: perm must be [B,S]")
    return ref, est, B, S, T, ln, pm


def stoi_workspace_bytes(B, S, T, fs):
    """bytes of workspace diffsep_stoi needs (host arithmetic; raises for a sample rate or shape it refuses)"""
    return _workspace_bytes(lib().diffsep_stoi_workspace_bytes, B, S, T, fs)


def stoi(ref, est, fs, extended=True, lengths=None, perm=None):
    """STOI (extended: ESTOI) of every source of a zero-padded batch on the device: ref, est [B,S,T] float32 device tensors ->
    float64 [B,S] device tensor; estimate row perm[b][i] (default i) against reference row i over the first lengths[b]
    (default T) samples.  The algorithm of metrics.stoi in float64 (csrc/stoi.hip); asynchronous on the current stream."""
    ref, est, B, S, T, ln, pm = _pair_call("stoi", ref, est, lengths, perm)
    nbytes = stoi_workspace_bytes(B, S, T, fs)
    out = torch.empty((B, S), dtype=torch.float64, device=ref.device)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=ref.device)
    call(lib(), "diffsep_stoi", _ptr(ref), _ptr(est), _ptr(out), B, S, T, _ptr(ln), _ptr(pm), int(fs), int(bool(extended)),
         _ptr(ws), nbytes, _stream_ptr())
    return out


def composite_workspace_bytes(B, S, T, fs):
    """bytes of workspace diffsep_composite needs (host arithmetic; raises for a sample rate or shape it refuses)"""
    return _workspace_bytes(lib().diffsep_composite_workspace_bytes, B, S, T, fs)


def composite(ref, est, fs=16000, lengths=None, perm=None, frames=False):
    """LLR / WSS / segmental SNR (the ingredients of CSIG / CBAK / COVL) of every source of a zero-padded batch on the device:
    ref, est [B,S,T] float32 device tensors -> float64 [B,S,4] device tensor {llr_mean, wss_dist, segsnr, n_frames}; estimate
    row perm[b][i] (default i) against reference row i over the first lengths[b] (default T) samples.  frames=True: also the
    per-frame values, float64 [B,S,3,F] {llr, wss, segsnr} in frame order with F = the frame count of T (NaN beyond a row's
    own count).  The algorithm of metrics.composite in float64 (csrc/composite.hip); asynchronous on the current stream."""
    ref, est, B, S, T, ln, pm = _pair_call("composite", ref, est, lengths, perm)
    nbytes = composite_workspace_bytes(B, S, T, fs)
    out = torch.empty((B, S, 4), dtype=torch.float64, device=ref.device)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=ref.device)
    fr, cap = None, 0
    if frames:
        from . import metrics  # (metrics imports this module: resolved at the call, no cycle)
        cap = max(1, metrics.composite_num_frames(T, fs))
        fr = torch.full((B, S, 3, cap), float("nan"), dtype=torch.float64, device=ref.device)
    call(lib(), "diffsep_composite", _ptr(ref), _ptr(est), _ptr(out), _ptr(fr), cap, B, S, T, _ptr(ln), _ptr(pm), int(fs),
         _ptr(ws), nbytes, _stream_ptr())
    return (out, fr) if frames else out


BSS_EVAL_WORKSPACE_CAP = 1 << 29  # bytes of workspace one diffsep_bss_eval call of bss_eval() may take (512 MiB)


def bss_eval_workspace_bytes(B, S, T, L):
    """bytes of workspace diffsep_bss_eval needs (host arithmetic; raises for a shape it refuses)"""
    return _workspace_bytes(lib().diffsep_bss_eval_workspace_bytes, B, S, T, L)


def bss_eval(ref, est, filter_length=512, clamp_db=0.0, lengths=None, perm=None):
    """BSS-eval SDR / SIR / SAR with a filter_length-tap distortion filter of every utterance of a zero-padded batch on the
    device: ref, est [B,S,T] float32 device tensors -> (out float64 [B,3,S] {sdr, sir, sar} per source, pairs float64
    [B,2,S,S] the SDR and SIR tables [reference][estimate], perm int32 [B,S]) device tensors; perm None: searched (largest mean
    clamped SDR).  The algebra of metrics.bss_eval_host in float64 (csrc/bss_eval.hip); asynchronous on the current stream.  A
    batch whose workspace would exceed BSS_EVAL_WORKSPACE_CAP goes as several calls (a row's result does not depend on its
    batch); one utterance always goes, whatever it needs."""
    ref, est, B, S, T, ln, pm = _pair_call("bss_eval", ref, est, lengths, perm)
    L = int(filter_length)
    per = max(1, bss_eval_workspace_bytes(1, S, T, L))
    step = max(1, min(B, BSS_EVAL_WORKSPACE_CAP // per))
    dev = ref.device
    out = torch.empty((B, 3, S), dtype=torch.float64, device=dev)
    pairs = torch.empty((B, 2, S, S), dtype=torch.float64, device=dev)
    pout = torch.empty((B, S), dtype=torch.int32, device=dev)
    ws = torch.empty(bss_eval_workspace_bytes(step, S, T, L), dtype=torch.uint8, device=dev)
    for b0 in range(0, B, step):
        nb = min(step, B - b0)
        call(lib(), "diffsep_bss_eval", _ptr(ref[b0:]), _ptr(est[b0:]), _ptr(out[b0:]), _ptr(pairs[b0:]), _ptr(pout[b0:]), nb, S, T,
             _ptr(None if ln is None else ln[b0:]), _ptr(None if pm is None else pm[b0:]), L, float(clamp_db), _ptr(ws),
             ws.numel(), _stream_ptr())
    return out, pairs, pout


def resample_ratio(fs_in, fs_out):
    """(p, q) = fs_out / fs_in reduced (diffsep_resample_ratio: host arithmetic; raises for rates <= 0 or a factor beyond 1000)"""
    p, q = C.c_int32(), C.c_int32()
    call(lib(), "diffsep_resample_ratio", int(fs_in), int(fs_out), C.byref(p), C.byref(q))
    return p.value, q.value


def resample_length(n, p, q):
    """ceil(n p / q): the samples a row of n samples becomes (diffsep_resample_length: host arithmetic)"""
    return _workspace_bytes(lib().diffsep_resample_length, n, p, q)


def resample_design(p, q):
    """the project's anti-aliasing FIR of the reduced ratio p / q as the library designs it: float64 [2 L + 1], summing to p
    (diffsep_resample_design: host arithmetic; metrics.resample_filter(p, q)[0] * p up to libm's Bessel and sine)"""
    l = lib()
    n = l.diffsep_resample_design(int(p), int(q), None, 0)
    check(0 if n >= 1 else 1, l)
    taps = np.zeros(n, dtype=np.float64)
    check(0 if l.diffsep_resample_design(int(p), int(q), taps.ctypes.data_as(C.c_void_p), n) == n else 1, l)
    return taps


class _ResamplerHandle:
    """a diffsep_resampler of the current device: the polyphase-ordered tap table of (p, q, taps)"""

    def __init__(self, p, q, taps):
        taps = np.ascontiguousarray(np.asarray(taps, dtype=np.float64))
        if taps.ndim != 1:
            raise ValueError("Resampler: taps must be a vector")
        self.ptr = C.c_void_p()
        self.device = torch.cuda.current_device()
        call(lib(), "diffsep_resampler_create", p, q, taps.ctypes.data_as(C.c_void_p), taps.size, C.byref(self.ptr))

    def __del__(self):
        if getattr(self, "ptr", None):
            try:
                lib().diffsep_resampler_destroy(self.ptr)
            except Exception:  # (interpreter shutdown: the library may be gone already)
                pass
            self.ptr = None


class Resampler:
    """Band-limited sample-rate conversion fs_in -> fs_out on the device (csrc/resample.hip): y[m] = sum_j h[m q + L - p j] x[j]
    with p / q = fs_out / fs_in reduced, in float64 from the fp32 samples on.  taps=None: the project's filter
    (resample_design(p, q); one device table per (device, p, q) for the life of the process); otherwise any odd-length float64
    FIR h, applied as given, with a table of this object's own.

    resampler(x, lengths=None, out=None, dtype=torch.float32): x [..., T] float32 device tensor, lengths (one per index of x's
    first dimension, host values or a device int32 tensor; default T) -> (y [..., ceil(T p / q)] of dtype float32 / float64, new
    lengths: host ints for host lengths, a device int32 tensor for device lengths).  Columns past a row's own new length are
    zeros; T = 0 gives empty rows.  out: a dense tensor of y's shape and dtype to write into.  Asynchronous on the current stream, no readback."""
    _designed = {}

    def __init__(self, fs_in, fs_out, taps=None):
        self.fs_in, self.fs_out = int(fs_in), int(fs_out)
        self.p, self.q = resample_ratio(fs_in, fs_out)
        self._taps = taps
        self._own = {}

    def _handle(self, device):
        cache, key = (Resampler._designed, (device.index, self.p, self.q)) if self._taps is None else (self._own, device.index)
        if key not in cache:
            with torch.cuda.device(device):
                cache[key] = _ResamplerHandle(self.p, self.q, resample_design(self.p, self.q) if self._taps is None else self._taps)
        return cache[key]

    def length(self, n):
        return resample_length(n, self.p, self.q)

    def __call__(self, x, lengths=None, out=None, dtype=torch.float32):
        if x.dim() < 1 or x.dtype != torch.float32 or not x.is_cuda:
            raise ValueError("Resampler: x must be a float32 [..., T] device tensor")
        if dtype not in (torch.float32, torch.float64):
            raise TypeError("Resampler: dtype must be float32 or float64")
        x = x.contiguous()
        T = x.shape[-1]
        rows = x.numel() // max(T, 1)
        groups = x.shape[0] if x.dim() > 1 else 1
        n_max = self.length(T)
        shape = tuple(x.shape[:-1]) + (n_max,)
        if out is None:
            out = torch.empty(shape, dtype=dtype, device=x.device)
        elif out.dtype != dtype or not out.is_contiguous() or tuple(out.shape) != shape or out.device != x.device:
            raise ValueError(f"Resampler: out must be a dense {dtype} tensor of shape {shape} on x's device")
        ln = ln_out = None
        if lengths is None:
            new = [n_max] * groups
        else:
            on_device = isinstance(lengths, torch.Tensor) and lengths.is_cuda
            ln = _dev_i32(lengths, x.device)
            if ln.numel() != groups:
                raise ValueError("Resampler: one length per index of x's first dimension")
            if on_device:
                new = ln_out = torch.empty(groups, dtype=torch.int32, device=x.device)
            else:
                new = [self.length(min(max(int(v), 0), T)) for v in (lengths.tolist() if isinstance(lengths, torch.Tensor) else lengths)]
        if rows == 0 or T == 0:  # nothing to convert (a file without samples): empty rows, lengths 0
            if ln_out is not None:
                ln_out.zero_()
            return out, new
        with torch.cuda.device(x.device):
            call(lib(), "diffsep_resample", self._handle(x.device).ptr, _ptr(x), T, _ptr(out), n_max, rows, T, _ptr(ln),
                 max(1, rows // max(groups, 1)), _ptr(ln_out), _lib.F32 if dtype == torch.float32 else _lib.F64, _stream_ptr(x.device))
        return out, new


PIT_MODES = {None: _lib.PIT_NONE, "none": _lib.PIT_NONE, "true_mix": _lib.PIT_TRUE_MIX, "init_hack_pit": _lib.PIT_TRUE_MIX,
             "mean0": _lib.PIT_MEAN0, "allthetime": _lib.PIT_MEAN0}


def _f32c(v):
    return None if v is None else v.float().contiguous()


def sde_perturb(sde, x0, mix, t, z=None, sigma_mix=None, beta=None, redefine_z=False, lengths=None, seed=0, stream_id=0,
                z_out=None):
    """diffsep_sde_perturb — sample_prior of every init_hack mode in one pass:
    x_t = beta true_mix + (1 - beta) mean + L z,  z_out = z + (redefine_z ? beta L^-1 (true_mix - mean) : 0).
    z=None: Philox draws of diffsep_randn(seed, stream_id) laid out as [B,S,T].  Returns (x_t, z_out); z_out may be z."""
    x0, mix, t, z, sigma_mix, beta = (_f32c(v) for v in (x0, mix, t, z, sigma_mix, beta))
    B, S, T = x0.shape
    assert mix.shape == (B, 1, T) and t.shape == (B,)
    ln = None if lengths is None else _dev_i32(lengths, x0.device)
    x_t = torch.empty_like(x0)
    z_out = torch.empty_like(x0) if z_out is None else z_out
    call(lib(), "diffsep_sde_perturb", C.byref(sde_config(sde)), _ptr(x0), _ptr(mix), _ptr(t), _ptr(z), _ptr(sigma_mix),
         _ptr(beta), int(bool(redefine_z)), _ptr(ln), int(seed) % (1 << 64), int(stream_id), _ptr(x_t), _ptr(z_out), B, S, T,
         _stream_ptr())
    return x_t, z_out


def batch_seeds(seed, B):
    """the per-utterance seeds the sampler derives from one seed on a mixed-length batch (diffsep_sampler_ext): seed + b * 0x9E3779B97F4A7C15"""
    return [(int(seed) + 0x9E3779B97F4A7C15 * b) % (1 << 64) for b in range(B)]


def warm_start(sde, est, mix, mix_norm, mean, std, t, *, scale="ls", mean_from="mix", noise=None, seed=0, seeds=None, lengths=None):
    """diffsep_warm_start — from another separator's estimates est [B,S,T] to the state the sampler starts from at the
    per-utterance times t [B] (Engine.pc_sample(x_init=, first_step=)): (x_init [B,S,T], gains [B,S] float64, fallback [B] int32).
    sde: the dict of an SDE's engine_config(), or the SDE object.  mix [B,1,T] raw, mix_norm / mean / std as normalize_batch
    returns them (per utterance over its own samples on a zero-padded batch, mix_norm zero beyond lengths).
    scale "ls": per utterance the gains g minimising || mix - sum_s g_s est_s ||^2 (an SI-SDR-trained separator's output has
    arbitrary scale and sign) — all 1 with fallback[b] = 1 where the estimates are silent or proportional; "none": gains of 1.
    x0 = (g est - mean) / std; x_init = m + exp(-lambda t)(x0 - m) + L(t) z with m = mix_norm / S (mean_from "mix") or the
    source average of x0 (mean_from "estimate": the reference's marginal_prob exactly).  z = noise [B,S,T], or generated in the
    kernel: draw 0 of randn_batch(seeds, lengths) with seeds (or with lengths: the seeds the sampler derives from seed), else draw
    0 of randn(B S T, seed) — the draw the sampler's prior would have used.  Asynchronous on the current stream, no readback."""
    sde = sde if isinstance(sde, dict) else sde.engine_config()
    est, mix, mix_norm, noise = (_f32c(v) for v in (est, mix, mix_norm, noise))
    B, S, T = est.shape
    dev = est.device
    mean, std, t = (_f32c(v).reshape(-1) for v in (mean, std, t))
    assert mean.numel() == B and std.numel() == B and t.numel() == B, "mean, std and t hold one value per utterance"
    for name, v in (("mix", mix), ("mix_norm", mix_norm)):
        assert v is None or tuple(v.shape) == (B, 1, T), f"{name} must be [B,1,T]"
    assert noise is None or tuple(noise.shape) == (B, S, T), "noise must be [B,S,T]"
    if scale not in _lib.WARM_SCALES or mean_from not in _lib.WARM_MEANS:
        raise ValueError(f"warm_start: scale is one of {list(_lib.WARM_SCALES)}, mean_from one of {list(_lib.WARM_MEANS)}")
    ln = None if lengths is None else _dev_i32(lengths, dev)
    if noise is None and seeds is None and lengths is not None:
        seeds = batch_seeds(seed, B)
    sd = None
    if seeds is not None and noise is None:
        h = torch.as_tensor(np.ascontiguousarray(np.asarray([int(s) % (1 << 64) for s in seeds], dtype=np.uint64)).view(np.int64))
        assert h.numel() == B, "seeds must be [B]"
        sd = h.pin_memory().to(dev, non_blocking=True)
    smix = sde_sigma_mix(mix_norm, sde.get("avg_len", 510)) if sde.get("kind", _lib.SDE_MIX) == _lib.SDE_PRIORMIX else None
    x = torch.empty_like(est)
    gains = torch.empty((B, S), dtype=torch.float64, device=dev)
    fallback = torch.empty((B,), dtype=torch.int32, device=dev)
    nbytes = _workspace_bytes(lib().diffsep_warm_start_workspace_bytes, B, S) if scale == "ls" else 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
    call(lib(), "diffsep_warm_start", C.byref(sde_config(sde)), _ptr(est), _ptr(mix), _ptr(mix_norm), _ptr(mean), _ptr(std), _ptr(t),
         _ptr(noise), _ptr(smix), _ptr(ln), _ptr(sd), int(seed) % (1 << 64), _lib.WARM_SCALES[scale], _lib.WARM_MEANS[mean_from],
         _ptr(x), _ptr(gains), _ptr(fallback), B, S, T, _ptr(ws), nbytes, _stream_ptr())
    return x, gains, fallback


def score_loss_workspace_bytes(B, S, T):
    """bytes of workspace the loss entries need (host arithmetic; raises for a shape they refuse)"""
    return _workspace_bytes(lib().diffsep_score_loss_workspace_bytes, B, S, T)


def score_loss_reduce(sde, score, z, t, x0=None, mix=None, sigma_mix=None, lengths=None, pit=None, want_coef=False):
    """diffsep_score_loss_reduce: float64 [B,P] device tensor of mean_{s, t < len}((L score + z_p)^2), P = 1 (pit=None) or S!
    (pit="true_mix" / "mean0": z_p = z + L^-1 (anchor - mean_p)), plus (best [B] float64, argbest [B] int32); want_coef adds
    the kernels' (exp(-lambda t), sqrt(ev1), sqrt(ev2)) as a float32 [B,3] tensor."""
    score, z, t, x0, mix, sigma_mix = (_f32c(v) for v in (score, z, t, x0, mix, sigma_mix))
    B, S, T = score.shape
    mode = PIT_MODES[pit]
    P = math.factorial(S) if mode else 1
    ln = None if lengths is None else _dev_i32(lengths, score.device)
    out = torch.empty((B, P), dtype=torch.float64, device=score.device)
    best = torch.empty(B, dtype=torch.float64, device=score.device)
    arg = torch.empty(B, dtype=torch.int32, device=score.device)
    coef = torch.empty((B, 3), dtype=torch.float32, device=score.device) if want_coef else None
    nbytes = score_loss_workspace_bytes(B, S, T)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=score.device)
    call(lib(), "diffsep_score_loss_reduce", C.byref(sde_config(sde)), _ptr(score), _ptr(z), _ptr(x0), _ptr(mix), _ptr(t),
         _ptr(sigma_mix), _ptr(ln), mode, _ptr(out), _ptr(best), _ptr(arg), _ptr(coef), B, S, T, _ptr(ws), nbytes,
         _stream_ptr())
    return (out, best, arg, coef) if want_coef else (out, best, arg)


def score_loss(engine, sde, mix_norm, target, t, beta=None, z=None, seed=0, lengths=None, pit=None, redefine_z=False,
               debug=False):
    """diffsep_score_loss on an Engine: perturb -> one score evaluation -> reduce, asynchronous on the current stream.
    Returns (out [B,P] float64, best [B] float64, argbest [B] int32) and, with debug, (x_t, score) [B,S,T] as well."""
    mix_norm, target, t, beta, z = (_f32c(v) for v in (mix_norm, target, t, beta, z))
    B, S, T = target.shape
    assert mix_norm.shape == (B, 1, T) and t.shape == (B,) and S == engine.S
    mode = PIT_MODES[pit]
    P = math.factorial(S) if mode else 1
    dev = target.device
    out = torch.empty((B, P), dtype=torch.float64, device=dev)
    best = torch.empty(B, dtype=torch.float64, device=dev)
    arg = torch.empty(B, dtype=torch.int32, device=dev)
    x_t = torch.empty_like(target) if debug else None
    score = torch.empty_like(target) if debug else None
    la, lp = (None, None) if lengths is None else host_array(lengths, np.int64, B, "lengths")
    nbytes = score_loss_workspace_bytes(B, S, T)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    sc, lc = sde_config(sde), LossConfig(mode, int(bool(redefine_z)))
    with torch.cuda.device(engine.device):
        call(engine._L, "diffsep_score_loss", engine._h, C.byref(sc), C.byref(lc), _ptr(mix_norm), _ptr(target), _ptr(t),
             _ptr(beta), _ptr(z), int(seed) % (1 << 64), lp, _ptr(out),
             _ptr(best), _ptr(arg), _ptr(x_t), _ptr(score), B, T, _ptr(ws), nbytes, _stream_ptr(engine.device))
    return (out, best, arg, x_t, score) if debug else (out, best, arg)


def _ode_unit(K, coef, k_out):
    """the unit wrappers' view of a stage list: (B, S, T, coefficients as a float64 array); K: float32 [B,S,T] tensors"""
    B, S, T = K[0].shape
    c = np.ascontiguousarray(coef, dtype=np.float64)
    assert len(c) <= len(K) and k_out < len(K) and all(k.shape == (B, S, T) and k.dtype == torch.float32 for k in K)
    return B, S, T, c


def _ode_ptrs(K):
    return (C.c_void_p * max(1, len(K)))(*[k.data_ptr() for k in K])


def ode_stage_update(sde, K, coef, h, y, k_out=-1, x=None, t=None, score=None, sigma_mix=None, x_out=None,
                     y_new_out=None):
    """diffsep_ode_stage_update: K[k_out] = probability-flow drift of (x, t, score) (k_out >= 0), then with
    acc = sum_j coef[j] K[j]: x_out = fp32(y + acc h), or (y_new_out given) y_new_out = y + h acc and x_out = fp32 of it.
    K: list of float32 [B,S,T] tensors (written in place at k_out); y float64 [B,S,T]."""
    B, S, T, c = _ode_unit(K, coef, k_out)
    call(lib(), "diffsep_ode_stage_update", C.byref(sde_config(sde)), _ptr(x), _ptr(t), _ptr(score), _ptr(sigma_mix), _ptr(y),
         _ode_ptrs(K), c.ctypes.data_as(C.c_void_p), len(c), int(k_out), float(h), _ptr(x_out), _ptr(y_new_out), B, S, T,
         _stream_ptr())
    return x_out, y_new_out


def ode_error_norm(sde, K, coef, h, y, rtol, atol, y_new=None, k_out=-1, x=None, t=None, score=None, sigma_mix=None):
    """diffsep_ode_error_norm: float64 [2] device tensor (||acc h / sc||_rms, ||y / sc||_rms), sc = atol + max(|y|,
    |y_new|) rtol; with k_out >= 0 the drift K[k_out] is produced in the same pass."""
    B, S, T, c = _ode_unit(K, coef, k_out)
    out = torch.empty(2, dtype=torch.float64, device=K[0].device)
    ws = torch.empty(ODE_WORKSPACE_BYTES, dtype=torch.uint8, device=K[0].device)
    call(lib(), "diffsep_ode_error_norm", C.byref(sde_config(sde)), _ptr(x), _ptr(t), _ptr(score), _ptr(sigma_mix), _ptr(y),
         _ptr(y_new), _ode_ptrs(K), c.ctypes.data_as(C.c_void_p), len(c), int(k_out), float(h), float(rtol), float(atol),
         _ptr(out), B, S, T, _ptr(ws), ws.numel(), _stream_ptr())
    return out


def _ode_tables(h, active, lengths, B, dev):
    """the per-utterance device tables of the *_each passes: h float64 [B], active int32 [B], lengths int32 [B]"""
    tabs = (torch.as_tensor(h, dtype=torch.float64).to(dev).contiguous(),
            torch.as_tensor(active, dtype=torch.int32).to(dev).contiguous(),
            torch.as_tensor(lengths, dtype=torch.int32).to(dev).contiguous())
    assert all(v.shape == (B,) for v in tabs), "h, active and lengths must be [B]"
    return tabs


def ode_stage_update_each(sde, K, coef, h, active, lengths, y, k_out=-1, x=None, t=None, score=None, sigma_mix=None,
                          x_out=None, y_new_out=None):
    """diffsep_ode_stage_update_each: ode_stage_update with a step size h[b] per utterance; utterances with active[b] == 0
    are skipped, samples t >= lengths[b] are never read and written as exact zeros."""
    B, S, T, c = _ode_unit(K, coef, k_out)
    hd, ad, ld = _ode_tables(h, active, lengths, B, K[0].device)
    call(lib(), "diffsep_ode_stage_update_each", C.byref(sde_config(sde)), _ptr(x), _ptr(t), _ptr(score), _ptr(sigma_mix),
         _ptr(y), _ode_ptrs(K), c.ctypes.data_as(C.c_void_p), len(c), int(k_out), _ptr(hd), _ptr(ad), _ptr(ld), _ptr(x_out),
         _ptr(y_new_out), B, S, T, _stream_ptr())
    return x_out, y_new_out


def ode_error_norm_each(sde, K, coef, h, active, lengths, y, rtol, atol, y_new=None, k_out=-1, x=None, t=None, score=None,
                        sigma_mix=None, out=None):
    """diffsep_ode_error_norm_each: float64 [B,2] device tensor, row b = the two norms of ode_error_norm over utterance
    b's lengths[b] samples alone (rows of inactive utterances keep the value of `out`, zeros when it is not given)."""
    B, S, T, c = _ode_unit(K, coef, k_out)
    hd, ad, ld = _ode_tables(h, active, lengths, B, K[0].device)
    if out is None:
        out = torch.zeros(B, 2, dtype=torch.float64, device=K[0].device)
    assert out.shape == (B, 2) and out.dtype == torch.float64 and out.is_contiguous()
    ws = torch.empty(B * ODE_WORKSPACE_BYTES, dtype=torch.uint8, device=K[0].device)
    call(lib(), "diffsep_ode_error_norm_each", C.byref(sde_config(sde)), _ptr(x), _ptr(t), _ptr(score), _ptr(sigma_mix),
         _ptr(y), _ptr(y_new), _ode_ptrs(K), c.ctypes.data_as(C.c_void_p), len(c), int(k_out), _ptr(hd), _ptr(ad), _ptr(ld),
         float(rtol), float(atol), _ptr(out), B, S, T, _ptr(ws), ws.numel(), _stream_ptr())
    return out


def expint_update_each(sde, y, score, coef, active, lengths, x0_prev=None, sigma_mix=None, want_norms=False, out=None):
    """diffsep_expint_update_each: one step of DDIM / DPM-Solver++ 2M on caller buffers.  y float64 [B,S,T], score float32
    [B,S,T], coef: one row of _lib.expint_coefficients (host), x0_prev: the previous step's X0 (float64; None: the w1 terms
    are absent), sigma_mix [B,T] for PriorMixSDE; active / lengths [B] as in ode_stage_update_each.  out: optional
    (x0, y_new, x) to write into (inactive rows keep what they hold), else zeros.  Returns (x0 float64, y_new float64,
    x float32[, norms float64 [B,2]: RMS of the step minus its DDIM step, RMS of y])."""
    B, S, T = y.shape
    assert y.dtype == torch.float64 and score.dtype == torch.float32 and score.shape == y.shape
    assert x0_prev is None or (x0_prev.dtype == torch.float64 and x0_prev.shape == y.shape)
    c = np.ascontiguousarray(coef, dtype=np.float64).reshape(-1)
    assert c.size == _lib.EXPINT_COEFS, f"coef must hold {_lib.EXPINT_COEFS} values"
    dev = y.device
    ad = torch.as_tensor(active, dtype=torch.int32).to(dev).contiguous()
    ld = torch.as_tensor(lengths, dtype=torch.int32).to(dev).contiguous()
    assert ad.shape == (B,) and ld.shape == (B,), "active and lengths must be [B]"
    if out is None:
        out = (torch.zeros_like(y), torch.zeros_like(y), torch.zeros_like(score))
    x0, y_new, x = out
    norms = torch.zeros(B, 2, dtype=torch.float64, device=dev) if want_norms else None
    ws = torch.empty(B * ODE_WORKSPACE_BYTES, dtype=torch.uint8, device=dev) if want_norms else None
    call(lib(), "diffsep_expint_update_each", C.byref(sde_config(sde)), _ptr(y), _ptr(score), _ptr(sigma_mix), _ptr(x0_prev),
         c.ctypes.data_as(C.c_void_p), _ptr(ad), _ptr(ld), _ptr(x0), _ptr(y_new), _ptr(x), _ptr(norms), B, S, T, _ptr(ws),
         ws.numel() if want_norms else 0, _stream_ptr())
    return (x0, y_new, x, norms) if want_norms else (x0, y_new, x)
