"""Plain references and inputs for the fused attention kernel (csrc/attn_fused.hip), shared by tests/test_attn_fused_gpu.py and
tests/test_attn_fused_ref_cpu.py.  Nothing here touches the GPU.

The operation, on the operands the kernel is given (x in the storage type, M = Wk^T Wq, Wv, Wo in the storage type as
w[out][in], fp32 biases b', b_v, b_o and an fp32 (scale, shift) table [B,128]):

    h = x*scale + shift;  V = h Wv^T + b_v;  Q' = h M^T + b';  S = Q' h^T / sqrt(128);  P = softmax_j(S);  O = P V
    v = (O Wo^T + b_o + x) / sqrt(2)

attn_ref(op) computes it without intermediate rounding ("ref_exact"); attn_ref(op, mirror=True) rounds to the storage type where
the kernel does ("ref_mirror"): h (the LDS copy), V (the V^T tile in LDS), Q' (accumulator -> fragment), P after the
normalisation (accumulator -> fragment), O (accumulator -> fragment) and the stored y = round(v).  S, the softmax sums, O Wo^T
and v stay in fp32 in the kernel and unrounded here.  Both return v before the final rounding, y, and the channel sums of v and
v^2 over the L rows of the sample (what the kernel adds to the consumer's GroupNorm accumulators).

`keys` and `rows` restate the kernel's padding for the sensitivity checks: a tile of 32 pixels past L holds h = 0 rows (so
V = b_v there); keys = L - 1 drops the last key, keys = L + 1 lets one padded key into the softmax, rows = L + 1 also computes
the first padded query row (which the kernel computes and must neither store nor count)."""
import math
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

from diffsep_amd import synth

C = 128
BATCH = 3
GROUPS = 32
EPS = 1e-6
BF, HF = torch.bfloat16, torch.float16
DTYPES = [BF, HF]
# L = H * W by instantiation (LT tiles of 32 pixels): whole and ragged
L_BY_LT = {1: (16, 32), 2: (48, 64), 4: (80, 112, 128), 8: (144, 192, 240, 256)}
L_ALL = [L for ls in L_BY_LT.values() for L in ls]
L_RAGGED = [L for L in L_ALL if L % 32]
L_ACC = (48, 192)                    # the accumulator form: ragged and large
BLOCK_HW = ((16, 4), (16, 12))       # block-level cases: L = 64 and L = 192


def dt_id(dt):
    return str(dt).replace("torch.", "")


def rnd(tag, shape, scale=1.0):
    return torch.from_numpy(synth.synth_noise(tag, shape)) * scale


def rms(a):
    return float(a.detach().double().pow(2).mean().sqrt())


def rel_rms(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return rms(a - b) / (rms(b) + 1e-300)


def attn_ref(op, mirror=False, cdt=torch.float64, keys=None, rows=None):
    dt = op.x.dtype
    rd = (lambda t: t.to(dt).to(cdt)) if mirror else (lambda t: t)
    x = op.x.to(cdt)
    B, L, _ = x.shape
    keys = L if keys is None else keys
    rows = L if rows is None else rows
    R = max(L, keys, rows)
    M, Wv, Wo = op.M.to(cdt), op.Wv.to(cdt), op.Wo.to(cdt)
    # (one rounding, like the kernel's fmaf: the product of two fp32 values is exact in float64)
    h = rd((op.x.double() * op.scale.double()[:, None, :] + op.shift.double()[:, None, :]).to(cdt))
    if R > L:  # padded pixels: h = 0 (not the shift), no residual
        pad = torch.zeros((B, R - L, C), dtype=cdt)
        h, x = torch.cat([h, pad], 1), torch.cat([x, pad], 1)
    V = rd(h[:, :keys] @ Wv.T + op.bv.to(cdt))
    Q = rd(h[:, :rows] @ M.T + op.bq.to(cdt))
    S = Q @ h[:, :keys].transpose(1, 2) / math.sqrt(C)
    P = rd(torch.softmax(S, -1))
    O = rd(P @ V)
    branch = O @ Wo.T + op.bo.to(cdt)
    v = (branch + x[:, :rows]) / math.sqrt(2.0)
    n = min(rows, L)
    return SimpleNamespace(v=v, y=v.to(dt), s1=v[:, :n].sum(1), s2=(v[:, :n] ** 2).sum(1), P=P, branch=branch)


def gate_terms(mir):
    """per (sample, channel) magnitudes the statistics gate scales with: sum |v| and sum v^2 over the sample's rows"""
    return mir.v.abs().sum(1), (mir.v ** 2).sum(1)


# ------------------------------------------------------------------------------------------------ inputs
KEY_OFFSET = 3.0  # mean logit of a real key below that of a padded one (whose h = 0 row scores exactly 0)


def sign_vector():
    return torch.sign(rnd("af.u", (C,)))


def weights(dt):
    """M, Wv, Wo (storage type, w[out][in]) and the fp32 biases: one set for every L.  M's scale keeps the softmax between
    uniform and one-hot; b_o has a non-zero mean so that a wrongly counted padded row shows in the statistics; b' has a
    component against the common part of the shift (unit_case), which puts the logits of the real keys KEY_OFFSET below zero:
    the softmax does not see it (it is the same for every real key), a padded key let into the softmax does."""
    return dict(M=rnd("af.M", (C, C), 0.15).to(dt), Wv=rnd("af.Wv", (C, C), 1.0 / math.sqrt(C)).to(dt),
                Wo=rnd("af.Wo", (C, C), 2.0 / math.sqrt(C)).to(dt),
                bq=rnd("af.bq", (C,), 0.1) - 2.0 * KEY_OFFSET / math.sqrt(C) * sign_vector(), bv=rnd("af.bv", (C,), 0.1),
                bo=0.5 + rnd("af.bo", (C,), 0.1))


def unit_case(L, dt, B=BATCH):
    """x small, scale large: h is O(1) while the residual is not, so the attention branch carries the output; a different table
    per sample (the shifts share the component 0.5 * sign_vector(): b' . shift / sqrt(C) = -KEY_OFFSET on average).  The last
    pixel is drawn 1.5 times larger: its logits spread wider, so the last key holds enough softmax mass at every L for a mask
    that drops it to show above the storage rounding."""
    x = rnd(f"af.x{L}", (B, L, C), 0.05)
    x[:, L - 1] *= 1.5
    return SimpleNamespace(x=x.to(dt), scale=20.0 * (1.0 + rnd(f"af.sc{L}", (B, C), 0.2)),
                           shift=rnd(f"af.sh{L}", (B, C), 0.2) + 0.5 * sign_vector(), L=L, **weights(dt))


def gn_affine():
    return 1.0 + rnd("af.gamma", (C,), 0.2), rnd("af.beta", (C,), 0.1)


def gn_table64(x, gamma, beta, groups=GROUPS, eps=EPS):
    """(scale, shift) [B,C] float64 with x*scale + shift == F.group_norm(x) computed in float64 (x [B,L,C], biased variance)"""
    B, L, Cc = x.shape
    xd = x.double()
    ones, zeros = torch.ones(Cc, dtype=torch.float64), torch.zeros(Cc, dtype=torch.float64)
    n = F.group_norm(xd.transpose(1, 2), groups, ones, zeros, eps).transpose(1, 2)  # (x - mean) * rstd
    g = xd.reshape(B, L, groups, Cc // groups)
    mean = g.mean((1, 3))
    rstd = 1.0 / torch.sqrt(g.var((1, 3), unbiased=False) + eps)
    assert rel_rms(((g - mean[:, None, :, None]) * rstd[:, None, :, None]).reshape(B, L, Cc), n) < 1e-12
    scale = rstd.repeat_interleave(Cc // groups, 1) * gamma.double()
    return scale, beta.double() - mean.repeat_interleave(Cc // groups, 1) * scale


def acc_case(L, dt, B=BATCH):
    """the unit case with its table taken from GroupNorm(x) (float64, then fp32) instead of a free draw"""
    op = unit_case(L, dt, B)
    op.gamma, op.beta = gn_affine()
    s, t = gn_table64(op.x, op.gamma, op.beta)
    op.scale, op.shift = s.float(), t.float()
    return op


def block_case(H, W, dt, B=BATCH):
    """AttnBlockpp parameters in the NIN layout of oracle/diffsep_oracle.py (W [in][out]: y = x @ W + b), scaled so that the
    attention branch is several times the residual: x small, gamma = 1.  Returns the oracle's state dict (float32 numpy), the
    parameter list of ops.attnblock_forward, x [B,C,H,W] fp32 already rounded to the storage type, the operands of ref_exact
    (M = Wk^T Wq and b' = Wk^T b_q folded in float64, nothing rounded) and those of ref_mirror (folded in fp32, then the storage
    type, as the engine does); both with the float64 GroupNorm table of the stored x."""
    a = math.sqrt(0.15 / math.sqrt(C))  # |M| entries about 0.15, as in the unit cases
    sd = {"GroupNorm_0.weight": np.ones(C, np.float32), "GroupNorm_0.bias": rnd("afb.beta", (C,), 0.1).numpy()}
    for i, (s, b0) in enumerate([(a, 0.0), (a, 0.0), (1.0 / math.sqrt(C), 0.0), (2.0 / math.sqrt(C), 0.5)]):
        sd[f"NIN_{i}.W"] = rnd(f"afb.W{i}", (C, C), s).numpy()
        sd[f"NIN_{i}.b"] = (b0 + rnd(f"afb.b{i}", (C,), 0.1)).numpy()
    names = ["GroupNorm_0.weight", "GroupNorm_0.bias"] + [f"NIN_{i}.{n}" for i in range(4) for n in ("W", "b")]
    x = (rnd(f"afb.x{H}.{W}", (B, C, H, W), 0.05) + 0.01).to(dt).float()
    xs = x.permute(0, 2, 3, 1).reshape(B, H * W, C).to(dt)
    t = {k: torch.from_numpy(v) for k, v in sd.items()}
    scale, shift = gn_table64(xs, t["GroupNorm_0.weight"], t["GroupNorm_0.bias"])
    Wq, Wk, Wv, Wo = (t[f"NIN_{i}.W"].double() for i in range(4))
    exact = SimpleNamespace(x=xs, scale=scale, shift=shift, M=Wk @ Wq.T, bq=Wk @ t["NIN_0.b"].double(), Wv=Wv.T,
                            bv=t["NIN_2.b"], Wo=Wo.T, bo=t["NIN_3.b"], L=H * W)
    mirror = SimpleNamespace(x=xs, scale=scale.float(), shift=shift.float(), M=(Wk.float() @ Wq.float().T).to(dt),
                             bq=Wk.float() @ t["NIN_0.b"], Wv=Wv.T.to(dt), bv=t["NIN_2.b"], Wo=Wo.T.to(dt), bo=t["NIN_3.b"],
                             L=H * W)
    return SimpleNamespace(sd=sd, params=[sd[n] for n in names], x=x, exact=exact, mirror=mirror)


def effective_keys(P):
    """mean over the rows of exp(entropy) of the attention distribution"""
    p = P.double().clamp_min(1e-300)
    return float(torch.exp(-(p * p.log()).sum(-1)).mean())
