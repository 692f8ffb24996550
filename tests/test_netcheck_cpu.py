"""The walk of tests/netcheck.py tested without a GPU: a simulated engine, and the wiring faults the relative-RMS gates let through.

SimEngine is a torch forward of a small configuration (nf = 16, ch_mult (1, 2, 2) on the 256-row spectrogram, attention at 64 rows:
plain, narrow, folded-skip, resampling and cat blocks, two Combines, three pyramid heads, unfused attention) that does what the device
engine does between its kernels: it rounds every stored tensor to the storage type, stages SiLU(GroupNorm(x)) in the storage type,
keeps fixed-point accumulators of the values BEFORE the output rounding, builds every GroupNorm table from those accumulators by the
kernels' expression (conv_device.h: ds_gn_affine_from_acc, restated in table_from_acc below) and emits the trace records of the real
engine.  Each convolution is one float32 torch convolution.  two_launch="sw" / "no_sw" runs the cat blocks with equal halves as the
device runs cat(128, 128) -> 128: Conv_0 as two launches, and (no_sw) Conv_1 + skip as two launches.

The walk must pass on it in bfloat16, half and float32.  Then one fault at a time is planted in one block; for each the test prints the
end-to-end relative RMS against the float64 oracle next to the gates it would have to break (5e-2 for 16-bit engines in
tests/test_engine_gpu.py, 1e-4 for fp32) and the walk's worst err / bound, and asserts that the walk fails.  Figures of one run
(bfloat16 | float32: end-to-end rel. RMS with the fault, walk's worst ratio) are kept in FAULT_FIGURES below.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import diffsep_oracle as O  # noqa: E402

import convcheck as CC  # noqa: E402
import gncheck as GC  # noqa: E402
import netcheck as NC  # noqa: E402
import stftcheck as SC  # noqa: E402
from diffsep_amd import synth  # noqa: E402

torch.set_grad_enabled(False)
BF, HF, F32 = CC.BF, CC.HF, CC.F32
CFG = NC.cfg_dict(16, ch_mult=(1, 2, 2), attn_resolution=64)
B, W = 2, 64
T = 128 * W - (510 - 128) - 1          # the longest signal of W frames (Engine.bucket_length)
TIMES = (0.03, 0.8)
SEED, IN_SCALE = 7, 0.3                # synth_state_dict seed and input scale: every layer's stored input stays inside DOMAIN
RMS_GATE = {BF: 5e-2, HF: 5e-2, F32: 1e-4}
FAULTS = ("temb_next", "bias_stride", "drop_conv2_bias", "acc_swapped", "gamma_other_half", "scale_before_res", "stats_before_res")
# Records of a run of this file (printed by test_planted_fault_is_caught; nothing asserts them).  Without a fault the simulated engine is
# 1.71e-2 (bfloat16) / 4.12e-6 (float32) from the float64 oracle.  fault -> (bfloat16, float32), each (end-to-end relative RMS with the
# fault, walk's worst err / bound).  In this 3-level nf = 16 network one block is a large share of the whole, so most faults also
# break the end-to-end gates (5e-2 / 1e-4); the batch-stride fault and the dropped Conv_2 bias stay under the bfloat16 gate, and the
# batch-stride fault is 1.18e-4 against 1e-4 in float32.  The walk sees every one of them with a factor of at least 4 to spare.
CLEAN_RMS = {"bf16": 1.71e-2, "f32": 4.12e-6}
FAULT_FIGURES = {
    "temb_next": ((1.23e-1, 30.2), (1.22e-1, 3.48e3)), "bias_stride": ((1.71e-2, 17.2), (1.18e-4, 1.94e3)),
    "drop_conv2_bias": ((2.69e-2, 4.28), (1.99e-2, 344.0)), "acc_swapped": ((2.00e-1, 32.3), (2.02e-1, 3.79e3)),
    "gamma_other_half": ((6.17e-2, 9.28), (5.94e-2, 1.14e3)), "scale_before_res": ((1.77e-1, 34.7), (1.79e-1, 1.27e4)),
    "stats_before_res": ((3.29e-1, 351.0), (3.29e-1, 1.77e3)),
}


def table_from_acc(sa, sb, gamma, beta, groups, npix):
    """ds_gn_affine_from_acc (conv_device.h) on the group totals of int64 accumulators [B,C*,2]: fp32 scale, shift [B,C]"""
    acc = (torch.cat([sa, sb], 1) if sb is not None else sa).numpy()
    Bn, C, _ = acc.shape
    cpg = C // groups
    tot = acc.reshape(Bn, groups, cpg, 2).sum(2)
    inv = float(np.float32(1.0 / (float(npix) * cpg)))
    mean = tot[..., 0].astype(np.float64) * (1.0 / 2.0 ** 24) * inv
    var = np.maximum(tot[..., 1].astype(np.float64) * (1.0 / 2.0 ** 16) * inv - mean * mean, 0.0)
    rstd = (1.0 / np.sqrt(var + float(np.float32(1e-6)))).astype(np.float32)
    g, be = gamma.numpy().astype(np.float32), beta.numpy().astype(np.float32)
    sc = np.repeat(rstd, cpg, 1) * g[None]
    sh = be[None] - np.repeat(mean.astype(np.float32), cpg, 1) * sc
    return torch.from_numpy(sc.astype(np.float32)), torch.from_numpy(sh.astype(np.float32))


class SimTensor:
    def __init__(self, y, acc, idx):
        self.y, self.acc, self.idx = y, acc, idx

    @property
    def C(self):
        return self.y.shape[-1]


class SimEngine:
    """see the module docstring.  fault = (name, module index) or None."""

    def __init__(self, cfg, sd, dt, xt, t, mix, fault=None, two_launch=None):
        self.cfg, self.dt, self.split, self.stft_route = cfg, dt, False, "f32"
        self.sd = {k: torch.as_tensor(np.asarray(v)).float() for k, v in sd.items()}
        self.xt, self.t, self.mix = xt, t, mix
        self.fault, self.two_launch = fault or (None, -1), two_launch
        self.records, self.store, self.accs = [], [], []
        self.mod = -1
        self.out = None
        self._forward()

    # ---- provider interface
    def tensor(self, rec):
        return self.store[rec["offset"]]

    def stats(self, rec):
        return self.accs[rec["stats"]]

    def table(self, sa, sb, gamma, beta, groups, npix):
        return table_from_acc(sa, sb, gamma, beta, groups, npix)

    # ---- storage
    def emit(self, kind, role, v, stats=False, f32=False, stats_of=None):
        """store v (the value before the output rounding) and record it; stats: fixed-point accumulators of v"""
        y = v.float() if (f32 or self.dt == F32) else v.float().to(self.dt)
        acc = None
        if stats:
            sv = (v if stats_of is None else stats_of).double()
            acc = torch.stack([(sv * 2.0 ** 24).round().sum((1, 2)), (sv * sv * 2.0 ** 16).round().sum((1, 2))], -1).to(torch.int64)
            self.accs.append(acc)
        if y.dim() == 2:
            Bn, H, Wd, C = y.shape[0], 1, 1, y.shape[1]
        else:
            Bn, H, Wd, C = y.shape
        self.store.append(y.reshape(Bn, H, Wd, C))
        self.records.append(dict(kind=kind, role=role, kernel="sim", mod=self.mod, B=Bn, H=H, W=Wd, C=C, ld=C, f32=bool(f32),
                                 offset=len(self.store) - 1, stats=len(self.accs) - 1 if stats else -1))
        return SimTensor(self.store[-1].reshape(y.shape), acc, len(self.store) - 1)

    def par(self, n):
        return self.sd[n]

    def wq(self, w):
        return w if self.dt == F32 else w.to(self.dt).float()

    def conv(self, role, x, table, w, bias=None, bb=None, res=None, skip=None, scale=1.0, stats=False, scale_before_res=False,
             stats_before_res=False):
        """one launch: float32 convolution of the staged input (stored type) with the stored-type weights"""
        xs = torch.cat([t.y.float() for t in x if t is not None], -1)
        if table is not None:
            sc, sh = table
            h = F.silu(xs * sc[:, None, None, :] + sh[:, None, None, :])
            xs = h if self.dt == F32 else h.to(self.dt).float()
        if w.shape[1] < xs.shape[-1]:
            w = F.pad(w, (0, 0, 0, 0, 0, xs.shape[-1] - w.shape[1]))
        v = F.conv2d(xs.permute(0, 3, 1, 2), self.wq(w), None, padding=w.shape[-1] // 2).permute(0, 2, 3, 1)
        if skip is not None:
            sx = torch.cat([t.y.float() for t in skip[:2] if t is not None], -1)
            v = v + F.conv2d(sx.permute(0, 3, 1, 2), self.wq(skip[2])).permute(0, 2, 3, 1)
        if bias is not None:
            v = v + bias
        if bb is not None:
            v = v + bb[:, None, None, :]
        pre = v
        if res is not None:
            v = (v * scale + res.y.float()[..., :v.shape[-1]]) if scale_before_res else (v + res.y.float()[..., :v.shape[-1]]) * scale
        else:
            v = v * scale
        return self.emit("conv", role, v, stats=stats, stats_of=(pre * scale) if stats_before_res else None)

    def gn_apply(self, x, table, act, mode, roles):
        xs = x.y.float()
        outs = []
        if table is not None:
            a = xs * table[0][:, None, None, :] + table[1][:, None, None, :]
            a = F.silu(a) if act else a
            outs.append(self.emit("gn_apply", roles[0], GC.fir(a, mode)))
        if mode:
            outs.append(self.emit("gn_apply", roles[-1], GC.fir(xs, mode)))
        return outs

    def table_of(self, a, b, gamma, beta, materialise=False):
        C = a.C + (b.C if b is not None else 0)
        npix = a.y.shape[1] * a.y.shape[2]
        t = table_from_acc(a.acc, b.acc if b is not None else None, gamma, beta, NC.groups_of(C), npix)
        if materialise:
            self.emit("gn_finalize", "scale", t[0], f32=True)
            self.emit("gn_finalize", "shift", t[1], f32=True)
        return t

    # ---- blocks
    def res_block(self, mi, x, up=False, down=False):
        self.mod = mi
        pre = f"all_modules.{mi}."
        p = self.par
        a, b = x
        fname = self.fault[0] if self.fault[1] == mi else None
        w0 = p(pre + "Conv_0.weight")
        out_ch = w0.shape[0]
        off = self.temb_off
        self.temb_off += out_ch
        mode = 1 if up else (2 if down else 0)
        has2 = (pre + "Conv_2.weight") in self.sd
        g0w, g0b = p(pre + "GroupNorm_0.weight"), p(pre + "GroupNorm_0.bias")
        if fname == "gamma_other_half":
            g0w, g0b = torch.roll(g0w, a.C), torch.roll(g0b, a.C)
        t0 = self.table_of(b, a, g0w, g0b) if fname == "acc_swapped" else self.table_of(a, b, g0w, g0b, materialise=bool(mode))
        if fname == "temb_next":
            off += out_ch
        temb = self.proj[:, off:off + out_ch]
        if fname == "bias_stride":  # row b of the projection read at b * out_ch instead of b * dense_total
            flat = self.proj.reshape(-1)
            temb = torch.stack([flat[bi * out_ch + off:bi * out_ch + off + out_ch] for bi in range(self.proj.shape[0])])
        b0 = p(pre + "Conv_0.bias")
        xr = x
        two = self.two_launch if (b is not None and a.C == b.C == out_ch and not mode) else None
        if mode:
            h0m, xrr = self.gn_apply(a, t0, 1, mode, ("h0m", "xr"))
            xr = (xrr, None)
            h1 = self.conv("h1", (h0m,), None, w0, bias=b0, bb=temb, stats=True)
        elif two:
            C1 = a.C
            h1p = self.conv("h1p", (a,), (t0[0][:, :C1], t0[1][:, :C1]), w0[:, :C1], bias=b0, bb=temb)
            h1 = self.conv("h1", (b,), (t0[0][:, C1:], t0[1][:, C1:]), w0[:, C1:], res=h1p, stats=True)
        else:
            h1 = self.conv("h1", (a, b), t0, w0, bias=b0, bb=temb, stats=True)
        t1 = self.table_of(h1, None, p(pre + "GroupNorm_1.weight"), p(pre + "GroupNorm_1.bias"))
        w1, b1 = p(pre + "Conv_1.weight"), p(pre + "Conv_1.bias")
        s = NC.INV_SQRT2
        kw = dict(scale_before_res=fname == "scale_before_res", stats_before_res=fname == "stats_before_res")
        if has2:
            w2, b2 = p(pre + "Conv_2.weight"), p(pre + "Conv_2.bias")
            b2e = None if fname == "drop_conv2_bias" else b2[None].expand(a.y.shape[0], -1)
            if two == "no_sw":
                C1 = a.C
                outp = self.conv("outp", (h1,), t1, w1, bias=b1, bb=b2e, skip=(a, None, w2[:, :C1]))
                return self.conv("out", (b,), None, w2[:, C1:], res=outp, scale=s, stats=True, **kw)
            if out_ch <= 16:  # narrow: the skip convolution as a launch of its own
                skip = self.conv("skip", xr, None, w2, bias=None if fname == "drop_conv2_bias" else b2)
                return self.conv("out", (h1,), t1, w1, bias=b1, res=skip, scale=s, stats=True, **kw)
            return self.conv("out", (h1,), t1, w1, bias=b1, bb=b2e, skip=(xr[0], xr[1], w2), scale=s, stats=True)
        return self.conv("out", (h1,), t1, w1, bias=b1, res=xr[0], scale=s, stats=True, **kw)

    def attn_block(self, mi, x):
        self.mod = mi
        pre = f"all_modules.{mi}."
        p = self.par
        Bn, H, Wd, C = x.y.shape
        L = H * Wd
        Lp = (L + 7) // 8 * 8
        t0 = self.table_of(x, None, p(pre + "GroupNorm_0.weight"), p(pre + "GroupNorm_0.bias"), materialise=True)
        h, = self.gn_apply(x, t0, 0, 0, ("h",))
        nin = lambda i: p(pre + f"NIN_{i}.W").T.contiguous()[:, :, None, None]
        q = self.conv("q", (h,), None, nin(0), bias=p(pre + "NIN_0.b"))
        k = self.conv("k", (h,), None, nin(1), bias=p(pre + "NIN_1.b"))
        hf = h.y.float().reshape(Bn, L, C)
        vt = torch.einsum("oc,blc->bol", self.wq(p(pre + "NIN_2.W").T.contiguous()), hf) + p(pre + "NIN_2.b")[None, :, None]
        vt = self.emit("gemm", "vt", F.pad(vt, (0, Lp - L)).reshape(Bn, 1, C, Lp))
        sc = torch.einsum("bic,bjc->bij", q.y.float().reshape(Bn, L, C), k.y.float().reshape(Bn, L, C)) * (C ** -0.5)
        scs = self.emit("gemm", "scores", F.pad(sc, (0, Lp - L)).reshape(Bn, 1, L, Lp))
        pr = torch.softmax(scs.y.float().reshape(Bn, L, Lp)[..., :L], -1)
        prs = self.emit("softmax", "probs", F.pad(pr, (0, Lp - L)).reshape(Bn, 1, L, Lp))
        o = torch.einsum("bij,bcj->bic", prs.y.float().reshape(Bn, L, Lp), vt.y.float().reshape(Bn, C, Lp))
        os_ = self.emit("gemm", "o", o.reshape(Bn, H, Wd, C))
        # (the records say L real columns for V^T and the scores, as the engine's do: ld = Lp)
        for r in self.records[-4:-2]:
            r["C"] = L
            self.store[r["offset"]] = self.store[r["offset"]][..., :L]
        return self.conv("out", (os_,), None, nin(3), bias=p(pre + "NIN_3.b"), res=x, scale=NC.INV_SQRT2, stats=True)

    def _forward(self):
        c, p = self.cfg, self.par
        nf, S, L, nrb = c["nf"], c["num_sources"], len(c["ch_mult"]), c["num_res_blocks"]
        dt = self.dt
        # front end: the float64 reference rounded once (the kernels' own simulations are tests/test_stftcheck_cpu.py's subject)
        self.mod = -1
        x0 = self.emit("stft", "x0", SC.stft_ref(self.xt, self.mix, W, c["spec_abs_exponent"], c["spec_factor"], shift=True)["y"])
        t64 = self.t.double()
        xp = torch.log(t64)[:, None] * p("all_modules.0.W").double()[None] * 2.0 * NC.SD.PI32
        emb = self.emit("fourier", "emb", torch.cat([torch.sin(xp), torch.cos(xp)], -1), f32=True)
        t1 = self.emit("linear", "t1", F.linear(emb.y.double(), p("all_modules.1.weight").double(), p("all_modules.1.bias").double()), f32=True)
        temb = self.emit("linear", "temb", F.linear(F.silu(t1.y.double()), p("all_modules.2.weight").double(),
                                                    p("all_modules.2.bias").double()), f32=True)
        dense = [n[:-len("Dense_0.weight")] for n in self.sd if n.endswith("Dense_0.weight")]  # (state-dict order = module order)
        Wd = torch.cat([p(n + "Dense_0.weight") for n in dense]).double()
        bd = torch.cat([p(n + "Dense_0.bias") for n in dense]).double()
        self.proj = self.emit("linear", "proj", F.linear(F.silu(temb.y.double()), Wd, bd), f32=True).y.reshape(self.t.shape[0], -1)
        self.temb_off = 0
        mi = 3
        self.mod = mi
        h = self.conv("conv_in", (x0,), None, p("all_modules.3.weight"), bias=p("all_modules.3.bias"), stats=True)
        mi += 1
        hs = [h]
        pyr_in = x0
        for i in range(L):
            for _ in range(nrb):
                h = self.res_block(mi, (hs[-1], None)); mi += 1
                if h.y.shape[1] == c["attn_resolution"]:
                    h = self.attn_block(mi, h); mi += 1
                hs.append(h)
            if i != L - 1:
                h = self.res_block(mi, (hs[-1], None), down=True); mi += 1
                self.mod = mi
                pyr_in, = self.gn_apply(pyr_in, None, 0, 2, ("pd",))
                pre = f"all_modules.{mi}."
                h = self.conv("combine", (pyr_in,), None, p(pre + "Conv_0.weight"), bias=p(pre + "Conv_0.bias"), res=h, stats=True); mi += 1
                hs.append(h)
        h = self.res_block(mi, (hs[-1], None)); mi += 1
        h = self.attn_block(mi, h); mi += 1
        h = self.res_block(mi, (h, None)); mi += 1
        pyramid = None
        for i in reversed(range(L)):
            for _ in range(nrb + 1):
                h = self.res_block(mi, (h, hs.pop())); mi += 1
            if h.y.shape[1] == c["attn_resolution"]:
                h = self.attn_block(mi, h); mi += 1
            gpre, pre = f"all_modules.{mi}.", f"all_modules.{mi + 1}."
            mi += 2
            self.mod = mi - 1
            tb = self.table_of(h, None, p(gpre + "weight"), p(gpre + "bias"))
            pu = self.gn_apply(pyramid, None, 0, 1, ("pu",))[0] if pyramid is not None else None
            w = F.pad(p(pre + "weight"), (0, 0, 0, 0, 0, 0, 0, 2))  # (the packed head writes 8 channels: 6 + zero padding)
            pyramid = self.conv("pnew", (h,), tb, w, bias=F.pad(p(pre + "bias"), (0, 2)), res=pu)
            if i != 0:
                h = self.res_block(mi, (h, None), up=True); mi += 1
        assert not hs
        self.mod = -1
        ref = SC.istft_ref(pyramid.y, S, self.xt.shape[-1], c["spec_abs_exponent"], c["spec_factor"],
                           ow=p("output_layer.weight")[:, :, 0, 0], ob=p("output_layer.bias"), tdiv=self.t)
        self.out = ref["out"].float()


# ------------------------------------------------------------------------------------------------ inputs, shared references
@functools.lru_cache(None)
def inputs():
    sd = synth.synth_state_dict(O.param_table(CFG), SEED)
    xt, mix = SC.signal("nw.sig", B, CFG["num_sources"], T, IN_SCALE)
    t = torch.tensor(TIMES, dtype=torch.float32)
    return sd, xt.float(), t, mix.float()


@functools.lru_cache(None)
def oracle_out():
    sd, xt, t, mix = inputs()
    p64 = {k: torch.from_numpy(np.asarray(v)).double() for k, v in sd.items()}
    return O.score_forward(p64, CFG, xt.double(), t.double(), mix.double())


@functools.lru_cache(None)
def sim(dt, fault=None, two_launch=None):
    sd, xt, t, mix = inputs()
    return SimEngine(CFG, sd, dt, xt, t, mix, fault=fault, two_launch=two_launch)


def cat_block_with_equal_halves():
    """module index of an up-path block cat(32, 32) -> 32 with Conv_2 (folded skip), and of a narrow one (cat -> 16)"""
    w = NC.Walk(sim(F32))
    cats = [s for s in w.steps if "cat" in s.name and "Conv_0" in s.name]
    eq = next(s.mod for s in cats if "(cat 64->32)" in s.name)
    narrow = next(s.mod for s in cats if "->16)" in s.name)
    return eq, narrow


DT_IDS = {BF: "bf16", HF: "f16", F32: "f32"}


@pytest.mark.parametrize("dt", [BF, HF, F32], ids=DT_IDS.get)
def test_walk_passes_on_the_simulated_engine(dt):
    w = NC.Walk(sim(dt))
    ratios = w.run()
    NC.report(f"sim {DT_IDS[dt]}", ratios)
    assert w.ran == len(w.steps) and max(ratios.values()) <= 1.0
    kinds = {s.kind for s in w.steps}
    assert {"stft", "temb", "proj", "conv", "gn_apply", "table", "gemm", "attention", "istft"} <= kinds
    roles = {r["role"] for r in w.p.records}
    assert {"h0m", "xr", "skip", "pd", "combine", "pu", "pnew", "scores", "probs"} <= roles
    e2e = CC.rel_rms(w.p.out, oracle_out())
    print(f"[netcheck sim {DT_IDS[dt]}] end-to-end relative RMS against the float64 oracle {e2e:.2e} (gate {RMS_GATE[dt]:.0e})")
    assert e2e < RMS_GATE[dt]


@pytest.mark.parametrize("two", ["sw", "no_sw"])
@pytest.mark.parametrize("dt", [BF, F32], ids=DT_IDS.get)
def test_walk_follows_the_two_launch_routes(dt, two):
    w = NC.Walk(sim(dt, two_launch=two))
    roles = [r["role"] for r in w.p.records]
    assert "h1p" in roles and (("outp" in roles) == (two == "no_sw"))
    ratios = w.run(select=lambda s: any(o.rec["role"] in ("h1p", "outp") for o in s.outs) or "half" in s.name)
    NC.report(f"sim {DT_IDS[dt]} two-launch {two}", ratios)
    assert w.ran >= 2 and max(ratios.values()) <= 1.0


def test_closure_a_record_nobody_claims_and_a_step_without_record():
    s = sim(F32)
    extra = dict(s.records[10], role="stale")
    prov = type("P", (), {})()
    prov.__dict__.update(s.__dict__)
    prov.tensor, prov.stats, prov.table = s.tensor, s.stats, s.table
    prov.records = s.records[:11] + [extra] + s.records[11:]
    with pytest.raises(AssertionError, match="belong to no step"):
        NC.Walk(prov)
    victim = next(i for i, r in enumerate(s.records) if r["role"] == "pd")
    prov.records = s.records[:victim] + s.records[victim + 1:]
    with pytest.raises(AssertionError, match="skipped a step"):
        NC.Walk(prov)


@pytest.mark.parametrize("fault", FAULTS)
def test_planted_fault_is_caught(fault):
    eq, narrow = cat_block_with_equal_halves()
    # the faults of the residual / 1/sqrt 2 / statistics need a block whose Conv_1 takes a residual tensor: the narrow cat block
    mod = narrow if fault in ("scale_before_res", "stats_before_res") else eq
    under = []
    for dt in (BF, F32):
        clean = CC.rel_rms(sim(dt).out, oracle_out())
        s = sim(dt, fault=(fault, mod))
        e2e = CC.rel_rms(s.out, oracle_out())
        w = NC.Walk(s)
        ratios = w.run(select=lambda st: st.mod in (mod, mod + 1), strict=False)
        worst = max(ratios.values())
        print(f"[netcheck fault {fault} in module {mod}, {DT_IDS[dt]}] end-to-end rel. RMS {clean:.2e} -> {e2e:.2e} (gate {RMS_GATE[dt]:.0e}: "
              f"{'stays under' if e2e < RMS_GATE[dt] else 'breaks it'}); walk's worst err / bound {worst:.3g} in {len(w.failures)} checks")
        if e2e < RMS_GATE[dt]:
            under.append(DT_IDS[dt])
        assert worst > 1.0 and w.failures, f"{fault} ({DT_IDS[dt]}): the walk did not notice"
        with pytest.raises(AssertionError):
            NC.Walk(s).run(select=lambda st: st.mod in (mod, mod + 1))
    print(f"[netcheck fault {fault}] stays under the relative-RMS gate in: {under or 'no type'}")
