"""The walk: every tensor one score evaluation STORES, checked against the float64 reference of the ONE operation that produced it,
fed with the stored outputs of that operation's producers.  The unit instruments (tests/convcheck.py, gncheck.py, gemmcheck.py,
attn_fused_ref.py, stftcheck.py, sdecheck.py) say whether a kernel computes its operation on the operands it is given; this module says
whether the code BETWEEN the kernels gives each launch the right operands: which tensor, which concat half first, whose GroupNorm
accumulators, which slice of the time-embedding projection, which half of which weight, where the bias, the residual and 1/sqrt 2 go.

The dataflow below is a restatement of oracle/diffsep_oracle.py (ncsnpp_forward, _res_block, _attn_block, score_forward) and of the
model configuration: module order, parameter names all_modules.N.*, the skip stack, cat([h, hs.pop()]), the running offset of a block's
Dense_0 slice (the sum of the out_ch of the residual blocks before it), the two pyramids.  It is not written from the engine: what it
takes from the engine is the TRACE (option "trace", Engine.debug_trace): one record per tensor written, with (module index, role),
shape, arena offset, accumulator offset and, for convolutions, the kernel name.  Records say what was written, never what was read.

A trace provider (the device engine: tests/test_net_walk_gpu.py; a simulated engine: tests/test_netcheck_cpu.py) has
    cfg      dict: nf, num_sources, ch_mult, num_res_blocks, attn_resolution, spec_abs_exponent, spec_factor
    sd       {parameter name: float32 tensor} in the reference layout
    dt, split            storage type of the tensors; split-fp32 products
    records  [dict]      the trace
    tensor(rec), stats(rec)    the stored tensor [B,H,W,C] / its int64 accumulators [B,C,2], on the CPU
    table(sa, sb, gamma, beta, groups, npix)   the (scale, shift) fp32 table the kernels build from accumulators, bit for bit
                         (device: ops.groupnorm_from_acc, tests/test_gn_table_gpu.py)
    xt, t, mix, out      the evaluation's inputs and its result (CPU float32); stft_route "fused" | "split" | "f32"

For every step the walk (1) takes its inputs from the outputs IT identified as the producers', (2) takes the parameters by name,
(3) builds the unit test's instrument on them and (4) asserts err / bound <= 1 per element.  Errors do not compound from layer to
layer (each reference starts from stored values), so the unit bounds apply unchanged in every storage type.  Two closure assertions:
every record of the trace is claimed by exactly one step (nothing the engine stores goes unchecked), and every step finds its record
(the engine skipped nothing).  Which of a block's launch sequences ran is read from the ROLES present: h0m / xr (resampling), skip
(narrow: a separate 1x1), h1p (Conv_0 of a cat(128, 128) block as two launches), outp (its Conv_1 + skip as two launches); a block
with Conv_2 and neither skip nor outp has the skip folded into Conv_1, Conv_2's bias riding as the second bias.

THE PACKED-HALF RULE (stated once; tests/test_f16_gpu.py, test_sw_gpu.py, test_rw_gpu.py apply it case by case): an activated launch of
the half-precision build stages in packed half precision when the recorded kernel is conv3x3_ws1_kernel ("pk"), conv3x3_rw_kernel or
conv3x3_sw_kernel ("pk" when a residual or folded skip shares the accumulators, "pk_fold" otherwise); every other kernel, every raw
launch and every other storage type takes ConvCheck's ordinary model (packed=None).
Likewise GnCheck's pre_round (tests/test_gn_gpu.py): the recorded kernel gn_fir_down_tiled_kernel rounds the activated value to the
storage type in front of the filter; no other resampling kernel does.

ACCUMULATORS (acc_bounds).  A producer adds, per channel and sample, the values v BEFORE the output rounding: per lane an fp32 chain
(one rounding per addend: v_add_f32 / fmaf), the lanes of a block in double, one llrint per block and slot, integer atomics.  Against
the sums of the STORED y = round(v) over the N = H W pixels:
    |v - y| <= h |y|, h = (u/2) (1 + u)            half a storage ulp of v, written in terms of y (u = 2^-7 | 2^-10 | 0; half: + 2^-25)
    |v^2 - y^2| = |v - y| (|v| + |y|) <= h (2 + h) y^2                                            ("a relative u_out on the squares")
    chains: a lane adds at most N values; each addition rounds the running sum, itself at most sum |v|: N 2^-24 sum |v| (sum v^2)
    fixed point: half a quantum per llrint, at most one per addend: N 2^-24 (sum), N 2^-16 (squares)
    bound_sum = (h + N 2^-24 (1 + h)) sum |y| + N (2^-24 + sub),   bound_sq = (h (2 + h) + N 2^-24 (1 + h)^2) sum y^2 + N 2^-16
Nothing here is fitted to device output.

WHAT IT SEES: any stored element outside its own rounding budget, for whatever reason the launch got wrong operands — the neighbouring
block's temb slice, a dropped Conv_2 bias, a table from the other concat half's accumulators, gamma / beta of the wrong half, a batch
stride that matters for B > 1 only, 1/sqrt 2 on the wrong side of the residual, statistics of the wrong tensor
(tests/test_netcheck_cpu.py plants each and prints the end-to-end relative RMS it causes next to the suite's gates).  WHAT IT CANNOT
SEE: an error below one storage ulp of the element; that stays the job of the exact-integer unit cases.

MEASURED below: worst err / bound per step kind on the MI355X, copied from the output of tests/test_net_walk_gpu.py.  Records, not
gates; the gate is 1 everywhere (1.5 E_round for the fused attention block, as tests/test_attn_fused_gpu.py).
"""
import math
from collections import defaultdict
from types import SimpleNamespace

import numpy as np
import torch

import attn_fused_ref as AR
import convcheck as CC
import gemmcheck as GM
import gncheck as GC
import sdecheck as SD
import stftcheck as SC
from diffsep_amd import ops

BF, HF, F32 = CC.BF, CC.HF, CC.F32
INV_SQRT2 = float(np.float32(0.70710678118654752440))  # the fp32 constant of the launch

# engine -> {step kind: worst err / bound} on the MI355X (tests/test_net_walk_gpu.py prints them; records, not gates)
# 256 x 64, B = 2, t = (0.03, 0.8).  16-bit raw launches and resampling sit just under 0.5 (the half ulp of the output rounding
# against u_out), the STFT just under 1 (stftcheck: a value just above a power of two), activated convolutions at 0.12 .. 0.16
# as in the unit tests; the fp32 engines spend a few percent of the convolution bounds and most of the elementwise ones.  The
# accumulators reach 0.87 in 16-bit over a whole walk and 0.02 .. 0.04 on the convolutions of the 256- and 128-row levels alone (the
# B = 4 and nf = 128 rows below).  Fused attention: rel_rms(y, ref_exact) / E_round = 1.000 (bfloat16, y equal to ref_mirror.y bit for bit) and
# 0.999 (half) against the limit 1.5: with the network's weights the residual carries the block's output, so E_round is the
# output rounding itself.
MEASURED = {
    "nf16 f32 (S = 2 | 3)": {"conv3x3 act": (0.020, 0.022), "conv3x3 raw": (0.027, 0.026), "conv1x1 raw": (0.124, 0.103),
                             "pyramid head": (0.017, 0.014), "gn_apply mode 0": (0.871, 0.762), "gn_apply mode 1 y / xr": ((0.417, 0.747), (0.426, 0.745)),
                             "gn_apply mode 2 y / xr": ((0.374, 0.586), (0.374, 0.583)), "fir down / up": ((0.549, 0.691), (0.541, 0.769)),
                             "attention scores / probabilities / output": ((0.049, 0.020, 0.010), (0.048, 0.021, 0.011)), "gemm vt": (0.037, 0.041),
                             "acc sum / squares": ((0.111, 0.125), (0.103, 0.125)), "stft / istft": ((0.004, 0.003), (0.005, 0.003)),
                             "fourier / linear / temb / proj": (0.385, 0.094, 0.008, 0.061)},
    "nf64 bf16": {"conv3x3 act": 0.157, "conv3x3 raw": 0.496, "conv1x1 raw": 0.498, "pyramid head": 0.142, "gn_apply mode 0": 0.470,
                  "gn_apply mode 1 y / xr": (0.497, 0.498), "gn_apply mode 2 y / xr": (0.497, 0.498), "fir down / up": (0.498, 0.498),
                  "attn_fused rel_rms / (1.5 E_round)": 0.667, "attention scores / probabilities / output": (0.859, 0.296, 0.243),
                  "gemm vt": 0.461, "acc sum / squares": (0.701, 0.867), "stft / istft": (0.939, 0.018),
                  "fourier / linear / temb / proj": (0.385, 0.077, 0.003, 0.029)},
    "nf64 bf16 B = 4, the 14 steps whose kernel differs from B = 2": {"conv3x3 act": 0.158, "conv3x3 raw": 0.463, "acc sum / squares": (0.024, 0.032)},
    "nf64 bf16 no_attn_fused, attention blocks": {"gn_apply mode 0": 0.497, "conv1x1 raw": 0.493, "gemm vt": 0.493,
                                                  "attention scores / probabilities / output": (0.972, 0.514, 0.225),
                                                  "acc sum / squares": (0.627, 0.702)},
    "nf64 f16": {"conv3x3 act": 0.140, "conv3x3 act pk": 0.079, "conv3x3 raw": 0.486, "conv1x1 raw": 0.498, "pyramid head": 0.212,
                 "gn_apply mode 0": 0.481, "gn_apply mode 1 y / xr": (0.492, 0.500), "gn_apply mode 2 y / xr": (0.491, 0.499),
                 "fir down / up": (0.499, 0.500), "attn_fused rel_rms / (1.5 E_round)": 0.666,
                 "attention scores / probabilities / output": (0.715, 0.277, 0.265), "gemm vt": 0.432, "acc sum / squares": (0.744, 0.753),
                 "stft / istft": (0.722, 0.019), "fourier / linear / temb / proj": (0.385, 0.077, 0.003, 0.029)},
    "nf64 split": {"conv3x3 act": 0.015, "conv3x3 raw": 0.216, "conv1x1 raw": 0.779, "pyramid head": 0.012, "gn_apply mode 0": 0.857,
                   "gn_apply mode 1 y / xr": (0.433, 0.745), "gn_apply mode 2 y / xr": (0.357, 0.589), "fir down / up": (0.551, 0.651),
                   "attention scores / probabilities / output": (0.096, 0.039, 0.027), "gemm vt": 0.090, "acc sum / squares": (0.297, 0.126),
                   "stft / istft": (0.011, 0.007)},
    "nf64 f32": {"conv3x3 act": 0.005, "conv3x3 raw": 0.027, "conv1x1 raw": 0.111, "pyramid head": 0.004, "gn_apply mode 0": 0.863,
                 "gn_apply mode 1 y / xr": (0.456, 0.790), "gn_apply mode 2 y / xr": (0.410, 0.591), "fir down / up": (0.549, 0.716),
                 "attention scores / probabilities / output": (0.014, 0.006, 0.002), "gemm vt": 0.013, "acc sum / squares": (0.110, 0.125),
                 "stft / istft": (0.004, 0.005)},
    "nf128 bf16 cat(128, 128) blocks: default | no_sw | no_sw + no_split256": {"conv3x3 act": (0.120, 0.115, 0.115), "conv1x1 raw (no_sw)": 0.496,
                                                                             "acc sum / squares": ((0.016, 0.020), (0.024, 0.035), (0.024, 0.035))},
    "nf128 bf16 attention blocks (256 channels: unfused)": {"gn_apply mode 0": 0.496, "conv1x1 raw": 0.487, "gemm vt": 0.482,
                                                           "attention scores / probabilities / output": (0.938, 0.480, 0.299),
                                                           "acc sum / squares": (0.733, 0.709)},
}


def groups_of(C):
    """nn.GroupNorm(min(C // 4, 32), C)"""
    return min(C // 4, 32)


def packed_mode(dt, kernel, activated, shares_accumulators):
    """the packed-half rule of the module docstring"""
    if dt != HF or not activated:
        return None
    if kernel.startswith("conv3x3_ws1_kernel"):
        return "pk"
    if kernel.startswith("conv3x3_rw_kernel") or kernel.startswith("conv3x3_sw_kernel"):
        return "pk" if shares_accumulators else "pk_fold"
    return None


def acc_bounds(y, dt):
    """(sum, bound) and (sum of squares, bound) [B,C] float64 of the stored tensor y [B,H,W,C] (module docstring)"""
    yd = y.double()
    N = yd.shape[1] * yd.shape[2]
    u = CC.ulp_of(dt)
    h = 0.5 * u * (1.0 + u)
    sub = 2.0 ** -25 if dt == HF else 0.0
    chain = N * 2.0 ** -24
    s, q, sa = yd.sum((1, 2)), (yd * yd).sum((1, 2)), yd.abs().sum((1, 2))
    return (s, (h + chain * (1.0 + h)) * sa + N * (2.0 ** -24 + sub)), (q, (h * (2.0 + h) + chain * (1.0 + h) ** 2) * q + N * 2.0 ** -16)


def worst(y, ref, bound):
    """max err / bound; an element with bound 0 must be exact, a non-finite value is infinitely wrong"""
    y = y.detach().double().cpu() if isinstance(y, torch.Tensor) else torch.as_tensor(np.asarray(y), dtype=torch.float64)
    ref = ref if isinstance(ref, torch.Tensor) else torch.from_numpy(np.asarray(ref, np.float64))
    bound = bound if isinstance(bound, torch.Tensor) else torch.from_numpy(np.asarray(bound, np.float64))
    assert tuple(y.shape) == tuple(ref.shape) == tuple(bound.shape), (tuple(y.shape), tuple(ref.shape), tuple(bound.shape))
    if not bool(torch.isfinite(y).all()):
        return float("inf")
    err = (y - ref).abs()
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(r.max())


class Out:
    """a tensor the walk has identified: the record that wrote it"""

    def __init__(self, walk, idx):
        self.walk, self.idx = walk, idx
        self.rec = walk.p.records[idx]

    def t(self):
        return self.walk._tensor(self.idx)

    def acc(self):
        assert self.rec["stats"] >= 0, f"{self.walk._name(self.rec)}: the walk expects accumulators on this tensor, the trace has none"
        return self.walk._stats(self.idx)

    @property
    def C(self):
        return self.rec["C"]

    @property
    def npix(self):
        return self.rec["H"] * self.rec["W"]


class Step:
    def __init__(self, group, kind, name, outs, fn):
        self.group, self.kind, self.name, self.outs, self.fn = group, kind, name, outs, fn
        self.mod = outs[0].rec["mod"] if outs else -1
        self.key = (self.mod, outs[0].rec["role"]) if outs else (-1, name)
        self.kernel = outs[0].rec["kernel"] if outs else ""


class Walk:
    """Builds the list of steps (locating every record: both closure assertions hold once the constructor returns); run() executes the
    checks of the selected steps and returns {kind: worst err / bound}.  strict=False records ratios above 1 instead of raising."""

    def __init__(self, provider):
        self.p = provider
        self.dt, self.split = provider.dt, provider.split
        self.sd = provider.sd
        self.claimed = {}
        self.by_key = defaultdict(list)
        for i, r in enumerate(provider.records):
            self.by_key[(r["mod"], r["role"])].append(i)
        self.steps = []
        self._cache = {}
        self.ratios = defaultdict(float)
        self.strict = True
        self.failures = []
        self._build()
        left = [self._name(r) for i, r in enumerate(provider.records) if i not in self.claimed]
        assert not left, f"{len(left)} records of the trace belong to no step of the reference's dataflow (stored, never checked): {left[:8]}"

    # ------------------------------------------------------------------ records
    @staticmethod
    def _name(r):
        return f"module {r['mod']} {r['role']} ({r['kind']} {r['B']}x{r['H']}x{r['W']}x{r['C']} {r['kernel']})"

    def take(self, mod, role, optional=False, stats=None):
        """the next unclaimed record (module, role); claims it.  Missing: None if optional, else the engine skipped a step."""
        for i in self.by_key.get((mod, role), ()):
            if i not in self.claimed:
                self.claimed[i] = True
                o = Out(self, i)
                if stats is not None:
                    assert (o.rec["stats"] >= 0) == stats, f"{self._name(o.rec)}: accumulators {'missing' if stats else 'unexpected'}"
                return o
        assert optional, f"the trace has no record for module {mod} role '{role}': the engine skipped a step of the reference's dataflow"
        return None

    def _tensor(self, i):
        if ("t", i) not in self._cache:
            self._cache[("t", i)] = self.p.tensor(self.p.records[i])
        return self._cache[("t", i)]

    def _stats(self, i):
        if ("s", i) not in self._cache:
            self._cache[("s", i)] = self.p.stats(self.p.records[i])
        return self._cache[("s", i)]

    def par(self, name):
        assert name in self.sd, f"the state dict has no parameter '{name}'"
        return self.sd[name].detach().cpu().float()

    # ------------------------------------------------------------------ comparison
    def cmp(self, kind, y, ref, bound, what, limit=1.0):
        r = worst(y, ref, bound) / limit
        self.ratios[kind] = max(self.ratios[kind], r)
        if not r <= 1.0:
            msg = f"{what} [{kind}]: worst err / bound {r:.3g}"
            if self.strict:
                if isinstance(ref, torch.Tensor) and isinstance(y, torch.Tensor) and limit == 1.0:
                    CC.assert_elementwise(y, ref, bound, what)  # (raises with the element's position)
                raise AssertionError(msg)
            self.failures.append(msg)
        return r

    def exact(self, cond, what):
        if not cond:
            self.ratios["exact"] = float("inf")
            if self.strict:
                raise AssertionError(what)
            self.failures.append(what)

    def check_acc(self, o, what):
        """the accumulator pair of a stored tensor against the sums of that tensor"""
        (s, bs), (q, bq) = acc_bounds(o.t(), self.dt)
        got = ops.stats_to_float(o.acc())
        self.cmp("acc sum", got[..., 0], s, bs, what + " channel sums")
        self.cmp("acc squares", got[..., 1], q, bq, what + " channel sums of squares")

    def table(self, a, b, gamma, beta, npix):
        C = a.C + (b.C if b is not None else 0)
        sc, sh = self.p.table(a.acc(), b.acc() if b is not None else None, gamma, beta, groups_of(C), npix)
        return sc.detach().cpu().float(), sh.detach().cpu().float()

    def conv(self, out, x, gn, w, what, bias=None, bb=None, res=None, skip=None, out_scale=1.0, cout=None, kind=None):
        """ConvCheck of one launch on the stored operands; x / skip sources are Out handles, res an Out"""
        a, b = x
        xs = (a.t(), b.t() if b is not None else None)
        cin = a.C + (b.C if b is not None else 0)
        if w.shape[1] < cin:  # (channel padding of the packed spectrogram: the packed weight has zeros there)
            w = torch.nn.functional.pad(w, (0, 0, 0, 0, 0, cin - w.shape[1]))
        sk = None
        if skip is not None:
            sa, sb, sw = skip
            sk = (sa.t(), sb.t() if sb is not None else None, sw)
        packed = packed_mode(self.dt, out.rec["kernel"], gn is not None, res is not None or skip is not None)
        cc = CC.ConvCheck(xs, gn, w, self.dt, bias=bias, bb=bb, res=res.t() if res is not None else None, skip=sk,
                          out_scale=out_scale, split=self.split, packed=packed, cout=cout)
        CO = cc.CO
        y = out.t()
        k = kind or (("conv3x3" if w.shape[-1] == 3 else "conv1x1") + (" act" if gn is not None else " raw") + (f" {packed}" if packed else ""))
        self.cmp(k, y[..., :CO], cc.ref[..., :CO], cc.bound[..., :CO], what)
        if y.shape[-1] > CO:
            self.exact(not bool(y[..., CO:].any()), f"{what}: padding channels [{CO}, {y.shape[-1]}) not zero")
        if out.rec["stats"] >= 0:
            self.check_acc(out, what)

    def add(self, group, kind, name, outs, fn):
        self.steps.append(Step(group, kind, name, outs, fn))

    # ------------------------------------------------------------------ the dataflow (oracle/diffsep_oracle.py)
    def _build(self):
        c, p = self.p.cfg, self.p
        nf, S, L, nrb = c["nf"], c["num_sources"], len(c["ch_mult"]), c["num_res_blocks"]
        chan_in = 2 * S + 2
        self.chan_in = chan_in
        # ---- pre_process: STFT of cat(xt, mix), compressed, packed, 2 x - 1
        x0 = self.take(-1, "x0")
        self.rows = x0.rec["H"]
        self.add("front", "stft", "x0", [x0], lambda: self._stft(x0))
        # ---- time embedding and every block's Dense_0(act(temb)), side by side in module order
        emb, t1, temb, proj = (self.take(-1, r) for r in ("emb", "t1", "temb", "proj"))
        self.proj = proj
        self.add("front", "temb", "time embedding", [emb, t1, temb], lambda: self._temb(emb, t1, temb))
        self.dense = []  # (module index, out_ch) of the residual blocks in module order: the projection's layout
        self.add("front", "proj", "dense projection", [proj], lambda: self._proj(temb, proj))
        self.mi = 3
        self.off = 0
        cin = self.take(3, "conv_in", stats=True)
        pre = "all_modules.3."
        self.add(("down", self.rows), "conv", "input conv", [cin],
                 lambda: self.conv(cin, (x0, None), None, self.par(pre + "weight"), "input conv", bias=self.par(pre + "bias")))
        self.mi = 4
        hs = [cin]
        pyr_in = x0
        h = cin
        for i in range(L):
            for _ in range(nrb):
                h = self.res_block("down", (hs[-1], None))
                if h.rec["H"] == c["attn_resolution"]:
                    h = self.attn_block("down", h)
                hs.append(h)
            if i != L - 1:
                h = self.res_block("down", (hs[-1], None), down=True)
                pyr_in, h = self.combine(pyr_in, h)
                hs.append(h)
        h = self.res_block("mid", (hs[-1], None))
        h = self.attn_block("mid", h)
        h = self.res_block("mid", (h, None))
        pyramid = None
        for i in reversed(range(L)):
            for _ in range(nrb + 1):
                h = self.res_block("up", (h, hs.pop()))
            if h.rec["H"] == c["attn_resolution"]:
                h = self.attn_block("up", h)
            pyramid = self.pyramid_head(h, pyramid)
            if i != 0:
                h = self.res_block("up", (h, None), up=True)
        assert not hs
        assert self.off == proj.C, f"the residual blocks' out_ch sum to {self.off}, the projection has {proj.C} columns"
        # ---- post_process: output_layer(pyramid / t), decompress, iSTFT
        if p.out is not None:
            self.add("back", "istft", "score output", [], lambda: self._istft(pyramid))

    def _next(self):
        self.mi += 1
        return self.mi - 1, f"all_modules.{self.mi - 1}."

    def res_block(self, seg, x, up=False, down=False):
        """ResnetBlockBigGANpp.forward (_res_block); x = (first, second | None) sources of the concat"""
        mi, pre = self._next()
        a, b = x
        in_ch = a.C + (b.C if b is not None else 0)
        w0 = self.par(pre + "Conv_0.weight")
        out_ch = w0.shape[0]
        assert w0.shape[1] == in_ch, f"module {mi}: Conv_0 takes {w0.shape[1]} channels, the walk's sources have {in_ch}"
        off = self.off
        self.off += out_ch
        self.dense.append((mi, out_ch))
        has2 = (pre + "Conv_2.weight") in self.sd
        mode = 1 if up else (2 if down else 0)
        Hin = a.rec["H"]
        Ho = 2 * Hin if up else (Hin // 2 if down else Hin)
        g0w, g0b = self.par(pre + "GroupNorm_0.weight"), self.par(pre + "GroupNorm_0.bias")
        g1w, g1b = self.par(pre + "GroupNorm_1.weight"), self.par(pre + "GroupNorm_1.bias")
        b0, w1, b1 = self.par(pre + "Conv_0.bias"), self.par(pre + "Conv_1.weight"), self.par(pre + "Conv_1.bias")
        w2, b2 = (self.par(pre + "Conv_2.weight"), self.par(pre + "Conv_2.bias")) if has2 else (None, None)
        group = (seg, Ho)
        tag = f"module {mi} ({'cat ' if b is not None else ''}{in_ch}->{out_ch}{' up' if up else ' down' if down else ''})"
        table0 = lambda: self.table(a, b, g0w, g0b, a.npix)
        temb = lambda: self.proj.t().reshape(self.proj.rec["B"], -1)[:, off:off + out_ch]
        sc_r, sh_r = self.take(mi, "scale", optional=True), self.take(mi, "shift", optional=True)
        if sc_r is not None or sh_r is not None:
            assert sc_r is not None and sh_r is not None
            self.add(group, "table", tag + " GroupNorm_0 table", [sc_r, sh_r], lambda: self._table_arrays(sc_r, sh_r, table0, tag))
        xr = x
        if mode:
            assert b is None
            h0m, xrr = self.take(mi, "h0m", stats=False), self.take(mi, "xr", stats=False)
            xr = (xrr, None)

            def resample():
                g = GC.GnCheck(a.t(), table0(), 1, mode, self.dt, pre_round=h0m.rec["kernel"].startswith("gn_fir_down_tiled_kernel"))
                self.cmp(f"gn_apply mode {mode} y", h0m.t(), g.ref_y, g.bound_y, tag + " h0m")
                self.cmp(f"gn_apply mode {mode} xr", xrr.t(), g.ref_xr, g.bound_xr, tag + " xr")
            self.add(group, "gn_apply", tag + " h0m / xr", [h0m, xrr], resample)
            h1 = self.take(mi, "h1", stats=True)
            self.add(group, "conv", tag + " Conv_0", [h1], lambda: self.conv(h1, (h0m, None), None, w0, tag + " Conv_0", bias=b0, bb=temb()))
        else:
            h1p = self.take(mi, "h1p", optional=True, stats=False)
            h1 = self.take(mi, "h1", stats=True)
            if h1p is not None:  # conv(cat(a, b)) = conv_a(a) + conv_b(b), the second launch taking the first's result as its residual
                assert b is not None
                C1 = a.C

                def first():
                    sc, sh = table0()
                    self.conv(h1p, (a, None), (sc[:, :C1], sh[:, :C1], 1), w0[:, :C1], tag + " Conv_0 first half", bias=b0, bb=temb())

                def second():
                    sc, sh = table0()
                    self.conv(h1, (b, None), (sc[:, C1:], sh[:, C1:], 1), w0[:, C1:], tag + " Conv_0 second half", res=h1p)
                self.add(group, "conv", tag + " Conv_0 first half", [h1p], first)
                self.add(group, "conv", tag + " Conv_0 second half", [h1], second)
            else:
                def conv0():
                    sc, sh = table0()
                    self.conv(h1, (a, b), (sc, sh, 1), w0, tag + " Conv_0", bias=b0, bb=temb())
                self.add(group, "conv", tag + " Conv_0", [h1], conv0)
        table1 = lambda: self.table(h1, None, g1w, g1b, h1.npix) + (1,)
        outp = self.take(mi, "outp", optional=True, stats=False)
        skip = self.take(mi, "skip", optional=True, stats=False)
        out = self.take(mi, "out", stats=True)
        B = out.rec["B"]
        if outp is not None:  # Conv_1 with the first half of Conv_2 folded, then the 1x1 of the second half on top
            assert has2 and b is not None and skip is None
            C1 = a.C
            self.add(group, "conv", tag + " Conv_1 + first skip half", [outp],
                     lambda: self.conv(outp, (h1, None), table1(), w1, tag + " Conv_1 + first skip half", bias=b1, bb=b2[None].expand(B, -1),
                                       skip=(a, None, w2[:, :C1])))
            self.add(group, "conv", tag + " second skip half", [out],
                     lambda: self.conv(out, (b, None), None, w2[:, C1:], tag + " second skip half", res=outp, out_scale=INV_SQRT2))
        elif skip is not None:  # narrow blocks: Conv_2 as a launch of its own
            assert has2
            self.add(group, "conv", tag + " Conv_2", [skip], lambda: self.conv(skip, xr, None, w2, tag + " Conv_2", bias=b2))
            self.add(group, "conv", tag + " Conv_1", [out],
                     lambda: self.conv(out, (h1, None), table1(), w1, tag + " Conv_1", bias=b1, res=skip, out_scale=INV_SQRT2))
        elif has2:  # Conv_2 folded into Conv_1 as extra K, its bias as the second bias
            self.add(group, "conv", tag + " Conv_1 + folded Conv_2", [out],
                     lambda: self.conv(out, (h1, None), table1(), w1, tag + " Conv_1 + folded Conv_2", bias=b1, bb=b2[None].expand(B, -1),
                                       skip=(xr[0], xr[1], w2), out_scale=INV_SQRT2))
        else:
            assert xr[1] is None, f"{tag}: identity skip on a concat"
            self.add(group, "conv", tag + " Conv_1", [out],
                     lambda: self.conv(out, (h1, None), table1(), w1, tag + " Conv_1", bias=b1, res=xr[0], out_scale=INV_SQRT2))
        return out

    def _table_arrays(self, sc_r, sh_r, table, what):
        """materialised scale / shift arrays: the kernels' own table of the sources' accumulators, bit for bit"""
        assert sc_r.rec["kind"] == "gn_finalize", f"{what}: a score evaluation finalizes every table from accumulators, not {sc_r.rec['kind']}"
        sc, sh = table()
        B = sc.shape[0]
        self.exact(torch.equal(sc_r.t().reshape(B, -1), sc) and torch.equal(sh_r.t().reshape(B, -1), sh),
                   f"{what}: the stored scale / shift arrays are not the table of the sources' accumulators")
        self.ratios["table"] = max(self.ratios["table"], 0.0)

    def attn_block(self, seg, x):
        """AttnBlockpp.forward (_attn_block)"""
        mi, pre = self._next()
        C, B, H, W = x.C, x.rec["B"], x.rec["H"], x.rec["W"]
        L = H * W
        group = (seg, H)
        tag = f"module {mi} (attention {C}, L = {L})"
        gw, gb = self.par(pre + "GroupNorm_0.weight"), self.par(pre + "GroupNorm_0.bias")
        Wn = [self.par(pre + f"NIN_{k}.W") for k in range(4)]  # [in][out]
        bn = [self.par(pre + f"NIN_{k}.b") for k in range(4)]
        table = lambda: self.table(x, None, gw, gb, L)
        h = self.take(mi, "h", optional=True, stats=False)
        out = self.take(mi, "out", stats=True)
        if h is None:  # the whole block in one launch
            assert out.rec["kind"] == "attn_fused", f"{tag}: no h record and the output is not the fused kernel's"
            self.add(group, "attn_fused", tag + " fused", [out], lambda: self._attn_fused(x, out, table, Wn, bn, tag))
            return out
        sc_r, sh_r = self.take(mi, "scale"), self.take(mi, "shift")
        self.add(group, "table", tag + " table", [sc_r, sh_r], lambda: self._table_arrays(sc_r, sh_r, table, tag))

        def gn():
            g = GC.GnCheck(x.t(), table(), 0, 0, self.dt)
            self.cmp("gn_apply mode 0", h.t(), g.ref_y, g.bound_y, tag + " h")
        self.add(group, "gn_apply", tag + " h", [h], gn)
        q, k = self.take(mi, "q", stats=False), self.take(mi, "k", stats=False)
        nin = lambda i: Wn[i].T.contiguous()[:, :, None, None]  # NIN: y = x @ W + b, as a 1x1 convolution OIHW
        self.add(group, "conv", tag + " q", [q], lambda: self.conv(q, (h, None), None, nin(0), tag + " q", bias=bn[0]))
        self.add(group, "conv", tag + " k", [k], lambda: self.conv(k, (h, None), None, nin(1), tag + " k", bias=bn[1]))
        vt, s, pr, o = (self.take(mi, r, stats=False) for r in ("vt", "scores", "probs", "o"))

        def vt_step():  # V^T[b, c, l] = sum_c' Wv[c', c] h[b, l, c'] + b[c]: A = the stored Wv^T, Bt = h, bias along the rows
            a = Wn[2].T.contiguous()
            a = a if self.dt == F32 else a.to(self.dt)
            g = GM.GemmCheck(a, h.t().reshape(B, L, C), self.dt, B=B, bias=bn[2], bias_mode=1, split=self.split)
            self.cmp("gemm vt", vt.t().reshape(B, C, -1)[..., :L], g.ref, g.bound, tag + " V^T")

        def core():
            v = vt.t().reshape(B, C, -1)[..., :L].transpose(1, 2)
            ac = GM.AttnCheck(q.t().reshape(B, L, C), k.t().reshape(B, L, C), v, self.dt, split=self.split)
            self.cmp("attention scores", s.t().reshape(B, L, -1)[..., :L], ac.s, ac.s_bound, tag + " scores")
            pc = pr.t().reshape(B, L, -1)
            self.exact(not bool(pc[..., L:].any()), f"{tag}: probability padding columns [L, Lp) not zero")
            self.cmp("attention probabilities", pc[..., :L], ac.p, ac.p_bound, tag + " probabilities")
            self.cmp("attention output", o.t().reshape(B, L, C), ac.o, ac.o_bound, tag + " o")
        self.add(group, "gemm", tag + " V^T", [vt], vt_step)
        self.add(group, "attention", tag + " scores / probabilities / o", [s, pr, o], core)
        self.add(group, "conv", tag + " out", [out],
                 lambda: self.conv(out, (o, None), None, nin(3), tag + " out", bias=bn[3], res=x, out_scale=INV_SQRT2))
        return out

    def _attn_fused(self, x, out, table, Wn, bn, tag):
        """the block-level instrument of tests/attn_fused_ref.py on the stored input and the table of its accumulators: gate 1
        (rel_rms(y, ref_exact) <= 1.5 E_round, E_round = rel_rms(ref_mirror.y, ref_exact.v) from the references alone)"""
        B, L, C = x.rec["B"], x.npix, x.C
        assert C == AR.C
        dt = self.dt
        xs = x.t().reshape(B, L, C)
        sc, sh = table()
        Wq, Wk, Wv, Wo = (w.double() for w in Wn)
        ex = SimpleNamespace(x=xs, scale=sc.double(), shift=sh.double(), M=Wk @ Wq.T, bq=Wk @ bn[0].double(), Wv=Wv.T, bv=bn[2], Wo=Wo.T,
                             bo=bn[3], L=L)
        mir = SimpleNamespace(x=xs, scale=sc, shift=sh, M=(Wk.float() @ Wq.float().T).to(dt), bq=Wk.float() @ bn[0], Wv=Wv.T.to(dt), bv=bn[2],
                              Wo=Wo.T.to(dt), bo=bn[3], L=L)
        e, m = AR.attn_ref(ex), AR.attn_ref(mir, mirror=True)
        E = AR.rel_rms(m.y, e.v)
        y = out.t().reshape(B, L, C)
        r = AR.rel_rms(y, e.v) / E if bool(torch.isfinite(y.float()).all()) else float("inf")
        print(f"[netcheck {tag}] E_round {E:.2e}  exact {r:.3f} (limit 1.5)  mirror {AR.rel_rms(y, m.y) / E:.3f}")
        self.ratios["attn_fused (rel_rms / 1.5 E_round)"] = max(self.ratios["attn_fused (rel_rms / 1.5 E_round)"], r / 1.5)
        if not r <= 1.5:
            msg = f"{tag}: rel_rms against ref_exact is {r:.3f} E_round (limit 1.5)"
            if self.strict:
                raise AssertionError(msg)
            self.failures.append(msg)
        self.check_acc(out, tag)

    def combine(self, pyr_in, h):
        """pyr = fir_down2(pyr); h = Conv_0(pyr) + h   (Combine 'sum')"""
        mi, pre = self._next()
        pd = self.take(mi, "pd", stats=False)
        hc = self.take(mi, "combine", stats=True)
        group = ("down", hc.rec["H"])
        tag = f"module {mi} (Combine)"

        def down():
            g = GC.GnCheck(pyr_in.t(), None, 0, 2, self.dt)
            self.cmp("fir down", pd.t(), g.ref_xr, g.bound_xr, tag + " pd")
        self.add(group, "gn_apply", tag + " pd", [pd], down)
        self.add(group, "conv", tag, [hc], lambda: self.conv(hc, (pd, None), None, self.par(pre + "Conv_0.weight"), tag,
                                                              bias=self.par(pre + "Conv_0.bias"), res=h))
        return pd, hc

    def pyramid_head(self, h, pyramid):
        """ph = conv3x3(act(GN(h))); pyramid = ph | fir_up2(pyramid) + ph"""
        gi, gpre = self._next()
        mi, pre = self._next()
        gw, gb = self.par(gpre + "weight"), self.par(gpre + "bias")
        w, bias = self.par(pre + "weight"), self.par(pre + "bias")
        group = ("up", h.rec["H"])
        tag = f"module {mi} (pyramid head {h.C})"
        table = lambda: self.table(h, None, gw, gb, h.npix)
        sc_r, sh_r = self.take(mi, "scale", optional=True), self.take(mi, "shift", optional=True)
        if sc_r is not None:
            self.add(group, "table", tag + " table", [sc_r, sh_r], lambda: self._table_arrays(sc_r, sh_r, table, tag))
        pu = None
        if pyramid is not None:
            pu = self.take(mi, "pu", stats=False)

            def up():
                g = GC.GnCheck(pyramid.t(), None, 0, 1, self.dt)
                self.cmp("fir up", pu.t(), g.ref_xr, g.bound_xr, tag + " pu")
            self.add(group, "gn_apply", tag + " pu", [pu], up)
        pnew = self.take(mi, "pnew", stats=False)
        self.add(group, "conv", tag, [pnew], lambda: self.conv(pnew, (h, None), table() + (1,), w, tag, bias=bias, res=pu, cout=self.chan_in,
                                                               kind="pyramid head"))
        return pnew

    # ------------------------------------------------------------------ front and back
    def _stft(self, x0):
        p, c = self.p, self.p.cfg
        y = x0.t()
        if x0.rec["kind"] != "stft":
            raise AssertionError("the walk checks score evaluations (x0 from the STFT)")
        ref = SC.stft_ref(p.xt, p.mix, x0.rec["W"], c["spec_abs_exponent"], c["spec_factor"], shift=True)
        self.cmp("stft", y, ref["y"], SC.stft_bound(ref, p.stft_route, self.dt), "x0 = packed STFT")

    def _temb(self, emb, t1, temb):
        B = emb.rec["B"]
        t = SD._tt(self.p.t)
        Wf = SD.f64(self.par("all_modules.0.W"))
        w1, b1, w2, b2 = (self.par(n) for n in ("all_modules.1.weight", "all_modules.1.bias", "all_modules.2.weight", "all_modules.2.bias"))
        nf = Wf.shape[0]
        xp = np.log(t)[:, None] * Wf[None] * 2.0 * SD.PI32
        e_xp = np.abs(xp) * (SD.fu("logf") + 2.0)
        ref = np.concatenate([np.sin(xp), np.cos(xp)], -1)
        e_emb = np.concatenate([e_xp, e_xp], -1) + SD.fu("sinf") * np.abs(ref)
        self.cmp("fourier", emb.t().reshape(B, -1), ref, SD.U * e_emb, "Fourier embedding")
        es = SD.f64(emb.t().reshape(B, -1))
        y1, e1 = SD._linear(es, np.zeros_like(es), SD.f64(w1), SD.f64(b1), math.ceil(2 * nf / 64) + 7)
        self.cmp("linear", t1.t().reshape(B, -1), y1, SD.U * e1, "Linear_1 of the stored embedding")
        ref, bound = SD.time_embedding(self.p.t, self.par("all_modules.0.W"), w1, b1, w2, b2)
        self.cmp("temb", temb.t().reshape(B, -1), ref, bound, "time embedding")

    def _proj(self, temb, proj):
        B = proj.rec["B"]
        ws = [self.par(f"all_modules.{mi}.Dense_0.weight") for mi, _ in self.dense]
        bs = [self.par(f"all_modules.{mi}.Dense_0.bias") for mi, _ in self.dense]
        ref, bound = SD.dense_projection(temb.t().reshape(B, -1), ws, bs)
        self.cmp("proj", proj.t().reshape(B, -1), ref, bound, "dense projection of every block, in module order")

    def _istft(self, pyramid):
        p, c = self.p, self.p.cfg
        S = c["num_sources"]
        T = p.xt.shape[-1]
        ow = self.par("output_layer.weight")[:, :, 0, 0]
        ref = SC.istft_ref(pyramid.t(), S, T, c["spec_abs_exponent"], c["spec_factor"], ow=ow, ob=self.par("output_layer.bias"),
                           tdiv=torch.as_tensor(np.asarray(p.t, np.float32)))
        self.cmp("istft", p.out, ref["out"], SC.istft_bound(ref, p.stft_route), "score = iSTFT(output_layer(pyramid / t))")

    # ------------------------------------------------------------------ running
    def groups(self):
        out = []
        for s in self.steps:
            if s.group not in out:
                out.append(s.group)
        return out

    def run(self, select=None, strict=True):
        """execute the checks of the steps select(step) accepts (default: all); {kind: worst err / bound}"""
        self.strict = strict
        self.ratios = defaultdict(float)
        self.failures = []
        n = 0
        for s in self.steps:
            if select is None or select(s):
                s.fn()
                n += 1
        self.ran = n
        return dict(self.ratios)


def report(tag, ratios):
    for k in sorted(ratios):
        print(f"[netcheck {tag}] {k}: worst err / bound {ratios[k]:.3f}")


def cfg_dict(nf, num_sources=2, ch_mult=(1, 1, 2, 2, 2, 2, 2), num_res_blocks=2, attn_resolution=16, spec_abs_exponent=0.5,
             spec_factor=0.33):
    return dict(nf=nf, num_sources=num_sources, ch_mult=tuple(ch_mult), num_res_blocks=num_res_blocks, attn_resolution=attn_resolution,
                n_fft=510, hop=128, spec_abs_exponent=spec_abs_exponent, spec_factor=spec_factor)


class EngineProvider:
    """the device engine as a trace provider: one eager score evaluation with option "trace" on; tensors are copied from the arena
    on demand (the arena keeps one forward's intermediates until the next call)"""

    def __init__(self, eng, sd, cfg, xt, t, mix, options=()):
        from diffsep_amd import _lib
        self.eng, self.cfg = eng, cfg
        self.sd = {k: torch.as_tensor(np.asarray(v)) for k, v in sd.items()}
        self.dt = eng.storage_dtype()
        self.split = eng.cfg.dtype == _lib.F32_SPLIT
        self.stft_route = "fused" if self.dt != F32 else ("split" if self.split else "f32")
        self.xt, self.t, self.mix = xt, t, mix
        for o in options:
            eng.set_option(o, 1)
        eng.set_option("trace", 1)
        try:
            self.out = eng.score(xt.cuda(), t.cuda(), mix.cuda()).cpu()
            torch.cuda.synchronize()
            self.records = eng.debug_trace()
        finally:
            eng.set_option("trace", 0)
            for o in options:
                eng.set_option(o, 0)
        # the arena belongs to the engine and its next call overwrites it: one copy of the span the records cover, now
        esz = torch.empty((), dtype=self.dt).element_size()
        spans = [(r["offset"], r["offset"] + r["B"] * r["H"] * r["W"] * r["ld"] * (4 if r["f32"] else esz)) for r in self.records]
        spans += [(r["stats"], r["stats"] + r["B"] * r["C"] * 16) for r in self.records if r["stats"] >= 0]
        assert all(lo >= 0 for lo, _ in spans), "a record of a score evaluation lies outside the arena"
        self.lo = min(lo for lo, _ in spans) // 16 * 16
        self.snap = eng.debug_arena()[0][self.lo:max(hi for _, hi in spans)].cpu()

    def _shifted(self, rec):
        return dict(rec, offset=rec["offset"] - self.lo, stats=rec["stats"] - self.lo if rec["stats"] >= 0 else -1)

    def tensor(self, rec):
        return self.eng.trace_view(self._shifted(rec), self.snap).contiguous()

    def stats(self, rec):
        return self.eng.trace_stats(self._shifted(rec), self.snap).contiguous()

    def table(self, sa, sb, gamma, beta, groups, npix):
        sc, sh = ops.groupnorm_from_acc(sa.cuda(), sb.cuda() if sb is not None else None, gamma.cuda(), beta.cuda(), groups, npix)
        return sc.cpu(), sh.cpu()
