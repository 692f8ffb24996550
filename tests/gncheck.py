"""Two instruments for the GroupNorm-apply / FIR x2 resampling kernels of csrc/norm.hip (ops.gn_apply: a caller's scale / shift
table, a forced or dispatched kernel, leading dimensions of the caller's choice), on the pattern of tests/convcheck.py, whose
round_dt, silu64, ulp_of, D_ABS, DOMAIN, assert_elementwise and _ints are used here as they are.

1. EXACT CASES (exact_inputs / exact_reference / check_exact): bit for bit.  x holds integers 0..3, the table is scale = 32,
   shift = 32 in every (b, c): the activated values are 32, 64, 96, 128 with act = 0 and with act = 1 alike (SiLU is the identity
   there in fp32: 1 + exp(-32) == 1).  The [1,3,3,1] x [1,3,3,1] FIR of them is a multiple of 1/2 up to 128 (down) or of 2 (up), the
   FIR of the raw values a multiple of 1/64 up to 3 (down) or of 1/16 (up): all exact in bfloat16, half and float32 in any summation
   order, which exact_reference asserts ON THE REFERENCE (round trip through both 16-bit types; the float32 FIR equals the float64
   one) before anything is compared.  The zero padding of the activated tensor is 0, not SiLU(shift) = 32: a kernel that activates
   the padded column or row of a border output is off by 32 / 8 = 4 there (down; 32 / 4 = 8 up).  Second table, for
   mode 0: scale = 2, shift = -1, act = 0, the engine's 2x - 1; the pyramid launches have no table.  torch.equal on y, on xr, and
   on the extra lanes of padded buffers, which must still hold the NaN they were filled with.
   Sees: a wrong tap, weight, halo, seam, strip end, border row, padding, sample or channel block on one element.  Cannot see:
   rounding behaviour, the SiLU at ordinary arguments.

2. PER-ELEMENT BOUND (GnCheck) on ordinary random data.  Reference in float64 from the STORED x and the SAME fp32 table the kernel
   is given: a = act(x * sc + sh), ref_y = FIR(a), ref_xr = FIR(x).  Per element

       bound_y  = FIR(d_k) + n * 2^-24 * FIR(|a|) + u_out * |ref_y|
       bound_xr =            n * 2^-24 * FIR(|x|) + u_out * |ref_xr|

   d_k: the activated value's own error.  16-bit tensors: D_ABS = 2^-16 on the asserted domain |x sc| + |sh| <= 32 — the kernels run
   the fma and silu_t<bf16_t> chain that convcheck's derivation walks through (one fp32 rounding of v, v_exp_f32, v_rcp_f32).  fp32
   tensors: convcheck's plain-fp32 term 1.1 * 2^-24 (|x sc| + |v|) + (2 sigma(-v) + 2) 2^-24 |a| (silu_t<float>).  FIR(.) of a
   per-element error is the same filter with the same zero padding: a border output sums fewer errors.
   n: fp32 roundings of the filter, each at most 2^-24 of a partial sum, itself at most FIR(|a|): 4 horizontal + 4 vertical steps
   down (n = 8), 2 + 2 up (n = 4), none in mode 0.
   u_out = 2^-7 | 2^-10 (+ 2^-24 absolute in half, for subnormals) | 0: half a storage ulp is u_out / 2 |ref|, the other half covers
   the rounding of a value that is itself off by the rest (as in convcheck).
   gn_fir_down_tiled_kernel only (pre_round=True): it rounds the activated value once to half on the way to LDS, so d_k gains
   u_in * |a| (+ 2^-24) inside the FIR.  Nothing here is fitted to device output.
   Sees: any element off by more than its rounding budget — a seam whose halo reads zero, a halo from the neighbouring sample, a
   stale row at a strip end (tests/test_gncheck_cpu.py shows each passes the relative-RMS gates of 1e-2 / 1.5e-3).  Cannot see: an
   error below one storage ulp of the output; that is what instrument 1 is for.

MEASURED below: worst err / bound the GPU tests printed on the MI355X.  They are records, not gates; the gate is 1.
"""
import numpy as np
import torch

from convcheck import BF, HF, F32, D_ABS, DOMAIN, _ints, assert_elementwise, rel_rms, round_dt, silu64, ulp_of  # noqa: F401
from diffsep_amd import synth

# case family -> worst err / bound on the MI355X (copied from the output of tests/test_gn_gpu.py; records, not gates)
# (y, xr); 16-bit outputs sit just under 0.5, the half ulp of the output rounding against u_out; fp32 outputs have only the n fp32
# roundings and d_k to spend.  Statistics: worst dscale / tolerance 0.894, dshift / tolerance 0.596 over all cases.
MEASURED = {
    "apply mode 0 f32 / bf16 / f16": (0.558, 0.493, 0.485),
    "apply mode 1 (forced) f32 / bf16 / f16": ((0.412, 0.556), (0.489, 0.498), (0.485, 0.498)),
    "apply mode 2 f32 / bf16 / f16": ((0.230, 0.290), (0.480, 0.490), (0.477, 0.491)),
    "pyramid up f32 / bf16 / f16 (xr)": (0.592, 0.498, 0.499), "pyramid down f32 / bf16 / f16 (xr)": (0.290, 0.465, 0.477),
    "2x2 blocks up f32 / bf16 / f16": ((0.334, 0.524), (0.489, 0.498), (0.480, 0.498)),
    "2x2 blocks down f32 / bf16 / f16": ((0.177, 0.171), (0.483, 0.475), (0.459, 0.473)),
    "strips<4> bf16 / f16": ((0.483, 0.494), (0.463, 0.496)), "strips<8> bf16 / f16": ((0.490, 0.498), (0.479, 0.490)),
    "row tiles<4> / <8> / <4> by dispatch": ((0.377, 0.499), (0.387, 0.499), (0.383, 0.499)),
    "up tiles f32 / bf16 / f16": ((0.429, 0.707), (0.497, 0.498), (0.493, 0.500)),
}

RMS_GATE = {BF: 1e-2, HF: 1.5e-3}  # the relative-RMS gates of test_groupnorm_silu_resample / test_f16_elementwise_kernels


# ------------------------------------------------------------------------------------------------ the filter
def _fir_axis(t, axis, mode):
    """[1,3,3,1] x2 resampling along one axis, zeros outside (norm.hip's closed forms):
    down: y[m] = (x[2m-1] + 3 x[2m] + 3 x[2m+1] + x[2m+2]) / 8;  up: y[2m] = x[m-1]/4 + 3 x[m]/4, y[2m+1] = 3 x[m]/4 + x[m+1]/4"""
    t = t.movedim(axis, 0)
    n = t.shape[0]
    z = torch.zeros_like(t[:1])
    p = torch.cat([z, t, z], 0)  # p[i] = x[i - 1]
    if mode == 2:
        assert n % 2 == 0
        out = (p[0:n:2] + 3.0 * p[1:n + 1:2] + 3.0 * p[2:n + 2:2] + p[3:n + 3:2]) / 8.0
    else:
        even = (p[0:n] + 3.0 * p[1:n + 1]) / 4.0
        odd = (3.0 * p[1:n + 1] + p[2:n + 2]) / 4.0
        out = torch.stack([even, odd], 1).reshape((2 * n,) + tuple(t.shape[1:]))
    return out.movedim(0, axis)


def fir(t, mode):
    """NHWC [B,H,W,C]: mode 0 identity, 1 FIR x2 up, 2 FIR x2 down (in t's own precision)"""
    if mode == 0:
        return t
    return _fir_axis(_fir_axis(t, 2, mode), 1, mode)


# ------------------------------------------------------------------------------------------------ 1. exact cases
def exact_inputs(tag, B, H, W, C):
    """x [B,H,W,C] float32 holding integers 0..3, every (sample, channel) plane different (large tensors: one drawn sample, the
    others are its cyclic shifts by (b, 5 b) pixels)"""
    if B * H * W * C <= 1 << 22:
        return _ints(tag + ".x", (B, H, W, C), 0, 3)
    base = _ints(tag + ".x", (H, W, C), 0, 3)
    return torch.stack([torch.roll(base, (b, 5 * b), (0, 1)) for b in range(B)])


def exact_reference(x, table, mode, big=False):
    """(ref_y | None, ref_xr | None) float64 for integer x and table = (scale, shift) constants or None (the pyramid); asserts that
    every number is exact in bfloat16, half and float32 alike.  big: the filter in float32 only (it equals the float64 one on these
    numbers: asserted here on every other case, and in tests/test_gncheck_cpu.py)"""
    xd = x.float() if big else x.double()
    out = []
    for t in ((xd * table[0] + table[1]) if table is not None else None, xd if mode != 0 else None):
        if t is None:
            out.append(None)
            continue
        ref = fir(t, mode)
        if not big:
            assert torch.equal(fir(t.float(), mode).double(), ref), "the float32 filter differs from the float64 one"
        for dt in (BF, HF):
            assert torch.equal(ref.to(dt).to(ref.dtype), ref), f"the exact reference does not survive {dt}"
        out.append(ref)
    if table is not None and table[0] == 32.0:
        v = torch.tensor([32.0, 64.0, 96.0, 128.0])
        assert torch.equal(torch.nn.functional.silu(v), v), "the CPU's float32 SiLU is not the identity at 32, 64, 96, 128"
    return tuple(out)


def _where(bad):
    idx = bad.nonzero()
    b, i, j, k = (int(v) for v in idx[0])
    return (f"{len(idx)} elements differ; first at (b, h, w, c) = ({b}, {i}, {j}, {k}); samples {sorted(set(idx[:, 0].tolist()))[:8]}, "
            f"rows {int(idx[:, 1].min())}..{int(idx[:, 1].max())}, columns {int(idx[:, 2].min())}..{int(idx[:, 2].max())}, "
            f"channels {int(idx[:, 3].min())}..{int(idx[:, 3].max())}"), (b, i, j, k)


def check_lanes(buf, C, dt, what):
    """the lanes beyond C of an output buffer still hold the NaN pattern they were filled with"""
    if buf is not None and buf.shape[-1] > C:
        lanes = buf.detach().cpu()[..., C:].contiguous()
        bits = torch.int32 if dt == F32 else torch.int16
        fill = torch.full(lanes.shape, float("nan"), dtype=dt)
        assert torch.equal(lanes.view(bits), fill.view(bits)), f"{what}: lanes beyond C written"


def check_exact(out, buf, ref, dt, what):
    """torch.equal of a kernel output (the first C lanes) with the exact reference in the storage type, and of the buffer's extra
    lanes with the NaN they were filled with"""
    o = out.detach().cpu()
    want = ref.to(dt)
    assert o.dtype == dt and o.shape == want.shape, f"{what}: {o.dtype} {tuple(o.shape)} for {dt} {tuple(want.shape)}"
    if not torch.equal(o, want):
        msg, at = _where(o != want)
        raise AssertionError(f"{what}: {msg}: kernel {float(o[at])}, reference {float(ref[at])}")
    check_lanes(buf, o.shape[-1], dt, what)


# ------------------------------------------------------------------------------------------------ 2. the per-element bound
def random_inputs(tag, B, H, W, C, dt):
    """x [B,H,W,C] in the storage type (mean 0.3, deviation 1.5, as test_groupnorm_silu_resample), scale, shift [B,C] float32"""
    x = (torch.from_numpy(synth.synth_noise(tag + ".x", (B, H, W, C))) * 1.5 + 0.3).to(dt)
    sc = 1.0 + torch.from_numpy(synth.synth_noise(tag + ".sc", (B, C))) * 0.2
    sh = torch.from_numpy(synth.synth_noise(tag + ".sh", (B, C))) * 0.2
    return x, sc.float(), sh.float()


class GnCheck:
    """Reference and per-element bounds of one case, computed once: x stored tensor [B,H,W,C] of type dt, table (sc, sh) [B,C]
    float32 or None (pyramid: xr only), act 0 / 1, mode 0 / 1 / 2; pre_round: the kernel rounds the activated value to the storage
    type in front of the filter (gn_fir_down_tiled_kernel).  y(...) / xr(...) assert one output and return its worst err / bound."""

    def __init__(self, x, table, act, mode, dt, pre_round=False):
        xd = x.detach().cpu().double()
        assert x.dtype == dt
        u = ulp_of(dt)
        sub = 2.0 ** -24 if dt == HF else 0.0
        n = {0: 0, 1: 4, 2: 8}[mode]
        self.mode, self.dt = mode, dt
        self.a = self.ref_y = self.bound_y = self.ref_xr = self.bound_xr = None
        if table is not None:
            sc, sh = (t.detach().cpu().double()[:, None, None, :] for t in table)
            assert table[0].dtype == torch.float32 and table[1].dtype == torch.float32
            xs = xd * sc
            dom = float((xs.abs() + sh.abs()).max())
            assert dom <= DOMAIN, f"|x sc| + |sh| = {dom} leaves the domain of d_abs"
            v = xs + sh
            a = silu64(v) if act else v
            if dt == F32:  # convcheck's plain-fp32 term
                dk = 1.1 * 2.0 ** -24 * (xs.abs() + v.abs())
                if act:
                    dk = dk + (2.0 * torch.sigmoid(-v) + 2.0) * 2.0 ** -24 * a.abs()
            else:
                dk = torch.full_like(a, D_ABS)
            if pre_round:
                assert dt != F32
                dk = dk + u * a.abs() + sub
            self.a = a
            self.ref_y = fir(a, mode)
            self.bound_y = fir(dk, mode) + n * 2.0 ** -24 * fir(a.abs(), mode) + u * self.ref_y.abs() + sub
        if mode != 0:
            self.ref_xr = fir(xd, mode)
            self.bound_xr = n * 2.0 ** -24 * fir(xd.abs(), mode) + u * self.ref_xr.abs() + sub

    def y(self, out, what):
        return assert_elementwise(out, self.ref_y, self.bound_y, what + " y")

    def xr(self, out, what):
        return assert_elementwise(out, self.ref_xr, self.bound_xr, what + " xr")


def ratio(out, ref, bound):
    """worst err / bound without asserting (the self-test's faults)"""
    err = (out.detach().double().cpu() - ref).abs()
    return float((err / bound.clamp_min(1e-300)).max())


# ------------------------------------------------------------------------------------------------ statistics
def stats_reference(xa, xb, gamma, beta, groups, eps=1e-6):
    """float64 scale, shift [B,C] of GroupNorm over cat([xa, xb], channel) ([B,H,W,C*] holding INTEGERS: the sums below are exact),
    and the asserted tolerances of gn_stats_kernel + gn_finalize_kernel (float64 sums; mean and rstd cast to float, then
    scale = rstd * gamma and shift = beta - mean * scale in fp32):
        |dscale| <= 2^-23 |scale|                                  (the cast and one product)
        |dshift| <= 2^-22 |mean * scale| + 2^-24 |shift|           (cast of the mean, product, the scale's own error; subtraction or fma)
    returns (scale, shift, tol_scale, tol_shift)"""
    x = (torch.cat([xa, xb], -1) if xb is not None else xa).double()
    assert torch.equal(x, x.round()) and float(x.abs().max()) < 2.0 ** 20
    B, H, W, C = x.shape
    s, q = x.sum((1, 2)), (x * x).sum((1, 2))  # exact: integers far below 2^53
    cpg = C // groups
    cnt = float(H * W * cpg)
    mean = (s.reshape(B, groups, cpg).sum(-1) / cnt).repeat_interleave(cpg, 1)
    var = ((q.reshape(B, groups, cpg).sum(-1) / cnt).repeat_interleave(cpg, 1) - mean * mean).clamp_min(0.0)
    scale = gamma.double()[None] / torch.sqrt(var + float(np.float32(eps)))  # (eps is a float argument of the launch)
    shift = beta.double()[None] - mean * scale
    return scale, shift, 2.0 ** -23 * scale.abs(), 2.0 ** -22 * (mean * scale).abs() + 2.0 ** -24 * shift.abs()
