"""tests/stftcheck.py tested without a GPU: the float64 references are the oracle's operations, the simulated (correct) fused kernels
stay inside the derived bounds on every input of tests/test_stft_gpu.py, and six injected faults that pass a relative-RMS gate of
the older tests break the bounds."""
import pytest
import torch

import diffsep_oracle as O
import stftcheck as sc
from stftcheck import BF, HF

torch.set_grad_enabled(False)
KIND = {BF: "bf16", HF: "f16"}


def _cfg(S, exponent=0.5, factor=0.33):
    cfg = O.default_config(16, S)
    cfg["spec_factor"], cfg["spec_abs_exponent"] = sc.f32(factor), sc.f32(exponent)  # the float32 values the C entry points receive
    return cfg


# ------------------------------------------------------------------------------------------------ the references are the oracle's
# 1e-12 of the element's own scale: the sum of magnitudes that forms it (compressed: factor A^e; inverse: sum_f P / env).  An element
# at a zero crossing has no relative accuracy in ANY float64 evaluation (the FFT's error is 1e-16 of that same sum), and the oracle's
# exp(1j * angle) leaves 1e-16 |z| in the imaginary parts of DC and Nyquist, which are exactly 0 here.
@pytest.mark.parametrize("T", [300, 3713, 3714, 4000])
@pytest.mark.parametrize("S", [1, 2, 3])
def test_references_equal_the_oracle_in_float64(S, T):
    cfg = _cfg(S)
    xt, mix = sc.signal(f"ref.{T}.{S}", 2, S, T)
    spec, _, n_pad = O.pre_process(cfg, torch.cat([xt, mix], 1).double())
    W = spec.shape[-1]
    r = sc.stft_ref(xt, mix, W)
    assert W - n_pad == r["F"] == sc.n_frames(T)
    mine = r["y"][..., :2 * (S + 1)].permute(0, 3, 1, 2)
    A = r["A_re"] + r["A_im"]
    scale = torch.zeros_like(mine)
    scale[..., :r["F"]] = (r["fac"] * torch.cat([A, A], -1) ** r["e"]).permute(0, 3, 1, 2)
    assert bool(((mine - spec).abs() <= 1e-12 * scale).all()), float(((mine - spec).abs() / scale.clamp(min=1e-300)).max())
    assert not bool(r["y"][..., 2 * (S + 1):].any()) and not bool(mine[..., r["F"]:].any())
    shifted = sc.stft_ref(xt, mix, W, shift=True)["y"][..., :2 * (S + 1)].permute(0, 3, 1, 2)
    assert bool(((shifted - (2 * spec - 1)).abs() <= 2e-12 * scale).all())

    x = sc.pixels(f"ref.p.{T}.{S}", 2, S, T, torch.float32, W=W).double()
    want = O.post_process(cfg, x[..., :2 * S].permute(0, 3, 1, 2).contiguous(), T, n_pad)
    ri = sc.istft_ref(x, S, T)
    assert ri["out"].shape == want.shape == (2, S, T)
    assert bool(((ri["out"] - want).abs() <= 1e-12 * ri["Pola"] / ri["env"]).all())


@pytest.mark.parametrize("S,e", [(1, 0.5), (2, 0.7), (3, 1.0)])
def test_reference_with_output_layer_equals_oracle_layer_then_post_process(S, e):
    T, B = 3713, 2
    cfg = _cfg(S, exponent=e)
    W = sc.width(T, 64)
    x = sc.pixels(f"ref.l.{S}", B, S, T, torch.float32, W=W, fill=None).double()
    ow, ob, tdiv = sc.layer(f"ref.l.{S}", B, S)
    h = x[..., :2 * (S + 1)].permute(0, 3, 1, 2) / tdiv.double()[:, None, None, None]     # scale_by_sigma, then the 1x1 convolution
    v = torch.nn.functional.conv2d(h, ow.double()[:, :, None, None], ob.double())
    want = O.post_process(cfg, v, T, W - sc.n_frames(T))
    ri = sc.istft_ref(x, S, T, e, 0.33, ow, ob, tdiv)
    assert bool(((ri["out"] - want).abs() <= 1e-12 * ri["Pola"] / ri["env"]).all())
    assert float(tdiv.max() / tdiv.min()) > 10.0


def test_compression_bound_holds_on_random_pairs():
    # |g(z + dz) - g(z)| <= compress_bound(|z|, |dz|, e) for g(z) = z |z|^(e-1): both branches, |dz| from far below to far above |z|
    g = lambda z, e: z * z.abs().clamp(min=1e-300) ** (e - 1.0)
    for e in (0.5, 0.7, 0.25, 1.0):
        z = torch.complex(sc.rnd(f"cb.zr.{e}", (20000,)).double(), sc.rnd(f"cb.zi.{e}", (20000,)).double())
        d = torch.complex(sc.rnd(f"cb.dr.{e}", (20000,)).double(), sc.rnd(f"cb.di.{e}", (20000,)).double())
        d = d * 10.0 ** (sc.rnd(f"cb.s.{e}", (20000,)).double() * 3.0 - 3.0).clamp(-8.0, 3.0)   # (below 1e-8 the float64 difference is noise)
        got = (g(z + d, e) - g(z, e)).abs()
        assert bool((got <= sc.compress_bound(z.abs(), d.abs(), e) * (1 + 1e-7)).all()), e


# ------------------------------------------------------------------------------------------------ correct simulated kernels
@pytest.mark.parametrize("dt", [BF, HF], ids=["bf16", "f16"])
def test_simulated_fused_stft_is_inside_the_bound(dt):
    worst = {}
    for cid, c in sc.fwd_cases():
        xt, mix = sc.fwd_input(cid, c)
        W = sc.FWD_W[c["T"]]
        ref = sc.stft_ref(xt, mix, W, c["exponent"], c["factor"], c["shift"])
        y = sc.sim_stft_fused(xt, mix, W, c["exponent"], c["factor"], c["shift"], dt)
        r = sc.worst_ratio(y, ref["y"], sc.stft_bound(ref, "fused", dt))
        fam = "cancelling" if c["kind"] == "cancel" else "noise"
        worst[fam] = max(worst.get(fam, 0.0), r)
        print(f"[sim stft {KIND[dt]} {cid}] err / bound {r:.3f}")
        assert r < 1.0, (cid, r)
    xt, mix = sc.impulse_input()
    ref = sc.stft_ref(xt, mix, 64)
    y = sc.sim_stft_fused(xt, mix, 64, out_dt=dt)
    worst["impulse"] = sc.worst_ratio(y, ref["y"], sc.stft_bound(ref, "fused", dt))
    assert worst["impulse"] < 1.0
    print(f"[sim stft {KIND[dt]}] worst err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("dt", [BF, HF], ids=["bf16", "f16"])
def test_simulated_fused_istft_is_inside_the_bound(dt):
    worst = {}
    for cid, c in sc.inv_cases():
        if c["kind"] == "large" and dt != HF:
            continue
        x, lay = sc.inv_input(cid, c, dt)
        ref = sc.istft_ref(x, c["S"], c["T"], c["exponent"], c["factor"], *lay)
        y = sc.sim_istft_fused(x, c["S"], c["T"], c["exponent"], c["factor"], *lay)
        bound = sc.istft_bound(ref, "fused")
        r = sc.worst_ratio(y, ref["out"], bound)
        fam = "large" if c["kind"] == "large" else ("layer" if c["layer"] else "noise")
        worst[fam] = max(worst.get(fam, 0.0), r)
        print(f"[sim istft {KIND[dt]} {cid}] err / bound {r:.3f}, mean bound / mean |out| {float(bound.mean() / ref['out'].abs().mean()):.2e}")
        assert r < 1.0, (cid, r)
    for f in sc.ONEHOT_F:
        x, _ = sc.onehot_input(f, dt)
        ref = sc.istft_ref(x, 2, sc.ONEHOT_T)
        y = sc.sim_istft_fused(x, 2, sc.ONEHOT_T)
        worst["one-hot"] = max(worst.get("one-hot", 0.0), sc.worst_ratio(y, ref["out"], sc.istft_bound(ref, "fused")))
    assert worst["one-hot"] < 1.0
    print(f"[sim istft {KIND[dt]}] worst err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


# ------------------------------------------------------------------------------------------------ injected faults
# Every fault is run at T = 32000, S = 2, B = 2, a shape of the older tests' RMS gates (a gate divides by the whole tensor's energy:
# the shorter the signal, the more it sees), with the simulated kernel of the named build, and must (a) pass that build's gate
# and (b) break the bound.  The swapped bin passes only the bfloat16 gate, the missing frame only the bfloat16 round-trip gate.
FWD_GATE = {BF: 5e-3, HF: 6e-4}      # test_fused_stft_matches_oracle
RT_GATE = {BF: 1e-2, HF: 1e-3}       # the round trip of test_fused_istft_matches_oracle_and_roundtrip, the one gate on the inverse
#                                      transform that compares with something outside the project at S != 2 or T != 4000


@pytest.fixture(scope="module")
def fwd_fault_case():
    xt, mix = sc.signal("fault.fwd", 2, 2, 32000)
    W = sc.width(32000, 64)
    return xt, mix, W, sc.stft_ref(xt, mix, W)


@pytest.mark.parametrize("dt,fault,what", [
    (BF, ("hop", 1, 0, 32, 2), "frame 32 (first of the second tile) reads one 16-tap fragment one hop early"),
    (HF, ("hop", 1, 0, 32, 2), "frame 32 (first of the second tile) reads one 16-tap fragment one hop early"),
    (BF, ("swap", 1, 0, 40, 127), "Re and Im of bin 127 (last of the first row half) change places in one frame"),
    (BF, ("swap", 1, 0, 40, 128), "Re and Im of bin 128 (first of the second row half) change places in one frame"),
    (BF, ("lo", 1, 0, 1), "the lo plane of one channel's samples is dropped in one tile"),
    (HF, ("lo", 1, 0, 1), "the lo plane of one channel's samples is dropped in one tile")])
def test_forward_fault_passes_the_rms_gate_and_breaks_the_bound(fwd_fault_case, dt, fault, what):
    xt, mix, W, ref = fwd_fault_case
    y = sc.sim_stft_fused(xt, mix, W, out_dt=dt, fault=fault)
    rms, ratio = sc.rel_rms(y, ref["y"]), sc.worst_ratio(y, ref["y"], sc.stft_bound(ref, "fused", dt))
    print(f"[fault {KIND[dt]}: {what}] rel rms {rms:.2e} (gate {FWD_GATE[dt]:g}), err / bound {ratio:.1f}")
    assert rms < FWD_GATE[dt]
    assert ratio > 1.0


@pytest.fixture(scope="module")
def inv_fault_case():
    T, S, B = 32000, 2, 2
    x = sc.pixels("fault.inv", B, S, T, BF, W=sc.width(T, 64), fill=None)
    lay = sc.layer("fault.inv", B, S)
    return x, lay, T, S


@pytest.mark.parametrize("dt,fault,what", [
    (BF, ("miss_prev", 1, 0, 1), "the first 128 samples of segment 1 miss frame 28, the previous segment's last"),
    (BF, ("stale", 1, 1, 3712, 2), "overlap-add copy 2 is read one sample early at the seam of segments 0 and 1"),
    (HF, ("stale", 1, 1, 3712, 2), "overlap-add copy 2 is read one sample early at the seam of segments 0 and 1")])
def test_inverse_fault_passes_the_rms_gate_and_breaks_the_bound(inv_fault_case, dt, fault, what):
    x, _, T, S = inv_fault_case
    x = x.float().to(dt)
    ref = sc.istft_ref(x, S, T)
    y = sc.sim_istft_fused(x, S, T, fault=fault)
    rms, ratio = sc.rel_rms(y, ref["out"]), sc.worst_ratio(y, ref["out"], sc.istft_bound(ref, "fused"))
    print(f"[fault {KIND[dt]}: {what}] rel rms {rms:.2e} (gate {RT_GATE[dt]:g}), err / bound {ratio:.1f}")
    assert rms < RT_GATE[dt]
    assert ratio > 1.0


def test_missing_bias_passes_the_rms_gate_and_breaks_the_bound(inv_fault_case):
    # ob omitted for the imaginary channel of source 1, everywhere.  Only the end-to-end gates (1e-2 at best) see the output layer.
    x, (ow, ob, tdiv), T, S = inv_fault_case
    ref = sc.istft_ref(x, S, T, 0.5, 0.33, ow, ob, tdiv)
    ob_bad = ob.clone()
    ob_bad[S + 1] = 0.0
    y = sc.sim_istft_fused(x, S, T, 0.5, 0.33, ow, ob_bad, tdiv)
    rms, ratio = sc.rel_rms(y, ref["out"]), sc.worst_ratio(y, ref["out"], sc.istft_bound(ref, "fused"))
    print(f"[fault bf16: the bias of source 1's imaginary channel is omitted] rel rms {rms:.2e} (gate 1e-2), err / bound {ratio:.1f}")
    assert rms < 1e-2
    assert ratio > 1.0


# ------------------------------------------------------------------------------------------------ the vacuous branch
def test_istft_length_always_exceeds_the_signal():
    # 128 (F - 1) > T for every T at n_fft = 510, hop = 128: the zero-tail code of istft_ola_kernel and istft_fused_kernel (samples
    # beyond the iSTFT's own length, `t >= 128 (F - 1)`) is UNREACHABLE in this configuration, and so are the older tests'
    # `if T > 128 * (F_ - 1)` assertions.  No test here or in tests/test_stft_gpu.py claims to have run it.
    assert all(sc.HOP * (sc.n_frames(T) - 1) > T for T in range(1, 20001))
