"""Round-5 GPU tests, all through the C-ABI:
  * the shipped default at the published width (dtype "auto" = hybrid at nf = 128, spec_factor 0.15) against the CPU oracle at
    the FULL utterance length (T = 32000, N = 30, injected noise) — round 4 had that gate at T = 8000 only;
  * the range margin of half-precision storage: the largest |activation| of a score evaluation (every tensor scanned, both ends
    of the time axis, mixture peak x 1 and x 100) leaves a factor >= 8 to 65504 at nf = 64 and nf = 128; the all-weights-x-s
    sweep of the round-4 review is run for the record (it compounds along the un-normalised trunk);
  * batch (in)dependence at the bench's batch: the f16 engine on B = 16 against sixteen B = 1 calls with the same per-utterance
    seeds agrees to the mode's rounding (the dispatch depends on B); the fp32 engine bit for bit;
  * overflow through the layers the round-4 test did not touch: an attention NIN weight and a weight that feeds a GroupNorm
    accumulator of a large level are scaled past the half-precision range: the net must still see it (non-finite samples)
    and the split twin's result must be returned.
"""
import warnings

import numpy as np
import pytest
import torch

import diffsep_oracle as O
from diffsep_amd import _lib, ops, synth
from diffsep_amd.engine import Engine, pack_state_dict, param_table
from diffsep_amd.pl_model import DiffSepModel, default_config, HYBRID_HEAD_STEPS

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda"
SDE2 = dict(ndim=2, d_lambda=2.0, sigma_min=0.05, sigma_max=0.5)


def rms(a):
    return float(a.detach().double().pow(2).mean().sqrt())


def rel_rms(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return rms(a - b) / (rms(b) + 1e-30)


def rnd(tag, shape, scale=1.0):
    return torch.from_numpy(synth.synth_noise(tag, shape)) * scale


def make_engine(nf, dtype, sd=None, seed=7, spec_factor=0.33, **kw):
    cfg = _lib.model_config(nf=nf, num_sources=2, dtype=dtype, spec_factor=spec_factor)
    if sd is None:
        sd = synth.synth_state_dict([(n, s) for n, s, _ in param_table(cfg)], seed)
    return Engine(cfg, pack_state_dict(cfg, sd), **kw), sd


# ------------------------------------------------------------------------------------------------ nf = 128, full length
def test_nf128_hybrid_default_full_length_parity_with_oracle():
    # ~2 - 4 minutes of CPU oracle (60 evaluations of the nf = 128 network at 256 x 256), once per session
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    cfg = O.default_config(128, 2, spec_factor=0.15)
    T, N = 32000, 30
    eng16, sd = make_engine(128, _lib.F16, spec_factor=0.15)
    head, _ = make_engine(128, _lib.F32_SPLIT, sd=sd, spec_factor=0.15, lib_kind="f16")
    mix = torch.from_numpy(synth.synth_batch(1, T=T)[0])
    draws = [rnd(f"n128full.z{i}", (1, 2, T)) for i in range(1 + 2 * N)]
    ref, nfe = O.separate(O.to_torch(sd), cfg, mix, draws, N=N, corrector_steps=1, snr=0.5, eps=0.03, denoise=True)
    mn, _, _ = ops.normalize_batch(mix.to(DEV))
    kw = dict(N=N, corrector_steps=1, snr=0.5, eps=0.03, denoise=True, noise=torch.stack(draws).to(DEV))
    seph, nfeh = eng16.pc_sample(mn, SDE2, tail=head, head_steps=HYBRID_HEAD_STEPS, **kw)
    outh = ops.scale_output(mix.to(DEV), seph).cpu()
    dh, rh = rms(outh - ref), rel_rms(outh, ref)
    out16 = ops.scale_output(mix.to(DEV), eng16.pc_sample(mn, SDE2, **kw)[0]).cpu()
    print(f"\n[nf128 hybrid (the shipped default) T=32000 N30 vs oracle, injected noise] out rms {rms(ref):.4f} diff rms {dh:.3e} "
          f"rel {rh:.3e}; f16 alone {rms(out16 - ref):.3e} / {rel_rms(out16, ref):.3e}")
    assert nfe == nfeh == 60 and torch.isfinite(outh).all()
    assert dh < 1e-3 and rh < 1e-2, f"hybrid default at T = 32000: {dh:.3e} abs / {rh:.3e} rel RMS from the oracle"


# ------------------------------------------------------------------------------------------------ range margin of f16
def _scaled_state(nf, s, spec_factor):
    cfg = _lib.model_config(nf=nf, num_sources=2, spec_factor=spec_factor)
    sd = synth.synth_state_dict([(n, sh) for n, sh, _ in param_table(cfg)], 7)
    out = {}
    for k, v in sd.items():
        conv = k.endswith(".weight") and v.ndim == 4          # every 3x3 / 1x1 convolution kernel
        nin = k.endswith(".W") and v.ndim == 2                 # the attention blocks' NIN matrices
        out[k] = (v * np.float32(s)).astype(np.float32) if (conv or nin) else v
    return out


@pytest.mark.parametrize("nf,spec_factor", [(64, 0.33), (128, 0.15)])
def test_f16_range_margin(nf, spec_factor):
    # (i) How far is the half-precision engine from 65504?  Every activation tensor of one score evaluation is scanned
    # (engine option "track_tensors", diffsep_engine_debug_absmax) at both ends of the time axis and for a mixture 100 x
    # louder (normalize_batch divides the scale out, the state x_t is what the sampler makes of it): the largest |value|
    # anywhere must leave a factor >= 8.
    T, B = 32000, 2
    eng, sd = make_engine(nf, _lib.F16, spec_factor=spec_factor)
    eng.set_option("track_tensors", 1)
    mix = torch.from_numpy(synth.synth_batch(B, T=T)[0]).to(DEV)
    worst, where = 0.0, None
    for peak in (1.0, 100.0):
        mn, _, _ = ops.normalize_batch(mix * peak)
        for tv in (1.0, 0.5, 0.03):
            t = torch.full((B,), tv, device=DEV)
            xt = ops.sde_prior(SDE2, mn, rnd(f"rng.z{tv}", (B, 2, T)).to(DEV)) if tv == 1.0 else (0.5 * mn.expand(B, 2, T) + tv * rnd(f"rng.x{tv}", (B, 2, T)).to(DEV)).contiguous()
            out = eng.score(xt, t, mn)
            assert torch.isfinite(out).all()
            scan = eng.debug_absmax()
            assert len(scan) > 100 and all(bad == 0 for _, bad, _, _ in scan)
            i = max(range(len(scan)), key=lambda k: scan[k][0])
            if scan[i][0] > worst:
                worst, where = scan[i][0], (i, scan[i][2], scan[i][3], tv, peak)
            top = sorted(scan, key=lambda r: -r[0])[:3]
            print(f"[f16 range nf={nf} t={tv} peak x{peak:g}] largest |activation| {scan[i][0]:.1f} (tensor {i}: {scan[i][2]} rows, {scan[i][3]} channels); "
                  f"next {[round(r[0], 1) for r in top[1:]]}")
    margin = 65504.0 / worst
    print(f"[f16 range nf={nf}] largest |activation| of the network {worst:.1f} at {where}: margin {margin:.0f}x to 65504")
    assert margin >= 8.0, f"half-precision range margin at nf = {nf} is only {margin:.1f}x"
    eng.close()
    # (ii) ALL convolution / NIN matrices x s at once (the sweep of the round-4 review), for the record: the factor compounds
    # along the un-normalised trunk (every up / down block's 1x1 skip multiplies it again), so s = 4 stands for 4^k on the trunk
    # after k such blocks — the first s that trips the overflow net says little about a single layer's headroom, (i) does.
    mnb, _, _ = ops.normalize_batch(mix)
    first_bad = None
    for s_ in (2, 4, 8):
        e2, _ = make_engine(nf, _lib.F16, sd=_scaled_state(nf, s_, spec_factor), spec_factor=spec_factor)
        sep, _ = e2.pc_sample(mnb[:, :, :16000].contiguous(), SDE2, N=2, corrector_steps=1, snr=0.5, eps=0.03, denoise=True, seed=9)
        ok = bool(torch.isfinite(sep).all())
        e2.close()
        print(f"[f16 range nf={nf}] all conv / NIN weights x {s_}: {'finite' if ok else 'NON-FINITE (the net repeats such a batch on the split engine)'}")
        if not ok:
            first_bad = s_
            break
    assert first_bad is None or first_bad >= 4


# ------------------------------------------------------------------------------------------------ batch independence
def test_f16_batch_of_16_equals_sixteen_single_calls():
    T, N, B = 32000, 2, 16
    eng, _ = make_engine(64, _lib.F16)
    mix = torch.from_numpy(synth.synth_batch(B, T=T)[0]).to(DEV)
    mn, _, _ = ops.normalize_batch(mix)
    seeds = [1000 + 7 * i for i in range(B)]
    kw = dict(N=N, corrector_steps=1, snr=0.5, eps=0.03, denoise=True)
    full, nfe = eng.pc_sample(mn, SDE2, seeds=seeds, lengths=[T] * B, **kw)
    assert nfe == 4 and torch.isfinite(full).all()
    worst = 0.0
    nbits = 0
    for i in range(B):
        one, _ = eng.pc_sample(mn[i:i + 1].contiguous(), SDE2, seeds=[seeds[i]], lengths=[T], **kw)
        if torch.equal(one[0], full[i]):
            nbits += 1
        worst = max(worst, rel_rms(one[0], full[i]))
    print(f"\n[f16 B=16 vs 16 x B=1] bit-identical utterances {nbits}/16, worst rel rms {worst:.3e} after {nfe} evaluations")
    # NOT bit-identical, and not expected to be: the kernel DISPATCH depends on the batch (a launch with fewer tiles than CUs
    # stays on the weight-stationary / generic tiles: at B = 1 that is every level below 256 rows), and those kernels round
    # differently (fp32 instead of packed-half activation, other summation orders); inside one kernel the GroupNorm partial
    # sums of the persistent blocks depend on the tile range, i.e. on B.  What holds is agreement at the level of the mode's
    # own rounding (the f16 engine is 3.5e-3 from the fp32 engine after 60 evaluations) ...
    assert worst < 1e-2
    # ... and for the fp32 engine, whose kernels are exact fmaf chains in a fixed order, batch independence bit for bit:
    e32, _ = make_engine(16, _lib.F32)
    mixs = torch.from_numpy(synth.synth_batch(4, T=8000)[0]).to(DEV)
    mns, _, _ = ops.normalize_batch(mixs)
    full32, _ = e32.pc_sample(mns, SDE2, seeds=seeds[:4], lengths=[8000] * 4, **kw)
    for i in range(4):
        one, _ = e32.pc_sample(mns[i:i + 1].contiguous(), SDE2, seeds=[seeds[i]], lengths=[8000], **kw)
        assert torch.equal(one[0], full32[i]), f"fp32 engine: utterance {i} depends on the batch it rides in"


# ------------------------------------------------------------------------------------------------ overflow elsewhere
@pytest.mark.parametrize("key,scale", [("attn_nin", 3.0e5), ("gn_feeder_32row", 2.0e5)])
def test_f16_overflow_in_attention_and_in_front_of_groupnorm_reaches_the_net(key, scale):
    nf = 16
    cfg = _lib.model_config(nf=nf, num_sources=2)
    sd = synth.synth_state_dict([(n, s) for n, s, _ in param_table(cfg)], 7)
    if key == "attn_nin":      # the value projection of the first attention block (module 21: NIN_2.W)
        name = next(k for k in sd if k.startswith("all_modules.21.") and k.endswith("NIN_2.W"))
    else:                      # Conv_0 of the first residual block of the 32-row level: its output (~2e5 in EVERY pixel) feeds
        # GroupNorm_1's fixed-point accumulators.  (Not a 256-row layer: int64 sums of squares at scale 2^16 hold 65536 pixels of
        # |v| <= 4.6e4 per channel — a tensor that is past the half-precision range in every pixel of a large level is past the
        # accumulators' range too, for every engine)
        name = "all_modules.16.Conv_0.weight"
    sd[name] = (sd[name] * np.float32(scale)).astype(np.float32)
    state = {"backbone." + k: torch.from_numpy(v) for k, v in sd.items()}
    B, T, N = 2, 4000, 2
    mix = torch.from_numpy(synth.synth_batch(B, T=T)[0]).to(DEV)
    m16 = DiffSepModel(default_config(nf=nf), dtype="f16")
    m16.load_state_dict(state)
    (mn, _), *_ = m16.normalize_batch((mix, None))
    kw = dict(N=N, corrector_steps=1, snr=0.5, seed=11)
    raw, _ = m16.get_pc_sampler("reverse_diffusion", "ald2", mn, check_finite=False, **kw)()
    assert not bool(torch.isfinite(raw).all()), f"{name} x {scale:g} was meant to overflow half precision visibly"
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        est, nfe = m16.get_pc_sampler("reverse_diffusion", "ald2", mn, **kw)()
    assert nfe == 4 and bool(torch.isfinite(est).all()) and m16.fallback_batches == 1
    msp = DiffSepModel(default_config(nf=nf), dtype="split")
    msp.load_state_dict(state)
    direct, _ = msp.get_pc_sampler("reverse_diffusion", "ald2", mn, **kw)()
    assert torch.equal(est, direct)
    # new weights AFTER the fallback exists: the twin follows (advisor finding of round 4)
    sd2 = synth.synth_state_dict([(n, s) for n, s, _ in param_table(cfg)], 8)
    sd2[name] = (sd2[name] * np.float32(scale)).astype(np.float32)
    state2 = {"backbone." + k: torch.from_numpy(v) for k, v in sd2.items()}
    m16.load_state_dict(state2)
    msp.load_state_dict(state2)
    est2, _ = m16.get_pc_sampler("reverse_diffusion", "ald2", mn, **kw)()
    direct2, _ = msp.get_pc_sampler("reverse_diffusion", "ald2", mn, **kw)()
    assert m16.fallback_batches == 2 and torch.equal(est2, direct2) and not torch.equal(est2, est)


# ------------------------------------------------------------------------------------------------ fused STFT / iSTFT (16-bit engines)
@pytest.mark.parametrize("dtype,tol", [(torch.float16, 6e-4), (torch.bfloat16, 5e-3)])
@pytest.mark.parametrize("T,S", [(4000, 2), (31999, 2), (32000, 2), (32001, 2), (100000, 3), (300, 1)])
def test_fused_stft_matches_oracle(dtype, tol, T, S):
    # stft_fused_kernel (one launch: frames from LDS, hi / lo split products, compress + pack in the accumulator layout) against
    # the oracle's pre_process; the only difference allowed is the storage rounding of the output tensor
    cfg = O.default_config(16, S)
    x = rnd(f"r5.stft.{T}.{S}", (2, S + 1, T), 0.3)
    spec, _, n_pad = O.pre_process(cfg, x)
    W = spec.shape[-1]
    y = ops.stft_pack(x[:, :S].contiguous().to(DEV), x[:, S:].contiguous().to(DEV), W, 8, dtype=dtype)
    assert ops.last_conv_kernel("f16" if dtype == torch.float16 else "bf16") == f"stft_fused_kernel<{S + 1}>"
    assert y.dtype == dtype
    got = ops.to_nchw(y.float(), 2 * (S + 1)).cpu()
    assert rel_rms(got, spec) < tol
    # against the fp32 launch sequence on the same input: the transform itself agrees to 2e-5 before the storage rounding
    y32 = ops.to_nchw(ops.stft_pack(x[:, :S].contiguous().to(DEV), x[:, S:].contiguous().to(DEV), W, 8), 2 * (S + 1)).cpu()
    assert rel_rms(got, y32.to(dtype).float()) < tol / 2
    F_ = W - n_pad
    if n_pad:
        assert float(got[..., F_:].abs().max()) == 0.0
    y2 = ops.to_nchw(ops.stft_pack(x[:, :S].contiguous().to(DEV), x[:, S:].contiguous().to(DEV), W, 8, shift=True, dtype=dtype).float(),
                     2 * (S + 1)).cpu()
    assert rel_rms(y2, 2 * spec - 1) < tol
    if n_pad:
        assert torch.all(y2[..., F_:] == -1.0)
    assert torch.all(ops.stft_pack(x[:, :S].contiguous().to(DEV), x[:, S:].contiguous().to(DEV), W, 8, shift=True, dtype=dtype)[..., 2 * (S + 1):] == 0)


def test_fused_stft_frame_indexing_bit_exact():
    # an impulse at sample n0 appears in exactly the frames whose support [128 f - 255, 128 f + 255) contains it (tap 0 of the
    # periodic Hann window is exactly 0) — the frame arithmetic of the fused kernel (LDS sample index 128 r + n) is torch.stft's
    T, W = 2000, 64
    for n0 in (0, 1, 254, 255, 256, 1000, 1999):
        x = torch.zeros(1, 3, T)
        x[0, 0, n0] = 1.0
        y = ops.to_nchw(ops.stft_pack(x[:, :2].contiguous().to(DEV), x[:, 2:].contiguous().to(DEV), W, 8, dtype=torch.float16).float(), 6).cpu()
        energy = (y[0, 0] ** 2 + y[0, 3] ** 2).sum(0)
        F_ = 1 + (T + 382) // 128
        hit = [f for f in range(W) if energy[f] > 0]
        n_in = lambda f: n0 - (128 * f - 255)
        want = [f for f in range(F_) if 1 <= n_in(f) <= 509]
        assert hit == want, (n0, hit, want)
        assert float((y[0, 1] ** 2 + y[0, 4] ** 2 + y[0, 2] ** 2 + y[0, 5] ** 2).sum()) == 0.0   # the silent channels stay silent


@pytest.mark.parametrize("dtype,tol", [(torch.float16, 1e-3), (torch.bfloat16, 1e-2)])
@pytest.mark.parametrize("T,S", [(4000, 2), (32000, 2), (31999, 2), (100000, 3), (300, 1)])
def test_fused_istft_matches_oracle_and_roundtrip(dtype, tol, T, S):
    # istft_fused_kernel (decompress, inverse DFT, overlap-add, envelope in one launch) against the fp32 launch sequence on the
    # SAME (already rounded) 16-bit input — the transform is exact to 2e-5 — and a round trip through both fused kernels
    F_ = 1 + (T + 382) // 128
    W = 64 * ((F_ + 63) // 64)
    yy = rnd(f"r5.istft.{T}.{S}", (2, 2 * S, 256, W), 0.2)
    x16 = ops.to_nhwc(yy, 8).to(DEV, dtype)
    out = ops.istft_unpack(x16, S, T)
    assert ops.last_conv_kernel("f16" if dtype == torch.float16 else "bf16") == f"istft_fused_kernel<{2 if S == 2 else 1},0>"
    ref = ops.istft_unpack(x16.float(), S, T)     # fp32 kernels on the same values
    assert ops.last_conv_kernel() == "istft_ola_kernel"
    assert out.shape == (2, S, T) and torch.isfinite(out).all()
    assert rel_rms(out, ref) < 3e-5
    if T > 128 * (F_ - 1):                        # beyond the iSTFT length adjust_length pads zeros (score_models.py:99-105)
        assert torch.all(out[..., 128 * (F_ - 1):] == 0)
    x = rnd(f"r5.rt.{T}", (2, S + 1, T), 0.3)
    spec = ops.stft_pack(x[:, :S].contiguous().to(DEV), x[:, S:].contiguous().to(DEV), W, 8, dtype=dtype)
    sel = torch.zeros_like(spec)
    for s_ in range(S):
        sel[..., s_] = spec[..., s_]
        sel[..., S + s_] = spec[..., S + 1 + s_]
    back = ops.istft_unpack(sel, S, T)
    n_ok = min(T, 128 * (F_ - 1))
    assert rel_rms(back[..., :n_ok].cpu(), x[:, :S, :n_ok]) < tol
