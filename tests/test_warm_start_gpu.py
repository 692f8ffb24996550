"""Warm start and the sampler's open ends on the MI355X: diffsep_warm_start (ops.warm_start), diffsep_pc_sample_from
(Engine.pc_sample(x_init=, first_step=, last_step=), sdes.get_pc_sampler(...), DiffSepModel.refine, separate --init-dir).
The tiny engine of tests/test_trace_gpu.py (nf = 16, S = 2, synthetic weights of seed 7) and its mixed lengths, which share one
padded width; float64 references and bounds in tests/warm_start_ref.py (notation of tests/sdecheck.py).

MEASURED on the MI355X (records copied from this file's output, not gates): see DESIGN.md section 5k."""
import ctypes as C

import numpy as np
import pytest
import torch

import diffsep_oracle as O
import sdecheck as K
import warm_start_ref as W
from diffsep_amd import _lib, ops, sdes, synth, wavio
from diffsep_amd import separate as sep_cli
from diffsep_amd.engine import param_table
from diffsep_amd.pl_model import DiffSepModel, default_config
from test_trace_gpu import LENS, MIX, S, SEEDS, Injected, engine, model16, padded

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

PMIX = dict(MIX, kind=_lib.SDE_PRIORMIX, avg_len=510)
T3 = np.array([0.03, 0.5, 1.0], np.float32)
_cache = {}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------- 1. the perturbation against the float64 reference
def perturb_case(kind, S_, T):
    tag = f"ws.{kind}.{S_}.{T}"
    B = 3
    lens = [T, max(1, T - 3), (T + 1) // 2]
    est = K.noise(tag + ".e", (B, S_, T), 0.3)
    mixn = K.noise(tag + ".y", (B, 1, T))
    raw = (K.noise(tag + ".r", (B, 1, T), 0.2) + est.sum(1, keepdims=True)).astype(np.float32)
    z = K.noise(tag + ".z", (B, S_, T))
    for b, L in enumerate(lens):  # (the mixture of a zero-padded batch is zero beyond the length, as the sampler keeps it)
        mixn[b, :, L:] = 0.0
    mean = np.array([0.01, -0.02, 0.0], np.float32)
    std = np.array([0.11, 0.07, 0.3], np.float32)
    return dict(B=B, lens=lens, est=est, mixn=mixn, raw=raw, z=z, mean=mean, std=std)


@pytest.mark.parametrize("T", [1, 255, 1000, 4099])
@pytest.mark.parametrize("S_", [2, 3])
@pytest.mark.parametrize("kind", ["mix", "priormix"])
def test_perturbation_against_float64_reference(kind, S_, T):
    c = perturb_case(kind, S_, T)
    sde = dict(PMIX if kind == "priormix" else MIX, ndim=S_)
    est, mixn, raw, z = (dev(c[k]) for k in ("est", "mixn", "raw", "z"))
    mean, std, t = dev(c["mean"]), dev(c["std"]), dev(T3)
    smix = ops.sde_sigma_mix(mixn, 510).cpu().numpy() if kind == "priormix" else None  # (a stored input of the reference)
    worst = {}
    for lens in (None, c["lens"]):
        for scale, mean_from in (("none", "mix"), ("none", "estimate"), ("ls", "mix")):
            x, gains, fb = ops.warm_start(sde, est, raw, mixn, mean, std, t, scale=scale, mean_from=mean_from, noise=z, lengths=lens)
            g = None
            if scale == "ls":  # (one sample: the Gram matrix of S >= 2 estimates has rank 1, the fit falls back to gains of 1)
                assert fb.tolist() == ([1, 1, 1] if T == 1 else [0, 0, 0])
                g = gains.cpu().numpy()
                assert T > 1 or bool((gains == 1.0).all())
            else:
                assert bool((gains == 1.0).all()) and int(fb.sum()) == 0
            rb = W.perturb(sde, c["est"], c["mixn"], c["mean"], c["std"], T3, c["z"], gains=g, smix=smix, mean_from=mean_from,
                           lengths=lens)
            what = f"warm_start {kind} S={S_} T={T} {scale}/{mean_from} lens={lens is not None}"
            worst[what] = K.check(x, rb, what)
            if lens is not None:
                for b, L in enumerate(lens):
                    assert float(x[b, :, L:].abs().max() if L < T else 0.0) == 0.0, (what, b)
    print({k: round(v, 3) for k, v in worst.items()})


# ---------------------------------------------------------------- 2. device noise
def noise_inputs():
    if "noise" not in _cache:
        mixn, tgt = padded()
        T = max(LENS)
        est = torch.zeros_like(tgt)
        for b, L in enumerate(LENS):
            est[b, :, :L] = 0.8 * tgt[b, :, :L] + 0.05 * tgt[b, :, :L].flip(0)
            est[b, :, L:] = 9.0  # (never read)
        raw = torch.zeros(len(LENS), 1, T, device="cuda")
        for b, L in enumerate(LENS):
            raw[b, :, :L] = torch.from_numpy(synth.synth_mixture(b, T=L)[0]).cuda()
        mean = torch.tensor([0.0, 0.01, -0.01], device="cuda")
        std = torch.tensor([0.2, 0.25, 0.15], device="cuda")
        _cache["noise"] = (est, raw, mixn, mean, std, torch.tensor([0.5, 0.5, 0.25], device="cuda"))
    return _cache["noise"]


@pytest.mark.parametrize("kind", ["mix", "priormix"])
def test_device_noise_is_draw_zero_of_the_sampler(kind):
    sde = PMIX if kind == "priormix" else MIX
    est, raw, mixn, mean, std, t = noise_inputs()
    B, _, T = mixn.shape
    a = ops.warm_start(sde, est, raw, mixn, mean, std, t, seeds=SEEDS, lengths=LENS)
    z = ops.randn_batch(B, S, T, SEEDS, LENS, stream_id=0)
    b = ops.warm_start(sde, est, raw, mixn, mean, std, t, noise=z, lengths=LENS)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    # one seed on a mixed-length batch: the seeds the sampler derives from it
    a1 = ops.warm_start(sde, est, raw, mixn, mean, std, t, seed=77, lengths=LENS)
    z1 = ops.randn_batch(B, S, T, ops.batch_seeds(77, B), LENS, stream_id=0)
    assert torch.equal(a1[0], ops.warm_start(sde, est, raw, mixn, mean, std, t, noise=z1, lengths=LENS)[0])
    # one seed, no lengths: draw 0 of diffsep_randn over the whole [B,S,T] (the fused sampler's prior draw)
    full = est.clone()
    full[full == 9.0] = 0.0
    a2 = ops.warm_start(sde, full, raw, mixn, mean, std, t, seed=5)
    z2 = ops.randn(B * S * T, 5, 0).view(B, S, T)
    assert torch.equal(a2[0], ops.warm_start(sde, full, raw, mixn, mean, std, t, noise=z2)[0])
    # every row is its own B = 1 call at its own width, also on a second stream
    side = torch.cuda.Stream()
    for r, L in enumerate(LENS):
        args = (est[r:r + 1, :, :L].contiguous(), raw[r:r + 1, :, :L].contiguous(), mixn[r:r + 1, :, :L].contiguous(),
                mean[r:r + 1], std[r:r + 1], t[r:r + 1])
        one = ops.warm_start(sde, *args, seed=SEEDS[r])
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            two = ops.warm_start(sde, *args, seeds=[SEEDS[r]])
        side.synchronize()
        for got in (one, two):
            assert torch.equal(got[0][0], a[0][r, :, :L]) and torch.equal(got[1][0], a[1][r]) and int(got[2][0]) == int(a[2][r]), r
        assert float(a[0][r, :, L:].abs().max() if L < T else 0.0) == 0.0


# ---------------------------------------------------------------- 3. gains
def fit_batch():
    """the estimates e0 = 0.37 t0 + 0.05 t1, e1 = -1.9 t1 of the synthetic sources of utterance b over LENS[b] samples, padded"""
    T = max(LENS)
    est, raw = np.full((len(LENS), S, T), 7.0, np.float32), np.zeros((len(LENS), 1, T), np.float32)
    for b, L in enumerate(LENS):
        mix, tgt = synth.synth_mixture(b, T=L)
        est[b, :, :L] = np.stack([0.37 * tgt[0] + 0.05 * tgt[1], -1.9 * tgt[1]]).astype(np.float32)
        raw[b, :, :L] = mix
    return est, raw


def test_gains_against_float64_reference():
    est, raw = fit_batch()
    mixn, _ = padded()
    B = len(LENS)
    mean, std, t = torch.zeros(B, device="cuda"), torch.ones(B, device="cuda"), torch.full((B,), 0.5, device="cuda")
    x, gains, fb = ops.warm_start(MIX, dev(est), dev(raw), mixn, mean, std, t, seeds=SEEDS, lengths=LENS)
    assert fb.tolist() == [0, 0, 0]
    g = gains.cpu().numpy()
    for b, L in enumerate(LENS):
        want, fbr, cond = W.fit(est[b], raw[b], L)
        assert cond <= 100, cond
        # |dg|_inf <= 2 ||g||_2 cond(G) 2^-53 (n (S + sqrt S) + 8 S^2): n-term float64 sums of exact products through the normal
        # equations, doubled for the reference's own error (tests/warm_start_ref.py, gain_bound) — from n and cond alone
        bound = W.gain_bound(want, cond, L)
        same = W.fit(est[b], raw[b], L, sums=W.sums_device_order)[0]
        print(f"row {b}: n = {L}, cond(G) = {cond:.2f}, gains {g[b]}, |d| = {np.abs(g[b] - want).max():.3e}, bound {bound:.3e}, "
              f"bit-equal to the restated summation order: {np.array_equal(same, g[b])}")
        assert fbr == 0 and np.abs(g[b] - want).max() <= bound
        assert np.abs(g[b] - np.array([1.0 / 0.37, 0.05 / (0.37 * 1.9) - 1.0 / 1.9])).max() <= 1e-5
    # scale none: gains exactly 1
    x1, g1, f1 = ops.warm_start(MIX, dev(est), dev(raw), mixn, mean, std, t, seeds=SEEDS, lengths=LENS, scale="none")
    assert bool((g1 == 1.0).all()) and f1.tolist() == [0, 0, 0] and not torch.equal(x1, x)
    # a silent estimate / two identical estimates in row 1: gains 1 and the flag on that row only, the others bit for bit
    for how in ("silent", "identical"):
        bad = est.copy()
        if how == "silent":
            bad[1, 1, :LENS[1]] = 0.0
        else:
            bad[1, 1] = bad[1, 0]
        xb, gb, fbb = ops.warm_start(MIX, dev(bad), dev(raw), mixn, mean, std, t, seeds=SEEDS, lengths=LENS)
        assert fbb.tolist() == [0, 1, 0] and bool((gb[1] == 1.0).all()), how
        assert torch.equal(gb[[0, 2]], gains[[0, 2]]) and torch.equal(xb[[0, 2]], x[[0, 2]]), how
        assert torch.equal(xb[1], ops.warm_start(MIX, dev(bad), dev(raw), mixn, mean, std, t, seeds=SEEDS, lengths=LENS,
                                                 scale="none")[0][1])


# ---------------------------------------------------------------- 4. resume, bit for bit
def resume(eng, kw, ks, N):
    mixn, _ = padded()
    full, nfe = eng.pc_sample(mixn, MIX, **kw)
    assert torch.isfinite(full).all()
    for k in ks:
        a, nfe_a = eng.pc_sample(mixn, MIX, **kw, last_step=k)
        b, nfe_b = eng.pc_sample(mixn, MIX, **kw, x_init=a, first_step=k)
        assert torch.equal(b, full), (k, float((b - full).abs().max()))
        assert nfe_a + nfe_b == nfe and nfe_a > 0 and nfe_b > 0, (k, nfe_a, nfe_b, nfe)
        assert not torch.equal(a, full)
    return full


@pytest.mark.parametrize("csteps", [1, 2])
def test_resume_is_the_full_run_bit_for_bit(csteps):
    N = 4
    kw = dict(N=N, corrector_steps=csteps, snr=0.5, eps=0.03, lengths=LENS, seeds=SEEDS)
    full = resume(engine(), kw, (1, 2, 3), N)
    # last_step < N hands out the state whatever denoise says; a denoised full run differs from the undenoised one
    assert not torch.equal(full, engine().pc_sample(padded()[0], MIX, **kw, denoise=False)[0])
    # first_step = 0 from the prior of the unit entry on draw 0
    mixn, _ = padded()
    z0 = ops.randn_batch(len(LENS), S, max(LENS), SEEDS, LENS, stream_id=0)
    assert torch.equal(engine().pc_sample(mixn, MIX, **kw, x_init=ops.sde_prior(MIX, mixn, z0), first_step=0)[0], full)


@pytest.mark.parametrize("variant", ["noise", "schedule", "predictor none", "corrector none"])
def test_resume_variants(variant):
    N, c = 4, 1
    kw = dict(N=N, corrector_steps=c, snr=0.5, eps=0.03, lengths=LENS)
    if variant == "noise":
        n_draws = 1 + N * (c + 1)
        kw["noise"] = ops.randn(n_draws * len(LENS) * S * max(LENS), 11, 3).view(n_draws, len(LENS), S, max(LENS))
    else:
        kw["seeds"] = SEEDS
    if variant == "schedule":
        kw["timesteps"] = sdes.sampler_timesteps(N, 0.03, "log")
    if variant == "predictor none":
        kw["predictor"] = "none"
    if variant == "corrector none":
        kw["corrector"] = "none"
    resume(engine(), kw, (1, 2, 3), N)


def test_resume_f16_with_a_head_engine():
    kw = dict(N=4, corrector_steps=1, snr=0.5, eps=0.03, lengths=LENS, seeds=SEEDS, tail=engine(_lib.F32_SPLIT, "f16"), head_steps=1)
    resume(engine(_lib.F16), kw, (1, 2), 4)


# ---------------------------------------------------------------- 5. the generic loop
@pytest.mark.parametrize("sde_name", ["mix", "priormix"])
def test_generic_loop_from_a_state(sde_name):
    m = model16()
    B, T, N, cs, k = 2, 4000, 3, 1, 1
    sde_kw = dict(ndim=2, d_lambda=2.0, sigma_min=0.05, sigma_max=0.5, N=N)
    sde = sdes.MixSDE(**sde_kw) if sde_name == "mix" else sdes.PriorMixSDE(**sde_kw, avg_len=510)
    mix = torch.from_numpy(synth.synth_batch(B, T=T)[0]).cuda()
    (mixn, _), *_ = m.normalize_batch((mix, None))
    n_draws = 1 + N * (cs + 1)
    draws = [torch.from_numpy(synth.synth_noise(f"ws.loop.{sde_name}.z{i}", (B, S, T))).cuda() for i in range(n_draws)]
    kw = dict(N=N, corrector_steps=cs, snr=0.5, eps=0.03, noise=torch.stack(draws))
    eng = m.engine()
    full, _ = eng.pc_sample(mixn, sde.engine_config(), **kw)
    a, _ = eng.pc_sample(mixn, sde.engine_config(), **kw, last_step=k)
    rest = draws[1 + k * (cs + 1):]
    with Injected(rest) as inj:  # (no draw for the prior: the loop starts from x_init)
        x_ref, ns, im = sdes.get_pc_sampler("reverse_diffusion", "ald2", sde, m, mixn, snr=0.5, eps=0.03, corrector_steps=cs,
                                            intermediate=True, x_init=a, first_step=k)()
        assert inj.i == len(rest)
    out, nfe, tr = eng.pc_sample(mixn, sde.engine_config(), **kw, x_init=a, first_step=k, snapshots="all")
    assert nfe == ns == (N - k) * (cs + 1) and tr.steps == [1, 2] and len(im) == N - k
    for i, (xt, xm) in enumerate(im):
        assert torch.equal(tr.x[i], xt) and torch.equal(tr.x_mean[i], xm), i
    assert torch.equal(out, x_ref) and torch.equal(out, full)
    # the reference-shaped factory on the fused path takes the same arguments
    xf, nsf = m.get_pc_sampler("reverse_diffusion", "ald2", mixn, N=N, corrector_steps=cs, snr=0.5, seed=3, x_init=a, first_step=k)()
    assert nsf == (N - k) * (cs + 1) and torch.isfinite(xf).all()
    xs, nss = m.get_pc_sampler("reverse_diffusion", "ald2", mixn, N=N, corrector_steps=cs, snr=0.5, seed=3, last_step=k)()
    assert nss == k * (cs + 1)
    xm_, _ = m.get_pc_sampler("reverse_diffusion", "ald2", mixn, N=N, corrector_steps=cs, snr=0.5, seed=3, x_init=a, first_step=k,
                              minibatch=1)()
    assert xm_.shape == xf.shape and torch.equal(xm_[0], xf[0])  # (minibatch 0 has the seed itself; x_init split along the batch)


# ---------------------------------------------------------------- 6. against the reference's restatement
@pytest.mark.parametrize("sde_name", ["mix", "priormix"])
def test_warm_started_chain_against_the_oracle(sde_name):
    """MEASURED on the MI355X: see DESIGN.md section 5k (the values this test prints)."""
    B, T, N, cs, k = 2, 4000, 3, 1, 1
    ocfg = O.default_config(16, 2)
    sd = synth.synth_state_dict([(n, s) for n, s, _ in param_table(_lib.model_config(nf=16, num_sources=2))], 7)
    p = O.to_torch(sd)
    mix, tgt = synth.synth_batch(B, T=T)
    mix, tgt = torch.from_numpy(mix), torch.from_numpy(tgt)
    est = (0.9 * tgt + 0.1 * tgt.flip(1)).contiguous()  # an imperfect estimate at the right scale
    draws = [torch.from_numpy(synth.synth_noise(f"ws.oracle.{sde_name}.z{i}", (B, S, T))) for i in range(1 + N * (cs + 1))]
    ts = torch.linspace(1.0, 0.03, N, dtype=torch.float32)
    # the oracle's chain: normalise, marginal_prob at ts[k] on draw 0, then the reverse steps k .. N - 1
    y, mean, std = O.normalize_batch(mix)
    x0 = (est - mean) / std
    smix = O.sigma_mix(y, 510) if sde_name == "priormix" else None
    tk = torch.ones(B) * ts[k]
    x = O.sde_mean(ocfg, x0, tk) + O._apply_std(O.mix_std(ocfg, tk, S), draws[0], smix)
    xm = x
    it = iter(draws[1 + k * (cs + 1):])
    for i in range(k, N):
        vt = torch.ones(B) * ts[i]
        for _ in range(cs):
            x, xm = O.corrector_ald2(ocfg, x, vt, O.score_forward(p, ocfg, x, vt, y), next(it), 0.5, smix)
        x, xm = O.predictor_reverse_diffusion(ocfg, x, vt, O.score_forward(p, ocfg, x, vt, y), next(it), N, smix)
    ref = xm
    # the device: warm_start (mean_from estimate = marginal_prob, gains 1) -> the fused sampler from step k
    sde = PMIX if sde_name == "priormix" else MIX
    mix_d = mix.cuda()
    yn, mu, sg = ops.normalize_batch(mix_d)
    tkd = torch.full((B,), float(ts[k]), device="cuda")
    x_init, _, _ = ops.warm_start(sde, est.cuda(), mix_d, yn, mu, sg, tkd, scale="none", mean_from="estimate", noise=draws[0].cuda())
    out, nfe = engine().pc_sample(yn, sde, N=N, corrector_steps=cs, snr=0.5, eps=0.03, noise=torch.stack(draws).cuda(),
                                  x_init=x_init, first_step=k)
    d = float((out.double().cpu() - ref.double()).pow(2).mean().sqrt())
    r = d / (float(ref.double().pow(2).mean().sqrt()) + 1e-30)
    print(f"{sde_name}: warm-started chain from step {k} of {N} against the oracle: diff_rms {d:.3e}, rel_rms {r:.3e}")
    assert nfe == (N - k) * (cs + 1)
    assert d < 1e-3 and r < 1e-4  # the gate of the fused sampler against the reference golden (tests/test_engine_gpu.py)


# ---------------------------------------------------------------- 7. trace with a range
def test_trace_with_a_range():
    mixn, tgt = padded()
    eng = engine()
    kw = dict(N=3, corrector_steps=1, snr=0.5, eps=0.03, lengths=LENS, seeds=SEEDS)
    out, _, full = eng.pc_sample(mixn, MIX, **kw, snapshots="all", target=tgt)
    a, _, head = eng.pc_sample(mixn, MIX, **kw, last_step=1, snapshots="all", target=tgt)
    assert head.steps == [0] and torch.equal(head.x[0], full.x[0]) and torch.equal(head.x_mean[0], full.x_mean[0])
    assert torch.equal(head.gram[0], full.gram[0]) and bool(torch.isnan(head.gram[1:]).all())
    b, nfe, rest = eng.pc_sample(mixn, MIX, **kw, x_init=a, first_step=1, snapshots=[1, 2], target=tgt)
    assert nfe == 4 and torch.equal(b, out) and rest.steps == [1, 2]
    assert torch.equal(rest.x, full.x[1:]) and torch.equal(rest.x_mean, full.x_mean[1:])
    assert torch.equal(rest.gram[1:], full.gram[1:]) and bool(torch.isnan(rest.gram[0]).all())
    for bad in ([0], [0, 1], [3]):
        with pytest.raises(_lib.DiffsepError, match="snapshot steps"):
            eng.pc_sample(mixn, MIX, **kw, x_init=a, first_step=1, snapshots=bad)
    with pytest.raises(_lib.DiffsepError, match="snapshot steps"):
        eng.pc_sample(mixn, MIX, **kw, last_step=2, snapshots=[2])


# ---------------------------------------------------------------- 8. refusals
def raw_from(eng, mixn, out, x_init, first, last, steps=(), snap=None, N=3):
    """diffsep_pc_sample_from with exactly these arguments"""
    B, _, T = mixn.shape
    sc = _lib.sde_config(MIX)
    sm = _lib.SamplerConfig(N, 1, 0.5, 0.03, 1, _lib.PRED_REVERSE_DIFFUSION, _lib.CORR_ALD2)
    arr = np.ascontiguousarray(list(steps), dtype=np.int32)
    _lib.call(eng._L, "diffsep_pc_sample_from", eng._h, C.byref(sc), C.byref(sm), None, _lib._ptr(mixn), _lib._ptr(out), B, T,
              None, 5, None, None, len(steps), arr.ctypes.data_as(C.POINTER(C.c_int32)), _lib._ptr(snap), None, None, None,
              _lib._ptr(x_init), first, last, _lib._stream_ptr())


def test_refusals_leave_out_untouched():
    mixn, _ = padded()
    eng, B, T, N = engine(), 3, 7000, 3
    SENT = 7.5
    out = torch.full((B, S, T), SENT, device="cuda")
    snap = torch.full((1, B, S, T), SENT, device="cuda")
    x0 = torch.zeros((B, S, T), device="cuda")
    cases = [(None, 1, 0, (), None), (x0, -1, 0, (), None), (x0, 2, 2, (), None), (x0, 2, 1, (), None), (x0, 0, N + 1, (), None),
             (x0, N, 0, (), None), (x0, 1, 0, (0,), snap), (x0, 0, 2, (2,), snap)]
    for xi, first, last, steps, sn in cases:
        with pytest.raises(_lib.DiffsepError, match="pc_sample"):
            raw_from(eng, mixn, out, xi, first, last, steps, sn)
        torch.cuda.synchronize()
        assert bool((out == SENT).all()) and bool((snap == SENT).all()), (first, last, steps)
    raw_from(eng, mixn, out, x0, 1, 0, (1,), snap)  # (the same pointers are fine when the request is)
    assert torch.isfinite(out).all() and not bool((out == SENT).any()) and not bool((snap == SENT).any())
    # Engine.pc_sample and the factory refuse the same requests
    for bad in (dict(first_step=1), dict(x_init=x0, first_step=3), dict(last_step=0), dict(last_step=4)):
        with pytest.raises(_lib.DiffsepError, match="pc_sample"):
            eng.pc_sample(mixn, MIX, N=3, **bad)
    # warm_start: refusals name the argument and write nothing
    est, raw, _, mean, std, t = noise_inputs()
    with pytest.raises(_lib.DiffsepError, match="sigma_mix"):
        _lib.call(_lib.lib(), "diffsep_warm_start", C.byref(_lib.sde_config(PMIX)), _lib._ptr(est), _lib._ptr(raw), _lib._ptr(mixn),
                  _lib._ptr(mean), _lib._ptr(std), _lib._ptr(t), None, None, None, None, 0, 0, 0, _lib._ptr(out), _lib._ptr(x0),
                  _lib._ptr(x0), B, S, T, None, 0, _lib._stream_ptr())
    with pytest.raises(_lib.DiffsepError, match="workspace"):
        _lib.call(_lib.lib(), "diffsep_warm_start", C.byref(_lib.sde_config(MIX)), _lib._ptr(est), _lib._ptr(raw), _lib._ptr(mixn),
                  _lib._ptr(mean), _lib._ptr(std), _lib._ptr(t), None, None, None, None, 0, 1, 0, _lib._ptr(out), _lib._ptr(x0),
                  _lib._ptr(x0), B, S, T, None, 0, _lib._stream_ptr())


# ---------------------------------------------------------------- 9. refine and the CLI
def test_refine_and_the_cli(tmp_path, capsys):
    ind, first_out, second_out = tmp_path / "in", tmp_path / "first", tmp_path / "second"
    ind.mkdir()
    lens = [6400, 6017]
    for i, L in enumerate(lens):
        wavio.save(ind / f"u{i}.wav", torch.from_numpy(synth.synth_mixture(i, T=L)[0]), 8000, bits=32)
    common = ["--synthetic-weights", "16", "-N", "4", "--dtype", "f32", "--seed", "3"]
    sep_cli.main([str(ind), str(first_out)] + common)
    capsys.readouterr()
    sep_cli.main([str(ind), str(second_out)] + common + ["--init-dir", str(first_out), "--t-start", "0.5", "--batch", "2"])
    line = [l for l in capsys.readouterr().out.splitlines() if l.startswith("refined")]
    assert len(line) == 1
    N = 4
    first = sdes.first_step_for(0.5, sdes.sampler_timesteps(N, 0.03))
    assert first == 2 and f"steps [{first}, {N}) of {N}" in line[0] and f"NFE {(N - first) * 2} per file" in line[0]
    assert "fell back" not in line[0]
    # the same request through DiffSepModel.refine, file by file, on the same tensors and seeds
    m = DiffSepModel(default_config(nf=16), dtype="f32", device="cuda:0")
    m.to("cuda:0")
    from diffsep_amd import inflight
    seeds = inflight.utterance_seeds(len(lens), 3)
    for i, L in enumerate(lens):
        mix = wavio.load(ind / f"u{i}.wav")[0][:1].cuda()[None]
        est = torch.stack([wavio.load(first_out / f"s{k}" / f"u{i}.wav")[0][0] for k in range(S)])[None].cuda()
        got = torch.stack([wavio.load(second_out / f"s{k}" / f"u{i}.wav")[0][0] for k in range(S)])
        assert got.shape == (S, L) and torch.isfinite(got).all()
        assert not torch.equal(got, est[0].cpu())
        sep, info = m.refine(mix, est, t_start=0.5, seeds=[seeds[i]], N=N, corrector_steps=1, snr=0.5)
        assert info["first_step"] == first and info["nfe"] == (N - first) * 2 and info["fallback"].tolist() == [0]
        assert info["t"] == float(sdes.sampler_timesteps(N, 0.03)[first])
        assert torch.equal(sep[0].cpu(), got), i
