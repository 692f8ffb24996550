"""The fixed-step probability-flow ODE sampler on the MI355X (diffsep_ode_sample_fixed, Engine.ode_sample_fixed,
sdes.get_ode_fixed_sampler, the two CLIs): the device solve against a float64 host loop over the same drift bit for bit, the
denoise step, independent rows of a zero-padded batch, grids and start times, the hybrid-precision head, the local-error
trace, convergence towards the adaptive solve, the CPU oracle end to end, that the call does not block, and the CLIs.

Measured on the MI355X (synthetic weights, nf = 16, T = 4000; printed by the tests):
  against the adaptive solve (RK45 at 1e-5, 1418 evaluations), rel RMS of Heun at M = 32 / 64 / 128: 0.0762 / 0.0371 / 0.0202;
  against the CPU oracle, Heun M = 8 with denoise: rel RMS 6.6e-6 (MixSDE), 1.0e-5 (PriorMixSDE); gate 1e-3;
  largest local error of Heun: 1.08 at M = 8, 0.45 at M = 16."""
import json

import numpy as np
import pytest
import torch

import diffsep_oracle as O
from diffsep_amd import _lib, ops, sdes, synth, wavio
from diffsep_amd import evaluate as eval_cli
from diffsep_amd import separate as sep_cli
from diffsep_amd.engine import Engine, pack_state_dict, param_table

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

NF, S, T = 16, 2, 4000
EPS = 0.03
MIX = dict(kind=_lib.SDE_MIX, ndim=2, d_lambda=2.0, sigma_min=0.05, sigma_max=0.5)
PRIOR = dict(kind=_lib.SDE_PRIORMIX, ndim=2, d_lambda=2.0, sigma_min=0.05, sigma_max=0.5, avg_len=510)
SDES = {"mix": MIX, "priormix": PRIOR}
# (C, rows of A, B) of the one-step methods, written from their definitions
TABLEAU = {"euler": ([0.0], [[]], [1.0]),
           "heun": ([0.0, 1.0], [[], [1.0]], [0.5, 0.5]),
           "midpoint": ([0.0, 0.5], [[], [0.5]], [0.0, 1.0]),
           "rk4": ([0.0, 0.5, 0.5, 1.0], [[], [0.5], [0.0, 0.5], [0.0, 0.0, 1.0]], [1.0 / 6, 1.0 / 3, 1.0 / 3, 1.0 / 6])}
_cache = {}


def rel_rms(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(np.mean((a - b) ** 2)) / (np.sqrt(np.mean(b ** 2)) + 1e-30))


def weights(spec_factor=0.33):
    cfg = _lib.model_config(nf=NF, num_sources=S, spec_factor=spec_factor)
    return synth.synth_state_dict([(n, s) for n, s, _ in param_table(cfg)], 7)


def engine(spec_factor=0.33, dtype=_lib.F32, lib_kind=None):
    key = (spec_factor, dtype, lib_kind)
    if key not in _cache:
        cfg = _lib.model_config(nf=NF, num_sources=S, spec_factor=spec_factor, dtype=dtype)
        _cache[key] = Engine(cfg, pack_state_dict(cfg, weights(spec_factor)), lib_kind=lib_kind)
    return _cache[key]


def inputs(B, sde, tag="a"):
    mix = torch.from_numpy(synth.synth_batch(B, T=T)[0]).cuda()
    mix_norm, _, _ = ops.normalize_batch(mix)
    z = torch.from_numpy(synth.synth_noise(f"odef.{tag}", (B, S, T))).cuda()
    smix = ops.sde_sigma_mix(mix_norm, sde["avg_len"]) if sde["kind"] == _lib.SDE_PRIORMIX else None
    return mix_norm, ops.sde_prior(sde, mix_norm, z, smix), smix


def uniform_grid(M, t0=1.0, eps=EPS):
    """the entry's own grid: t_i = t0 + (eps - t0) i / M for i < M, t_M = eps"""
    return np.array([t0 + (eps - t0) * i / M for i in range(M)] + [eps])


def host_solve(eng, sde, mix_norm, x_T, smix, method, ts):
    """The solve in numpy float64 around the engine's own drift (eng.score + ops.sde_coefficients + ops.sde_reverse_drift):
    every stage input is fp32(y + (sum_j a_j K_j) h), the terms summed in the order the pass sums them (j = 0, 1, ...; the
    pass-level test of tests/test_ode_gpu.py shows it).  -> (last state float64, evaluations, per step (h, y_i, [K used]))"""
    B = x_T.shape[0]
    evals = [0]

    def drift(t, x32):
        x = torch.from_numpy(x32).cuda()
        tt = torch.full((B,), float(np.float32(t)), device="cuda")
        f, G = ops.sde_coefficients(sde, x, tt, smix)
        evals[0] += 1
        return ops.sde_reverse_drift(f, G, eng.score(x, tt, mix_norm), probability_flow=True).cpu().numpy().astype(np.float64)

    def comb(c, K):
        acc = np.zeros_like(K[0])
        for cj, kj in zip(c, K):
            acc = acc + cj * kj
        return acc

    y = x_T.cpu().numpy().astype(np.float64)
    steps, k_prev, h_prev = [], None, None
    for i in range(len(ts) - 1):
        t, h = ts[i], ts[i + 1] - ts[i]
        if method == "ab2" and i > 0:
            w = h / h_prev
            K = [k_prev, drift(t, y.astype(np.float32))]
            new = y + h * comb([-(w / 2), 1.0 + w / 2], K)
            k_prev = K[1]
        else:
            C, A, Bc = TABLEAU["heun" if method == "ab2" else method]
            K = [drift(t, y.astype(np.float32))]
            for s in range(1, len(C)):
                K.append(drift(t + C[s] * h, (y + comb(A[s], K) * h).astype(np.float32)))
            new = y + h * comb(Bc, K)
            k_prev = K[0]
        steps.append((h, y, K))
        y, h_prev = new, h
    return y, evals[0], steps


def host_case(kind, method, M):
    """one solve of test 1, computed once: (engine inputs, the host loop's result)"""
    key = ("host", kind, method, M)
    if key not in _cache:
        sde = SDES[kind]
        mix_norm, x_T, smix = inputs(2, sde, "loop")
        _cache[key] = (mix_norm, x_T, smix, host_solve(engine(), sde, mix_norm, x_T, smix, method, uniform_grid(M)))
    return _cache[key]


# ---------------------------------------------------------------- 1. same drift, two integrators, bit for bit
@pytest.mark.parametrize("kind", ["mix", "priormix"])
@pytest.mark.parametrize("method, M", [("euler", 4), ("heun", 3), ("rk4", 2), ("ab2", 4)])
def test_device_solve_is_the_host_loop_bit_for_bit(method, M, kind):
    mix_norm, x_T, smix, (y, n, _) = host_case(kind, method, M)
    out, info = engine().ode_sample_fixed(mix_norm, SDES[kind], method=method, steps=M, eps=EPS, denoise=False, x_init=x_T)
    assert info["nfe"] == n == _lib.odef_nfe(method, M) and info["method"] == method and info["steps"] == M
    assert np.array_equal(out.cpu().numpy(), y.astype(np.float32))
    again, _ = engine().ode_sample_fixed(mix_norm, SDES[kind], method=method, steps=M, eps=EPS, denoise=False, x_init=x_T)
    assert torch.equal(out, again)


def test_midpoint_matches_the_host_loop_too():
    mix_norm, x_T, smix, (y, n, _) = host_case("mix", "midpoint", 2)
    out, info = engine().ode_sample_fixed(mix_norm, MIX, method="midpoint", steps=2, eps=EPS, denoise=False, x_init=x_T)
    assert info["nfe"] == n == 4 and np.array_equal(out.cpu().numpy(), y.astype(np.float32))


# ---------------------------------------------------------------- 2. denoise
def test_denoise_is_one_predictor_step_at_eps():
    eng = engine()
    mix_norm, x_T, _ = inputs(2, MIX, "denoise")
    raw, i0 = eng.ode_sample_fixed(mix_norm, MIX, steps=3, eps=EPS, denoise=False, x_init=x_T, N=30)
    den, i1 = eng.ode_sample_fixed(mix_norm, MIX, steps=3, eps=EPS, denoise=True, x_init=x_T, N=30)
    assert i0 == i1 and i0["nfe"] == 6
    te = torch.full((2,), np.float32(EPS), device="cuda")
    _, xm = ops.sde_predictor_update(MIX, 30, raw, te, eng.score(raw, te, mix_norm), None)
    assert torch.equal(xm, den)


# ---------------------------------------------------------------- 3. rows of a zero-padded batch
def test_rows_equal_their_solo_calls_bit_for_bit():
    eng = engine()
    lens, seeds = [4000, 3900], [5, 9]
    utts = [ops.normalize_batch(torch.from_numpy(synth.synth_mixture(u, T=L)[0])[None].cuda())[0].contiguous()
            for u, L in enumerate(lens)]
    solo = [eng.ode_sample_fixed(utts[u], MIX, method="heun", steps=3, eps=EPS, seed=seeds[u])[0] for u in range(2)]
    for order in ([0, 1], [1, 0]):
        mixn = torch.zeros(2, 1, T, device="cuda")
        for b, u in enumerate(order):
            mixn[b, :, :lens[u]] = utts[u][0]
        out, info = eng.ode_sample_fixed(mixn, MIX, method="heun", steps=3, eps=EPS, lengths=[lens[u] for u in order],
                                         seeds=[seeds[u] for u in order])
        assert info["nfe"] == 6
        for b, u in enumerate(order):
            assert torch.equal(out[b, :, :lens[u]], solo[u][0]), (order, b)
            assert lens[u] == T or float(out[b, :, lens[u]:].abs().max()) == 0.0
    # without seeds row b draws under seed + b * 0x9E3779B97F4A7C15, as the PC sampler keys a batch with lengths
    out, _ = eng.ode_sample_fixed(mixn, MIX, method="heun", steps=3, eps=EPS, lengths=[3900, 4000], seed=9)
    assert torch.equal(out[0, :, :3900], solo[1][0])


# ---------------------------------------------------------------- 4. grid and start
class _Model:
    """the least a score function needs for the factories: an engine"""

    def engine(self):
        return engine()


def test_timesteps_equal_the_schedule_and_a_late_start_runs_from_t_start():
    eng = engine()
    sde = sdes.MixSDE(ndim=2, d_lambda=2.0, sigma_min=0.05, sigma_max=0.5, N=30)
    mix_norm, x_T, _ = inputs(2, MIX, "grid")
    a, nfe = sdes.get_ode_fixed_sampler(sde, _Model(), mix_norm, method="heun", steps=4, schedule="log", eps=EPS, seed=3)()
    ts = sdes.ode_fixed_timesteps(4, EPS, "log", 1.0)
    b, info = eng.ode_sample_fixed(mix_norm, sde.engine_config(), method="heun", steps=4, eps=EPS, timesteps=ts, N=30, seed=3)
    c, _ = eng.ode_sample_fixed(mix_norm, sde.engine_config(), method="heun", steps=4, eps=EPS, N=30, seed=3)
    assert nfe == info["nfe"] == 8 and torch.equal(a, b) and not torch.equal(a, c)
    # a start at t = 0.5 from a warm start: 4 steps over [0.5, eps]
    mix = torch.from_numpy(synth.synth_batch(2, T=T)[0]).cuda()
    est = torch.from_numpy(synth.synth_batch(2, T=T)[1]).cuda()
    mixn, mean, std = ops.normalize_batch(mix)
    t = torch.full((2,), 0.5, device="cuda")
    x_init, _, _ = ops.warm_start(MIX, est, mix, mixn, mean.reshape(2), std.reshape(2), t, seed=4)
    out, info = eng.ode_sample_fixed(mixn, MIX, method="heun", steps=4, t_start=0.5, eps=EPS, denoise=False, x_init=x_init)
    y, n, _ = host_solve(eng, MIX, mixn, x_init, None, "heun", uniform_grid(4, t0=0.5))
    assert info["nfe"] == n == 8 and np.array_equal(out.cpu().numpy(), y.astype(np.float32))
    via, nfe = sdes.get_ode_fixed_sampler(sde, _Model(), mixn, steps=4, t_start=0.5, eps=EPS, denoise=False, x_init=x_init)()
    assert nfe == 8 and torch.equal(via, out)
    with pytest.raises(_lib.DiffsepError, match="starts below 1 needs the state to start from"):
        eng.ode_sample_fixed(mixn, MIX, steps=4, t_start=0.5, eps=EPS)
    with pytest.raises(_lib.DiffsepError, match="x_init and noise are alternatives"):
        eng.ode_sample_fixed(mixn, MIX, steps=4, eps=EPS, x_init=x_init, noise=x_init)
    with pytest.raises(_lib.DiffsepError, match="err_out needs a method with an embedded Euler step"):
        eng.ode_sample_fixed(mixn, MIX, method="rk4", steps=4, eps=EPS, want_err=True)
    with pytest.raises(_lib.DiffsepError, match="steps \\+ 1 = 5 times"):
        eng.ode_sample_fixed(mixn, MIX, steps=4, eps=EPS, timesteps=[1.0, 0.5, 0.03])
    with pytest.raises(_lib.DiffsepError, match="padded frame count"):
        eng.ode_sample_fixed(torch.zeros(2, 1, 9000, device="cuda"), MIX, steps=2, lengths=[9000, 3000])


# ---------------------------------------------------------------- 5. hybrid precision
def test_head_steps_run_on_the_other_engine_and_none_leaves_it_alone():
    # (read of the code: the prior is not drawn here — x_init; mixture copy, cast, the passes and the rounding are fp32 / fp64
    # kernels of sde.hip / ode.hip that do not depend on the engine's precision; only run_nfe does)
    M = 3
    half = engine(dtype=_lib.F16)
    full = engine(lib_kind="f16")  # an fp32 engine of the half-precision build: what an F16 engine can name as its tail
    mix_norm, x_T, _ = inputs(2, MIX, "hybrid")
    want, _ = full.ode_sample_fixed(mix_norm, MIX, method="heun", steps=M, eps=EPS, denoise=False, x_init=x_T)
    got, info = half.ode_sample_fixed(mix_norm, MIX, method="heun", steps=M, eps=EPS, denoise=False, x_init=x_T, tail=full,
                                      head_steps=M)
    own, _ = half.ode_sample_fixed(mix_norm, MIX, method="heun", steps=M, eps=EPS, denoise=False, x_init=x_T)
    assert info["nfe"] == 2 * M and torch.equal(got, want) and not torch.equal(own, want)
    # tail_steps: the last step on the other engine differs from both
    mixed, _ = half.ode_sample_fixed(mix_norm, MIX, method="heun", steps=M, eps=EPS, denoise=False, x_init=x_T, tail=full,
                                     tail_steps=1)
    assert not torch.equal(mixed, own) and not torch.equal(mixed, want)
    # no such step: a sentinel in the other engine's sampler state (the arena below the forward region) stays as it is
    torch.cuda.synchronize()
    arena, fwd = full.debug_arena()
    arena[:fwd].fill_(0x5A)
    before = arena.clone()
    none, _ = half.ode_sample_fixed(mix_norm, MIX, method="heun", steps=M, eps=EPS, denoise=False, x_init=x_T, tail=full,
                                    head_steps=0, tail_steps=0)
    torch.cuda.synchronize()
    assert torch.equal(none, own) and torch.equal(full.debug_arena()[0], before)
    _cache.pop((0.33, _lib.F32, "f16"))  # (its sampler state holds the sentinel now)


# ---------------------------------------------------------------- 6. the local-error trace
def test_error_trace_is_the_embedded_euler_difference():
    eng = engine()
    M = 3
    mix_norm, x_T, smix, (y, n, steps) = host_case("mix", "heun", M)
    plain, _ = eng.ode_sample_fixed(mix_norm, MIX, method="heun", steps=M, eps=EPS, denoise=False, x_init=x_T)
    out, info = eng.ode_sample_fixed(mix_norm, MIX, method="heun", steps=M, eps=EPS, denoise=False, x_init=x_T, want_err=True)
    err = info["err"].cpu().numpy()
    assert err.shape == (M, 2, 2) and torch.equal(out, plain)
    for i, (h, y_i, K) in enumerate(steps):
        for b in range(2):
            d = np.sqrt(np.mean((h * (K[1][b] - K[0][b]) / 2) ** 2))
            r = np.sqrt(np.mean(y_i[b] ** 2))
            assert abs(err[i, b, 0] - d) <= 1e-12 * d and abs(err[i, b, 1] - r) <= 1e-12 * r, (i, b)
    worst = []
    for m in (8, 16):
        _, info = eng.ode_sample_fixed(mix_norm, MIX, method="heun", steps=m, eps=EPS, denoise=False, x_init=x_T, want_err=True)
        worst.append(float(info["err"][:, :, 0].max()))
    print(f"largest local error of Heun: {worst[0]:.4g} at M = 8, {worst[1]:.4g} at M = 16")
    assert worst[1] < worst[0]
    for method in ("midpoint", "ab2"):  # the other two traces: finite, positive, the result untouched
        a, _ = eng.ode_sample_fixed(mix_norm, MIX, method=method, steps=4, eps=EPS, denoise=False, x_init=x_T)
        b, info = eng.ode_sample_fixed(mix_norm, MIX, method=method, steps=4, eps=EPS, denoise=False, x_init=x_T, want_err=True)
        assert torch.equal(a, b) and bool((info["err"] > 0).all()) and bool(torch.isfinite(info["err"]).all())


# ---------------------------------------------------------------- 7. against the adaptive solve
def test_heun_approaches_the_adaptive_solve():
    eng = engine()
    mix_norm, x_T, _ = inputs(2, MIX, "adaptive")
    ref, info = eng.ode_sample(mix_norm, MIX, rtol=1e-5, atol=1e-5, eps=EPS, denoise=False, x_init=x_T)
    assert info["status"] == 0
    d = {}
    for M in (32, 64, 128):
        out, _ = eng.ode_sample_fixed(mix_norm, MIX, method="heun", steps=M, eps=EPS, denoise=False, x_init=x_T)
        d[M] = rel_rms(out.cpu(), ref.cpu())
    print(f"Heun against RK45 at 1e-5 ({info['nfev']} evaluations): rel RMS {d[32]:.4g} (M = 32), {d[64]:.4g} (64), {d[128]:.4g} (128)")
    assert d[128] < d[64] < d[32]


# ---------------------------------------------------------------- 8. oracle gate
@pytest.mark.parametrize("kind, spec_factor", [("mix", 0.33), ("priormix", 0.15)], ids=["mix", "priormix-enhancement"])
def test_engine_matches_cpu_oracle_end_to_end(kind, spec_factor):
    sde = SDES[kind]
    eng = engine(spec_factor)
    B, N, M = 1, 30, 8
    mix_norm, x_T, _ = inputs(B, sde, "oracle")
    ocfg = O.default_config(NF, S, spec_factor=spec_factor)
    p = O.to_torch(weights(spec_factor))
    mix_c = mix_norm.cpu()
    sm = O.sigma_mix(mix_c, sde["avg_len"]) if kind == "priormix" else None

    def drift(t, y):
        x = torch.from_numpy(y.astype(np.float32))
        tt = torch.ones(B) * float(np.float32(t))
        score = O.score_forward(p, ocfg, x, tt, mix_c)
        f, G = O.sde_coefficients(ocfg, x, tt, None if sm is None else sm[:, 0])
        G = G if G.dim() == 3 else G[:, None, None]
        return (f - 0.5 * G ** 2 * score).double().numpy()

    ts = uniform_grid(M)
    y = x_T.cpu().double().numpy()
    for i in range(M):  # Heun's method, float64 state
        h = ts[i + 1] - ts[i]
        k1 = drift(ts[i], y)
        k2 = drift(ts[i] + h, y + h * k1)
        y = y + h * (0.5 * k1 + 0.5 * k2)
    x = torch.from_numpy(y.astype(np.float32))
    te = torch.ones(B) * EPS
    _, ref = O.predictor_reverse_diffusion(ocfg, x, te, O.score_forward(p, ocfg, x, te, mix_c), torch.zeros_like(x), N, smix=sm)
    out, info = eng.ode_sample_fixed(mix_norm, sde, method="heun", steps=M, eps=EPS, N=N, x_init=x_T)
    err = rel_rms(out.cpu(), ref)
    print(f"{kind}: Heun M = {M} with denoise against the CPU oracle: rel rms {err:.3e}")
    assert info["nfe"] == 2 * M and err <= 1e-3


# ---------------------------------------------------------------- 9. the call does not block
def test_call_returns_before_the_solve_has_run():
    eng = engine()
    mix_norm, x_T, _ = inputs(2, MIX, "async")
    kw = dict(method="rk4", steps=64, eps=EPS, x_init=x_T)
    want, _ = eng.ode_sample_fixed(mix_norm, MIX, **kw)  # (also: plan, graph and buffers exist before the timed call)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        out, info = eng.ode_sample_fixed(mix_norm, MIX, **kw)
        running = not side.query()
    side.synchronize()
    assert info["nfe"] == 256 and running, "the 256 evaluations had drained when the call returned"
    assert torch.equal(out, want)


# ---------------------------------------------------------------- 10. the model's methods, the CLIs
def test_model_separate_and_refine_with_the_fixed_sampler():
    from diffsep_amd.pl_model import DiffSepModel, default_config
    model = DiffSepModel(default_config(nf=16), dtype="f16", device="cuda")  # (a mode with the overflow net around the sampler)
    mix = torch.from_numpy(synth.synth_batch(2, T=T)[0]).cuda()
    a = model.separate(mix, sampler="ode-fixed", method="euler", steps=3, seed=7)
    b = model.separate(mix, sampler="ode-fixed", method="euler", steps=3, seed=7)
    assert tuple(a.shape) == (2, S, T) and bool(torch.isfinite(a).all()) and torch.equal(a, b)
    sampler = model.get_ode_fixed_sampler(ops.normalize_batch(mix)[0], method="ab2", steps=3, seed=7)
    x, nfe = sampler()
    assert nfe == 4 and sampler.info["steps"] == 3 and sampler.info["method"] == "ab2" and bool(torch.isfinite(x).all())
    out, info = model.refine(mix, a, t_start=0.4, sampler="ode-fixed", method="heun", steps=2, seeds=[1, 2])
    assert info["t"] == 0.4 and info["nfe"] == 4 and info["steps"] == 2 and info["method"] == "heun"  # t_start as given: no snapping
    assert tuple(out.shape) == (2, S, T) and bool(torch.isfinite(out).all()) and not torch.equal(out, a)
    with pytest.raises(ValueError, match="t_start = 0.01 must lie in"):
        model.refine(mix, a, t_start=0.01, sampler="ode-fixed")
    with pytest.raises(ValueError, match="sampler must be 'pc' or 'ode-fixed'"):
        model.separate(mix, sampler="ode")


def _same_tree(a, b, names, lens):
    for name, L in zip(names, lens):
        for k in range(2):
            x, sra = wavio.load(a / f"s{k}" / f"{name}.wav")
            y, srb = wavio.load(b / f"s{k}" / f"{name}.wav")
            assert sra == srb == 8000 and x.shape == y.shape == (1, L) and torch.isfinite(x).all()
            assert x.numpy().tobytes() == y.numpy().tobytes(), (name, k)


def test_separate_cli(tmp_path, capsys):
    ind = tmp_path / "in"
    ind.mkdir()
    lens = [4000, 3900, 3800]
    names = [f"utt{i}" for i in range(3)]
    for i, L in enumerate(lens):
        wavio.save(ind / f"utt{i}.wav", torch.from_numpy(synth.synth_mixture(i, T=L)[0]), 8000)
    common = ["--sampler", "ode-fixed", "--ode-method", "heun", "--ode-steps", "4", "--synthetic-weights", "16", "--dtype", "f32",
              "--seed", "11"]
    sep_cli.main([str(ind), str(tmp_path / "b1"), "--batch", "1", "--streams", "1"] + common)
    sep_cli.main([str(ind), str(tmp_path / "b3"), "--batch", "3"] + common)
    sep_cli.main([str(ind), str(tmp_path / "s2"), "--batch", "1", "--streams", "2"] + common)
    _same_tree(tmp_path / "b1", tmp_path / "b3", names, lens)
    _same_tree(tmp_path / "b1", tmp_path / "s2", names, lens)
    capsys.readouterr()
    sep_cli.main([str(ind), str(tmp_path / "ref"), "--batch", "3", "--init-dir", str(tmp_path / "b1"), "--t-start", "0.5"] + common)
    said = capsys.readouterr().out
    assert "4 heun steps of the probability-flow ODE from t = 0.5, NFE 8 per file" in said, said
    for name, L in zip(names, lens):
        x, _ = wavio.load(tmp_path / "ref" / "s0" / f"{name}.wav")
        y, _ = wavio.load(tmp_path / "b1" / "s0" / f"{name}.wav")
        assert x.shape == (1, L) and torch.isfinite(x).all() and not torch.equal(x, y)


def test_evaluate_cli(tmp_path):
    eval_cli.main(["--synthetic", "2", "--samples", "4000", "--synthetic-weights", "16", "--dtype", "f32", "--flat-output",
                   "--streams", "2", "--batch", "1", "--save-n", "0", "--no-stoi", "--sampler", "ode-fixed", "--ode-steps", "4",
                   "--ode-err", "-o", str(tmp_path)])
    rec = json.load(open(tmp_path / "test.json"))
    summ = json.load(open(tmp_path / "test_summary.json"))
    assert [r["batch_idx"] for r in rec] == [0, 1]
    assert all(r["nfe"] == 8 and np.isfinite(r["ode_local_err"]) and r["ode_local_err"] > 0 and np.isfinite(r["si_sdr"]).all()
               for r in rec)
    assert summ["sampler"] == "ode-fixed" and summ["ode_method"] == "heun" and summ["ode_steps"] == 4 and summ["nfe"] == 8
    assert summ["ode_local_err"] == pytest.approx(np.mean([r["ode_local_err"] for r in rec]))
