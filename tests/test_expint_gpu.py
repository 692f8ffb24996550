"""The exponential-integrator samplers on the MI355X (diffsep_ode_sample_expint, diffsep_expint_update_each,
Engine.ode_sample_fixed(method="ddim" / "dpmpp2m") and the layers above): the pass against the numpy float64 restatement of
tests/expint_ref.py bit for bit on both access paths, the device solve against a host loop around the engine's score and the
unit pass bit for bit, the denoise step, independent rows, a late start, the hybrid-precision head, that the call does not
block, the local-error trace, the CPU oracle end to end, and the model and CLI entries.

Measured on the MI355X (synthetic weights, nf = 16, T = 4000; printed by the tests): see DESIGN.md section 5m."""
import json

import numpy as np
import pytest
import torch

import diffsep_oracle as O
import expint_ref as R
from diffsep_amd import _lib, ops, synth
from diffsep_amd import evaluate as eval_cli
from diffsep_amd.engine import Engine, pack_state_dict, param_table

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

NF, S, T = 16, 2, 4000
EPS = 0.03
MIX = dict(kind=_lib.SDE_MIX, ndim=2, d_lambda=2.0, sigma_min=0.05, sigma_max=0.5)
PRIOR = dict(kind=_lib.SDE_PRIORMIX, ndim=2, d_lambda=2.0, sigma_min=0.05, sigma_max=0.5, avg_len=510)
SDES = {"mix": MIX, "priormix": PRIOR}
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
    z = torch.from_numpy(synth.synth_noise(f"expint.{tag}", (B, S, T))).cuda()
    smix = ops.sde_sigma_mix(mix_norm, sde["avg_len"]) if sde["kind"] == _lib.SDE_PRIORMIX else None
    return mix_norm, ops.sde_prior(sde, mix_norm, z, smix), smix


def grid_of(kind, M, t0=1.0):
    return R.uniform_grid(M, t0, EPS) if kind == "uniform" else R.log_grid(M, t0, EPS)


def host_solve(eng, sde, mix_norm, x_T, smix, method, ts, want_norms=False):
    """The solve as a host loop: eng.score at (float) t_i on fp32(y), then the unit pass with the library's table.
    -> (last state float64 tensor, per step (y_i, X0_prev or None, score) as numpy, norms [M,B,2] or None)"""
    B = x_T.shape[0]
    M = len(ts) - 1
    tab = _lib.expint_coefficients(sde, method, M, eps=EPS, timesteps=ts)
    y = x_T.double()
    x = x_T.clone()
    prev, steps, norms = None, [], []
    for i in range(M):
        tt = torch.full((B,), float(np.float32(ts[i])), device="cuda")
        score = eng.score(x, tt, mix_norm)
        use = prev if (method == "dpmpp2m" and i >= 1) else None
        res = ops.expint_update_each(sde, y, score, tab[i], [1] * B, [T] * B, x0_prev=use, sigma_mix=smix, want_norms=want_norms)
        steps.append((y.cpu().numpy(), None if use is None else use.cpu().numpy(), score.cpu().numpy()))
        if want_norms:
            norms.append(res[3].cpu().numpy())
        prev, y, x = res[0], res[1], res[2]
    return y, steps, (np.stack(norms) if want_norms else None), tab


def host_case(kind, method, M, grid):
    key = ("host", kind, method, M, grid)
    if key not in _cache:
        sde = SDES[kind]
        mix_norm, x_T, smix = inputs(2, sde, "loop")
        ts = grid_of(grid, M)
        _cache[key] = (mix_norm, x_T, smix, ts, host_solve(engine(), sde, mix_norm, x_T, smix, method, ts, want_norms=True))
    return _cache[key]


# ---------------------------------------------------------------- 6. the pass against numpy, bit for bit
def unit_data(B, S_, T_, seed):
    g = np.random.default_rng(seed)
    y = g.standard_normal((B, S_, T_))
    score = (3.0 * g.standard_normal((B, S_, T_))).astype(np.float32)
    prev = 0.5 * g.standard_normal((B, S_, T_))
    smix = (0.2 + g.random((B, T_))).astype(np.float32)
    return y, score, prev, smix


@pytest.mark.parametrize("with_prev", [False, True], ids=["first-step", "with-previous-X0"])
@pytest.mark.parametrize("kind", ["mix", "priormix"])
@pytest.mark.parametrize("S_", [2, 3])
@pytest.mark.parametrize("T_", [4000, 3999])
def test_pass_is_the_numpy_restatement_bit_for_bit(T_, S_, kind, with_prev):
    sde = dict(SDES[kind], ndim=S_)
    B = 3
    row = R.table(sde, "dpmpp2m", R.log_grid(5))[2 if with_prev else 0]
    assert (row[R.W1_P] != 0.0) == with_prev
    y, score, prev, smix = unit_data(B, S_, T_, 11 * S_ + T_)
    dev = lambda a: None if a is None else torch.from_numpy(a).cuda()
    length_sets = [[T_, T_ - 97, 1]]
    if T_ % 4:
        length_sets.append([T_ - 3, 8, 4])  # rows of a multiple of 4 samples inside unaligned rows: items of 4, loaded by element
    for lens in length_sets:
        x0, yn, x, norms = ops.expint_update_each(sde, dev(y), dev(score), row, [1] * B, lens, x0_prev=dev(prev) if with_prev else None,
                                                  sigma_mix=dev(smix) if kind == "priormix" else None, want_norms=True)
        x0, yn, x, norms = (v.cpu().numpy() for v in (x0, yn, x, norms))
        for b, L in enumerate(lens):
            w0, wy, wd = R.step(y[b, :, :L], score[b, :, :L], row, prev[b, :, :L] if with_prev else None,
                                smix[b, :L] if kind == "priormix" else None)
            assert np.array_equal(x0[b, :, :L], w0), (lens, b)
            assert np.array_equal(yn[b, :, :L], wy), (lens, b)
            assert np.array_equal(x[b, :, :L], wy.astype(np.float32)), (lens, b)
            for out in (x0, yn, x):  # the tail: exact zeros
                assert not out[b, :, L:].any(), (lens, b)
            rms = lambda v: np.sqrt(np.mean(v * v))
            assert abs(norms[b, 1] - rms(y[b, :, :L])) <= 1e-12 * rms(y[b, :, :L])
            if with_prev:
                assert abs(norms[b, 0] - rms(wd)) <= 1e-12 * rms(wd)
            else:
                assert norms[b, 0] == 0.0
    # an inactive row is left as it is, its neighbours are not
    lens = length_sets[0]
    keep = tuple(torch.full((B, S_, T_), 7.0, dtype=dt, device="cuda") for dt in (torch.float64, torch.float64, torch.float32))
    x0, yn, x = ops.expint_update_each(sde, dev(y), dev(score), row, [1, 0, 1], lens, x0_prev=dev(prev) if with_prev else None,
                                       sigma_mix=dev(smix) if kind == "priormix" else None, out=keep)
    for out in (x0, yn, x):
        assert bool((out[1] == 7.0).all()) and not bool((out[0] == 7.0).any()) and not bool((out[2] == 7.0).any())


def test_pass_refusals():
    y, score, prev, smix = (torch.from_numpy(a).cuda() for a in unit_data(1, 2, 64, 0))
    row = R.table(MIX, "ddim", R.uniform_grid(2))[0]
    with pytest.raises(_lib.DiffsepError, match="PriorMixSDE with sigma_mix, MixSDE without"):
        ops.expint_update_each(MIX, y, score, row, [1], [64], sigma_mix=smix)
    with pytest.raises(_lib.DiffsepError, match="an output aliases an input"):
        ops.expint_update_each(MIX, y, score, row, [1], [64], out=(torch.zeros_like(y), y, torch.zeros_like(score)))
    bad = row.copy()
    bad[R.AL_P] = 0.0
    with pytest.raises(_lib.DiffsepError, match="bad coefficient row"):
        ops.expint_update_each(MIX, y, score, bad, [1], [64])


# ---------------------------------------------------------------- 7. the device solve is the host loop
@pytest.mark.parametrize("kind", ["mix", "priormix"])
@pytest.mark.parametrize("grid", ["uniform", "log"])
@pytest.mark.parametrize("method, M", [("ddim", 4), ("dpmpp2m", 5)])
def test_device_solve_is_the_host_loop_bit_for_bit(method, M, grid, kind):
    mix_norm, x_T, smix, ts, (y, steps, _, tab) = host_case(kind, method, M, grid)
    kw = dict(method=method, steps=M, eps=EPS, x_init=x_T, timesteps=None if grid == "uniform" else ts)
    out, info = engine().ode_sample_fixed(mix_norm, SDES[kind], denoise=False, **kw)
    assert info["nfe"] == M and info["method"] == method and info["steps"] == M
    assert torch.equal(out, y.float())
    again, _ = engine().ode_sample_fixed(mix_norm, SDES[kind], denoise=False, **kw)
    assert torch.equal(out, again)
    # the unit pass inside the loop is the numpy restatement too (first and last step; the pass-level test covers the rest)
    for i in (0, M - 1):
        y_i, prev, score = steps[i]
        want = R.step(y_i, score, tab[i], prev, None if smix is None else smix.cpu().numpy())[1]
        got = steps[i + 1][0] if i + 1 < M else y.cpu().numpy()
        assert np.array_equal(got, want)
    # the denoise step: x_mean of one predictor step at eps on the solve's result
    den, i1 = engine().ode_sample_fixed(mix_norm, SDES[kind], denoise=True, N=30, **kw)
    te = torch.full((2,), np.float32(EPS), device="cuda")
    _, xm = ops.sde_predictor_update(SDES[kind], 30, out, te, engine().score(out, te, mix_norm), None, sigma_mix=smix)
    assert i1["nfe"] == M and torch.equal(xm, den)


# ---------------------------------------------------------------- 8. rows, late start, hybrid precision
def test_rows_equal_their_solo_calls_bit_for_bit():
    eng = engine()
    lens, seeds = [4000, 3900], [5, 9]
    utts = [ops.normalize_batch(torch.from_numpy(synth.synth_mixture(u, T=L)[0])[None].cuda())[0].contiguous()
            for u, L in enumerate(lens)]
    for method in ("ddim", "dpmpp2m"):
        solo = [eng.ode_sample_fixed(utts[u], MIX, method=method, steps=3, eps=EPS, seed=seeds[u])[0] for u in range(2)]
        for order in ([0, 1], [1, 0]):
            mixn = torch.zeros(2, 1, T, device="cuda")
            for b, u in enumerate(order):
                mixn[b, :, :lens[u]] = utts[u][0]
            out, info = eng.ode_sample_fixed(mixn, MIX, method=method, steps=3, eps=EPS, lengths=[lens[u] for u in order],
                                             seeds=[seeds[u] for u in order])
            assert info["nfe"] == 3
            for b, u in enumerate(order):
                assert torch.equal(out[b, :, :lens[u]], solo[u][0]), (method, order, b)
                assert lens[u] == T or float(out[b, :, lens[u]:].abs().max()) == 0.0


def test_a_late_start_runs_from_a_warm_start_state():
    eng = engine()
    mix = torch.from_numpy(synth.synth_batch(2, T=T)[0]).cuda()
    est = torch.from_numpy(synth.synth_batch(2, T=T)[1]).cuda()
    mixn, mean, std = ops.normalize_batch(mix)
    t = torch.full((2,), 0.5, device="cuda")
    x_init, _, _ = ops.warm_start(MIX, est, mix, mixn, mean.reshape(2), std.reshape(2), t, seed=4)
    out, info = eng.ode_sample_fixed(mixn, MIX, method="dpmpp2m", steps=4, t_start=0.5, eps=EPS, denoise=False, x_init=x_init)
    y, _, _, _ = host_solve(eng, MIX, mixn, x_init, None, "dpmpp2m", R.uniform_grid(4, t0=0.5))
    assert info["nfe"] == 4 and torch.equal(out, y.float())
    with pytest.raises(_lib.DiffsepError, match="starts below 1 needs the state to start from"):
        eng.ode_sample_fixed(mixn, MIX, method="ddim", steps=4, t_start=0.5, eps=EPS)
    with pytest.raises(_lib.DiffsepError, match="x_init and noise are alternatives"):
        eng.ode_sample_fixed(mixn, MIX, method="ddim", steps=4, eps=EPS, x_init=x_init, noise=x_init)
    with pytest.raises(_lib.DiffsepError, match="err_out needs the second-order method"):
        eng.ode_sample_fixed(mixn, MIX, method="ddim", steps=4, eps=EPS, want_err=True)
    with pytest.raises(_lib.DiffsepError, match="steps \\+ 1 = 5 times"):
        eng.ode_sample_fixed(mixn, MIX, method="ddim", steps=4, eps=EPS, timesteps=[1.0, 0.5, 0.03])
    with pytest.raises(NotImplementedError, match="ode_sample_fixed: method 'dpmpp3m'"):
        eng.ode_sample_fixed(mixn, MIX, method="dpmpp3m", steps=4, eps=EPS)


def test_head_steps_run_on_the_other_engine():
    M = 3
    half = engine(dtype=_lib.F16)
    full = engine(lib_kind="f16")  # an fp32 engine of the half-precision build: what an F16 engine can name as its tail
    mix_norm, x_T, _ = inputs(2, MIX, "hybrid")
    kw = dict(method="dpmpp2m", steps=M, eps=EPS, denoise=False, x_init=x_T)
    want, _ = full.ode_sample_fixed(mix_norm, MIX, **kw)
    got, info = half.ode_sample_fixed(mix_norm, MIX, tail=full, head_steps=M, **kw)
    own, _ = half.ode_sample_fixed(mix_norm, MIX, **kw)
    assert info["nfe"] == M and torch.equal(got, want) and not torch.equal(own, want)
    mixed, _ = half.ode_sample_fixed(mix_norm, MIX, tail=full, tail_steps=1, **kw)
    assert not torch.equal(mixed, own) and not torch.equal(mixed, want)


# ---------------------------------------------------------------- 9. the call does not block
def test_call_returns_before_the_solve_has_run():
    eng = engine()
    mix_norm, x_T, _ = inputs(2, MIX, "async")
    kw = dict(method="dpmpp2m", steps=128, eps=EPS, x_init=x_T)
    want, _ = eng.ode_sample_fixed(mix_norm, MIX, **kw)  # (also: plan, graph and buffers exist before the timed call)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        out, info = eng.ode_sample_fixed(mix_norm, MIX, **kw)
        running = not side.query()
    side.synchronize()
    assert info["nfe"] == 128 and running, "the 128 evaluations had drained when the call returned"
    assert torch.equal(out, want)


# ---------------------------------------------------------------- 10. the local-error trace
@pytest.mark.parametrize("kind", ["mix", "priormix"])
def test_error_trace_is_the_step_minus_its_ddim_step(kind):
    M = 5
    mix_norm, x_T, smix, ts, (y, steps, norms, tab) = host_case(kind, "dpmpp2m", M, "log")
    kw = dict(method="dpmpp2m", steps=M, eps=EPS, denoise=False, x_init=x_T, timesteps=ts)
    plain, _ = engine().ode_sample_fixed(mix_norm, SDES[kind], **kw)
    out, info = engine().ode_sample_fixed(mix_norm, SDES[kind], want_err=True, **kw)
    err = info["err"].cpu().numpy()
    assert err.shape == (M, 2, 2) and torch.equal(out, plain)
    assert np.all(err[0, :, 0] == 0.0) and np.all(err[1:] > 0.0)
    sm = None if smix is None else smix.cpu().numpy()
    rms = lambda v: np.sqrt(np.mean(v * v))
    for i, (y_i, prev, score) in enumerate(steps):
        d = R.step(y_i, score, tab[i], prev, sm)[2]
        for b in range(2):
            assert abs(err[i, b, 0] - rms(d[b])) <= 1e-12 * rms(d[b]), (i, b)
            assert abs(err[i, b, 1] - rms(y_i[b])) <= 1e-12 * rms(y_i[b]), (i, b)
    assert np.array_equal(err, norms)  # ... and the unit entry's norms are the driver's


# ---------------------------------------------------------------- 11. against the independent network
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
    ts = R.uniform_grid(M)
    tab = R.table(sde, "dpmpp2m", ts)

    def score_fn(t, y):
        x = torch.from_numpy(y.astype(np.float32))
        return O.score_forward(p, ocfg, x, torch.ones(B) * float(np.float32(t)), mix_c).numpy()

    y, prev = x_T.cpu().double().numpy(), None
    for i in range(M):  # the restatement's steps around the oracle's network
        x0, y, _ = R.step(y, score_fn(ts[i], y), tab[i], prev if i >= 1 else None, None if sm is None else sm[:, 0].numpy())
        prev = x0
    x = torch.from_numpy(y.astype(np.float32))
    te = torch.ones(B) * EPS
    _, ref = O.predictor_reverse_diffusion(ocfg, x, te, O.score_forward(p, ocfg, x, te, mix_c), torch.zeros_like(x), N, smix=sm)
    out, info = eng.ode_sample_fixed(mix_norm, sde, method="dpmpp2m", steps=M, eps=EPS, N=N, x_init=x_T)
    err = rel_rms(out.cpu(), ref)
    print(f"{kind}: dpmpp2m M = {M} with denoise against the CPU oracle: rel rms {err:.3e}")
    assert info["nfe"] == M and err <= 1e-3


# ---------------------------------------------------------------- the model's methods and evaluate
def test_model_and_evaluate_cli_with_the_new_methods(tmp_path):
    from diffsep_amd.pl_model import DiffSepModel, default_config
    model = DiffSepModel(default_config(nf=16), dtype="f32", device="cuda")
    mix = torch.from_numpy(synth.synth_batch(2, T=T)[0]).cuda()
    a = model.separate(mix, sampler="ode-fixed", method="ddim", steps=3, seed=7)
    b = model.separate(mix, sampler="ode-fixed", method="ddim", steps=3, seed=7)
    assert tuple(a.shape) == (2, S, T) and bool(torch.isfinite(a).all()) and torch.equal(a, b)
    out, info = model.refine(mix, a, t_start=0.4, sampler="ode-fixed", method="dpmpp2m", steps=2, seeds=[1, 2])
    assert info["t"] == 0.4 and info["nfe"] == 2 and info["steps"] == 2 and info["method"] == "dpmpp2m"
    assert tuple(out.shape) == (2, S, T) and bool(torch.isfinite(out).all()) and not torch.equal(out, a)
    eval_cli.main(["--synthetic", "2", "--samples", "4000", "--synthetic-weights", "16", "--dtype", "f32", "--flat-output",
                   "--batch", "2", "--save-n", "0", "--no-stoi", "--sampler", "ode-fixed", "--ode-method", "dpmpp2m",
                   "--ode-steps", "4", "--ode-err", "-o", str(tmp_path)])
    rec = json.load(open(tmp_path / "test.json"))
    summ = json.load(open(tmp_path / "test_summary.json"))
    assert all(r["nfe"] == 4 and np.isfinite(r["ode_local_err"]) and r["ode_local_err"] > 0 for r in rec)
    assert summ["sampler"] == "ode-fixed" and summ["ode_method"] == "dpmpp2m" and summ["ode_steps"] == 4 and summ["nfe"] == 4
