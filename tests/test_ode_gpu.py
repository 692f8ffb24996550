"""The probability-flow ODE sampler on the MI355X (diffsep_ode_sample, sdes.get_ode_sampler; reference
sdes/__init__.py:193-278): its two passes in isolation, the device controller against scipy's solve_ivp driven by the
same drift, the CPU oracle end to end, denoise semantics, determinism, the 16-bit bound and the CLI."""
import numpy as np
import pytest
import scipy.integrate
import torch

import diffsep_oracle as O
from diffsep_amd import _lib, ops, sdes, synth, wavio
from diffsep_amd import separate as sep_cli
from diffsep_amd.engine import Engine, pack_state_dict, param_table
from diffsep_amd.pl_model import DiffSepModel, default_config

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

NF, S, T = 16, 2, 4000
MIX = dict(kind=_lib.SDE_MIX, ndim=2, d_lambda=2.0, sigma_min=0.05, sigma_max=0.5)
PRIOR = dict(kind=_lib.SDE_PRIORMIX, ndim=2, d_lambda=2.0, sigma_min=0.05, sigma_max=0.5, avg_len=510)
_cache = {}


def rel_rms(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(np.mean((a - b) ** 2)) / (np.sqrt(np.mean(b ** 2)) + 1e-30))


def engine(spec_factor=0.33, dtype=_lib.F32):
    key = (spec_factor, dtype)
    if key not in _cache:
        cfg = _lib.model_config(nf=NF, num_sources=S, spec_factor=spec_factor, dtype=dtype)
        sd = synth.synth_state_dict([(n, s) for n, s, _ in param_table(cfg)], 7)
        _cache[key] = (Engine(cfg, pack_state_dict(cfg, sd)), sd)
    return _cache[key]


def inputs(B, sde, tag="a"):
    mix = torch.from_numpy(synth.synth_batch(B, T=T)[0]).cuda()
    mix_norm, _, _ = ops.normalize_batch(mix)
    z = torch.from_numpy(synth.synth_noise(f"ode.{tag}", (B, S, T))).cuda()
    smix = ops.sde_sigma_mix(mix_norm, sde["avg_len"]) if sde["kind"] == _lib.SDE_PRIORMIX else None
    x_T = ops.sde_prior(sde, mix_norm, z, smix)
    return mix_norm, x_T, smix


# ---------------------------------------------------------------- 1. the two passes in isolation
def test_stage_and_error_passes_match_numpy_float64():
    B = 2
    g = torch.Generator().manual_seed(3)
    K = [torch.randn(B, S, T, generator=g).cuda() for _ in range(7)]
    y = torch.randn(B, S, T, generator=g, dtype=torch.float64).cuda()
    y2 = y + 1e-3 * torch.randn(B, S, T, generator=g, dtype=torch.float64).cuda()
    A, Bt, C, E, ns, _ = _lib.ode_tableau("RK45")
    h = -0.0123456789
    Kn = [k.cpu().double().numpy() for k in K]
    yn, y2n = y.cpu().numpy(), y2.cpu().numpy()

    def comb(c, n):
        acc = np.zeros_like(yn)
        for j in range(n):
            acc = acc + c[j] * Kn[j]
        return acc

    for rep in range(2):
        outs = []
        for s in range(1, ns):  # stage inputs fp32(y + (sum_j a_sj K_j) h)
            xo = torch.empty(B, S, T, device="cuda")
            ops.ode_stage_update(MIX, K, A[s, :s], h, y, x_out=xo)
            want = (yn + comb(A[s], s) * h).astype(np.float32)
            assert np.array_equal(xo.cpu().numpy(), want), s
            outs.append(xo)
        yo, xo = torch.empty_like(y), torch.empty(B, S, T, device="cuda")
        ops.ode_stage_update(MIX, K, Bt, h, y, x_out=xo, y_new_out=yo)
        want = yn + h * comb(Bt, ns)
        assert np.array_equal(yo.cpu().numpy(), want) and np.array_equal(xo.cpu().numpy(), want.astype(np.float32))
        nrm = ops.ode_error_norm(MIX, K, E, h, y, 1e-5, 1e-5, y_new=y2).cpu().numpy()
        sc = 1e-5 + np.maximum(np.abs(yn), np.abs(y2n)) * 1e-5
        e0 = np.linalg.norm(comb(E, ns + 1) * h / sc) / np.sqrt(yn.size)
        e1 = np.linalg.norm(yn / sc) / np.sqrt(yn.size)
        assert abs(nrm[0] - e0) <= 1e-12 * e0 and abs(nrm[1] - e1) <= 1e-12 * e1
        if rep == 0:
            first = [o.clone() for o in outs] + [yo.clone(), xo.clone(), torch.from_numpy(nrm)]
        else:
            again = outs + [yo, xo, torch.from_numpy(nrm)]
            assert all(torch.equal(a, b) for a, b in zip(first, again))  # repeated runs: the same bits


@pytest.mark.parametrize("T_", [262401, 1049604], ids=["one_sample_items", "four_sample_items"])
def test_passes_beyond_the_capped_grid_match_numpy_float64(T_):
    # more than DS_ODE_MAX_BLOCKS x 256 = 262144 thread items in one system (262401 of one sample; 262401 of four): the grid
    # is capped and the grid-stride loop takes a second trip, which no other test does
    g = torch.Generator(device="cuda").manual_seed(5)
    K = [torch.randn(1, S, T_, generator=g, device="cuda") for _ in range(7)]
    y = torch.randn(1, S, T_, generator=g, dtype=torch.float64, device="cuda")
    y2 = y + 1e-3 * torch.randn(1, S, T_, generator=g, dtype=torch.float64, device="cuda")
    A, Bt, C, E, ns, _ = _lib.ode_tableau("RK45")
    h = -0.0123456789
    Kn = [k.cpu().double().numpy() for k in K]
    yn, y2n = y.cpu().numpy(), y2.cpu().numpy()

    def comb(c, n):
        acc = np.zeros_like(yn)
        for j in range(n):
            acc = acc + c[j] * Kn[j]
        return acc

    for s in range(1, ns):
        xo = torch.empty(1, S, T_, device="cuda")
        ops.ode_stage_update(MIX, K, A[s, :s], h, y, x_out=xo)
        assert np.array_equal(xo.cpu().numpy(), (yn + comb(A[s], s) * h).astype(np.float32)), s
    yo, xo = torch.empty_like(y), torch.empty(1, S, T_, device="cuda")
    ops.ode_stage_update(MIX, K, Bt, h, y, x_out=xo, y_new_out=yo)
    want = yn + h * comb(Bt, ns)
    assert np.array_equal(yo.cpu().numpy(), want) and np.array_equal(xo.cpu().numpy(), want.astype(np.float32))
    nrm = ops.ode_error_norm(MIX, K, E, h, y, 1e-5, 1e-5, y_new=y2).cpu().numpy()
    sc = 1e-5 + np.maximum(np.abs(yn), np.abs(y2n)) * 1e-5
    e0 = np.linalg.norm(comb(E, ns + 1) * h / sc) / np.sqrt(yn.size)
    e1 = np.linalg.norm(yn / sc) / np.sqrt(yn.size)
    print(f"T = {T_}: norms {nrm}, numpy {e0} {e1}")
    assert abs(nrm[0] - e0) <= 1e-12 * e0 and abs(nrm[1] - e1) <= 1e-12 * e1


@pytest.mark.parametrize("sde", [MIX, PRIOR], ids=["mix", "priormix"])
def test_fused_drift_is_the_unit_drift_bit_for_bit(sde):
    eng, _ = engine()
    B = 2
    mix_norm, x, smix = inputs(B, sde, "drift")
    t = torch.full((B,), 0.4321, device="cuda")
    score = eng.score(x, t, mix_norm)
    f, G = ops.sde_coefficients(sde, x, t, smix)
    want = ops.sde_reverse_drift(f, G, score, probability_flow=True)
    K = [torch.zeros(B, S, T, device="cuda") for _ in range(2)]
    y = x.double()
    xo = torch.empty_like(x)
    ops.ode_stage_update(sde, K, [0.5, 0.25], -0.01, y, k_out=1, x=x, t=t, score=score,
                         sigma_mix=smix, x_out=xo)  # drift into K[1] fused with a stage combination
    assert torch.equal(K[1], want)
    nrm = ops.ode_error_norm(sde, K, [0.0, 1.0], 1.0, y, 1e-5, 1e-5, k_out=1, x=x, t=t, score=score, sigma_mix=smix)
    assert torch.equal(K[1], want) and torch.isfinite(nrm).all()


# ---------------------------------------------------------------- 2. same drift, two integrators
def _scipy_on_engine_drift(eng, sde, mix_norm, x_T, method, rtol, atol, eps=0.03):
    B = x_T.shape[0]
    shape = tuple(x_T.shape)

    def fun(t, yv):
        x = torch.from_numpy(yv.astype(np.float32).reshape(shape)).cuda()
        tt = torch.ones(B, device="cuda") * float(t)
        score = eng.score(x, tt, mix_norm)
        f, G = ops.sde_coefficients(sde, x, tt)
        return ops.sde_reverse_drift(f, G, score, probability_flow=True).cpu().double().numpy().reshape(-1)

    ts = []
    solver_cls = {"RK45": scipy.integrate.RK45, "RK23": scipy.integrate.RK23}[method]
    orig = solver_cls._step_impl

    def step(self):  # count accepted / rejected attempts: every attempt costs n_stages evaluations
        ok, msg = orig(self)
        if ok:
            ts.append(self.t)
        return ok, msg

    solver_cls._step_impl = step
    try:
        sol = scipy.integrate.solve_ivp(fun, (1.0, eps), x_T.cpu().double().numpy().reshape(-1), method=method,
                                        rtol=rtol, atol=atol)
    finally:
        solver_cls._step_impl = orig
    return sol, ts


@pytest.mark.parametrize("method, tol", [("RK45", 1e-5), ("RK45", 1e-3), ("RK23", 1e-3)])
def test_device_controller_matches_scipy_on_the_same_drift(method, tol):
    eng, _ = engine()
    mix_norm, x_T, _ = inputs(2, MIX, "scipy")
    sol, ts = _scipy_on_engine_drift(eng, MIX, mix_norm, x_T, method, tol, tol)
    ns = {"RK45": 6, "RK23": 3}[method]
    out, info = eng.ode_sample(mix_norm, MIX, method=method, rtol=tol, atol=tol, eps=0.03, denoise=False, x_init=x_T)
    n_att = (sol.nfev - 2) // ns
    print(f"{method} tol {tol}: scipy nfev {sol.nfev} ({len(ts)} accepted), device {info}")
    assert sol.status == 0 and info["status"] == 0
    assert info["nfev"] == sol.nfev and info["n_accepted"] == len(ts) and info["n_rejected"] == n_att - len(ts)
    assert abs(info["t_final"] - ts[-1]) <= 1e-9
    assert rel_rms(out.cpu(), sol.y[:, -1].reshape(out.shape)) <= 1e-5


def test_accepted_time_grid_matches_scipy():
    # the accepted t grid itself (RK45 at 1e-4): the device solver's steps are recorded through max_nfe prefixes
    eng, _ = engine()
    mix_norm, x_T, _ = inputs(2, MIX, "grid")
    sol, ts = _scipy_on_engine_drift(eng, MIX, mix_norm, x_T, "RK45", 1e-4, 1e-4)
    _, full = eng.ode_sample(mix_norm, MIX, rtol=1e-4, atol=1e-4, denoise=False, x_init=x_T)
    assert full["n_accepted"] == len(ts) and abs(full["t_final"] - ts[-1]) <= 1e-9
    for m in range(8, min(full["nfev"], 8 + 6 * 4) + 1, 6):  # the first few attempts, one at a time
        _, info = eng.ode_sample(mix_norm, MIX, rtol=1e-4, atol=1e-4, denoise=False, x_init=x_T, max_nfe=m)
        if info["n_accepted"]:
            assert abs(info["t_final"] - ts[info["n_accepted"] - 1]) <= 1e-9


# ---------------------------------------------------------------- 3. oracle gate
@pytest.mark.parametrize("sde, spec_factor", [(MIX, 0.33), (PRIOR, 0.15)], ids=["mix", "priormix-enhancement"])
def test_engine_matches_cpu_oracle_end_to_end(sde, spec_factor):
    eng, sd = engine(spec_factor)
    B, N, eps, tol = 1, 30, 0.03, 1e-4
    mix_norm, x_T, _ = inputs(B, sde, "oracle")
    ocfg = O.default_config(NF, S, spec_factor=spec_factor)
    p = O.to_torch(sd)
    mix_c = mix_norm.cpu()
    sm = O.sigma_mix(mix_c, sde["avg_len"]) if sde["kind"] == _lib.SDE_PRIORMIX else None
    shape = tuple(x_T.shape)

    def fun(t, yv):
        x = torch.from_numpy(yv.astype(np.float32).reshape(shape))
        tt = torch.ones(B) * float(t)
        score = O.score_forward(p, ocfg, x, tt, mix_c)
        f, G = O.sde_coefficients(ocfg, x, tt, None if sm is None else sm[:, 0])
        G = G if G.dim() == 3 else G[:, None, None]
        return (f - 0.5 * G ** 2 * score).double().numpy().reshape(-1)

    sol = scipy.integrate.solve_ivp(fun, (1.0, eps), x_T.cpu().double().numpy().reshape(-1), method="RK45", rtol=tol,
                                    atol=tol)
    x = torch.from_numpy(sol.y[:, -1].astype(np.float32).reshape(shape))
    te = torch.ones(B) * eps
    _, ref = O.predictor_reverse_diffusion(ocfg, x, te, O.score_forward(p, ocfg, x, te, mix_c), torch.zeros_like(x), N,
                                           smix=sm)
    out, info = eng.ode_sample(mix_norm, sde, rtol=tol, atol=tol, eps=eps, N=N, x_init=x_T)
    err = rel_rms(out.cpu(), ref)
    print(f"oracle nfev {sol.nfev}, engine nfev {info['nfev']} ({info}), rel rms {err:.2e}")
    assert info["status"] == 0 and abs(info["nfev"] - sol.nfev) <= 6
    assert err <= 1e-3


# ---------------------------------------------------------------- 4. denoise semantics
def test_denoise_is_one_predictor_step_at_eps():
    eng, _ = engine()
    mix_norm, x_T, _ = inputs(2, MIX, "denoise")
    raw, i0 = eng.ode_sample(mix_norm, MIX, rtol=1e-3, atol=1e-3, denoise=False, x_init=x_T, N=30)
    den, i1 = eng.ode_sample(mix_norm, MIX, rtol=1e-3, atol=1e-3, denoise=True, x_init=x_T, N=30)
    assert i0 == i1
    te = torch.full((2,), np.float32(0.03), device="cuda")
    _, xm = ops.sde_predictor_update(MIX, 30, raw, te, eng.score(raw, te, mix_norm), None)
    assert torch.equal(xm, den)


# ---------------------------------------------------------------- 5. determinism, workspace
def test_seeded_runs_are_bit_identical_and_the_pc_workspace_is_unchanged():
    cfg = _lib.model_config(nf=NF, num_sources=S)
    blob = pack_state_dict(cfg, synth.synth_state_dict([(n, s) for n, s, _ in param_table(cfg)], 7))
    e1, e2 = Engine(cfg, blob), Engine(cfg, blob)
    mix_norm, _, _ = inputs(2, MIX, "det")
    for e in (e1, e2):
        e.pc_sample(mix_norm, MIX, N=2, seed=1)
    b0 = e1.device_bytes()
    assert e2.device_bytes() == b0
    a, ia = e1.ode_sample(mix_norm, MIX, rtol=1e-3, atol=1e-3, seed=5)
    b, ib = e1.ode_sample(mix_norm, MIX, rtol=1e-3, atol=1e-3, seed=5)
    c, _ = e1.ode_sample(mix_norm, MIX, rtol=1e-3, atol=1e-3, seed=6)
    assert torch.equal(a, b) and ia == ib and not torch.equal(a, c)
    assert e1.device_bytes() > b0  # the ODE buffers, allocated at its first call ...
    e2.pc_sample(mix_norm, MIX, N=2, seed=1)
    assert e2.device_bytes() == b0  # ... and only on the engine that ran it
    with pytest.raises(_lib.DiffsepError):
        e1.ode_sample(mix_norm, MIX, lengths=[T, T - 100])
    with pytest.raises(_lib.DiffsepError):
        e1.ode_sample(mix_norm, MIX, tail=e2)


# ---------------------------------------------------------------- 6. bounded work on a 16-bit engine
def test_f16_engine_is_bounded_by_max_nfe():
    eng, _ = engine(dtype=_lib.F16)
    mix_norm, x_T, _ = inputs(2, MIX, "f16")
    out, info = eng.ode_sample(mix_norm, MIX, max_nfe=60, x_init=x_T)
    print(f"f16 at rtol = atol = 1e-5, max_nfe 60: {info}")
    assert torch.isfinite(out).all() and info["status"] == 1 and info["nfev"] <= 60


# ---------------------------------------------------------------- 7. API + CLI
def test_get_ode_sampler_and_cli(tmp_path):
    ind, outd = tmp_path / "in", tmp_path / "out"
    ind.mkdir()
    for i in range(2):
        wavio.save(ind / f"utt{i}.wav", torch.from_numpy(synth.synth_mixture(i, T=T)[0]), 8000)
    sep_cli.main([str(ind), str(outd), "--synthetic-weights", "16", "--dtype", "f32", "--sampler", "ode", "--rtol", "1e-3",
                  "--atol", "1e-3", "--seed", "11"])
    model = DiffSepModel(default_config(nf=16), dtype="f32", device="cuda")
    seeds = torch.randint(0, 2 ** 62, (2,), generator=torch.Generator().manual_seed(11)).tolist()
    for i in range(2):
        mix, _ = wavio.load(ind / f"utt{i}.wav")
        mix = mix[None].cuda()
        (mix_norm, _), *_ = model.normalize_batch((mix, None))
        sampler = model.get_ode_sampler(mix_norm, rtol=1e-3, atol=1e-3, seed=seeds[i])
        sep, nfe = sampler()
        assert nfe == sampler.info["nfev"] > 2 and sampler.info["status"] == 0
        want = sep_cli.scale_output(mix, sep).cpu()
        for k in range(2):
            y, sr = wavio.load(outd / f"s{k}" / f"utt{i}.wav")
            assert sr == 8000 and torch.isfinite(y).all() and torch.equal(y[0], want[0, k])
    # the reference's z: the caller's x_T
    z = torch.randn(1, 2, T, device="cuda")
    xa, _ = model.get_ode_sampler(mix_norm, rtol=1e-3, atol=1e-3)(z=z)
    xb, _ = model.get_ode_sampler(mix_norm, rtol=1e-3, atol=1e-3)(z=z)
    assert torch.equal(xa, xb)
    with pytest.raises(NotImplementedError):
        sdes.get_ode_sampler(model.sde, model, mix_norm, method="LSODA")
