"""Warm start, host side (no GPU): the float64 references of tests/warm_start_ref.py against the restated reference
(oracle.sde_mean / mix_std / sigma_mix = marginal_prob) and against numpy.linalg.lstsq, sdes.first_step_for on every grid the
sampler uses, and the refusals of `separate --init-dir`, each of which comes before an engine is needed."""
import numpy as np
import pytest
import torch

import diffsep_oracle as O
import sdecheck as K
import warm_start_ref as W
from diffsep_amd import sdes, synth, wavio
from diffsep_amd import separate as sep_cli

SDE = dict(d_lambda=2.0, sigma_min=0.05, sigma_max=0.5)


# ---------------------------------------------------------------- 1. perturb == marginal_prob of the restated reference
@pytest.mark.parametrize("kind", ["mix", "priormix"])
@pytest.mark.parametrize("S", [2, 3])
def test_perturb_reference_is_marginal_prob(kind, S):
    B, T = 3, 257
    x0 = K.noise(f"ws.cpu.x0.{kind}.{S}", (B, S, T), 0.7)
    z = K.noise(f"ws.cpu.z.{kind}.{S}", (B, S, T))
    y = K.noise(f"ws.cpu.y.{kind}.{S}", (B, 1, T))
    t = np.array([0.03, 0.5, 1.0], np.float32)
    cfg = dict(SDE, ndim=S, kind=1 if kind == "priormix" else 0)
    smix = O.sigma_mix(torch.from_numpy(y).double(), 5)[:, 0].float().numpy() if kind == "priormix" else None
    zero, one = np.zeros(B, np.float32), np.ones(B, np.float32)
    ref, bound = W.perturb(cfg, x0, y, zero, one, t, z, smix=smix, mean_from="estimate")
    td, x0d, zd = torch.from_numpy(t).double(), torch.from_numpy(x0).double(), torch.from_numpy(z).double()
    # (the oracle in float64 on the fp32 SDE scalars the kernel is given, as the reference rounds them: sigma_min = fp32(0.05))
    c32 = {k: (K.f32(v) if isinstance(v, float) else v) for k, v in cfg.items()}
    want = O.sde_mean(c32, x0d, td) + O._apply_std(O.mix_std(c32, td, S), zd, None if smix is None else torch.from_numpy(smix).double()[:, None])
    err = np.abs(ref - want.numpy()).max()
    print(f"{kind} S = {S}: max |perturb - (sde_mean + mix_std z)| = {err:.3e}, smallest bound {bound[bound > 0].min():.3e}")
    # two float64 evaluations of the same expression in different association: a few float64 roundings of values of order 1
    assert err <= 64 * 2.0 ** -53 * max(1.0, np.abs(want.numpy()).max())
    assert (bound > 0).all()
    # the other mode moves only the source average, by (1 - e^{-lambda t}) (y / S - mean_s x0)
    ref_m, _ = W.perturb(cfg, x0, y, zero, one, t, z, smix=smix, mean_from="mix")
    decay = np.exp(-K.f64(t) * 2.0)[:, None]
    assert np.allclose((ref_m - ref).mean(1), (1.0 - decay) * (K.f64(y)[:, 0] / S - K.f64(x0).mean(1)), rtol=0, atol=1e-12)
    assert np.allclose(ref_m - ref_m.mean(1, keepdims=True), ref - ref.mean(1, keepdims=True), rtol=0, atol=1e-12)


# ---------------------------------------------------------------- 2. the gain fit == lstsq
def fit_case(b, T):
    """the estimates e0 = 0.37 t0 + 0.05 t1, e1 = -1.9 t1 of the synthetic sources t0, t1 of mixture b, and that mixture"""
    mix, tgt = synth.synth_mixture(b, T=T)
    est = np.stack([0.37 * tgt[0] + 0.05 * tgt[1], -1.9 * tgt[1]]).astype(np.float32)
    return est, mix


FIT_ANSWER = (1.0 / 0.37, 0.05 / (0.37 * 1.9) - 1.0 / 1.9)


# cond(G) of these inputs, computed here: 26.5, 30.2, 29.7 (utterance 0 at T = 1000, 4099, 7000).  At T = 255 the two synthetic
# sources are correlated enough over 32 ms that cond(G) is 116 (utterances 1 .. 3: 158 .. 1762): that length is not one of the
# cases, the gate cond <= 100 stays as it is.
@pytest.mark.parametrize("T", [1000, 4099, 7000])
def test_gain_fit_reference_is_lstsq(T):
    est, mix = fit_case(0, T)
    g, fb, cond = W.fit(est, mix)
    assert cond <= 100, cond
    E, y = K.f64(est).T, K.f64(mix).reshape(-1)
    want = np.linalg.lstsq(E, y, rcond=None)[0]
    bound = W.gain_bound(want, cond, T)
    print(f"T = {T}: cond(G) = {cond:.2f}, gains {g}, lstsq {want}, |d| = {np.abs(g - want).max():.3e}, bound {bound:.3e}")
    assert fb == 0 and np.abs(g - want).max() <= bound
    # the answer by construction, to the fp32 rounding of the stored estimates and mixture
    assert np.abs(g - np.array(FIT_ANSWER)).max() <= 1e-5
    g2, fb2, _ = W.fit(est, mix, sums=W.sums_device_order)
    assert fb2 == 0 and np.abs(g2 - want).max() <= bound


def test_gain_fit_fallback_rule():
    est, mix = fit_case(1, 1000)
    silent = est.copy()
    silent[1] = 0.0
    assert W.fit(silent, mix)[1] == 1 and np.array_equal(W.fit(silent, mix)[0], np.ones(2))
    same = np.stack([est[0], est[0]])
    assert W.fit(same, mix)[1] == 1
    assert W.fit(est, mix)[1] == 0
    assert W.fit(np.zeros_like(est), mix)[1] == 1  # (trace 0: the pivot 0 is not above the threshold 0)


# ---------------------------------------------------------------- 3. first_step_for
def _grids():
    N, eps = 30, 0.03
    return {sch: sdes.sampler_timesteps(N, eps, sch) for sch in (None, "linear", "log", "revlog")}


@pytest.mark.parametrize("schedule", [None, "linear", "log", "revlog"])
def test_first_step_for(schedule):
    ts = _grids()[schedule]
    assert ts.dtype == np.float32 and ts.shape == (30,) and ts[0] == 1.0 and (np.diff(ts) < 0).all()
    if schedule is None:  # the grid of the fused sampler's default: torch.linspace(1, eps, N) in float32
        assert np.array_equal(ts, torch.linspace(1.0, 0.03, 30).numpy()) and ts[-1] == np.float32(0.03)
    for i in (0, 1, 7, 15, 29):
        on = float(ts[i])
        up = float(np.nextafter(ts[i], np.float32(np.inf)))
        dn = float(np.nextafter(ts[i], np.float32(-np.inf)))
        assert sdes.first_step_for(on, ts) == i
        assert sdes.first_step_for(up, ts) == i  # (one ulp above the point: still the first step at or below it)
        if i < 29:
            assert sdes.first_step_for(dn, ts) == i + 1
        else:
            with pytest.raises(ValueError, match="last step time"):
                sdes.first_step_for(dn, ts)
    assert sdes.first_step_for(1.0, ts) == 0 and sdes.first_step_for(1.5, ts) == 0 and sdes.first_step_for(1e9, ts) == 0
    with pytest.raises(ValueError):
        sdes.first_step_for(0.01, ts)
    with pytest.raises(ValueError):
        sdes.first_step_for(float("nan"), ts)
    assert sdes.first_step_for(0.5, torch.from_numpy(ts)) == sdes.first_step_for(0.5, list(ts))
    assert ts[sdes.first_step_for(0.5, ts)] <= 0.5 < ts[sdes.first_step_for(0.5, ts) - 1]


def test_sampler_range_is_checked_before_any_engine():
    sde = sdes.MixSDE(ndim=2, d_lambda=2.0, sigma_min=0.05, sigma_max=0.5, N=4)
    y = torch.zeros(1, 1, 100)
    for bad in (dict(first_step=1), dict(first_step=2, last_step=2, x_init=y), dict(last_step=5), dict(first_step=-1, x_init=y)):
        with pytest.raises(ValueError, match="first_step"):
            sdes.get_pc_sampler("reverse_diffusion", "ald2", sde, lambda *a: None, y, **bad)


# ---------------------------------------------------------------- 4. the CLI's refusals
def _tree(tmp_path, n=400, sr=8000, est_n=None, est_sr=None, skip=None):
    ind, init = tmp_path / "in", tmp_path / "init"
    ind.mkdir(parents=True)
    for name in ("a", "b"):
        wavio.save(ind / f"{name}.wav", torch.zeros(1, n), sr, bits=32)
        for k in range(2):
            if skip == (name, k):
                continue
            (init / f"s{k}").mkdir(parents=True, exist_ok=True)
            wavio.save(init / f"s{k}" / f"{name}.wav", torch.zeros(1, est_n or n), est_sr or sr, bits=32)
    return str(ind), str(tmp_path / "out"), str(init)


def _refused(argv, match, monkeypatch):
    # reaching the model would be a failure of the test: every refusal comes before an engine is needed
    monkeypatch.setattr(sep_cli, "get_model", lambda args: pytest.fail("the request reached get_model"))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: pytest.fail("the request reached the GPU check"))
    with pytest.raises(SystemExit, match=match):
        sep_cli.main(argv)


def test_cli_refusals(tmp_path, monkeypatch):
    ind, out, init = _tree(tmp_path)
    base = [ind, out, "--synthetic-weights", "16"]
    _refused(base + ["--t-start", "0.5"], "--t-start goes with --init-dir", monkeypatch)
    _refused(base + ["--init-scale", "none"], "--init-scale goes with --init-dir", monkeypatch)
    _refused(base + ["--init-mean", "mix"], "--init-mean goes with --init-dir", monkeypatch)
    _refused(base + ["--init-dir", init], "--init-dir needs --t-start", monkeypatch)
    ok = base + ["--init-dir", init, "--t-start", "0.5"]
    _refused(ok + ["--chunk", "4"], "--init-dir with --chunk", monkeypatch)
    _refused(ok + ["--draws", "2", "--batch", "2"], "--init-dir with --draws", monkeypatch)
    _refused(ok + ["--sampler", "ode"], "--init-dir with --sampler ode", monkeypatch)
    _refused(ok + ["--resample", "file"], "--init-dir with --resample", monkeypatch)
    _refused(base + ["--init-dir", init, "--t-start", "0"], "--t-start 0", monkeypatch)


def test_cli_refuses_bad_estimate_files(tmp_path, monkeypatch):
    ind, out, init = _tree(tmp_path / "missing", skip=("b", 1))
    _refused([ind, out, "--init-dir", init, "--t-start", "0.5"], r"missing estimate file .*s1.b\.wav", monkeypatch)
    ind, out, init = _tree(tmp_path / "length", est_n=399)
    _refused([ind, out, "--init-dir", init, "--t-start", "0.5"], r"a\.wav has 399 samples, its mixture .* has 400", monkeypatch)
    ind, out, init = _tree(tmp_path / "rate", est_sr=16000)
    _refused([ind, out, "--init-dir", init, "--t-start", "0.5"], r"a\.wav is at 16000 Hz, its mixture .* at 8000 Hz", monkeypatch)
    ind, out, init = _tree(tmp_path / "nodir")
    _refused([ind, out, "--init-dir", str(tmp_path / "nowhere"), "--t-start", "0.5"], "missing estimate file", monkeypatch)
