"""The exponential-integrator solve (DDIM, DPM-Solver++ 2M), host side (no GPU): the coefficient table of
diffsep_expint_coefficients against the numpy restatement of tests/expint_ref.py; the table walked in float64 on a point-mass
score (where one DDIM step is exact) and on a Gaussian score (observed orders, cost against Heun); every refusal by its message;
the bindings, the factory and the two CLIs with stand-ins in place of engines; and the stand-alone program
tests/expint_main.cpp, which walks csrc/ode_host.h's plan itself, once plainly and once under AddressSanitizer + UBSan.

Measured here (float64, MixSDE d_lambda = 2, sigma 0.05 .. 0.5; printed by the tests):
  table against numpy: largest relative deviation 5.7e-14 (gate 1e-12);
  point mass (S = 3), 1 -> 0.03: one DDIM step off by 2.2e-16, 7 steps of 2M by 1.7e-16, Euler at 30 steps by 5.0e-3;
  Gaussian data N(0.6, 1), uniform grid, M = 64 -> 128: observed order 0.995 (DDIM), 1.995 (2M); at M = 16 the error of 2M
  (16 evaluations) is 8.2e-3, of Heun (32 evaluations) 1.16e-2."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import expint_ref as R
from diffsep_amd import _lib, sdes
from diffsep_amd import evaluate as eval_cli
from diffsep_amd import separate as sep_cli

HERE = os.path.dirname(os.path.abspath(__file__))
EPS = 0.03
MIX = dict(kind=_lib.SDE_MIX, ndim=2, d_lambda=2.0, sigma_min=0.05, sigma_max=0.5)
PRIOR = dict(kind=_lib.SDE_PRIORMIX, ndim=2, d_lambda=1.5, sigma_min=0.03, sigma_max=0.7, avg_len=510)
SDES = {"mix": MIX, "priormix": PRIOR}
METHODS = ["ddim", "dpmpp2m"]


def rel_dev(got, want):
    scale = np.where(want == 0.0, 1.0, np.abs(want))  # (w1 = 0 of a first-order step: compared absolutely, it is exact)
    return float(np.max(np.abs(got - want) / scale))


# ---------------------------------------------------------------- 1. the table against numpy
@pytest.mark.parametrize("kind", ["mix", "priormix"])
@pytest.mark.parametrize("grid", ["uniform", "log", "late"])
@pytest.mark.parametrize("method", METHODS)
def test_coefficient_table_matches_the_numpy_restatement(method, grid, kind):
    sde = SDES[kind]
    worst = 0.0
    for M in (1, 2, 9, 128):
        if grid == "uniform":
            ts = R.uniform_grid(M)
            got = _lib.expint_coefficients(sde, method, M, eps=EPS)
        elif grid == "log":
            ts = R.log_grid(M)
            got = _lib.expint_coefficients(sde, method, M, eps=EPS, timesteps=ts)
        else:  # a start at t_start = 0.5
            ts = R.uniform_grid(M, t0=0.5)
            got = _lib.expint_coefficients(sde, method, M, t_start=0.5, eps=EPS)
        want = R.table(sde, method, ts)
        assert got.shape == want.shape == (M, _lib.EXPINT_COEFS)
        worst = max(worst, rel_dev(got, want))
        assert np.all(got[0, [R.W0_A, R.W0_P]] == 1.0) and np.all(got[0, [R.W1_A, R.W1_P]] == 0.0)  # step 0 is a DDIM step
        if method == "ddim":
            assert np.all(got[:, [R.W0_A, R.W0_P]] == 1.0) and np.all(got[:, [R.W1_A, R.W1_P]] == 0.0)
        assert np.all(got[:, R.AL_A] == 1.0)
    print(f"{method} {grid} {kind}: largest relative deviation of the table {worst:.3g}")
    assert worst <= 1e-12


# ---------------------------------------------------------------- 2. exact on a point mass
def point_mass(sde, c, z, ts):
    """(score function, start state at ts[0], the exact state at ts[-1]) for data concentrated at c [S,1]; A = 11^T / S"""
    proj = lambda v: (np.mean(v, axis=0, keepdims=True), v - np.mean(v, axis=0, keepdims=True))

    def at(t):
        (cA, cP), (zA, zP) = proj(c), proj(z)
        ev1, ev2 = R.eig(sde, t)
        return cA + R.alphas(sde, t)[1] * cP + np.sqrt(ev1) * zA + np.sqrt(ev2) * zP

    def score(t, u):
        (cA, cP), (uA, uP) = proj(c), proj(u)
        ev1, ev2 = R.eig(sde, t)
        return -((uA - cA) / ev1 + (uP - R.alphas(sde, t)[1] * cP) / ev2)

    return score, at(ts[0]), at(ts[-1])


def test_one_ddim_step_is_exact_on_a_point_mass_and_euler_is_not():
    c = np.array([[0.7], [-0.4], [0.15]])
    z = np.array([[0.3], [-1.1], [0.6]])
    for method, M in (("ddim", 1), ("dpmpp2m", 7)):
        ts = R.uniform_grid(M)
        score, u1, want = point_mass(MIX, c, z, ts)
        got, _ = R.solve(score, u1, _lib.expint_coefficients(MIX, method, M, eps=EPS), ts, method)
        err = float(np.max(np.abs(got - want)))
        print(f"{method}, {M} step(s) from 1 to {EPS} on a point mass: off by {err:.3g}")
        assert err <= 1e-12
    ts = R.uniform_grid(30)
    score, u, want = point_mass(MIX, c, z, ts)
    lam = R.params(MIX)[0]
    for i in range(30):  # Euler on f(x,t) - 0.5 g(t)^2 score, f = -lambda P x
        drift = -lam * (u - np.mean(u, axis=0, keepdims=True)) - 0.5 * R.g2(MIX, ts[i]) * score(ts[i], u)
        u = u + (ts[i + 1] - ts[i]) * drift
    err = float(np.max(np.abs(u - want)))
    print(f"Euler, 30 steps on the same score: off by {err:.3g}")
    assert err > 1e-3


# ---------------------------------------------------------------- 3. orders on Gaussian data
def gaussian_case(sde, j, m=0.6, v=1.0, u1=1.3):
    """eigenspace j as a scalar diffusion with data N(m, v): (score(t, u), exact(t), ode right-hand side(t, u)).
    v = 1: the models see mixtures normalised to unit variance, so that is the scale of the data a sampler meets; m and the
    start u1 are off zero so that the alpha m term takes part.  (The orders do not depend on the choice; the comparison with
    Heun does: a narrow data distribution, v << ev(1), approaches the point mass where these methods are exact and Heun is
    stiff, a wider one favours Heun — DESIGN.md section 5m has the scan.)"""
    al = lambda t: R.alphas(sde, t)[j]
    V = lambda t: al(t) ** 2 * v + R.eig(sde, t)[j]
    a = (0.0, R.params(sde)[0])[j]
    score = lambda t, u: -(u - al(t) * m) / V(t)
    exact = lambda t: al(t) * m + np.sqrt(V(t) / V(1.0)) * (u1 - al(1.0) * m)
    rhs = lambda t, u: -a * u - 0.5 * R.g2(sde, t) * score(t, u)
    return score, exact, rhs, u1


def expint_error(sde, method, M):
    """largest error over the two eigenspaces of the table's walk on Gaussian data at eps"""
    ts = R.uniform_grid(M)
    tab = _lib.expint_coefficients(sde, method, M, eps=EPS)
    worst = 0.0
    for j in range(2):
        score, exact, _, u = gaussian_case(sde, j)
        prev = None
        for i in range(M):
            cx, cd, w0, w1 = tab[i, 4 * j:4 * j + 4]
            al, ev = tab[i, R.AL_A + 2 * j], tab[i, R.EV_A + 2 * j]
            x0 = (u + ev * score(ts[i], u)) / al
            u = cx * u + cd * (w0 * x0 + (w1 * prev if prev is not None else 0.0))
            prev = x0
        worst = max(worst, abs(u - exact(EPS)))
    return worst


def heun_error(sde, M):
    ts = R.uniform_grid(M)
    worst = 0.0
    for j in range(2):
        _, exact, rhs, u = gaussian_case(sde, j)
        for i in range(M):
            h = ts[i + 1] - ts[i]
            k1 = rhs(ts[i], u)
            k2 = rhs(ts[i + 1], u + h * k1)
            u = u + h * (0.5 * k1 + 0.5 * k2)
        worst = max(worst, abs(u - exact(EPS)))
    return worst


def test_observed_orders_and_cost_against_heun():
    bounds = {"ddim": (0.9, 1.1), "dpmpp2m": (1.8, 2.2)}
    for method in METHODS:
        e64, e128 = expint_error(MIX, method, 64), expint_error(MIX, method, 128)
        order = np.log2(e64 / e128)
        print(f"{method}: error {e64:.3g} at M = 64, {e128:.3g} at 128: observed order {order:.3f}")
        assert bounds[method][0] <= order <= bounds[method][1]
    e2m, eh = expint_error(MIX, "dpmpp2m", 16), heun_error(MIX, 16)
    print(f"M = 16: dpmpp2m (16 evaluations) {e2m:.3g}, Heun (32 evaluations) {eh:.3g}")
    assert 0.5 * eh <= e2m <= 2.0 * eh


# ---------------------------------------------------------------- 4. refusals, bindings, factory, CLIs
def test_refusals_of_the_table_by_message():
    def refused(match, sde=MIX, method="ddim", steps=4, **kw):
        with pytest.raises(_lib.DiffsepError) as ei:
            _lib.expint_coefficients(sde, method, steps, **kw)
        assert "expint_coefficients: " in str(ei.value) and match in str(ei.value), str(ei.value)

    refused("method must be DIFFSEP_EXPINT_DDIM or DIFFSEP_EXPINT_DPMPP2M", method=2)
    refused("need a MixSDE or a PriorMixSDE", sde=dict(MIX, kind=2))
    refused("steps must be >= 1", steps=0)
    refused("steps must be <= 16384", steps=16385)
    assert _lib.expint_coefficients(MIX, "dpmpp2m", 16384, eps=EPS).shape == (16384, 12)
    refused("eps must be in (0, 1)", eps=0.0)
    refused("eps must be in (0, 1)", eps=1.0)
    refused("t_start must be above eps", t_start=0.03, eps=EPS)
    refused("the time grid must be strictly descending inside (0, 1]", t_start=1.5)
    refused("the time grid must be strictly descending inside (0, 1]", steps=2, timesteps=[1.0, 0.5, 0.5])
    refused("the time grid must be strictly descending inside (0, 1]", steps=2, timesteps=[1.0, 0.4, 0.5])
    refused("the time grid must be strictly descending inside (0, 1]", steps=2, timesteps=[1.0, 0.5, 0.0])
    refused("ev_1 <= 0", sde=dict(MIX, sigma_max=0.05))
    refused("timesteps must hold steps + 1 = 5 times", timesteps=[1.0, 0.5, 0.03])


def test_binding_constants():
    assert _lib.EXPINT_METHODS == {"ddim": 0, "dpmpp2m": 1} and _lib.EXPINT_ERR_METHODS == ("dpmpp2m",)
    assert (_lib.EXPINT_DDIM, _lib.EXPINT_DPMPP2M, _lib.EXPINT_COEFS) == (0, 1, 12)
    for name in ("diffsep_ode_sample_expint", "diffsep_expint_coefficients", "diffsep_expint_update_each"):
        assert name in _lib.EXPORTS
    # the old names are what they were
    assert _lib.ODEF_METHODS == {"euler": 0, "heun": 1, "midpoint": 2, "rk4": 3, "ab2": 4}
    assert _lib.ODEF_ERR_METHODS == ("heun", "midpoint", "ab2") and _lib.odef_nfe("ab2", 30) == 31
    with pytest.raises(KeyError):
        _lib.odef_nfe("ddim", 30)


class _FakeEngine:
    def __init__(self):
        self.calls = []

    def ode_sample_fixed(self, y, sde, **kw):
        self.calls.append(kw)
        return torch.zeros(y.shape[0], 2, y.shape[2]), dict(nfe=kw["steps"], method=kw["method"], steps=kw["steps"])


class _FakeModel:
    def __init__(self):
        self.eng = _FakeEngine()

    def engine(self):
        return self.eng


def test_factory_passes_the_new_methods_on():
    sde = sdes.MixSDE(ndim=2, d_lambda=2.0, sigma_min=0.05, sigma_max=0.5, N=6)
    y = torch.zeros(1, 1, 100)
    model = _FakeModel()
    x, nfe = sdes.get_ode_fixed_sampler(sde, model, y, method="ddim", seed=3)()
    kw = model.eng.calls[-1]
    assert nfe == 6 and kw["method"] == "ddim" and kw["steps"] == 6 and kw["N"] == 6 and kw["timesteps"] is None
    s = sdes.get_ode_fixed_sampler(sde, model, y, method="dpmpp2m", steps=9, schedule="log", t_start=0.5, x_init=y, want_err=True)
    assert s()[1] == 9 and s.info["steps"] == 9 and s.info["method"] == "dpmpp2m"
    kw = model.eng.calls[-1]
    assert np.array_equal(kw["timesteps"], sdes.ode_fixed_timesteps(9, 0.03, "log", 0.5)) and kw["x_init"] is y and kw["want_err"]
    with pytest.raises(NotImplementedError, match="get_ode_fixed_sampler: method 'dpmpp3m'"):
        sdes.get_ode_fixed_sampler(sde, model, y, method="dpmpp3m")


class _Reached(Exception):
    pass


def _reached():
    raise _Reached()


def test_cli_plumbing(tmp_path, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", _reached)  # a request that passes every check gets as far as the GPU check
    ind = tmp_path / "in"
    ind.mkdir()
    sep = [str(ind), str(tmp_path / "out"), "--synthetic-weights", "16", "--sampler", "ode-fixed"]
    ev = ["--synthetic", "2", "--synthetic-weights", "16", "-o", str(tmp_path), "--sampler", "ode-fixed"]
    for method in METHODS:
        with pytest.raises(_Reached):
            sep_cli.main(sep + ["--ode-method", method, "--ode-steps", "4"])
        with pytest.raises(_Reached):
            eval_cli.main(ev + ["--ode-method", method])
    with pytest.raises(_Reached):
        eval_cli.main(ev + ["--ode-method", "dpmpp2m", "--ode-err"])
    with pytest.raises(SystemExit, match="--ode-err with --ode-method ddim"):
        eval_cli.main(ev + ["--ode-method", "ddim", "--ode-err"])
    for main, base in ((sep_cli.main, sep), (eval_cli.main, ev)):
        with pytest.raises(SystemExit):  # argparse: still no such method
            main(base + ["--ode-method", "rk45"])
    # the refusals of the sampler hold for the new methods word for word
    for flag, argv in (("--chunk", ["--chunk", "4"]), ("--draws", ["--draws", "2", "--batch", "2"])):
        with pytest.raises(SystemExit, match=f"{flag} with --sampler ode-fixed is not supported"):
            sep_cli.main(sep + ["--ode-method", "dpmpp2m"] + argv)
    for flag in ("--fig", "--trajectory"):
        with pytest.raises(SystemExit, match=f"{flag} with --sampler ode-fixed is not supported"):
            eval_cli.main(ev + ["--ode-method", "ddim", flag])
    with pytest.raises(SystemExit, match="--ode-method goes with --sampler ode-fixed"):
        sep_cli.main(sep[:-2] + ["--ode-method", "ddim"])


# ---------------------------------------------------------------- 5. the plan walked by the stand-alone program
def _compiler():
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    return next((c for c in (os.path.join(rocm, "llvm", "bin", "clang++"), shutil.which("g++"), shutil.which("clang++"))
                 if c and os.path.exists(c)), None)


def _runner(exe):
    def run(method, M, t_start=0.0, eps=EPS, denoise=0, N=30, want_err=0, sde=MIX, ts=None):
        argv = [exe, str(R.METHODS.get(method, method)), str(M), repr(float(t_start)), repr(float(eps)), str(denoise), str(N),
                str(want_err), str(sde["kind"]), repr(sde["d_lambda"]), repr(sde["sigma_min"]), repr(sde["sigma_max"])]
        argv += [repr(float(t)) for t in (ts if ts is not None else [])]
        return json.loads(subprocess.run(argv, check=True, capture_output=True, text=True).stdout)
    return run


def _check_program(run):
    for method, M in (("ddim", 1), ("dpmpp2m", 7), ("dpmpp2m", 9)):
        for kind, ts in (("uniform", R.uniform_grid(M)), ("log", R.log_grid(M))):
            got = run(method, M, ts=None if kind == "uniform" else ts, want_err=int(method == "dpmpp2m"))
            assert got["steps"] == M and np.array_equal(np.array(got["t"]), ts)
            coef = np.array(got["coef"]).reshape(M, 12)
            assert rel_dev(coef, R.table(MIX, method, ts)) <= 1e-12
            # ... and the library's table is this plan's (the same code from another compiler: the table's gate)
            assert rel_dev(coef, _lib.expint_coefficients(MIX, method, M, eps=EPS, timesteps=None if kind == "uniform" else ts)) <= 1e-12
            u = np.array(got["u"]).reshape(M, 2)[-1]
            c, z = np.array([0.7, -0.4]), np.array([0.3, -1.1])
            want = np.array(R.alphas(MIX, EPS)) * c + np.sqrt(np.array(R.eig(MIX, EPS))) * z
            assert np.max(np.abs(u - want)) <= 1e-12
            err = np.array(got["err"]).reshape(M, 2)
            assert np.all(err[0] == 0.0) and np.max(np.abs(err)) <= 1e-12  # X0 is c at every step: 2M's correction vanishes
    assert "refused" not in run("dpmpp2m", 2, want_err=1)
    for got, match in ((run("ddim", 2, want_err=1), "err_out needs the second-order method (DPMPP2M: step minus its DDIM step), not DDIM"),
                       (run(2, 2), "method must be DIFFSEP_EXPINT_DDIM or DIFFSEP_EXPINT_DPMPP2M"),
                       (run("ddim", 2, sde=dict(MIX, kind=3)), "need a MixSDE or a PriorMixSDE"),
                       (run("ddim", 0), "steps must be >= 1"),
                       (run("ddim", 2, denoise=1, N=0), "the denoise step needs N >= 1"),
                       (run("ddim", 2, t_start=0.01), "t_start must be above eps"),
                       (run("ddim", 2, ts=[1.0, 0.4, 0.5]), "the time grid must be strictly descending inside (0, 1]"),
                       (run("ddim", 2, sde=dict(MIX, sigma_max=0.04)), "ev_1 <= 0")):
        assert "refused" in got and got["refused"].startswith("expint_main: ") and match in got["refused"], got


def test_program_walks_the_plan(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (the ROCm toolchain's clang++ or g++)")
    exe = str(tmp_path / "expint_main")
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", os.path.join(HERE, "expint_main.cpp"), "-o", exe])
    _check_program(_runner(exe))


def test_program_runs_clean_under_asan_and_ubsan(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (the ROCm toolchain's clang++ or g++)")
    exe = str(tmp_path / "expint_main_san")
    # (the sanitizer runtimes linked statically — clang's default — so that the program stands alone)
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx).startswith("g++") else []
    built = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static,
                            "-ffp-contract=off", "-Wall", os.path.join(HERE, "expint_main.cpp"), "-o", exe],
                           capture_output=True, text=True)
    if built.returncode != 0 and "sanitizer" in built.stderr.lower() + built.stdout.lower():
        pytest.skip("this compiler has no AddressSanitizer / UBSan runtime")
    assert built.returncode == 0, built.stderr
    run = _runner(exe)  # (check=True: a sanitizer report ends the program with a non-zero status)
    _check_program(run)
    assert run("dpmpp2m", 16384)["steps"] == 16384 and "refused" in run("dpmpp2m", 16385)
