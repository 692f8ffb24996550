"""The fixed-step probability-flow solve, host side (no GPU): csrc/ode_host.h's OdeFixedPlan walked by the stand-alone program
tests/ode_fixed_main.cpp on a small float64 system, against a numpy restatement of the five methods written here from their
definitions; the order each method shows against the closed-form solution; every refusal of the plan by its message; the
grids and refusals of the Python layers and of the two CLIs with stand-ins in place of engines; and the program once more
under AddressSanitizer + UBSan (host code only)."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from diffsep_amd import _lib, sdes
from diffsep_amd import evaluate as eval_cli
from diffsep_amd import separate as sep_cli

HERE = os.path.dirname(os.path.abspath(__file__))
MAT = np.array([[-1.3, 2, 0], [-2, -0.7, 0.5], [0.1, -0.4, -2.1]])
Y0 = np.array([1.0, -0.5, 0.25])
METHODS = ["euler", "heun", "midpoint", "rk4", "ab2"]
CODE = {m: i for i, m in enumerate(METHODS)}
EVALS = {"euler": lambda M: M, "heun": lambda M: 2 * M, "midpoint": lambda M: 2 * M, "rk4": lambda M: 4 * M,
         "ab2": lambda M: M + 1}
ORDER = {"euler": 1, "heun": 2, "midpoint": 2, "rk4": 4, "ab2": 2}
EPS = 0.03


def fun(t, y):
    return (1.0 + 2 * t) * (MAT @ y)


def exact(t, t0=1.0):
    """y' = a(t) M y, a = 1 + 2 t:  y(t) = V exp(lambda (A(t) - A(t0))) V^-1 y0,  A(t) = t + t^2"""
    lam, V = np.linalg.eig(MAT)
    return (V @ (np.exp(lam * ((t + t * t) - (t0 + t0 * t0))) * np.linalg.solve(V, Y0.astype(complex)))).real


def grid(kind, M, t0=1.0, eps=EPS):
    if kind == "uniform":  # the plan's own rule: t_i = t0 + (eps - t0) i / M, t_M = eps
        return np.array([t0 + (eps - t0) * i / M for i in range(M)] + [eps])
    ts = np.logspace(np.log10(t0), np.log10(eps), M + 1)
    ts[0], ts[-1] = t0, eps
    return ts


def ref_solve(method, ts):
    """the method on the grid ts, float64, written from its definition -> (states [M,3], evaluations, err [M,2] or None)"""
    y, n, states, errs = Y0.copy(), 0, [], []
    k_prev = h_prev = None
    for i in range(len(ts) - 1):
        t, h = ts[i], ts[i + 1] - ts[i]
        if method == "euler":
            k1 = fun(t, y); n += 1
            new = y + h * k1
        elif method == "heun" or (method == "ab2" and i == 0):
            k1 = fun(t, y)
            k2 = fun(t + h, y + h * k1); n += 2
            new = y + h * (0.5 * k1 + 0.5 * k2)
            errs.append((h * (k2 - k1) / 2, y))
            k_prev = k1
        elif method == "midpoint":
            k1 = fun(t, y)
            k2 = fun(t + 0.5 * h, y + 0.5 * h * k1); n += 2
            new = y + h * k2
            errs.append((h * (k2 - k1), y))
        elif method == "rk4":
            k1 = fun(t, y)
            k2 = fun(t + 0.5 * h, y + 0.5 * h * k1)
            k3 = fun(t + 0.5 * h, y + 0.5 * h * k2)
            k4 = fun(t + h, y + h * k3); n += 4
            new = y + h * (k1 / 6 + k2 / 3 + k3 / 3 + k4 / 6)
        else:  # ab2 on a possibly non-uniform grid
            k = fun(t, y); n += 1
            w = h / h_prev
            new = y + h * ((1 + w / 2) * k - (w / 2) * k_prev)
            errs.append((h * (w / 2) * (k - k_prev), y))
            k_prev = k
        h_prev = h
        y = new
        states.append(y)
    rms = lambda v: np.sqrt(np.mean(v * v))
    return np.array(states), n, (np.array([[rms(d), rms(yy)] for d, yy in errs]) if errs else None)


def _compiler():
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    return next((c for c in (os.path.join(rocm, "llvm", "bin", "clang++"), shutil.which("g++"), shutil.which("clang++"))
                 if c and os.path.exists(c)), None)


def _runner(exe):
    def run(method, M, t_start=0.0, eps=EPS, denoise=0, N=30, want_err=0, ts=None):
        argv = [exe, str(CODE.get(method, method)), str(M), repr(float(t_start)), repr(float(eps)), str(denoise), str(N),
                str(want_err)] + [repr(float(t)) for t in (ts if ts is not None else [])]
        return json.loads(subprocess.run(argv, check=True, capture_output=True, text=True).stdout)
    return run


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (the ROCm toolchain's clang++ or g++)")
    exe = str(tmp_path_factory.mktemp("ode_fixed") / "ode_fixed_main")
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", os.path.join(HERE, "ode_fixed_main.cpp"),
                           "-o", exe])
    return _runner(exe)


# ---------------------------------------------------------------- 1. the plan's walk against numpy
@pytest.mark.parametrize("kind", ["uniform", "log"])
@pytest.mark.parametrize("method", METHODS)
def test_plan_walk_matches_the_numpy_restatement(program, method, kind):
    M = 12
    ts = grid(kind, M)
    got = program(method, M, ts=None if kind == "uniform" else ts)
    want, n, err = ref_solve(method, ts)
    assert got["steps"] == M and got["n_evals"] == n == EVALS[method](M) and len(got["t_eval"]) == n
    assert np.array_equal(np.array(got["t"]), ts)  # the uniform grid is the plan's own: the same rule, the same float64 times
    y = np.array(got["y"]).reshape(M, 3)
    dev = np.max(np.abs(y - want) / np.abs(want))
    print(f"{method} {kind}: {n} evaluations, largest relative deviation {dev:.3g}")
    assert dev <= 1e-13
    assert got["step_of"] == sorted(got["step_of"]) and set(got["step_of"]) == set(range(M))
    if err is None:
        assert got["has_err"] == 0 and got["err"] == []
    else:
        e = np.array(got["err"]).reshape(M, 2)
        assert got["has_err"] == 1 and np.max(np.abs(e - err) / err) <= 1e-12


def test_t_start_and_stage_times(program):
    got = program("rk4", 4, t_start=0.5)
    ts = grid("uniform", 4, t0=0.5)
    assert np.array_equal(np.array(got["t"]), ts)
    want = [ts[i] + c * (ts[i + 1] - ts[i]) for i in range(4) for c in (0.0, 0.5, 0.5, 1.0)]  # t_i + C[s] h_i
    assert got["t_eval"] == want
    assert program("euler", 3, t_start=-1.0)["t"][0] == 1.0  # t_start <= 0: sde.T


# ---------------------------------------------------------------- 2. the order each method shows
@pytest.mark.parametrize("method", METHODS)
def test_observed_order(program, method):
    # the restatement (the reference, not the code under test) against the closed form, M = 64 -> 128 on the uniform grid
    M = 64
    errs = []
    for m in (M, 2 * M):
        ts = grid("uniform", m)
        y = ref_solve(method, ts)[0][-1]
        errs.append(np.max(np.abs(y - exact(EPS))))
        got = np.array(program(method, m)["y"]).reshape(m, 3)[-1]
        assert np.max(np.abs(got - y) / np.abs(y)) <= 1e-13  # ... and the plan's walk shows the same errors
    order = np.log2(errs[0] / errs[1])
    print(f"{method}: error {errs[0]:.3g} at M = {M}, {errs[1]:.3g} at {2 * M}: observed order {order:.3f}")
    assert abs(order - ORDER[method]) <= 0.25


# ---------------------------------------------------------------- 3. refusals of the plan, by message
def test_plan_refusals(program):
    def refused(match, *a, **k):
        got = program(*a, **k)
        assert "refused" in got and got["refused"].startswith("ode_fixed_main: ") and match in got["refused"], got

    refused("method must be DIFFSEP_ODEF_EULER, HEUN, MIDPOINT, RK4 or AB2", 7, 4)
    refused("steps must be >= 1", "heun", 0)
    refused("steps x stages must be <= 16384", "rk4", 4097)
    assert program("rk4", 4096)["n_evals"] == 16384 and program("ab2", 8192)["n_evals"] == 8193
    refused("steps x stages must be <= 16384", "euler", 16385)
    refused("the time grid must be strictly descending inside (0, 1]", "heun", 2, ts=[1.0, 0.5, 0.5])
    refused("the time grid must be strictly descending inside (0, 1]", "heun", 2, ts=[1.0, 0.4, 0.5])
    refused("the time grid must be strictly descending inside (0, 1]", "heun", 2, ts=[1.5, 0.5, 0.1])
    refused("the time grid must be strictly descending inside (0, 1]", "heun", 2, ts=[1.0, 0.5, 0.0])
    refused("the time grid must be strictly descending inside (0, 1]", "heun", 2, t_start=1.5)
    refused("eps must be in (0, 1)", "heun", 2, eps=0.0)
    refused("eps must be in (0, 1)", "heun", 2, eps=1.0)
    refused("t_start must be above eps", "heun", 2, t_start=0.03)
    refused("t_start must be above eps", "heun", 2, t_start=0.01)
    refused("the denoise step needs N >= 1", "heun", 2, denoise=1, N=0)
    assert "refused" not in program("heun", 2, denoise=0, N=0)
    for m in ("euler", "rk4"):
        refused("err_out needs a method with an embedded Euler step (HEUN, MIDPOINT, AB2), not EULER or RK4", m, 2, want_err=1)
    for m in ("heun", "midpoint", "ab2"):
        assert "refused" not in program(m, 2, want_err=1)


# ---------------------------------------------------------------- 4. sanitizer run of the host code
def test_program_runs_clean_under_asan_and_ubsan(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (the ROCm toolchain's clang++ or g++)")
    exe = str(tmp_path / "ode_fixed_main_san")
    # (the sanitizer runtimes linked statically — clang's default — so that the program stands alone)
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx).startswith("g++") else []
    built = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static,
                            "-ffp-contract=off", "-Wall", os.path.join(HERE, "ode_fixed_main.cpp"), "-o", exe],
                           capture_output=True, text=True)
    if built.returncode != 0 and "sanitizer" in built.stderr.lower() + built.stdout.lower():
        pytest.skip("this compiler has no AddressSanitizer / UBSan runtime")
    assert built.returncode == 0, built.stderr
    run = _runner(exe)  # (check=True: a sanitizer report ends the program with a non-zero status)
    for method in METHODS:
        assert run(method, 9)["n_evals"] == EVALS[method](9)
        assert run(method, 5, ts=grid("log", 5))["steps"] == 5
    assert run("rk4", 4096)["n_evals"] == 16384
    assert "refused" in run("heun", 2, ts=[1.0, 0.4, 0.5]) and "refused" in run("euler", 2, want_err=1)


# ---------------------------------------------------------------- 5. the Python layers with stand-in engines
def test_binding_constants_and_counts():
    assert [_lib.ODEF_METHODS[m] for m in METHODS] == [0, 1, 2, 3, 4]
    assert "diffsep_ode_sample_fixed" in _lib.EXPORTS
    for m in METHODS:
        assert _lib.odef_nfe(m, 30) == EVALS[m](30)
    assert set(_lib.ODEF_ERR_METHODS) == {"heun", "midpoint", "ab2"}


def test_schedules_build_the_grid_between_t_start_and_eps():
    lin = sdes.ode_fixed_timesteps(8, 0.03, "linear", 0.5)
    assert lin.dtype == np.float64 and lin.shape == (9,) and lin[0] == 0.5 and lin[-1] == 0.03
    assert np.allclose(lin, np.linspace(0.5, 0.03, 9), rtol=1e-14, atol=0)
    log = sdes.ode_fixed_timesteps(8, 0.03, "log", 1.0)
    assert log[0] == 1.0 and log[-1] == 0.03 and np.all(np.diff(log) < 0)
    assert np.allclose(log, np.logspace(0, np.log10(0.03), 9), rtol=1e-13, atol=0)
    rev = sdes.ode_fixed_timesteps(8, 0.03, "revlog", 1.0)
    assert np.allclose(rev, np.logspace(np.log10(0.03), 0, 9)[::-1], rtol=1e-13, atol=0)
    with pytest.raises(NotImplementedError, match="Schedule 'cosine'"):
        sdes.ode_fixed_timesteps(8, 0.03, "cosine")


class _FakeEngine:
    def __init__(self):
        self.calls = []

    def ode_sample_fixed(self, y, sde, **kw):
        self.calls.append(kw)
        return torch.zeros(y.shape[0], 2, y.shape[2]), dict(nfe=_lib.odef_nfe(kw["method"], kw["steps"]), method=kw["method"],
                                                            steps=kw["steps"])


class _FakeModel:
    def __init__(self):
        self.eng = _FakeEngine()

    def engine(self):
        return self.eng


def test_factory_passes_the_request_on_and_refuses_what_it_cannot_run():
    sde = sdes.MixSDE(ndim=2, d_lambda=2.0, sigma_min=0.05, sigma_max=0.5, N=6)
    y = torch.zeros(1, 1, 100)
    model = _FakeModel()
    x, nfe = sdes.get_ode_fixed_sampler(sde, model, y, seed=3)()
    kw = model.eng.calls[-1]
    assert nfe == 12 and kw["method"] == "heun" and kw["steps"] == 6 and kw["N"] == 6 and kw["timesteps"] is None
    assert kw["seed"] == 3 and kw["t_start"] is None and kw["tail"] is None and kw["want_err"] is False
    s = sdes.get_ode_fixed_sampler(sde, model, y, method="ab2", steps=9, schedule="log", t_start=0.5, x_init=y, want_err=True)
    assert s()[1] == 10 and s.info["steps"] == 9
    kw = model.eng.calls[-1]
    assert np.array_equal(kw["timesteps"], sdes.ode_fixed_timesteps(9, 0.03, "log", 0.5)) and kw["x_init"] is y and kw["want_err"]
    with pytest.raises(ValueError, match="get_ode_fixed_sampler: score_fn has no engine"):
        sdes.get_ode_fixed_sampler(sde, lambda *a: None, y)
    with pytest.raises(NotImplementedError, match="get_ode_fixed_sampler: method 'RK45'"):
        sdes.get_ode_fixed_sampler(sde, model, y, method="RK45")
    with pytest.raises(TypeError, match="rtol"):
        sdes.get_ode_fixed_sampler(sde, model, y, rtol=1e-5)
    with pytest.raises(ValueError, match="schedule= and timesteps= are alternatives"):
        sdes.get_ode_fixed_sampler(sde, model, y, schedule="log", timesteps=[1.0, 0.03])


# ---------------------------------------------------------------- 6. the CLIs' refusals, before an engine is needed
def _sep_refused(argv, match, monkeypatch):
    monkeypatch.setattr(sep_cli, "get_model", lambda args: pytest.fail("the request reached get_model"))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: pytest.fail("the request reached the GPU check"))
    with pytest.raises(SystemExit, match=match):
        sep_cli.main(argv)


def _eval_refused(argv, match, monkeypatch):
    monkeypatch.setattr(eval_cli, "DiffSepModel", lambda *a, **k: pytest.fail("the request reached the model"))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: pytest.fail("the request reached the GPU check"))
    with pytest.raises(SystemExit, match=match):
        eval_cli.main(argv)


def test_separate_refusals(tmp_path, monkeypatch):
    ind = tmp_path / "in"
    ind.mkdir()
    base = [str(ind), str(tmp_path / "out"), "--synthetic-weights", "16", "--sampler", "ode-fixed"]
    _sep_refused(base + ["--chunk", "4"], "--chunk with --sampler ode-fixed is not supported", monkeypatch)
    _sep_refused(base + ["--draws", "2", "--batch", "2"], "--draws with --sampler ode-fixed is not supported", monkeypatch)
    _sep_refused(base + ["--ode-steps", "0"], "--ode-steps 0: at least one step", monkeypatch)
    plain = base[:-2]
    _sep_refused(plain + ["--ode-method", "heun"], "--ode-method goes with --sampler ode-fixed", monkeypatch)
    _sep_refused(plain + ["--sampler", "ode", "--ode-steps", "4"], "--ode-steps goes with --sampler ode-fixed", monkeypatch)
    with pytest.raises(SystemExit):  # argparse: an unknown method
        sep_cli.main(base + ["--ode-method", "rk45"])


def test_evaluate_refusals(tmp_path, monkeypatch):
    base = ["--synthetic", "2", "--synthetic-weights", "16", "-o", str(tmp_path), "--sampler", "ode-fixed"]
    _eval_refused(base + ["--fig"], "--fig with --sampler ode-fixed is not supported", monkeypatch)
    _eval_refused(base + ["--trajectory"], "--trajectory with --sampler ode-fixed is not supported", monkeypatch)
    _eval_refused(base + ["--draws", "2"], "--draws with --sampler ode-fixed is not supported", monkeypatch)
    _eval_refused(base + ["--ode-err", "--ode-method", "rk4"], "--ode-err with --ode-method rk4", monkeypatch)
    _eval_refused(base + ["--ode-err", "--ode-method", "euler"], "--ode-err with --ode-method euler", monkeypatch)
    _eval_refused(base + ["--ode-steps", "0"], "--ode-steps 0: at least one step", monkeypatch)
    plain = base[:-2]
    _eval_refused(plain + ["--ode-err"], "--ode-err goes with --sampler ode-fixed", monkeypatch)
    _eval_refused(plain + ["--sampler", "ode", "--ode-method", "heun"], "--ode-method goes with --sampler ode-fixed", monkeypatch)
