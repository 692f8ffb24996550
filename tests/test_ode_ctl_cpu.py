"""The ODE sampler's step controller (csrc/ode_host.h: OdePlan, OdeCtl, the tableaux) against scipy.integrate.solve_ivp on
the CPU: tests/ode_ctl_main.cpp, a stand-alone program that includes nothing but that header, integrates a small float64
system with it; scipy integrates the same system.  The controller's decisions — step counts, accepted times — must be
scipy's; the arithmetic agrees to rounding (scipy's BLAS dot sums in another order, so bit identity is not available: a
Python transcription of the controller gave grid deviations <= 2.9e-11 relative and final states within 1.8e-11 on
these four cases; the bounds below are those figures with a margin for that ordering)."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
import scipy.integrate

HERE = os.path.dirname(os.path.abspath(__file__))
M = np.array([[-1.3, 2, 0], [-2, -0.7, 0.5], [0.1, -0.4, -2.1]])
Y0 = np.array([1.0, -0.5, 0.25])
T0, T_END = 1.0, 0.03
NS = {"RK45": 6, "RK23": 3}
CODE = {"RK45": 0, "RK23": 1}


def fun(t, y):
    i = np.arange(3)
    return M @ y + 0.1 * (i + 1) * np.sin(3 * t) + 5.0 * (i + 1) * np.tanh(40 * (t - 0.5))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cxx = next((c for c in (os.path.join(rocm, "llvm", "bin", "clang++"), shutil.which("g++"), shutil.which("clang++"))
                if c and os.path.exists(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler (the ROCm toolchain's clang++ or g++)")
    exe = str(tmp_path_factory.mktemp("ode_ctl") / "ode_ctl_main")
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", os.path.join(HERE, "ode_ctl_main.cpp"),
                           "-o", exe])

    def run(method, tol, first_step=0.0, max_step=0.0, max_nfe=0):
        out = subprocess.run([exe, str(CODE[method]), repr(tol), repr(first_step), repr(max_step), str(max_nfe)],
                             check=True, capture_output=True, text=True).stdout
        return json.loads(out)
    return run


@pytest.mark.parametrize("method", ["RK45", "RK23"])
@pytest.mark.parametrize("tol", [1e-3, 1e-5])
def test_controller_takes_scipys_steps(program, method, tol):
    got = program(method, tol)
    ref = scipy.integrate.solve_ivp(fun, (T0, T_END), Y0, method=method, rtol=tol, atol=tol)
    ns = NS[method]
    ref_acc = len(ref.t) - 1
    ref_rej = (ref.nfev - 2) // ns - ref_acc  # nfev = f0 + select_initial_step's f1 + ns per attempt
    t = np.array(got["t"])
    dev_t = np.max(np.abs(t - ref.t[1:]) / np.abs(ref.t[1:])) if len(t) == ref_acc else float("nan")
    dev_y = np.max(np.abs(np.array(got["y"]) - ref.y[:, -1]))
    print(f"{method} tol {tol}: nfev {got['nfev']} / {ref.nfev}, accepted {got['accepted']} / {ref_acc}, rejected "
          f"{got['rejected']} / {ref_rej}, grid deviation {dev_t:.3g} relative, final state {dev_y:.3g}")
    assert ref.status == 0 and (ref.nfev - 2) % ns == 0 and ref_rej >= 1  # (a case without a rejected step tests half the rules)
    assert got["status"] == 0 and got["nfev"] == ref.nfev
    assert got["accepted"] == ref_acc == len(t) and got["rejected"] == ref_rej
    assert t[-1] == T_END
    assert dev_t <= 1e-9
    assert dev_y <= 1e-10


def test_first_step_skips_the_initial_step_evaluation(program):
    got = program("RK45", 1e-3, first_step=0.01)
    assert got["status"] == 0 and (got["nfev"] - 1) % 6 == 0
    assert got["nfev"] == 1 + 6 * (got["accepted"] + got["rejected"])
    assert abs((T0 - got["t"][0]) - 0.01) <= 4 * np.finfo(float).eps  # (tanh(40 (t - 0.5)) is flat near t = 1: the first attempt is accepted)


def test_max_step_bounds_every_accepted_step(program):
    got = program("RK45", 1e-3, max_step=0.05)
    steps = -np.diff([T0] + got["t"])
    assert got["status"] == 0 and got["t"][-1] == T_END
    assert steps.max() <= 0.05 + 4 * np.finfo(float).eps and steps.min() > 0
    assert got["accepted"] >= (T0 - T_END) / 0.05


def test_max_nfe_stops_before_the_attempt_that_would_exceed_it(program):
    free = program("RK45", 1e-3)
    got = program("RK45", 1e-3, max_nfe=free["nfev"] - 1)
    assert got["status"] == 1 and got["nfev"] <= free["nfev"] - 1
    assert got["nfev"] == free["nfev"] - 6 and got["t"] == free["t"][:len(got["t"])] and got["t"][-1] > T_END


def test_first_step_beyond_the_interval_is_refused(program):
    got = program("RK45", 1e-3, first_step=0.98)  # the interval is 0.97
    assert "first_step exceeds the interval" in got["refused"] and got["refused"].startswith("ode_ctl_main: ")
    assert "refused" not in program("RK45", 1e-3, first_step=0.97)
