"""The probability-flow ODE sampler's host surface (no GPU): the RK tableaux the device solver uses against scipy's,
and sdes.get_ode_sampler's reference signature and refusals (reference sdes/__init__.py:193-278)."""
import inspect

import numpy as np
import pytest
import torch
from scipy.integrate import RK23, RK45

from diffsep_amd import _lib, sdes
from diffsep_amd.sdes import MixSDE


@pytest.mark.parametrize("method, cls", [("RK45", RK45), ("RK23", RK23)])
def test_tableau_equals_scipy(method, cls):
    A, B, C, E, ns, eo = _lib.ode_tableau(method)
    assert ns == cls.n_stages and eo == cls.error_estimator_order
    # (scipy stores RK45's A as 6 x 5: the last column of an explicit tableau is zero; ours is square)
    k = cls.A.shape[1]
    assert A.shape == (ns, ns) and (A[:, :k] == cls.A).all() and (A[:, k:] == 0).all()
    assert (B == cls.B).all() and (C == cls.C).all() and (E == cls.E).all()


def test_tableau_refuses_unknown_method():
    l = _lib.lib()
    assert l.diffsep_ode_tableau(7, None, None, None, None, None, None) != 0
    assert b"RK45" in l.diffsep_last_error()


def test_get_ode_sampler_has_the_reference_signature():
    assert "get_ode_sampler" in sdes.__all__
    sig = inspect.signature(sdes.get_ode_sampler)
    want = [("sde", inspect.Parameter.empty), ("score_fn", inspect.Parameter.empty), ("y", inspect.Parameter.empty),
            ("inverse_scaler", None), ("denoise", True), ("rtol", 1e-5), ("atol", 1e-5), ("method", "RK45"),
            ("eps", 3e-2), ("device", "cuda")]
    params = list(sig.parameters.values())
    assert [(p.name, p.default) for p in params[:-1]] == want
    assert params[-1].kind is inspect.Parameter.VAR_KEYWORD


class _Engineless:
    def __call__(self, x, t, mix):
        return x


def test_get_ode_sampler_refusals():
    sde = MixSDE(2, 2.0, 0.05, 0.5, N=30)
    y = torch.zeros(1, 1, 400)
    with pytest.raises(NotImplementedError):
        sdes.get_ode_sampler(sde, _Engineless(), y, method="DOP853")
    with pytest.raises(TypeError):
        sdes.get_ode_sampler(sde, _Engineless(), y, t_eval=np.linspace(1, 0.03, 5))
    with pytest.raises(ValueError, match="no engine"):  # no host fallback
        sdes.get_ode_sampler(sde, _Engineless(), y)
    with pytest.raises(ValueError, match="no engine"):
        sdes.get_ode_sampler(sde, lambda x, t, mix: x, y, first_step=1e-3, max_step=0.1, max_nfe=10, seed=1)


def test_ode_config_struct_mirrors_the_header():
    import ctypes as C
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                            "diffsep_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    ctype = {"int32_t": C.c_int32, "double": C.c_double}
    for name, cls in (("diffsep_ode_config", _lib.OdeConfig), ("diffsep_ode_info", _lib.OdeInfo)):
        body = re.search(r"typedef struct \{([^}]*)\}\s*" + name + ";", hdr).group(1)
        fields = []
        for decl in [d.strip() for d in body.split(";") if d.strip()]:
            typ, names = decl.split(None, 1)
            fields += [(n.strip(), ctype[typ]) for n in names.split(",")]
        assert [(n, C.sizeof(t)) for n, t in cls._fields_] == [(n, C.sizeof(t)) for n, t in fields], name
