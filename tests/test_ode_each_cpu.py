"""The per-utterance ODE sampler's host surface (no GPU): the three new C symbols in the header and in both built
libraries, the struct that carries lengths / seeds, and sdes.get_ode_sampler's refusals with the new keyword arguments."""
import ctypes as C
import os
import re

import pytest
import torch

from diffsep_amd import _lib, sdes
from diffsep_amd.sdes import MixSDE

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "diffsep_hip.h")
NEW = ("diffsep_ode_sample_each", "diffsep_ode_stage_update_each", "diffsep_ode_error_norm_each")


def test_header_declares_and_libraries_export_the_new_symbols():
    text = open(HEADER).read()
    for name in NEW:
        assert re.search(r"\bint32_t\s+" + name + r"\s*\(", text), name
        assert name in _lib.EXPORTS
        for kind in ("bf16", "f16"):
            assert getattr(_lib.lib(kind), name) is not None, (kind, name)
    assert re.search(r"const int64_t\*\s*lengths_host;\s*const uint64_t\*\s*seeds_host;\s*}\s*diffsep_ode_ext;", text)


def test_ode_ext_struct_mirrors_the_header():
    assert [n for n, _ in _lib.OdeExt._fields_] == ["lengths_host", "seeds_host"]
    assert C.sizeof(_lib.OdeExt) == 2 * C.sizeof(C.c_void_p)


def test_unit_entries_refuse_null_tables_without_a_gpu():
    l = _lib.lib()
    sc = _lib.SdeConfig(_lib.SDE_MIX, 2, 2.0, 0.05, 0.5, 0)
    assert l.diffsep_ode_stage_update_each(C.byref(sc), None, None, None, None, None, None, None, 0, -1, None, None, None,
                                           None, None, 1, 2, 8, None) != 0
    assert b"null table" in l.diffsep_last_error()


class _Engineless:
    def __call__(self, x, t, mix):
        return x


def test_get_ode_sampler_refusals_with_the_new_keywords():
    sde = MixSDE(2, 2.0, 0.05, 0.5, N=30)
    y = torch.zeros(2, 1, 400)
    for kw in (dict(lengths=[400, 390]), dict(seeds=[1, 2]), dict(per_utterance=True),
               dict(lengths=[400, 390], seeds=[1, 2], max_nfe=10)):
        with pytest.raises(ValueError, match="no engine"):  # no host fallback, as without them
            sdes.get_ode_sampler(sde, _Engineless(), y, **kw)
    with pytest.raises(TypeError):
        sdes.get_ode_sampler(sde, _Engineless(), y, lengths=[400, 390], length=[400, 390])
    with pytest.raises(TypeError):
        sdes.get_ode_sampler(sde, _Engineless(), y, per_batch=True)
