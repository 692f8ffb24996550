"""What every sampler entry refuses of the batch extensions (lengths, seeds, the other engine), message by message: the one
table the shared validation (csrc/sampler.hip: check_batch_ext) is held to.  Every refusal comes before anything is enqueued
or allocated, so the engine computes afterwards bit for bit what it computed before."""
import re

import pytest
import torch

from diffsep_amd import _lib, ops, synth
from diffsep_amd.engine import Engine, pack_state_dict, param_table

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

NF, S, T = 16, 2, 4000
MIX = dict(kind=_lib.SDE_MIX, ndim=2, d_lambda=2.0, sigma_min=0.05, sigma_max=0.5)

# entry -> (the name in its messages, the call with the extension arguments left open)
ENTRIES = {
    "pc_sample": ("pc_sample", lambda eng, mixn, **kw: eng.pc_sample(mixn, MIX, N=1, corrector_steps=1, **kw)),
    "ode_sample_each": ("ode_sample_each", lambda eng, mixn, **kw: eng.ode_sample_each(mixn, MIX, **kw)),
    "ode_sample_fixed(heun)": ("ode_sample_fixed", lambda eng, mixn, **kw: eng.ode_sample_fixed(mixn, MIX, method="heun", steps=2, **kw)),
    "ode_sample_fixed(ddim)": ("ode_sample_expint", lambda eng, mixn, **kw: eng.ode_sample_fixed(mixn, MIX, method="ddim", steps=2, **kw)),
}
SEEDS_WITH_NOISE = {  # (ode_sample_each has its own wording: it takes seeds with neither noise nor x_init)
    "pc_sample": "pc_sample: per-utterance seeds are for device noise (noise == NULL)",
    "ode_sample_each": "ode_sample_each: per-utterance seeds are for device noise (noise == NULL, x_init == NULL)",
    "ode_sample_fixed(heun)": "ode_sample_fixed: per-utterance seeds are for device noise (noise == NULL)",
    "ode_sample_fixed(ddim)": "ode_sample_expint: per-utterance seeds are for device noise (noise == NULL)",
}


def make_engine(spec_factor):
    cfg = _lib.model_config(nf=NF, num_sources=S, spec_factor=spec_factor)
    sd = synth.synth_state_dict([(n, s) for n, s, _ in param_table(cfg)], 7)
    return Engine(cfg, pack_state_dict(cfg, sd))


def refused(expected, fn, *a, **kw):
    """the call is refused with exactly `expected` after the library's "<source file>:<line>: " """
    with pytest.raises(_lib.DiffsepError) as ei:
        fn(*a, **kw)
    m = re.fullmatch(r"\S+:\d+: (.*)", str(ei.value), re.S)
    assert m and m.group(1) == expected, str(ei.value)


def test_extension_refusals_by_message_and_the_engine_untouched():
    eng, other = make_engine(0.33), make_engine(0.5)  # (spec_factor is a field of diffsep_model_config: another architecture)
    mixn, _, _ = ops.normalize_batch(torch.from_numpy(synth.synth_batch(2, T=T)[0]).cuda())
    before, info = eng.ode_sample_fixed(mixn, MIX, method="heun", steps=2, seed=3)
    long_mix = torch.zeros(2, 1, 9000, device="cuda")  # 9000 and 3000 samples have different padded frame counts
    assert eng.padded_frames(9000) != eng.padded_frames(3000)
    for key, (who, fn) in ENTRIES.items():
        refused(f"{who}: utterance length outside [1, T]", fn, eng, mixn, lengths=[T, 0])
        refused(f"{who}: utterance length outside [1, T]", fn, eng, mixn, lengths=[T, T + 1])
        refused(f"{who}: every utterance of a mixed-length batch must have the padded frame count of T", fn, eng, long_mix,
                lengths=[9000, 3000])
        draws = (3,) if key == "pc_sample" else ()  # pc_sample: the prior's draw, the corrector's, the predictor's
        refused(SEEDS_WITH_NOISE[key], fn, eng, mixn, seeds=[1, 2], noise=torch.zeros(*draws, 2, S, T, device="cuda"))
        if key == "ode_sample_each":  # (no other engine)
            continue
        refused(f"{who}: the tail engine must be a different engine", fn, eng, mixn, tail=eng, head_steps=1)
        refused(f"{who}: the tail engine must have the same architecture", fn, eng, mixn, tail=other, head_steps=1)
        refused(f"{who}: the tail engine must have the same architecture", fn, eng, mixn, tail=other, tail_steps=1)
    after, info2 = eng.ode_sample_fixed(mixn, MIX, method="heun", steps=2, seed=3)
    assert torch.equal(before, after) and info == info2
