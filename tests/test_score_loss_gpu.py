"""The score-matching loss on the MI355X (csrc/score_loss.hip): the two kernels against the reference fixture and the numpy
restatement, determinism, the in-kernel Philox draws, the dense inverse, the fused call on the fp32 engine end to end, the
Python mirror of the reference's loss methods, mixed-length batches and the evaluate flag."""
import json

import numpy as np
import pytest
import torch

import score_loss_cases as SC
from diffsep_amd import _lib, ops, synth
from diffsep_amd import evaluate as eval_cli
from diffsep_amd.engine import Engine, pack_state_dict, param_table
from diffsep_amd.pl_model import DiffSepModel, default_config
from test_score_loss_cpu import HACK_CASES, case_arrays

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
_cache = {}


@pytest.fixture(scope="module")
def fx():
    return SC.load()


def dev(a, dtype=torch.float32):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def engine(S, dtype=_lib.F32):
    if (S, dtype) not in _cache:
        cfg = _lib.model_config(nf=SC.NF, num_sources=S, dtype=dtype)
        sd = synth.synth_state_dict([(n, s) for n, s, _ in param_table(cfg)], 7)
        _cache[(S, dtype)] = Engine(cfg, pack_state_dict(cfg, sd))
    return _cache[(S, dtype)]


def setup(sde_tag):
    sde, S = SC.SDES[sde_tag], SC.SDES[sde_tag]["ndim"]
    mix, tgt = SC.inputs(S)
    smix = ops.sde_sigma_mix(dev(mix), sde["avg_len"]) if sde["kind"] == 1 else None
    return sde, S, mix, tgt, SC.noise("z", S), smix


@pytest.mark.parametrize("sde_tag, hack", HACK_CASES)
def test_perturb_matches_the_reference(fx, sde_tag, hack):
    sde, S, mix, tgt, z, smix = setup(sde_tag)
    tag, _ = case_arrays(fx, sde_tag, hack)
    x_t, zr = ops.sde_perturb(sde, dev(tgt), dev(mix), dev(fx[f"{tag}_time"]), z=dev(z), sigma_mix=smix,
                              beta=dev(fx[f"{tag}_beta"]), redefine_z=hack in (1, 3, 4))
    e_x = SC.rel_rms(x_t[..., :SC.HEAD].cpu(), fx[f"{tag}_xt_head"])
    e_z = SC.rel_rms(zr[..., :SC.HEAD].cpu(), fx[f"{tag}_z_head"])
    print(tag, "x_t", e_x, "z'", e_z)
    assert e_x <= 1e-6 and e_z <= 1e-6


@pytest.mark.parametrize("hack", [0, 1, 2, 4])
def test_perturb_priormix_modes_match_the_restatement(fx, hack):
    # (the reference fixture holds PriorMixSDE for init_hack 3; the other modes against the float64 restatement, which the CPU
    # suite ties to the reference for every mode)
    sde, S, mix, tgt, z, smix = setup("p2")
    t, beta = fx[f"m2_h{hack}_time"], fx[f"m2_h{hack}_beta"]
    x_t, zr = ops.sde_perturb(sde, dev(tgt), dev(mix), dev(t), z=dev(z), sigma_mix=smix, beta=dev(beta), redefine_z=hack in (1, 4))
    rx, rz = SC.perturb(sde, tgt, mix, t, z, beta=beta, redefine=hack in (1, 4), smix=smix.cpu().numpy())
    assert SC.rel_rms(x_t.cpu(), rx) <= 1e-6 and SC.rel_rms(zr.cpu(), rz) <= 1e-6


@pytest.mark.parametrize("tag, pit", [("m2_h3", None), ("p2_h3", None), ("m2_pit1", "true_mix"), ("m3_pit2", "mean0")])
def test_loss_reduce_matches_the_restatement_and_is_deterministic(fx, tag, pit):
    """out against the restatement run on the kernel's own fp32 per-sample arithmetic (float32 operations in the kernel's order
    on the kernel's coefficients; the squares and sums in float64): 1e-12 relative.  Then bit-identity across a second run,
    four B = 1 calls and a side stream."""
    sde_tag = tag[:2]
    sde, S, mix, tgt, z, smix = setup(sde_tag)
    t = fx[f"{tag}_time"]
    if pit is None:
        pred = case_arrays(fx, sde_tag, 3)[1]
        zr = SC.perturb(sde, tgt, mix, t, z, beta=fx[f"{tag}_beta"], redefine=True, smix=None if smix is None else smix.cpu().numpy(),
                        dtype=np.float32)[1]
    else:
        pred, zr = fx[f"{tag}_pred"], z
        if pit == "mean0":
            tgt = np.take_along_axis(tgt, fx[f"{tag}_perm"][..., None], axis=1)
    args = dict(x0=dev(tgt), mix=dev(mix), sigma_mix=smix, pit=pit)
    out, best, arg, coef = ops.score_loss_reduce(sde, dev(pred), dev(zr), dev(t), want_coef=True, **args)
    ref = SC.reduce(sde, pred, zr, t, x0=tgt, mix=mix, smix=None if smix is None else smix.cpu().numpy(),
                    pit=ops.PIT_MODES[pit], dtype=np.float32, coef=coef.cpu().numpy())
    rel = np.abs(out.cpu().numpy() - ref) / ref
    print(tag, "max rel", rel.max())
    assert np.all(rel <= 1e-12)
    # the kernel's coefficients themselves against the float64 ones: powf / expf / sqrtf good to 2 ulp each, amplified by the
    # cancellation in srp - 1 and srp - exp(-2 lambda t) at small t
    c64, ulp = SC.coefs(sde, t), 2.0 ** -23
    srp = (sde["sigma_max"] / sde["sigma_min"]) ** (2.0 * t.astype(np.float64))
    amp = srp / np.minimum(srp - 1.0, srp - np.exp(-2.0 * sde["d_lambda"] * t.astype(np.float64)))
    crel = np.abs(coef.cpu().numpy().astype(np.float64) - c64) / c64
    print(tag, "coef rel", crel.max(), "bound", ((2 * amp + 2) * ulp).max())
    assert np.all(crel <= ((2 * amp + 2) * ulp)[:, None])
    assert torch.equal(best, out.min(dim=1).values) and torch.equal(arg.long(), out.argmin(dim=1))
    again = ops.score_loss_reduce(sde, dev(pred), dev(zr), dev(t), **args)[0]
    assert torch.equal(again, out)
    for b in range(SC.B):
        one = ops.score_loss_reduce(sde, dev(pred[b:b + 1]), dev(zr[b:b + 1]), dev(t[b:b + 1]), x0=dev(tgt[b:b + 1]),
                                    mix=dev(mix[b:b + 1]), sigma_mix=None if smix is None else smix[b:b + 1].contiguous(), pit=pit)[0]
        assert torch.equal(one[0], out[b])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = ops.score_loss_reduce(sde, dev(pred), dev(zr), dev(t), **args)[0]
    side.synchronize()
    assert torch.equal(other, out)


@pytest.mark.parametrize("T", [4000, 3999])
def test_in_kernel_philox_draws_are_the_bits_of_randn(T):
    sde, S = SC.SDES["m2"], 2
    mix, tgt = (torch.from_numpy(v).cuda() for v in synth.synth_batch(3, T=T))
    t = torch.tensor([0.03, 0.5, 1.0]).cuda()
    zi = ops.randn(3 * S * T, 1234, 7).view(3, S, T)
    a = ops.sde_perturb(sde, tgt, mix, t, z=zi, seed=0)
    b = ops.sde_perturb(sde, tgt, mix, t, z=None, seed=1234, stream_id=7)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(b[1], zi)


@pytest.mark.parametrize("sde_tag", ["m2", "m3", "p2"])
def test_mult_std_inv_inverts_mult_std_and_agrees_with_the_closed_form(sde_tag):
    sde, S, mix, tgt, z, smix = setup(sde_tag)
    t = dev(np.array([0.03, 0.2, 0.53, 1.0]))
    std = ops.sde_std(sde, t, S, T=SC.T, sigma_mix=smix)
    x = dev(z)
    y = ops.sde_mult_std_inv(std, x)
    back = ops.sde_mult_std(std, y)
    assert SC.rel_rms(back.cpu(), z) <= 2e-6  # two roundings of a well-conditioned S x S system (cond <= 1.1 here)
    c = SC.coefs(sde, t.cpu().numpy())
    sm = 1.0 if smix is None else smix.cpu().numpy().astype(np.float64)[:, None, :]
    closed = SC.linv(z.astype(np.float64), c[:, 1, None, None] * sm, c[:, 2, None, None] * sm, S, np.float64)
    assert SC.rel_rms(y.cpu(), closed) <= 2e-6


def cs_bound(sde, pred, zr, t, smix, n):
    """|d loss_b| <= (2 |r_b| |L d_b| + |L d_b|^2) / n with |L d_b| <= sqrt(max(ev1, ev2)) max(sigma_mix) 1e-4 |score_b|"""
    c = SC.coefs(sde, t)
    sm = None if smix is None else smix.cpu().numpy()
    S = pred.shape[1]
    mg = pred.astype(np.float64).mean(axis=1, keepdims=True)
    scale = 1.0 if sm is None else sm.astype(np.float64)[:, None, :]
    r = (c[:, 1, None, None] * mg + c[:, 2, None, None] * (pred - mg)) * scale + zr
    nr = np.sqrt((r ** 2).sum(axis=(1, 2)))
    ld = np.maximum(c[:, 1], c[:, 2]) * (1.0 if sm is None else sm.max()) * 1e-4 * np.sqrt((pred.astype(np.float64) ** 2).sum(axis=(1, 2)))
    return (2 * nr * ld + ld ** 2) / n


def pit_bounds(fx, tag, pit, sde, S, mix, tgt, z, t):
    """(reference per-permutation losses [B,P], bound on each): the Cauchy-Schwarz bound of the 1e-4 score bar on r_p = L score
    + z_p, plus what the reference's own per-permutation x_t rounding moves (measured by the fixture generator) and the 1e-6 of
    the plain-loss check"""
    ref = fx[f"{tag}_perm_losses"].astype(np.float64)
    rounding = (float(fx[f"{tag}_xt_rounding_rel"][0]) + 1e-6) * ref
    c = SC.coefs(sde, t)
    mx = tgt.astype(np.float64).mean(axis=1, keepdims=True)
    mean0 = mx + c[:, 0, None, None] * (tgt - mx)
    bounds = np.zeros_like(ref)
    for p, perm in enumerate(SC.perms(S)):
        d = (mix.astype(np.float64) / S if pit == "true_mix" else mean0) - mean0[:, list(perm), :]
        zp = z + SC.linv(d, c[:, 1, None, None], c[:, 2, None, None], S, np.float64)
        bounds[:, p] = cs_bound(sde, fx[f"{tag}_pred"], zp, t, None, S * SC.T) + rounding[:, p]
    return ref, bounds


@pytest.mark.parametrize("sde_tag, hack", [("m2", 0), ("m2", 3), ("m2", 4), ("p2", 3)])
def test_fused_loss_end_to_end_on_the_fp32_engine(fx, sde_tag, hack):
    sde, S, mix, tgt, z, smix = setup(sde_tag)
    tag, pred = case_arrays(fx, sde_tag, hack)
    t, beta = fx[f"{tag}_time"], fx[f"{tag}_beta"]
    out, _, _, x_t, score = ops.score_loss(engine(S), sde, dev(mix), dev(tgt), dev(t), beta=dev(beta), z=dev(z),
                                           redefine_z=hack in (1, 3, 4), debug=True)
    rx, rz = SC.perturb(sde, tgt, mix, t, z, beta=beta, redefine=hack in (1, 3, 4), smix=None if smix is None else smix.cpu().numpy())
    e_x, e_s = SC.rel_rms(x_t.cpu(), rx), SC.rel_rms(score.cpu(), pred)
    print(tag, "x_t", e_x, "score", e_s)
    assert e_x <= 1e-4 and e_s <= 1e-4
    bound = cs_bound(sde, pred, rz, t, smix, S * SC.T) + 1e-6 * fx[f"{tag}_loss"]
    err = np.abs(out[:, 0].cpu().numpy() - fx[f"{tag}_loss"])
    print(tag, "loss err", err, "bound", bound)
    assert np.all(err <= bound)


@pytest.mark.parametrize("tag, pit", [("m2_pit1", "true_mix"), ("m3_pit2", "mean0")])
def test_fused_pit_loss_end_to_end(fx, tag, pit):
    sde_tag = tag[:2]
    sde, S, mix, tgt, z, smix = setup(sde_tag)
    t = fx[f"{tag}_time"]
    if pit == "mean0":
        tgt = np.take_along_axis(tgt, fx[f"{tag}_perm"][..., None], axis=1)
    beta = np.ones(SC.B) if pit == "true_mix" else None
    out, best, arg, x_t, score = ops.score_loss(engine(S), sde, dev(mix), dev(tgt), dev(t), beta=dev(beta), z=dev(z), pit=pit,
                                                debug=True)
    assert SC.rel_rms(score.cpu(), fx[f"{tag}_pred"]) <= 1e-4
    ref, bounds = pit_bounds(fx, tag, pit, sde, S, mix, tgt, z, t)
    err = np.abs(out.cpu().numpy() - ref)
    print(tag, "err", err.max(axis=1), "bound", bounds.min(axis=1))
    assert np.all(err <= bounds)
    srt = np.sort(ref, axis=1)
    clear = (srt[:, 1] - srt[:, 0]) > 2 * bounds.max(axis=1)
    assert clear.any() and np.all(arg.cpu().numpy()[clear] == np.argmin(ref, axis=1)[clear])
    assert torch.equal(best, out.min(dim=1).values)


def model_for(S, hack, prior=False, dtype="f32"):
    cfg = default_config(nf=SC.NF, n_speakers=S)
    cfg["model"]["init_hack"] = hack
    if prior:
        cfg["model"]["sde"] = {"_target_": "sdes.sdes.PriorMixSDE", "ndim": S, "d_lambda": 2.0, "sigma_min": 0.05,
                               "sigma_max": 0.5, "N": 30}
    m = DiffSepModel(cfg, dtype=dtype)
    c = m.score_model.cfg
    m.load_state_dict({"backbone." + k: torch.from_numpy(v) for k, v in
                       synth.synth_state_dict([(n, s) for n, s, _ in param_table(c)], 7).items()})
    return m


def test_python_methods_with_the_reference_draws(fx):
    mix, tgt = SC.inputs(2)
    z = SC.noise("z", 2)
    for hack in (0, 1, 2, 3, 4):
        tag, pred = case_arrays(fx, "m2", hack)
        m = model_for(2, hack if hack else False)
        m.sde.N = 2 if hack == 4 else 30
        kw = dict(time=dev(fx["m2_h0_time"]), z=dev(z))
        if hack == 4:
            kw["select"] = dev(fx[f"{tag}_select"])
        x_t, time, L, zr = m.sample_prior(dev(mix), dev(tgt), **kw)
        assert np.array_equal(time.cpu().numpy(), fx[f"{tag}_time"]) and L.shape == (SC.B, 2, 2)
        assert SC.rel_rms(x_t[..., :SC.HEAD].cpu(), fx[f"{tag}_xt_head"]) <= 1e-6
        assert SC.rel_rms(zr[..., :SC.HEAD].cpu(), fx[f"{tag}_z_head"]) <= 1e-6
        per = m.compute_score_loss(dev(mix), dev(tgt), per_utterance=True, **kw).cpu().numpy()
        bound = cs_bound(SC.SDES["m2"], pred, SC.perturb(SC.SDES["m2"], tgt, mix, fx[f"{tag}_time"], z, beta=fx[f"{tag}_beta"],
                                                         redefine=hack in (1, 3, 4))[1], fx[f"{tag}_time"], None, 2 * SC.T)
        assert np.all(np.abs(per - fx[f"{tag}_loss"]) <= bound + 1e-6 * fx[f"{tag}_loss"])
        scalar = m.compute_score_loss(dev(mix), dev(tgt), **kw)
        assert scalar.dim() == 0 and abs(float(scalar) - per.mean()) <= 1e-6 * per.mean()
    # the PIT forms: the minimum over permutations moves by at most the largest per-permutation bound of the end-to-end test
    m7 = model_for(2, 7)
    sde2 = SC.SDES["m2"]
    best = m7.compute_score_loss_init_hack_pit(dev(mix), dev(tgt), z=dev(z)).cpu().numpy()
    ref, bounds = pit_bounds(fx, "m2_pit1", "true_mix", sde2, 2, mix, tgt, z, fx["m2_pit1_time"])
    assert np.all(np.abs(best - ref.min(axis=1)) <= bounds.max(axis=1))
    m3 = model_for(3, 7)
    mix3, tgt3 = SC.inputs(3)
    z3 = SC.noise("z", 3)
    best = m3.compute_score_loss_with_pit_allthetime(dev(mix3), dev(tgt3), time=dev(fx["m3_pit2_time"]), z=dev(z3),
                                                     perm=fx["m3_pit2_perm"]).cpu().numpy()
    tgt3s = np.take_along_axis(tgt3, fx["m3_pit2_perm"][..., None], axis=1)
    ref, bounds = pit_bounds(fx, "m3_pit2", "mean0", SC.SDES["m3"], 3, mix3, tgt3s, z3, fx["m3_pit2_time"])
    assert np.all(np.abs(best - ref.min(axis=1)) <= bounds.max(axis=1))
    # PriorMixSDE through the Python layer (sigma_mix computed by the model's SDE object)
    mp = model_for(2, 3, prior=True)
    tag, pred = case_arrays(fx, "p2", 3)
    kw = dict(time=dev(fx[f"{tag}_time"]), z=dev(z))
    x_t, time, L, zr = mp.sample_prior(dev(mix), dev(tgt), **kw)
    assert L.shape == (SC.B, 2, 2, SC.T)
    assert SC.rel_rms(x_t[..., :SC.HEAD].cpu(), fx[f"{tag}_xt_head"]) <= 1e-6
    assert SC.rel_rms(zr[..., :SC.HEAD].cpu(), fx[f"{tag}_z_head"]) <= 1e-6
    per = mp.compute_score_loss(dev(mix), dev(tgt), per_utterance=True, **kw).cpu().numpy()
    smix = ops.sde_sigma_mix(dev(mix), 510)
    bound = cs_bound(SC.SDES["p2"], pred, zr.cpu().numpy(), fx[f"{tag}_time"], smix, 2 * SC.T)
    assert np.all(np.abs(per - fx[f"{tag}_loss"]) <= bound + 1e-6 * fx[f"{tag}_loss"])
    with pytest.raises(NotImplementedError):
        m7.compute_score_loss_with_pit(dev(mix), dev(tgt))
    with pytest.raises(NotImplementedError):
        m7.training_step((dev(mix), dev(tgt)))


def test_python_methods_without_injections_are_reproducible():
    mix, tgt = SC.inputs(2)
    for hack, strat in ((False, "uniform"), (3, "varprop"), (4, "uniform")):
        m = model_for(2, hack)
        m.time_sampling_strategy = strat
        torch.manual_seed(11)
        x1, t1, _, z1 = m.sample_prior(dev(mix), dev(tgt))
        l1 = m.compute_score_loss(dev(mix), dev(tgt))
        torch.manual_seed(11)
        x2, t2, _, z2 = m.sample_prior(dev(mix), dev(tgt))
        l2 = m.compute_score_loss(dev(mix), dev(tgt))
        assert torch.equal(x1, x2) and torch.equal(t1, t2) and torch.equal(z1, z2) and torch.equal(l1, l2)
        assert bool(torch.isfinite(l1)) and float(t1.min()) >= m.t_eps and float(t1.max()) <= m.sde.T
    m7 = model_for(2, 7)
    torch.manual_seed(5)
    a = m7.train_step_init_7(dev(mix), dev(tgt))
    torch.manual_seed(5)
    b = m7.train_step_init_7(dev(mix), dev(tgt))
    assert torch.equal(a, b) and bool(torch.isfinite(a))
    m5 = model_for(2, 5)
    torch.manual_seed(6)
    a5 = m5.train_step_init_5(dev(mix), dev(tgt), pit_mask=[True, False, False, True])
    torch.manual_seed(6)
    assert torch.equal(a5, m5.train_step_init_5(dev(mix), dev(tgt), pit_mask=[True, False, False, True])) and bool(torch.isfinite(a5))
    m0 = model_for(2, False)
    torch.manual_seed(7)
    v0 = m0.validation_step((dev(mix) * 0.1, dev(tgt) * 0.1))
    assert set(v0) == {"val/score_loss", "val/si_sdr"} and v0["val/score_loss"].dim() == 0
    out = m7.validation_step((dev(mix) * 0.1, dev(tgt) * 0.1))
    assert set(out) == {"val/score_loss", "val/si_sdr"} and np.isfinite(float(out["val/si_sdr"]))
    assert set(m7.validation_step((dev(mix) * 0.1, dev(tgt) * 0.1))) == {"val/score_loss"}  # valid_max_sep_batches = 1


# largest per-utterance |loss_16 - loss_fp32| / loss_fp32 over t in {0.03, 0.2, 0.53, 1.0} measured at nf = 64, T = 32000, B = 16
# (DESIGN.md section 5d): f16 1.96e-3, bf16 8.78e-3; gated at twice that, rounded up to one significant digit (the margin covers
# the GroupNorm-sum regrouping between batch shapes, tests/test_round5_gpu.py)
GATE_16BIT = {"f16": 4e-3, "bf16": 2e-2}


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_16bit_engine_loss_against_the_fp32_twin(dtype):
    nf, S, T, B = 64, 2, 32000, 16
    mix, tgt = (torch.from_numpy(v).cuda() for v in synth.synth_batch(B, T=T))
    mix_n, mean, std = ops.normalize_batch(mix)
    tgt_n = ((tgt - mean) / std).contiguous()
    z = ops.randn(B * S * T, 99, 0).view(B, S, T)
    m = DiffSepModel(default_config(nf=nf), dtype=dtype)
    m.load_state_dict({"backbone." + k: torch.from_numpy(v) for k, v in
                       synth.synth_state_dict([(n, s) for n, s, _ in param_table(m.score_model.cfg)], 7).items()})
    worst = {}
    for t in (0.03, 0.2, 0.53, 1.0):
        tv = torch.full((B,), t, device="cuda")
        own = m.compute_score_loss(mix_n, tgt_n, time=tv, z=z, per_utterance=True).double().cpu().numpy()
        ref = m.compute_score_loss(mix_n, tgt_n, time=tv, z=z, per_utterance=True, dtype="f32").double().cpu().numpy()
        worst[t] = float((np.abs(own - ref) / ref).max())
    print(dtype, worst)
    assert m._loss_engine("f32").dtype == _lib.F32 and m._loss_engine("f32") is not m.score_model.engine()
    assert max(worst.values()) <= GATE_16BIT[dtype]
    assert 0 < max(worst.values())  # (not the same engine twice)


def test_rows_of_a_padded_batch_equal_their_own_call():
    sde, S = SC.SDES["m2"], 2
    mix, tgt = SC.inputs(S)
    z = SC.noise("z", S)
    lens = [4000, 3900, 3971, 3970]
    for b, n in enumerate(lens):
        mix[b, :, n:], tgt[b, :, n:], z[b, :, n:] = 0, 0, 0
    t = np.array([0.2, 0.5, 0.03, 1.0], np.float32)
    eng = engine(S)
    out = ops.score_loss(eng, sde, dev(mix), dev(tgt), dev(t), z=dev(z), lengths=lens)[0]
    for b, n in enumerate(lens):
        one = ops.score_loss(eng, sde, dev(mix[b:b + 1, :, :n]), dev(tgt[b:b + 1, :, :n]), dev(t[b:b + 1]), z=dev(z[b:b + 1, :, :n]))[0]
        assert torch.equal(one[0], out[b]), (b, one, out[b])
    # (every length up to T = 4000 has the padded frame count 64: that refusal is exercised on the host, tests/test_score_loss_cpu.py)
    with pytest.raises(_lib.DiffsepError, match="utterance length outside"):
        ops.score_loss(eng, sde, dev(mix), dev(tgt), dev(t), z=dev(z), lengths=[4000, 5000, 4000, 4000])


def test_evaluate_score_loss_flag(tmp_path):
    common = ["--synthetic", "5", "--synthetic-weights", "16", "--samples", "4000", "--samples-max", "4600",
              "--dtype", "f32", "-N", "2", "--no-stoi", "--save-n", "0", "--flat-output"]

    def run(name, extra):
        out = tmp_path / name
        eval_cli.main(common + ["-o", str(out)] + extra)
        recs = json.load(open(out / "test.json"))
        return recs, json.load(open(out / "test_summary.json"))

    plain, plain_sum = run("a", ["--batch", "4", "--streams", "2"])
    with_k, with_sum = run("b", ["--batch", "4", "--streams", "2", "--score-loss", "3"])
    single, _ = run("c", ["--batch", "1", "--streams", "1", "--score-loss", "3"])
    assert all("score_loss" not in r for r in plain) and "score_loss" not in plain_sum
    drop = lambda r: {k: v for k, v in r.items() if k not in ("runtime", "score_loss")}
    assert [drop(r) for r in with_k] == [drop(r) for r in plain]
    vals = [r["score_loss"] for r in with_k]
    assert all(np.isfinite(v) and v > 0 for v in vals)
    assert abs(with_sum["score_loss"] - np.mean(vals)) <= 1e-12 * np.mean(vals)
    assert [r["score_loss"] for r in single] == vals  # batch- and stream-independent on the fp32 engine
