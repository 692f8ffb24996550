"""The score-matching loss without a GPU: the numpy restatement (tests/score_loss_cases.py) against the reference fixture
(tests/golden/gen_golden_score_loss.py), the closed-form inverse of the marginal std against numpy.linalg.solve, the
one-evaluation PIT loss against the reference's per-permutation losses, and the host-side half of the C-ABI."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import score_loss_cases as SC
from diffsep_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HACK_CASES = [("m2", 0), ("m2", 1), ("m2", 2), ("m2", 3), ("m2", 4), ("p2", 3)]


@pytest.fixture(scope="module")
def fx():
    return SC.load()


def case_arrays(fx, sde_tag, hack):
    """the fixture's arrays of one init_hack case; pred_score rows that the case does not store are those of <sde>_h3"""
    tag = f"{sde_tag}_h{hack}"
    pred = fx[f"{sde_tag}_h3_pred_rows"].copy()
    pred[fx[f"{tag}_rows"]] = fx[f"{tag}_pred_rows"]
    return tag, pred


@pytest.mark.parametrize("sde_tag, hack", HACK_CASES)
def test_restatement_reproduces_the_reference_sample_prior_and_loss(fx, sde_tag, hack):
    sde, S = SC.SDES[sde_tag], SC.SDES[sde_tag]["ndim"]
    tag, pred = case_arrays(fx, sde_tag, hack)
    mix, tgt = SC.inputs(S)
    z = SC.noise("z", S)
    smix = SC.sigma_mix(mix, sde["avg_len"]) if sde["kind"] == 1 else None
    t, beta = fx[f"{tag}_time"], fx[f"{tag}_beta"]
    x_t, zr = SC.perturb(sde, tgt, mix, t, z, beta=beta, redefine=hack in (1, 3, 4), smix=smix)
    e_x, e_z = SC.rel_rms(x_t[..., :SC.HEAD], fx[f"{tag}_xt_head"]), SC.rel_rms(zr[..., :SC.HEAD], fx[f"{tag}_z_head"])
    print(tag, "x_t", e_x, "z'", e_z)
    assert e_x <= 1e-6 and e_z <= 1e-6
    loss = SC.reduce(sde, pred, zr, t, smix=smix)[:, 0]
    rel = np.abs(loss - fx[f"{tag}_loss"]) / fx[f"{tag}_loss"]
    print(tag, "loss", loss, "rel", rel)
    assert np.all(rel <= 1e-6)


def test_fixture_times_cover_both_ends(fx):
    t = fx["m2_h3_time"]
    assert t.min() < 2 * SC.T_EPS and t.max() > 1.0 - SC.T_REV_INIT
    assert fx["m2_h4_select"].sum() == 1 and np.all(fx["m2_h4_time"][fx["m2_h4_select"] > 0] == 1.0)
    assert fx["m2_h1_beta"].sum() == 1 and 0 < fx["m2_h3_beta"].max() < 1


@pytest.mark.parametrize("sde_tag", ["m2", "m3", "p2"])
def test_closed_form_inverse_equals_linalg_solve(fx, sde_tag):
    sde, S = SC.SDES[sde_tag], SC.SDES[sde_tag]["ndim"]
    mix, tgt = SC.inputs(S)
    smix = SC.sigma_mix(mix, sde["avg_len"]) if sde["kind"] == 1 else None
    times = np.concatenate([fx["m2_h3_time"], fx["m2_h4_time"], fx["m2_pit1_time"], fx["m3_pit2_time"]]).astype(np.float64)
    d = tgt.astype(np.float64)
    for t in np.unique(times):
        tv = np.full(SC.B, t)
        L = SC.dense_std(sde, tv, S, smix)
        c = SC.coefs(sde, tv)
        sm = 1.0 if smix is None else smix.astype(np.float64)[:, None, :]
        mine = SC.linv(d, c[:, 1, None, None] * sm, c[:, 2, None, None] * sm, S, np.float64)
        if smix is None:
            ref = np.linalg.solve(L, d)
        else:
            ref = np.linalg.solve(L.transpose(0, 3, 1, 2), d.transpose(0, 2, 1)[..., None])[..., 0].transpose(0, 2, 1)
        assert SC.rel_rms(mine, ref) <= 1e-12, (sde_tag, t)


@pytest.mark.parametrize("tag, pit", [("m2_pit1", 1), ("m3_pit2", 2)])
def test_one_evaluation_pit_loss_matches_the_per_permutation_reference(fx, tag, pit):
    """The reference evaluates the network once per permutation; its x_t differ by fp32 rounding only (xt_maxdiff) and the
    generator measured how far that moves a loss (xt_rounding_rel).  One evaluation (the first permutation's pred_score)
    must give every permutation's loss within that measured bound plus the 1e-6 of the plain-loss check."""
    sde_tag = tag[:2]
    sde, S = SC.SDES[sde_tag], SC.SDES[sde_tag]["ndim"]
    mix, tgt = SC.inputs(S)
    z0 = SC.noise("z", S)
    t = fx[f"{tag}_time"]
    if pit == 2:
        tgt = np.take_along_axis(tgt, fx[f"{tag}_perm"][..., None], axis=1)
    x_t, _ = SC.perturb(sde, tgt, mix, t, z0, beta=np.ones(SC.B) if pit == 1 else None)
    assert SC.rel_rms(x_t[..., :SC.HEAD], fx[f"{tag}_xt_head"]) <= 1e-6
    assert float(fx[f"{tag}_xt_maxdiff"][0]) <= 1e-6
    out = SC.reduce(sde, fx[f"{tag}_pred"], z0, t, x0=tgt, mix=mix, pit=pit)
    ref = fx[f"{tag}_perm_losses"].astype(np.float64)
    bound = float(fx[f"{tag}_xt_rounding_rel"][0]) + 1e-6
    rel = np.abs(out - ref) / ref
    print(tag, "max rel", rel.max(), "bound", bound)
    assert out.shape == (SC.B, len(SC.perms(S))) and np.all(rel <= bound)
    gap = np.sort(ref, axis=1)
    clear = (gap[:, 1] - gap[:, 0]) > 2 * bound * gap[:, 1]
    assert np.all(np.argmin(out, axis=1)[clear] == np.argmin(ref, axis=1)[clear])


def test_masked_rows_equal_their_own_short_call():
    sde, S = SC.SDES["m2"], 2
    mix, tgt = SC.inputs(S)
    z, lens, t = SC.noise("z", S), [4000, 3900, 3971, 3970], np.array([0.2, 0.5, 0.03, 1.0])
    x_t, zr = SC.perturb(sde, tgt, mix, t, z, lengths=lens)
    out = SC.reduce(sde, x_t, zr, t, lengths=lens)
    for b, n in enumerate(lens):
        assert not x_t[b, :, n:].any() and not zr[b, :, n:].any()
        xb, zb = SC.perturb(sde, tgt[b:b + 1, :, :n], mix[b:b + 1, :, :n], t[b:b + 1], z[b:b + 1, :, :n])
        assert np.array_equal(xb[0], x_t[b, :, :n])
        assert abs(SC.reduce(sde, xb, zb, t[b:b + 1])[0, 0] - out[b, 0]) <= 1e-14 * out[b, 0]


# ---------------------------------------------------------------- the C-ABI without a GPU
NEW = ("diffsep_sde_mult_std_inv", "diffsep_sde_perturb", "diffsep_score_loss_reduce", "diffsep_score_loss_workspace_bytes",
       "diffsep_score_loss", "diffsep_score_loss_validate")


def test_header_and_lib_agree_on_the_new_entries():
    hdr = open(os.path.join(ROOT, "include", "diffsep_hip.h")).read()
    declared = set(re.findall(r"\b(diffsep_[a-z0-9_]+)\s*\(", hdr))
    for kind in ("bf16", "f16"):
        l = _lib.lib(kind)
        for name in NEW:
            assert name in declared and name in _lib.EXPORTS and hasattr(l, name), name
    body = re.search(r"typedef struct \{([^}]*)\}\s*diffsep_loss_config;", re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)).group(1)
    fields = [d.split()[-1] for d in body.split(";") if d.strip()]
    assert fields == [n for n, _ in _lib.LossConfig._fields_] and all(t is C.c_int32 for _, t in _lib.LossConfig._fields_)
    codes = {n: int(v) for n, v in re.findall(r"#define (DIFFSEP_PIT_\w+)\s+(\d+)", hdr)}
    assert codes == {"DIFFSEP_PIT_NONE": _lib.PIT_NONE, "DIFFSEP_PIT_TRUE_MIX": _lib.PIT_TRUE_MIX, "DIFFSEP_PIT_MEAN0": _lib.PIT_MEAN0}


def test_workspace_arithmetic_and_refusals_without_a_gpu():
    l = _lib.lib()
    # one slab row of 6 float64 per block of 256 threads x 4 samples, per utterance
    for B, S, T in ((1, 2, 1), (4, 2, 4000), (16, 3, 32000), (3, 1, 1025)):
        assert l.diffsep_score_loss_workspace_bytes(B, S, T) == B * (((T + 3) // 4 + 255) // 256) * 48
    assert l.diffsep_score_loss_workspace_bytes(4, 4, 4000) == -1 and b"S in 1..3" in l.diffsep_last_error()
    assert l.diffsep_score_loss_workspace_bytes(0, 2, 4000) == -1
    sde = _lib.SdeConfig(0, 2, 2.0, 0.05, 0.5, 0)
    fake = C.c_void_p(4096)  # never dereferenced: every refusal below comes before the first launch
    need = l.diffsep_score_loss_workspace_bytes(4, 2, 4000)
    rc = l.diffsep_score_loss_reduce(C.byref(sde), fake, fake, None, None, fake, None, None, 0, fake, None, None, None, 4, 4,
                                     4000, fake, need, None)
    assert rc != 0 and b"sources" in l.diffsep_last_error()
    rc = l.diffsep_score_loss_reduce(C.byref(sde), fake, fake, None, None, fake, None, None, 0, fake, None, None, None, 4, 2,
                                     4000, fake, need - 1, None)
    assert rc != 0 and b"workspace too small" in l.diffsep_last_error()
    rc = l.diffsep_score_loss_reduce(C.byref(sde), fake, fake, None, None, fake, None, None, 1, fake, None, None, None, 4, 2,
                                     4000, fake, need, None)
    assert rc != 0 and b"x0 and mix" in l.diffsep_last_error()
    rc = l.diffsep_sde_perturb(C.byref(sde), fake, fake, fake, None, None, None, 0, None, 0, 0, fake, fake, 4, 5, 4000, None)
    assert rc != 0 and b"sources" in l.diffsep_last_error()
    # the fused call's own checks, from the model configuration alone
    cfg, loss = _lib.model_config(nf=16), _lib.LossConfig(0, 0)
    ok = (C.c_int64 * 4)(4000, 3900, 3970, 3969)   # all 35 frames -> 64 padded
    assert l.diffsep_score_loss_validate(C.byref(cfg), C.byref(loss), 4, 4000, ok, need) == 0
    T = 8000  # 66 frames -> 128 padded; an utterance of 7000 samples has 58 -> 64
    need8 = l.diffsep_score_loss_workspace_bytes(2, 2, T)
    bad = (C.c_int64 * 2)(8000, 7000)
    assert l.diffsep_padded_frames(C.byref(cfg), 8000) != l.diffsep_padded_frames(C.byref(cfg), 7000)
    assert l.diffsep_score_loss_validate(C.byref(cfg), C.byref(loss), 2, T, bad, need8) != 0
    assert b"padded frame count" in l.diffsep_last_error()
    assert l.diffsep_score_loss_validate(C.byref(cfg), C.byref(loss), 4, 4000, ok, need - 8) != 0
    assert b"workspace too small" in l.diffsep_last_error()
    assert l.diffsep_score_loss_validate(C.byref(cfg), C.byref(_lib.LossConfig(3, 0)), 4, 4000, None, need) != 0
    assert b"pit_mode" in l.diffsep_last_error()
