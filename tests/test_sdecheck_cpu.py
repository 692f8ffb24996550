"""The instruments of tests/sdecheck.py checked on the CPU: the Philox reference against the Random123 known answers, every
float64 reference against the stored goldens and the fp32 oracle (inside the old RMS gates, and inside the new per-element
bound scaled for two fp32 evaluations: the bounds are neither vacuous nor impossibly tight), the conditions the GPU cases rely
on, and planted errors that must exceed the bound — each printed with the relative RMS it produces, most of which the old gates
(1e-6 .. 2e-5) would have let through."""
import numpy as np
import pytest
import torch

import diffsep_oracle as O
import sdecheck as C
from diffsep_amd import synth

torch.set_grad_enabled(False)


# ------------------------------------------------------------------------------------------------ Philox
def test_philox_reference_known_answers():
    kat = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for ctr, key, want in kat:
        out = C.philox4x32_10(np.array([ctr], np.uint32), key)[0]
        assert " ".join(f"{int(v):08x}" for v in out) == want
    # the stream's counter and key words: (q, 0, sid lo, sid hi) under (seed lo, seed hi)
    sid, seed = (7 << 32) | 5, (9 << 32) | 3
    assert np.array_equal(C.stream_words(3, seed, sid)[2], C.philox4x32_10(np.array([[2, 0, 5, 7]], np.uint32), (3, 9))[0])


def test_uniform_mapping_and_box_muller():
    # u == 1.0 for c >> 8 == 0xffffff (the fp32 sum 16777215.5 rounds to even): radius 0, not infinity; the smallest u is 2^-25
    u = C.uniform_f32(np.array([0xffffffff, 0xffffff00, 0xfffffe00, 0, 0x100], np.uint32))
    assert u.dtype == np.float32 and u[0] == 1.0 and u[1] == 1.0 and u[2] < 1.0 and u[3] == 2.0 ** -25 and u[4] == 1.5 * 2.0 ** -24
    v = C.box_muller(u[:1], u[2:3], u[3:4], u[4:5])
    assert np.all(v[0, :2] == 0.0) and np.all(np.isfinite(v)) and abs(np.hypot(v[0, 2], v[0, 3]) - np.sqrt(50.0 * np.log(2.0))) < 1e-12
    ref, bound = C.randn_ref(1 << 16, 123, 0)
    assert abs(ref.mean()) < 2e-2 and abs(ref.std() - 1.0) < 1e-2 and abs((ref ** 4).mean() - 3.0) < 0.1
    assert (bound[ref != 0] > 0).all() and C.NOISE_C == 5.5
    # the batch layout: value s * len + t, zero tail, every S * len % 4 residue in lens = [9, 1, 0, 6] at S in {1, 3}
    for S in (1, 3):
        lens, seeds = [9, 1, 0, 6], [11, 2 ** 40 + 5, 3, 2 ** 64 - 1]
        assert {(S * n) % 4 for n in lens} >= ({0, 1, 2} if S == 1 else {0, 2, 3})
        rb, bb = C.randn_batch_ref(S, 9, seeds, lens, 1)
        for b, n in enumerate(lens):
            one = C.randn_ref(S * n, seeds[b], 1)[0].reshape(S, n)
            assert np.array_equal(rb[b, :, :n], one) and not rb[b, :, n:].any() and not bb[b, :, n:].any()
    assert {(S * n) % 4 for S in (1, 3) for n in (9, 1, 0, 6)} == {0, 1, 2, 3}


# ------------------------------------------------------------------------------------------------ references against what exists
@pytest.fixture(scope="module")
def g9(golden):
    """the inputs of the golden updates at B = 2, S = 2, T = 4000 (tests/test_oracle_golden.py builds the same)"""
    g, _ = golden
    cfg = O.default_config(16, 2)
    p = O.to_torch(synth.synth_state_dict(O.param_table(cfg), 7))
    B, S, T = 2, 2, 4000
    mix_norm = torch.from_numpy(g["g10_mix_norm"])
    x0 = torch.from_numpy(synth.synth_noise("g9.x0", (B, S, T))) * 0.5
    tv = torch.tensor([0.8, 0.2])
    sc = O.score_forward(p, cfg, x0, tv, mix_norm)
    draws = [torch.from_numpy(synth.synth_noise(f"g9.z{i}", (B, S, T))) for i in range(3)]
    return dict(g=g, cfg=cfg, mix_norm=mix_norm, x0=x0, tv=tv, sc=sc, draws=draws, smix=O.sigma_mix(mix_norm, 510)[:, 0])


def _against(name, rb, gold, gate, oracle32, oracle64=None, fp32_sums=False):
    """a float64 reference with its bound against the golden (RMS gate), the fp32 oracle (RMS gate and 2 x the bound per
    element) and, where given, the oracle evaluated in float64 (which must be float64 and agree to 1e-6).  fp32_sums: the oracle
    reduces T samples in fp32 where the kernel sums in fp64, so its error is not the kernel's: the ratio is printed only."""
    ref, bound = rb
    assert ref.dtype == np.float64 and bound.dtype == np.float64 and ref.shape == bound.shape
    o32 = oracle32.numpy() if hasattr(oracle32, "numpy") else np.asarray(oracle32)
    assert o32.dtype == np.float32
    ref = ref.reshape(o32.shape) if ref.size == o32.size else np.broadcast_to(ref, o32.shape)
    bound = bound.reshape(o32.shape) if bound.size == o32.size else np.broadcast_to(bound, o32.shape)
    if gold is not None:
        assert C.rel_rms(ref, gold) < gate, (name, C.rel_rms(ref, gold))
    assert C.rel_rms(ref, o32) < gate, (name, C.rel_rms(ref, o32))
    r = C.ratio(o32, ref, 2.0 * bound)
    assert (bound[ref != 0] > 0).all(), name
    line = f"[sdecheck cpu {name}] fp32 oracle err / (2 bound) {r:.3f}"
    if oracle64 is not None:
        assert oracle64.dtype == torch.float64
        d = C.rel_rms(ref, oracle64.numpy())
        assert d < 1e-6, (name, d)
        line += f", float64 oracle rel rms {d:.1e}"
    print(line)
    assert r <= 1.0 or fp32_sums, (name, r)
    return r


def test_references_match_goldens_and_oracle_mix(g9):
    g, cfg, x0, tv, sc, dr, mn = g9["g"], g9["cfg"], g9["x0"], g9["tv"], g9["sc"], g9["draws"], g9["mix_norm"]
    d = lambda t: t.double()  # noqa: E731
    _against("prior", C.prior(C.MIX, mn, dr[0]), g["g9_prior"], 1e-6, O.prior_sampling(cfg, mn, dr[0]), O.prior_sampling(cfg, d(mn), d(dr[0])))
    (xc, xcm) = C.corrector(C.MIX, 0.5, x0, tv, sc, dr[1])
    oc, ocm = O.corrector_ald2(cfg, x0, tv, sc, dr[1], 0.5)
    oc64, ocm64 = O.corrector_ald2(cfg, d(x0), d(tv), d(sc), d(dr[1]), 0.5)
    _against("ald2 x", xc, g["g9_corr_x"], 2e-5, oc, oc64)
    _against("ald2 mean", xcm, g["g9_corr_mean"], 2e-5, ocm, ocm64)
    (xp, xpm) = C.predictor(C.MIX, 3, x0, tv, sc, dr[2])
    op, opm = O.predictor_reverse_diffusion(cfg, x0, tv, sc, dr[2], 3)
    op64, opm64 = O.predictor_reverse_diffusion(cfg, d(x0), d(tv), d(sc), d(dr[2]), 3)
    _against("predictor x", xp, g["g9_pred_x"], 2e-5, op, op64)
    _against("predictor mean", xpm, g["g9_pred_mean"], 2e-5, opm, opm64)
    _against("em x", xp, g["g12_em_x"], 2e-5, op)
    (xa, xam) = C.corrector(C.MIX, 0.5, x0, tv, sc, dr[1], variant=1)
    oa, oam = O.corrector_ald(cfg, x0, tv, sc, dr[1], 0.5)
    _against("ald x", xa, g["g12_ald_x"], 2e-5, oa, O.corrector_ald(cfg, d(x0), d(tv), d(sc), d(dr[1]), 0.5)[0])
    _against("ald mean", xam, g["g12_ald_mean"], 2e-5, oam)
    xl, xlm, _ = C.langevin(0.5, x0, sc, dr[1])
    ol, olm = O.corrector_langevin(x0, sc, dr[1], 0.5)
    _against("langevin x", xl, g["g12_langevin_x"], 2e-5, ol, O.corrector_langevin(d(x0), d(sc), d(dr[1]), 0.5)[0])
    _against("langevin mean", xlm, g["g12_langevin_mean"], 2e-5, olm)
    (pf, pfm) = C.predictor(C.MIX, 3, x0, tv, sc, None, pflow=True)
    rf, _ = O.rsde_discretize(cfg, x0, tv, sc, 3, None, probability_flow=True)
    _against("probability flow", pfm, g["g12_pflow_mean"], 2e-5, x0 - rf)
    assert pf[0] is pfm[0]


def test_references_match_goldens_and_oracle_priormix(g9):
    g, cfg, x0, tv, sc, dr, mn, smix = (g9[k] for k in ("g", "cfg", "x0", "tv", "sc", "draws", "mix_norm", "smix"))
    sm3 = smix[:, None, :]
    _against("sigma_mix 510", C.sigma_mix(mn, 510), g["g11_sigma_mix"][:, 0], 1e-6, smix, O.sigma_mix(mn.double(), 510)[:, 0])
    _against("pmix prior", C.prior(C.PMIX, mn, dr[0], smix), g["g11_prior"], 1e-6, O.prior_sampling(cfg, mn, dr[0], sm3))
    xc, xcm = C.corrector(C.PMIX, 0.5, x0, tv, sc, dr[1], smix)
    oc, ocm = O.corrector_ald2(cfg, x0, tv, sc, dr[1], 0.5, sm3)
    _against("pmix ald2 x", xc, g["g11_corr_x"], 2e-5, oc)
    _against("pmix ald2 mean", xcm, g["g11_corr_mean"], 2e-5, ocm)
    xp, xpm = C.predictor(C.PMIX, 3, x0, tv, sc, dr[2], smix)
    op, opm = O.predictor_reverse_diffusion(cfg, x0, tv, sc, dr[2], 3, sm3)
    _against("pmix predictor x", xp, g["g11_pred_x"], 2e-5, op)
    _against("pmix predictor mean", xpm, g["g11_pred_mean"], 2e-5, opm)


def test_references_match_goldens_and_oracle_surface(g9, golden2):
    cfg, x0, tv, sc, smix, g2 = g9["cfg"], g9["x0"], g9["tv"], g9["sc"], g9["smix"], golden2
    for tag, sde, sm in (("mix", C.MIX, None), ("pmix", C.PMIX, smix)):
        od, og = O.sde_coefficients(cfg, x0, tv, sm)
        cd, cg = C.sde_coefficients(sde, x0, tv, sm)
        _against(f"{tag} drift", cd, g2[f"g13_{tag}_drift"], 1e-6, od)
        _against(f"{tag} diffusion", cg, g2[f"g13_{tag}_diffusion"], 1e-6, og)
        _against(f"{tag} mean", C.sde_mean(sde, x0, tv), g2[f"g13_{tag}_mean"], 1e-6, O.sde_mean(cfg, x0, tv), O.sde_mean(cfg, x0.double(), tv.double()))
        ostd = O.sde_std(cfg, tv, 2, sm)
        _against(f"{tag} std", C.sde_std(sde, tv, 2, sm, T=x0.shape[-1]), g2[f"g13_{tag}_std"], 1e-6, ostd)
        _against(f"{tag} mult_std", C.sde_mult_std(ostd, x0), g2[f"g13_{tag}_mult_std"], 1e-6, O.sde_mult_std(ostd, x0))
        of, oG = O.sde_discretize(cfg, x0, tv, 3, sm)
        dt = np.float32(1.0 / 3)
        cf, cG = C.sde_coefficients(sde, x0, tv, sm, f_scale=dt, g_scale=np.sqrt(dt))
        _against(f"{tag} f", cf, g2[f"g13_{tag}_f"], 1e-6, of)
        _against(f"{tag} G", cG, g2[f"g13_{tag}_G"], 1e-6, oG)
        orf, _ = O.rsde_discretize(cfg, x0, tv, sc, 3, sm)
        _against(f"{tag} rev_f", C.sde_reverse_drift(of, oG, sc), g2[f"g13_{tag}_rev_f"], 2e-5, orf)


def test_references_match_goldens_and_oracle_three_sources_and_embedding(g9, golden2, golden3):
    g2 = golden2
    cfg = O.default_config(16, 3)
    p = O.to_torch(synth.synth_state_dict(O.param_table(cfg), 7))
    B, T = 2, 4000
    x0 = torch.from_numpy(synth.synth_noise("g15.x0", (B, 3, T))) * 0.5
    z = [torch.from_numpy(synth.synth_noise(f"g15.z{i}", (B, 3, T))) for i in range(2)]
    tv = g9["tv"]
    sde3 = dict(C.MIX, ndim=3)
    _against("S = 3 std", C.sde_std(sde3, tv, 3), g2["g15_std"], 1e-6, O.mix_std(cfg, tv, 3), O.mix_std(cfg, tv.double(), 3))
    sc = O.score_forward(p, cfg, x0, tv, g9["mix_norm"])
    xc, xcm = C.corrector(sde3, 0.5, x0, tv, sc, z[0])
    oc, ocm = O.corrector_ald2(cfg, x0, tv, sc, z[0], 0.5)
    _against("S = 3 ald2 x", xc, g2["g15_corr_x"], 2e-5, oc)
    _against("S = 3 ald2 mean", xcm, g2["g15_corr_mean"], 2e-5, ocm)
    xp, xpm = C.predictor(sde3, 3, x0, tv, sc, z[1])
    op, opm = O.predictor_reverse_diffusion(cfg, x0, tv, sc, z[1], 3)
    _against("S = 3 predictor x", xp, g2["g15_pred_x"], 2e-5, op)
    _against("S = 3 predictor mean", xpm, g2["g15_pred_mean"], 2e-5, opm)
    for nf in (16, 64):
        c = O.default_config(nf, 2)
        sd = synth.synth_state_dict(O.param_table(c), 7)
        t = torch.tensor([1.0, 0.53, 0.2, 0.03])
        rb = C.time_embedding(t, *(sd[k] for k in ("all_modules.0.W", "all_modules.1.weight", "all_modules.1.bias", "all_modules.2.weight",
                                                   "all_modules.2.bias")))
        _against(f"time embedding nf {nf}", rb, golden3[f"g16_temb_nf{nf}"], 2e-5, O.time_embedding(O.to_torch(sd), t))
    # normalize_batch / scale_output on the golden mixture
    g = g9["g"]
    mix = torch.from_numpy(synth.synth_batch(2, T=4000)[0])
    nb = C.normalize_batch(mix)
    om, omean, ostd = O.normalize_batch(mix)
    _against("normalize out", nb["out"], g["g10_mix_norm"], 1e-6, om, fp32_sums=True)
    _against("normalize mean", nb["mean"], None, 1e-5, omean.reshape(-1), fp32_sums=True)
    _against("normalize std", nb["std"], None, 1e-6, ostd.reshape(-1), fp32_sums=True)
    sep = torch.from_numpy(g["g9_sep"])
    _against("scale_output", C.scale_output(mix, sep), g["g10_scale_output"], 1e-6, O.scale_output(mix, sep), fp32_sums=True)


# ------------------------------------------------------------------------------------------------ conditions on the inputs
def test_case_conditions():
    m = C.sigma_mix_signals()
    floor = 0.5 * np.sqrt(C.SIGMA_FLOOR)
    for k in (1, 2, 3, 8, 509, 510, 2000):
        ref, bound = C.sigma_mix(m, k)
        at, above = int((ref[1] == floor).sum()), int((ref[1] > floor).sum())
        want = O.sigma_mix(torch.from_numpy(m).double()[:, None], k)[:, 0].numpy()
        assert ref.shape == (2, 700) and np.abs(ref - want).max() < 1e-7 * want.max(), k  # (the oracle clamps at the double 1e-4)
        assert (bound > 0).all() and (ref >= floor).all()
        # at least avg_len outputs exactly at the floor and as many above it — wherever 700 samples with 600 zeros can hold
        # both (2 k <= 700); a window of 509 / 510 is all silence at 600 - k + 1 = 92 / 91 outputs, one of 2000 nowhere
        assert at >= max(0, 600 - k + 1) and above >= min(k, 100), (k, at, above)
        if 2 * k <= 700:
            assert at >= k and above >= k, (k, at, above)
    assert int((C.sigma_mix(m, 2000)[0][1] == floor).sum()) == 0
    # no bound is zero where the reference is not, on every family at the smallest shapes of the GPU file
    for pm in (False, True):
        sde = C.PMIX if pm else C.MIX
        for S in (1, 2, 3, 4):
            c = C.state_case(f"cond{S}{pm}", 3, S, 5, pm)
            outs = [C.prior(sde, c["y"], c["z"], c["smix"])]
            outs += C.corrector(sde, 0.5, c["x"], C.T_CASES, c["score"], c["z"], c["smix"])
            outs += C.predictor(sde, 30, c["x"], C.T_CASES, c["score"], c["z"], c["smix"])
            outs += C.predictor(sde, 1, c["x"], C.T_CASES, c["score"], None, c["smix"], pflow=True)
            outs += C.sde_coefficients(sde, c["x"], C.T_CASES, c["smix"], 0.25, 0.5)
            outs += [C.sde_mean(sde, c["x"], C.T_CASES), C.sde_std(sde, C.T_CASES, S, c["smix"], T=5)]
            outs += C.langevin(0.5, c["x"], c["score"], c["z"])[:2]
            outs += [C.scale_output(c["y"], c["x"]), C.gram(c["x"], c["z"])]
            for ref, bound in outs:
                assert ref.dtype == np.float64 and np.isfinite(ref).all() and np.isfinite(bound).all()
                assert (bound[ref != 0] > 0).all(), (pm, S)
    # S = 1: the P part is exactly zero in the reference too
    c = C.state_case("cond.s1", 3, 1, 5, False)
    assert np.array_equal(C.sde_coefficients(C.MIX, c["x"], C.T_CASES)[0][0], np.zeros((3, 1, 5)))
    # the cancellation of ev1 at the sampler's last time: the coefficient error grows as t -> 0 and stays far below 1
    co = C.mix_coef(C.MIX, C.T_CASES)
    assert co.ra[2] > co.ra[0] and co.ra[2] * C.U < 1e-5 and (co.a > 0).all() and (co.p > 0).all()
    # exact-integer projection: every partial sum is an integer below 2^24
    x, ws, bs = C.int_case("cond.int", 17, 1024, (65,))
    y, _ = C.dense_projection(x, ws, bs, silu_in=False)
    assert np.array_equal(y, np.round(y)) and np.abs(x).max() <= 3 and 9 * 1024 + 8 < 2 ** 24
    assert np.array_equal((torch.from_numpy(x) @ torch.from_numpy(ws[0]).T + torch.from_numpy(bs[0])).double().numpy(), y)
    ks = {K for K, _, _ in C.dense_cases()}
    assert ks == set(C.DENSE_K16 + C.DENSE_KGEN)
    for route in (C.DENSE_K16, C.DENSE_KGEN):
        on = [(o, b) for K, o, b in C.dense_cases() if K in route]
        assert {sum(o) for o, _ in on} >= set(C.DENSE_O) and {b for _, b in on} >= set(C.DENSE_B)
    assert C.dense_roundings(128) == 25 and C.dense_roundings(96) == 97


# ------------------------------------------------------------------------------------------------ planted errors
def _plant(name, bad, ref, bound, old_gate):
    """old_gate: the relative-RMS gate of the test that covered this kernel before, None where no value was compared at all"""
    r, rms = C.ratio(bad, ref, bound), C.rel_rms(bad, ref)
    verdict = "no value was compared before" if old_gate is None else f"{'passes' if rms < old_gate else 'fails'} the old gate of {old_gate:.0e}"
    print(f"[sdecheck plant] {name}: err / bound {r:.1f}, relative RMS {rms:.2e} ({verdict})")
    assert r > 1.0, (name, r)
    return rms


def test_planted_errors_exceed_the_bound(monkeypatch):
    B, S, T = 3, 3, 1000
    c = C.state_case("plant", B, S, T, False)
    # 1. the last time index of the last utterance takes utterance 0's coefficient
    for name, fn in (("corrector", lambda t: C.corrector(C.MIX, 0.5, c["x"], t, c["score"], c["z"])[0]),
                     ("predictor", lambda t: C.predictor(C.MIX, 30, c["x"], t, c["score"], c["z"])[0]),
                     ("sde_mean", lambda t: C.sde_mean(C.MIX, c["x"], t))):
        ref, bound = fn(C.T_CASES)
        bad = ref.copy()
        bad[-1, :, -1] = fn(np.full(B, C.T_CASES[0], np.float32))[0][-1, :, -1]
        _plant(f"{name}: last index of the last utterance on utterance 0's coefficient", bad, ref, bound, 2e-5)
    # 2. the source mean divides by 2 at S = 3
    ref, bound = C.prior(dict(C.MIX, ndim=3), c["y"], c["z"])
    rp, bp = C.predictor(C.MIX, 30, c["x"], C.T_CASES, c["score"], c["z"])[1]
    monkeypatch.setattr(C, "_ms", lambda v: v.sum(1, keepdims=True) / 2.0)
    _plant("prior: source mean / 2 at S = 3", C.prior(dict(C.MIX, ndim=3), c["y"], c["z"])[0], ref, bound, 1e-6)
    _plant("predictor: source mean / 2 at S = 3", C.predictor(C.MIX, 30, c["x"], C.T_CASES, c["score"], c["z"])[1][0], rp, bp, 2e-5)
    monkeypatch.undo()
    # 3. Box-Muller pairing (u0, u1), (u2, u3) -> (u0, u2), (u1, u3);  4. the stream id's high word dropped
    n, seed, sid = 4099, 2 ** 40 + 5, 2 ** 32 + 1
    ref, bound = C.randn_ref(n, seed, sid)
    u = C.uniform_f32(C.stream_words((n + 3) // 4, seed, sid))
    bad = C.box_muller(u[:, 0], u[:, 2], u[:, 1], u[:, 3]).reshape(-1)[:n]
    _plant("randn: Box-Muller pairs (u0, u2), (u1, u3)", bad, ref, bound, None)
    assert abs(bad.mean()) < 5e-2 and abs(bad.std() - 1.0) < 5e-2 and abs((bad ** 4).mean() - 3.0) < 0.5  # (the old moments test passes)
    bad = C.randn_ref(n, seed, sid & 0xFFFFFFFF)[0]
    _plant("randn: stream id without its high word", bad, ref, bound, None)
    assert abs(bad.mean()) < 5e-2 and abs(bad.std() - 1.0) < 5e-2
    # 5. the projection misses its B % 16 tail row (left as the buffer was: zeros)
    x, ws, bs = C.rand_case("plant.dense", 17, 128, (65,))
    ref, bound = C.dense_projection(x, ws, bs)
    bad = ref.copy()
    bad[16] = 0.0
    _plant("dense projection: row 16 of B = 17 not written", bad, ref, bound, 2e-5)
    # and what must NOT exceed it: the reference rounded to fp32
    for ref, bound in (C.dense_projection(x, ws, bs), C.prior(C.MIX, c["y"], c["z"][:, :2]), C.randn_ref(n, seed, sid)):
        assert C.ratio(ref.astype(np.float32), ref, bound) <= 1.0
