"""Posterior draws on the GPU: the kernels of csrc/ensemble.hip against the numpy restatement (tests/ensemble_ref.py) at the
shapes where indexing can go wrong, DiffSepModel.separate_draws on the engine, and separate / evaluate --draws.

Every kernel case runs a batch of B = 3 utterances of lengths (T, 1, an odd value below T) whose inputs beyond the length are
NaN and whose outputs are pre-filled with NaN: whatever is read or left unwritten beyond a length shows."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import ensemble_ref as R
from diffsep_amd import _lib, inflight, ops, synth, wavio
from diffsep_amd import evaluate as eval_cli
from diffsep_amd import separate as sep_cli
from diffsep_amd.engine import param_table
from diffsep_amd.pl_model import DiffSepModel, default_config

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

TS = [1, 5, 256, 257, 4099]
NAN = float("nan")


def lengths_of(T):
    return [T, 1, 1 if T < 3 else ((2 * T) // 3) | 1]  # (T, 1, an odd value below T)


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def bits64(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def nan_padded(x, lengths):
    """x [B, ..., T] float32 with everything beyond each utterance's length replaced by NaN"""
    x = x.copy()
    for b, n in enumerate(lengths):
        x[b, ..., n:] = NAN
    return x


def run(draws, lengths=None, anchor=None):
    """diffsep_ensemble through the C-ABI with every output asked for and pre-filled with NaN (integers: -7) -> dict of
    device tensors"""
    l = _lib.lib()
    d = torch.from_numpy(draws).cuda()
    B, K, S, T = d.shape
    a = None if anchor is None else torch.from_numpy(anchor).cuda()
    ln = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device="cuda")
    o = dict(mean=torch.full((B, S, T), NAN, device="cuda"), std=torch.full((B, S, T), NAN, device="cuda"),
             pick=torch.full((B, S, T), NAN, device="cuda"), perm=torch.full((B, K, S), -7, dtype=torch.int32, device="cuda"),
             dist=torch.full((B, K), NAN, dtype=torch.float64, device="cuda"),
             medoid=torch.full((B,), -7, dtype=torch.int32, device="cuda"),
             gram=torch.full((B, K, S, S), NAN, dtype=torch.float64, device="cuda"))
    need = l.diffsep_ensemble_workspace_bytes(B, K, S)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    _lib.call(l, "diffsep_ensemble", P(d), P(a), P(ln), B, K, S, T, P(o["mean"]), P(o["std"]), P(o["pick"]), P(o["perm"]),
              P(o["dist"]), P(o["medoid"]), P(o["gram"]), P(ws), need, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.current_stream().synchronize()
    return o


def check_padding_and_nan(o, lengths):
    for name in ("mean", "std", "pick"):
        w = bits(o[name])
        for b, n in enumerate(lengths):
            assert not w[b, :, n:].any(), (name, b)  # +0.0 beyond the length: all bits clear
        assert bool(torch.isfinite(o[name]).all()), name
    assert bool(torch.isfinite(o["dist"]).all()) and bool(torch.isfinite(o["gram"]).all())


# ------------------------------------------------------------------------------------------------ 1. exact integers
@pytest.mark.parametrize("K", [1, 2, 4])
@pytest.mark.parametrize("S", [1, 2, 3])
@pytest.mark.parametrize("T", TS)
def test_exact_integers(T, S, K):
    """integers in [-8, 8] and K a power of two: every product, sum, mean and squared deviation is exact in float64 and the
    mean in float32, so the device and the restatement agree whatever their summation orders — tolerance zero"""
    rng = np.random.default_rng(1000 * T + 10 * S + K)
    B, lens = 3, lengths_of(T)
    clean = rng.integers(-8, 9, (B, K, S, T)).astype(np.float32)
    anchor = rng.integers(-8, 9, (B, S, T)).astype(np.float32)
    for with_anchor in (False, True):
        o = run(nan_padded(clean, lens), lens, nan_padded(anchor, lens) if with_anchor else None)
        ref = R.ensemble(clean, lens, anchor if with_anchor else None)
        check_padding_and_nan(o, lens)
        for b, n in enumerate(lens):
            r = ref[b]
            a = (anchor[b] if with_anchor else clean[b, 0])[:, :n]
            for k in range(K):
                assert np.array_equal(o["gram"][b, k].cpu().numpy(), R.cross_gram_int(a, clean[b, k][:, :n]).astype(np.float64))
            assert np.array_equal(o["perm"][b].cpu().numpy(), r["perm"]), (b, with_anchor)
            assert np.array_equal(bits(o["mean"][b, :, :n]), bits(r["mean"]))
            # the spread from the exactly recomputed variance: sqrt and the rounding to float32 are correctly rounded on both sides
            assert np.array_equal(bits(o["std"][b, :, :n]), bits(np.sqrt(r["var64"]).astype(np.float32)))
            assert np.array_equal(bits64(o["dist"][b]), bits64(r["dist"]))
            assert int(o["medoid"][b]) == r["medoid"]
            assert np.array_equal(bits(o["pick"][b, :, :n]), bits(r["pick"]))


# ------------------------------------------------------------------------------------------------ 2. planted permutations
@pytest.mark.parametrize("S", [1, 2, 3])
@pytest.mark.parametrize("T", TS)
def test_planted_permutations(T, S):
    """(utterances shorter than 5 samples cannot hold a noisy plant — at T = 1 all three are: there the silence, identical-rows,
    anchor=None and permuted-anchor checks and the restatement still apply)"""
    rng = np.random.default_rng(7 * T + S)
    B, lens = 3, lengths_of(T)
    qs = R.perms(S)
    K = len(qs) + 2
    anchor = rng.standard_normal((B, S, T)).astype(np.float32)
    draws = np.zeros((B, K, S, T), np.float32)
    for b in range(B):
        for k, q in enumerate(qs):  # draw k: the anchor's rows in the order q_k, plus noise
            draws[b, k] = anchor[b][list(q)] + 0.1 * rng.standard_normal((S, T)).astype(np.float32)
        # draw S!: all silent.  draw S! + 1: its first and last rows identical (S = 1: just a row)
        draws[b, K - 1] = rng.standard_normal((S, T)).astype(np.float32)
        draws[b, K - 1, S - 1] = draws[b, K - 1, 0]
    o = run(nan_padded(draws, lens), lens, nan_padded(anchor, lens))
    check_padding_and_nan(o, lens)
    ref = R.ensemble(draws, lens, anchor)
    perm = o["perm"].cpu().numpy()
    for b, n in enumerate(lens):
        if n >= 5:  # (one sample of noise can outweigh the plant; the restatement is still matched below)
            for k, q in enumerate(qs):
                assert tuple(perm[b, k]) == tuple(np.argsort(q)), (b, k)  # undoes q_k: d[k][r[i]] = anchor[i] + noise
        assert tuple(perm[b, K - 2]) == tuple(range(S))  # silence: every candidate ties at zero, the identity stays
        g = o["gram"][b, K - 1].cpu().numpy()
        assert np.array_equal(g[:, 0], g[:, S - 1])  # identical rows: identical sums, bit for bit, so a genuine tie
        assert tuple(perm[b, K - 1]) == R.best_perm(g) == R.best_perm_brute(g)  # the earliest maximiser
        assert np.array_equal(perm[b], ref[b]["perm"]), b
    # anchor = None: draw 0 is the anchor and keeps its order by construction
    o = run(nan_padded(draws, lens), lens, None)
    assert np.array_equal(o["perm"][:, 0].cpu().numpy(), np.tile(np.arange(S, dtype=np.int32), (B, 1)))
    assert np.array_equal(o["perm"].cpu().numpy(), np.stack([r["perm"] for r in R.ensemble(draws, lens, None)]))
    # a caller's anchor that is the target permuted by p (row i of the target moved to row p[i]): draw 0 = the target gets
    # p's inverse, v_0[i] = d[0][pinv[i]] = target[pinv[i]] = anchor[i]
    p = {1: (0,), 2: (1, 0), 3: (1, 2, 0)}[S]
    pinv = tuple(np.argsort(p))
    target = draws[:, :1].copy()
    moved = np.zeros_like(anchor)
    for i in range(S):
        moved[:, p[i]] = target[:, 0, i]
    o = run(nan_padded(target, lens), lens, nan_padded(moved, lens))
    assert np.array_equal(o["perm"][:, 0].cpu().numpy(), np.tile(np.array(pinv, np.int32), (B, 1)))
    for b, n in enumerate(lens):
        assert np.array_equal(bits(o["mean"][b, :, :n]), bits(moved[b, :, :n]))


# ------------------------------------------------------------------------------------------------ 3. real values
def real_case(B, K, S, T, seed):
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((B, S, T)).astype(np.float32)
    draws = np.zeros((B, K, S, T), np.float32)
    for b in range(B):
        for k in range(K):
            draws[b, k] = base[b][rng.permutation(S)] + 0.3 * rng.standard_normal((S, T)).astype(np.float32)
    return draws


def test_real_values_against_float64():
    """K = 5, S = 3, T = 4099, lengths (4099, 1, 2733) against the float64 restatement; the worst ratio to each bound is
    printed.  Measured on an MI355X: gram 7.7e-4 of its bound, std 0 ulp, dist 1.4e-4 of its bound."""
    B, K, S, T, seed = 3, 5, 3, 4099, 20
    lens = lengths_of(T)
    draws = real_case(B, K, S, T, seed)
    ref = R.ensemble(draws, lens)
    o = run(nan_padded(draws, lens), lens)
    check_padding_and_nan(o, lens)
    worst = dict(gram=0.0, std=0.0, dist=0.0)
    for b, n in enumerate(lens):
        r = ref[b]
        # precondition on the restatement: the two smallest distances are further apart than the bound on either of them
        d = np.sort(r["dist"])
        rel = (S * n + 4) * 2.0 ** -52
        assert d[1] - d[0] > rel * (d[0] + d[1]), (b, d)
        # products of two float32 are exact in float64: only the additions round, fewer than n per entry
        gb = n * 2.0 ** -52 * r["gram_mag"]
        ge = np.abs(o["gram"][b].cpu().numpy() - r["gram"])
        worst["gram"] = max(worst["gram"], float(np.max(ge / gb)))
        assert np.all(ge <= gb), (b, ge / gb)
        assert np.array_equal(o["perm"][b].cpu().numpy(), r["perm"])
        # an in-order float64 add chain and one division: nothing a compiler could contract, nothing a summation order changes
        assert np.array_equal(bits(o["mean"][b, :, :n]), bits(r["mean"]))
        se = np.abs(o["std"][b, :, :n].cpu().numpy().astype(np.float64) - r["std"].astype(np.float64))
        sb = R.ulp32(r["std"])
        worst["std"] = max(worst["std"], float(np.max(se / sb)))
        assert np.all(se <= sb)
        # non-negative terms, one rounding in each and one per addition
        de = np.abs(o["dist"][b].cpu().numpy() - r["dist"])
        db = rel * r["dist"]
        worst["dist"] = max(worst["dist"], float(np.max(de / db)))
        assert np.all(de <= db), (b, de / db)
        assert int(o["medoid"][b]) == r["medoid"]
        assert np.array_equal(bits(o["pick"][b, :, :n]), bits(r["pick"]))
    print(f"K={K} S={S} T={T}: worst |gram - ref| / bound = {worst['gram']:.3e}, |std - ref| / ulp = {worst['std']:.3f}, "
          f"|dist - ref| / bound = {worst['dist']:.3e}")


# ------------------------------------------------------------------------------------------------ 4. independence
@pytest.mark.parametrize("K,S", [(5, 3), (4, 2)])
@pytest.mark.parametrize("T", [256, 257, 4099, 4100])
def test_batch_width_and_stream_independence(T, K, S):
    """every utterance of the B = 3 call, alone (B = 1, T = its length) on a side stream: the same bits in every output.  At
    T = 256 and 4100 the batch reads 16 bytes at a time and the lone utterances of odd length sample by sample."""
    B, lens = 3, lengths_of(T)
    draws = real_case(B, K, S, T, 31 * T + K)
    anchor = real_case(B, 1, S, T, T)[:, 0]
    for with_anchor in (False, True):
        o = run(nan_padded(draws, lens), lens, nan_padded(anchor, lens) if with_anchor else None)
        again = run(nan_padded(draws, lens), lens, nan_padded(anchor, lens) if with_anchor else None)
        for name in o:
            assert torch.equal(o[name].view(torch.uint8), again[name].view(torch.uint8)), name
        side = torch.cuda.Stream()
        for b, n in enumerate(lens):
            with torch.cuda.stream(side):
                solo = run(np.ascontiguousarray(draws[b:b + 1, :, :, :n]), None,
                           np.ascontiguousarray(anchor[b:b + 1, :, :n]) if with_anchor else None)
            side.synchronize()
            for name in ("mean", "std", "pick"):
                assert np.array_equal(bits(o[name][b, :, :n]), bits(solo[name][0])), (name, b, with_anchor)
            assert np.array_equal(bits64(o["gram"][b]), bits64(solo["gram"][0])), (b, with_anchor)
            assert np.array_equal(bits64(o["dist"][b]), bits64(solo["dist"][0])), (b, with_anchor)
            assert torch.equal(o["perm"][b], solo["perm"][0]) and int(o["medoid"][b]) == int(solo["medoid"][0])


# ------------------------------------------------------------------------------------------------ 5. K = 1
@pytest.mark.parametrize("S", [1, 2, 3])
@pytest.mark.parametrize("T", TS)
def test_one_draw_is_itself(T, S):
    B, lens = 3, lengths_of(T)
    draws = real_case(B, 1, S, T, T + S)
    o = run(nan_padded(draws, lens), lens)
    check_padding_and_nan(o, lens)
    for b, n in enumerate(lens):
        assert np.array_equal(bits(o["mean"][b, :, :n]), bits(draws[b, 0, :, :n]))
        assert np.array_equal(bits(o["pick"][b, :, :n]), bits(draws[b, 0, :, :n]))
    assert not bits(o["std"]).any() and not bits64(o["dist"]).any() and not o["medoid"].any()
    assert np.array_equal(o["perm"].cpu().numpy(), np.tile(np.arange(S, dtype=np.int32), (B, 1, 1)))


def test_ops_wrapper():
    B, K, S, T = 3, 4, 2, 257
    lens = lengths_of(T)
    draws = real_case(B, K, S, T, 3)
    o = run(nan_padded(draws, lens), lens)
    d = torch.from_numpy(nan_padded(draws, lens)).cuda()
    res = ops.ensemble(d, lengths=lens, want_std=True, want_pick=True, want_gram=True)
    for name in o:
        assert torch.equal(getattr(res, name).view(torch.uint8), o[name].view(torch.uint8)), name
    bare = ops.ensemble(d, lengths=lens)
    assert bare.std is None and bare.pick is None and bare.gram is None and torch.equal(bare.mean, res.mean)
    al = res.aligned(torch.from_numpy(draws).cuda())
    ref = R.ensemble(draws, lens)
    for b, n in enumerate(lens):
        assert np.array_equal(bits(al[b, :, :, :n]), bits(ref[b]["aligned"]))
    with pytest.raises(ValueError):
        ops.ensemble(d[0])
    with pytest.raises(_lib.DiffsepError, match="K = 33"):
        ops.ensemble(torch.zeros(1, 33, 2, 8, device="cuda"))


# ------------------------------------------------------------------------------------------------ 6. engine
def model16(dtype="f32"):
    m = DiffSepModel(default_config(nf=16), dtype=dtype)
    table = [(n, s) for n, s, _ in param_table(m.score_model.cfg)]
    sd = synth.synth_state_dict(table, 7)
    m.score_model.load_state_dict({"backbone." + k: torch.from_numpy(v) for k, v in sd.items()})
    return m.to("cuda:0")


def test_separate_draws_on_the_engine():
    m = model16()
    kw = dict(N=2, corrector_steps=1, snr=0.5)
    T, T1, K, seed = 4000, 3000, 3, 11
    assert m.engine().padded_frames(T) == m.engine().padded_frames(T1)
    mix = torch.from_numpy(synth.synth_mixture(0, T=T)[0]).cuda()[None]  # [1, 1, T]
    est, res, al = m.separate_draws(mix, K, seeds=[seed], out="all", **kw)
    assert est.shape == (1, 2, T) and al.shape == (1, K, 2, T) and bool(torch.isfinite(al).all())
    assert m.draws_info["seeds"] == [inflight.draw_seeds(seed, K)] and m.draws_info["K"] == K
    # the draws are the rows of the fused sampler on the mixture repeated K times under the file's seed
    (mix_n, _), mean, std = m.normalize_batch((mix, None))
    rows, *_ = m.get_pc_sampler("reverse_diffusion", "ald2", mix_n.repeat(K, 1, 1), seed=seed, lengths=[T] * K, **kw)()
    rows = m.denormalize_batch(rows, mean, std)[None]  # [1, K, S, T]
    assert np.array_equal(bits(al), bits(torch.gather(rows, 2, res.perm.long()[..., None].expand_as(rows))))
    # draw 0 keeps its order (it is the anchor) and is `separate` of the file alone with that seed
    assert res.perm[0, 0].tolist() == [0, 1]
    assert np.array_equal(bits(al[0, 0]), bits(m.separate(mix, seed=seed, **kw)[0]))
    # the mean is ops.ensemble of those rows
    again = ops.ensemble(rows)
    assert np.array_equal(bits(est), bits(again.mean)) and torch.equal(again.perm, res.perm) and torch.equal(again.dist, res.dist)
    medoid, res_m = m.separate_draws(mix, K, seeds=[seed], out="medoid", **kw)
    assert np.array_equal(bits(medoid), bits(al[:, int(res.medoid[0])])) and torch.equal(res_m.dist, res.dist)
    # two files of different lengths in one call: each is its solo result
    mix1 = torch.from_numpy(synth.synth_mixture(1, T=T1)[0]).cuda()[None]
    both = torch.zeros(2, 1, T, device="cuda")
    both[0], both[1, :, :T1] = mix[0], mix1[0]
    est2, res2, al2 = m.separate_draws(both, K, lengths=[T, T1], seeds=[seed, seed + 1], out="all", **kw)
    est1, res1, al1 = m.separate_draws(mix1, K, seeds=[seed + 1], out="all", **kw)
    assert np.array_equal(bits(est2[0]), bits(est[0])) and np.array_equal(bits(al2[0]), bits(al[0]))
    assert np.array_equal(bits(est2[1, :, :T1]), bits(est1[0])) and np.array_equal(bits(al2[1, :, :, :T1]), bits(al1[0]))
    assert not bits(est2[1, :, T1:]).any() and not bits(al2[1, :, :, T1:]).any()
    assert torch.equal(res2.dist, torch.cat([res.dist, res1.dist])) and torch.equal(res2.perm, torch.cat([res.perm, res1.perm]))
    # one 16-bit run of the same call
    h = model16("f16")
    est_h, res_h = h.separate_draws(both, K, lengths=[T, T1], seeds=[seed, seed + 1], **kw)
    assert est_h.shape == (2, 2, T) and bool(torch.isfinite(est_h).all()) and bool(torch.isfinite(res_h.dist).all())


# ------------------------------------------------------------------------------------------------ 7. CLIs
def test_separate_cli_draws(tmp_path):
    ind = tmp_path / "in"
    ind.mkdir()
    lens = {"a": 4000, "b": 3000}
    for i, (name, T) in enumerate(lens.items()):
        wavio.save(ind / f"{name}.wav", torch.from_numpy(synth.synth_mixture(i, T=T)[0]), 8000)
    common = ["--synthetic-weights", "16", "-N", "2", "--dtype", "f32", "--seed", "5"]
    sep_cli.main([str(ind), str(tmp_path / "plain"), "--batch", "2"] + common)
    sep_cli.main([str(ind), str(tmp_path / "one"), "--batch", "2", "--draws", "1"] + common)
    sep_cli.main([str(ind), str(tmp_path / "all"), "--batch", "6", "--draws", "3", "--draws-out", "all"] + common)
    for name, T in lens.items():
        for s in ("s0", "s1"):
            plain = (tmp_path / "plain" / s / f"{name}.wav").read_bytes()
            assert (tmp_path / "one" / s / f"{name}.wav").read_bytes() == plain  # --draws 1: the run without the flag
            mean, sr = wavio.load(tmp_path / "all" / s / f"{name}.wav")
            each = [wavio.load(tmp_path / "all" / s / f"{name}_draw{k}.wav")[0] for k in range(3)]
            assert sr == 8000 and mean.shape == (1, T) and all(d.shape == (1, T) for d in each)
            acc = each[0].numpy().astype(np.float64)
            for d in each[1:]:
                acc = acc + d.numpy().astype(np.float64)
            assert np.array_equal(bits(mean), bits((acc / 3.0).astype(np.float32)))
            assert not (tmp_path / "all" / s / f"{name}_draw3.wav").exists()
        # draw 0 is the file's ordinary output (the anchor keeps its source order)
        for s in ("s0", "s1"):
            assert (tmp_path / "all" / s / f"{name}_draw0.wav").read_bytes() == (tmp_path / "plain" / s / f"{name}.wav").read_bytes()


def test_evaluate_cli_draws(tmp_path):
    K, S = 3, 2
    for mode in ("mean", "medoid"):
        out = tmp_path / mode
        eval_cli.main(["--synthetic", "2", "--synthetic-weights", "16", "-N", "2", "--dtype", "f32", "--samples", "4000", "--batch", "6",
                       "--streams", "1", "--no-stoi", "--save-n", "0", "--flat-output", "-o", str(out), "--draws", str(K),
                       "--draws-out", mode])
        recs = json.loads((out / "test.json").read_text())
        summary = json.loads((out / "test_summary.json").read_text())
        assert len(recs) == 2 and summary["draws"] == K and summary["draws_out"] == mode
        for r in recs:
            assert np.asarray(r["si_sdr_draws"]).shape == (K, S) and len(r["si_sdr_mean"]) == S and len(r["si_sdr_medoid"]) == S
            assert len(r["draws_dist"]) == K and 0 <= r["draws_medoid"] < K
            assert r["draws_medoid"] == int(np.argmin(r["draws_dist"]))
            assert r["si_sdr_draws"][r["draws_medoid"]] == r["si_sdr_medoid"]
            assert r["si_sdr"][0] == (r["si_sdr_mean"] if mode == "mean" else r["si_sdr_medoid"])
            assert r["runtime"] > 0 and np.all(np.isfinite(r["si_sdr_draws"]))
        for name in ("si_sdr_draws", "si_sdr_mean", "si_sdr_medoid", "draws_dist"):
            assert np.isclose(summary[name], np.mean([np.mean(r[name]) for r in recs]))
        assert "draws_medoid" not in summary
