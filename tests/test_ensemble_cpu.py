"""Posterior draws without a GPU: the numpy restatement against brute force, the host side of diffsep_ensemble (workspace
arithmetic, every refusal — checked before the first device call), the draws' seeds and the CLIs' argument checks."""
import ctypes as C

import numpy as np
import pytest

import ensemble_ref as R
from diffsep_amd import _lib, inflight
from diffsep_amd import evaluate as eval_cli
from diffsep_amd import separate as sep_cli


@pytest.mark.parametrize("S", [1, 2, 3])
def test_permutation_search_equals_brute_force(S):
    rng = np.random.default_rng(S)
    assert R.perms(3) == [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]
    for trial in range(300):
        c = rng.standard_normal((S, S))
        if trial % 3 == 1:
            c = rng.integers(-2, 3, (S, S)).astype(np.float64)  # small integers: ties are common
        if trial % 3 == 2:
            c[:, -1] = c[:, 0]  # two identical columns (two identical rows of a draw): always a tie
        assert R.best_perm(c) == R.best_perm_brute(c), c
    assert R.best_perm(np.zeros((S, S))) == tuple(range(S))  # an all-silent draw keeps the identity


def test_restatement_on_a_planted_case():
    rng = np.random.default_rng(0)
    a = rng.standard_normal((3, 64)).astype(np.float32)
    q = [(0, 1, 2), (2, 0, 1), (1, 0, 2), (2, 1, 0)]
    draws = np.stack([a[list(p)] for p in q])  # draw k = the anchor's rows in order q_k, exactly
    r = R.ensemble_one(draws)
    assert [tuple(p) for p in r["perm"]] == [tuple(np.argsort(p)) for p in q]
    assert np.array_equal(r["mean"], a) and not r["std"].any() and not r["dist"].any() and r["medoid"] == 0
    assert np.array_equal(r["pick"], a)


def test_workspace_bytes_positive_and_monotone():
    l = _lib.lib()
    for S in (1, 2, 3):
        prev = 0
        for B in (1, 2, 3, 16, 64):
            n = l.diffsep_ensemble_workspace_bytes(B, 4, S)
            assert n > prev
            prev = n
        prev = 0
        for K in (1, 2, 3, 4, 5, 31, 32):
            n = l.diffsep_ensemble_workspace_bytes(3, K, S)
            assert n > prev
            prev = n
    for (B, K, S), word in (((1, 0, 2), b"K"), ((1, 33, 2), b"K"), ((1, 4, 0), b"S"), ((1, 4, 4), b"S"), ((0, 4, 2), b"B")):
        assert l.diffsep_ensemble_workspace_bytes(B, K, S) == -1
        assert word + b" = " in l.diffsep_last_error(), l.diffsep_last_error()


def test_refusals_need_no_device():
    """every refusal is decided before the first device call: dummy addresses stand in for device memory, nothing is touched"""
    l = _lib.lib()
    B, K, S, T = 2, 4, 2, 100
    need = l.diffsep_ensemble_workspace_bytes(B, K, S)
    dummy = C.c_void_p(4096)
    names = ("draws", "anchor", "lengths", "mean_out", "std_out", "pick_out", "perm_out", "dist_out", "medoid_out", "gram_out",
             "workspace")

    def call(B_=B, K_=K, S_=S, T_=T, nbytes=need, null=None):
        p = {n: (None if n == null else dummy) for n in names}
        return l.diffsep_ensemble(p["draws"], p["anchor"], p["lengths"], B_, K_, S_, T_, p["mean_out"], p["std_out"], p["pick_out"],
                                  p["perm_out"], p["dist_out"], p["medoid_out"], p["gram_out"], p["workspace"], nbytes, None)

    cases = [(dict(K_=0), b"K = 0"), (dict(K_=33), b"K = 33"), (dict(S_=0), b"S = 0"), (dict(S_=4), b"S = 4"),
             (dict(B_=0), b"B = 0"), (dict(T_=0), b"T = 0"), (dict(nbytes=need - 1), b"workspace_bytes"),
             (dict(nbytes=0), b"workspace_bytes")]
    cases += [(dict(null=n), n.encode() + b" is null") for n in ("draws", "mean_out", "perm_out", "dist_out", "medoid_out",
                                                                 "workspace")]
    for kw, word in cases:
        assert call(**kw) != 0, kw
        assert b"ensemble" in l.diffsep_last_error() and word in l.diffsep_last_error(), (kw, l.diffsep_last_error())


def test_draw_seeds():
    stride = 0x9E3779B97F4A7C15
    assert inflight.WINDOW_SEED_STRIDE == stride
    for s in (0, 5, 2 ** 62 - 1, 2 ** 64 - 3):
        seeds = inflight.draw_seeds(s, 5)
        assert seeds[0] == s and len(seeds) == 5
        assert seeds == [(s + stride * k) % 2 ** 64 for k in range(5)]
        assert all(0 <= v < 2 ** 64 for v in seeds)
    assert inflight.draw_seeds(7, 1) == [7] and inflight.draw_seeds(7, 3) == inflight.window_seeds(7, 3)


def test_draw_batches_hold_whole_files():
    lengths = [32000] * 7
    groups = inflight.plan_draw_batches(range(7), lengths, lambda T: 256, 16, 4)
    assert [len(g) for g in groups] == [4, 3] and sorted(i for g in groups for i in g) == list(range(7))
    assert [len(g) for g in inflight.plan_draw_batches(range(7), lengths, lambda T: 256, 4, 3)] == [1] * 7
    with pytest.raises(ValueError, match="--draws 5 does not fit --batch 4"):
        inflight.plan_draw_batches(range(7), lengths, lambda T: 256, 4, 5)


@pytest.mark.parametrize("mode", ["mean", "medoid", "all"])
def test_overflow_net_sees_every_draw_whatever_is_written(mode):
    """An overflow in draw 1 makes the mean non-finite there and every distance NaN, so the medoid search keeps draw 0, which
    is finite: the request hands the MEAN to the overflow net (element 0 of its result), not the estimate that is written."""
    import torch
    from diffsep_amd import ops
    from diffsep_amd.pl_model import DiffSepModel
    draws = torch.ones(1, 3, 2, 8)
    draws[0, 1, 0, 5] = float("inf")
    mean = draws.double().mean(1).float()
    res = ops.EnsembleResult(mean, None, draws[:, 0].clone(), torch.zeros(1, 3, 2, dtype=torch.int32),
                             torch.full((1, 3), float("nan"), dtype=torch.float64), torch.zeros(1, dtype=torch.int32), None)
    seen = {}

    class Model:
        dtype, fallback_batches = "f16", 0
        has_fallback = DiffSepModel.has_fallback
        rerun_if_nonfinite = DiffSepModel.rerun_if_nonfinite

        def __init__(self, finite=False):
            self.finite = finite

        def fallback_model(self):
            return Model(finite=True)

        def separate_draws(self, mix, K, out="mean", **kw):
            seen.update(kw, out=out, K=K)
            r = ops.EnsembleResult(torch.ones(1, 2, 8), None, res.pick, res.perm, res.dist, res.medoid, None) if self.finite else res
            est = r.pick if out == "medoid" else r.mean
            return (est, r, draws) if out == "all" else (est, r)

    request = lambda model: sep_cli.draws_request(model, None, 3, [8], [5], mode, {"N": 2})
    first = request(Model())
    assert first[0] is res.mean and not bool(torch.isfinite(first[0]).all())
    assert bool(torch.isfinite(res.pick).all())  # the medoid alone would have passed
    assert seen["out"] == mode and seen["check_finite"] is False and seen["rescale"] is sep_cli.scale_draws and seen["N"] == 2
    m = Model()
    with pytest.warns(RuntimeWarning, match="non-finite"):
        again = m.rerun_if_nonfinite(first, request, what="a test")
    assert m.fallback_batches == 1 and bool(torch.isfinite(again[0]).all()) and (again[3] is not None) == (mode == "all")


def test_separate_argument_checks(tmp_path):
    """refused at argument parsing, by name: before a GPU, a model or a file is looked for"""
    io = [str(tmp_path / "in"), str(tmp_path / "out")]

    def refused(*argv):
        with pytest.raises(SystemExit) as e:
            sep_cli.main(io + list(argv))
        return str(e.value)

    msg = refused("--draws", "3", "--chunk", "4", "--batch", "4")
    assert "--draws" in msg and "--chunk" in msg
    msg = refused("--draws", "3", "--sampler", "ode", "--batch", "4")
    assert "--draws" in msg and "--sampler ode" in msg
    msg = refused("--draws", "5", "--batch", "4")
    assert "--draws 5" in msg and "--batch 4" in msg
    assert "--draws" in refused("--draws", "0", "--batch", "4") and "--draws" in refused("--draws", "33", "--batch", "64")
    assert "--draws-out" in refused("--draws-out", "all")
    assert not (tmp_path / "out").exists()


def test_evaluate_argument_checks(tmp_path):
    base = ["--synthetic", "2", "--synthetic-weights", "16", "-o", str(tmp_path / "out")]

    def refused(*argv):
        with pytest.raises(SystemExit) as e:
            eval_cli.main(base + list(argv))
        return str(e.value)

    msg = refused("--draws", "3", "--sampler", "ode")
    assert "--draws" in msg and "--sampler ode" in msg
    msg = refused("--draws", "3", "--trajectory")
    assert "--draws" in msg and "--trajectory" in msg
    msg = refused("--draws", "5", "--batch", "4")
    assert "--draws 5" in msg and "--batch 4" in msg
    assert "--draws-out" in refused("--draws-out", "medoid")
    args = eval_cli.build_parser().parse_args(base)
    assert args.draws is None and args.draws_out is None  # off by default
    assert not (tmp_path / "out").exists()
