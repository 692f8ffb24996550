"""The host side of the sampler's tap (no GPU): metrics.si_bss_from_gram against the scale-invariant definitions written out
per waveform in float64, the figure's panel steps against the reference's expression, figures.evolution_figure on stand-in
arrays, and the refusals of evaluate --fig / --trajectory."""
import itertools

import numpy as np
import pytest

from diffsep_amd import evaluate as eval_cli
from diffsep_amd import figures, metrics


def _db(num, den):
    return 10.0 * np.log10(num / den)


def si_bss_time_domain(ref, est):
    """[S,S,3]: SI-SDR / SI-SIR / SI-SAR of estimate j against reference i, by projections of the waveforms (float64)"""
    S = ref.shape[0]
    out = np.zeros((S, S, 3))
    for j in range(S):
        coef = np.linalg.lstsq(ref.T, est[j], rcond=None)[0]
        e_proj = coef @ ref
        for i in range(S):
            s_target = (est[j] @ ref[i]) / (ref[i] @ ref[i]) * ref[i]
            e_interf, e_artif = e_proj - s_target, est[j] - e_proj
            out[i, j] = (_db(s_target @ s_target, (est[j] - s_target) @ (est[j] - s_target)),
                         _db(s_target @ s_target, e_interf @ e_interf), _db(e_proj @ e_proj, e_artif @ e_artif))
    return out


def gram_numpy(ref, est):
    """[B,3,S,S] float64 = {ref ref^T, ref est^T, est est^T}"""
    return np.stack([np.stack([r @ r.T, r @ e.T, e @ e.T]) for r, e in zip(ref, est)])


@pytest.mark.parametrize("shape", [(3, 2, 500), (2, 3, 400)])
def test_si_bss_from_gram_matches_the_definitions(shape):
    B, S, T = shape
    rng = np.random.default_rng(11)
    ref = rng.standard_normal(shape)
    mixing = np.eye(S)[::-1] + 0.3 * rng.standard_normal((B, S, S))  # estimates: the sources swapped and leaking, plus noise
    est = mixing @ ref + 0.2 * rng.standard_normal(shape)
    sdr, sir, sar, perm = metrics.si_bss_from_gram(gram_numpy(ref, est))
    for b in range(B):
        want = si_bss_time_domain(ref[b], est[b])
        best = max(itertools.permutations(range(S)), key=lambda p: np.mean([want[i, p[i], 0] for i in range(S)]))
        assert tuple(perm[b]) == best
        for i in range(S):
            got = (sdr[b, i], sir[b, i], sar[b, i])
            assert np.max(np.abs(np.array(got) - want[i, best[i]])) < 1e-9, (b, i, got, want[i, best[i]])


def test_si_bss_from_gram_with_a_fixed_permutation():
    B, S, T = 3, 3, 400
    rng = np.random.default_rng(5)
    ref = rng.standard_normal((B, S, T))
    est = ref[:, ::-1] + 0.5 * rng.standard_normal((B, S, T))
    perms = [[1, 2, 0], [0, 1, 2], [2, 0, 1]]  # not the best ones
    sdr, sir, sar, perm = metrics.si_bss_from_gram(gram_numpy(ref, est), perm=perms)
    assert perm.tolist() == perms
    # the same thing by reordering the estimates first and reading the identity assignment
    est_p = np.stack([est[b, perms[b]] for b in range(B)])
    for b in range(B):
        want = si_bss_time_domain(ref[b], est_p[b])
        for i in range(S):
            assert np.max(np.abs(np.array([sdr[b, i], sir[b, i], sar[b, i]]) - want[i, i])) < 1e-9
    ident = metrics.si_bss_from_gram(gram_numpy(ref, est_p), perm=[list(range(S))] * B)
    for a, b_ in zip((sdr, sir, sar), ident[:3]):
        assert np.max(np.abs(a - b_)) < 1e-9


@pytest.mark.parametrize("N", [1, 2, 5, 6, 30])
def test_panel_steps_are_the_reference_expression(N):
    n_fig = 6
    intmet = list(range(N))  # evaluate.py:37 takes the steps from the length of the list of intermediates
    want = np.round(np.linspace(0, 1, n_fig) * (len(intmet) - 1)).astype(np.int64)
    got = figures.panel_steps(N)
    assert got.dtype == np.int64 and got.tolist() == want.tolist()
    if N == 30:
        assert got.tolist() == [0, 6, 12, 17, 23, 29]
    steps, panel_of = figures.snapshot_request(N)
    assert all(a < b for a, b in zip(steps, steps[1:])) and 0 <= steps[0] and steps[-1] < N
    assert [steps[p] for p in panel_of] == want.tolist()


def test_snapshot_request_for_two_steps():
    steps, panel_of = figures.snapshot_request(2)
    assert steps == [0, 1]
    assert panel_of == [0, 0, 0, 1, 1, 1]  # round(0, .2, .4, .6, .8, 1) half-to-even
    assert [figures.panel_time(2, steps[p]) for p in panel_of] == [1.0, 1.0, 1.0, 0.0, 0.0, 0.0]
    assert figures.panel_time(1, 0) == 1.0


def test_evolution_figure_on_stand_in_arrays(tmp_path):
    pytest.importorskip("matplotlib")
    S, T, N = 2, 4000, 30
    rng = np.random.default_rng(2)
    states = 0.1 * rng.standard_normal((figures.N_FIG, S, T))
    target = np.stack([np.sin(0.3 * np.arange(T)), np.zeros(T)])  # (an all-zero target row)
    steps = figures.panel_steps(N)
    a = figures.evolution_figure(states, steps, N, target, tmp_path / "a.pdf")
    np.random.seed(123)  # the global state is not what the "clean" column's noise comes from
    np.random.randn(7)
    b = figures.evolution_figure(states, steps, N, target, tmp_path / "b.pdf")
    for name in ("a.pdf", "b.pdf"):
        assert (tmp_path / name).read_bytes().startswith(b"%PDF")
    assert a["axes"] == b["axes"] == S * (figures.N_FIG + 1) + 1
    assert len(a["clean"]) == S and all(np.array_equal(x, y) for x, y in zip(a["clean"], b["clean"]))
    assert np.max(np.abs(a["clean"][1])) < 1e-8 and np.any(a["clean"][1] != 0)  # zero row + 1e-10 noise


@pytest.mark.parametrize("argv, flag", [
    (["--fig", "--sampler", "ode", "--synthetic", "2", "--synthetic-weights", "16"], "--fig"),
    (["--trajectory", "--sampler", "ode", "--synthetic", "2", "--synthetic-weights", "16"], "--trajectory"),
    (["__no_proc__", "--trajectory", "--synthetic", "2"], "--trajectory"),
    (["__no_proc__", "--fig", "--synthetic", "2"], "--fig"),
])
def test_evaluate_refuses_by_name(argv, flag, tmp_path):
    with pytest.raises(SystemExit) as exc:
        eval_cli.main(argv + ["-o", str(tmp_path)])
    assert str(exc.value).startswith(flag + ":")
    assert not any(tmp_path.iterdir())  # refused before anything was set up


def test_fig_without_matplotlib_exits_naming_it(monkeypatch, tmp_path):
    import builtins
    real = builtins.__import__

    def no_mpl(name, *a, **k):
        if name == "matplotlib" or name.startswith("matplotlib."):
            raise ImportError("No module named 'matplotlib'")
        return real(name, *a, **k)
    monkeypatch.setattr(builtins, "__import__", no_mpl)
    with pytest.raises(SystemExit) as exc:
        eval_cli.main(["--fig", "--synthetic", "2", "--synthetic-weights", "16", "-o", str(tmp_path)])
    assert "matplotlib" in str(exc.value) and "--fig" in str(exc.value)
