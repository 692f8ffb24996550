"""diffsep_amd.inflight — what evaluate and separate share to keep K batches in flight — on stand-in streams, engines and
models: the order of launches, synchronises and collects of the ring, the overflow re-run, the seed formula, worker
set-up (engines before streams), the workspace reserve and the per-utterance normalisation.  No GPU involved."""
import argparse
import contextlib

import pytest
import torch

from diffsep_amd import evaluate, inflight
from diffsep_amd.pl_model import DiffSepModel, default_config


class _Stream:
    def __init__(self, log, name=None):
        self.log, self.name = log, name
        log.append(("stream", name))

    def synchronize(self):
        self.log.append(("sync", self))


class _Engine:
    def __init__(self, log, what):
        self.reserved = []
        log.append(("engine", what))

    def padded_frames(self, T):
        return 64 * ((1 + (T + 382) // 128 + 63) // 64)

    def bucket_length(self, W):
        return 128 * W - 383

    def reserve(self, B, T):
        self.reserved.append((B, T))


class _ScoreModel:
    def __init__(self, log):
        self.log, self._e = log, None

    def engine(self):
        self._e = self._e or _Engine(self.log, "score")
        return self._e


class _Model:
    """engines are made lazily, like the real model's; rerun_if_nonfinite IS the real model's"""

    def __init__(self, log, hybrid=False, dtype="f16"):
        self.log, self.hybrid, self.dtype, self.throughput, self._tail = log, hybrid, dtype, False, None
        self.config = default_config(nf=16)
        self.score_model = _ScoreModel(log)

    def replica(self):
        return _Model(self.log, self.hybrid, self.dtype)

    def set_throughput_mode(self, on=True):
        self.throughput = on

    def tail_engine(self):
        if self.hybrid:
            self._tail = self._tail or _Engine(self.log, "tail")
        return self._tail

    def fallback_model(self):
        return None if self.dtype == "split" else _Model(self.log, dtype="split")

    rerun_if_nonfinite = DiffSepModel.rerun_if_nonfinite

    def normalize_batch(self, batch):
        mix, tgt = batch
        mean, std = mix.mean(dim=(1, 2), keepdim=True), mix.std(dim=(1, 2), keepdim=True).clamp(min=1e-5)
        return ((mix - mean) / std, None if tgt is None else (tgt - mean) / std), mean, std


@pytest.fixture
def device(monkeypatch):
    """torch.cuda's stream calls replaced by recording stand-ins -> (log, list whose last entry is the current stream)"""
    log, current = [], ["default"]

    @contextlib.contextmanager
    def stream(s):
        current.append(s)
        try:
            yield
        finally:
            current.pop()
    monkeypatch.setattr(torch.cuda, "Stream", lambda: _Stream(log))
    monkeypatch.setattr(torch.cuda, "stream", stream)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda: _Stream(log, "current"))
    return log, current


@pytest.mark.parametrize("K,n", [(1, 3), (2, 7), (4, 7), (4, 2)])
def test_ring_order_and_overflow_rerun(device, K, n):
    log, current = device
    streams = [torch.cuda.Stream() for _ in range(K)]
    model = _Model(log)
    bad = n // 2  # this batch's first result is non-finite
    reissued, seen = [], {}

    def launch(w, j, group):
        assert current[-1] is streams[w] and group == [10 * j]
        log.append(("launch", w, j))
        return j, torch.tensor([float("inf") if j == bad else float(j)])

    def reissue(fb, w, j):
        assert current[-1] is streams[w] and fb.dtype == "split"
        log.append(("reissue", w, j))
        reissued.append(j)
        return (torch.tensor([100.0 + j]),)

    def collect(w, item):
        j, x = item
        assert log[-1] == ("sync", streams[w])  # the worker's stream was drained first
        log.append(("collect", w, j))
        with pytest.warns(RuntimeWarning) if j == bad else contextlib.nullcontext():
            (x,) = inflight.finite_or_rerun(model, streams[w], (x,), lambda fb: reissue(fb, w, j), what=f"batch {j}")
        seen[j] = float(x)

    inflight.Ring(streams, launch, collect).run([[10 * j] for j in range(n)])

    ev = [e for e in log if e[0] in ("launch", "collect")]
    assert sorted(e[2] for e in ev if e[0] == "launch") == list(range(n)) == sorted(e[2] for e in ev if e[0] == "collect")
    assert all(w == j % K for _, w, j in ev)
    in_flight = 0
    for e in ev:
        in_flight += 1 if e[0] == "launch" else -1
        assert 0 <= in_flight <= K
        if e[0] == "launch" and e[2] >= K:  # worker w's previous batch was collected before this one went onto it
            assert ev.index(("collect", e[1], e[2] - K)) < ev.index(e)
    # after the last launch the workers are drained in index order
    tail = ev[ev.index(("launch", (n - 1) % K, n - 1)) + 1:]
    assert [e[0] for e in tail] == ["collect"] * len(tail) and [e[1] for e in tail] == sorted(e[1] for e in tail)
    assert len(tail) == min(K, n)
    # the non-finite batch was re-issued once, on its worker's stream, which was drained again before the result was used;
    # collect saw the repeat's result, every other batch its own
    assert reissued == [bad]
    at = log.index(("reissue", bad % K, bad))
    assert log[at + 1] == ("sync", streams[bad % K])
    assert seen == {j: (100.0 + j if j == bad else float(j)) for j in range(n)}


def test_overflow_rerun_raises_when_the_repeat_is_non_finite_too(device):
    log, _ = device
    with pytest.warns(RuntimeWarning), pytest.raises(FloatingPointError):
        inflight.finite_or_rerun(_Model(log), torch.cuda.Stream(), (torch.tensor([float("nan")]),),
                                 lambda fb: (torch.tensor([float("inf")]),), what="a batch")


@pytest.mark.parametrize("n,seed", [(0, 0), (1, 5), (13, 5), (512, 0), (7, 2 ** 40 + 3)])
def test_utterance_seeds_formula(n, seed):
    want = torch.randint(0, 2 ** 62, (max(n, 1),), generator=torch.Generator().manual_seed(seed)).tolist()
    assert inflight.utterance_seeds(n, seed) == want


@pytest.mark.parametrize("K", [1, 2, 4])
def test_setup_workers_creates_every_engine_before_the_first_stream(device, K):
    log, _ = device
    model = _Model(log, hybrid=True)
    models, streams = inflight.setup_workers(model, K)
    assert models[0] is model and len(models) == len(streams) == K and len(set(map(id, models))) == K
    assert all(m.throughput == (K > 1) for m in models)
    kinds = [e[0] for e in log]
    assert kinds == ["engine"] * (2 * K) + ["stream"] * K  # a score and a tail engine per model, THEN the streams
    assert all(m.score_model._e is not None and m._tail is not None for m in models)
    # nothing to separate with: streams only
    assert inflight.setup_workers(None, K)[0] == []


def test_setup_workers_single_worker_on_the_current_stream(device):
    log, _ = device
    models, streams = inflight.setup_workers(_Model(log), 1, own_stream=False)
    assert len(models) == 1 and [s.name for s in streams] == ["current"] and not models[0].throughput
    assert [e[0] for e in log] == ["engine", "stream"]
    assert [s.name for s in inflight.setup_workers(_Model(log), 2, own_stream=False)[1]] == [None, None]


def test_reserve_largest_covers_every_engine(device):
    log, _ = device
    models, _ = inflight.setup_workers(_Model(log, hybrid=True), 3)
    lengths = [8000, 30000, 7000, 31000, 12000]
    eng = models[0].score_model.engine()
    batches = inflight.plan_batches(range(5), lengths, eng.padded_frames, 2)
    inflight.reserve_largest(models, batches, lengths)
    want = [(2, eng.bucket_length(eng.padded_frames(31000)))]
    assert all(m.score_model.engine().reserved == want and m.tail_engine().reserved == want for m in models)
    inflight.reserve_largest(models, [], lengths)  # nothing planned: nothing reserved
    assert models[0].score_model.engine().reserved == want


def test_normalize_padded_is_per_utterance_over_its_samples(device):
    model, g = _Model(device[0]), torch.Generator().manual_seed(3)
    lens = [50, 31, 8]
    mix, tgt = torch.zeros(3, 1, 64), torch.zeros(3, 2, 64)
    for b, L in enumerate(lens):
        mix[b, :, :L], tgt[b, :, :L] = torch.randn(1, L, generator=g) * (b + 1) + b, torch.randn(2, L, generator=g)
    mix_n, tgt_n = inflight.normalize_padded(model, lens, mix, tgt)
    for b, L in enumerate(lens):
        (m, t), *_ = model.normalize_batch((mix[b:b + 1, :, :L], tgt[b:b + 1, :, :L]))
        assert torch.equal(mix_n[b, :, :L], m[0]) and torch.equal(tgt_n[b, :, :L], t[0])
        assert not mix_n[b, :, L:].any() and not tgt_n[b, :, L:].any()
    only_mix, none = inflight.normalize_padded(model, lens, mix)
    assert none is None and torch.equal(only_mix, mix_n)


def test_settings_arguments_and_the_names_evaluate_keeps():
    cfg = default_config(nf=16)
    cfg["model"]["sampler"] = {"N": 17, "corrector_steps": 2, "snr": 0.25}
    ns = argparse.Namespace(N=None, corrector_steps=None, snr=None)
    assert inflight.sampler_settings(cfg, ns) == (17, 2, 0.25)
    assert inflight.sampler_settings(cfg, argparse.Namespace(N=3, corrector_steps=0, snr=0.1)) == (3, 0, 0.1)
    ap = argparse.ArgumentParser()
    inflight.add_precision_arguments(ap)
    got = ap.parse_args(["--dtype", "hybrid", "--fp32-steps", "4"])
    assert (got.dtype, got.fp32_steps) == ("hybrid", 4) and ap.parse_args([]).dtype == "auto"
    ev = evaluate.build_parser().parse_args(["--synthetic", "2"])
    assert (ev.dtype, ev.fp32_steps) == ("auto", None)
    assert evaluate.plan_batches is inflight.plan_batches
