"""The fused sampler's tap on the MI355X (diffsep_pc_sample_trace, Engine.pc_sample(snapshots=, target=),
sdes.get_pc_sampler(snapshots=, target=), evaluate --fig / --trajectory): snapshots of chosen reverse steps and the Gram
sums of every step against a target, taken between the corrector and the predictor of a step.  nf = 16, S = 2, synthetic
weights of seed 7; N <= 3, T between 4000 and 7000.

test_snapshots_equal_the_generic_loop: both paths run the same launchers on the same draws, and a replayed graph equals the
eager evaluation bitwise, so on the f32 engine every (xt, xt_mean) and the result are asserted bit for bit (the two paths'
final results were bit-identical before the tap existed)."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from diffsep_amd import _lib, metrics, ops, sdes, synth
from diffsep_amd import evaluate as eval_cli
from diffsep_amd.engine import Engine, pack_state_dict, param_table
from diffsep_amd.pl_model import DiffSepModel, default_config
from diffsep_amd.sdes import noise as sde_noise

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

NF, S = 16, 2
MIX = dict(kind=_lib.SDE_MIX, ndim=2, d_lambda=2.0, sigma_min=0.05, sigma_max=0.5)
LENS = [7000, 6500, 6017]  # 58, 54, 51 frames: one padded width (64) for all
SEEDS = [101, 202, 303]
KW = dict(N=3, corrector_steps=1, snr=0.5, eps=0.03)
_cache = {}


def engine(dtype=_lib.F32, lib_kind=None):
    if ("eng", dtype, lib_kind) not in _cache:
        cfg = _lib.model_config(nf=NF, num_sources=S, dtype=dtype)
        sd = synth.synth_state_dict([(n, s) for n, s, _ in param_table(cfg)], 7)
        _cache["eng", dtype, lib_kind] = Engine(cfg, pack_state_dict(cfg, sd), lib_kind=lib_kind)
    return _cache["eng", dtype, lib_kind]


def model16():
    if "model" not in _cache:
        m = DiffSepModel(default_config(nf=NF), dtype="f32")
        sd = synth.synth_state_dict([(n, s) for n, s, _ in param_table(m.score_model.cfg)], 7)
        m.score_model.load_state_dict({"backbone." + k: torch.from_numpy(v) for k, v in sd.items()})
        _cache["model"] = m.to("cuda:0")
    return _cache["model"]


def padded():
    """the three utterances as one right-zero-padded batch: (mix_norm [3,1,7000], target [3,S,7000], zero beyond LENS)"""
    if "padded" not in _cache:
        T = max(LENS)
        mixn, tgt = torch.zeros(len(LENS), 1, T, device="cuda"), torch.zeros(len(LENS), S, T, device="cuda")
        for b, L in enumerate(LENS):
            mix_b, tgt_b = synth.synth_mixture(b, T=L)
            mix_b = torch.from_numpy(mix_b)[None].cuda()
            mixn[b, :, :L] = ops.normalize_batch(mix_b)[0][0]
            tgt[b, :, :L] = torch.from_numpy(tgt_b).cuda() / mix_b.std()
        _cache["padded"] = (mixn, tgt)
    return _cache["padded"]


def traced_all():
    """the mixed-length batch on the f32 engine, every step kept, with a target: (out, nfe, trace); computed once"""
    if "all" not in _cache:
        mixn, tgt = padded()
        _cache["all"] = engine().pc_sample(mixn, MIX, **KW, lengths=LENS, seeds=SEEDS, snapshots="all", target=tgt)
    return _cache["all"]


# ---------------------------------------------------------------- 1. against the generic loop
class Injected:
    """the draws of the step-by-step loop (sdes/noise.py) from a list"""
    def __init__(self, draws):
        self.draws, self.i = list(draws), 0

    def __enter__(self):
        def nxt(shape, like):
            z = self.draws[self.i]
            self.i += 1
            assert tuple(z.shape) == tuple(shape)
            return z.to(like.device)
        self.prev = sde_noise.set_source(nxt)
        return self

    def __exit__(self, *a):
        sde_noise.set_source(self.prev)


@pytest.mark.parametrize("sde_name", ["mix", "priormix"])
@pytest.mark.parametrize("csteps", [1, 2])
def test_snapshots_equal_the_generic_loop(sde_name, csteps):
    m = model16()
    B, T, N = 2, 4000, 3
    sde_kw = dict(ndim=2, d_lambda=2.0, sigma_min=0.05, sigma_max=0.5, N=N)
    sde = sdes.MixSDE(**sde_kw) if sde_name == "mix" else sdes.PriorMixSDE(**sde_kw, avg_len=510)
    mix = torch.from_numpy(synth.synth_batch(B, T=T)[0]).cuda()
    (mixn, _), *_ = m.normalize_batch((mix, None))
    n_draws = 1 + N * (csteps + 1)
    draws = [torch.from_numpy(synth.synth_noise(f"trace.{sde_name}.{csteps}.z{i}", (B, S, T))).cuda() for i in range(n_draws)]
    with Injected(draws) as inj:
        x_ref, ns, im = sdes.get_pc_sampler("reverse_diffusion", "ald2", sde, m, mixn, snr=0.5, eps=0.03,
                                            corrector_steps=csteps, intermediate=True)()
        assert inj.i == n_draws
    out, nfe, tr = m.engine().pc_sample(mixn, sde.engine_config(), N=N, corrector_steps=csteps, snr=0.5, eps=0.03,
                                        noise=torch.stack(draws), snapshots="all")
    assert nfe == ns == N * (csteps + 1) and tr.steps == [0, 1, 2] and len(im) == N and tr.gram is None
    for i, (xt, xm) in enumerate(im):
        d = float((tr.x[i] - xt).abs().max()), float((tr.x_mean[i] - xm).abs().max())
        print(f"step {i}: max |x - x_loop| {d[0]:.3e}, max |x_mean - x_mean_loop| {d[1]:.3e}")
        assert torch.equal(tr.x[i], xt) and torch.equal(tr.x_mean[i], xm), (i, d)
    assert torch.equal(out, x_ref)


# ---------------------------------------------------------------- 2. the tap changes nothing
@pytest.mark.parametrize("mode", ["f32", "f16", "f16+head"])
def test_the_tap_does_not_change_the_result(mode):
    mixn, tgt = padded()
    eng = engine() if mode == "f32" else engine(_lib.F16)
    extra = dict(tail=engine(_lib.F32_SPLIT, "f16"), head_steps=1) if mode == "f16+head" else {}
    plain, nfe = eng.pc_sample(mixn, MIX, **KW, lengths=LENS, seeds=SEEDS, **extra)
    out, nfe2, tr = eng.pc_sample(mixn, MIX, **KW, lengths=LENS, seeds=SEEDS, snapshots="all", target=tgt, **extra)
    assert nfe == nfe2 == 6 and torch.isfinite(out).all()
    assert torch.equal(out, plain)
    assert tr.x.shape == (3, 3, S, 7000) and tr.gram.shape == (4, 3, 3, S, S)
    assert torch.equal(tr.gram[3], ops.gram(tgt, out))
    if mode == "f32":
        assert torch.equal(out, traced_all()[0])


# ---------------------------------------------------------------- 3. subsets
def test_subsets_of_the_steps():
    mixn, tgt = padded()
    out, _, full = traced_all()
    o2, _, sub = engine().pc_sample(mixn, MIX, **KW, lengths=LENS, seeds=SEEDS, snapshots=[0, 2])
    assert sub.steps == [0, 2] and sub.gram is None and torch.equal(o2, out)
    assert torch.equal(sub.x[0], full.x[0]) and torch.equal(sub.x[1], full.x[2])
    assert torch.equal(sub.x_mean[0], full.x_mean[0]) and torch.equal(sub.x_mean[1], full.x_mean[2])
    o3, _, nomean = engine().pc_sample(mixn, MIX, **KW, lengths=LENS, seeds=SEEDS, snapshots=[1], snapshot_means=False)
    assert nomean.x_mean is None and torch.equal(nomean.x[0], full.x[1]) and torch.equal(o3, out)
    assert nomean.intermediates()[0][1] is None
    o4, _, rows = engine().pc_sample(mixn, MIX, **KW, lengths=LENS, seeds=SEEDS, snapshots=[], target=tgt)
    assert rows.steps == [] and rows.x.shape[0] == 0 and torch.equal(rows.gram, full.gram) and torch.equal(o4, out)


# ---------------------------------------------------------------- 4. Gram rows
def test_gram_rows_are_diffsep_gram_bit_for_bit():
    mixn, tgt = padded()
    out, _, tr = traced_all()
    for i in range(3):
        assert torch.equal(tr.gram[i], ops.gram(tgt, tr.x[i].contiguous())), i
    assert torch.equal(tr.gram[3], ops.gram(tgt, out))
    got = metrics.si_bss_from_gram(tr.gram[3].cpu().numpy())
    want = metrics.si_bss_eval_sources(tgt, out)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    fixed = metrics.si_bss_from_gram(tr.gram[0].cpu().numpy(), perm=want[3])
    assert np.array_equal(fixed[3], want[3]) and np.isfinite(fixed[0]).all()


# ---------------------------------------------------------------- 5. mixed lengths
def test_every_row_of_a_mixed_length_batch_is_its_own_call():
    mixn, tgt = padded()
    _, _, tr = traced_all()
    for b, L in enumerate(LENS):
        o1, _, one = engine().pc_sample(mixn[b:b + 1, :, :L].contiguous(), MIX, **KW, seed=SEEDS[b], snapshots="all",
                                        target=tgt[b:b + 1, :, :L].contiguous())
        assert torch.equal(tr.x[:, b, :, :L], one.x[:, 0]) and torch.equal(tr.x_mean[:, b, :, :L], one.x_mean[:, 0]), b
        assert torch.equal(tr.gram[:, b], one.gram[:, 0]), b
        if L < max(LENS):
            assert float(tr.x[:, b, :, L:].abs().max()) == 0.0 and float(tr.x_mean[:, b, :, L:].abs().max()) == 0.0


# ---------------------------------------------------------------- 6. degenerate samplers
def test_degenerate_samplers():
    mixn, tgt = padded()
    eng = engine()
    kw = dict(lengths=LENS, seeds=SEEDS, snapshots="all", target=tgt)
    out, nfe, tr = eng.pc_sample(mixn, MIX, **KW, corrector="none", **kw)
    assert nfe == 3 and torch.equal(tr.x_mean, tr.x)  # the loop's "corrector" returns (x, x)
    assert torch.equal(out, eng.pc_sample(mixn, MIX, **KW, corrector="none", lengths=LENS, seeds=SEEDS)[0])
    assert not torch.equal(tr.x[1], tr.x[0])
    out, _, tr = eng.pc_sample(mixn, MIX, **{**KW, "corrector_steps": 0}, **kw)
    assert torch.equal(tr.x_mean, tr.x)
    out, nfe, tr = eng.pc_sample(mixn, MIX, **KW, predictor="none", **kw)
    assert nfe == 6 and torch.equal(out, eng.pc_sample(mixn, MIX, **KW, predictor="none", lengths=LENS, seeds=SEEDS)[0])
    assert torch.equal(tr.gram[2], ops.gram(tgt, tr.x[2].contiguous())) and not torch.equal(tr.x_mean, tr.x)
    out, nfe, tr = eng.pc_sample(mixn, MIX, **{**KW, "N": 1}, lengths=LENS, seeds=SEEDS, snapshots=[0], target=tgt)
    assert nfe == 2 and tr.x.shape[0] == 1 and tr.gram.shape[0] == 2
    assert torch.equal(out, eng.pc_sample(mixn, MIX, **{**KW, "N": 1}, lengths=LENS, seeds=SEEDS)[0])
    assert torch.equal(tr.gram[0], ops.gram(tgt, tr.x[0].contiguous())) and torch.equal(tr.gram[1], ops.gram(tgt, out))


# ---------------------------------------------------------------- 7. refusals
def raw_trace(eng, mixn, out, steps, snap_x, snap_xm, target, gram, N=3):
    """diffsep_pc_sample_trace with exactly these pointers"""
    B, _, T = mixn.shape
    sc = _lib.sde_config(MIX)
    sm = _lib.SamplerConfig(N, 1, 0.5, 0.03, 1, _lib.PRED_REVERSE_DIFFUSION, _lib.CORR_ALD2)
    arr = np.ascontiguousarray(steps, dtype=np.int32)
    _lib.call(eng._L, "diffsep_pc_sample_trace", eng._h, C.byref(sc), C.byref(sm), None, _lib._ptr(mixn), _lib._ptr(out), B, T,
              None, 5, None, None, len(steps), arr.ctypes.data_as(C.POINTER(C.c_int32)), _lib._ptr(snap_x), _lib._ptr(snap_xm),
              _lib._ptr(target), _lib._ptr(gram), _lib._stream_ptr())


def test_refusals_leave_out_untouched():
    mixn, tgt = padded()
    eng, B, T, N = engine(), 3, 7000, 3
    SENT = 7.5
    out = torch.full((B, S, T), SENT, device="cuda")
    snap = torch.full((2, B, S, T), SENT, device="cuda")
    gram = torch.full((N + 1, B, 3, S, S), SENT, dtype=torch.float64, device="cuda")
    cases = [([2, 1], snap, None, None, None), ([1, 1], snap, None, None, None), ([N], snap, None, None, None),
             ([-1], snap, None, None, None), ([0], None, None, None, None), ([], None, None, tgt, None),
             ([], None, None, None, gram)]
    for steps, sx, sxm, t, g in cases:
        with pytest.raises(_lib.DiffsepError, match="pc_sample"):
            raw_trace(eng, mixn, out, steps, sx, sxm, t, g)
        torch.cuda.synchronize()
        assert bool((out == SENT).all()) and bool((snap == SENT).all()) and bool((gram == SENT).all()), steps
    raw_trace(eng, mixn, out, [0, 2], snap, None, tgt, gram)  # (the same pointers are fine when the request is)
    assert torch.isfinite(out).all() and not bool((out == SENT).any()) and not bool((gram == SENT).any())
    m = model16()
    for bad in (dict(snapshots=[0]), dict(target=tgt)):
        with pytest.raises(ValueError, match="fused"):
            m.get_pc_sampler("reverse_diffusion", "ald2", mixn, N=3, intermediate=True, **bad)


# ---------------------------------------------------------------- 8. the reference-shaped API
def test_get_pc_sampler_with_a_trace():
    m = model16()
    mixn, tgt = padded()
    kw = dict(N=3, corrector_steps=1, snr=0.5, seeds=SEEDS, lengths=LENS)
    plain, ns0 = m.get_pc_sampler("reverse_diffusion", "ald2", mixn, **kw)()
    sampler = m.get_pc_sampler("reverse_diffusion", "ald2", mixn, **kw, snapshots=[0, 2], target=tgt)
    assert sampler.trace is None
    x, ns, im = sampler()
    assert ns == ns0 == 6 and torch.equal(x, plain)
    assert len(im) == 2 and all(xt.shape == x.shape and xm.shape == x.shape for xt, xm in im)
    tr = sampler.trace
    assert tr.steps == [0, 2] and tr.gram.shape == (4, 3, 3, S, S) and torch.equal(tr.gram[3], ops.gram(tgt, x))
    assert torch.equal(im[1][0], tr.x[1]) and torch.equal(tr.gram[2], ops.gram(tgt, im[1][0].contiguous()))
    # the scheduled sampler takes the same kwargs; minibatch= joins the minibatches' traces along the batch
    xs, _, ims = m.get_pc_sampler("reverse_diffusion", "ald2", mixn, **kw, schedule="linear", snapshots=[1])()
    assert len(ims) == 1 and torch.isfinite(xs).all()
    batched = m.get_pc_sampler("reverse_diffusion", "ald2", mixn, N=3, corrector_steps=1, snr=0.5, seed=9, minibatch=2,
                               snapshots=[0, 2], target=tgt)
    xb, nsb, imb = batched()
    assert nsb == [6, 6] and len(imb) == 2 and imb[0][0].shape == xb.shape
    assert batched.trace.gram.shape == (4, 3, 3, S, S) and torch.equal(batched.trace.gram[3], ops.gram(tgt, xb))


def test_profile_records_of_the_tap():
    mixn, tgt = padded()
    eng = engine()
    names = []
    for kw in (dict(), dict(snapshots=[1], target=tgt), dict(snapshots=[1])):
        eng.profile_begin()
        eng.pc_sample(mixn, MIX, **KW, lengths=LENS, seeds=SEEDS, **kw)
        eng.profile_end()
        names.append([(r["kernel"], r["cls"]) for r in eng.profile_records()])
    taps = [[r for r in n if r[0].startswith("trace_tap")] for n in names]
    assert [len(t) for t in taps] == [0, 3, 1] and all(cls == -1 for t in taps for _, cls in t)
    rest = [[r for r in n if not r[0].startswith("trace_tap")] for n in names]
    assert rest[0] == rest[1] == rest[2] and len(rest[0]) > 0


# ---------------------------------------------------------------- 9. evaluate --trajectory / --fig
def test_evaluate_cli_trajectory_and_fig(tmp_path):
    common = ["--synthetic", "3", "--samples", "4000", "--synthetic-weights", "16", "-N", "2", "--dtype", "f32", "--flat-output",
              "--no-stoi"]
    recs = {}
    for name, extra in (("plain", ["--save-n", "0", "--streams", "1"]), ("s1", ["--save-n", "0", "--streams", "1", "--trajectory"]),
                        ("s2", ["--save-n", "0", "--streams", "2", "--trajectory"])):
        eval_cli.main(common + extra + ["-o", str(tmp_path / name)])
        recs[name] = json.load(open(tmp_path / name / "test.json"))

    def strip(rec, *keys):
        return [{k: v for k, v in r.items() if k not in ("runtime",) + keys} for r in rec]
    assert strip(recs["s1"]) == strip(recs["s2"])
    assert strip(recs["s1"], "si_sdr_steps") == strip(recs["plain"])
    for r in recs["s1"]:
        steps = r["si_sdr_steps"]
        assert len(steps) == 3 and all(len(row) == S for row in steps) and np.isfinite(steps).all()
        assert steps[-1] == r["si_sdr"][0]
    summ = json.load(open(tmp_path / "s1" / "test_summary.json"))
    assert np.allclose(summ["si_sdr_steps"], np.mean([r["si_sdr_steps"] for r in recs["s1"]], axis=0), rtol=0, atol=1e-12)
    assert "si_sdr_steps" not in json.load(open(tmp_path / "plain" / "test_summary.json"))
    try:
        import matplotlib  # noqa: F401
    except ImportError:
        return  # (the figure needs matplotlib; everything on the device was checked above)
    eval_cli.main(common + ["--streams", "2", "--fig", "--trajectory", "--save-n", "2", "-o", str(tmp_path / "fig")])
    figs = sorted(p.name for p in (tmp_path / "fig" / "fig" / "test").iterdir())
    assert figs == ["evo_000.pdf", "evo_001.pdf"]
    assert all((tmp_path / "fig" / "fig" / "test" / f).read_bytes().startswith(b"%PDF") for f in figs)
    assert strip(json.load(open(tmp_path / "fig" / "test.json"))) == strip(recs["s1"])
