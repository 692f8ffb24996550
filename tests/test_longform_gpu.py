"""Long recordings on the GPU: the stitch kernels (csrc/longform.hip) against the numpy restatement (tests/longform_ref.py),
DiffSepModel.separate_long on the engine, and separate --chunk."""
import ctypes as C

import numpy as np
import pytest
import torch

import longform_ref as R
from diffsep_amd import _lib, inflight, ops, synth, wavio
from diffsep_amd import separate as sep_cli
from diffsep_amd.engine import param_table
from diffsep_amd.pl_model import DiffSepModel, default_config

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def run_stitch(win, T, Tv, want_gram=False):
    wd = torch.from_numpy(win).cuda()
    out = torch.full((win.shape[1], T), float("nan"), dtype=torch.float32, device="cuda")
    return ops.longform_stitch(wd, T, Tv, want_gram=want_gram, out=out)


# ------------------------------------------------------------------------------------------------ 1. exact reassembly
@pytest.mark.parametrize("S,Tw,Tv,T", [(1, 1024, 256, 5000), (2, 1024, 256, 5000), (3, 1024, 256, 5000), (3, 1024, 341, 1025),
                                       (2, 32000, 4000, 100001)])
def test_exact_reassembly(S, Tw, Tv, T):
    x, win, q = R.reassembly_case(S, T, Tw, Tv)
    ref_out, ref_perm, _ = R.stitch(win, T, Tv)
    assert np.array_equal(bits(ref_out), bits(x[list(q[0])]))  # (the restatement's own precondition, tests/test_longform_cpu.py)
    out, perm = run_stitch(win, T, Tv)
    assert np.array_equal(perm.cpu().numpy(), ref_perm)
    assert np.array_equal(bits(out), bits(x[list(q[0])]))


def test_one_window_is_the_file():
    x = np.random.default_rng(5).standard_normal((1, 2, 1024)).astype(np.float32)
    out, perm = run_stitch(x, 700, 256)  # K = 1: T = 700 < Tw
    assert np.array_equal(bits(out), bits(x[0][:, :700])) and perm.cpu().tolist() == [[0, 1]]


# ------------------------------------------------------------------------------------------------ 2. cross-Gram
@pytest.mark.parametrize("S,Tw,Tv,T", [(3, 1024, 256, 5000), (2, 1024, 341, 1025)])
def test_cross_gram_bound_and_reproducibility(S, Tw, Tv, T):
    _, win, _ = R.reassembly_case(S, T, Tw, Tv, seed=1)
    out, perm, gram = run_stitch(win, T, Tv, want_gram=True)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        out2, perm2, gram2 = run_stitch(win, T, Tv, want_gram=True)
    side.synchronize()
    assert torch.equal(gram, gram2) and torch.equal(perm, perm2) and np.array_equal(bits(out), bits(out2))
    starts = R.plan(T, Tw, Tv)
    g = gram.cpu().numpy()
    assert g.shape == (len(starts) - 1, S, S)
    worst = 0.0
    for k, (b, ov) in enumerate(R.overlaps(starts, Tw)):
        c, m = R.cross_gram_exact(win[k][:, b - starts[k]:b - starts[k] + ov], win[k + 1][:, :ov])
        bound = ov * 2.0 ** -52 * m  # products of two float32 are exact in float64: only the additions round
        worst = max(worst, float(np.max(np.abs(g[k] - c) / bound)))
        assert np.all(np.abs(g[k] - c) <= bound), (k, np.abs(g[k] - c) / bound)
    print(f"S={S} Tw={Tw} Tv={Tv} T={T}: worst |gram - exact| / bound = {worst:.3e}")


# ------------------------------------------------------------------------------------------------ 3. blend
def test_blend_of_windows_that_disagree():
    Tw, Tv, K = 1024, 256, 3
    T = Tw + (K - 1) * (Tw - Tv)
    assert len(R.plan(T, Tw, Tv)) == K
    win = np.random.default_rng(9).standard_normal((K, 1, Tw)).astype(np.float32)
    out, perm = run_stitch(win, T, Tv)
    out = out.cpu().numpy()[0]
    assert perm.cpu().tolist() == [[0]] * K
    ref, mag, seam = R.blend_f64(win, T, Tv)
    assert int(seam.sum()) == (K - 1) * Tv
    err = np.abs(out.astype(np.float64) - ref)
    # one rounding each in the subtraction, the ratio, the product and the sum, each bounded by the operands
    bound = 6 * 2.0 ** -24 * mag
    print(f"blend: worst |out - ref| / bound inside seams = {float(np.max(err[seam] / bound[seam])):.3f}")
    assert np.all(err[seam] <= bound[seam])
    assert np.array_equal(bits(out[~seam]), bits(ref[~seam].astype(np.float32)))  # outside seams: the owning window, bit for bit
    assert np.array_equal(bits(out), bits(R.blend(win, T, Tv, np.zeros((K, 1), np.int32))[0]))


# ------------------------------------------------------------------------------------------------ 4. tie rule
def test_silent_overlap_keeps_the_identity():
    Tw, Tv, T = 1024, 256, 1792  # K = 2, overlap exactly Tv
    rng = np.random.default_rng(3)
    win = rng.standard_normal((2, 3, Tw)).astype(np.float32)
    win[0][:, Tw - Tv:] = 0.0
    win[1][:, :Tv] = 0.0
    out, perm, gram = run_stitch(win, T, Tv, want_gram=True)
    assert perm.cpu().tolist() == [[0, 1, 2], [0, 1, 2]] and float(gram.abs().max()) == 0.0
    assert np.array_equal(bits(out), bits(R.stitch(win, T, Tv)[0]))


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals_write_nothing():
    l = _lib.lib()
    K, S, Tw, Tv, T = 7, 2, 1024, 256, 5000
    win = torch.randn(K, 4, Tw, device="cuda")
    out = torch.full((4, T), -7.0, device="cuda")
    perm = torch.full((K + 1, 4), -7, dtype=torch.int32, device="cuda")
    need = l.diffsep_longform_workspace_bytes(K, S)
    ws = torch.empty(need + 4096, dtype=torch.uint8, device="cuda")
    P = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(K_=K, S_=S, Tv_=Tv, nbytes=need, win_=win):
        return l.diffsep_longform_stitch(P(win_) if win_ is not None else None, K_, S_, Tw, T, Tv_, P(out), P(perm), None, P(ws),
                                         nbytes, st)

    for kw, word in ((dict(S_=4), b"sources"), (dict(K_=6), b"windows"), (dict(K_=8), b"windows"), (dict(Tv_=342), b"3 Tv > Tw"),
                     (dict(nbytes=need - 1), b"workspace too small"), (dict(win_=None), b"null")):
        assert call(**kw) != 0
        assert word in l.diffsep_last_error(), (kw, l.diffsep_last_error())
        torch.cuda.synchronize()
        assert bool((out == -7.0).all()) and bool((perm == -7).all()), kw
    assert call() == 0  # the same buffers, nothing refused: everything of [S, T] and [K, S] is written
    torch.cuda.synchronize()
    assert bool((out.view(-1)[:S * T] != -7.0).all()) and bool((perm.view(-1)[:K * S] >= 0).all())
    assert bool((out.view(-1)[S * T:] == -7.0).all()) and bool((perm.view(-1)[K * S:] == -7).all())


# ------------------------------------------------------------------------------------------------ 6. end to end on the engine
def model16(dtype="f32"):
    m = DiffSepModel(default_config(nf=16), dtype=dtype)
    table = [(n, s) for n, s, _ in param_table(m.score_model.cfg)]
    sd = synth.synth_state_dict(table, 7)
    m.score_model.load_state_dict({"backbone." + k: torch.from_numpy(v) for k, v in sd.items()})
    return m.to("cuda:0")


def test_separate_long_on_the_engine():
    m = model16()
    kw = dict(N=2, corrector_steps=1, snr=0.5)
    T, window, overlap, seed = 10000, 4000, 1000, 11
    mix = torch.from_numpy(synth.synth_mixture(0, T=T)[0]).cuda()  # [1, T]
    out = m.separate_long(mix, window, overlap, batch=1, seed=seed, **kw)
    info = m.longform_info
    assert out.shape == (1, 2, T) and bool(torch.isfinite(out).all())
    assert info["K"] == 3 and info["starts"] == R.plan(T, window, overlap) == [0, 3000, 6000]
    assert info["seeds"] == [(seed + 0x9E3779B97F4A7C15 * k) % (1 << 64) for k in range(3)]
    assert m.engine().padded_frames(window) == 64
    wins = [sep_cli.separate_on_device(mix[None, :, s:s + window], m, kw, "cuda:0", lengths=[window], seeds=[sd])
            for s, sd in zip(info["starts"], info["seeds"])]
    ref, perm = ops.longform_stitch(torch.cat(wins), T, overlap)
    assert torch.equal(perm, info["perm"]) and np.array_equal(bits(out[0]), bits(ref))
    # the fp32 engine is batch-independent bit for bit (tests/test_round5_gpu.py, tests/test_round2_gpu.py)
    out3 = m.separate_long(mix, window, overlap, batch=3, seed=seed, **kw)
    assert np.array_equal(bits(out3), bits(out))
    # a file no longer than the window: what separate_on_device returns for it
    short = mix[:, :3000].contiguous()
    one = m.separate_long(short, window, overlap, seed=seed, **kw)
    same = sep_cli.separate_on_device(short[None], m, kw, "cuda:0", lengths=[3000], seeds=[seed])
    assert m.longform_info["K"] == 1 and m.longform_info["perm"].cpu().tolist() == [[0, 1]]
    assert one.shape == (1, 2, 3000) and np.array_equal(bits(one), bits(same))


# ------------------------------------------------------------------------------------------------ 7. CLI
def test_separate_cli_chunked(tmp_path):
    ind, short = tmp_path / "in", tmp_path / "short"
    ind.mkdir()
    short.mkdir()
    lens = {"a_long": 10000, "b_short": 3000, "c_short": 3000}
    for i, (name, T) in enumerate(lens.items()):
        wav = torch.from_numpy(synth.synth_mixture(i, T=T)[0])
        wavio.save(ind / f"{name}.wav", wav, 8000)
        if T == 3000:
            wavio.save(short / f"{name}.wav", wav, 8000)
    common = ["--synthetic-weights", "16", "-N", "2", "--dtype", "f32", "--batch", "4", "--seed", "5"]
    chunk = ["--chunk", "0.5", "--overlap", "0.125"]
    outs = []
    for k in (1, 2):
        outd = tmp_path / f"out{k}"
        sep_cli.main([str(ind), str(outd)] + chunk + common + ["--streams", str(k)])
        got = {}
        for name, T in lens.items():
            for s in ("s0", "s1"):
                y, sr = wavio.load(outd / s / f"{name}.wav")
                assert sr == 8000 and y.shape == (1, T) and bool(torch.isfinite(y).all())
                got[name, s] = (outd / s / f"{name}.wav").read_bytes()
        outs.append(got)
    assert outs[0] == outs[1]
    # short files only: --chunk changes nothing
    sep_cli.main([str(short), str(tmp_path / "s_chunk"), "--chunk", "0.5"] + common)
    sep_cli.main([str(short), str(tmp_path / "s_plain")] + common)
    for name in ("b_short", "c_short"):
        for s in ("s0", "s1"):
            assert (tmp_path / "s_chunk" / s / f"{name}.wav").read_bytes() == (tmp_path / "s_plain" / s / f"{name}.wav").read_bytes()
    with pytest.raises(SystemExit) as e:
        sep_cli.main([str(short), str(tmp_path / "nope"), "--sampler", "ode", "--chunk", "0.5"] + common)
    assert "--sampler ode --chunk is not supported" in str(e.value)
    assert inflight.window_seeds(5, 2) == [5, 5 + 0x9E3779B97F4A7C15]
