"""Device STOI / ESTOI (csrc/stoi.hip: ops.stoi, metrics.stoi_batch, evaluate --stoi-on device) against the two float64 host
forms (diffsep_amd.metrics.stoi and the loop-form oracle/stoi_oracle.py) at the bound those two are held to against each
other (1e-9, tests/test_metrics_cpu.py), plus the batch / permutation / determinism properties of the C-ABI entry."""
import ctypes as C
import itertools
import json

import numpy as np
import pytest
import torch

import stoi_cases as SC
import stoi_oracle as SO
from diffsep_amd import _lib, metrics, ops, synth

pytestmark = pytest.mark.gpu
TOL = 1e-9


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _speechlike(i, T, fs=8000):
    return synth.synth_mixture(i, T=T, fs=fs)[1][0].astype(np.float32)


@pytest.mark.parametrize("fs,T", SC.CONFIGS)
def test_device_matches_both_host_forms(fs, T):
    pairs = [SC.pair(i, T, fs) for i in range(SC.N_UTT)]
    ref = np.stack([p[0] for p in pairs])  # [8, 2, T]
    est = np.stack([p[1] for p in pairs])
    for r in ref.reshape(-1, T):               # the precondition: no keep decision within 0.1 dB of the threshold
        assert SC.threshold_margin(r, fs)[0] >= 0.1
    worst = 0.0
    for extended in (True, False):
        got = ops.stoi(_dev(ref), _dev(est), fs, extended=extended).cpu().numpy()
        assert got.shape == (SC.N_UTT, 2) and got.dtype == np.float64
        for b in range(SC.N_UTT):
            for i in range(2):
                a = metrics.stoi(ref[b, i], est[b, i], fs, extended)
                o = SO.stoi(ref[b, i], est[b, i], fs, extended)
                d = max(abs(got[b, i] - a), abs(got[b, i] - o))
                worst = max(worst, d)
                print(f"fs={fs} T={T} ext={extended} b={b} i={i} device={got[b, i]:.15f} metrics={a:.15f} oracle={o:.15f} diff={d:.2e}")
                assert abs(got[b, i] - a) < TOL and abs(got[b, i] - o) < TOL, (fs, T, extended, b, i, got[b, i], a, o)
    print(f"fs={fs} T={T}: worst |device - host| = {worst:.3e}")


def test_mixed_batch_equals_single_rows_bit_for_bit():
    fs, T, lens = 8000, 32000, [32000, 31999, 12345, 3400]
    ref, est = np.zeros((4, 2, T), np.float32), np.zeros((4, 2, T), np.float32)
    for b, n in enumerate(lens):
        r, e = SC.pair(b, n, fs)
        ref[b, :, :n], est[b, :, :n] = r, e
    junk_r, junk_e = ref.copy(), est.copy()
    rng = np.random.default_rng(5)
    for b, n in enumerate(lens):  # garbage, not zeros, beyond each row's length
        junk_r[b, :, n:] = 50.0 * rng.standard_normal((2, T - n))
        junk_e[b, :, n:] = 50.0 * rng.standard_normal((2, T - n))
    for extended in (True, False):
        batch = ops.stoi(_dev(ref), _dev(est), fs, extended=extended, lengths=lens).cpu().numpy()
        junk = ops.stoi(_dev(junk_r), _dev(junk_e), fs, extended=extended, lengths=lens).cpu().numpy()
        assert np.array_equal(batch, junk), (batch, junk)
        assert np.all(np.isfinite(batch))
        for b, n in enumerate(lens):
            padded = ops.stoi(_dev(junk_r[b:b + 1]), _dev(junk_e[b:b + 1]), fs, extended=extended, lengths=[n]).cpu().numpy()
            alone = ops.stoi(_dev(ref[b:b + 1, :, :n]), _dev(est[b:b + 1, :, :n]), fs, extended=extended).cpu().numpy()
            assert np.array_equal(batch[b:b + 1], padded) and np.array_equal(batch[b:b + 1], alone), (b, batch[b], padded, alone)
        for i in range(2):  # the full-length row against the host, and the short row's sentinel or value
            assert SC.threshold_margin(ref[0, i], fs)[0] >= 0.1 and SC.threshold_margin(ref[3, i, :3400], fs)[0] >= 0.1
            assert abs(batch[0, i] - metrics.stoi(ref[0, i], est[0, i], fs, extended)) < TOL
            assert abs(batch[3, i] - metrics.stoi(ref[3, i, :3400], est[3, i, :3400], fs, extended)) < TOL


def test_permutations():
    fs, T, S = 8000, 32000, 3
    ref = np.stack([SC.pair(i, T, fs)[0][0] for i in range(S)])[None]  # [1, 3, T]
    est = np.stack([SC.pair(i, T, fs)[1][0] for i in range(S)])[None]
    for extended in (True, False):
        ident = ops.stoi(_dev(ref), _dev(est), fs, extended=extended).cpu().numpy()
        for p in itertools.permutations(range(S)):
            got = ops.stoi(_dev(ref), _dev(est), fs, extended=extended, perm=[list(p)]).cpu().numpy()
            for i in range(S):
                want = metrics.stoi(ref[0, i], est[0, p[i]], fs, extended)
                assert abs(got[0, i] - want) < TOL, (p, i, got[0, i], want)
            if p == tuple(range(S)):
                assert np.array_equal(got, ident)                                # NULL = identity
        via_metrics = metrics.stoi_batch(_dev(ref), _dev(est), fs, extended=extended, perm=np.array([[2, 0, 1]]))
        assert isinstance(via_metrics, np.ndarray) and via_metrics.shape == (1, S)
        assert abs(via_metrics[0, 0] - metrics.stoi(ref[0, 0], est[0, 2], fs, extended)) < TOL


def test_edge_rows():
    fs, T = 8000, 32000
    x = _speechlike(0, T)
    n = (0.3 * np.std(x) * synth.normal("edge", T, 0)).astype(np.float32)
    zero = np.zeros(T, np.float32)
    for extended in (True, False):
        one = lambda r, e, **kw: float(ops.stoi(_dev(r)[None, None], _dev(e)[None, None], fs, extended=extended, **kw).cpu()[0, 0])
        for r, e, want in ((zero, x + n, 0.0), (x, zero, 0.0)):
            got = one(r, e)
            assert np.isfinite(got) and got == want and abs(metrics.stoi(r, e, fs, extended) - want) < TOL, (got, want)
        assert one(x[:200], x[:200]) == 1e-5 == metrics.stoi(x[:200], x[:200], fs, extended)     # no frame at all
        assert one(x[:3000], x[:3000]) == 1e-5 == metrics.stoi(x[:3000], x[:3000], fs, extended)  # fewer than 30 frames
        assert one(x, x, lengths=[200]) == 1e-5 and one(x, x, lengths=[3000]) == 1e-5
        assert abs(one(x[:3400], x[:3400]) - 1.0) < TOL and abs(metrics.stoi(x[:3400], x[:3400], fs, extended) - 1.0) < TOL
        assert abs(one(x, x) - 1.0) < TOL
        # (y on a 2^-14 grid: 7.5 y is then exact in float32, so the scaled estimate is the same signal, not a re-rounded one)
        y = (np.round((x + n).astype(np.float64) * 16384.0) / 16384.0).astype(np.float32)
        assert np.array_equal((7.5 * y).astype(np.float64), 7.5 * y.astype(np.float64))
        a, b = one(x, y), one(x, 7.5 * y)
        assert abs(a - b) < TOL and abs(a - metrics.stoi(x, y, fs, extended)) < TOL


def test_resampler_through_tones():
    for fs in (8000, 16000):
        T = fs
        t = np.arange(T) / fs
        tone = np.sin(2 * np.pi * 1000 * t).astype(np.float32)
        noisy = (tone + 0.3 * synth.normal("tone", T, fs)).astype(np.float32)
        assert SC.threshold_margin(tone, fs)[0] >= 0.1
        for extended in (True, False):
            got = float(ops.stoi(_dev(tone)[None, None], _dev(noisy)[None, None], fs, extended=extended).cpu()[0, 0])
            assert abs(got - metrics.stoi(tone, noisy, fs, extended)) < TOL
            assert abs(got - SO.stoi(tone, noisy, fs, extended)) < TOL
    # 16 kHz -> 10 kHz: a 6.5 kHz tone must be rejected, not aliased to 3.5 kHz (host: 1 - 4e-9 against 0.90 / 0.99 aliased)
    fs, T = 16000, 32000
    x = _speechlike(0, T, fs)
    t = np.arange(T) / fs
    for extended in (True, False):
        got = {}
        for f in (6500, 3500):
            y = (x + 0.5 * np.std(x) * np.sin(2 * np.pi * f * t)).astype(np.float32)
            got[f] = float(ops.stoi(_dev(x)[None, None], _dev(y)[None, None], fs, extended=extended).cpu()[0, 0])
            assert abs(got[f] - metrics.stoi(x, y, fs, extended)) < TOL
        assert got[6500] > 0.9999 and got[3500] < 0.99


def test_determinism_also_beside_a_running_sampler():
    from diffsep_amd.pl_model import DiffSepModel, default_config
    fs, T, B = 8000, 32000, 4
    pairs = [SC.pair(i, T, fs) for i in range(B)]
    ref, est = _dev(np.stack([p[0] for p in pairs])), _dev(np.stack([p[1] for p in pairs]))
    first = ops.stoi(ref, est, fs)
    second = ops.stoi(ref, est, fs)
    torch.cuda.synchronize()
    assert torch.equal(first, second)
    model = DiffSepModel(default_config(nf=16), dtype="f32")
    mix = torch.from_numpy(synth.synth_batch(2, T=8000)[0]).cuda()
    (mix_n, _), *_ = model.normalize_batch((mix, None))
    s_model, s_side = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s_model):
        sampler = model.get_pc_sampler("reverse_diffusion", "ald2", mix_n, N=10, corrector_steps=1, snr=0.5, denoise=True,
                                       intermediate=False, lengths=[8000, 8000], seeds=[1, 2], check_finite=False)
        sep, nfe, *_ = sampler()   # enqueued; still running while the side stream scores
    with torch.cuda.stream(s_side):
        side = [ops.stoi(ref, est, fs) for _ in range(3)]
    torch.cuda.synchronize()
    assert torch.isfinite(sep).all()
    for s in side:
        assert torch.equal(first, s)


def test_unsupported_input_is_an_error_and_writes_nothing():
    fs, T = 8000, 4000
    x = _dev(_speechlike(0, T))[None, None]
    with pytest.raises(_lib.DiffsepError, match="sample rate"):
        ops.stoi(x, x, 0)
    with pytest.raises(_lib.DiffsepError, match="sample rate"):
        ops.stoi(x, x, 9999)
    l = _lib.lib()
    out = torch.full((1, 1), -7.0, dtype=torch.float64, device="cuda")
    need = ops.stoi_workspace_bytes(1, 1, T, fs)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    P = lambda t: C.c_void_p(t.data_ptr())
    assert l.diffsep_stoi(P(x), P(x), P(out), 0, 1, T, None, None, fs, 1, P(ws), need, None) != 0
    assert b"bad shape" in l.diffsep_last_error()
    assert l.diffsep_stoi(P(x), P(x), P(out), 1, 1, T, None, None, fs, 1, P(ws), need - 1, None) != 0
    assert b"workspace too small" in l.diffsep_last_error()
    torch.cuda.synchronize()
    assert float(out.cpu()[0, 0]) == -7.0
    assert l.diffsep_stoi(P(x), P(x), P(out), 1, 1, T, None, None, fs, 1, P(ws), need, None) == 0
    torch.cuda.synchronize()
    assert abs(float(out.cpu()[0, 0]) - 1.0) < TOL


def _run_evaluate(tmp_path, name, extra):
    from diffsep_amd import evaluate as ev
    out = tmp_path / name
    ev.main(["--synthetic", "16", "--synthetic-weights", "16", "--flat-output", "-o", str(out)] + extra)
    return json.load(open(out / "test.json")), json.load(open(out / "test_summary.json"))


@pytest.mark.parametrize("K", [1, 2])
def test_evaluate_stoi_on_device_matches_host(tmp_path, K):
    common = ["--streams", str(K), "--save-n", "1"]
    host, hs = _run_evaluate(tmp_path, "host", common + ["--stoi-on", "host"])
    dev, ds = _run_evaluate(tmp_path, "dev", common + ["--stoi-on", "device"])
    assert hs["stoi_on"] == "host" and ds["stoi_on"] == "device" and hs["number"] == ds["number"] == 16
    assert [r["si_sdr"] for r in host] == [r["si_sdr"] for r in dev]
    assert [r["perm"] for r in host] == [r["perm"] for r in dev]
    worst = 0.0
    for h, d in zip(host, dev):
        assert len(h["stoi"]) == len(d["stoi"]) == 2
        worst = max(worst, max(abs(a - b) for a, b in zip(h["stoi"], d["stoi"])))
    print(f"K={K}: worst |stoi host - device| over 16 utterances = {worst:.3e}")
    assert worst < TOL
    assert abs(hs["stoi"] - ds["stoi"]) < TOL


def test_evaluate_enhance_scores_the_first_source_only(tmp_path):
    from diffsep_amd import evaluate as ev
    recs = {}
    for on in ("host", "device"):
        out = tmp_path / on
        ev.main(["--synthetic", "3", "--samples", "8000", "--synthetic-weights", "16", "-N", "2", "--dtype", "f32", "--enhance",
                 "--save-n", "0", "--flat-output", "-o", str(out), "--stoi-on", on])
        recs[on] = json.load(open(out / "test.json"))
    for h, d in zip(recs["host"], recs["device"]):
        assert len(h["stoi"]) == len(d["stoi"]) == 1 and h["perm"] == d["perm"]
        assert abs(h["stoi"][0] - d["stoi"][0]) < TOL


def test_evaluate_on_device_copies_no_waveform_to_the_host(tmp_path, monkeypatch):
    calls = []
    real_cpu = torch.Tensor.cpu

    def counting_cpu(self, *a, **kw):
        if self.is_cuda and self.numel() >= 32000:
            calls.append(tuple(self.shape))
        return real_cpu(self, *a, **kw)
    monkeypatch.setattr(torch.Tensor, "cpu", counting_cpu)
    rec, summ = _run_evaluate(tmp_path, "nocopy", ["--save-n", "0", "--stoi-on", "device"])
    assert summ["stoi_on"] == "device" and "stoi" not in summ["not_computed"]
    assert all(len(r["stoi"]) == 2 and all(np.isfinite(v) for v in r["stoi"]) for r in rec)
    assert calls == [], calls
    _run_evaluate(tmp_path, "copy", ["--save-n", "0", "--stoi-on", "host"])
    assert calls  # the host path is what needs them
