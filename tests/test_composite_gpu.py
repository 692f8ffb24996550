"""Device LLR / WSS / segmental SNR (csrc/composite.hip: ops.composite, metrics.composite_batch, evaluate_covl --on device,
evaluate --composite) against the float64 host form diffsep_amd.metrics.composite at the bound the project holds between its host
and device STOI (1e-9 max(1, |v|): both sides are float64, and the inputs' slopes stay at least 1e-6 dB away from the sign tests of
the peak search, tests/test_composite_cpu.py), against the reference's own values (tests/golden/golden_composite.npz, within the
deviations recorded there), plus the batch / permutation / determinism / refusal properties of the C-ABI entry."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import composite_cases as CC
from conftest import GOLDEN_DIR
from diffsep_amd import _lib, evaluate_covl, metrics, ops, wavio

pytestmark = pytest.mark.gpu
TOL = 1e-9


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLDEN_DIR, "golden_composite.npz")))


@pytest.fixture(scope="module")
def host():
    """metrics.composite of every input, once"""
    return {(fs, T, i): metrics.composite(*CC.pair(i, T, fs), fs) for fs, T in CC.SHAPES for i in range(CC.N_UTT)}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _close(a, b, tol):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(np.all((np.abs(a - b) <= tol) | (np.isnan(a) & np.isnan(b))))


def _rel(v):
    return TOL * np.maximum(1.0, np.abs(np.nan_to_num(np.asarray(v, np.float64))))


def _batch(fs, T):
    """the shape's inputs as one [N_UTT, 2, T] batch: source 0 = utterance i's pair, source 1 = utterance (i + 1)'s"""
    pairs = [CC.pair(i, T, fs) for i in range(CC.N_UTT)]
    src = lambda i: [i, (i + 1) % CC.N_UTT]
    ref = np.stack([np.stack([pairs[j][0] for j in src(i)]) for i in range(CC.N_UTT)])
    est = np.stack([np.stack([pairs[j][1] for j in src(i)]) for i in range(CC.N_UTT)])
    return ref, est, src


@pytest.mark.parametrize("fs,T", CC.SHAPES)
def test_device_matches_host_form_and_reference(gold, host, fs, T):
    ref, est, src = _batch(fs, T)
    n = CC.FRAMES[(fs, T)]
    out, frames = ops.composite(_dev(ref), _dev(est), fs, frames=True)
    out_only = ops.composite(_dev(ref), _dev(est), fs)  # frames_out = NULL: the same aggregates
    out, frames, out_only = out.cpu().numpy(), frames.cpu().numpy(), out_only.cpu().numpy()
    assert out.shape == (CC.N_UTT, 2, 4) and out.dtype == np.float64 and frames.shape == (CC.N_UTT, 2, 3, max(1, n))
    assert np.array_equal(out, out_only, equal_nan=True)
    dev_llr_frame, dev_llr_mean, _, dev_seg_frame = gold[f"dev_fs{fs}_T{T}"]
    for b in range(CC.N_UTT):
        for s, i in enumerate(src(b)):
            h, k = host[(fs, T, i)], CC.key(fs, T, i)
            assert out[b, s, 3] == n == h["n_frames"]
            if n == 0:
                assert np.all(np.isnan(out[b, s, :3])) and np.all(np.isnan(frames[b, s]))  # NaN, and no frame written
                continue
            d = [np.max(np.abs(frames[b, s, q] - h[name])) for q, name in enumerate(("llr_frames", "wss_frames", "segsnr_frames"))]
            a = [abs(out[b, s, q] - h[name]) for q, name in enumerate(("llr", "wss", "segsnr"))]
            print(f"{k}: |device - host| frames llr {d[0]:.2e} wss {d[1]:.2e} segsnr {d[2]:.2e}; aggregates {a[0]:.2e} {a[1]:.2e} {a[2]:.2e}")
            for q, name in enumerate(("llr", "wss", "segsnr")):
                assert _close(frames[b, s, q], h[name + "_frames"], _rel(h[name + "_frames"])), (k, name)
                assert _close(out[b, s, q], h[name], _rel(h[name])), (k, name, out[b, s, q], h[name])
            # ... and the reference's values directly, within what the generator recorded for the host form (+ the bound above)
            agg = gold[k + "_agg"]
            assert _close(frames[b, s, 0], gold[k + "_llr_frames"], 4 * dev_llr_frame + TOL)
            assert _close(frames[b, s, 1], gold[k + "_wss_frames"], _rel(gold[k + "_wss_frames"]))
            assert _close(frames[b, s, 2], gold[k + "_segsnr_frames"], 4 * dev_seg_frame + TOL)
            assert abs(out[b, s, 0] - agg[0]) <= 4 * dev_llr_mean + TOL
            assert abs(out[b, s, 1] - agg[1]) <= TOL * max(1, abs(agg[1]))
            assert abs(out[b, s, 2] - agg[2]) <= 4 * dev_seg_frame + TOL


def test_mixed_batch_equals_single_rows_bit_for_bit(host):
    fs, T, lens = 16000, 16100, [16100, 4080, 600]
    perm = [[1, 0], [0, 1], [1, 0]]
    ref, est = np.zeros((3, 2, T), np.float32), np.zeros((3, 2, T), np.float32)
    for b, n in enumerate(lens):
        for s in range(2):
            r, e = CC.pair(s, n, fs)
            ref[b, s, :n], est[b, perm[b][s], :n] = r, e  # estimate row perm[b][s] belongs to reference row s
    rng = np.random.default_rng(5)
    for b, n in enumerate(lens):  # garbage, not zeros, beyond each row's length: never read
        ref[b, :, n:] = 50.0 * rng.standard_normal((2, T - n))
        est[b, :, n:] = 50.0 * rng.standard_normal((2, T - n))
    dref, dest = _dev(ref), _dev(est)
    out, frames = ops.composite(dref, dest, fs, lengths=lens, perm=perm, frames=True)
    out2, frames2 = ops.composite(dref, dest, fs, lengths=lens, perm=perm, frames=True)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        out3, frames3 = ops.composite(dref, dest, fs, lengths=lens, perm=perm, frames=True)
    torch.cuda.synchronize()
    for o, f in ((out2, frames2), (out3, frames3)):
        assert torch.equal(out.view(torch.int64), o.view(torch.int64)) and torch.equal(frames.view(torch.int64), f.view(torch.int64))
    out, frames = out.cpu().numpy(), frames.cpu().numpy()
    for b, n in enumerate(lens):
        nfr = CC.FRAMES[(fs, n)]
        # alone: the row cut to its own length, estimates put into the references' order on the host
        r1, e1 = ref[b:b + 1, :, :n], est[b:b + 1, perm[b], :n]
        o1, f1 = ops.composite(_dev(r1), _dev(e1), fs, frames=True)
        o1, f1 = o1.cpu().numpy(), f1.cpu().numpy()
        assert np.array_equal(out[b:b + 1], o1), (b, out[b], o1)
        assert np.array_equal(frames[b:b + 1, :, :, :nfr], f1[..., :nfr]) and np.all(np.isnan(frames[b, :, :, nfr:]))
        for s in range(2):
            h = host[(fs, n, s)]
            assert out[b, s, 3] == nfr
            for q, name in enumerate(("llr", "wss", "segsnr")):
                assert _close(out[b, s, q], h[name], _rel(h[name])), (b, s, name)
    via = metrics.composite_batch(dref, dest, fs, lengths=lens, perm=np.array(perm))
    assert isinstance(via, np.ndarray) and np.array_equal(via, out)


def test_refusals_write_nothing_and_leave_the_stream_usable(host):
    fs, T = 16000, 1680
    r, e = CC.pair(0, T, fs)
    x, y = _dev(r)[None, None], _dev(e)[None, None]
    with pytest.raises(_lib.DiffsepError, match="sample rate"):
        ops.composite(x, y, 44100)
    with pytest.raises(_lib.DiffsepError, match="bad shape"):
        ops.composite(x.expand(1, 4, T), y.expand(1, 4, T), fs)
    l = _lib.lib()
    out = torch.full((1, 1, 4), -7.0, dtype=torch.float64, device="cuda")
    fr = torch.full((1, 1, 3, 10), -7.0, dtype=torch.float64, device="cuda")
    need = ops.composite_workspace_bytes(1, 1, T, fs)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    P = lambda t: C.c_void_p(t.data_ptr())
    call = lambda out_p, fs_, wsb, cap=10: l.diffsep_composite(P(x), P(y), out_p, P(fr), cap, 1, 1, T, None, None, fs_, P(ws), wsb, None)
    assert call(P(out), 44100, need) != 0 and b"sample rate" in l.diffsep_last_error()
    assert call(P(out), fs, need - 1) != 0 and b"workspace too small" in l.diffsep_last_error()
    assert call(None, fs, need) != 0 and b"null pointer" in l.diffsep_last_error()
    assert call(P(out), fs, need, cap=9) != 0 and b"frames_cap" in l.diffsep_last_error()
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((fr == -7.0).all())
    assert call(P(out), fs, need) == 0
    torch.cuda.synchronize()
    h = host[(fs, T, 0)]
    got = out.cpu().numpy()[0, 0]
    assert got[3] == 10 and all(abs(got[q] - h[name]) <= TOL * max(1, abs(h[name])) for q, name in enumerate(("llr", "wss", "segsnr")))
    assert _close(fr.cpu().numpy()[0, 0, 1], h["wss_frames"], _rel(h["wss_frames"]))


def test_evaluate_covl_on_device_matches_host(tmp_path):
    wav = tmp_path / "exp" / "wav" / "test"
    wav.mkdir(parents=True)
    for i, T in enumerate((4080, 16100, 1680)):
        ref, est = CC.pair(i % CC.N_UTT, T, 16000)
        s = 0.5 / np.abs(est).max()
        wavio.save(wav / f"{i:04d}.tgt0.wav", torch.from_numpy(ref * s)[None], 16000, bits=16)
        wavio.save(wav / f"{i:04d}.enh0.wav", torch.from_numpy(est * s)[None], 16000, bits=16)
    pj = tmp_path / "pesq.json"
    json.dump({str(i): [2.0 + 0.5 * i] for i in range(3)}, open(pj, "w"))
    got = {}
    for on in ("host", "device"):
        out = evaluate_covl.main([str(wav), str(wav), "--on", on, "--batch", "2", "--pesq-json", str(pj)])
        got[on] = (json.load(open(out / "test_covl.json")), json.load(open(out / "test_summary_covl.json")))
    (hr, hs), (dr, ds) = got["host"], got["device"]
    assert sorted(hr) == sorted(dr) == ["0", "1", "2"] and hs["on"] == "host" and ds["on"] == "device"
    for i in hr:
        assert sorted(hr[i]) == sorted(dr[i]) == ["cbak", "covl", "csig", "llr", "segsnr", "wss"]
        for k in hr[i]:
            assert len(hr[i][k]) == len(dr[i][k]) == 1 and abs(hr[i][k][0] - dr[i][k][0]) <= TOL * max(1, abs(hr[i][k][0])), (i, k)
    for k in ("csig", "cbak", "covl", "llr", "wss", "segsnr"):
        assert abs(hs[k] - ds[k]) <= TOL * max(1, abs(hs[k]))
    assert hs["not_computed"] == ds["not_computed"] == [] and hs["number"] == ds["number"] == 3


def test_evaluate_composite_flag_adds_the_six_keys(tmp_path):
    from diffsep_amd import evaluate as ev
    recs = {}
    for name, extra in (("plain", []), ("comp", ["--composite"])):
        out = tmp_path / name
        ev.main(["--synthetic", "3", "--samples", "8000", "--synthetic-weights", "16", "-N", "2", "--dtype", "f32", "--enhance",
                 "--save-n", "0", "--flat-output", "-o", str(out), "--stoi-on", "device"] + extra)
        recs[name] = (json.load(open(out / "test.json")), json.load(open(out / "test_summary.json")))
    (plain, ps), (comp, cs) = recs["plain"], recs["comp"]
    today = {"batch_idx", "si_sdr", "si_sir", "si_sar", "perm", "pesq", "stoi", "nfe", "runtime", "len_s"}
    assert len(plain) == len(comp) == 3
    for p, c in zip(plain, comp):
        assert set(p) == today and set(c) == today | {"llr", "wss", "segsnr", "csig", "cbak", "covl"}
        assert p["si_sdr"] == c["si_sdr"] and p["perm"] == c["perm"] and p["stoi"] == c["stoi"]
        for k in ("llr", "wss", "segsnr"):
            assert len(c[k]) == 1 and np.isfinite(c[k][0])
        assert c["csig"] is None and c["cbak"] is None and c["covl"] is None
    assert ps["not_computed"] == ["pesq"] and cs["not_computed"] == ["pesq", "csig", "cbak", "covl"]
    assert all(np.isfinite(cs[k]) for k in ("llr", "wss", "segsnr")) and "llr" not in ps
