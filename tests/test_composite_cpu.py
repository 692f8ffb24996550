"""Host side of the composite enhancement measures: diffsep_amd.metrics.composite / eval_composite against the values the
reference's evaluate_covl.py gave (tests/golden/golden_composite.npz, written by tests/golden/gen_golden_composite.py), the
integer forms of its frame count and trimming count, the host-only workspace function of the C-ABI, and the
`python -m diffsep_amd.evaluate_covl --on host` command line.

Tolerances.  The reference's LLR and the preprocessing of its SSNR are float32, metrics.composite is float64 throughout, so
those deviations are what the generator measured (`dev_*`, per shape); 4 x the recorded value is allowed, because another
numpy / BLAS build may sum the reference's float32 terms in another, equally valid order and move it by about its own rounding
noise.  The mean segmental SNR moves by no more than its frames do.  WSS is float64 on both sides: 1e-9 max(1, |v|)."""
import json
import math
import os

import numpy as np
import pytest
import torch

import composite_cases as CC
from conftest import GOLDEN_DIR
from diffsep_amd import _lib, evaluate_covl, metrics, ops, wavio


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLDEN_DIR, "golden_composite.npz")))


def _close(a, b, tol):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(np.all((np.abs(a - b) <= tol) | (np.isnan(a) & np.isnan(b))))


@pytest.mark.parametrize("fs,T", CC.SHAPES)
def test_host_form_matches_the_reference(gold, fs, T):
    dev_llr_frame, dev_llr_mean, _, dev_seg_frame = gold[f"dev_fs{fs}_T{T}"]
    for i in range(CC.N_UTT):
        ref, est = CC.pair(i, T, fs)
        r0, e0 = ref.copy(), est.copy()
        got = metrics.composite(ref, est, fs)
        assert np.array_equal(ref, r0) and np.array_equal(est, e0)  # the arguments are not modified
        k = CC.key(fs, T, i)
        n = CC.FRAMES[(fs, T)]
        assert got["n_frames"] == n == len(gold[k + "_wss_frames"])
        llr_f, wss_f, seg_f, agg = (gold[k + s] for s in ("_llr_frames", "_wss_frames", "_segsnr_frames", "_agg"))
        if n:
            print(f"{k}: llr frame {np.max(np.abs(got['llr_frames'] - llr_f)):.3e} mean {abs(got['llr'] - agg[0]):.3e} "
                  f"wss frame {np.max(np.abs(got['wss_frames'] - wss_f)):.3e} segsnr frame "
                  f"{np.max(np.abs(got['segsnr_frames'] - seg_f)):.3e} mean {abs(got['segsnr'] - agg[2]):.3e}")
        assert _close(got["llr_frames"], llr_f, 4 * dev_llr_frame)
        assert _close(got["segsnr_frames"], seg_f, 4 * dev_seg_frame)
        assert _close(got["wss_frames"], wss_f, 1e-9 * np.maximum(1, np.abs(wss_f)))
        if n == 0:
            assert all(math.isnan(got[q]) for q in ("llr", "wss", "segsnr")) and np.all(np.isnan(agg))
        else:
            assert abs(got["llr"] - agg[0]) <= 4 * dev_llr_mean
            assert abs(got["wss"] - agg[1]) <= 1e-9 * max(1, abs(agg[1]))
            assert abs(got["segsnr"] - agg[2]) <= 4 * dev_seg_frame


def test_zero_stretch_hits_the_guards(gold):
    # frames inside the all-zero stretch of the reference: LLR log(1e-10 / 1e-10) = 0 and the -10 dB clamp, in the golden file too
    k = CC.key(16000, 16000, 0)
    ref, est = CC.pair(0, 16000, 16000)
    got = metrics.composite(ref, est, 16000)
    inside = [f for f in range(got["n_frames"]) if 4000 <= f * 120 and f * 120 + 480 <= 5000]
    assert len(inside) >= 4
    for f in inside:
        assert got["llr_frames"][f] == 0.0 == gold[k + "_llr_frames"][f]
        assert got["segsnr_frames"][f] == -10.0 == gold[k + "_segsnr_frames"][f]
    assert got["segsnr_frames"].max() <= 35.0 and got["segsnr_frames"].min() >= -10.0


def test_eval_composite_matches_the_reference_formulas(gold):
    seen = set()
    for fs, T in CC.SHAPES:
        for i in range(CC.N_UTT):
            k = CC.key(fs, T, i)
            agg, cov = gold[k + "_agg"], gold[k + "_cov"]
            for j, p in enumerate(CC.PESQ_STUBS):
                got = metrics.eval_composite(agg[0], agg[1], agg[2], p)
                assert list(got) == ["csig", "cbak", "covl"]
                if CC.FRAMES[(fs, T)] == 0:
                    continue
                for q, name in enumerate(got):
                    assert abs(got[name] - cov[j, q]) <= 1e-12, (k, p, name, got[name], cov[j, q])
                    seen.add(float(cov[j, q]))
    assert 5.0 in seen  # the upper trim is in the golden file (pesq stub 4.5) ...
    low = metrics.eval_composite(3.0, 80.0, -10.0, 1.0)  # ... the lower one: a poor estimate
    assert low == {"csig": 1, "cbak": 1, "covl": 1}
    assert metrics.eval_composite(0.0, 0.0, 35.0, 4.5) == {"csig": 5, "cbak": 5, "covl": 5}
    assert metrics.eval_composite(0.1, 5.0, 7.0, None) == {"csig": None, "cbak": None, "covl": None}


@pytest.mark.parametrize("fs", [16000, 8000])
def test_frame_count_is_the_reference_expression(fs):
    winlength = round(30 * fs / 1000.0)
    skiprate = np.floor(winlength / 4)
    for n in range(0, 20001):
        want = int(n / skiprate - (winlength / skiprate))  # evaluate_covl.py:249,374 (:131 with an integer skiprate: the same)
        assert want == int(n / (winlength // 4) - (winlength / (winlength // 4)))
        assert metrics.composite_num_frames(n, fs) == max(0, want), n
    for (f, T), frames in CC.FRAMES.items():
        assert metrics.composite_num_frames(T, f) == frames


def test_trim_count_is_round_half_even_of_the_double_product():
    for n in range(0, 2001):
        assert metrics.composite_trim_count(n) == int(round(n * 0.95)) == int(np.rint(np.float64(n) * 0.95))
    assert metrics.composite_trim_count(10) == 10 and metrics.composite_trim_count(30) == 28


def test_slope_margin_of_every_input():
    worst = np.inf
    for fs, T in CC.SHAPES:
        for i in range(CC.N_UTT):
            for x in CC.pair(i, T, fs):
                worst = min(worst, CC.slope_margin(x, fs))
    print(f"smallest non-zero |slope| over all inputs: {worst:.3e} dB")
    assert worst >= CC.MIN_MARGIN


def test_unsupported_rate_and_length_mismatch():
    x = CC.pair(0, 1680, 16000)[0]
    with pytest.raises(ValueError, match="sample rate"):
        metrics.composite(x, x, 44100)
    with pytest.raises(ValueError, match="same length"):
        metrics.composite(x, x[:-1], 16000)


def test_workspace_bytes_is_host_arithmetic():
    l = _lib.lib()
    f = l.diffsep_composite_workspace_bytes
    for fs, T in CC.SHAPES:
        assert f(1, 1, T, fs) > 0 and f(4, 2, T, fs) > 0
    for fs in (16000, 8000):
        last = 0
        for B in (1, 2, 3, 16):
            v = f(B, 2, 16100, fs)
            assert v >= last > -1 and v > 0
            last = v
        assert f(16, 2, 16100, fs) > f(1, 2, 16100, fs)
        last = 0
        for T in (1, 599, 600, 1680, 16000, 16100, 160000):
            v = f(4, 2, T, fs)
            assert v >= last and v > 0
            last = v
        assert f(4, 2, 160000, fs) > f(4, 2, 1680, fs)
    for bad, word in (((1, 2, 16000, 44100), b"sample rate"), ((1, 4, 16000, 16000), b"bad shape"), ((1, 0, 16000, 16000), b"bad shape"),
                      ((1, 2, 0, 16000), b"bad shape"), ((1, 2, -5, 16000), b"bad shape"), ((0, 2, 16000, 16000), b"bad shape"),
                      ((1, 1, 120 * 65537 + 480, 16000), b"frames")):
        assert f(*bad) == -1
        assert word in l.diffsep_last_error(), (bad, l.diffsep_last_error())
    assert f(1, 1, 120 * 65536 + 480, 16000) > 0  # the most frames per row the on-device ranking takes
    with pytest.raises(_lib.DiffsepError, match="sample rate"):
        ops.composite_workspace_bytes(1, 2, 16000, 44100)
    assert ops.composite_workspace_bytes(1, 2, 16000, 16000) == f(1, 2, 16000, 16000)


def _write_folder(root, n=2, fs=16000):
    wav = root / "exp" / "wav" / "test"
    wav.mkdir(parents=True)
    for i in range(n):
        ref, est = CC.pair(i, 4080 + 120 * i, fs)
        s = 0.5 / np.abs(est).max()
        wavio.save(wav / f"{i:04d}.tgt0.wav", torch.from_numpy(ref * s)[None], fs, bits=16)
        wavio.save(wav / f"{i:04d}.enh0.wav", torch.from_numpy(est * s)[None], fs, bits=16)
    return wav


def test_evaluate_covl_on_host(tmp_path):
    wav = _write_folder(tmp_path)
    out = evaluate_covl.main([str(wav), str(wav), "--on", "host"])
    assert out == tmp_path / "exp"
    rec = json.load(open(out / "test_covl.json"))
    summ = json.load(open(out / "test_summary_covl.json"))
    assert sorted(rec) == ["0", "1"]
    for i in ("0", "1"):
        assert sorted(rec[i]) == ["cbak", "covl", "csig", "llr", "segsnr", "wss"]
        assert rec[i]["csig"] == rec[i]["cbak"] == rec[i]["covl"] == [None]
        ref, est = (wavio.load(wav / f"{int(i):04d}.{w}0.wav")[0][0].numpy() for w in ("tgt", "enh"))
        want = metrics.composite(ref, est, 16000)
        assert rec[i]["llr"] == [want["llr"]] and rec[i]["wss"] == [want["wss"]] and rec[i]["segsnr"] == [want["segsnr"]]
    assert summ["number"] == 2 and summ["not_computed"] == ["csig", "cbak", "covl"] and summ["on"] == "host"
    assert abs(summ["llr"] - np.mean([rec[i]["llr"][0] for i in rec])) < 1e-12 and "csig" not in summ

    pj = tmp_path / "pesq.json"
    json.dump({"0": [2.5], "1": [1.0]}, open(pj, "w"))
    evaluate_covl.main([str(wav), str(wav), "--on", "host", "--pesq-json", str(pj)])
    rec2 = json.load(open(out / "test_covl.json"))
    summ2 = json.load(open(out / "test_summary_covl.json"))
    assert summ2["not_computed"] == []
    for i, p in (("0", 2.5), ("1", 1.0)):
        want = metrics.eval_composite(rec[i]["llr"][0], rec[i]["wss"][0], rec[i]["segsnr"][0], p)
        for k, v in want.items():
            assert rec2[i][k] == [v] and 1 <= v <= 5
    assert abs(summ2["covl"] - np.mean([rec2[i]["covl"][0] for i in rec2])) < 1e-12
    json.dump({"0": [2.5]}, open(pj, "w"))
    with pytest.raises(SystemExit, match="sample 1"):
        evaluate_covl.main([str(wav), str(wav), "--on", "host", "--pesq-json", str(pj)])


def test_evaluate_covl_reads_the_names_evaluate_writes_and_refuses_other_rates(tmp_path):
    wav = tmp_path / "run" / "wav" / "test"
    wav.mkdir(parents=True)
    ref, est = CC.pair(0, 4080, 16000)
    wavio.save(wav / "000_tgt0.wav", torch.from_numpy(ref)[None], 16000, bits=32)
    wavio.save(wav / "000_enh0.wav", torch.from_numpy(est)[None], 16000, bits=32)
    wavio.save(wav / "000_mix.wav", torch.from_numpy(est)[None], 16000, bits=32)
    out = evaluate_covl.main([str(wav), str(wav), "--on", "host"])
    rec = json.load(open(out / "test_covl.json"))
    assert list(rec) == ["0"] and rec["0"]["wss"] == [metrics.composite(ref, est, 16000)["wss"]]
    bad = tmp_path / "other" / "wav" / "test"
    bad.mkdir(parents=True)
    wavio.save(bad / "0000.tgt0.wav", torch.from_numpy(ref)[None], 22050)
    wavio.save(bad / "0000.enh0.wav", torch.from_numpy(est)[None], 22050)
    with pytest.raises(SystemExit, match=r"0000\.tgt0\.wav.*22050"):
        evaluate_covl.main([str(bad), str(bad), "--on", "host"])
