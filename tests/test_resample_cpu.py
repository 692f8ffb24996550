"""Host side of the sample-rate converter (csrc/resample.hip, ops.Resampler, separate --resample, evaluate_covl --resample): the
float64 definition tests/resample_ref.py states against scipy, the C-ABI's host arithmetic (ratio, length, filter design) against
Python integers and the project's numpy design, and the CLIs' argument handling.  No GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import resample_ref as R
from diffsep_amd import _lib, evaluate_covl, metrics, ops, separate, wavio


def test_direct_form_is_what_resample_poly_computes():
    from scipy.signal import resample_poly
    rng = np.random.default_rng(0)
    for p, q in R.RATIOS:
        h = metrics.resample_filter(p, q)[0] * p
        for n in R.LENGTHS:
            x = rng.standard_normal(n).astype(np.float32)
            y, sabs, cnt = R.direct(x, p, q, h, full=True)
            z = resample_poly(x.astype(np.float64), p, q, window=h / p)
            assert y.shape == z.shape == (R.n_out(n, p, q),)
            assert np.all(np.abs(y - z) <= R.bound64(sabs, cnt)), (p, q, n)
    # the definition itself, term by term, on a case small enough to write out: p / q = 3 / 2, h = 1 .. 7 (L = 3), x = (1, 10, 100)
    h, x = np.arange(1.0, 8.0), np.array([1.0, 10.0, 100.0])
    want = [sum(h[m * 2 + 3 - 3 * j] * x[j] for j in range(3) if 0 <= m * 2 + 3 - 3 * j <= 6) for m in range(5)]
    assert R.direct(x, 3, 2, h).tolist() == want == [4.0 + 10.0, 6.0 + 30.0, 50.0 + 200.0, 70.0 + 400.0, 600.0]


def test_public_names_of_the_host_form():
    assert metrics.resample is metrics._resample and metrics.resample_filter is metrics._resample_filter


def test_ratio_and_length_against_python_integers():
    from math import gcd
    for fs_in, fs_out in [(16000, 8000), (8000, 16000), (44100, 8000), (8000, 44100), (48000, 16000), (48000, 8000), (16000, 10000),
                          (8000, 8000), (22050, 16000), (1000, 1), (1, 1000)]:
        g = gcd(fs_in, fs_out)
        assert ops.resample_ratio(fs_in, fs_out) == (fs_out // g, fs_in // g)
    for p, q in R.RATIOS + [(3, 2), (2, 3), (1, 1)]:
        for n in (0, 1, 2, 37, 1000, 479999, 2 ** 31 - 1, 2 ** 40):
            assert ops.resample_length(n, p, q) == R.n_out(n, p, q) == (n * p + q - 1) // q
            assert ops.resample_length(ops.resample_length(n, p, q), q, p) >= n  # converting back is always a crop
    for bad, word in [((0, 8000), "positive"), ((8000, -1), "positive"), ((44101, 8000), "beyond the largest supported factor 1000"),
                      ((8000, 8001), "beyond the largest supported factor 1000")]:
        with pytest.raises(_lib.DiffsepError, match=word):
            ops.resample_ratio(*bad)
    for bad in [(-1, 1, 2), (5, 0, 2), (5, 2, 0)]:
        with pytest.raises(_lib.DiffsepError, match="resample_length"):
            ops.resample_length(*bad)
    big = (2 ** 63 - 1 - 80) // 441  # the largest n whose n p + q - 1 still fits in 64 bits
    assert ops.resample_length(big, 441, 80) == (big * 441 + 79) // 80
    with pytest.raises(_lib.DiffsepError, match="does not fit in 64 bits"):
        ops.resample_length(big + 1, 441, 80)


# largest |design - numpy design| / largest tap measured over R.RATIOS on the CPU: 3.7e-15 (the 441-based ratios; libm's Bessel
# function and sine against numpy's over 31947 taps); 1.1e-15 for 2:1, 1.7e-16 for 3:1.  The gate is four times that.
DESIGN_MEASURED, DESIGN_GATE = 3.7e-15, 1.5e-14


def test_design_matches_the_numpy_design():
    worst = 0.0
    for p, q in R.RATIOS:
        h = ops.resample_design(p, q)
        g, pp, qq = metrics.resample_filter(p, q)
        L = int(np.ceil(52.0 / (28.714 / (20.0 * max(p, q)))))
        assert (pp, qq) == (p, q) and h.shape == g.shape == (2 * L + 1,)
        d = float(np.max(np.abs(h - g * p)) / np.max(np.abs(g * p)))
        print(f"{p}/{q}: {2 * L + 1} taps, |library - numpy| / max tap = {d:.2e}")
        worst = max(worst, d)
        assert abs(h.sum() - p) <= 1e-12 * p  # the taps sum to p
    assert worst <= DESIGN_GATE, worst
    assert {(p, q): len(ops.resample_design(p, q)) for p, q in [(1, 2), (1, 3), (80, 441)]} == {(1, 2): 147, (1, 3): 219, (80, 441): 31947}
    assert ops.resample_design(1, 1).tolist() == [1.0]  # p = q = 1: a copy, no filter
    l = _lib.lib()
    buf = np.full(147, -7.0)
    assert l.diffsep_resample_design(1, 2, None, 0) == 147  # the count alone
    assert l.diffsep_resample_design(1, 2, buf.ctypes.data_as(C.c_void_p), 146) == -1 and b"do not fit" in l.diffsep_last_error()
    assert np.all(buf == -7.0)
    for bad in [(2, 4), (0, 1), (1001, 1), (1, 1001)]:
        assert l.diffsep_resample_design(*bad, None, 0) == -1 and b"must be reduced" in l.diffsep_last_error()


def test_resampler_create_refusals_need_no_device():
    l = _lib.lib()
    taps = np.ones(7)
    P = taps.ctypes.data_as(C.c_void_p)
    h = C.c_void_p(123)
    for args, word in [((3, 2, None, 7), b"null taps"), ((3, 2, P, 6), b"odd"), ((3, 2, P, 0), b"odd"),
                       ((3, 2, P, (1 << 17) + 1), b"more than 131072 taps"), ((4, 2, P, 7), b"must be reduced"),
                       ((1001, 1, P, 7), b"must be reduced")]:
        assert l.diffsep_resampler_create(*args, C.byref(h)) != 0 and word in l.diffsep_last_error(), args
        assert h.value is None  # no handle comes back from a refusal
        h = C.c_void_p(123)
    l.diffsep_resampler_destroy(None)  # a no-op


def _wav(path, n, sr):
    wavio.save(path, torch.from_numpy(np.sin(np.arange(n) / 7.0).astype(np.float32) * 0.3)[None], sr)
    return path


def test_separate_argument_handling(tmp_path, capsys):
    with pytest.raises(SystemExit):
        separate.main([str(tmp_path), str(tmp_path / "o"), "--resample", "device"])
    assert "invalid choice" in capsys.readouterr().err
    files = [_wav(tmp_path / "a.wav", 8000, 16000), _wav(tmp_path / "b.wav", 4000, 8000), _wav(tmp_path / "c.wav", 441, 44100)]
    plain = separate.Rates(None, 8000, files)
    assert plain.lengths == plain.ns == [8000, 4000, 441] and plain.rates == [16000, 8000, 44100]
    assert not any(plain.converts(sr) for sr in plain.rates)
    for mode in ("file", "model"):
        r = separate.Rates(mode, 8000, files)
        assert r.lengths == [4000, 4000, 80] and r.ns == [8000, 4000, 441]
        assert [r.converts(sr) for sr in r.rates] == [True, False, True]
    with pytest.raises(_lib.DiffsepError, match="beyond the largest supported factor"):
        separate.Rates("file", 8000, [_wav(tmp_path / "d.wav", 10, 8001)])
    # without the flag the warning of the reference is what a mismatch draws, with it nothing
    capsys.readouterr()
    assert plain.load(0).shape == (1, 8000) and "this model expects 8000 Hz, but the file is 16000 Hz" in capsys.readouterr().out
    assert separate.Rates("file", 8000, files).load(0).shape == (1, 8000) and capsys.readouterr().out == ""


def test_files_at_the_model_rate_meet_no_resampler(tmp_path, monkeypatch):
    files = [_wav(tmp_path / "a.wav", 4000, 8000), _wav(tmp_path / "b.wav", 3000, 8000)]

    def boom(*a, **k):
        raise AssertionError("a resampler object was made for a file at the model's rate")
    monkeypatch.setattr(ops, "Resampler", boom)
    for mode in (None, "file", "model"):
        r = separate.Rates(mode, 8000, files)
        wavs = [r.load(i) for i in range(2)]
        rows = r.rows([0, 1], wavs, "cpu")
        assert all(a is b for a, b in zip(rows, wavs)) and r.lengths == [4000, 3000]
        seps = [torch.zeros(2, 4000), torch.zeros(2, 3000)]
        back = r.restore([0, 1], seps)
        assert all(x is s and sr == 8000 for (x, sr), s in zip(back, seps))


def test_evaluate_covl_refuses_or_converts_on_the_host(tmp_path):
    import json
    wav = tmp_path / "exp" / "wav" / "test"
    wav.mkdir(parents=True)
    rng = np.random.default_rng(3)
    t = np.arange(8000) / 8000.0
    ref = 0.3 * np.sin(2 * np.pi * 440 * t) * (1 + 0.5 * np.sin(2 * np.pi * 3 * t)) + 0.01 * rng.standard_normal(8000)
    est = ref + 0.02 * rng.standard_normal(8000)
    wavio.save(wav / "0000.tgt0.wav", torch.from_numpy(ref.astype(np.float32))[None], 8000, bits=16)
    wavio.save(wav / "0000.enh0.wav", torch.from_numpy(est.astype(np.float32))[None], 8000, bits=16)
    with pytest.raises(SystemExit, match="sample rate 8000, not 16000"):
        evaluate_covl.main([str(wav), str(wav), "--on", "host"])
    out = evaluate_covl.main([str(wav), str(wav), "--on", "host", "--resample"])
    got = json.load(open(out / "test_covl.json"))["0"]
    r16 = [metrics.resample(wavio.load(wav / f"0000.{k}0.wav")[0][0].numpy().astype(np.float64), 16000, 8000).astype(np.float32)
           for k in ("tgt", "enh")]
    assert len(r16[0]) == 16000
    want = metrics.composite(r16[0], r16[1], 16000)
    assert got["llr"] == [want["llr"]] and got["wss"] == [want["wss"]] and got["segsnr"] == [want["segsnr"]]
