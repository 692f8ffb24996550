"""The device sample-rate converter (csrc/resample.hip through diffsep_resample / ops.Resampler) against the float64 definition of
tests/resample_ref.py: bit for bit where every sum is exact (integer taps and samples over every tile boundary, impulses through
the designed filters), within the summation-error bound of K products elsewhere (nothing measured: resample_ref.bound64 / bound32),
bit-identical rows alone, in a batch and on a second stream, tones through the designed filters at the gates the host form holds,
the refusals of the C-ABI, and separate --resample / evaluate_covl --resample end to end."""
import ctypes as C
import functools
import json

import numpy as np
import pytest
import torch

import resample_ref as R
from diffsep_amd import _lib, evaluate_covl, inflight, metrics, ops, wavio
from diffsep_amd import separate as sep_cli

pytestmark = pytest.mark.gpu


def bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else np.int32)


def _both(rs, x, lengths=None):
    """(float64 output, float32 output, new lengths) of one resampler on one input"""
    y64, new = rs(x, lengths=lengths, dtype=torch.float64)
    y32, new32 = rs(x, lengths=lengths, dtype=torch.float32)
    assert y64.dtype == torch.float64 and y32.dtype == torch.float32 and y64.shape == y32.shape
    assert (new.tolist() if isinstance(new, torch.Tensor) else new) == (new32.tolist() if isinstance(new32, torch.Tensor) else new32)
    return y64.cpu().numpy(), y32.cpu().numpy(), new


# ------------------------------------------------------------------------------------------------ 1. exact, every tile boundary
@pytest.mark.parametrize("p,q", [(3, 2), (2, 3)])
def test_integer_taps_and_samples_are_exact_over_every_tile_boundary(p, q):
    rng = np.random.default_rng(p)
    h = rng.integers(-8, 9, 7).astype(np.float64)
    h[[0, 6]] = [-8.0, 5.0]  # both end taps in use
    rows = 740
    x = rng.integers(-64, 65, (rows, rows)).astype(np.float32)
    rs = ops.Resampler(q, p, taps=h)
    assert (rs.p, rs.q) == (p, q)
    n_max = R.n_out(rows, p, q)
    for rpl in (1, 2):
        lengths = list(range(1, rows + 1)) if rpl == 1 else list(range(2, rows + 1, 2))
        xin = torch.from_numpy(x).cuda().reshape((rows, rows) if rpl == 1 else (rows // 2, 2, rows))
        y64, y32, new = _both(rs, xin, lengths)  # ONE launch each: 740 rows, n_out = 1 .. 1110 for 3 / 2
        y64, y32 = y64.reshape(rows, n_max), y32.reshape(rows, n_max)
        assert new == [R.n_out(n, p, q) for n in lengths]
        for r in range(rows):
            n = lengths[r // rpl]
            want = np.zeros(n_max)
            want[:R.n_out(n, p, q)] = R.direct(x[r, :n], p, q, h)
            assert np.array_equal(bits(y64[r]), bits(want)), (rpl, r)  # the zero fill past n_out included
            assert np.array_equal(bits(y32[r]), bits(want.astype(np.float32))), (rpl, r)
    if (p, q) == (3, 2):
        assert n_max == 1110 and sorted(set(new)) == list(range(3, 1111, 3))


def test_ratios_whose_tile_span_passes_lds_take_the_gather_kernel():
    # 1 / 70 with 7 taps: a tile of 256 outputs spans 255 * 70 + 8 samples, beyond the 16000 floats a block stages -> the kernel
    # that gathers x from global memory; exact as above.  1 / 100 with the designed filter (7245 taps per output): the bound.
    rng = np.random.default_rng(70)
    h = rng.integers(-8, 9, 7).astype(np.float64)
    lens = [1, 69, 70, 71, 139, 141, 20000, 17921]  # n_out 1, 1, 1, 2, 2, 3, 286 (two blocks), 257
    x = rng.integers(-64, 65, (len(lens), max(lens))).astype(np.float32)
    y64, y32, new = _both(ops.Resampler(70, 1, taps=h), torch.from_numpy(x).cuda(), lens)
    assert new == [1, 1, 1, 2, 2, 3, 286, 257] and y64.shape == (len(lens), 286)
    for r, n in enumerate(lens):
        want = np.zeros(286)
        want[:new[r]] = R.direct(x[r, :n], 1, 70, h)
        assert np.array_equal(bits(y64[r]), bits(want)) and np.array_equal(bits(y32[r]), bits(want.astype(np.float32))), r
    xr = R.random_rows(100, (2, 30000))
    hd = ops.resample_design(1, 100)
    y64, y32, new = _both(ops.Resampler(100, 1), torch.from_numpy(xr).cuda(), [30000, 12345])
    assert len(hd) == 7245 and new == [300, 124]
    for r, n in enumerate((30000, 12345)):
        y, sabs, cnt = R.direct(xr[r, :n], 1, 100, hd, full=True)
        assert np.all(np.abs(y64[r, :new[r]] - y) <= R.bound64(sabs, cnt)) and not y64[r, new[r]:].any()
        assert np.all(np.abs(y32[r, :new[r]].astype(np.float64) - y) <= R.bound32(sabs, cnt, y))


# ------------------------------------------------------------------------------------------------ 2. impulses
@pytest.mark.parametrize("p,q", [(1, 2), (2, 1), (80, 441), (441, 80)])
def test_impulse_returns_the_taps_bit_for_bit(p, q):
    n, h = 37, ops.resample_design(p, q)
    L = (len(h) - 1) // 2
    where = [0, 1, n - 1]
    x = np.zeros((3, n), np.float32)
    x[np.arange(3), where] = 1.0
    y, new = ops.Resampler(q, p)(torch.from_numpy(x).cuda(), dtype=torch.float64)
    y = y.cpu().numpy()
    m = np.arange(R.n_out(n, p, q))
    assert new == [len(m)] * 3 and y.shape == (3, len(m))
    for r, j in enumerate(where):
        idx = m * q + L - p * j
        want = np.where((idx >= 0) & (idx <= 2 * L), h[np.clip(idx, 0, 2 * L)], 0.0) + 0.0
        assert np.array_equal(bits(y[r]), bits(want)), (p, q, j)
        assert np.count_nonzero(want) > 0


# ------------------------------------------------------------------------------------------------ 3. element bound
@functools.lru_cache(maxsize=None)
def _case(p, q, k):
    """(x [3,2,T] float32, lengths, {(b, s): (direct, sum |h x|, products)}) of one ratio and one set of lengths, computed once"""
    lens = R.BOUND_LENGTHS[k]
    x = R.random_rows(1000 * p + q + k, (3, 2, max(lens)))
    h = ops.resample_design(p, q)
    ref = {(b, s): R.direct(x[b, s, :lens[b]], p, q, h, full=True) for b in range(3) for s in range(2)}
    return x, lens, ref


@pytest.mark.parametrize("k", [0, 1])
@pytest.mark.parametrize("p,q", R.BOUND_RATIOS)
def test_random_input_within_the_summation_bound(p, q, k):
    x, lens, ref = _case(p, q, k)
    rs = ops.Resampler(q, p)
    y64, y32, new = _both(rs, torch.from_numpy(x).cuda(), lens)
    assert new == [R.n_out(n, p, q) for n in lens] and y64.shape == (3, 2, R.n_out(max(lens), p, q))
    worst = 0.0
    for (b, s), (y, sabs, cnt) in ref.items():
        n = len(y)
        assert cnt.max() <= (len(ops.resample_design(p, q)) + p - 1) // p
        e64, e32 = np.abs(y64[b, s, :n] - y), np.abs(y32[b, s, :n].astype(np.float64) - y)
        worst = max(worst, float(np.max(e64 / np.maximum(R.bound64(sabs, cnt), 1e-300))))
        assert np.all(e64 <= R.bound64(sabs, cnt)), (b, s, float(np.max(e64 - R.bound64(sabs, cnt))))
        assert np.all(e32 <= R.bound32(sabs, cnt, y)), (b, s)
        assert not y64[b, s, n:].any() and not y32[b, s, n:].any()  # zeros past the row's own n_out
    print(f"{p}/{q} lengths {lens}: largest |device - direct| = {worst:.3f} of the float64 bound")
    # device lengths in, device lengths out (diffsep_resample's lengths_out), the same rows
    yd, newd = rs(torch.from_numpy(x).cuda(), lengths=torch.tensor(lens, dtype=torch.int32, device="cuda"), dtype=torch.float64)
    assert newd.dtype == torch.int32 and newd.tolist() == new and np.array_equal(bits(yd), bits(y64))


# ------------------------------------------------------------------------------------------------ 4. bit identity
@pytest.mark.parametrize("p,q", [(2, 1), (80, 441), (441, 80)])
def test_rows_alone_in_a_batch_and_on_a_second_stream_are_the_same_bits(p, q):
    x, lens, _ = _case(p, q, 1)
    rs = ops.Resampler(q, p)
    xd = torch.from_numpy(x).cuda()
    busy = torch.from_numpy(R.random_rows(5, (16, 2, 32000))).cuda()
    y64, new = rs(xd, lengths=lens, dtype=torch.float64)
    y32, _ = rs(xd, lengths=lens)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    for _ in range(3):
        rs(busy)  # the first stream runs another resample meanwhile
    with torch.cuda.stream(side):
        z64, _ = rs(xd, lengths=lens, dtype=torch.float64)
        z32, _ = rs(xd, lengths=lens)
    torch.cuda.synchronize()
    assert np.array_equal(bits(y64), bits(z64)) and np.array_equal(bits(y32), bits(z32))
    for b in range(3):
        for s in range(2):
            one = xd[b, s, :lens[b]].contiguous()[None]  # rows = 1, T = the row's own length
            a64, n1 = rs(one, dtype=torch.float64)
            a32, _ = rs(one)
            assert n1 == [new[b]]
            assert np.array_equal(bits(a64[0]), bits(y64[b, s, :new[b]])) and np.array_equal(bits(a32[0]), bits(y32[b, s, :new[b]]))


# ------------------------------------------------------------------------------------------------ 5. tones
@pytest.mark.parametrize("fs_in,fs_out,f0,keeps", [(16000, 8000, 1000, True), (8000, 16000, 1000, True), (16000, 10000, 6500, False)])
def test_tones_through_the_designed_filters(fs_in, fs_out, f0, keeps):
    # the gates tests/test_metrics_cpu.py holds the host form to, away from the edge outputs
    x = np.sin(2 * np.pi * f0 * np.arange(fs_in) / fs_in).astype(np.float32)
    g, p, q = metrics.resample_filter(fs_out, fs_in)
    y, new = ops.Resampler(fs_in, fs_out)(torch.from_numpy(x).cuda()[None], dtype=torch.float64)
    y = y.cpu().numpy()[0]
    assert new == [fs_out] and y.shape == (fs_out,)
    want = np.sin(2 * np.pi * f0 * np.arange(fs_out) / fs_out) if keeps else np.zeros(fs_out)
    assert np.max(np.abs(y[500:-500] - want[500:-500])) < 2e-3
    # the host form on the same taps: within the bound of the element test
    yt, _ = ops.Resampler(fs_in, fs_out, taps=g * p)(torch.from_numpy(x).cuda()[None], dtype=torch.float64)
    host = metrics.resample(x.astype(np.float64), fs_out, fs_in)
    _, sabs, cnt = R.direct(x, p, q, g * p, full=True)
    assert host.shape == (fs_out,) and np.all(np.abs(yt.cpu().numpy()[0] - host) <= R.bound64(sabs, cnt))


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_write_nothing():
    l = _lib.lib()
    h = np.arange(1.0, 8.0)
    r = C.c_void_p()
    assert l.diffsep_resampler_create(3, 2, h.ctypes.data_as(C.c_void_p), 7, C.byref(r)) == 0 and r.value
    T, rows = 100, 2
    x = torch.ones((rows, T), device="cuda")
    y = torch.full((rows, 150), -7.0, dtype=torch.float64, device="cuda")
    lo = torch.full((rows,), -7, dtype=torch.int32, device="cuda")
    P = lambda t: C.c_void_p(t.data_ptr())

    def call(rr=r, xp=P(x), ldx=T, yp=P(y), ldy=150, n=rows, T_=T, dt=_lib.F64, rpl=1):
        return l.diffsep_resample(rr, xp, ldx, yp, ldy, n, T_, None, rpl, P(lo), dt, None)
    for kw, word in [(dict(ldy=149), b"ldy 149 < ceil(T p / q) = 150"), (dict(T_=2 ** 31, ldx=2 ** 31, ldy=2 ** 33), b"T must be in 1..2^31-1"),
                     (dict(T_=0), b"T must be in"), (dict(rr=None), b"null pointer"), (dict(xp=None), b"null pointer"),
                     (dict(yp=None), b"null pointer"), (dict(dt=1), b"unknown out_dtype 1"), (dict(dt=7), b"unknown out_dtype 7"),
                     (dict(ldx=T - 1), b"ldx 99 < T 100"), (dict(n=0), b"rows must be"), (dict(rpl=0), b"rows_per_length")]:
        assert call(**kw) != 0 and word in l.diffsep_last_error(), (kw, l.diffsep_last_error())
    torch.cuda.synchronize()
    assert bool((y == -7.0).all()) and bool((lo == -7).all())
    assert call() == 0  # ... and the same arguments unbroken do run
    torch.cuda.synchronize()
    want = R.direct(np.ones(T), 3, 2, h)
    assert np.array_equal(y.cpu().numpy(), np.stack([want, want])) and lo.tolist() == [150, 150]
    l.diffsep_resampler_destroy(r)
    with pytest.raises(_lib.DiffsepError, match="odd"):
        ops.Resampler(2, 3, taps=np.ones(6))(x)
    with pytest.raises(ValueError, match="float32"):
        ops.Resampler(2, 3)(x.double())
    # no samples: empty rows and zero lengths, no launch
    y0, n0 = ops.Resampler(2, 3)(torch.empty((2, 0), device="cuda"), lengths=[0, 0])
    assert y0.shape == (2, 0) and n0 == [0, 0]


# ------------------------------------------------------------------------------------------------ 7. CLIs
def _model16():
    """(model, sampler arguments) as `separate --synthetic-weights 16 -N 2 --dtype f32` builds them"""
    import argparse
    return sep_cli.get_model(argparse.Namespace(synthetic_weights=16, dtype="f32", device="cuda:0", fp32_steps=None, N=2,
                                                corrector_steps=None, snr=None, denoise=True, schedule=None))


def _tone_mix(i, n, fs):
    """a band-limited two-voice mixture (below 3 kHz: the same material at 8 and at 16 kHz), [1, n] float32"""
    t = np.arange(n) / fs
    a = np.sin(2 * np.pi * (220 + 30 * i) * t) * (1 + 0.5 * np.sin(2 * np.pi * 3 * t))
    b = np.sin(2 * np.pi * (1310 + 70 * i) * t + 0.3) * (1 + 0.5 * np.cos(2 * np.pi * 5 * t))
    return torch.from_numpy((0.2 * a + 0.15 * b).astype(np.float32))[None]


def test_separate_cli_resample_file(tmp_path):
    # (nf = 16: the narrowest model the suite runs the CLI at; fp32 engine: a file's result does not depend on its batch)
    ind = tmp_path / "in"
    ind.mkdir()
    spec = {"a16": (8000, 16000), "b16": (7999, 16000), "c08": (4000, 8000)}  # 0.5 s each; 7999 -> 4000 -> 8000: a crop of one
    for i, (name, (n, fs)) in enumerate(spec.items()):
        wavio.save(ind / f"{name}.wav", _tone_mix(i, n, fs), fs, bits=32)
    common = ["--synthetic-weights", "16", "-N", "2", "--dtype", "f32", "--batch", "3", "--seed", "1"]
    sep_cli.main([str(ind), str(tmp_path / "file"), "--resample", "file"] + common)
    sep_cli.main([str(ind), str(tmp_path / "chunk"), "--resample", "file", "--chunk", "0.32", "--overlap", "0.1"] + common)
    sep_cli.main([str(ind), str(tmp_path / "model"), "--resample", "model"] + common)
    sep_cli.main([str(ind), str(tmp_path / "plain")] + common)
    got = {}
    for run in ("file", "chunk", "model", "plain"):
        for name, (n, fs) in spec.items():
            for s in ("s0", "s1"):
                y, sr = wavio.load(tmp_path / run / s / f"{name}.wav")
                at_model = run == "model" and fs != 8000
                assert sr == (8000 if at_model else fs) and y.shape == (1, 4000 if at_model else n) and bool(torch.isfinite(y).all())
                got[run, name, s] = y[0]
    # the manual chain with the same seeds: Resampler -> separate_on_device -> Resampler -> crop
    model, kw = _model16()
    seeds = inflight.utterance_seeds(3, 1)
    down, up = ops.Resampler(16000, 8000), ops.Resampler(8000, 16000)
    for i, name in enumerate(("a16", "b16")):
        n = spec[name][0]
        mix8, (n8,) = down(wavio.load(ind / f"{name}.wav")[0][:1].cuda()[None])
        assert n8 == 4000
        sep8 = sep_cli.separate_on_device(mix8, model, kw, "cuda:0", lengths=[n8], seeds=[seeds[i]])
        back, (nb,) = up(sep8)
        assert nb == 8000 >= n
        for k, s in enumerate(("s0", "s1")):
            assert np.array_equal(bits(got["file", name, s]), bits(back[0, k, :n])), (name, s)
            assert np.array_equal(bits(got["model", name, s]), bits(sep8[0, k, :n8])), (name, s)
    # the file at the model's rate: what a run without the flag writes (where the 16 kHz files go to the model as they are)
    for s in ("s0", "s1"):
        assert np.array_equal(bits(got["file", "c08", s]), bits(got["plain", "c08", s]))
        assert np.array_equal(bits(got["model", "c08", s]), bits(got["plain", "c08", s]))
        assert not np.array_equal(bits(got["file", "a16", s]), bits(got["plain", "a16", s]))
    # --chunk 0.32 --overlap 0.1: a window shorter than the files; the whole file is converted, then cut, stitched, converted back
    window, overlap = 2560, 800
    starts = ops.longform_plan(4000, window, overlap)
    for name, i in (("a16", 0), ("c08", 2)):
        n, fs = spec[name]
        x = wavio.load(ind / f"{name}.wav")[0][:1].cuda()[None]
        mix8 = down(x)[0] if fs != 8000 else x
        ws = inflight.window_seeds(seeds[i], len(starts))
        wins = [sep_cli.separate_on_device(mix8[:, :, st:st + window].contiguous(), model, kw, "cuda:0", lengths=[window], seeds=[sd])
                for st, sd in zip(starts, ws)]
        out, _ = ops.longform_stitch(torch.cat(wins), 4000, overlap)
        out = up(out[None])[0][0, :, :n] if fs != 8000 else out
        for k, s in enumerate(("s0", "s1")):
            assert np.array_equal(bits(got["chunk", name, s]), bits(out[k])), (name, s)


def test_separate_cli_resample_streams_do_not_change_the_files(tmp_path):
    """--streams 2 against --streams 1, plain and with --chunk.  --batch 1 --chunk 0.32 cuts the 2 s file into 9 windows that go
    to the two workers in turn: every window after the first is cut, on the OTHER stream, from the row the first window's launch
    converted.  fp32 engine: the throughput mode of --streams K > 1 leaves its results bit for bit."""
    ind = tmp_path / "in"
    ind.mkdir()
    spec = {"a16": (32000, 16000), "b08": (4000, 8000), "c16": (7999, 16000), "d44": (22050, 44100)}
    for i, (name, (n, fs)) in enumerate(spec.items()):
        wavio.save(ind / f"{name}.wav", _tone_mix(i, n, fs), fs, bits=32)
    common = ["--synthetic-weights", "16", "-N", "2", "--dtype", "f32", "--seed", "3", "--resample", "file"]
    for tag, extra in (("plain", ["--batch", "2"]), ("chunk", ["--batch", "1", "--chunk", "0.32", "--overlap", "0.1"])):
        for k in (1, 2):
            sep_cli.main([str(ind), str(tmp_path / f"{tag}{k}"), "--streams", str(k)] + extra + common)
        for name, (n, fs) in spec.items():
            for s in ("s0", "s1"):
                a, sra = wavio.load(tmp_path / f"{tag}1" / s / f"{name}.wav")
                b, srb = wavio.load(tmp_path / f"{tag}2" / s / f"{name}.wav")
                assert sra == srb == fs and a.shape == b.shape == (1, n) and bool(torch.isfinite(a).all())
                assert np.array_equal(bits(a), bits(b)), (tag, name, s)
    assert len(ops.longform_plan(16000, 2560, 800)) == 9


def test_separate_cli_resample_with_the_ode_sampler(tmp_path):
    # --sampler ode: one engine call per file (--batch 1) and the files of a batch behind one call (--batch 3) write the same files
    ind = tmp_path / "in"
    ind.mkdir()
    spec = {"a16": (8001, 16000), "b08": (4000, 8000), "c16": (7000, 16000)}
    for i, (name, (n, fs)) in enumerate(spec.items()):
        wavio.save(ind / f"{name}.wav", _tone_mix(i, n, fs), fs, bits=32)
    common = ["--synthetic-weights", "16", "--dtype", "f32", "--sampler", "ode", "--rtol", "1e-3", "--atol", "1e-3", "--seed", "11",
              "--resample", "file"]
    sep_cli.main([str(ind), str(tmp_path / "b3"), "--batch", "3"] + common)
    sep_cli.main([str(ind), str(tmp_path / "b1"), "--batch", "1"] + common)
    for name, (n, fs) in spec.items():
        for s in ("s0", "s1"):
            a, sra = wavio.load(tmp_path / "b3" / s / f"{name}.wav")
            b, srb = wavio.load(tmp_path / "b1" / s / f"{name}.wav")
            assert sra == srb == fs and a.shape == b.shape == (1, n) and bool(torch.isfinite(a).all())
            assert np.array_equal(bits(a), bits(b)), (name, s)


def test_evaluate_covl_resample_on_device_matches_the_host_form(tmp_path):
    """An 8 kHz pair through evaluate_covl --resample --batch 2 against metrics.composite of the host-resampled signals, at the
    1e-9 max(1, |v|) tests/test_composite_gpu.py holds between the device and the host measures.  The inputs are that file's
    material (composite_cases.pair) at 8 kHz.  Measured on the MI355X: the device-resampled float32 signals equal the
    host-resampled ones in every sample (asserted below through the device measures, bit for bit), so what is left is the
    distance between the two forms of the measures themselves on a band-limited signal: LLR 6.2e-10 and 9.4e-10 of the bound's
    1e-9, WSS and segmental SNR below 1e-15 (an LPC fit of order 16 to a signal with an empty upper half band is poorly
    conditioned: on a bare amplitude-modulated tone the same distance was 2.7e-9)."""
    import composite_cases as CC
    wav = tmp_path / "exp" / "wav" / "test"
    wav.mkdir(parents=True)
    for i, n in enumerate((8000, 6001)):
        ref, est = CC.pair(i, n, 8000)
        s = 0.5 / np.abs(est).max()
        wavio.save(wav / f"{i:04d}.tgt0.wav", torch.from_numpy(ref * s)[None], 8000, bits=16)
        wavio.save(wav / f"{i:04d}.enh0.wav", torch.from_numpy(est * s)[None], 8000, bits=16)
    with pytest.raises(SystemExit, match="sample rate 8000, not 16000"):
        evaluate_covl.main([str(wav), str(wav), "--batch", "2"])
    out = evaluate_covl.main([str(wav), str(wav), "--resample", "--batch", "2"])
    got = json.load(open(out / "test_covl.json"))
    for i, n in enumerate((8000, 6001)):
        r16 = [metrics.resample(wavio.load(wav / f"{i:04d}.{k}0.wav")[0][0].numpy().astype(np.float64), 16000, 8000).astype(np.float32)
               for k in ("tgt", "enh")]
        assert len(r16[0]) == 2 * n
        want = metrics.composite(r16[0], r16[1], 16000)
        same = metrics.composite_batch(torch.from_numpy(r16[0]).cuda()[None, None], torch.from_numpy(r16[1]).cuda()[None, None], 16000)[0, 0]
        for j, k in enumerate(("llr", "wss", "segsnr")):
            print(f"file {i} {k}: |device - host| = {abs(got[str(i)][k][0] - want[k]):.2e}")
            assert got[str(i)][k][0] == float(same[j]), (i, k)  # the device measures saw the host-resampled samples, bit for bit
            assert abs(got[str(i)][k][0] - want[k]) <= 1e-9 * max(1.0, abs(want[k])), (i, k)
