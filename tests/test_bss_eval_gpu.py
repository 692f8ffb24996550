"""Device BSS-eval SDR / SIR / SAR (csrc/bss_eval.hip: ops.bss_eval, metrics.bss_eval_sources / bss_eval_batch, evaluate
--bss-eval) against the float64 host form metrics.bss_eval_host, plus the batch / stream / permutation / refusal properties of
the C-ABI entry.

The bound on |device - host form| is 100 x the largest |host form - explicit least-squares form| measured on the CPU over the
same cases (tests/test_bss_eval_cpu.py: 6.0e-13 dB), where |value| < 60 dB; inf / NaN positions and the permutation are equal.
Both sides are float64 forms of one algebra whose error grows with cond(R) (<= 3.6e3 over the cases), so the two full-width
cases (L = 512) take the same bound times cond(R) / 3.6e3 where their R is worse conditioned than that.  Where R is singular by
construction (bss_eval_cases.full_rank) SDR and the permutation are compared, as on the CPU."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import bss_eval_cases as BC
from diffsep_amd import _lib, metrics, ops, wavio

pytestmark = pytest.mark.gpu
BOUND = 100 * BC.HOST_VS_EXPLICIT_MAX  # dB
COND_CASES = 3.6e3                  # the largest cond(R) of the full-rank cases (tests/test_bss_eval_cpu.py prints them)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _run(ref, est, L, **kw):
    """ops.bss_eval -> numpy (out [B,3,S], pairs [B,2,S,S], perm [B,S])"""
    return tuple(t.cpu().numpy() for t in ops.bss_eval(_dev(ref), _dev(est), L, **kw))


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else a.dtype)


def _same(a, b):
    return all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _compare(case, got, h, bound):
    """device tables against the host form's: values within bound where |value| < 60 dB, inf / NaN where it has them"""
    out, pairs, perm = got
    tabs = {"sdr": (pairs[0, 0], h["sdr_pairs"][0]), "sir": (pairs[0, 1], h["sir_pairs"][0])}
    sar_dev = np.full(len(perm[0]), np.nan)
    sar_dev[perm[0]] = out[0, 2]  # out's SAR is per reference i = SAR of estimate perm[i]
    tabs["sar"] = (sar_dev, h["sar_all"][0])
    for k in BC.compared(*case):
        d, v = tabs[k]
        print(f"{case} {k}: |device - host| {BC.max_diff(d, v):.2e} dB (bound {bound:.1e})")
        assert np.array_equal(np.isnan(d), np.isnan(v)) and np.array_equal(np.isposinf(d), np.isposinf(v)), (case, k, d, v)
        assert np.array_equal(np.isneginf(d), np.isneginf(v)), (case, k)
        assert BC.max_diff(d, v) <= bound, (case, k, d, v)
    assert np.array_equal(perm[0], h["perm"][0])
    i = np.arange(len(perm[0]))
    assert np.array_equal(_bits(out[0, 0]), _bits(pairs[0, 0][i, perm[0]])) and np.array_equal(_bits(out[0, 1]), _bits(pairs[0, 1][i, perm[0]]))


@pytest.mark.parametrize("case", BC.CASES, ids=str)
def test_device_matches_host_form(case):
    S, n, L = case
    ref, est = BC.signals(S, n, L)
    h = metrics.bss_eval_host(ref[None], est[None], L)
    _compare(case, _run(ref[None], est[None], L), h, BOUND)
    via = metrics.bss_eval_sources(_dev(ref[None]), _dev(est[None]), filter_length=L)
    hs = metrics.bss_eval_sources(ref[None], est[None], filter_length=L, on="host")
    assert np.array_equal(via[3], hs[3]) and via[3].dtype == np.int64 and all(v.shape == (1, S) for v in via)
    if BC.full_rank(*case):
        assert all(BC.max_diff(a, b) <= BOUND and np.array_equal(np.isfinite(a), np.isfinite(b)) for a, b in zip(via[:3], hs[:3]))


@pytest.mark.parametrize("case", [(2, 8000, 512), (3, 4000, 512)], ids=str)
def test_full_width_filter(case):
    S, n, L = case
    ref, est = BC.signals(S, n, L)
    h = metrics.bss_eval_host(ref[None], est[None], L)
    cond = BC.cond_R_toeplitz(ref, L)
    bound = BOUND * max(1.0, cond / COND_CASES)
    print(f"{case}: cond(R) {cond:.2e}")
    assert BC.full_rank(*case) and cond <= BC.COND_MAX
    _compare(case, _run(ref[None], est[None], L), h, bound)


def test_ragged_batch_equals_single_rows_bit_for_bit_on_any_stream():
    S, L, lens = 2, 32, [1500, 257, 1]
    rows = [BC.signals(S, n, L) for n in lens]
    alone = [_run(r[None], e[None], L) for r, e in rows]  # B = 1, T = n
    for T in (1501, 2048):
        for fill in (0.0, np.nan):  # samples beyond a row's length are never read
            ref, est = np.full((3, S, T), fill, np.float32), np.full((3, S, T), fill, np.float32)
            for b, (n, (r, e)) in enumerate(zip(lens, rows)):
                ref[b, :, :n], est[b, :, :n] = r, e
            got = _run(ref, est, L, lengths=lens)
            for b in range(3):
                assert _same([g[b:b + 1] for g in got], alone[b]), (T, fill, b)
    dref, dest = _dev(ref), _dev(est)
    first = ops.bss_eval(dref, dest, L, lengths=lens)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        second = ops.bss_eval(dref, dest, L, lengths=lens)
    torch.cuda.synchronize()
    assert _same([t.cpu().numpy() for t in first], [t.cpu().numpy() for t in second]) and _same([t.cpu().numpy() for t in first], got)
    # the wrapper splits a batch whose workspace would pass its cap: the rows do not change
    cap = ops.BSS_EVAL_WORKSPACE_CAP
    try:
        ops.BSS_EVAL_WORKSPACE_CAP = ops.bss_eval_workspace_bytes(1, S, 2048, L) * 2
        split = ops.bss_eval(dref, dest, L, lengths=lens)
    finally:
        ops.BSS_EVAL_WORKSPACE_CAP = cap
    assert _same([t.cpu().numpy() for t in split], got)


def test_given_permutation_equals_the_searched_one_given_back():
    S, n, L = 3, 900, 43
    ref, est = BC.signals(S, n, L)
    est = est[[2, 0, 1]]
    searched = _run(ref[None], est[None], L, clamp_db=100.0)
    assert list(searched[2][0]) == [1, 2, 0]
    given = _run(ref[None], est[None], L, clamp_db=100.0, perm=searched[2])
    assert _same(searched, given)
    other = _run(ref[None], est[None], L, clamp_db=100.0, perm=[[0, 1, 2]])
    assert np.array_equal(_bits(other[1]), _bits(searched[1])) and list(other[2][0]) == [0, 1, 2]  # same tables, another row
    assert np.array_equal(_bits(other[0][0, 0]), _bits(np.diag(searched[1][0, 0])))


def test_rules_for_undefined_values_on_the_device():
    S, n, L = 2, 500, 8
    ref, est = BC.signals(S, n, L)
    ref2, est2 = np.stack([ref, ref]), np.stack([est, est])
    ref2[1, 1] = 0.0  # a silent reference in the second utterance
    h = metrics.bss_eval_host(ref2, est2, L)
    out, pairs, perm = _run(ref2, est2, L)
    assert np.array_equal(perm, h["perm"])
    assert np.all(np.isfinite(out[0])) and np.all(np.isfinite(pairs[0]))
    assert np.all(np.isnan(pairs[1, 0, 1])) and np.all(np.isfinite(pairs[1, 0, 0])) and np.all(np.isnan(pairs[1, 1]))
    assert np.isfinite(out[1, 0, 0]) and np.isnan(out[1, 0, 1]) and np.all(np.isnan(out[1, 1:]))
    assert BC.max_diff(pairs[:, 0], h["sdr_pairs"]) <= BOUND and BC.max_diff(out[0], np.stack([h["sdr"][0], h["sir"][0], h["sar"][0]])) <= BOUND
    # one source: SIR is +inf exactly, the clamp brings it to the clamp
    r1, e1 = BC.signals(1, 300, 8)
    assert _run(r1[None], e1[None], 8)[0][0, 1, 0] == np.inf and _run(r1[None], e1[None], 8, clamp_db=30.0)[0][0, 1, 0] == 30.0
    # a delayed copy: beyond 80 dB (or the clamp) where SI-SDR is below 0 dB, and the permutation comes out swapped
    rng = np.random.default_rng(11)
    w = rng.standard_normal((2, 600)).astype(np.float32)
    w[:, -16:] = 0
    e = np.stack([np.concatenate([np.zeros(7, np.float32), w[1, :-7]]), w[0] + 0.1 * rng.standard_normal(600).astype(np.float32)])
    for clamp in (0.0, 100.0):
        o, p, pm = _run(w[None], e[None], 16, clamp_db=clamp)
        assert p[0, 0, 1, 0] > 80.0 and (clamp == 0.0 or p[0, 0, 1, 0] <= clamp) and list(pm[0]) == [1, 0]
    assert metrics.si_bss_eval_sources(_dev(w[None]), _dev(e[None]))[0][0, 1] < 0.0
    # scaling the estimates by 4 changes no bit of a finite output
    a, b = _run(ref[None], est[None], L), _run(ref[None], 4.0 * est[None], L)
    assert _same(a, b)


def test_refusals_write_nothing_and_leave_the_stream_usable():
    B, S, T, L = 1, 2, 700, 33
    ref, est = BC.signals(S, T, L)
    x, y = _dev(ref[None]), _dev(est[None])
    l = _lib.lib()
    out = torch.full((B, 3, S), -7.0, dtype=torch.float64, device="cuda")
    pairs = torch.full((B, 2, S, S), -7.0, dtype=torch.float64, device="cuda")
    pm = torch.full((B, S), -7, dtype=torch.int32, device="cuda")
    need = ops.bss_eval_workspace_bytes(B, S, T, L)
    ws = torch.empty(need + 8, dtype=torch.uint8, device="cuda")
    P = lambda t: C.c_void_p(t.data_ptr())

    def call(ref_=P(x), out_=P(out), S_=S, L_=L, clamp=0.0, w=P(ws), wb=need):
        return l.diffsep_bss_eval(ref_, P(y), out_, P(pairs), P(pm), B, S_, T, None, None, L_, clamp, w, wb, None)

    for kw, word in [(dict(ref_=None), b"ref is null"), (dict(out_=None), b"out is null"), (dict(S_=4), b"S outside"),
                     (dict(L_=1025), b"L outside"), (dict(clamp=-1.0), b"clamp_db"), (dict(w=None), b"workspace is null"),
                     (dict(wb=need - 1), b"workspace_bytes"), (dict(w=C.c_void_p(ws.data_ptr() + 4)), b"8-byte aligned")]:
        assert call(**kw) != 0 and word in l.diffsep_last_error(), kw
    with pytest.raises(_lib.DiffsepError, match="L outside"):
        ops.bss_eval(x, y, 2000)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((pairs == -7.0).all()) and bool((pm == -7).all())
    assert call() == 0
    torch.cuda.synchronize()
    good = ops.bss_eval(x, y, L)
    assert _same([out.cpu().numpy(), pairs.cpu().numpy(), pm.cpu().numpy()], [t.cpu().numpy() for t in good])


def test_evaluate_bss_eval_flag(tmp_path, monkeypatch):
    from diffsep_amd import evaluate as ev
    seen = []
    real = metrics.bss_eval_batch

    def spy(ref, est, filter_length=512, clamp_db=100.0, lengths=None, perm=None):
        got = real(ref, est, filter_length, clamp_db=clamp_db, lengths=lengths, perm=perm)
        seen.append((ref.clone(), est.clone(), filter_length, clamp_db, list(lengths), [list(p) for p in perm], got))
        return got

    monkeypatch.setattr(metrics, "bss_eval_batch", spy)
    recs = {}
    for name, extra in (("plain", []), ("bss", ["--bss-eval", "--bss-filter-length", "32"])):
        out = tmp_path / name
        ev.main(["--synthetic", "2", "--samples", "4000", "--synthetic-weights", "16", "-N", "2", "--dtype", "f32", "--no-stoi",
                 "--flat-output", "-o", str(out)] + extra)
        recs[name] = (json.load(open(out / "test.json")), json.load(open(out / "test_summary.json")))
    (plain, ps), (bss, bs) = recs["plain"], recs["bss"]
    today = {"batch_idx", "si_sdr", "si_sir", "si_sar", "perm", "pesq", "stoi", "nfe", "runtime", "len_s"}
    assert len(plain) == len(bss) == 2 and len(seen) >= 1
    for p, c in zip(plain, bss):
        assert set(p) == today and set(c) == today | {"sdr", "sir", "sar"}
        assert p["si_sdr"] == c["si_sdr"] and p["perm"] == c["perm"]
    assert "sdr" not in ps and "bss_filter_length" not in ps and bs["bss_filter_length"] == 32
    assert set(bs) - set(ps) == {"sdr", "sir", "sar", "bss_filter_length"}
    for k in ("sdr", "sir", "sar"):
        assert abs(bs[k] - np.mean([np.mean(c[k]) for c in bss])) <= 1e-12 * max(1.0, abs(bs[k]))
    # the records are what the device call on the scored tensors gave, under the records' permutations, and that is what
    # metrics.bss_eval_sources gives for the same tensors (bit for bit: a row does not depend on its batch)
    k = 0
    for ref, est, L, clamp, lens, perm, got in seen:
        assert L == 32 and clamp == 100.0
        sdr, sir, sar, pm = metrics.bss_eval_sources(ref, est, filter_length=32, clamp_db=100.0, lengths=lens, perm=perm)
        for b in range(ref.shape[0]):
            c = bss[k]
            k += 1
            assert perm[b] == c["perm"] and list(pm[b]) == c["perm"]
            assert c["sdr"] == list(got[b, 0]) == list(sdr[b]) and c["sir"] == list(got[b, 1]) == list(sir[b])
            assert c["sar"] == list(got[b, 2]) == list(sar[b]) and all(np.isfinite(c["sdr"]))
    assert k == 2
    # ... and, within what one fp32 rounding of the common peak scaling of the saved files can move them, of the saved wavs
    # (estimates saved in the targets' order): a relative perturbation u = 2^-24 of every sample moves a projection energy by
    # at most about 2 sqrt(cond(R)) u relatively, references and estimates both, and a value v dB by (10 / ln 10) times the
    # relative change of its numerator and of its denominator; the change is relative to the larger of the two energies, so
    # the smaller one moves 10^(|v| / 10) times more
    for i, c in enumerate(bss):
        tgt = np.stack([wavio.load(out / "wav" / "test" / f"{i:03d}_tgt{s}.wav")[0][0].numpy() for s in range(2)])
        enh = np.stack([wavio.load(out / "wav" / "test" / f"{i:03d}_enh{s}.wav")[0][0].numpy() for s in range(2)])
        cond = BC.cond_R(tgt, 32)[0]
        sdr, sir, sar, _ = metrics.bss_eval_sources(_dev(tgt[None]), _dev(enh[None]), filter_length=32, clamp_db=100.0, perm=[[0, 1]])
        for name, v in (("sdr", sdr[0]), ("sir", sir[0]), ("sar", sar[0])):
            tol = (10 / np.log(10)) * 4 * np.sqrt(cond) * 2.0 ** -24 * (1 + 10 ** (np.abs(v) / 10))
            print(f"utt {i} {name}: record {c[name]} saved wavs {v} (cond {cond:.2e}, tol {tol})")
            assert np.all(np.abs(np.asarray(c[name]) - v) <= tol), (i, name)
