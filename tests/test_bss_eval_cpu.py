"""BSS-eval SDR / SIR / SAR without a GPU: the float64 host form (diffsep_amd.metrics.bss_eval_host, the Toeplitz algebra of
csrc/bss_eval.hip with scipy's Cholesky) against the explicit least-squares form of the definition (tests/bss_eval_cases.py),
the one-tap case against the SI forms, the rules for what the formulas leave undefined, and the host side of the C-ABI entry
(workspace formula, refusals before any device call, the evaluate flags).

Measured here (float64, OpenBLAS), the largest |host form - explicit form| over every case of bss_eval_cases.CASES, entries with
|value| < 60 dB:  6.0e-13 dB  (SDR 4.3e-13, SIR 1.3e-13, SAR 6.0e-13; cond(R) <= 3.6e3).  The gate is that maximum with a
factor of 100 for other BLAS builds, and tests/test_bss_eval_gpu.py holds the device to the host form at the same 100 x.
Two of the issue's cases, (2, 40, 64) and (2, 1, 4), have more columns in A than rows: R is singular whatever the signals are,
so cond(R) is unbounded and SIR / SAR are undefined there (bss_eval_cases.full_rank); the diagonal blocks are well conditioned
and SDR and the permutation are compared."""
import ctypes as C

import numpy as np
import pytest

import bss_eval_cases as BC
from diffsep_amd import _lib, evaluate, metrics

HOST_VS_EXPLICIT_MAX = BC.HOST_VS_EXPLICIT_MAX  # 6.0e-13 dB, measured (module docstring)
GATE = 100 * HOST_VS_EXPLICIT_MAX


@pytest.fixture(scope="module")
def host():
    """bss_eval_host of every case, once: (ref, est, result)"""
    out = {}
    for S, n, L in BC.CASES:
        ref, est = BC.signals(S, n, L)
        out[(S, n, L)] = (ref, est, metrics.bss_eval_host(ref[None], est[None], L))
    return out


def test_host_form_matches_the_explicit_least_squares_form(host):
    worst = 0.0
    for case in BC.CASES:
        S, n, L = case
        ref, est, h = host[case]
        cond, cond_diag = BC.cond_R(ref, L)
        assert cond_diag <= BC.COND_MAX and (cond <= BC.COND_MAX or not BC.full_rank(S, n, L)), (case, cond, cond_diag)
        sdr, sir, sar = BC.explicit(ref, est, L)
        d = {"sdr": BC.max_diff(h["sdr_pairs"][0], sdr), "sir": BC.max_diff(h["sir_pairs"][0], sir),
             "sar": BC.max_diff(h["sar_all"][0], sar)}
        print(f"{case}: cond(R) {cond:.2e}, |host - explicit| dB sdr {d['sdr']:.2e} sir {d['sir']:.2e} sar {d['sar']:.2e}")
        for k in BC.compared(S, n, L):
            worst = max(worst, d[k])
            assert d[k] <= GATE, (case, k, d[k])
        if BC.full_rank(S, n, L):  # every value is finite and compared, none slipped through max_diff's filter
            assert all(np.all(np.abs(v) < BC.LIMIT_DB) for v in (sdr, sar)) and (S == 1 or np.all(np.abs(sir) < BC.LIMIT_DB))
            assert np.all(np.isfinite(h["sdr_pairs"])) and np.all(np.isfinite(h["sar_all"]))
        # the permutation: the largest mean SDR of the explicit table
        assert list(h["perm"][0]) == list(range(S))
        assert np.array_equal(h["sdr"][0], np.diag(h["sdr_pairs"][0])) and np.array_equal(h["sar"][0], h["sar_all"][0], equal_nan=True)
    print(f"largest |host - explicit| over the cases: {worst:.2e} dB (recorded: {HOST_VS_EXPLICIT_MAX:.1e})")


@pytest.mark.parametrize("S,n", [(3, 257), (2, 1000), (1, 300)])
def test_one_tap_is_the_scale_invariant_form(S, n):
    ref, est = BC.signals(S, n, 1)
    ref[...] = ref[::-1].copy()  # (the estimates were mixed for the other order: the permutation found is not the identity)
    r, e = ref.astype(np.float64), est.astype(np.float64)
    G = np.stack([r @ r.T, r @ e.T, e @ e.T])[None]
    sdr, sir, sar, perm = metrics.si_bss_from_gram(G, clamp_db=100.0)
    got = metrics.bss_eval_sources(ref[None], est[None], filter_length=1, clamp_db=100.0, on="host")
    assert S == 1 or list(perm[0]) != list(range(S))
    assert np.array_equal(got[3], perm)
    for name, a, b in (("sdr", got[0], sdr), ("sir", got[1], sir), ("sar", got[2], sar)):
        print(f"S={S} n={n} {name}: |one tap - SI form| {np.max(np.abs(a - b)):.2e} dB")
        assert np.max(np.abs(a - b)) <= GATE, (name, a, b)
    if S == 1:
        assert got[1][0, 0] == 100.0


def _white(S, n, seed, tail=16):
    x = np.random.default_rng(seed).standard_normal((S, n)).astype(np.float32)
    x[:, n - tail:] = 0  # a delayed copy stays inside the n samples
    return x


def test_a_delayed_copy_is_a_perfect_projection_and_swaps_the_permutation():
    n, L, d = 600, 16, 7
    ref = _white(2, n, 11)
    est = np.zeros_like(ref)
    est[0, d:] = ref[1, :n - d]
    est[1] = ref[0] + 0.1 * _white(1, n, 12)[0]
    for clamp in (None, 100.0):
        h = metrics.bss_eval_host(ref[None], est[None], L, clamp_db=clamp)
        v = h["sdr_pairs"][0, 1, 0]
        assert v > 80.0 and (clamp is None or v <= clamp), v
        assert list(h["perm"][0]) == [1, 0] and h["sdr"][0, 1] == v
    r, e = ref.astype(np.float64), est.astype(np.float64)
    si = metrics.si_bss_from_gram(np.stack([r @ r.T, r @ e.T, e @ e.T])[None], perm=[[1, 0]])[0]
    assert si[0, 1] < 0.0, si  # one gain cannot undo a delay of white noise


def test_a_silent_reference_is_nan_where_its_factorisation_is_used_and_nowhere_else():
    S, n, L = 2, 500, 8
    ref, est = BC.signals(S, n, L)
    ref2, est2 = np.stack([ref, ref]), np.stack([est, est])
    ref2[1, 1] = 0.0
    h = metrics.bss_eval_host(ref2, est2, L)
    one = metrics.bss_eval_host(ref[None], est[None], L)
    for k in ("sdr", "sir", "sar", "sdr_pairs", "sir_pairs", "sar_all", "perm"):
        assert np.array_equal(h[k][0], one[k][0]) and np.all(np.isfinite(h[k][0])), k  # the other utterance is untouched
    assert np.all(np.isnan(h["sdr_pairs"][1, 1])) and np.all(np.isfinite(h["sdr_pairs"][1, 0]))
    assert np.all(np.isnan(h["sir_pairs"][1])) and np.all(np.isnan(h["sar_all"][1]))
    # the search counts NaN as -inf: both candidates sum to -inf, the first (the identity) stays
    assert list(h["perm"][1]) == [0, 1]
    assert np.isfinite(h["sdr"][1, 0]) and np.isnan(h["sdr"][1, 1]) and np.all(np.isnan(h["sir"][1])) and np.all(np.isnan(h["sar"][1]))


def test_one_source_has_infinite_sir_exactly():
    for case in [c for c in BC.CASES if c[0] == 1]:
        ref, est = BC.signals(*case)
        h = metrics.bss_eval_host(ref[None], est[None], case[2])
        assert h["sir"][0, 0] == np.inf and np.isfinite(h["sdr"][0, 0]) and h["sdr"][0, 0] == h["sar"][0, 0]
        assert metrics.bss_eval_host(ref[None], est[None], case[2], clamp_db=30.0)["sir"][0, 0] == 30.0


def test_scaling_the_estimates_by_four_changes_no_bit(host):
    for case in BC.CASES:
        ref, est, h = host[case]
        h4 = metrics.bss_eval_host(ref[None], 4.0 * est[None], case[2])
        for k in ("sdr_pairs", "sir_pairs", "sar_all", "perm"):
            fin = np.isfinite(h[k])
            assert np.array_equal(np.isfinite(h4[k]), fin) and np.array_equal(h4[k][fin], h[k][fin]), (case, k)


def _formula(B, S, T, L):
    up = lambda v: (v + 255) // 256 * 256
    J, Cn = 2 * S * S + S, -(-T // 2048)
    return up(8 * B * J * Cn * L) + up(8 * B * J * L) + up(8 * B * ((S * L + S) * S * L + (S - 1) * (L + S) * L)) + up(4 * B * S)


def test_workspace_bytes_accepts_and_refuses():
    l = _lib.lib()
    f = l.diffsep_bss_eval_workspace_bytes
    for shape in [(1, 1, 1, 1), (16, 2, 32000, 512), (16, 3, 32000, 512), (1, 3, 2 ** 31 - 1, 1024), (21845, 3, 5, 1), (3, 2, 2049, 33)]:
        assert f(*shape) == _formula(*shape), shape
    assert f(1, 3, 4000, 512) > 23_000_000  # (the header's figure for one utterance)
    for shape, word in [((0, 2, 100, 8), b"B"), ((21846, 3, 100, 8), b"B"), ((1, 0, 100, 8), b"S"), ((1, 4, 100, 8), b"S"),
                        ((1, 2, 0, 8), b"T"), ((1, 2, 2 ** 31, 8), b"T"), ((1, 2, 100, 0), b"L"), ((1, 2, 100, 1025), b"L")]:
        assert f(*shape) == -1 and word + b" outside" in l.diffsep_last_error(), shape


def test_refusals_come_before_any_device_call():
    l = _lib.lib()
    B, S, T, L = 1, 2, 100, 8
    need = l.diffsep_bss_eval_workspace_bytes(B, S, T, L)
    x = np.zeros((B, S, T), np.float32)
    out = np.full((B, 3, S), -7.0)
    ws = np.zeros(need + 16, np.uint8)
    P = lambda a: C.c_void_p(a.ctypes.data)
    base = ws.ctypes.data + (-ws.ctypes.data) % 8

    def call(ref=P(x), est=P(x), o=P(out), S_=S, L_=L, clamp=0.0, w=C.c_void_p(base), wb=need):
        return l.diffsep_bss_eval(ref, est, o, None, None, B, S_, T, None, None, L_, clamp, w, wb, None)

    for kw, word in [(dict(ref=None), b"ref is null"), (dict(est=None), b"est is null"), (dict(o=None), b"out is null"),
                     (dict(w=None), b"workspace is null"), (dict(wb=need - 1), b"workspace_bytes"), (dict(S_=4), b"S outside"),
                     (dict(L_=0), b"L outside"), (dict(L_=1025), b"L outside"), (dict(clamp=-1.0), b"clamp_db"),
                     (dict(w=C.c_void_p(base + 4)), b"8-byte aligned")]:
        assert call(**kw) != 0 and word in l.diffsep_last_error(), kw
    assert np.all(out == -7.0)


def test_evaluate_flags():
    ap = evaluate.build_parser()
    a = ap.parse_args(["--synthetic", "2"])
    assert a.bss_eval is False and a.bss_filter_length == 512
    a = ap.parse_args(["--synthetic", "2", "--bss-eval"])
    assert a.bss_eval is True and a.bss_filter_length == 512
    a = ap.parse_args(["--synthetic", "2", "--bss-eval", "--bss-filter-length", "32"])
    assert a.bss_eval is True and a.bss_filter_length == 32
    with pytest.raises(SystemExit):
        evaluate.main(["--synthetic", "2", "--synthetic-weights", "16", "--bss-eval", "--bss-filter-length", "2000"])
