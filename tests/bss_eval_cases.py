"""Inputs of the BSS-eval tests (tests/test_bss_eval_cpu.py, tests/test_bss_eval_gpu.py) and the explicit reference they are
held to: the least-squares form of the definition, written from it and not from the Toeplitz algebra of the code under test.

Signals: every reference is band-passed white noise under a slow amplitude modulation plus a white floor of 5 % (it bounds the
condition of the correlation matrix); every estimate is a mixture of the references (mostly its own) through a short FIR plus
white noise.  Seeded, float32, a function of the case alone."""
import numpy as np

PANEL = 64  # the Cholesky panel width of csrc/bss_eval.hip (kNB)

# (S, n, L).  The first eight are the issue's; then S L one below, at, one above and at two-plus-one times the panel width.
CASES = [(1, 300, 8), (2, 1000, 16), (3, 1500, 32), (2, 700, 33), (2, 4000, 64), (2, 40, 64), (2, 1, 4), (3, 257, 1),
         (3, 500, 21), (2, 600, 32), (1, 350, 64), (1, 400, 65), (3, 900, 43)]
assert {S * L for S, _, L in CASES} >= {PANEL - 1, PANEL, PANEL + 1, 2 * PANEL + 1}

COND_MAX = 1e7     # of R for every case whose R is not singular by construction
LIMIT_DB = 60.0    # values are compared where |value| < 60 dB
# dB: the largest |host form - explicit form| over CASES measured on the CPU (tests/test_bss_eval_cpu.py prints and gates it)
HOST_VS_EXPLICIT_MAX = 6.0e-13


def full_rank(S, n, L):
    """A = [A_0 ... A_{S-1}] has n + L - 1 rows and S L columns: with more columns than rows R = A^T A is singular whatever
    the signals are ((2, 40, 64): 128 columns, 103 rows; (2, 1, 4): 8 columns, 4 rows).  The diagonal blocks R_ii stay positive
    definite (L shifts of one non-zero row are independent), so SDR and the permutation are defined there; SIR and SAR are not
    (e_artif is zero up to rounding), and neither is a bound on cond(R)."""
    return S * L <= n + L - 1


def _bandpass(rng, n, lo, hi):
    """white noise of n samples limited to the band [lo, hi] (fractions of the Nyquist rate) by a windowed-sinc FIR"""
    m = np.arange(-24, 25)
    h = (hi * np.sinc(hi * m) - lo * np.sinc(lo * m)) * np.hamming(len(m))
    return np.convolve(rng.standard_normal(n + len(m) - 1), h, mode="valid")


def signals(S, n, L, seed=0):
    """-> (ref [S, n], est [S, n]) float32"""
    rng = np.random.default_rng([seed, S, n, L])
    t = np.arange(n)
    ref = np.zeros((S, n))
    for i in range(S):
        x = _bandpass(rng, n, 0.08 + 0.15 * i, 0.45 + 0.2 * i)
        x *= 1.0 + 0.7 * np.sin(2 * np.pi * t / (180.0 + 70 * i) + i)
        x /= np.sqrt(np.mean(x * x)) + 1e-30
        ref[i] = x + 0.05 * rng.standard_normal(n)
    est = np.zeros((S, n))
    for j in range(S):
        mix = sum((1.0 if i == j else 0.25) * ref[i] for i in range(S))
        h = np.array([0.9, 0.3, -0.15, 0.05][:max(1, min(4, L))])
        est[j] = np.convolve(mix, h)[:n] + 0.1 * rng.standard_normal(n)
    return ref.astype(np.float32), est.astype(np.float32)


def delay_matrix(r, L):
    """A_i: (n + L - 1) x L, column tau = r delayed by tau samples, zero-padded"""
    n = len(r)
    A = np.zeros((n + L - 1, L))
    for tau in range(L):
        A[tau:tau + n, tau] = r
    return A


def explicit(ref, est, L):
    """The definition in float64 by numpy.linalg.lstsq on the explicit A: s_target = P_i e_j, e_interf = P e_j - P_i e_j,
    e_artif = e_j - P e_j -> (SDR [S, S], SIR [S, S] indexed [reference i][estimate j], SAR [S]) in dB, unclamped."""
    ref, est = np.asarray(ref, np.float64), np.asarray(est, np.float64)
    S, n = ref.shape
    Ai = [delay_matrix(ref[i], L) for i in range(S)]
    A = np.concatenate(Ai, axis=1)
    sdr, sir, sar = np.zeros((S, S)), np.zeros((S, S)), np.zeros(S)
    sq = lambda v: np.float64(np.dot(v, v))
    with np.errstate(divide="ignore", invalid="ignore"):
        for j in range(S):
            e = np.concatenate([est[j], np.zeros(L - 1)])
            Pe = A @ np.linalg.lstsq(A, e, rcond=None)[0]
            sar[j] = 10 * np.log10(sq(Pe) / sq(e - Pe))
            for i in range(S):
                st = Ai[i] @ np.linalg.lstsq(Ai[i], e, rcond=None)[0]
                sdr[i, j] = 10 * np.log10(sq(st) / sq(e - st))
                sir[i, j] = 10 * np.log10(sq(st) / sq(Pe - st))
    return sdr, sir, sar


def cond_R(ref, L):
    """(cond of R, largest cond of a diagonal block R_ii), from the explicit A"""
    ref = np.asarray(ref, np.float64)
    Ai = [delay_matrix(r, L) for r in ref]
    A = np.concatenate(Ai, axis=1)
    return float(np.linalg.cond(A.T @ A)), max(float(np.linalg.cond(a.T @ a)) for a in Ai)


def cond_R_toeplitz(ref, L):
    """cond of R from its correlations (for filters too long for the explicit A): the ratio of its extreme eigenvalues"""
    from scipy.linalg import toeplitz
    ref = np.asarray(ref, np.float64)
    S, n = ref.shape
    xc = lambda x, y: np.array([np.dot(x[:n - l], y[l:]) if l < n else 0.0 for l in range(L)])
    R = np.block([[toeplitz(xc(ref[i], ref[k]), xc(ref[k], ref[i])) for k in range(S)] for i in range(S)])
    w = np.linalg.eigvalsh(R)
    return float(w[-1] / w[0]) if w[0] > 0 else float("inf")


def compared(S, n, L):
    """which tables a comparison covers for the case: all three, or SDR alone where R is singular by construction"""
    return ("sdr", "sir", "sar") if full_rank(S, n, L) else ("sdr",)


def max_diff(a, b):
    """largest |a - b| over the entries where both are finite and below LIMIT_DB in magnitude (0.0 without one)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    ok = np.isfinite(a) & np.isfinite(b) & (np.abs(a) < LIMIT_DB) & (np.abs(b) < LIMIT_DB)
    return float(np.max(np.abs(a - b)[ok])) if np.any(ok) else 0.0
