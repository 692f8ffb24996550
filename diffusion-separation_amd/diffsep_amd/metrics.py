"""Separation metrics from Gram matrices (the waveform reductions run in the HIP `gram` kernel; the S x S algebra
below is host-side bookkeeping on a handful of float64 numbers per utterance).

Definitions follow fast_bss_eval.si_bss_eval_sources(ref, est, zero_mean=False, compute_permutation=True) as called by
the reference (evaluate.py:105-111): for estimate j scored against reference i
    s_target = <est_j, ref_i>/<ref_i, ref_i> ref_i
    e_proj   = orthogonal projection of est_j on span{ref_1..ref_S};  e_interf = e_proj - s_target;  e_artif = est_j - e_proj
    SI-SDR = |s_target|^2 / |est_j - s_target|^2,  SI-SIR = |s_target|^2 / |e_interf|^2,  SI-SAR = |e_proj|^2 / |e_artif|^2
and the permutation maximising the mean SI-SDR is returned.  fast_bss_eval itself is not installed here, so SIR/SAR are
pinned by these definitions (tests compare against a float64 time-domain restatement), SI-SDR also by closed-form cases.
"""
import itertools

import numpy as np
import torch

from . import ops


def _db(num, den):
    return 10.0 * np.log10(np.maximum(num, 1e-300) / np.maximum(den, 1e-300))


def si_bss_eval_sources(ref, est, clamp_db=100.0):
    """ref, est [B,S,T] device tensors -> (si_sdr, si_sir, si_sar [B,S] numpy, perm [B,S] int) with est[:, perm] aligned
    to ref."""
    return si_bss_from_gram(gram_to_host(ops.gram(ref.float(), est.float())), clamp_db=clamp_db)


def gram_to_host(Gd):
    """float64 Gram sums on the device -> numpy, through pinned memory on the CURRENT stream only (a pageable copy would
    stall every other stream's work)"""
    Gh = torch.empty(Gd.shape, dtype=Gd.dtype, pin_memory=True)
    Gh.copy_(Gd, non_blocking=True)
    torch.cuda.current_stream().synchronize()
    return Gh.numpy()


def si_bss_from_gram(G, clamp_db=100.0, perm=None):
    """The host algebra of si_bss_eval_sources on its own (pure numpy): G [B,3,S,S] float64 = {ref ref^T, ref est^T,
    est est^T} per utterance (diffsep_gram, or a row of the sampler's trace) -> (si_sdr, si_sir, si_sar [B,S], perm [B,S]).
    perm None: the permutation maximising the mean SI-SDR, as there; perm [B,S] given: the values of that fixed assignment
    (reference i against estimate perm[b][i]) — what lets a curve over the reverse steps follow one source."""
    G = np.asarray(G, dtype=np.float64)
    B, _, S, _ = G.shape
    sdr = np.zeros((B, S, S)); sir = np.zeros((B, S, S)); sar = np.zeros((B, S, S))
    for b in range(B):
        Grr, Gre, Gee = G[b, 0], G[b, 1], G[b, 2]
        for j in range(S):  # estimate j
            c = np.linalg.lstsq(Grr, Gre[:, j], rcond=None)[0]      # projection coefficients on all references
            proj2 = float(c @ Grr @ c)
            for i in range(S):  # reference i
                a = Gre[i, j] / max(Grr[i, i], 1e-300)
                tgt2 = a * a * Grr[i, i]
                sdr[b, i, j] = _db(tgt2, Gee[j, j] - 2 * a * Gre[i, j] + tgt2)
                interf2 = proj2 - 2 * a * float(c @ Grr[:, i]) + tgt2
                sir[b, i, j] = _db(tgt2, interf2)
                sar[b, i, j] = _db(proj2, Gee[j, j] - proj2)
    for m in (sdr, sir, sar):
        np.clip(m, -clamp_db, clamp_db, out=m)
    perms = list(itertools.permutations(range(S)))
    out = [np.zeros((B, S)) for _ in range(3)]
    best = np.zeros((B, S), dtype=np.int64)
    for b in range(B):
        if perm is None:
            scores = [np.mean([sdr[b, i, p[i]] for i in range(S)]) for p in perms]
            p = perms[int(np.argmax(scores))]
        else:
            p = tuple(int(v) for v in perm[b])
        best[b] = p
        for i in range(S):
            out[0][b, i], out[1][b, i], out[2][b, i] = sdr[b, i, p[i]], sir[b, i, p[i]], sar[b, i, p[i]]
    return out[0], out[1], out[2], best


# ---------------------------------------------------------------------------------------------------------------- BSS-eval
# SDR / SIR / SAR with a time-invariant distortion filter of L taps: mir_eval.separation.bss_eval_sources, and
# fast_bss_eval.bss_eval_sources(ref, est, filter_length=512) of the package the reference imports for the SI forms
# (evaluate.py:103-132).  Where SI-SDR allows the estimate one gain, SDR allows it an L-tap FIR.  With A_i the (n + L - 1) x L
# matrix whose column tau is reference i delayed by tau, A = [A_0 ... A_{S-1}], P_i and P the orthogonal projections onto
# their column spans:  s_target = P_i e_j,  e_interf = P e_j - P_i e_j,  e_artif = e_j - P e_j.  From correlations:
#   R = A^T A (block Toeplitz, S L x S L),  b_j = A^T e_j,  E_j = |e_j|^2,  q_ij = b_ij^T R_ii^-1 b_ij,  Q_j = b_j^T R^-1 b_j
#   SDR[i][j] = 10 log10(q_ij / (E_j - q_ij)),  SIR[i][j] = 10 log10(q_ij / (Q_j - q_ij)),  SAR[j] = 10 log10(Q_j / (E_j - Q_j))
# A denominator <= 0: +inf.  A non-positive Cholesky pivot (a silent reference): NaN for what depends on that factorisation
# (R_ii: row i of SDR and SIR; R: every SIR and SAR).  Neither package is installed here: parity with them is unpinned, and
# the explicit least-squares form of the definition above (tests/bss_eval_cases.py) stands in for them.
def _xcorr(x, y, L):
    """X(x, y, l) = sum_m x[m] y[m + l], l = 0 .. L - 1 (direct sums in float64; lags beyond the length are zero)"""
    n = len(x)
    return np.array([np.dot(x[:n - l], y[l:]) if l < n else 0.0 for l in range(L)])


def _bss_quad(R, rhs):
    """(y = chol(R)^-1 rhs [N, S], True), or (None, False) for a non-positive pivot"""
    import scipy.linalg
    if not np.all(np.isfinite(R)):
        return None, False
    try:
        c = scipy.linalg.cho_factor(R, lower=True, check_finite=False)[0]
    except np.linalg.LinAlgError:
        return None, False
    return scipy.linalg.solve_triangular(c, rhs, lower=True, check_finite=False), True


def _bss_db(num, den, clamp_db):
    with np.errstate(divide="ignore", invalid="ignore"):
        v = np.inf if den <= 0.0 else 10.0 * np.log10(num / den)
    if clamp_db and v == v:
        v = min(max(v, -clamp_db), clamp_db)
    return float(v)


def bss_eval_host(ref, est, filter_length=512, clamp_db=None, lengths=None, perm=None):
    """The float64 numpy / scipy form of diffsep_bss_eval (same Toeplitz algebra, scipy.linalg.cho_factor): ref, est [B,S,T]
    arrays -> dict(sdr, sir, sar [B,S], perm [B,S] int64, sdr_pairs, sir_pairs [B,S,S] indexed [reference][estimate],
    sar_all [B,S] per estimate).  perm None: the permutation of largest summed clamped SDR (NaN as -inf), the earliest of
    itertools.permutations on a tie."""
    import scipy.linalg
    ref, est = np.asarray(ref, dtype=np.float32), np.asarray(est, dtype=np.float32)
    if ref.shape != est.shape or ref.ndim != 3:
        raise ValueError("bss_eval: ref and est must be [B,S,T] arrays of one shape")
    B, S, T = ref.shape
    L, clamp = int(filter_length), float(clamp_db or 0.0)
    if not (1 <= S <= 3 and 1 <= L <= 1024):
        raise ValueError("bss_eval: S in 1..3 and filter_length in 1..1024")
    res = {"sdr": np.zeros((B, S)), "sir": np.zeros((B, S)), "sar": np.zeros((B, S)), "perm": np.zeros((B, S), dtype=np.int64),
           "sdr_pairs": np.zeros((B, S, S)), "sir_pairs": np.zeros((B, S, S)), "sar_all": np.zeros((B, S))}
    perms = list(itertools.permutations(range(S)))
    for b in range(B):
        n = T if lengths is None else min(max(int(lengths[b]), 0), T)
        r, e = ref[b, :, :n].astype(np.float64), est[b, :, :n].astype(np.float64)
        G = [[_xcorr(r[i], r[k], L) for k in range(S)] for i in range(S)]
        R = np.block([[scipy.linalg.toeplitz(G[i][k], G[k][i]) for k in range(S)] for i in range(S)])
        rhs = np.stack([np.concatenate([_xcorr(r[i], e[j], L) for i in range(S)]) for j in range(S)], axis=1)  # [S L, S]
        E = [float(np.dot(e[j], e[j])) for j in range(S)]
        y, ok = _bss_quad(R, rhs)
        q, okq = np.zeros((S, S)), [False] * S
        for i in range(S):
            if i == 0 and ok:  # chol(R_00) is the leading block of chol(R): the first L terms of the same sum
                yi, okq[i] = y[:L], True
            else:
                yi, okq[i] = _bss_quad(R[i * L:(i + 1) * L, i * L:(i + 1) * L], rhs[i * L:(i + 1) * L])
            if okq[i]:
                q[i] = [float(np.dot(yi[:, j], yi[:, j])) for j in range(S)]
        Q = [float(np.dot(y[:, j], y[:, j])) if ok else np.nan for j in range(S)]
        sdr, sir = res["sdr_pairs"][b], res["sir_pairs"][b]
        for j in range(S):
            res["sar_all"][b, j] = _bss_db(Q[j], E[j] - Q[j], clamp) if ok else np.nan
            for i in range(S):
                sdr[i, j] = _bss_db(q[i, j], E[j] - q[i, j], clamp) if okq[i] else np.nan
                sir[i, j] = _bss_db(q[i, j], Q[j] - q[i, j], clamp) if okq[i] and ok else np.nan
        if perm is None:
            cost = np.where(np.isnan(sdr), -np.inf, sdr)
            best, bestv = 0, 0.0
            for k, p in enumerate(perms):  # perm_search.h: sums from 0.0 with i ascending, strict >
                v = 0.0
                with np.errstate(invalid="ignore"):
                    for i in range(S):
                        v = v + cost[i, p[i]]
                if k == 0 or v > bestv:
                    best, bestv = k, v
            p = perms[best]
        else:
            p = tuple(min(max(int(v), 0), S - 1) for v in perm[b])
        res["perm"][b] = p
        for i in range(S):
            res["sdr"][b, i], res["sir"][b, i], res["sar"][b, i] = sdr[i, p[i]], sir[i, p[i]], res["sar_all"][b, p[i]]
    return res


def _to_host(d):
    h = torch.empty(d.shape, dtype=d.dtype, pin_memory=True)
    h.copy_(d, non_blocking=True)
    return h


def bss_eval_sources(ref, est, filter_length=512, clamp_db=None, lengths=None, perm=None, on="device"):
    """BSS-eval SDR / SIR / SAR with a filter_length-tap distortion filter: ref, est [B,S,T] -> (sdr, sir, sar [B,S] float64
    numpy, perm [B,S] int64) with est[:, perm] aligned to ref, shaped like si_bss_eval_sources.  clamp_db None / 0: no clamp.
    on="device": device tensors through diffsep_bss_eval (ops.bss_eval), one pinned readback on the current stream;
    on="host": bss_eval_host on arrays or host tensors (no GPU needed)."""
    if on == "host":
        as_np = lambda v: v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
        r = bss_eval_host(as_np(ref), as_np(est), filter_length, clamp_db, None if lengths is None else as_np(lengths),
                          None if perm is None else as_np(perm))
        return r["sdr"], r["sir"], r["sar"], r["perm"]
    if on != "device":
        raise ValueError("bss_eval_sources: on must be 'device' or 'host'")
    out, _, pout = ops.bss_eval(ref, est, filter_length, float(clamp_db or 0.0), lengths=lengths, perm=perm)
    oh, ph = _to_host(out), _to_host(pout)
    torch.cuda.current_stream().synchronize()
    o = oh.numpy().copy()
    return o[:, 0], o[:, 1], o[:, 2], ph.numpy().astype(np.int64)


def bss_eval_batch(ref, est, filter_length=512, clamp_db=100.0, lengths=None, perm=None):
    """bss_eval_sources on the device for evaluate: ref, est [B,S,T] device tensors -> [B,3,S] float64 numpy array {sdr, sir,
    sar} per source; estimate row perm[b][i] against reference row i over the first lengths[b] (default T) samples.  One
    pinned, non-blocking readback of 3 B S numbers on the current stream."""
    h = _to_host(ops.bss_eval(ref, est, filter_length, float(clamp_db or 0.0), lengths=lengths, perm=perm)[0])
    torch.cuda.current_stream().synchronize()
    return h.numpy().copy()


# ---------------------------------------------------------------------------------------------------------------- STOI / ESTOI
# The reference scores every source with pystoi's stoi(ref, est, fs, extended=True) (evaluate.py:113-130).  pystoi is a
# third-party package that is not installed here and is not under /root/reference: what follows restates the PUBLISHED
# algorithm — Taal, Hendriks, Heusdens, Jensen, "An Algorithm for Intelligibility Prediction of Time-Frequency Weighted Noisy
# Speech" (IEEE TASLP 2011) and Jensen, Taal, "An Algorithm for Predicting the Intelligibility of Speech Masked by Modulated
# Noise Maskers" (IEEE/ACM TASLP 2016, the extended measure) — with the constants of the authors' Matlab code that pystoi
# follows: 10 kHz, 256-sample Hann frames at 50 % overlap zero-padded to 512 bins, 15 one-third octave bands from 150 Hz,
# 30-frame (384 ms) segments, -15 dB clipping, 40 dB dynamic range for the silent-frame removal.  PARITY UNPINNED against the
# package (no vectors can be fetched); pinned by an independent loop-form restatement (oracle/stoi_oracle.py) and by the
# properties the papers state (tests/test_metrics_cpu.py).  Host-side numpy on a few seconds of audio per source.
_STOI_FS, _STOI_FRAME, _STOI_NFFT, _STOI_BANDS, _STOI_MINFREQ, _STOI_SEG, _STOI_BETA, _STOI_DYN = 10000, 256, 512, 15, 150.0, 30, -15.0, 40.0
_EPS = float(np.finfo(np.float64).eps)


def _hann_matlab(n):
    """Matlab's hanning(n): the n interior points of a symmetric (n + 2)-point Hann window (no zeros at the ends)"""
    return np.hanning(n + 2)[1:-1]


def _resample_filter(p, q):
    """Anti-aliasing FIR of Octave's resample(x, p, q) (Kaiser-windowed sinc, 60 dB rejection), unit DC gain"""
    g = int(np.gcd(p, q))
    p, q = p // g, q // g
    cutoff = 1.0 / (2.0 * max(p, q))
    rolloff = cutoff / 10.0
    rej_db = 60.0
    L = int(np.ceil((rej_db - 8.0) / (28.714 * rolloff)))
    t = np.arange(-L, L + 1)
    ideal = 2.0 * p * cutoff * np.sinc(2.0 * cutoff * t)
    beta = 0.1102 * (rej_db - 8.7)
    h = np.kaiser(2 * L + 1, beta) * ideal
    return h / np.sum(h), p, q


def _resample(x, fs_to, fs_from):
    from scipy.signal import resample_poly
    h, p, q = _resample_filter(int(fs_to), int(fs_from))
    return resample_poly(x, p, q, window=h)


# the host form under public names (ops.Resampler is the device form of the same definition with the same filter)
resample_filter = _resample_filter
resample = _resample


def _thirdoct(fs, nfft, num_bands, min_freq):
    """[num_bands, nfft/2+1] 0/1 matrix: DFT bins of each one-third octave band (band edges snapped to the nearest bin)"""
    f = np.linspace(0, fs, nfft + 1)[: nfft // 2 + 1]
    k = np.arange(num_bands, dtype=np.float64)
    lo = min_freq * 2.0 ** ((2 * k - 1) / 6.0)
    hi = min_freq * 2.0 ** ((2 * k + 1) / 6.0)
    obm = np.zeros((num_bands, f.size))
    for i in range(num_bands):
        a = int(np.argmin((f - lo[i]) ** 2))
        b = int(np.argmin((f - hi[i]) ** 2))
        obm[i, a:b] = 1.0
    return obm


def _frames(x, n, hop):
    """[number of frames, n] view-free framing; the last start is < len(x) - n (the authors' loop bound)"""
    starts = np.arange(0, len(x) - n, hop)
    if starts.size == 0:
        return np.zeros((0, n))
    return x[starts[:, None] + np.arange(n)[None, :]]


def _remove_silent_frames(x, y, dyn_range, n, hop):
    w = _hann_matlab(n)
    xf, yf = _frames(x, n, hop) * w, _frames(y, n, hop) * w
    if xf.shape[0] == 0:
        return np.zeros(0), np.zeros(0)
    energy = 20.0 * np.log10(np.linalg.norm(xf, axis=1) + _EPS)
    keep = (np.max(energy) - dyn_range - energy) < 0
    xf, yf = xf[keep], yf[keep]
    out = []
    for fr in (xf, yf):  # overlap-add of the kept frames
        sig = np.zeros((fr.shape[0] - 1) * hop + n if fr.shape[0] else 0)
        for i in range(fr.shape[0]):
            sig[i * hop:i * hop + n] += fr[i]
        out.append(sig)
    return out[0], out[1]


_OBM = None


def stoi(ref, est, fs, extended=True):
    """Short-time objective intelligibility of `est` with respect to the clean `ref` (1-D arrays, same length), sample rate
    fs.  extended=True: ESTOI (the reference's default, evaluate.py:215-217 --stoi-no-extended switches it off).  Signals with
    fewer than 30 frames after the removal of silent frames return 1e-5, like the package."""
    global _OBM
    x = np.asarray(ref, dtype=np.float64).reshape(-1)
    y = np.asarray(est, dtype=np.float64).reshape(-1)
    if x.shape != y.shape:
        raise ValueError("stoi: ref and est must have the same length")
    if int(fs) != _STOI_FS:
        x, y = _resample(x, _STOI_FS, fs), _resample(y, _STOI_FS, fs)
    x, y = _remove_silent_frames(x, y, _STOI_DYN, _STOI_FRAME, _STOI_FRAME // 2)
    w = _hann_matlab(_STOI_FRAME)
    X = np.fft.rfft(_frames(x, _STOI_FRAME, _STOI_FRAME // 2) * w, n=_STOI_NFFT).T  # [bins, frames]
    Y = np.fft.rfft(_frames(y, _STOI_FRAME, _STOI_FRAME // 2) * w, n=_STOI_NFFT).T
    if X.shape[-1] < _STOI_SEG:
        return 1e-5
    if _OBM is None:
        _OBM = _thirdoct(_STOI_FS, _STOI_NFFT, _STOI_BANDS, _STOI_MINFREQ)
    xt = np.sqrt(_OBM @ (np.abs(X) ** 2))  # [bands, frames]
    yt = np.sqrt(_OBM @ (np.abs(Y) ** 2))
    n = xt.shape[1] - _STOI_SEG + 1
    idx = np.arange(n)[:, None] + np.arange(_STOI_SEG)[None, :]
    xs, ys = xt[:, idx].transpose(1, 0, 2), yt[:, idx].transpose(1, 0, 2)  # [segments, bands, 30]
    if extended:
        def rowcol(a):  # rows (bands) then columns (frames) to zero mean / unit norm
            a = a - a.mean(axis=2, keepdims=True)
            a = a / (np.sqrt((a * a).sum(axis=2, keepdims=True)) + _EPS)
            a = a - a.mean(axis=1, keepdims=True)
            return a / (np.sqrt((a * a).sum(axis=1, keepdims=True)) + _EPS)
        return float(np.sum(rowcol(xs) * rowcol(ys)) / _STOI_SEG / n)
    norm = np.linalg.norm(xs, axis=2, keepdims=True) / (np.linalg.norm(ys, axis=2, keepdims=True) + _EPS)
    yn = ys * norm
    yp = np.minimum(yn, xs * (1.0 + 10.0 ** (-_STOI_BETA / 20.0)))
    yp = yp - yp.mean(axis=2, keepdims=True)
    xz = xs - xs.mean(axis=2, keepdims=True)
    yp = yp / (np.linalg.norm(yp, axis=2, keepdims=True) + _EPS)
    xz = xz / (np.linalg.norm(xz, axis=2, keepdims=True) + _EPS)
    return float(np.sum(yp * xz) / (n * _STOI_BANDS))


def stoi_batch(ref, est, fs, extended=True, lengths=None, perm=None):
    """stoi() of every source of a zero-padded batch, computed on the device (ops.stoi, csrc/stoi.hip): ref, est [B,S,T]
    device tensors -> [B,S] float64 numpy array; estimate row perm[b][i] (default i) against reference row i over the first
    lengths[b] (default T) samples.  One pinned, non-blocking readback of B * S numbers on the current stream."""
    d = ops.stoi(ref, est, fs, extended=extended, lengths=lengths, perm=perm)
    h = torch.empty(d.shape, dtype=d.dtype, pin_memory=True)
    h.copy_(d, non_blocking=True)
    torch.cuda.current_stream().synchronize()
    return h.numpy().copy()


# ---------------------------------------------------------------------------------------------------------------- composite
# The reference scores enhancement with evaluate_covl.py: Hu & Loizou's composite measures CSIG / CBAK / COVL, three linear
# formulas over the log-likelihood ratio (LLR), the weighted spectral slope (WSS), the segmental SNR and PESQ.  What follows
# restates its llr (:358-408, lpcoeff :62-95), wss (:155-355), SSNR (:106-152) and the aggregation of eval_composite (:18-54)
# in vectorised float64 numpy.  Not reproduced: the float32 casts of the autocorrelation, the LPC vector and the quadratic forms
# in lpcoeff / llr, and SSNR's in-place float32 mean removal and rescaling (rounding noise only; tests/golden records it).
_COMP_CENT = np.array([50.0, 120, 190, 260, 330, 400, 470, 540, 617.372, 703.378, 798.717, 904.128, 1020.38, 1148.30, 1288.72,
                       1442.54, 1610.70, 1794.16, 1993.93, 2211.08, 2446.71, 2701.97, 2978.04, 3276.17, 3597.63])
_COMP_BW = np.array([70.0, 70, 70, 70, 70, 70, 70, 77.3724, 86.0056, 95.3398, 105.411, 116.256, 127.914, 140.423, 153.823,
                     168.154, 183.457, 199.776, 217.153, 235.631, 255.255, 276.072, 298.126, 321.465, 346.136])
COMPOSITE_RATES = (8000, 16000)
_COMP_CACHE = {}


def composite_params(fs):
    """(win, skip, n_fft, LPC order, window [win], critical-band filters [25, n_fft / 2]) of a supported sample rate"""
    fs = int(fs)
    if fs not in COMPOSITE_RATES:
        raise ValueError(f"composite: unsupported sample rate {fs} (supported: 8000, 16000)")
    if fs not in _COMP_CACHE:
        win = int(round(30 * fs / 1000.0))
        skip = win // 4
        n_fft = int(2 ** np.ceil(np.log(2 * win) / np.log(2)))
        half = n_fft // 2
        window = 0.5 * (1 - np.cos(2 * np.pi * (np.linspace(1, win, win) / (win + 1))))
        max_freq = fs / 2
        min_factor = np.exp(-30.0 / (2 * 2.303))
        filt = np.zeros((25, half))
        j = np.arange(half)
        for i in range(25):
            f0 = (_COMP_CENT[i] / max_freq) * half
            bw = (_COMP_BW[i] / max_freq) * half
            norm_factor = np.log(_COMP_BW[0]) - np.log(_COMP_BW[i])
            row = np.exp(-11 * (((j - np.floor(f0)) / bw) ** 2) + norm_factor)
            filt[i] = row * (row > min_factor)
        _COMP_CACHE[fs] = (win, skip, n_fft, 10 if fs < 10000 else 16, window, filt)
    return _COMP_CACHE[fs]


def composite_num_frames(length, fs):
    """int(len / skip - win / skip) of the reference, in integers"""
    win, skip = composite_params(fs)[:2]
    return max(0, (int(length) - win) // skip)


def composite_trim_count(n):
    """int(round(n * 0.95)): Python's round of the double product, half to even"""
    return int(round(n * 0.95))


def _comp_frames(x, fs):
    win, skip, _, _, window, _ = composite_params(fs)
    n = composite_num_frames(len(x), fs)
    idx = (np.arange(n) * skip)[:, None] + np.arange(win)[None, :]
    return x[idx] * window[None, :] if n else np.zeros((0, win))


def composite_band_db(x, fs):
    """[frames, 25] critical-band energies in dB (floor 1e-10) of the windowed frames of x"""
    _, _, n_fft, _, _, filt = composite_params(fs)
    fr = _comp_frames(np.asarray(x, dtype=np.float64).reshape(-1), fs)
    spec = np.abs(np.fft.fft(fr, n_fft, axis=1)[:, : n_fft // 2]) ** 2
    return 10 * np.log10(np.maximum(spec @ filt.T, 1e-10))


def _comp_peaks(db, slope):
    """the reference's nearest-peak search (:292-315) on every frame at once: [frames, 24] peak levels"""
    n, nb = slope.shape
    rows = np.arange(n)
    out = np.zeros_like(slope)
    for i in range(nb):
        up = slope[:, i] > 0
        r = np.full(n, i)  # to the right while the slope stays > 0
        while True:
            go = up & (r < nb) & (slope[rows, np.minimum(r, nb - 1)] > 0)
            if not go.any():
                break
            r = r + go
        l = np.full(n, i)  # to the left while it stays <= 0
        while True:
            go = ~up & (l >= 0) & (slope[rows, np.maximum(l, 0)] <= 0)
            if not go.any():
                break
            l = l - go
        out[:, i] = np.where(up, db[rows, np.maximum(r - 1, 0)], db[rows, np.minimum(l + 1, nb)])
    return out


def _comp_wss(dbx, dby):
    sx, sy = np.diff(dbx, axis=1), np.diff(dby, axis=1)
    w = 0.0
    for db, slope in ((dbx, sx), (dby, sy)):
        peak = _comp_peaks(db, slope)
        wmax = 20 / (20 + db.max(axis=1, keepdims=True) - db[:, :-1])
        wloc = 1 / (1 + peak - db[:, :-1])
        w = w + wmax * wloc
    w = w / 2
    return np.sum(w * (sx - sy) ** 2, axis=1) / np.sum(w, axis=1)


def _comp_lpc(fr, P):
    """autocorrelation lags 0 .. P and Levinson-Durbin in the reference's operation order (:62-90), every frame at once
    -> (R [frames, P + 1], lp [frames, P + 1] = [1, -a])"""
    n, win = fr.shape
    R = np.stack([np.sum(fr[:, : win - k] * fr[:, k:], axis=1) for k in range(P + 1)], axis=1)
    a = np.ones((n, P))
    E = R[:, 0].copy()
    for i in range(P):
        sum_term = np.sum(a[:, :i] * R[:, i:0:-1], axis=1) if i else 0.0
        rc = (R[:, i + 1] - sum_term) / np.maximum(1e-15, E)
        if i:
            a[:, :i] = a[:, :i] - rc[:, None] * a[:, :i][:, ::-1]
        a[:, i] = rc
        E = (1 - rc * rc) * E
    return R, np.concatenate([np.ones((n, 1)), -a], axis=1)


def _comp_llr(frx, fry, P):
    Rx, ax = _comp_lpc(frx, P)
    _, ay = _comp_lpc(fry, P)
    k = np.abs(np.arange(P + 1)[:, None] - np.arange(P + 1)[None, :])
    toep = Rx[:, k]  # [frames, P + 1, P + 1]
    num = np.maximum(1e-10, np.einsum("ni,nij,nj->n", ay, toep, ay))
    den = np.maximum(1e-10, np.einsum("ni,nij,nj->n", ax, toep, ax))
    return np.log(num / den)


def _comp_segsnr(x, y, fs):
    with np.errstate(divide="ignore", invalid="ignore"):
        x = x - x.mean()
        y = y - y.mean()
        y = y * (np.max(np.abs(x)) / np.max(np.abs(y)))
        fx, fy = _comp_frames(x, fs), _comp_frames(y, fs)
        snr = 10 * np.log10(np.sum(fx ** 2, axis=1) / (np.sum((fx - fy) ** 2, axis=1) + 1e-10) + 1e-10)
    return np.minimum(np.maximum(snr, -10), 35)


def _comp_trimmed_mean(v, m):
    return float(np.cumsum(np.sort(v)[:m])[-1] / m) if m else float("nan")  # summed in ascending order


def composite(ref, est, fs=16000):
    """The signal measures behind CSIG / CBAK / COVL for one pair of 1-D arrays of one length (evaluate_covl.py, float64): ->
    dict(llr = mean of the int(round(0.95 n)) smallest frame LLRs, wss = the same of the frame WSS values, segsnr = mean
    segmental SNR, n_frames, llr_frames, wss_frames, segsnr_frames).  No frame (len < win + skip): NaN, like the reference's
    mean of an empty list.  The arguments are not modified (the reference's SSNR removes their means in place)."""
    x = np.asarray(ref, dtype=np.float64).reshape(-1)
    y = np.asarray(est, dtype=np.float64).reshape(-1)
    if x.shape != y.shape:
        raise ValueError("composite: ref and est must have the same length")
    P = composite_params(fs)[3]
    n = composite_num_frames(len(x), fs)
    if n == 0:
        z = np.zeros(0)
        return dict(llr=float("nan"), wss=float("nan"), segsnr=float("nan"), n_frames=0, llr_frames=z, wss_frames=z.copy(),
                    segsnr_frames=z.copy())
    with np.errstate(divide="ignore", invalid="ignore"):
        llr = _comp_llr(_comp_frames(x, fs), _comp_frames(y, fs), P)
        wss = _comp_wss(composite_band_db(x, fs), composite_band_db(y, fs))
    seg = _comp_segsnr(x, y, fs)
    m = composite_trim_count(n)
    return dict(llr=_comp_trimmed_mean(llr, m), wss=_comp_trimmed_mean(wss, m), segsnr=float(np.cumsum(seg)[-1] / n), n_frames=n,
                llr_frames=llr, wss_frames=wss, segsnr_frames=seg)


def composite_batch(ref, est, fs=16000, lengths=None, perm=None):
    """composite() of every source of a zero-padded batch, computed on the device (ops.composite, csrc/composite.hip): ref, est
    [B,S,T] device tensors -> [B,S,4] float64 numpy array {llr, wss, segsnr, n_frames}; estimate row perm[b][i] (default i)
    against reference row i over the first lengths[b] (default T) samples.  One pinned, non-blocking readback of 4 B S numbers
    on the current stream."""
    d = ops.composite(ref, est, fs=fs, lengths=lengths, perm=perm)
    h = torch.empty(d.shape, dtype=d.dtype, pin_memory=True)
    h.copy_(d, non_blocking=True)
    torch.cuda.current_stream().synchronize()
    return h.numpy().copy()


def eval_composite(llr, wss, segsnr, pesq):
    """CSIG / CBAK / COVL from the three signal measures and a PESQ score (evaluate_covl.py:47-59: Hu & Loizou's linear
    formulas, each trimmed to [1, 5]).  pesq=None (PESQ is third-party code this package does not restate): three Nones."""
    if pesq is None:
        return {"csig": None, "cbak": None, "covl": None}
    trim = lambda v: min(max(v, 1), 5)
    return {"csig": trim(3.093 - 1.029 * llr + 0.603 * pesq - 0.009 * wss),
            "cbak": trim(1.634 + 0.478 * pesq - 0.007 * wss + 0.063 * segsnr),
            "covl": trim(1.594 + 0.805 * pesq - 0.512 * llr - 0.007 * wss)}


def si_sdr_loss(est, ref, zero_mean=True, clamp_db=30.0, sign_flip=True):
    """SISDRLoss(zero_mean, clamp_db, sign_flip), mean-reduced (reference models/losses.py:8-37 over
    fast_bss_eval.si_sdr_pit_loss): the SI-SDR of the best source permutation from the Gram matrices above, averaged over
    sources and batch; sign_flip=True returns the SI-SDR itself, False its negative.  A float64 scalar tensor."""
    if zero_mean:
        est, ref = est - est.mean(dim=-1, keepdim=True), ref - ref.mean(dim=-1, keepdim=True)
    sdr, _, _, _ = si_bss_eval_sources(ref.contiguous(), est.contiguous(), clamp_db=float(clamp_db) if clamp_db else 100.0)
    v = float(np.mean(sdr))
    return torch.tensor(v if sign_flip else -v, dtype=torch.float64)
