"""Inputs of the composite-measure tests (tests/test_composite_cpu.py, tests/test_composite_gpu.py) and of the generator of
tests/golden/golden_composite.npz: speech-like references with an all-zero stretch (it hits every guard: the 1e-15 and 1e-10
clamps, the energy floor, the -10 dB clamp), noisy estimates, and the distance of every spectral slope from zero (so that no
comparison between two float64 implementations can turn on a branch of the peak search)."""
import numpy as np

from diffsep_amd import metrics, synth

# (fs, T) -> frames: the smallest shapes at which each piece can go wrong
#   16000:   599 -> 0 (NaN), 600 -> 1, 1680 -> 10 (m = 10 by half-to-even), 4080 -> 30 (m = 28), 16000 -> 129 (zero stretch),
#            16100 -> 130 (not a multiple of skip);   8000: 300 -> 1, 8000 -> 129 (P = 10, n_fft 512)
SHAPES = [(16000, 599), (16000, 600), (16000, 1680), (16000, 4080), (16000, 16000), (16000, 16100), (8000, 300), (8000, 8000)]
FRAMES = {(16000, 599): 0, (16000, 600): 1, (16000, 1680): 10, (16000, 4080): 30, (16000, 16000): 129, (16000, 16100): 130,
          (8000, 300): 1, (8000, 8000): 129}
N_UTT = 2          # utterances per shape in the golden file and the tests
PESQ_STUBS = (1.0, 2.5, 4.5)
MIN_MARGIN = 1e-6  # dB


def key(fs, T, i):
    return f"fs{fs}_T{T}_u{i}"


def pair(i, T, fs):
    """-> (ref [T], est [T]) float32: the first source of synth_mixture(i) with [T/4, T/4 + 1000) set to zero when T >= 8000,
    and ref + 0.3 std(ref) x synth.normal("probe", T, i)"""
    ref = synth.synth_mixture(i, T=T, fs=fs)[1][0].astype(np.float32)
    if T >= 8000:
        ref[T // 4:T // 4 + 1000] = 0
    est = ref + 0.3 * np.std(ref) * synth.normal("probe", T, i)
    return ref.astype(np.float32), est.astype(np.float32)


def slope_margin(x, fs):
    """smallest non-zero |slope| in dB over all frames and bands of x (inf without one).  A slope is exactly zero only where
    both band energies sit on the 1e-10 floor: deterministic, and allowed."""
    db = metrics.composite_band_db(x, fs)
    if db.shape[0] == 0:
        return float("inf")
    s = np.abs(np.diff(db, axis=1))
    zero = s == 0
    assert np.all((db[:, 1:][zero] == -100.0) & (db[:, :-1][zero] == -100.0)), "a zero slope away from the energy floor"
    return float(np.min(s[~zero])) if np.any(~zero) else float("inf")
