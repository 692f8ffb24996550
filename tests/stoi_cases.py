"""Inputs of the STOI tests (tests/test_stoi_cpu.py, tests/test_stoi_gpu.py): speech-like references with a stretch that the
silent-frame removal really drops, noisy estimates, and the distance of every frame's energy from the 40 dB threshold (so
that no comparison between two float64 implementations can turn on a keep decision)."""
import numpy as np

from diffsep_amd import metrics, synth

# (fs, T): 4 s / 8 kHz (the bench utterance), 10 s / 16 kHz, 12.5 s / 8 kHz, and 10 kHz (no resampling)
CONFIGS = [(8000, 32000), (16000, 160000), (8000, 100000), (10000, 32000)]
N_UTT = 8


def pair(i, T, fs):
    """-> (ref [2,T], est [2,T]) float32: the sources of synth_mixture(i) with [T/4, T/4 + T/8) scaled by 1e-4, and
    ref + 0.3 std(ref) x synth.normal("probe", T, i) ("probe1" for the second source)"""
    ref = synth.synth_mixture(i, T=T, fs=fs)[1].astype(np.float64)
    ref[:, T // 4:T // 4 + T // 8] *= 1e-4
    est = np.stack([r + 0.3 * np.std(r) * synth.normal("probe" if s == 0 else f"probe{s}", T, i) for s, r in enumerate(ref)])
    return ref.astype(np.float32), est.astype(np.float32)


def frame_energies(x, fs):
    """dB energies of the windowed 10 kHz frames of x, as metrics._remove_silent_frames computes them"""
    x = np.asarray(x, dtype=np.float64)
    if int(fs) != 10000:
        x = metrics._resample(x, 10000, fs)
    fr = metrics._frames(x, 256, 128) * metrics._hann_matlab(256)
    return 20.0 * np.log10(np.linalg.norm(fr, axis=1) + metrics._EPS)


def threshold_margin(x, fs):
    """(smallest distance in dB of a frame's energy from the keep threshold, frames, kept frames)"""
    e = frame_energies(x, fs)
    d = np.max(e) - 40.0 - e
    return float(np.min(np.abs(d))), int(e.size), int(np.sum(d < 0))
