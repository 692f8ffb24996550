"""Device STOI / ESTOI (csrc/stoi.hip, diffsep_stoi) — what can be checked without a GPU: the C-ABI surface, the host-side
workspace arithmetic and argument checks, the evaluate flag, and the precondition of the GPU parity tests (no frame of any
test signal near the 40 dB keep threshold)."""
import ctypes as C

import pytest

import stoi_cases as SC
from diffsep_amd import _lib
from diffsep_amd import evaluate as ev


@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_both_libraries_export_the_stoi_entries(kind):
    l = _lib.lib(kind)
    for name in ("diffsep_stoi", "diffsep_stoi_workspace_bytes"):
        assert name in _lib.EXPORTS and getattr(l, name) is not None


def test_workspace_bytes_is_monotone_and_rejects_bad_input():
    ws = _lib.lib().diffsep_stoi_workspace_bytes
    base = ws(4, 2, 32000, 8000)
    assert base > 0
    assert ws(5, 2, 32000, 8000) > base and ws(4, 3, 32000, 8000) > base and ws(4, 2, 32001, 8000) >= base
    assert ws(4, 2, 64000, 8000) > base
    prev = 0
    for T in (100, 300, 1000, 32000, 160000, 1000000):
        n = ws(2, 2, T, 16000)
        assert n > prev
        prev = n
    # the resampled signals alone: 2 x float64 x ceil(T 10000 / fs) per pair
    assert base >= 4 * 2 * 2 * 8 * 40000
    for fs in (8000, 10000, 16000, 44100, 48000):
        assert ws(1, 1, 32000, fs) > 0
    for bad in ((1, 1, 32000, 0), (1, 1, 32000, -8000), (1, 1, 32000, 9999), (0, 2, 32000, 8000), (2, 0, 32000, 8000),
                (2, 2, 0, 8000)):
        assert ws(*bad) == -1
        assert b"stoi" in _lib.lib().diffsep_last_error()


def test_bad_arguments_are_refused_before_anything_is_launched():
    # every check of diffsep_stoi precedes its first HIP call: these return non-zero with a message on a machine without a GPU
    l = _lib.lib()
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    big = 1 << 40
    assert l.diffsep_stoi(p, p, p, 1, 1, 300, None, None, 0, 1, p, big, None) != 0
    assert b"sample rate" in l.diffsep_last_error()
    assert l.diffsep_stoi(p, p, p, 0, 1, 300, None, None, 8000, 1, p, big, None) != 0
    assert b"bad shape" in l.diffsep_last_error()
    need = l.diffsep_stoi_workspace_bytes(1, 1, 300, 8000)
    assert l.diffsep_stoi(p, p, p, 1, 1, 300, None, None, 8000, 1, p, need - 1, None) != 0
    assert b"workspace too small" in l.diffsep_last_error()
    assert l.diffsep_stoi(None, p, p, 1, 1, 300, None, None, 8000, 1, p, big, None) != 0
    assert b"null pointer" in l.diffsep_last_error()


def test_evaluate_flag(capsys):
    ap = ev.build_parser()
    assert ap.parse_args(["--synthetic", "1"]).stoi_on == "host"           # the default does not change
    assert ap.parse_args(["--synthetic", "1", "--stoi-on", "device"]).stoi_on == "device"
    with pytest.raises(SystemExit):
        ap.parse_args(["--stoi-on", "gpu"])
    with pytest.raises(SystemExit):
        ap.parse_args(["--help"])
    text = capsys.readouterr().out
    assert "--stoi-on {host,device}" in text


def test_waveforms_stay_on_the_device_unless_saved_or_scored_on_the_host():
    ap = ev.build_parser()
    group = [3, 4, 5]
    host = ap.parse_args(["--save-n", "0"])
    dev = ap.parse_args(["--save-n", "0", "--stoi-on", "device"])
    assert ev.needs_host_waveforms(host, group) and not ev.needs_host_waveforms(dev, group)
    assert not ev.needs_host_waveforms(ap.parse_args(["--save-n", "0", "--no-stoi"]), group)
    assert ev.needs_host_waveforms(ap.parse_args(["--stoi-on", "device"]), group)                   # default: save all
    assert ev.needs_host_waveforms(ap.parse_args(["--save-n", "4", "--stoi-on", "device"]), group)  # utterance 3 is saved
    assert not ev.needs_host_waveforms(ap.parse_args(["--save-n", "3", "--stoi-on", "device"]), group)


@pytest.mark.parametrize("fs,T", SC.CONFIGS)
def test_no_test_signal_has_a_frame_near_the_keep_threshold(fs, T):
    # the GPU parity tests compare float64 implementations at 1e-9: that presupposes identical keep decisions, i.e. no frame
    # energy within rounding distance of max - 40 dB.  Demanded: 0.1 dB (found: >= 0.23 dB over all 64 signals).
    removed = 0
    for i in range(SC.N_UTT):
        ref, _ = SC.pair(i, T, fs)
        for r in ref:
            margin, n, kept = SC.threshold_margin(r, fs)
            assert margin >= 0.1, (fs, T, i, margin)
            assert 30 < kept < n                                               # frames really are removed
            removed += n - kept
    assert removed > 0
