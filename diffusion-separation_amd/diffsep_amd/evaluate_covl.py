"""Composite enhancement measures CSIG / CBAK / COVL (Hu & Loizou) of a folder of enhanced files — the reference's
evaluate_covl.py and its command line:

    python -m diffsep_amd.evaluate_covl clean_path enhanced_path

clean_path holds `NNNN.tgtK.wav`, enhanced_path `NNNN.enhK.wav` (filename_tgt2enh, evaluate_covl.py:411-416); the `NNN_tgtK.wav` /
`NNN_enhK.wav` names that diffsep_amd.evaluate writes into its wav/<split>/ folder are read the same way, so both arguments may
name that folder.  `<split>_covl.json` ({sample: {csig, cbak, covl: one value per channel}}) and `<split>_summary_covl.json`
(their means and "number") go two levels above enhanced_path, <split> being its name (evaluate_covl.py:442-443,471-474).

Extensions: every channel record also holds llr / wss / segsnr, the three signal measures the composites are built from.
--on {host,device}: diffsep_amd.metrics.composite in numpy, or the HIP kernels of diffsep_composite on --batch K files at a time
(zero-padded, with their lengths).  PESQ, the fourth ingredient, is ITU-T P.862 code behind the third-party `pesq` package and
is not restated: --pesq-json FILE ({sample: [pesq per channel]}, computed elsewhere) supplies it; without the file the package is
used if it imports; without both csig / cbak / covl are null and the summary lists them under "not_computed".

Differences from the reference, on purpose: it resamples every file to 16 kHz with librosa's default resampler; here a file at
another rate is refused by name, unless --resample asks for the conversion: then it is converted with the PROJECT's filter
(metrics.resample_filter: Octave's Kaiser-windowed sinc, 60 dB; not librosa's), by the HIP resampler --batch files at a time with
--on device and by metrics.resample with --on host, both on the same taps, rounded to float32 like a loaded file.  Its PESQ
call sees the signals after SSNR has removed their means and rescaled the estimate in place (a quirk, kept: the package, when
present, is handed the same signals)."""
import argparse
import json
import re
from pathlib import Path

import numpy as np

from . import metrics, wavio

FS = 16000
_NAME = re.compile(r"^(\d+)[._]tgt(\d+)$")


def filename_tgt2enh(tgt_path, enhanced_path):
    """NNNN.tgtK.wav -> (NNNN, K, enhanced_path / NNNN.enhK.wav); the separator and the digits of the target's name are kept"""
    m = _NAME.match(tgt_path.stem)
    if not m:
        return None
    sep = tgt_path.stem[len(m.group(1))]
    return int(m.group(1)), int(m.group(2)), enhanced_path / f"{m.group(1)}{sep}enh{m.group(2)}.wav"


def _load(path, resample=False):
    """channel 0 of the file; resample=False: refused unless it is at 16 kHz, True: (samples, rate) whatever the rate"""
    wav, sr = wavio.load(path)
    if resample:
        return wav[0].numpy(), sr
    if sr != FS:
        raise SystemExit(f"{path}: sample rate {sr}, not {FS} (the reference resamples with librosa; this tool does not: "
                         "resample the file first, or pass --resample for the project's own filter)")
    return wav[0].numpy()


def _to_16k(loaded, on, batch):
    """[(samples, rate)] -> float32 samples at 16 kHz: files at another rate through the project's filter, on the device `batch`
    rows of one rate per launch (ops.Resampler on the taps metrics.resample uses) or on the host (metrics.resample)"""
    out = [x if sr == FS else None for x, sr in loaded]
    for sr in sorted({sr for _, sr in loaded if sr != FS}):
        sel = [i for i, (_, r) in enumerate(loaded) if r == sr]
        if on == "host":
            for i in sel:
                out[i] = metrics.resample(loaded[i][0].astype(np.float64), FS, sr).astype(np.float32)
            continue
        import torch
        from . import ops
        if not torch.cuda.is_available():
            raise SystemExit("--on device needs a GPU (use --on host)")
        h, p, _ = metrics.resample_filter(FS, sr)
        rs = ops.Resampler(sr, FS, taps=h * p)
        for k in range(0, len(sel), batch):
            part = sel[k:k + batch]
            lens = [len(loaded[i][0]) for i in part]
            x = np.zeros((len(part), max(lens)), np.float32)
            for b, i in enumerate(part):
                x[b, :lens[b]] = loaded[i][0]
            y, new = rs(torch.from_numpy(x).cuda(), lengths=lens)
            y = y.cpu().numpy()
            for b, i in enumerate(part):
                out[i] = y[b, :new[b]]
    return out


def _pesq_fn():
    try:
        from pesq import pesq
    except Exception:
        return None

    def run(ref, est):  # the signals as the reference's SSNR leaves them (evaluate_covl.py:117-119), float32
        ref = ref - ref.mean()
        est = est - est.mean()
        est = est * (np.max(np.abs(ref)) / np.max(np.abs(est)))
        return float(pesq(FS, ref, est, "wb"))
    return run


def _score_host(pairs):
    return [[r["llr"], r["wss"], r["segsnr"]] for r in (metrics.composite(ref, est, FS) for ref, est in pairs)]


def _score_device(pairs, batch):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("--on device needs a GPU (use --on host)")
    out = []
    for k in range(0, len(pairs), batch):
        part = pairs[k:k + batch]
        lens = [len(r) for r, _ in part]
        ref = np.zeros((len(part), 1, max(lens)), np.float32)
        est = np.zeros_like(ref)
        for b, (r, e) in enumerate(part):
            ref[b, 0, :lens[b]], est[b, 0, :lens[b]] = r, e
        got = metrics.composite_batch(torch.from_numpy(ref).cuda(), torch.from_numpy(est).cuda(), FS, lengths=lens)
        out += [[float(v) for v in got[b, 0, :3]] for b in range(len(part))]
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description="Compute COVL, CSIG, and CBAK metrics from Hu and Loizou")
    ap.add_argument("clean_path", type=Path, help="Path to folder of clean files")
    ap.add_argument("enhanced_path", type=Path, help="Path to folder of enhanced files")
    ap.add_argument("--on", choices=["host", "device"], default="device",
                    help="where LLR / WSS / segmental SNR are computed: numpy on the host, or the HIP kernels (default)")
    ap.add_argument("--batch", type=int, default=16, help="--on device: files per kernel call (zero-padded to the longest)")
    ap.add_argument("--resample", action="store_true",
                    help="convert files that are not at 16 kHz with the project's filter (--on device: the HIP resampler, --batch "
                         "files per launch; --on host: numpy) instead of refusing them")
    ap.add_argument("--pesq-json", type=Path, default=None, help="{sample index: [PESQ per channel]} computed elsewhere")
    args = ap.parse_args(argv)

    todo = []
    for tgt in sorted(args.clean_path.rglob("*.wav")):
        hit = filename_tgt2enh(tgt, args.enhanced_path)
        if hit is not None:
            todo.append((hit[0], hit[1], tgt, hit[2]))
    todo.sort(key=lambda t: t[:2])
    if not todo:
        raise SystemExit(f"{args.clean_path}: no NNNN.tgtK.wav file")
    pairs = []
    if args.resample:
        loaded = _to_16k([_load(f, True) for _, _, tgt, enh in todo for f in (tgt, enh)], args.on, max(1, args.batch))
    for k, (_, _, tgt, enh) in enumerate(todo):
        ref, est = (loaded[2 * k], loaded[2 * k + 1]) if args.resample else (_load(tgt), _load(enh))
        n = min(len(ref), len(est))  # (evaluate_covl.py:23-26)
        pairs.append((ref[:n], est[:n]))

    pesq_table, pesq_fn = None, None
    if args.pesq_json is not None:
        with open(args.pesq_json) as f:
            pesq_table = {int(k): v for k, v in json.load(f).items()}
    else:
        pesq_fn = _pesq_fn()

    scores = _score_host(pairs) if args.on == "host" else _score_device(pairs, max(1, args.batch))
    keys = ("csig", "cbak", "covl", "llr", "wss", "segsnr")
    output = {}
    for (idx, ch, _, _), (ref, est), (llr, wss, seg) in zip(todo, pairs, scores):
        if pesq_table is not None:
            try:
                p = float(pesq_table[idx][ch])
            except (KeyError, IndexError):
                raise SystemExit(f"{args.pesq_json}: no PESQ value for sample {idx} channel {ch}")
        else:
            p = pesq_fn(ref, est) if pesq_fn is not None else None
        rec = output.setdefault(idx, {k: [] for k in keys})
        comp = metrics.eval_composite(llr, wss, seg, p)
        for k, v in (*comp.items(), ("llr", llr), ("wss", wss), ("segsnr", seg)):
            rec[k].append(None if v is None else float(v))

    missing = [k for k in keys if any(v is None for rec in output.values() for v in rec[k])]
    summary = {k: float(np.mean([np.mean(rec[k]) for rec in output.values()])) for k in keys if k not in missing}
    summary.update({"number": len(output), "not_computed": missing, "on": args.on})
    print(summary)

    split = args.enhanced_path.name
    output_path = args.enhanced_path.absolute().parents[1]
    with open(output_path / f"{split}_covl.json", "w") as f:
        json.dump(output, f, indent=2)
    with open(output_path / f"{split}_summary_covl.json", "w") as f:
        json.dump(summary, f, indent=2)
    return output_path


if __name__ == "__main__":
    main()
