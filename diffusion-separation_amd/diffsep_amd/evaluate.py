"""evaluate.py — the reference's evaluate.py / evaluate_mp.py (evaluate.py:164-443, evaluate_mp.py:154-326,495-528) on the
HIP engine, one rank per GPU.  The reference's command line runs verbatim:

    python -m diffsep_amd.evaluate exp/default/2022-xx/checkpoints/epoch-979.ckpt --test -s log -d 1 --save-n 10 -o results
    python -m diffsep_amd.evaluate --synthetic 32 --synthetic-weights 64 -o out/            (no data set / checkpoint at hand)
    python -m torch.distributed.run --nproc-per-node 8 -m diffsep_amd.evaluate ...          (8 GPUs)

Reference flags (evaluate.py:168-226), same names, defaults and meaning: ckpt (or `__no_proc__`: score the unprocessed
mixture, :245-262), -o/--output_dir, --enhance, -d/--device, -w/--dl-workers, --tag, -l/--limit, --save-n, --val, --test
(one of the two is required unless an extension below names the data), -N, --snr, --corrector-steps, --denoise (argparse
`type=bool` as in the reference: every non-empty value is True), --pesq-mode, --stoi-no-extended, -s/--schedule.  The data
sets come from `<ckpt>/../../hparams.yaml` -> datamodule.{val,test}.dataset like evaluate.py:264-288 (or --dataset-dir).
Output tree (evaluate.py:306-323,436-443): `<output_dir>/<exp>_<ckpt>_<tag_inf>/` (or `<tag>_<tag_inf>`), tag_inf =
`N-.._snr-.._corrstep-.._denoise-.._schedule-..`, holding `<split>.json`, `<split>_summary.json` and
`wav/<split>/NNN_{mix,enh0,enh1,tgt0,tgt1}.wav` (scaled to peak 0.95 together, estimates in the permutation that matches
the targets) for the first --save-n utterances (default: all), and with --fig `fig/<split>/evo_NNN.pdf` for the same
utterances (evaluate.py:29-61,362-376,413-436: the state of six reverse steps next to the clean sources; below).  Not
produced: the PESQ field (ITU-T P.862 C code, third-party `pesq`; null, named under `not_computed`).  STOI /
ESTOI is computed on loader threads (diffsep_amd.metrics.stoi, `--stoi-on host`, the default) or on the GPU
(diffsep_amd.metrics.stoi_batch, `--stoi-on device`: no waveform leaves the device unless it is saved).  --composite (off by
default; without it records and summaries are what they were) adds the signal measures of the reference's evaluate_covl.py to
every record: per-source llr, wss, segsnr from the GPU (diffsep_amd.metrics.composite_batch) and csig / cbak / covl as null
(they need PESQ: diffsep_amd.evaluate_covl takes it from a file).  --bss-eval [--bss-filter-length L] (off by default; without
it records and summaries are what they were) adds the BSS-eval measures with an L-tap distortion filter (default 512:
mir_eval's bss_eval_sources, fast_bss_eval.bss_eval_sources(filter_length=512)) to every record: per-source sdr, sir, sar
under the record's final permutation, clamped to +-100 dB like the SI forms, from the GPU on the worker's stream
(diffsep_amd.metrics.bss_eval_batch; 3 B S numbers cross PCIe); the summary holds their means and `bss_filter_length`.

Utterances are sharded over ranks in contiguous ranges (evaluate_mp.py:495-503); each rank separates its
share, records {batch_idx, si_sdr, si_sir, si_sar, pesq, stoi, nfe, runtime, len_s} per utterance (evaluate.py:394-405;
runtime is measured WITH a device sync, unlike evaluate.py:374-376) and rank 0 gathers everything (RCCL) and writes
<split>.json + <split>_summary.json (evaluate.py:436-443).  Dataset: --dataset-dir ROOT in the WSJ0-mix layout
(datasets/wsj0_mix.py:64-92; with --enhance the VoiceBank-DEMAND layout, datasets/vctk_demand.py:33-36), a flat
ROOT/{mix,s1,s2} folder, or --synthetic N speech-like mixtures.  SI-SDR (scale-invariant
SDR with the best source permutation) is computed in the normalised domain like evaluate.py:360,382.

The reference separates one utterance per sampler call (batch_size=1, evaluate.py:328) because lengths differ.  Here
utterances whose padded spectrogram width W = 64 ceil(F / 64) is equal ride in ONE engine call (--batch, default 16):
the batch is zero-padded on the right to its longest member, the engine keeps every utterance's tail at exactly zero
(diffsep_sampler_ext.lengths_host) and draws its noise from the utterance's own seed, so an utterance's record does
not depend on which batch, stream or rank it was separated in (bit-for-bit with --dtype f32; to the rounding of the
GroupNorm sums of the weight-stationary bf16 convolution otherwise).

--sampler ode [--rtol --atol --max-nfe] separates with the probability-flow ODE sampler instead (adaptive RK45 on the
device, one step controller per utterance: sdes.get_ode_sampler with lengths / seeds, diffsep_ode_sample_each).  The
batches and seeds are the same; an utterance's `nfe` is its own solver's count (solve_ivp's nfev), whatever the others of
its batch needed, each record carries its `ode_status` (0 reached eps, -1 step too small, 1 --max-nfe reached) and the
summary counts them (`ode_status_counts`) and names the `sampler`.  An ODE call blocks the host on one readback per step
attempt, so --streams adds nothing to it.

--sampler ode-fixed [--ode-method {euler,heun,midpoint,rk4,ab2,ddim,dpmpp2m} --ode-steps M --ode-err] separates with the same ODE on a
fixed grid (sdes.get_ode_fixed_sampler, diffsep_ode_sample_fixed): M steps (default N) from t = 1 down to
eps, -s/--schedule choosing the grid.  The call is enqueued like the PC sampler's and reads nothing back, so --streams keeps
batches in flight; `nfe` is the plan's count (heun: 2 M), the summary names `ode_method` and `ode_steps`, and --ode-err adds
`ode_local_err` to every record: the largest over the steps of rms(step - embedded Euler step) / rms(y), read once per batch at
collect time.  Whether such a solve separates as well as the PC sampler at equal cost is not known (no trained checkpoint was
at hand): the flag is the instrument.  Not with --fig, --trajectory or --draws in this version.  --ode-method ddim / dpmpp2m
 are the exponential integrators DDIM and DPM-Solver++ 2M: M evaluations each (`nfe` = M); --ode-err goes with
dpmpp2m, where the step is compared with its DDIM step.

--fig and --trajectory look inside the fused sampler through its tap (diffsep_pc_sample_trace: one small launch between the
corrector and the predictor of a reverse step; batches, streams, seeds, --dtype hybrid and the records are what they are
without them).  --fig: the batches that hold an utterance --save-n selects ask for snapshots of the figure's steps
(figures.snapshot_request: the unique ones of round(linspace(0, 1, 6) (N - 1)), x only) and diffsep_amd.figures draws them,
estimates in the targets' order like the saved wavs; it needs matplotlib and ends with a SystemExit that names it otherwise.
--trajectory: every record gets `si_sdr_steps`, N + 1 lists of the SI-SDR of its sources — the state after each step's
corrector, last the result — under the record's OWN final permutation at every step (a curve follows one source), from the
Gram sums the tap adds up on the device ((N + 1) 3 S^2 doubles per utterance cross PCIe); the last list is the record's
`si_sdr`, and the summary's `si_sdr_steps` is the mean over the utterances (measured: about 5 % of the run's rate, the Gram
pass of every step).  Warm-up calls trace nothing.  Neither runs with
--sampler ode (no fixed steps) or `__no_proc__` (no sampler).

--draws K [--draws-out {mean,medoid,all}] (off by default; without it records and summaries are what they were): every
utterance is separated K times in ONE engine call (it takes K rows of a --batch, which is filled with whole utterances; draw k
under the seed inflight.draw_seeds(utterance seed, K)[k], draw 0 being the run without the flag), the draws are aligned to one
source order and reduced on the device (DiffSepModel.separate_draws, ops.ensemble), and the record's
existing fields are those of the chosen estimate: the mean of the draws (default, and with `all`) or the draw nearest to it.
Added per record: `si_sdr_draws` [K][S], `si_sdr_mean` [S] and `si_sdr_medoid` [S] — each under its own best permutation against
the target, all from one diffsep_gram call — `draws_medoid` and `draws_dist` [K]; the summary gets their means (not of the
index), `draws` and `draws_out`.  `runtime` covers all K draws; `utt_per_s_rank0` counts utterances, i.e. files, not draws.
This is the instrument for the question nobody has measured here: what the mean of K draws buys over one draw.  Not with
--sampler ode, `__no_proc__`, --fig or --trajectory.

--streams K such calls are in flight on K engines / K HIP streams.  What that takes (hardware queues, engines before
streams, workspace reserve, per-utterance seeds and normalisation, pinned uploads, the launch / collect ring, the overflow
re-run) is inflight.py's, shared with separate.py.  Here: main() sets the run up, a SplitRun holds one split's state and
stages / launches / collects a batch and writes the two JSON files, run_split() is the warm-up and the timed region.
"""
import argparse
import json
import os
import time
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass, field
from pathlib import Path
from typing import Callable

import torch
import torch.distributed as dist

from . import _lib, datasets, figures, inflight, metrics, ops, synth, wavio
from .dist_utils import gather_objects, rank_indices
from .inflight import plan_batches  # (its callers import it from here)
from .pl_model import DiffSepModel, cfg_get, default_config, enhancement_config


def compute_metrics(est, ref, n_src=None):
    """est, ref [B,S,T] (zero-padded batches are fine: the zero tails add nothing to the Gram sums) -> per utterance a
    dict with the reference's metric fields (evaluate.py:103-132): the FULL source set is scored with the best
    permutation, then the first n_src entries are kept (n_src = 1 with --enhance: the clean speech; its permutation
    against the noise channel is still searched, evaluate.py:105-111,125-127).  The waveform reductions run in the HIP
    Gram kernel."""
    sdr, sir, sar, perm = metrics.si_bss_eval_sources(ref, est)
    k = sdr.shape[1] if n_src is None else n_src
    return [{"si_sdr": [[float(v) for v in sdr[b, :k]]], "si_sir": [[float(v) for v in sir[b, :k]]],
             "si_sar": [[float(v) for v in sar[b, :k]]], "perm": [int(v) for v in perm[b]]}
            for b in range(sdr.shape[0])]


def needs_host_waveforms(args, group):
    """does finish() have to copy this batch's waveforms to the host?  Only to save them, or to score STOI there."""
    return (not args.no_stoi and args.stoi_on == "host") or args.save_n is None or any(i < args.save_n for i in group)


def load_dataset(args, fs):
    """-> (number of utterances, get(i) -> (mix [1,T], tgt [S,T]) CPU tensors, lengths in samples)"""
    if args.dataset_dir and args.enhance:
        ds = datasets.NoisyDataset(args.dataset_dir, fs=fs, split=args.split)
        n = len(ds) if args.limit is None else min(len(ds), args.limit)
        return n, (lambda i: ds[i]), [ds.num_samples(i) for i in range(n)]
    if args.dataset_dir:
        root = Path(args.dataset_dir)
        if (root / "mix").is_dir():  # flat folder: mix/, s1/, s2/ ...
            names = sorted(p.name for p in (root / "mix").glob("*.wav"))[: args.limit]
            ds = datasets.WavPairs(root / "mix", [root / f"s{k + 1}" for k in range(args.n_speakers)], names, fs)
        else:
            ds = datasets.WSJ0_mix(root, n_spkr=args.n_speakers, fs=fs, cut=args.cut, split=args.split,
                                   max_n_samples=args.limit)
        return len(ds), (lambda i: tuple(t[..., : ds.num_samples(i)] for t in ds[i])), \
            [ds.num_samples(i) for i in range(len(ds))]
    n = args.synthetic
    hi = args.samples if args.samples_max is None else max(args.samples, args.samples_max)
    lens = [args.samples + (i * 7919) % (hi - args.samples + 1) for i in range(n)]  # (--samples-max: varied lengths)

    def get(i):
        mix, tgt = synth.synth_mixture(i, T=lens[i], fs=fs, n_src=args.n_speakers)
        return torch.from_numpy(mix), torch.from_numpy(tgt)
    return n, get, lens


def _hparams_datasets(args, fs_model, splits):
    """evaluate.py:264-288: the data sets named by the experiment's hparams.yaml (two levels above the checkpoint)."""
    import yaml
    hp = Path(args.ckpt).parents[1] / "hparams.yaml"
    if not hp.exists():
        raise SystemExit(f"{hp} not found: the reference reads the data set from it (evaluate.py:265-267); pass --dataset-dir "
                         "ROOT or --synthetic N instead")
    with open(hp, "r") as f:
        config = yaml.safe_load(f)["config"]
    out = {}
    if args.enhance:
        kw = dict(config["datamodule"]["test"]["dataset"])
        kw.pop("_target_", None)
        out["test"] = datasets.NoisyDataset(**kw)
        return out
    for split in splits:
        kw = dict(config["datamodule"][split]["dataset"])
        kw.pop("_target_", None)
        if not Path(kw["path"]).exists():
            kw["path"] = "./data/wsj0_mix"
        out[split] = datasets.WSJ0_mix(**kw)
    return out


def save_samples(mix, est, tgt, wav_out_dir, idx, fs):
    """evaluate.py:70-101: mixture, estimates (already in the targets' order) and targets, scaled TOGETHER to peak 0.95, as
    32-bit float wav (what torchaudio.save writes for a float tensor).  Every source is written (the reference's fixed five
    files are these for two sources)."""
    allw = torch.cat((mix, est, tgt), dim=0).clone()
    allw *= 0.95 / allw.abs().max().clamp(min=1e-30)
    S = est.shape[0]
    wav_out_dir.mkdir(parents=True, exist_ok=True)
    wavio.save(wav_out_dir / f"{idx:03d}_mix.wav", allw[0:1], fs, bits=32)
    for k in range(S):
        wavio.save(wav_out_dir / f"{idx:03d}_enh{k}.wav", allw[1 + k:2 + k], fs, bits=32)
    for k in range(tgt.shape[0]):
        wavio.save(wav_out_dir / f"{idx:03d}_tgt{k}.wav", allw[1 + S + k:2 + S + k], fs, bits=32)


def build_parser():
    ap = argparse.ArgumentParser(description="Run evaluation on validation or test dataset")
    # ---- the reference's arguments (evaluate.py:168-226)
    ap.add_argument("ckpt", nargs="?", default=None, type=Path, help="Path to checkpoint to use ('__no_proc__': score the mixture)")
    ap.add_argument("-o", "--output_dir", "--output-dir", dest="output_dir", type=Path, default=Path("results"), help="The output folder")
    ap.add_argument("--enhance", default=False, action="store_true",
                    help="Compute evaluation metrics for speech enhancement (evaluate.py:173-176,268-271): PriorMixSDE model, "
                         "metrics on the first source (clean speech) only")
    ap.add_argument("-d", "--device", default=0, help="Device to use (default: cuda:0); under torchrun LOCAL_RANK decides")
    ap.add_argument("-w", "--dl-workers", type=int, default=None,
                    help="Number of loader / STOI worker threads (default min(os.cpu_count(), 16))")
    ap.add_argument("--tag", type=str, default=None,
                    help="A tag name for the experiment. If not provided, the experiment and checkpoints name are used.")
    ap.add_argument("-l", "--limit", type=int, default=None, help="Limit the number of samples to process")
    ap.add_argument("--save-n", type=int, default=None, help="Save a limited number of output samples (default: save all)")
    ap.add_argument("--val", action="store_true", help="Run on validation dataset")
    ap.add_argument("--test", action="store_true", help="Run on test dataset")
    ap.add_argument("-N", type=int, default=None, help="Number of steps")
    ap.add_argument("--snr", type=float, default=None, help="Step size of corrector")
    ap.add_argument("--corrector-steps", type=int, default=None, help="Number of corrector steps")
    ap.add_argument("--denoise", type=bool, default=True, help="Use denoising in solver")
    ap.add_argument("--pesq-mode", type=str, choices=["nb", "wb"], default="nb",
                    help="Mode for PESQ 'wb' or 'nb' (accepted; PESQ is not computed: see not_computed in the summary)")
    ap.add_argument("--stoi-no-extended", action="store_true", help="Disable extended mode for STOI")
    ap.add_argument("-s", "--schedule", type=str, default=None, help="Pick a different schedule for the inference")
    # ---- extensions
    ap.add_argument("--split", default=None, choices=["train", "val", "test", "libri2mix_test"],
                    help="with --dataset-dir: the split folder (default test); --val / --test select it the reference's way")
    ap.add_argument("--synthetic-weights", type=int, default=0, metavar="NF")
    ap.add_argument("--dataset-dir", type=str, default=None)
    ap.add_argument("--synthetic", type=int, default=0, help="number of synthetic mixtures")
    ap.add_argument("--samples", type=int, default=32000)
    ap.add_argument("--samples-max", type=int, default=None,
                    help="--synthetic: utterance lengths spread over [--samples, --samples-max] instead of one length")
    ap.add_argument("--n-speakers", type=int, default=2)
    ap.add_argument("--cut", default="max", choices=["min", "max"])
    inflight.add_precision_arguments(ap)  # --dtype, --fp32-steps
    ap.add_argument("--flat-output", action="store_true",
                    help="write <split>.json / <split>_summary.json / wav/ directly into --output_dir instead of the reference's "
                         "<output_dir>/<exp>_<ckpt>_<tag_inf>/ folder")
    ap.add_argument("--no-stoi", action="store_true",
                    help="skip STOI (--stoi-on host: ~0.02 - 0.1 s per utterance and source on one core of the loader pool; "
                         "--stoi-on device: a few kernel launches per batch)")
    ap.add_argument("--stoi-on", choices=["host", "device"], default="host",
                    help="where STOI / ESTOI is computed: host = numpy on the loader threads (needs the waveforms on the host); "
                         "device = the HIP kernels of diffsep_stoi on the worker's stream (B x S numbers cross PCIe)")
    ap.add_argument("--composite", action="store_true",
                    help="also record the signal measures of the composite enhancement scores (evaluate_covl.py): per-source "
                         "llr, wss, segsnr from the HIP kernels of diffsep_composite on the worker's stream, and csig / cbak / covl "
                         "as null (they need PESQ: python -m diffsep_amd.evaluate_covl --pesq-json).  8 or 16 kHz models only")
    ap.add_argument("--bss-eval", action="store_true",
                    help="also record the BSS-eval SDR / SIR / SAR with a time-invariant distortion filter (mir_eval's "
                         "bss_eval_sources): per-source sdr, sir, sar from the HIP kernels of diffsep_bss_eval on the worker's stream")
    ap.add_argument("--bss-filter-length", type=int, default=512, metavar="L",
                    help="taps of the distortion filter of --bss-eval (default 512, 1..1024)")
    ap.add_argument("--score-loss", type=int, default=0, metavar="K",
                    help="also record every utterance's denoising score-matching loss (the reference's val/score_loss): the mean "
                         "of K plain losses at times linspace(t_eps, 1, K) with device noise keyed by the utterance's seed, one "
                         "network evaluation each, in the batch that is separated (default 0: off)")
    ap.add_argument("--seed", type=int, default=0, help="torch.manual_seed before the first utterance: the i-th "
                                                         "utterance gets the i-th draw as its device RNG seed")
    ap.add_argument("--balance", action="store_true",
                    help="multi-GPU: deal the utterances to the ranks by length (longest first, round-robin) instead of "
                         "the reference's contiguous index ranges; needs the lengths (wav headers)")
    ap.add_argument("--batch", type=int, default=16,
                    help="utterances per engine call: those with the same padded spectrogram width share a call "
                         "(zero-padded to the longest; --batch 1 = the reference's one-utterance loop)")
    ap.add_argument("--sampler", default="pc", choices=["pc", "ode", "ode-fixed"],
                    help="pc (default): the reference's predictor-corrector sampler; ode: the probability-flow ODE (adaptive "
                         "RK45), one step controller per utterance of a batch; ode-fixed: the same ODE on a fixed grid "
                         "(--ode-method, --ode-steps), enqueued like pc, so --streams keeps batches in flight")
    ap.add_argument("--ode-method", default=None, choices=["euler", "heun", "midpoint", "rk4", "ab2", "ddim", "dpmpp2m"],
                    help="--sampler ode-fixed: the integrator (default heun); network evaluations for M steps: euler M, heun and "
                         "midpoint 2 M, rk4 4 M, ab2 M + 1; ddim and dpmpp2m (DPM-Solver++ 2M), the exponential integrators: M")
    ap.add_argument("--ode-steps", type=int, default=None, metavar="M",
                    help="--sampler ode-fixed: solver steps from t = 1 down to eps (default: the sampler's N)")
    ap.add_argument("--ode-err", action="store_true",
                    help="--sampler ode-fixed with heun, midpoint or ab2: record ode_local_err, the utterance's largest relative "
                         "local error (max over the steps of rms(step - embedded Euler step) / rms(y)), read once per batch; with "
                         "dpmpp2m: of rms(step - its DDIM step) / rms(y)")
    ap.add_argument("--rtol", type=float, default=1e-5, help="--sampler ode: relative tolerance (reference default)")
    ap.add_argument("--atol", type=float, default=1e-5, help="--sampler ode: absolute tolerance (reference default)")
    ap.add_argument("--max-nfe", type=int, default=0,
                    help="--sampler ode: no step attempt of an utterance starts beyond this many network evaluations (0: unbounded)")
    ap.add_argument("--fig", action="store_true",
                    help="write fig/<split>/evo_NNN.pdf for the utterances --save-n selects (the reference's figure of the reverse "
                         "diffusion: the state of six steps next to the clean sources); needs matplotlib")
    ap.add_argument("--trajectory", action="store_true",
                    help="record si_sdr_steps: the SI-SDR of every source after each reverse step's corrector, and last of the "
                         "result, under the record's final permutation (Gram sums added up on the device inside the sampler)")
    ap.add_argument("--draws", type=int, default=None, metavar="K",
                    help="K posterior draws per utterance in one engine call (an utterance takes K rows of a --batch), aligned "
                         "and reduced on the device; the record's metrics are those of the estimate --draws-out names, and "
                         "si_sdr_draws / si_sdr_mean / si_sdr_medoid / draws_medoid / draws_dist are added (default: off)")
    ap.add_argument("--draws-out", default=None, choices=["mean", "medoid", "all"],
                    help="with --draws: the estimate that is scored and saved: the mean of the draws (default; also with `all`) or "
                         "the draw nearest to the mean")
    ap.add_argument("--streams", type=int, default=4,
                    help="engine calls (batches) in flight per GPU: K engines on K HIP streams; the records do not "
                         "depend on K.  'runtime' of an utterance is its batch's latency / batch size.")
    return ap


def main(argv=None):
    """Returns the folder the results were written to (rank 0; the reference's naming, evaluate.py:306-323)."""
    ap = build_parser()
    args = ap.parse_args(argv)
    splits = [s for s, on in (("val", args.val), ("test", args.test)) if on]
    if not splits:
        if args.split is not None or args.synthetic or args.dataset_dir:
            splits = [args.split or "test"]  # (extensions that name the data themselves)
        else:
            ap.error("No action requested, add --val or --test")
    if args.enhance:
        splits = ["test"] if not args.dataset_dir or args.split is None else [args.split]  # (evaluate.py:268-271: the test set)
    no_proc = str(args.ckpt) == "__no_proc__"
    if args.ckpt is None and not args.synthetic_weights and not no_proc:
        ap.error("a checkpoint (or --synthetic-weights NF) is required")
    if args.bss_eval and not 1 <= args.bss_filter_length <= 1024:
        ap.error("--bss-filter-length: 1..1024 taps")
    for flag, on in (("--fig", args.fig), ("--trajectory", args.trajectory)):
        if on and args.sampler == "ode":
            raise SystemExit(f"{flag}: the ODE sampler has no fixed reverse steps to look at (--sampler pc)")
        if on and no_proc:
            raise SystemExit(f"{flag}: __no_proc__ scores the mixture itself, there is no sampler to look into")
    if args.sampler != "ode-fixed":
        for flag, on in (("--ode-method", args.ode_method is not None), ("--ode-steps", args.ode_steps is not None),
                         ("--ode-err", args.ode_err)):
            if on:
                raise SystemExit(f"{flag} goes with --sampler ode-fixed")
    else:
        for flag, on in (("--fig", args.fig), ("--trajectory", args.trajectory), ("--draws", args.draws is not None)):
            if on:
                raise SystemExit(f"{flag} with --sampler ode-fixed is not supported in this version")
        if args.ode_steps is not None and args.ode_steps < 1:
            raise SystemExit(f"--ode-steps {args.ode_steps}: at least one step")
        args.ode_method = args.ode_method or "heun"
        if args.ode_err and args.ode_method in _lib.EXPINT_METHODS and args.ode_method not in _lib.EXPINT_ERR_METHODS:
            raise SystemExit(f"--ode-err with --ode-method {args.ode_method}: the first-order method has no lower-order step to "
                             "compare with (dpmpp2m)")
        if args.ode_err and args.ode_method not in _lib.ODEF_ERR_METHODS + _lib.EXPINT_ERR_METHODS:
            raise SystemExit(f"--ode-err with --ode-method {args.ode_method}: the method has no embedded Euler step (heun, midpoint, ab2)")
    if args.draws is None and args.draws_out is not None:
        raise SystemExit("--draws-out goes with --draws")
    if args.draws is not None:
        for flag, on in (("--sampler ode", args.sampler == "ode"), ("__no_proc__", no_proc), ("--fig", args.fig),
                         ("--trajectory", args.trajectory)):
            if on:
                raise SystemExit(f"--draws with {flag} is not supported: the draws are whole runs of the predictor-corrector sampler")
        if not 1 <= args.draws <= 32:
            raise SystemExit(f"--draws {args.draws}: 1 to 32 draws")
        if args.draws > max(1, args.batch):
            raise SystemExit(f"--draws {args.draws} does not fit --batch {args.batch}: an utterance takes one row of an engine "
                             "call per draw")
        args.draws_out = args.draws_out or "mean"
    if args.fig:
        figures.require_matplotlib("--fig")
    if args.streams > 1:
        inflight.default_hw_queues()  # (before the first torch.cuda call)

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    if "LOCAL_RANK" in os.environ:
        local = int(os.environ["LOCAL_RANK"])
    else:  # -d 1 / -d cuda:1 (evaluate.py:177-179)
        d = str(args.device)
        local = int(d.split(":")[1]) if ":" in d else (int(d) if d.isdigit() else 0)
    if not torch.cuda.is_available():
        raise SystemExit("No GPU visible: this build has no CPU path")
    torch.cuda.set_device(local)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    n_workers = max(2, min(os.cpu_count() or 2, 16) if args.dl_workers is None else args.dl_workers)

    model = None
    if not no_proc:
        if args.synthetic_weights or args.ckpt is None:
            cfg = (enhancement_config(nf=args.synthetic_weights or 128) if args.enhance
                   else default_config(nf=args.synthetic_weights or 64, n_speakers=args.n_speakers))
            model = DiffSepModel(cfg, dtype=args.dtype, head_steps=args.fp32_steps)
        else:
            model = DiffSepModel.load_from_checkpoint(args.ckpt, dtype=args.dtype, head_steps=args.fp32_steps)
        model.eval()
    models, streams = inflight.setup_workers(model, max(1, args.streams))  # (__no_proc__: no models, streams only)
    fs_model = cfg_get(model.config, "model.fs", 8000) if model is not None else None
    N, cs, snr = inflight.sampler_settings(model.config, args) if model is not None else (None, None, None)
    if args.composite and fs_model is not None and int(fs_model) not in metrics.COMPOSITE_RATES:
        ap.error(f"--composite: the model's sample rate {fs_model} is not one of {metrics.COMPOSITE_RATES}")

    # ---- the output folder (evaluate.py:257-262,306-323)
    if args.flat_output:
        output_dir = args.output_dir
    elif no_proc:
        output_dir = args.output_dir / ("mix" if args.tag is None else args.tag)
    else:
        tag_inf = f"N-{N}_snr-{snr}_corrstep-{cs}_denoise-{args.denoise}_schedule-{args.schedule}"
        if args.sampler == "ode":
            tag_inf += f"_sampler-ode_rtol-{args.rtol}_atol-{args.atol}"
        if args.sampler == "ode-fixed":
            tag_inf += f"_sampler-ode-fixed_method-{args.ode_method}_steps-{args.ode_steps or N}"
        if args.tag is not None:
            output_dir = args.output_dir / f"{args.tag}_{tag_inf}"
        elif args.ckpt is not None and not args.synthetic_weights:
            output_dir = args.output_dir / f"{Path(args.ckpt).absolute().parents[1].name}_{Path(args.ckpt).stem}_{tag_inf}"
        else:
            output_dir = args.output_dir / f"synthetic-nf{args.synthetic_weights}_random-init_{tag_inf}"
    if rank == 0:
        output_dir.mkdir(exist_ok=True, parents=True)
        print(f"Created output folder {output_dir}")

    # ---- the data sets, one per split (evaluate.py:245-288)
    from_hparams = None
    if not (args.synthetic or args.dataset_dir):
        if no_proc:  # evaluate.py:247-255
            from_hparams = {s: datasets.WSJ0_mix(path="data/wsj0_mix", n_spkr=2, cut="max", split=s) for s in splits}
        else:
            from_hparams = _hparams_datasets(args, fs_model, splits)

    # the reference's DataLoader has worker processes; here loader threads read / synthesise and pad the next batches while the
    # GPU separates the current ones (wav decoding and numpy release the GIL), and score STOI of the finished ones
    loader = ThreadPoolExecutor(max_workers=n_workers)
    common = dict(args=args, models=models, streams=streams, loader=loader, sampler_kw=dict(N=N, corrector_steps=cs, snr=snr),
                  output_dir=output_dir, rank=rank, world=world)
    for split in splits:
        if from_hparams is not None:
            ds = from_hparams[split]
            n = len(ds) if args.limit is None else min(len(ds), args.limit)
            get, lengths = (lambda i, ds=ds: tuple(t[..., : ds.num_samples(i)] for t in ds[i])), [ds.num_samples(i) for i in range(n)]
            fs = ds.fs
        else:
            args_split = argparse.Namespace(**{**vars(args), "split": split})
            fs = fs_model if fs_model is not None else 8000
            n, get, lengths = load_dataset(args_split, fs)
        if args.composite and int(fs) not in metrics.COMPOSITE_RATES:
            ap.error(f"--composite: the sample rate {fs} of {split} is not one of {metrics.COMPOSITE_RATES}")
        run_split(SplitRun(**common, split=split, fs=fs, n=n, get=get, lengths=lengths))
    loader.shutdown()
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    return output_dir


# One engine call in flight: what collect needs (utterance indices, their lengths in samples, ..., t0 = host time at which the
# sampler was enqueued, None when nothing was separated) and every tensor the asynchronous sampler reads (they stay referenced
# until the worker's stream has drained).
# draws (--draws): (ops.EnsembleResult, aligned draws [B,K,S,T]) of the call.
_Batch = namedtuple("_Batch", "group lens mix mix_n tgt_n est nfe t0 sampler sloss draws", defaults=(None, None))


@dataclass
class SplitRun:
    """One split on one rank: what main() set up, the split's data, the rank's plan, and what the batches leave behind."""
    args: argparse.Namespace
    models: list   # one per stream (none with __no_proc__: the mixture itself is scored)
    streams: list
    loader: ThreadPoolExecutor
    sampler_kw: dict  # N, corrector_steps, snr
    output_dir: Path
    rank: int
    world: int
    split: str
    fs: int
    n: int  # utterances of the split; get(i) -> (mix [1,T], tgt [S,T]) CPU tensors; lengths in samples
    get: Callable
    lengths: list
    records: list = field(default_factory=list)
    stoi_jobs: list = field(default_factory=list)  # (record, future of the per-source STOI list)
    fallbacks: list = field(default_factory=list)  # batches repeated on the split-precision engine after non-finite f16 samples
    ahead: dict = field(default_factory=dict)  # batch number -> future of its host_stage()
    ode_reruns: dict = field(default_factory=dict)  # first utterance of a repeated ODE batch -> the repeat's per-utterance infos
    trace_reruns: dict = field(default_factory=dict)  # first utterance of a repeated traced batch -> the repeat's trace
    fixed_reruns: dict = field(default_factory=dict)  # first utterance of a repeated ode-fixed batch -> the repeat's info

    def __post_init__(self):
        a = self.args
        self.no_proc = not self.models
        self.n_src = 1 if a.enhance else None  # (evaluate.py:268-271)
        if self.no_proc:
            self.width_of = lambda T: 64 * ((1 + (T + 382) // 128 + 63) // 64)
            self.bucket = lambda W: 128 * W - 383
        else:
            eng0 = self.models[0].score_model.engine()
            self.width_of, self.bucket = eng0.padded_frames, eng0.bucket_length
        # the reference's contiguous ranges (evaluate_mp.py:495-503), or sorted by length and dealt round-robin
        self.mine = rank_indices(self.n, self.world, self.rank, self.lengths, a.balance)
        self.draws = getattr(a, "draws", None) or 0  # --draws K: an utterance takes K rows of an engine call
        self.batches = inflight.plan_draw_batches(self.mine, self.lengths, self.width_of, max(1, a.batch), max(1, self.draws))
        self.seeds = inflight.utterance_seeds(self.n, a.seed)
        # --fig: the unique steps of the figure's panels (what the tap is asked for) and each panel's place among them
        self.fig_steps, self.fig_panels = figures.snapshot_request(self.sampler_kw["N"]) if a.fig else (None, None)

    def wants_fig(self, i):
        """is utterance i one of those --fig draws (the ones --save-n saves)?"""
        return self.args.fig and (self.args.save_n is None or i < self.args.save_n)

    def host_stage(self, group):
        """load and pad one batch on the host (runs on a loader thread, ahead of the GPU): mix / tgt + lengths"""
        items = [self.get(i) for i in group]
        # padded to the longest length of the batch's width bucket: one workspace plan / captured graph per (B, W)
        mix, tgt, lens = datasets.pad_batch(items, side="right",
                                            to=self.bucket(self.width_of(max(self.lengths[i] for i in group))))
        return mix.contiguous(), tgt.contiguous(), lens

    def prefetch(self, j):
        for jj in range(j, min(j + 2 * len(self.streams) + 2, len(self.batches))):
            if jj not in self.ahead:
                self.ahead[jj] = self.loader.submit(self.host_stage, self.batches[jj])

    def stage(self, w, j, group):
        """upload and normalise one batch on the current (worker w's) stream -> (mix, mix_n, tgt_n, lens)"""
        mix, tgt, lens = self.ahead.pop(j).result() if j in self.ahead else self.host_stage(group)
        mix, tgt = inflight.upload(mix), inflight.upload(tgt)
        if self.no_proc:  # (evaluate.py:349-355: the raw mixture against the raw targets)
            return mix, mix, tgt, lens
        return (mix, *inflight.normalize_padded(self.models[w], lens, mix, tgt), lens)

    def sampler_for(self, model, group, lens, mix_n, tgt_n=None, trace=True):
        """trace: ask the sampler's tap for what --fig (snapshots, in the batches that hold such an utterance) and
        --trajectory (Gram sums against tgt_n) need; False for a warm-up call"""
        if self.args.sampler == "ode":  # one step controller per utterance; sampler.info: the utterances' own counts
            a = self.args
            return model.get_ode_sampler(mix_n, N=self.sampler_kw["N"], denoise=a.denoise, rtol=a.rtol, atol=a.atol,
                                         max_nfe=a.max_nfe, lengths=lens, seeds=[self.seeds[i] for i in group])
        if self.args.sampler == "ode-fixed":  # a fixed grid: enqueued like the PC call; sampler.info: nfe, method, steps[, err]
            a = self.args
            return model.get_ode_fixed_sampler(mix_n, N=self.sampler_kw["N"], denoise=a.denoise, method=a.ode_method,
                                               steps=a.ode_steps, schedule=a.schedule, lengths=lens,
                                               seeds=[self.seeds[i] for i in group], want_err=a.ode_err, check_finite=False)
        tap = {}
        if trace and any(self.wants_fig(i) for i in group):
            tap["snapshots"] = self.fig_steps
        if trace and self.args.trajectory:
            tap["target"] = tgt_n
        return model.get_pc_sampler("reverse_diffusion", "ald2", mix_n, **self.sampler_kw, denoise=self.args.denoise,
                                    intermediate=False, schedule=self.args.schedule, lengths=lens,
                                    seeds=[self.seeds[i] for i in group], check_finite=False, **tap)

    def score_loss(self, model, group, lens, mix_n, tgt_n):
        """mean over K times of the plain score-matching loss of every utterance of the batch -> float64 [B] device tensor,
        enqueued on the current stream (diffsep_score_loss with lengths: a row does not depend on the batch it rides in)"""
        K = self.args.score_loss
        B, S, T = tgt_n.shape
        seeds = [self.seeds[i] for i in group]
        eng, sde = model.score_model.engine(), model.sde.engine_config()
        total = torch.zeros(B, dtype=torch.float64, device=tgt_n.device)
        for k, t in enumerate(torch.linspace(float(model.t_eps), float(model.sde.T), K).tolist()):
            # (stream ids from 2^32: the sampler's own draws of these seeds count up from 0)
            z = ops.randn_batch(B, S, T, seeds, lens, (1 << 32) + k, device=tgt_n.device)
            out, _, _ = ops.score_loss(eng, sde, mix_n, tgt_n, torch.full((B,), t, dtype=torch.float32, device=tgt_n.device),
                                       z=z, lengths=lens)
            total += out[:, 0]
        return total / K

    def launch(self, w, j, group):
        """enqueue batch j (None: a warm-up call, nothing was prefetched for it) on the current (worker w's) stream"""
        if j is not None:
            self.prefetch(j)
        mix, mix_n, tgt_n, lens = self.stage(w, j, group)
        if self.no_proc:
            est = mix_n.expand(-1, tgt_n.shape[1], -1).contiguous()  # x_result = broadcast_to(mix, target.shape)
            return _Batch(group, lens, mix, mix_n, tgt_n, est, 0, None, None)
        sloss = self.score_loss(self.models[w], group, lens, mix_n, tgt_n) if self.args.score_loss > 0 else None
        if self.draws:
            if len(self.streams) == 1:
                torch.cuda.synchronize()
            t0 = time.perf_counter()  # (the runtime covers all K draws and their reduction)
            _, est, nfe, extra = self.draw(self.models[w], group, lens, mix)
            return _Batch(group, lens, mix, mix_n, tgt_n, est, nfe, t0, None, sloss, extra)
        sampler = self.sampler_for(self.models[w], group, lens, mix_n, tgt_n, trace=j is not None)
        if len(self.streams) == 1:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        est, nfe, *_ = sampler()  # enqueues the whole sampler on the worker's stream
        return _Batch(group, lens, mix, mix_n, tgt_n, est, nfe, t0, sampler, sloss)

    def draw(self, model, group, lens, mix):
        """--draws: K draws of every utterance of the batch in ONE engine call, aligned and reduced on the current stream
        (DiffSepModel.separate_draws on the raw mixture: it normalises per utterance as stage() does, and the identity in place
        of the rescaling keeps the draws in the normalised domain the metrics are taken in)
        -> (mean of the draws, the estimate --draws-out names [B,S,T], nfe, (ops.EnsembleResult, aligned draws [B,K,S,T])).
        The mean comes first because it is what the overflow net looks at: a non-finite sample of any draw is a non-finite
        sample of their mean."""
        a = self.args
        mean, res, aligned = model.separate_draws(mix, self.draws, lengths=lens, seeds=[self.seeds[i] for i in group], out="all",
                                                  rescale=lambda mix_f, rows: rows, check_finite=False, **self.sampler_kw,
                                                  denoise=a.denoise, intermediate=False, schedule=a.schedule)
        return mean, (res.pick if a.draws_out == "medoid" else mean), model.draws_info["nfe"], (res, aligned)

    def draw_fields(self, b, extra, stream):
        """per utterance of batch b the record fields of --draws: SI-SDR of every aligned draw, of the mean and of the medoid,
        each under its own best permutation against the target (ONE diffsep_gram call over all of them), the medoid's index
        and every draw's squared distance to the mean"""
        res, aligned = extra
        B, K = aligned.shape[:2]
        with torch.cuda.stream(stream):
            cand = torch.cat([aligned.reshape(B * K, *aligned.shape[2:]), res.mean, res.pick])
            refs = torch.cat([b.tgt_n.repeat_interleave(K, dim=0), b.tgt_n, b.tgt_n])
            sdr = metrics.si_bss_eval_sources(refs, cand)[0]
            dist, medoid = metrics.gram_to_host(res.dist), metrics.gram_to_host(res.medoid)
        k_src = sdr.shape[1] if self.n_src is None else self.n_src
        row = lambda r: [float(v) for v in sdr[r, :k_src]]
        return [{"si_sdr_draws": [row(u * K + k) for k in range(K)], "si_sdr_mean": row(B * K + u),
                 "si_sdr_medoid": row(B * K + B + u), "draws_medoid": int(medoid[u]), "draws_dist": [float(v) for v in dist[u]]}
                for u in range(B)]

    def reissue(self, fb, b):
        """the same request on the fallback model: the same trace arguments, and the repeat's trace replaces the first"""
        self.fallbacks.append(list(b.group))
        if self.draws:
            return self.draw(fb, b.group, b.lens, b.mix)
        traced = getattr(b.sampler, "trace", None) is not None
        sampler = self.sampler_for(fb, b.group, b.lens, b.mix_n, b.tgt_n, trace=traced)
        out = sampler()
        if self.args.sampler == "ode":
            self.ode_reruns[b.group[0]] = sampler.info
        elif self.args.sampler == "ode-fixed":
            self.fixed_reruns[b.group[0]] = sampler.info
        elif traced:
            self.trace_reruns[b.group[0]] = sampler.trace
        return out

    def collect(self, w, b):
        """batch b, whose sampler has drained from worker w's stream, into records (+ STOI jobs, saved samples)"""
        a, stream, (group, lens, tgt_n, est, nfe) = self.args, self.streams[w], (b.group, b.lens, b.tgt_n, b.est, b.nfe)
        extra = b.draws
        if self.draws:
            _, est, nfe, extra = inflight.finite_or_rerun(self.models[w], stream, (extra[0].mean, est, nfe, extra),
                                                          lambda fb: self.reissue(fb, b), what=f"utterances {group[:3]}...")
        elif not self.no_proc:
            est, nfe, *_ = inflight.finite_or_rerun(self.models[w], stream, (est, nfe), lambda fb: self.reissue(fb, b),
                                                    what=f"utterances {group[:3]}...")
        runtime = 0.0 if b.t0 is None else (time.perf_counter() - b.t0) / len(group)
        ode = None  # --sampler ode: the utterances' own solver counts
        if not self.no_proc and a.sampler == "ode":
            ode = self.ode_reruns.pop(group[0], None) or b.sampler.info
        fixed_err = None  # --sampler ode-fixed --ode-err: per utterance max over the steps of err / rms(y), one read per batch
        if not self.no_proc and a.sampler == "ode-fixed" and a.ode_err:
            info = self.fixed_reruns.pop(group[0], None) or b.sampler.info
            with torch.cuda.stream(stream):
                fixed_err = (info["err"][:, :, 0] / info["err"][:, :, 1]).amax(dim=0).cpu().tolist()
        with torch.cuda.stream(stream):
            mets = compute_metrics(est, tgt_n, self.n_src)
        trace = None  # what the sampler's tap left (--fig, --trajectory; none for a warm-up call)
        if not self.no_proc and a.sampler == "pc":
            trace = self.trace_reruns.pop(group[0], None) or getattr(b.sampler, "trace", None)
        steps_sdr = None
        if trace is not None and trace.gram is not None:  # [N+1,B,3,S,S] -> per step the SI-SDR under the FINAL permutation
            with torch.cuda.stream(stream):
                G = metrics.gram_to_host(trace.gram)
            perms = [m["perm"] for m in mets]
            steps_sdr = [metrics.si_bss_from_gram(G[i], perm=perms)[0] for i in range(G.shape[0])]
        dfields = self.draw_fields(b, extra, stream) if self.draws else None
        need_host = needs_host_waveforms(a, group)
        stoi_dev = None
        if not a.no_stoi and a.stoi_on == "device":  # every source against its permuted estimate, whole batch at once
            with torch.cuda.stream(stream):
                stoi_dev = metrics.stoi_batch(tgt_n, est, self.fs, extended=not a.stoi_no_extended, lengths=lens,
                                              perm=[m["perm"] for m in mets])
        comp_dev = None
        if a.composite:  # LLR / WSS / segmental SNR of every source against its permuted estimate: 4 B S numbers cross PCIe
            with torch.cuda.stream(stream):
                comp_dev = metrics.composite_batch(tgt_n, est, self.fs, lengths=lens, perm=[m["perm"] for m in mets])
        bss_dev = None
        if a.bss_eval:  # SDR / SIR / SAR of every source against its permuted estimate: 3 B S numbers cross PCIe
            with torch.cuda.stream(stream):
                bss_dev = metrics.bss_eval_batch(tgt_n, est, a.bss_filter_length, clamp_db=100.0, lengths=lens,
                                                 perm=[m["perm"] for m in mets])
        if need_host:
            with torch.cuda.stream(stream):
                est_h, tgt_h, mix_h = est.cpu(), tgt_n.cpu(), b.mix_n.cpu()
        sloss = None
        if b.sloss is not None:
            with torch.cuda.stream(stream):
                sloss = b.sloss.cpu().tolist()
        for k, i in enumerate(group):
            rec = {"batch_idx": i, **mets[k], "pesq": None, "stoi": None, "nfe": int(nfe if ode is None else ode[k]["nfev"]),
                   "runtime": runtime, "len_s": lens[k] / self.fs}
            if ode is not None:
                rec["ode_status"] = int(ode[k]["status"])
            if fixed_err is not None:
                rec["ode_local_err"] = float(fixed_err[k])
            if sloss is not None:
                rec["score_loss"] = float(sloss[k])
            if dfields is not None:
                rec.update(dfields[k])
            self.records.append(rec)
            perm = mets[k]["perm"]
            k_src = len(perm) if self.n_src is None else self.n_src
            if steps_sdr is not None:
                rec["si_sdr_steps"] = [[float(v) for v in row[k, :k_src]] for row in steps_sdr]
            if trace is not None and trace.x.shape[0] and self.wants_fig(i):
                with torch.cuda.stream(stream):  # this utterance's snapshots [steps,S,L], sources in the targets' order
                    snaps = trace.x[:, k][:, perm, :lens[k]].cpu().numpy()
                    clean = tgt_n[k, :, :lens[k]].cpu().numpy()
                fig_dir = self.output_dir / "fig" / self.split
                fig_dir.mkdir(parents=True, exist_ok=True)
                figures.evolution_figure(snaps[self.fig_panels], [self.fig_steps[p] for p in self.fig_panels],
                                         self.sampler_kw["N"], clean, fig_dir / f"evo_{i:03d}.pdf")
            if stoi_dev is not None:
                rec["stoi"] = [float(v) for v in stoi_dev[k, :k_src]]
            if comp_dev is not None:
                for q, name in enumerate(("llr", "wss", "segsnr")):
                    rec[name] = [float(v) for v in comp_dev[k, :k_src, q]]
                rec.update({"csig": None, "cbak": None, "covl": None})  # (they need PESQ)
            if bss_dev is not None:
                for q, name in enumerate(("sdr", "sir", "sar")):
                    rec[name] = [float(v) for v in bss_dev[k, q, :k_src]]
            if need_host:
                est_k = est_h[k, perm, :lens[k]]  # "fix the permutation" (evaluate.py:392): estimates in the targets' order
                if not a.no_stoi and a.stoi_on == "host":
                    self.stoi_jobs.append((rec, self.loader.submit(_stoi_rows, tgt_h[k, :k_src, :lens[k]].numpy(),
                                                                   est_k[:k_src].numpy(), self.fs, not a.stoi_no_extended)))
                if a.save_n is None or i < a.save_n:  # (evaluate.py:341; figures are not produced)
                    save_samples(mix_h[k, :, :lens[k]], est_k, tgt_h[k, :, :lens[k]], self.output_dir / "wav" / self.split, i, self.fs)

    def write_results(self, allrec, wall):
        """rank 0: <split>.json (every rank's records, by utterance) and <split>_summary.json; wall: this rank's timed region"""
        a, model = self.args, self.models[0] if self.models else None
        flat = sorted([r for part in allrec for r in part], key=lambda r: r["batch_idx"])
        with open(self.output_dir / f"{self.split}.json", "w") as f:
            json.dump(flat, f, indent=2)
        summary = datasets.summarize([{k: v for k, v in r.items() if k not in ("batch_idx", "perm", "ode_status", "si_sdr_steps", "draws_medoid")}
                                      for r in flat])
        if a.trajectory and flat:  # per reverse step (and last the result): the mean over the utterances, per source
            import numpy as np
            summary["si_sdr_steps"] = np.mean([r["si_sdr_steps"] for r in flat], axis=0).tolist()
        tot_rt = sum(r["runtime"] for r in flat)
        summary.update({"rtf": tot_rt / max(sum(r["len_s"] for r in flat), 1e-9), "world_size": self.world,
                        "streams": len(self.streams), "batch": a.batch, "engine_calls_rank0": len(self.batches),
                        "dtype": model.dtype if model is not None else None,
                        "sampler": None if model is None else a.sampler,
                        **({"draws": self.draws, "draws_out": a.draws_out} if self.draws else {}),
                        **({"bss_filter_length": a.bss_filter_length} if a.bss_eval else {}),
                        "utt_per_s_rank0": len(self.mine) / max(wall, 1e-9), "split_fallback_batches_rank0": len(self.fallbacks),
                        # PESQ is ITU-T P.862 reference C code behind the third-party `pesq` package: not restated here
                        # (DESIGN.md section 7); STOI / ESTOI is diffsep_amd.metrics.stoi (published algorithm, restated)
                        "not_computed": ["pesq"] + (["stoi"] if a.no_stoi else []) + (["csig", "cbak", "covl"] if a.composite else []),
                        "stoi_on": a.stoi_on, "stoi_extended": not a.stoi_no_extended, "pesq_mode": a.pesq_mode})
        if model is not None and a.sampler == "ode-fixed":
            summary.update({"ode_method": a.ode_method, "ode_steps": int(a.ode_steps or self.sampler_kw["N"])})
        if model is not None and a.sampler == "ode":
            summary["ode_status_counts"] = {str(c): sum(1 for r in flat if r.get("ode_status") == c) for c in (0, -1, 1)}
        with open(self.output_dir / f"{self.split}_summary.json", "w") as f:
            json.dump(summary, f, indent=2)
        print(json.dumps(summary))


def _stoi_rows(tgt_rows, est_rows, fs, extended):
    return [metrics.stoi(t_, e_, fs, extended=extended) for t_, e_ in zip(tgt_rows, est_rows)]


def run_split(run):
    if run.rank == 0:
        print(f"Processing {run.split}: {run.n} samples")
    inflight.reserve_largest(run.models, run.batches, run.lengths, rows_per_item=max(1, run.draws))
    # warm every worker up on the first batch's shape (workspace plan, graph capture) outside the timed region
    if run.batches and not run.no_proc:
        for w, stream in enumerate(run.streams):
            with torch.cuda.stream(stream):
                run.launch(w, None, run.batches[0])
        torch.cuda.synchronize()
    t_all = time.perf_counter()
    run.prefetch(0)
    inflight.Ring(run.streams, run.launch, run.collect).run(run.batches)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t_all
    for rec, fut in run.stoi_jobs:
        rec["stoi"] = fut.result()
    allrec = gather_objects(run.records)
    if run.rank == 0:
        run.write_results(allrec, wall)


if __name__ == "__main__":
    main()
