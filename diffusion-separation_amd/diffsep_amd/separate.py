"""separate.py — same command line as the reference's separate.py:102-162:

    python -m diffsep_amd.separate input_dir output_dir [--model CKPT] [-d cuda:0] [-N 30] [--snr 0.5]
           [--corrector-steps 1] [--denoise True] [-s SCHEDULE]

For every *.wav in input_dir: load -> normalize_batch -> reverse-diffusion PC sampler on the HIP engine ->
scale_output -> write output_dir/s{i}/name.wav (directories s0, s1 like separate.py:157-158).
Additions: --synthetic-weights NF runs with random-init weights of width NF when no checkpoint is
available (there is no network here: the HF default 'fakufaku/diffsep' cannot be downloaded), --dtype (bf16 / f32 /
hybrid), --batch B: files whose padded spectrogram width is equal share one engine call (zero-padded to the longest,
each file's tail kept at zero by the engine: the docstring of evaluate.py has the details), --streams K engine calls
in flight on K engines / HIP streams (planning, worker set-up, workspace reserve, the launch / collect ring and the
overflow re-run are inflight.py's, shared with evaluate), and --seed (file i of the sorted folder then gets the i-th
draw of that generator as its device RNG seed: the written files do not depend on --batch or --streams), and --chunk SECONDS [--overlap SECONDS]: a file longer than the chunk is
cut into windows of that length (ops.longform_plan; the overlap defaults to an eighth of the chunk), the windows of all files are
what --batch groups and --streams keeps in flight, and a file is stitched on the device (ops.longform_stitch: source orders
aligned over the overlaps, seams cross-faded) and written when its last window has been collected; a file
no longer than the chunk is handled as without --chunk.  --sampler ode [--rtol --atol --max-nfe] runs the
probability-flow ODE sampler (sdes.get_ode_sampler, adaptive RK45 on the device) instead of the PC sampler.  With
--batch 1 a file is one engine call; with --batch K > 1 the files of a batch (the same plan as the PC path) share every
network evaluation while each keeps its own step controller (diffsep_ode_sample_each), so with --dtype f32 the written
files are those of --batch 1, bit for bit wherever the network evaluation does not depend on the batch.  --streams stays 1 there: the ODE driver blocks on a readback per step
attempt.  Output files are 32-bit float WAV like torchaudio.save of a float tensor (separate.py:160-162).
"""
import argparse
from pathlib import Path

import torch

from . import datasets, inflight, ops, wavio
from .pl_model import DiffSepModel, cfg_get, default_config

DEFAULT_MODEL = "fakufaku/diffsep"


def get_model(args):
    if args.synthetic_weights:
        model = DiffSepModel(default_config(nf=args.synthetic_weights), dtype=args.dtype, device=args.device,
                             head_steps=getattr(args, "fp32_steps", None))
    else:
        path = Path(args.model)
        if not path.exists():
            raise FileNotFoundError(f"checkpoint '{args.model}' not found (Hugging Face download needs network access; "
                                    "pass a local Lightning checkpoint or --synthetic-weights NF)")
        model = DiffSepModel.load_from_checkpoint(str(path), dtype=args.dtype, device=args.device,
                                                  head_steps=getattr(args, "fp32_steps", None))
    model.to(args.device)
    model.eval()
    N, cs, snr = inflight.sampler_settings(model.config, args)
    kwargs = {"N": N, "denoise": args.denoise, "intermediate": False, "corrector_steps": cs, "snr": snr,
              "schedule": args.schedule}
    return model, kwargs


def scale_output(mix, sep):
    """separate.py:73-78, in the HIP kernel."""
    return ops.scale_output(mix.contiguous(), sep.contiguous())


def separate_on_device(mix, model, sampler_kwargs, device, lengths=None, seeds=None, check_finite=False):
    """Enqueue the separation of mix [1,T] / [B,1,T] on the current stream; returns the device tensor [B,S,T].
    lengths [B]: mix is a right-zero-padded batch of files of those lengths (normalised and rescaled per file)."""
    mix = mix.to(device)
    if mix.dim() == 2:
        mix = mix[None]
    if lengths is None:
        (mix_norm, _), *_ = model.normalize_batch((mix, None))
    else:
        mix_norm, _ = inflight.normalize_padded(model, lengths, mix)
    extra = {} if lengths is None else {"lengths": list(lengths)}
    if seeds is not None:
        extra["seeds"] = list(seeds)
    # (check_finite=False: the callers below collect the result later and run the model's overflow net then)
    sampler = model.get_pc_sampler("reverse_diffusion", "ald2", mix_norm, check_finite=check_finite, **sampler_kwargs, **extra)
    with torch.no_grad():
        sep, nfe, *_ = sampler()
    if lengths is None:
        return scale_output(mix, sep)
    out = torch.zeros_like(sep)
    for b, L in enumerate(lengths):  # the least-squares scale of separate.py:73-78 is per file, over ITS samples
        out[b, :, :L] = scale_output(mix[b:b + 1, :, :L], sep[b:b + 1, :, :L])[0]
    return out


def separate_ode(mix, model, ode_kwargs, device, seed=None):
    """mix [1,T] / [B,1,T] through the probability-flow ODE sampler (DiffSepModel.get_ode_sampler); the same
    normalisation and output scaling as the PC path.  Returns (device tensor [B,S,T], nfe)."""
    mix = mix.to(device)
    if mix.dim() == 2:
        mix = mix[None]
    (mix_norm, _), *_ = model.normalize_batch((mix, None))
    kw = dict(ode_kwargs)
    if seed is not None:
        kw["seed"] = seed
    sep, nfe = model.get_ode_sampler(mix_norm, **kw)()
    return scale_output(mix, sep), nfe


def separate_ode_batch(mix, model, ode_kwargs, device, lengths, seeds=None):
    """mix [B,1,T], a right-zero-padded batch of files of those lengths, through the ODE sampler with one step controller
    per file (get_ode_sampler(lengths=, seeds=)); normalised and rescaled per file.  Returns (device tensor [B,S,T] with
    zero tails, the files' info dicts)."""
    mix = mix.to(device)
    mix_norm, _ = inflight.normalize_padded(model, lengths, mix)
    sampler = model.get_ode_sampler(mix_norm, lengths=list(lengths), seeds=None if seeds is None else list(seeds),
                                    per_utterance=True, **ode_kwargs)
    sep, _ = sampler()
    out = torch.zeros_like(sep)
    for b, L in enumerate(lengths):
        out[b, :, :L] = scale_output(mix[b:b + 1, :, :L], sep[b:b + 1, :, :L])[0]
    return out, sampler.info


def separate(mix, model, sampler_kwargs, device):
    """mix [1,T] (one file, like the reference) or [B,1,T] (a batch of equal-length files)."""
    return separate_on_device(mix, model, sampler_kwargs, device, check_finite=True).cpu()


def chunk_samples(args, fs):
    """(window, overlap) of --chunk / --overlap in samples at the model's rate, or SystemExit for a refused request"""
    window = int(round(args.chunk * fs))
    overlap = int(round((args.chunk / 8 if args.overlap is None else args.overlap) * fs))
    if window < 3:
        raise SystemExit(f"--chunk {args.chunk}: a window of {window} samples is too short")
    if overlap < 1:
        raise SystemExit(f"--overlap: an overlap of {overlap} samples is too short (at least one sample)")
    if 3 * overlap > window:
        raise SystemExit(f"--overlap {overlap / fs:g} s is more than a third of --chunk {args.chunk:g} s: the seams of "
                         "neighbouring windows would intersect")
    return window, overlap


def separate_chunked(args, files, lengths, seeds, models, streams, kw, model_sr):
    """--chunk: the windows of all files (file-major) are the items of the batches in flight; window results stay on the device
    until their file's last one has been collected, then the file is stitched there and written."""
    window, overlap = chunk_samples(args, model_sr)
    eng = models[0].score_model.engine()
    items, item_lengths, starts = inflight.plan_windows(lengths, window, overlap, ops.longform_plan)
    if seeds is None:  # one draw of torch's generator per file, as a file without --seed gets one per engine call
        seeds = [int(torch.randint(0, 2 ** 62, (1,)).item()) for _ in files]
    wseeds = [inflight.window_seeds(seeds[i], len(starts[i])) for i in range(len(files))]
    batches = inflight.plan_batches(range(len(items)), item_lengths, eng.padded_frames, max(1, args.batch))
    inflight.reserve_largest(models, batches, item_lengths)
    wavs, done = {}, {}  # per file: (samples, rate) while windows of it are still to be launched; collected windows by index

    def load(i):
        if i not in wavs:
            wav, sr = wavio.load(files[i])
            if sr != model_sr:  # the reference only warns (separate.py:151-155, quirk Q9)
                print(f"Warning: {files[i].stem}: this model expects {model_sr} Hz, but the file is {sr} Hz.")
            wavs[i] = (wav[:1], sr, len(starts[i]))
        wav, sr, left = wavs[i]
        wavs[i] = (wav, sr, left - 1)
        if left == 1:
            del wavs[i]
        return wav, sr

    def launch(w, j, group):
        parts, srs = [], []
        for n in group:
            i, k = items[n]
            wav, sr = load(i)
            seg = wav[:, starts[i][k]:starts[i][k] + item_lengths[n]]
            parts.append((seg, seg))
            srs.append(sr)
        mix, _, lens = datasets.pad_batch(parts, side="right",
                                          to=eng.bucket_length(eng.padded_frames(max(item_lengths[n] for n in group))))
        sds = [wseeds[items[n][0]][items[n][1]] for n in group]
        mix_d = inflight.upload(mix, args.device)
        sep = separate_on_device(mix_d, models[w], kw, args.device, lengths=lens, seeds=sds)
        return group, lens, srs, sep, mix_d, sds

    def collect(w, item):
        group, lens, srs, sep, mix_d, sds = item
        sep = inflight.finite_or_rerun(
            models[w], streams[w], (sep,),
            lambda fb: (separate_on_device(mix_d, fb, kw, args.device, lengths=lens, seeds=sds),),
            what=str([f"{files[items[n][0]].name}[{items[n][1]}]" for n in group]))[0]
        for b, n in enumerate(group):
            i, k = items[n]
            got = done.setdefault(i, {})
            got[k] = sep[b, :, :lens[b]]
            if len(got) < len(starts[i]):
                continue
            # every window of file i has been collected, i.e. its stream has drained: stitch on this worker's stream
            with torch.cuda.stream(streams[w]):
                if len(got) == 1:
                    out = got[0]
                else:
                    out, _ = ops.longform_stitch(torch.stack([got[q] for q in range(len(got))]), lengths[i], overlap)
                out = out.cpu()
            del done[i]
            for q in range(out.shape[0]):
                d = args.output_dir / f"s{q}"
                d.mkdir(parents=True, exist_ok=True)
                wavio.save(d / f"{files[i].stem}.wav", out[q:q + 1], srs[b], bits=32)

    inflight.Ring(streams, launch, collect).run(batches)
    print(f"separated {len(files)} files into {args.output_dir} ({len(items)} windows of up to {window} samples)")


def main(argv=None):
    ap = argparse.ArgumentParser(description="Separate all the wav files in a specified folder")
    ap.add_argument("input_dir", type=Path)
    ap.add_argument("output_dir", type=Path)
    ap.add_argument("--model", type=str, default=DEFAULT_MODEL, help="Path to a Lightning checkpoint")
    ap.add_argument("-d", "--device", type=str, default="cuda:0")
    ap.add_argument("-N", type=int, default=None, help="Number of steps")
    ap.add_argument("--snr", type=float, default=None, help="Step size of corrector")
    ap.add_argument("--corrector-steps", type=int, default=None)
    ap.add_argument("--denoise", type=bool, default=True)
    ap.add_argument("-s", "--schedule", type=str, default=None)
    ap.add_argument("--synthetic-weights", type=int, default=0, metavar="NF")
    inflight.add_precision_arguments(ap)  # --dtype, --fp32-steps
    ap.add_argument("--batch", type=int, default=1, help="files per engine call (equal padded width)")
    ap.add_argument("--streams", type=int, default=1, help="engine calls in flight: K engines on K HIP streams")
    ap.add_argument("--seed", type=int, default=None,
                    help="file i (sorted) gets the i-th draw of a generator with this seed as its device RNG seed")
    ap.add_argument("--sampler", default="pc", choices=["pc", "ode"],
                    help="pc (default): the reference's predictor-corrector sampler; ode: the probability-flow ODE "
                         "(adaptive RK45, sdes.get_ode_sampler); with --batch K the files of a batch share the network "
                         "evaluations, each with its own step controller")
    ap.add_argument("--rtol", type=float, default=1e-5, help="--sampler ode: relative tolerance (reference default)")
    ap.add_argument("--atol", type=float, default=1e-5, help="--sampler ode: absolute tolerance (reference default)")
    ap.add_argument("--max-nfe", type=int, default=0,
                    help="--sampler ode: no step attempt starts beyond this many network evaluations (0: unbounded)")
    ap.add_argument("--chunk", type=float, default=None, metavar="SECONDS",
                    help="cut files longer than this into windows of this length (4 = the shape the engine is tuned for), "
                         "separate the windows as the items of --batch / --streams and stitch them on the device")
    ap.add_argument("--overlap", type=float, default=None, metavar="SECONDS",
                    help="with --chunk: overlap of neighbouring windows (default: an eighth of the chunk; at most a third)")
    args = ap.parse_args(argv)
    if args.chunk is None and args.overlap is not None:
        raise SystemExit("--overlap goes with --chunk")
    if args.chunk is not None and args.sampler == "ode":
        raise SystemExit("--chunk runs the predictor-corrector sampler: --sampler ode --chunk is not supported")
    if args.chunk is not None and args.chunk <= 0:
        raise SystemExit("--chunk must be positive")
    if args.overlap is not None and not 0 < 3 * args.overlap <= args.chunk:
        raise SystemExit(f"--overlap {args.overlap:g} s must be positive and at most a third of --chunk {args.chunk:g} s: the "
                         "seams of neighbouring windows would intersect")
    if args.sampler == "ode" and args.streams > 1:
        raise SystemExit("--sampler ode blocks on a readback per step attempt: --streams must be 1 (use --batch)")
    K = max(1, args.streams)
    if K > 1:
        inflight.default_hw_queues()  # (before the first torch.cuda call)
    if not torch.cuda.is_available():
        raise SystemExit("No GPU visible: this build has no CPU path (the reference falls back to CPU here)")
    torch.cuda.set_device(torch.device(args.device))
    model, kw = get_model(args)
    models, streams = inflight.setup_workers(model, K, own_stream=False)  # (K = 1 runs on the current stream)
    model_sr = cfg_get(model.config, "model.fs", 8000)
    if args.output_dir.is_file():
        raise ValueError("Output directory is a file")
    args.output_dir.mkdir(parents=True, exist_ok=True)
    files = sorted(args.input_dir.glob("*.wav"))
    lengths = [wavio.info(p)[1] for p in files]
    seeds = inflight.utterance_seeds(len(files), args.seed) if args.seed is not None else None
    if args.sampler == "ode" and args.batch > 1:
        ode_kw = {"N": kw["N"], "denoise": args.denoise, "rtol": args.rtol, "atol": args.atol, "max_nfe": args.max_nfe}
        eng = model.score_model.engine()
        for group in inflight.plan_batches(range(len(files)), lengths, eng.padded_frames, args.batch):
            items, srs = [], []
            for i in group:
                wav, sr = wavio.load(files[i])
                if sr != model_sr:  # the reference only warns (separate.py:151-155, quirk Q9)
                    print(f"Warning: {files[i].stem}: this model expects {model_sr} Hz, but the file is {sr} Hz.")
                items.append((wav[:1], wav[:1]))
                srs.append(sr)
            mix, _, lens = datasets.pad_batch(items, side="right",
                                              to=eng.bucket_length(eng.padded_frames(max(lengths[i] for i in group))))
            # (files without --seed: one draw of torch's generator per file, as the --batch 1 loop takes them)
            sds = [seeds[i] if seeds is not None else int(torch.randint(0, 2 ** 62, (1,)).item()) for i in group]
            sep, _ = separate_ode_batch(mix, model, ode_kw, args.device, lens, seeds=sds)
            sep = sep.cpu()
            for b, i in enumerate(group):
                for k in range(sep.shape[1]):
                    d = args.output_dir / f"s{k}"
                    d.mkdir(parents=True, exist_ok=True)
                    wavio.save(d / f"{files[i].stem}.wav", sep[b, k:k + 1, :lens[b]], srs[b], bits=32)
        print(f"separated {len(files)} files into {args.output_dir} (probability-flow ODE, {args.batch} files per call)")
        return
    if args.sampler == "ode":
        ode_kw = {"N": kw["N"], "denoise": args.denoise, "rtol": args.rtol, "atol": args.atol, "max_nfe": args.max_nfe}
        for i, f in enumerate(files):
            wav, sr = wavio.load(f)
            if sr != model_sr:  # the reference only warns (separate.py:151-155, quirk Q9)
                print(f"Warning: {f.stem}: this model expects {model_sr} Hz, but the file is {sr} Hz.")
            sep, _ = separate_ode(wav[:1], model, ode_kw, args.device, seed=seeds[i] if seeds is not None else None)
            sep = sep.cpu()
            for k in range(sep.shape[1]):
                d = args.output_dir / f"s{k}"
                d.mkdir(parents=True, exist_ok=True)
                wavio.save(d / f"{f.stem}.wav", sep[0, k:k + 1], sr, bits=32)
        print(f"separated {len(files)} files into {args.output_dir} (probability-flow ODE)")
        return
    if args.chunk is not None:
        return separate_chunked(args, files, lengths, seeds, models, streams, kw, model_sr)
    eng = model.score_model.engine()
    batches = inflight.plan_batches(range(len(files)), lengths, eng.padded_frames, max(1, args.batch))
    inflight.reserve_largest(models, batches, lengths)

    def launch(w, j, group):
        """-> (file indices, lengths, sample rates, device result, and what a repeat of the request needs)"""
        items, srs = [], []
        for i in group:
            wav, sr = wavio.load(files[i])
            if sr != model_sr:  # the reference only warns (separate.py:151-155, quirk Q9)
                print(f"Warning: {files[i].stem}: this model expects {model_sr} Hz, but the file is {sr} Hz.")
            items.append((wav[:1], wav[:1]))
            srs.append(sr)
        mix, _, lens = datasets.pad_batch(items, side="right",
                                          to=eng.bucket_length(eng.padded_frames(max(lengths[i] for i in group))))
        sds = [seeds[i] for i in group] if seeds is not None else None
        mix_d = inflight.upload(mix, args.device)
        sep = separate_on_device(mix_d, models[w], kw, args.device, lengths=lens, seeds=sds)
        return group, lens, srs, sep, mix_d, sds

    def collect(w, item):
        group, lens, srs, sep, mix_d, sds = item
        sep = inflight.finite_or_rerun(
            models[w], streams[w], (sep,),
            lambda fb: (separate_on_device(mix_d, fb, kw, args.device, lengths=lens, seeds=sds),),
            what=str([files[i].name for i in group]))[0].cpu()
        for b, i in enumerate(group):
            for k in range(sep.shape[1]):
                d = args.output_dir / f"s{k}"
                d.mkdir(parents=True, exist_ok=True)
                wavio.save(d / f"{files[i].stem}.wav", sep[b, k:k + 1, :lens[b]], srs[b], bits=32)

    inflight.Ring(streams, launch, collect).run(batches)
    print(f"separated {len(files)} files into {args.output_dir}")


if __name__ == "__main__":
    main()
