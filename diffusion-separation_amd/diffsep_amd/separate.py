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
probability-flow ODE sampler (sdes.get_ode_sampler, adaptive RK45 on the device) instead of the PC sampler.
--resample {file,model}: a file whose rate is not the model's is converted to the model's rate on the device (ops.Resampler,
csrc/resample.hip: the project's Kaiser-windowed sinc; channel 0, one launch per distinct rate of a batch) and separated exactly as
a file of ceil(n p / q) samples at that rate would be; `file` converts every source back and crops it to the file's own n samples
(written at the file's rate), `model` writes at the model's rate.  With --chunk the whole file is converted first (one launch per
file, not per rate of a batch), then cut into windows.  A file already at the model's rate meets no resampler; without the flag such files only draw the reference's warning.  With
--batch 1 a file is one engine call; with --batch K > 1 the files of a batch (the same plan as the PC path) share every
network evaluation while each keeps its own step controller (diffsep_ode_sample_each), so with --dtype f32 the written
files are those of --batch 1, bit for bit wherever the network evaluation does not depend on the batch.  --streams stays 1 there: the ODE driver blocks on a readback per step
attempt.  Output files are 32-bit float WAV like torchaudio.save of a float tensor (separate.py:160-162).
--draws K [--draws-out {mean,medoid,all}]: K posterior draws per file in one engine call (a file takes K rows of a --batch, which
is filled with whole files; draw k under the seed inflight.draw_seeds(file seed, K)[k], draw 0 being the file's ordinary output),
each rescaled as a single draw is, their source orders aligned and the draws reduced on the device (DiffSepModel.separate_draws,
ops.ensemble): the mean (default) or the draw nearest to it is written where the file's output goes, and
with `all` the aligned draws next to the mean as <stem>_draw<k>.wav — their float64 mean, rounded, is the mean file sample for
sample wherever nothing is converted on the way out (with --resample file the mean and every draw are converted back
separately, and the identity holds only to that conversion's rounding).  The overflow net looks at the mean of the call's draws,
whatever is written: one non-finite sample in any draw repeats the call.  --draws 1 is the ordinary run.  Not with --chunk or --sampler ode in this version.
--init-dir DIR --t-start TAU [--init-scale {ls,none}] [--init-mean {mix,estimate}]: refine another separator's estimates
(DiffSepModel.refine, ops.warm_start).  For input_dir/name.wav the estimates are DIR/s{k}/name.wav — the
tree this tool writes.  They are scaled against the mixture (ls), normalised as the mixture is, diffused forward to the first
step time at or below TAU with the SDE's own marginal, and only the reverse steps from there run: TAU = 0.5 at -N 30 is half the
network evaluations.  The run prints the executed steps, the evaluations per file and the files whose gain fit fell back to 1.
A missing estimate, one whose length or rate differs from its mixture's, --t-start without --init-dir (or the reverse) and a
combination with --chunk, --draws, --sampler ode or --resample are refused by name before any engine is created.
--sampler ode-fixed [--ode-method {euler,heun,midpoint,rk4,ab2,ddim,dpmpp2m}] [--ode-steps M]: the probability-flow ODE on a fixed grid
(DiffSepModel.get_ode_fixed_sampler, diffsep_ode_sample_fixed) — M steps (default N) of Heun's method (default)
from t = 1 down to eps, deterministic given the seed, at a cost known beforehand (heun: 2 M network evaluations + the denoise
one).  The call is enqueued like the PC sampler's, so --batch, --streams, --seed, --schedule, --resample and the precision flags
(--fp32-steps counting solver steps) apply as they do there, and the written files do not depend on --batch or --streams.  With
--init-dir DIR --t-start TAU the solve starts at TAU itself (no snapping to a step grid) and runs M steps from there.  Not with
--chunk or --draws in this version.  Whether such a solve separates as well as the PC sampler at equal cost is not known (no
trained checkpoint was at hand): this is the instrument.  --ode-method ddim / dpmpp2m: DDIM and
DPM-Solver++ 2M, exponential integrators that treat the SDE's linear drift and noise schedule in closed form, M evaluations each.
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


class Rates:
    """The files' sample rates against the model's.  mode None (no --resample): a mismatch draws the reference's warning
    (separate.py:151-155, quirk Q9) and the samples go to the model as they are.  mode "file" / "model": such a file is converted
    to the model's rate on the device before anything else sees it; `lengths` are then the files' lengths at that rate, which is
    what batches and windows are planned with."""

    def __init__(self, mode, model_sr, files):
        info = [wavio.info(p) for p in files]
        self.mode, self.model_sr, self.files = mode, model_sr, files
        self.rates, self.ns = [sr for sr, _ in info], [n for _, n in info]
        self.lengths = [ops.Resampler(sr, model_sr).length(n) if self.converts(sr) else n for sr, n in zip(self.rates, self.ns)]

    def converts(self, sr):
        return self.mode is not None and sr != self.model_sr

    def load(self, i):
        """channel 0 of file i as a host tensor [1, n] (with the warning where the rate is wrong and nothing converts it)"""
        wav, sr = wavio.load(self.files[i])
        if sr != self.model_sr and self.mode is None:
            print(f"Warning: {self.files[i].stem}: this model expects {self.model_sr} Hz, but the file is {sr} Hz.")
        return wav[:1]

    def rows(self, idx, wavs, device):
        """files idx, loaded as wavs -> their [1, n] rows at the model's rate: the host tensors themselves where nothing is
        converted, device tensors from ONE resample launch per distinct rate otherwise"""
        out = list(wavs)
        for sr in sorted({self.rates[i] for i in idx if self.converts(self.rates[i])}):
            sel = [k for k, i in enumerate(idx) if self.rates[i] == sr]
            x, _, ns = datasets.pad_batch([(wavs[k], wavs[k]) for k in sel], side="right")
            y, new = ops.Resampler(sr, self.model_sr)(inflight.upload(x, device), lengths=ns)
            for r, k in enumerate(sel):
                out[k] = y[r, :, :new[r]]
        return out

    def restore(self, idx, seps):
        """seps[k] [S, lengths[i]] on the device, the sources of file i = idx[k] at the model's rate -> [(sources [S, n], rate)]
        as they are written: at the file's rate and cropped to its own n samples (mode "file": ceil(ceil(n p / q) q / p) >= n,
        always a crop; one launch per distinct rate), else untouched at the model's rate (at the file's without --resample)"""
        out = [(x, self.rates[i] if self.mode is None else self.model_sr) for i, x in zip(idx, seps)]
        if self.mode != "file":
            return out
        for sr in sorted({self.rates[i] for i in idx if self.converts(self.rates[i])}):
            sel = [k for k, i in enumerate(idx) if self.rates[i] == sr]
            tmax = max(seps[k].shape[-1] for k in sel)
            x = torch.stack([torch.nn.functional.pad(seps[k], (0, tmax - seps[k].shape[-1])) for k in sel])
            y, _ = ops.Resampler(self.model_sr, sr)(x, lengths=[seps[k].shape[-1] for k in sel])
            for r, k in enumerate(sel):
                out[k] = (y[r, :, :self.ns[idx[k]]], sr)
        return out


def padded_on_device(parts, to, device):
    """[1, n_b] rows on the host or on the device -> (mix [B,1,to] on the device, right-zero-padded; lengths [B])"""
    if not any(p.is_cuda for p in parts):
        mix, _, lens = datasets.pad_batch([(p, p) for p in parts], side="right", to=to)
        return inflight.upload(mix, device), lens
    lens = [int(p.shape[-1]) for p in parts]
    mix_d = torch.zeros((len(parts), 1, int(to)), dtype=torch.float32, device=device)
    host = [b for b, p in enumerate(parts) if not p.is_cuda]
    if host:
        up = inflight.upload(datasets.pad_batch([(parts[b], parts[b]) for b in host], side="right")[0], device)
    for b, p in enumerate(parts):
        mix_d[b, :, :lens[b]] = p if p.is_cuda else up[host.index(b), :, :lens[b]]
    return mix_d, lens


def write_sources(output_dir, stem, sources, sr):
    """sources [S, n] -> output_dir/s{k}/stem.wav, 32-bit float (separate.py:157-162)"""
    sources = sources.cpu()
    for k in range(sources.shape[0]):
        d = output_dir / f"s{k}"
        d.mkdir(parents=True, exist_ok=True)
        wavio.save(d / f"{stem}.wav", sources[k:k + 1], sr, bits=32)


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
    if sampler_kwargs.get("sampler") == "ode-fixed":  # --sampler ode-fixed: enqueued like the PC call (fixed_sampler_kwargs)
        fkw = {k: v for k, v in sampler_kwargs.items() if k != "sampler"}
        sampler = model.get_ode_fixed_sampler(mix_norm, check_finite=check_finite, **fkw, **extra)
    else:
        sampler = model.get_pc_sampler("reverse_diffusion", "ald2", mix_norm, check_finite=check_finite, **sampler_kwargs, **extra)
    with torch.no_grad():
        sep, nfe, *_ = sampler()
    if lengths is None:
        return scale_output(mix, sep)
    out = torch.zeros_like(sep)
    for b, L in enumerate(lengths):  # the least-squares scale of separate.py:73-78 is per file, over ITS samples
        out[b, :, :L] = scale_output(mix[b:b + 1, :, :L], sep[b:b + 1, :, :L])[0]
    return out


def add_ode_fixed_arguments(ap):
    ap.add_argument("--ode-method", default=None, choices=["euler", "heun", "midpoint", "rk4", "ab2", "ddim", "dpmpp2m"],
                    help="--sampler ode-fixed: the integrator (default heun); network evaluations for M steps: euler M, heun and "
                         "midpoint 2 M, rk4 4 M, ab2 M + 1; ddim and dpmpp2m (DPM-Solver++ 2M), the exponential integrators: M")
    ap.add_argument("--ode-steps", type=int, default=None, metavar="M",
                    help="--sampler ode-fixed: solver steps from t = 1 (or --t-start) down to eps (default: the sampler's N)")


def check_ode_fixed_arguments(args, unsupported):
    """SystemExit, naming the flag, for what --sampler ode-fixed does not run in this version (unsupported: (flag, given) pairs)
    and for its own flags given without it; args.ode_method gets its default"""
    if args.sampler != "ode-fixed":
        for flag, v in (("--ode-method", args.ode_method), ("--ode-steps", args.ode_steps)):
            if v is not None:
                raise SystemExit(f"{flag} goes with --sampler ode-fixed")
        return
    for flag, on in unsupported:
        if on:
            raise SystemExit(f"{flag} with --sampler ode-fixed is not supported in this version")
    if args.ode_steps is not None and args.ode_steps < 1:
        raise SystemExit(f"--ode-steps {args.ode_steps}: at least one step")
    args.ode_method = args.ode_method or "heun"


def fixed_sampler_kwargs(args, N):
    """what separate_on_device / DiffSepModel.refine pass on for --sampler ode-fixed (the key "sampler" marks them)"""
    return {"sampler": "ode-fixed", "N": N, "denoise": args.denoise, "schedule": args.schedule, "method": args.ode_method,
            "steps": args.ode_steps}


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


def separate_chunked(args, files, rates, seeds, models, streams, kw):
    """--chunk: the windows of all files (file-major) are the items of the batches in flight; window results stay on the device
    until their file's last one has been collected, then the file is stitched there and written.  (--resample: a file is
    converted whole, one launch per file, when its first window is launched; windows are cut from the converted row.)"""
    lengths = rates.lengths
    window, overlap = chunk_samples(args, rates.model_sr)
    eng = models[0].score_model.engine()
    items, item_lengths, starts = inflight.plan_windows(lengths, window, overlap, ops.longform_plan)
    if seeds is None:  # one draw of torch's generator per file, as a file without --seed gets one per engine call
        seeds = [int(torch.randint(0, 2 ** 62, (1,)).item()) for _ in files]
    wseeds = [inflight.window_seeds(seeds[i], len(starts[i])) for i in range(len(files))]
    batches = inflight.plan_batches(range(len(items)), item_lengths, eng.padded_frames, max(1, args.batch))
    inflight.reserve_largest(models, batches, item_lengths)
    wavs, done = {}, {}  # per file: its row while windows of it are still to be launched; collected windows by index

    def load(i):
        """file i's row at the model's rate, for one more window.  A converted row lives on the device and was written on the
        stream of the launch that met the file first; later windows are cut on other workers' streams.  So the conversion
        leaves an event, every stream waits for it before it reads the row, and the row is marked as in use on that stream
        (record_stream): its memory, from the converting stream's pool, is not handed out again while a read is pending."""
        if i not in wavs:
            row = rates.rows([i], [rates.load(i)], args.device)[0]
            ready = None
            if row.is_cuda:
                ready = torch.cuda.Event()
                ready.record()
            wavs[i] = (row, ready, len(starts[i]))
        row, ready, left = wavs[i]
        wavs[i] = (row, ready, left - 1)
        if left == 1:
            del wavs[i]
        if ready is not None:
            cur = torch.cuda.current_stream()
            cur.wait_event(ready)
            row.record_stream(cur)
        return row

    def launch(w, j, group):
        parts = []
        for n in group:
            i, k = items[n]
            parts.append(load(i)[:, starts[i][k]:starts[i][k] + item_lengths[n]])
        mix_d, lens = padded_on_device(parts, eng.bucket_length(eng.padded_frames(max(item_lengths[n] for n in group))), args.device)
        sds = [wseeds[items[n][0]][items[n][1]] for n in group]
        sep = separate_on_device(mix_d, models[w], kw, args.device, lengths=lens, seeds=sds)
        return group, lens, sep, mix_d, sds, parts  # (parts: what the copies into mix_d read stays referenced until the stream drains)

    def collect(w, item):
        group, lens, sep, mix_d, sds, _ = item
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
                (out, sr), = rates.restore([i], [out])
                out = out.cpu()
            del done[i]
            write_sources(args.output_dir, files[i].stem, out, sr)

    inflight.Ring(streams, launch, collect).run(batches)
    print(f"separated {len(files)} files into {args.output_dir} ({len(items)} windows of up to {window} samples)")


def add_draws_arguments(ap):
    ap.add_argument("--draws", type=int, default=None, metavar="K",
                    help="K posterior draws per file (seeds inflight.draw_seeds: draw 0 is the file's ordinary output), their "
                         "source orders aligned and the draws reduced on the device (ops.ensemble); a file takes K rows of a "
                         "--batch, so K must fit it")
    ap.add_argument("--draws-out", default=None, choices=["mean", "medoid", "all"],
                    help="with --draws: what is written — the mean of the draws (default), the draw nearest to the mean, or the "
                         "mean and every draw in the common source order")


def check_draws_arguments(args, chunk):
    """SystemExit, naming the flags, for a --draws request this version does not run; args.draws_out gets its default"""
    if args.draws is None:
        if args.draws_out is not None:
            raise SystemExit("--draws-out goes with --draws")
        return
    if chunk:
        raise SystemExit("--draws with --chunk is not supported: windows of several draws would have to be stitched per draw")
    if args.sampler == "ode":
        raise SystemExit("--draws with --sampler ode is not supported: the draws come from the predictor-corrector sampler")
    if not 1 <= args.draws <= 32:
        raise SystemExit(f"--draws {args.draws}: 1 to 32 draws")
    if args.draws > max(1, args.batch):
        raise SystemExit(f"--draws {args.draws} does not fit --batch {args.batch}: a file takes one row of an engine call per draw")
    args.draws_out = args.draws_out or "mean"


def scale_draws(mix_f, rows):
    """the least-squares scale of separate.py:73-78 for every draw of one file, each exactly as a single draw gets it"""
    return torch.cat([scale_output(mix_f, rows[k:k + 1]) for k in range(rows.shape[0])])


def draws_request(model, mix_d, K, lens, sds, draws_out, kw):
    """One engine call of --draws on the current stream -> (mean of the draws, the estimate draws_out names, EnsembleResult,
    aligned draws or None).  The MEAN comes first whatever is written: the overflow net (inflight.finite_or_rerun,
    DiffSepModel.rerun_if_nonfinite) looks at element 0, and a non-finite sample of ANY draw of the call is a non-finite
    sample of their mean — whereas the medoid may be a finite draw beside an overflowed one (every distance is then NaN and
    the strict < of the medoid search keeps draw 0)."""
    est, res, *al = model.separate_draws(mix_d, K, lengths=lens, seeds=sds, out=draws_out, rescale=scale_draws, check_finite=False,
                                         **kw)
    return res.mean, est, res, (al[0] if al else None)


def separate_with_draws(args, files, rates, seeds, models, streams, kw):
    """--draws K: an engine call holds batch // K whole files, K rows each (DiffSepModel.separate_draws); the mean / medoid is
    written where the file's output goes, with --draws-out all the aligned draws next to it as <stem>_draw<k>."""
    K, lengths = args.draws, rates.lengths
    eng = models[0].score_model.engine()
    if seeds is None:  # one draw of torch's generator per file, as a file without --seed gets one per engine call
        seeds = [int(torch.randint(0, 2 ** 62, (1,)).item()) for _ in files]
    batches = inflight.plan_draw_batches(range(len(files)), lengths, eng.padded_frames, max(1, args.batch), K)
    inflight.reserve_largest(models, batches, lengths, rows_per_item=K)

    def run(model, mix_d, lens, sds):
        return draws_request(model, mix_d, K, lens, sds, args.draws_out, kw)

    def launch(w, j, group):
        parts = rates.rows(group, [rates.load(i) for i in group], args.device)
        mix_d, lens = padded_on_device(parts, eng.bucket_length(eng.padded_frames(max(lengths[i] for i in group))), args.device)
        sds = [seeds[i] for i in group]
        return group, lens, run(models[w], mix_d, lens, sds), mix_d, sds

    def collect(w, item):
        group, lens, result, mix_d, sds = item
        _, est, res, al = inflight.finite_or_rerun(models[w], streams[w], result, lambda fb: run(fb, mix_d, lens, sds),
                                                   what=str([files[i].name for i in group]))
        rows = range(len(group))
        with torch.cuda.stream(streams[w]):
            outs = [(out.cpu(), sr) for out, sr in rates.restore(group, [est[b, :, :lens[b]] for b in rows])]
            each = [] if al is None else [[(out.cpu(), sr) for out, sr in rates.restore(group, [al[b, k, :, :lens[b]] for b in rows])]
                                          for k in range(K)]
        for b, i in enumerate(group):
            write_sources(args.output_dir, files[i].stem, *outs[b])
            for k, outs_k in enumerate(each):
                write_sources(args.output_dir, f"{files[i].stem}_draw{k}", *outs_k[b])

    inflight.Ring(streams, launch, collect).run(batches)
    print(f"separated {len(files)} files into {args.output_dir} ({K} draws each, {args.draws_out})")


def add_init_arguments(ap):
    ap.add_argument("--init-dir", type=Path, default=None, metavar="DIR",
                    help="refine another separator's estimates: for input_dir/name.wav read DIR/s{k}/name.wav, k = 0 .. S - 1 (the "
                         "tree this tool writes, so one run's output can feed the next), diffuse them forward to --t-start and run "
                         "only the reverse steps from there (DiffSepModel.refine).  Works with --batch, --streams, --seed, -N, "
                         "--schedule and the precision flags; NOT with --chunk, --draws, --sampler ode or --resample in this version")
    ap.add_argument("--t-start", type=float, default=None, metavar="TAU",
                    help="with --init-dir: the diffusion time in (eps, 1] to start from; the run begins at the first step time at "
                         "or below it (0.5 with -N 30: half the network evaluations); with --sampler ode-fixed the solve starts at TAU "
                         "itself and runs --ode-steps steps from there")
    ap.add_argument("--init-scale", default=None, choices=["ls", "none"],
                    help="with --init-dir: ls (default) fits one gain per estimate against the mixture first (estimates of "
                         "arbitrary scale and sign); none takes them as they are")
    ap.add_argument("--init-mean", default=None, choices=["mix", "estimate"],
                    help="with --init-dir: the source average of the perturbed state comes from the mixture (default: the network "
                         "was trained on sources that sum to it) or from the estimates (the reference's marginal_prob exactly)")


def check_init_arguments(args, files):
    """SystemExit, naming the flag or the file, for an --init-dir request this version does not run — before any engine exists;
    -> the number of s{k} folders found (None without --init-dir).  args.init_scale / init_mean get their defaults."""
    if args.init_dir is None:
        for flag, v in (("--t-start", args.t_start), ("--init-scale", args.init_scale), ("--init-mean", args.init_mean)):
            if v is not None:
                raise SystemExit(f"{flag} goes with --init-dir")
        return None
    if args.t_start is None:
        raise SystemExit("--init-dir needs --t-start: the diffusion time the refinement starts from")
    if args.chunk is not None:
        raise SystemExit("--init-dir with --chunk is not supported in this version: the estimates would have to be cut with the windows")
    if args.draws is not None:
        raise SystemExit("--init-dir with --draws is not supported in this version")
    if args.sampler == "ode":
        raise SystemExit("--init-dir with --sampler ode is not supported in this version: the ODE sampler has no start time")
    if args.resample is not None:
        raise SystemExit("--init-dir with --resample is not supported in this version: the estimates would have to be converted too")
    if not 0.0 < args.t_start:
        raise SystemExit(f"--t-start {args.t_start}: a diffusion time in (eps, 1] is needed")
    S = 0
    while (args.init_dir / f"s{S}").is_dir():
        S += 1
    for f in files:
        sr, n = wavio.info(f)
        for k in range(max(S, 1)):
            p = args.init_dir / f"s{k}" / f.name
            if not p.is_file():
                raise SystemExit(f"--init-dir: missing estimate file {p} (for {f})")
            sr_e, n_e = wavio.info(p)
            if sr_e != sr:
                raise SystemExit(f"--init-dir: {p} is at {sr_e} Hz, its mixture {f} at {sr} Hz")
            if n_e != n:
                raise SystemExit(f"--init-dir: {p} has {n_e} samples, its mixture {f} has {n}")
    args.init_scale, args.init_mean = args.init_scale or "ls", args.init_mean or "mix"
    return S


def separate_refined(args, files, rates, seeds, models, streams, kw, S):
    """--init-dir: the ring of the ordinary run with DiffSepModel.refine as the engine call; one line at the end with the executed
    steps, the network evaluations and the files whose gain fit fell back"""
    from . import sdes
    lengths = rates.lengths
    eng = models[0].score_model.engine()
    if S != eng.S:
        raise SystemExit(f"--init-dir: {S} source folders s0 .. s{S - 1} in {args.init_dir}, the model separates {eng.S} sources")
    N = kw["N"] if kw.get("N") is not None else models[0].sde.N
    fixed = kw.get("sampler") == "ode-fixed"
    if fixed:  # (the solve starts at --t-start itself: there is no step grid to snap to)
        if not models[0].t_eps < args.t_start <= models[0].sde.T:
            raise SystemExit(f"--t-start {args.t_start}: a diffusion time in (eps, 1] = ({models[0].t_eps:g}, {models[0].sde.T:g}] is needed")
    else:
        try:
            first = sdes.first_step_for(args.t_start, sdes.sampler_timesteps(N, models[0].t_eps, kw.get("schedule"), T=models[0].sde.T))
        except ValueError as e:
            raise SystemExit(f"--t-start {args.t_start}: {e}")
    if seeds is None:  # one draw of torch's generator per file, as a file without --seed gets one per engine call
        seeds = [int(torch.randint(0, 2 ** 62, (1,)).item()) for _ in files]
    batches = inflight.plan_batches(range(len(files)), lengths, eng.padded_frames, max(1, args.batch))
    inflight.reserve_largest(models, batches, lengths)
    seen = {"nfe": None, "fell_back": []}

    def run(model, mix_d, est_d, lens, sds):
        sep, info = model.refine(mix_d, est_d, t_start=args.t_start, lengths=lens, seeds=sds, scale=args.init_scale,
                                 mean_from=args.init_mean, check_finite=False, **kw)
        return sep, info

    def launch(w, j, group):
        parts = rates.rows(group, [rates.load(i) for i in group], args.device)
        to = eng.bucket_length(eng.padded_frames(max(lengths[i] for i in group)))
        mix_d, lens = padded_on_device(parts, to, args.device)
        est = torch.zeros((len(group), S, int(to)), dtype=torch.float32)
        for b, i in enumerate(group):
            for k in range(S):
                est[b, k, :lens[b]] = wavio.load(args.init_dir / f"s{k}" / files[i].name)[0][0]
        est_d = inflight.upload(est, args.device)
        sds = [seeds[i] for i in group]
        return group, lens, run(models[w], mix_d, est_d, lens, sds), mix_d, est_d, sds

    def collect(w, item):
        group, lens, result, mix_d, est_d, sds = item
        sep, info = inflight.finite_or_rerun(models[w], streams[w], result, lambda fb: run(fb, mix_d, est_d, lens, sds),
                                             what=str([files[i].name for i in group]))
        with torch.cuda.stream(streams[w]):
            outs = [(out.cpu(), sr) for out, sr in rates.restore(group, [sep[b, :, :lens[b]] for b in range(len(group))])]
            fell = info["fallback"].cpu().tolist()
        seen["nfe"] = info["nfe"]
        seen["fell_back"] += [files[i].name for b, i in enumerate(group) if fell[b]]
        for i, (out, sr) in zip(group, outs):
            write_sources(args.output_dir, files[i].stem, out, sr)

    inflight.Ring(streams, launch, collect).run(batches)
    fb = f"; gain fit fell back to 1 for {sorted(seen['fell_back'])}" if seen["fell_back"] else ""
    if fixed:
        print(f"refined {len(files)} files from {args.init_dir} into {args.output_dir}: {kw['steps'] or N} {kw['method']} steps of the "
              f"probability-flow ODE from t = {args.t_start:g}, NFE {seen['nfe']} per file{fb}")
        return
    print(f"refined {len(files)} files from {args.init_dir} into {args.output_dir}: steps [{first}, {N}) of {N} from t = {args.t_start:g}, "
          f"NFE {seen['nfe']} per file{fb}")


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
    ap.add_argument("--sampler", default="pc", choices=["pc", "ode", "ode-fixed"],
                    help="pc (default): the reference's predictor-corrector sampler; ode: the probability-flow ODE "
                         "(adaptive RK45, sdes.get_ode_sampler); with --batch K the files of a batch share the network "
                         "evaluations, each with its own step controller; ode-fixed: the same ODE on a fixed grid "
                         "(--ode-method, --ode-steps), deterministic given the seed, at a cost known beforehand, enqueued like pc "
                         "(--batch, --streams, --schedule, --init-dir / --t-start all apply)")
    add_ode_fixed_arguments(ap)
    ap.add_argument("--rtol", type=float, default=1e-5, help="--sampler ode: relative tolerance (reference default)")
    ap.add_argument("--atol", type=float, default=1e-5, help="--sampler ode: absolute tolerance (reference default)")
    ap.add_argument("--max-nfe", type=int, default=0,
                    help="--sampler ode: no step attempt starts beyond this many network evaluations (0: unbounded)")
    ap.add_argument("--chunk", type=float, default=None, metavar="SECONDS",
                    help="cut files longer than this into windows of this length (4 = the shape the engine is tuned for), "
                         "separate the windows as the items of --batch / --streams and stitch them on the device")
    ap.add_argument("--overlap", type=float, default=None, metavar="SECONDS",
                    help="with --chunk: overlap of neighbouring windows (default: an eighth of the chunk; at most a third)")
    ap.add_argument("--resample", default=None, choices=["file", "model"],
                    help="convert a file whose rate is not the model's to the model's rate on the device, separate it there, and "
                         "write the sources back at the file's rate, cropped to its length (file), or at the model's rate (model); "
                         "default: such a file only draws a warning and its samples go to the model as they are")
    add_draws_arguments(ap)
    add_init_arguments(ap)
    args = ap.parse_args(argv)
    check_ode_fixed_arguments(args, (("--chunk", args.chunk is not None), ("--draws", args.draws is not None)))
    check_draws_arguments(args, chunk=args.chunk is not None)
    init_sources = check_init_arguments(args, sorted(args.input_dir.glob("*.wav")))
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
    if args.sampler == "ode-fixed":
        kw = fixed_sampler_kwargs(args, kw["N"])
    models, streams = inflight.setup_workers(model, K, own_stream=False)  # (K = 1 runs on the current stream)
    model_sr = cfg_get(model.config, "model.fs", 8000)
    if args.output_dir.is_file():
        raise ValueError("Output directory is a file")
    args.output_dir.mkdir(parents=True, exist_ok=True)
    files = sorted(args.input_dir.glob("*.wav"))
    rates = Rates(args.resample, model_sr, files)
    lengths = rates.lengths
    seeds = inflight.utterance_seeds(len(files), args.seed) if args.seed is not None else None
    if args.sampler == "ode" and args.batch > 1:
        ode_kw = {"N": kw["N"], "denoise": args.denoise, "rtol": args.rtol, "atol": args.atol, "max_nfe": args.max_nfe}
        eng = model.score_model.engine()
        for group in inflight.plan_batches(range(len(files)), lengths, eng.padded_frames, args.batch):
            parts = rates.rows(group, [rates.load(i) for i in group], args.device)
            mix, lens = padded_on_device(parts, eng.bucket_length(eng.padded_frames(max(lengths[i] for i in group))), args.device)
            # (files without --seed: one draw of torch's generator per file, as the --batch 1 loop takes them)
            sds = [seeds[i] if seeds is not None else int(torch.randint(0, 2 ** 62, (1,)).item()) for i in group]
            sep, _ = separate_ode_batch(mix, model, ode_kw, args.device, lens, seeds=sds)
            for i, (out, sr) in zip(group, rates.restore(group, [sep[b, :, :lens[b]] for b in range(len(group))])):
                write_sources(args.output_dir, files[i].stem, out, sr)
        print(f"separated {len(files)} files into {args.output_dir} (probability-flow ODE, {args.batch} files per call)")
        return
    if args.sampler == "ode":
        ode_kw = {"N": kw["N"], "denoise": args.denoise, "rtol": args.rtol, "atol": args.atol, "max_nfe": args.max_nfe}
        for i, f in enumerate(files):
            row, = rates.rows([i], [rates.load(i)], args.device)
            sep, _ = separate_ode(row, model, ode_kw, args.device, seed=seeds[i] if seeds is not None else None)
            (out, sr), = rates.restore([i], [sep[0]])
            write_sources(args.output_dir, f.stem, out, sr)
        print(f"separated {len(files)} files into {args.output_dir} (probability-flow ODE)")
        return
    if args.chunk is not None:
        return separate_chunked(args, files, rates, seeds, models, streams, kw)
    if args.init_dir is not None:
        return separate_refined(args, files, rates, seeds, models, streams, kw, init_sources)
    if args.draws is not None and (args.draws > 1 or args.draws_out != "mean"):  # (--draws 1 = one draw: the ordinary run)
        return separate_with_draws(args, files, rates, seeds, models, streams, kw)
    eng = model.score_model.engine()
    batches = inflight.plan_batches(range(len(files)), lengths, eng.padded_frames, max(1, args.batch))
    inflight.reserve_largest(models, batches, lengths)

    def launch(w, j, group):
        """-> (file indices, lengths, device result, and what a repeat of the request needs)"""
        parts = rates.rows(group, [rates.load(i) for i in group], args.device)
        mix_d, lens = padded_on_device(parts, eng.bucket_length(eng.padded_frames(max(lengths[i] for i in group))), args.device)
        sds = [seeds[i] for i in group] if seeds is not None else None
        sep = separate_on_device(mix_d, models[w], kw, args.device, lengths=lens, seeds=sds)
        return group, lens, sep, mix_d, sds

    def collect(w, item):
        group, lens, sep, mix_d, sds = item
        sep = inflight.finite_or_rerun(
            models[w], streams[w], (sep,),
            lambda fb: (separate_on_device(mix_d, fb, kw, args.device, lengths=lens, seeds=sds),),
            what=str([files[i].name for i in group]))[0]
        with torch.cuda.stream(streams[w]):  # (the conversion back, if any, runs on the drained worker's stream)
            outs = [(out.cpu(), sr) for out, sr in rates.restore(group, [sep[b, :, :lens[b]] for b in range(len(group))])]
        for i, (out, sr) in zip(group, outs):
            write_sources(args.output_dir, files[i].stem, out, sr)

    inflight.Ring(streams, launch, collect).run(batches)
    print(f"separated {len(files)} files into {args.output_dir}")


if __name__ == "__main__":
    main()
