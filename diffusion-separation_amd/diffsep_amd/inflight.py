"""inflight.py — what the CLIs that keep K batches in flight on one GPU share (evaluate, separate): K engines on K HIP
streams over one set of parameters, driven by ONE host thread.  Every measured fact that shapes this code is written
down here, once.  The callers hand in model objects (nothing here constructs one) and the device is reached through
`torch.cuda.` attributes and tensor methods looked up at call time, so a CPU test can put stand-ins in their place.
"""
import os

import torch

from .pl_model import cfg_get


def default_hw_queues():
    """For a process that will run several worker streams; call it BEFORE the first torch.cuda call (the HIP runtime
    reads the variable when it initialises).  HIP maps streams onto GPU_MAX_HW_QUEUES (default 4) hardware queues, one
    of which the null stream holds: with the default, two of four worker streams share a queue (measured 10.7 instead
    of 18.5 utt/s)."""
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")


def add_precision_arguments(ap):
    ap.add_argument("--dtype", default="auto", choices=["auto", "f16", "bf16", "f32", "split", "hybrid"],
                    help="auto (default): f16 for backbones up to nf = 64, hybrid for wider ones; f16: 16-bit tensors in IEEE half precision, 50 dB from the fp32 result after 60 network "
                         "evaluations; bf16: the same kernels on bfloat16 tensors (32 dB); split / f32: fp32 tensors (bf16x3 / "
                         "exact fp32 matrix products); hybrid: f16 with the first reverse steps on a split engine")
    ap.add_argument("--fp32-steps", type=int, default=None,
                    help="with --dtype hybrid: the first K reverse steps run on the fp32 engine (default: pl_model.HYBRID_HEAD_STEPS)")


def sampler_settings(config, args):
    """-> (N, corrector_steps, snr): the command line's value, else the model config's (model.sampler.*)"""
    N = cfg_get(config, "model.sampler.N", 30) if args.N is None else args.N
    cs = cfg_get(config, "model.sampler.corrector_steps", 1) if args.corrector_steps is None else args.corrector_steps
    snr = cfg_get(config, "model.sampler.snr", 0.5) if args.snr is None else args.snr
    return N, cs, snr


def plan_batches(indices, lengths, width_of, batch):
    """Group utterance indices into engine batches: equal padded width W, at most `batch` per call, longest first
    inside a width (deterministic: ties by index).  Returns a list of index lists."""
    by_w = {}
    for i in indices:
        by_w.setdefault(width_of(lengths[i]), []).append(i)
    out = []
    for w in sorted(by_w):
        g = sorted(by_w[w], key=lambda i: (-lengths[i], i))
        out += [g[k:k + batch] for k in range(0, len(g), batch)]
    return out


def utterance_seeds(n, seed):
    """Utterance i of n gets the i-th draw of a generator seeded with `seed` as its device RNG seed: what is computed
    for it does not depend on the number of streams, of ranks, or on how the utterances are batched or dealt."""
    return torch.randint(0, 2 ** 62, (max(n, 1),), generator=torch.Generator().manual_seed(seed)).tolist()


WINDOW_SEED_STRIDE = 0x9E3779B97F4A7C15  # the stride get_pc_sampler(minibatch=) advances an explicit seed by


def window_seeds(seed, K):
    """Device RNG seeds of the K windows of one long file (DiffSepModel.separate_long, separate --chunk): window 0 has the
    file's seed, window k (seed + WINDOW_SEED_STRIDE k) mod 2^64 — what is computed for a window depends neither on how
    the windows are batched nor on the streams they run on."""
    return [(int(seed) + WINDOW_SEED_STRIDE * k) % (1 << 64) for k in range(K)]


def draw_seeds(seed, K):
    """Device RNG seeds of the K posterior draws of one file (DiffSepModel.separate_draws, separate / evaluate --draws): draw 0
    has the file's seed — it is the file's ordinary output — and draw k (seed + WINDOW_SEED_STRIDE k) mod 2^64: the stride the
    fused sampler itself applies to row k of a batch under one seed, so the draws are the rows of
    get_pc_sampler(..., seed=seed, lengths=[n] * K) on the mixture repeated K times."""
    return window_seeds(seed, int(K))


def plan_draw_batches(indices, lengths, width_of, batch, K):
    """plan_batches for files that each take K rows of an engine call: batches are filled with whole files, batch // K of
    them.  K must fit the batch (the CLIs refuse it by name before they get here)."""
    if K > batch:
        raise ValueError(f"--draws {K} does not fit --batch {batch}")
    return plan_batches(indices, lengths, width_of, batch // K)


def plan_windows(lengths, window, overlap, plan):
    """The windows of all files in file-major order: -> (items, item_lengths, starts), items[n] = (file index, window
    index), item_lengths[n] = its samples (min(file length, window)), starts[i] = plan(lengths[i], window, overlap), the
    window starts of file i (ops.longform_plan).  The items are what plan_batches groups in place of files."""
    items, item_lengths, starts = [], [], []
    for i, T in enumerate(lengths):
        st = plan(T, window, overlap)
        starts.append(st)
        items += [(i, k) for k in range(len(st))]
        item_lengths += [min(T, window)] * len(st)
    return items, item_lengths, starts


def setup_workers(model, K, own_stream=True):
    """-> (K models, K streams).  One engine (weights repacked on the device + workspace) per stream over ONE set of
    parameters: the model, then replica()s; in the throughput mode when several batches are in flight
    (pl_model.DiffSepModel.set_throughput_mode).  model None (nothing to separate with): no models, streams only.
    own_stream=False with K = 1: the one worker is the current stream."""
    models = [] if model is None else [model] + [model.replica() for _ in range(K - 1)]
    for m in models:
        if K > 1:
            m.set_throughput_mode(True)
        # engines are created BEFORE the worker streams: HIP hands out hardware queues in stream-creation order, and
        # engines created lazily in between left the workers sharing queues (measured 7.0 instead of 17 utt/s, K = 4)
        m.score_model.engine()
        m.tail_engine()
    if K == 1 and not own_stream:
        return models, [torch.cuda.current_stream()]
    return models, [torch.cuda.Stream() for _ in range(K)]


def reserve_largest(models, batches, lengths, rows_per_item=1):
    """Workspace of every engine for the largest planned call, now: growing it later synchronises the whole device,
    i.e. stalls every stream.  rows_per_item: rows of an engine call that an item of a batch takes (--draws K: K)."""
    if not batches or not models:
        return
    eng = models[0].score_model.engine()
    bmax = max(len(g) for g in batches) * rows_per_item
    tmax = eng.bucket_length(eng.padded_frames(max(lengths[i] for g in batches for i in g)))
    for m in models:
        for e in (m.score_model.engine(), m.tail_engine()):
            if e is not None:
                e.reserve(bmax, tmax)


def upload(t, device="cuda"):
    """Pinned staging + asynchronous copy on the current stream (a pageable host->device copy serialises the whole
    device).  The pinned memory is allocated on the calling thread: loader threads make no HIP runtime call."""
    return t.pin_memory().to(device, non_blocking=True)


def normalize_padded(model, lens, mix, tgt=None):
    """mix [B,1,T] (and tgt [B,S,T]) right-zero-padded, utterance b being lens[b] samples long -> (mix_n, tgt_n or
    None): every utterance normalised over ITS samples (pl_model.py:81-88), the tails left at zero."""
    mix_n, tgt_n = torch.zeros_like(mix), None if tgt is None else torch.zeros_like(tgt)
    for b, L in enumerate(lens):
        (m_b, t_b), *_ = model.normalize_batch((mix[b:b + 1, :, :L], None if tgt is None else tgt[b:b + 1, :, :L]))
        mix_n[b, :, :L] = m_b[0]
        if tgt is not None:
            tgt_n[b, :, :L] = t_b[0]
    return mix_n, tgt_n


class Ring:
    """K batches in flight on K streams.  launch(w, j, group), called inside torch.cuda.stream(streams[w]), enqueues
    batch j on worker w and returns an item: whatever collect needs, INCLUDING every tensor the asynchronous work
    reads (the item is what keeps them referenced until the stream has drained).  collect(w, item) is called after
    streams[w].synchronize().
    One host thread drives all K streams: a thread per stream was measured SLOWER (10.7 instead of 17 utt/s at K = 4;
    concurrent launches serialise inside the HIP runtime and a launch that waits for queue space holds them all up).
    Whatever runs between finish(w) and the launch is serial time on all K streams."""

    def __init__(self, streams, launch, collect):
        self.streams, self.launch, self.collect = streams, launch, collect
        self.pending = [None] * len(streams)  # per worker: the item of the batch running on its stream

    def finish(self, w):
        item, self.pending[w] = self.pending[w], None
        if item is not None:
            self.streams[w].synchronize()
            self.collect(w, item)

    def run(self, groups):
        K = len(self.streams)
        for j, group in enumerate(groups):
            w = j % K
            self.finish(w)  # the worker's previous batch (oldest in flight)
            with torch.cuda.stream(self.streams[w]):
                self.pending[w] = self.launch(w, j, group)
        for w in range(K):
            self.finish(w)


def finite_or_rerun(model, stream, result, reissue, what):
    """The overflow net of a collected batch.  Half precision overflows at 65504: a batch with non-finite samples is
    repeated on the model's split-precision twin (DiffSepModel.rerun_if_nonfinite — the one place that decides; raises
    if that is non-finite too).  result = (x, ...) of the worker's drained stream; reissue(fallback_model) enqueues the
    same request, here on the same worker's stream, which is drained before the repeat's result is looked at."""
    def rerun(fb):
        with torch.cuda.stream(stream):
            r = reissue(fb)
        stream.synchronize()
        return r
    return model.rerun_if_nonfinite(result, rerun, what=what)
