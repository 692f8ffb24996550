"""Cost of long-recording separation (csrc/longform.hip, DiffSepModel.separate_long, separate --chunk) on one GPU.

    python tools/longform_bench.py stitch [--reps 200] [--warmup 20]
    python tools/longform_bench.py file --seconds 60 [--chunk 4 | --no-chunk] [--nf 64] [--dtype f16] [--batch 16] [--reps 3]

stitch: one diffsep_longform_stitch call on a 60 s file at 8 kHz (K = 17 windows of 32000 samples, overlap 4000, S = 2) between
two HIP events, median / min / max of --reps calls after --warmup calls; beside it three launches of a one-element kernel
(diffsep_randn of one value: what three empty launches cost on this stream) and the time its tensors take at the HBM rate.
file: wall time, around a device synchronise, of one synthetic recording of --seconds through the model on synthetic weights:
with --chunk through DiffSepModel.separate_long (what separate --chunk runs per file), with --no-chunk through
separate.separate_on_device in one engine call (what separate runs without --chunk; this mode uses nothing the long-recording
change added, so the same script measures an older checkout); Engine.device_bytes() afterwards.  One JSON line per run.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diffusion-separation_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from diffsep_amd import _lib, ops, synth  # noqa: E402
from diffsep_amd import separate as sep_cli  # noqa: E402
from diffsep_amd.engine import param_table  # noqa: E402
from diffsep_amd.pl_model import DiffSepModel, default_config  # noqa: E402

HBM_BYTES_PER_S = 8.0e12  # MI355X peak


def median(v):
    return sorted(v)[len(v) // 2]


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return dict(ms_median=round(median(ms), 5), ms_min=round(min(ms), 5), ms_max=round(max(ms), 5))


def bench_stitch(args):
    K, S, Tw, Tv, T = 17, 2, 32000, 4000, 480000
    assert len(ops.longform_plan(T, Tw, Tv)) == K
    win = torch.randn(K, S, Tw, device="cuda")
    out = torch.empty(S, T, device="cuda")
    perm = torch.empty(K, S, dtype=torch.int32, device="cuda")
    l = _lib.lib()
    nbytes = l.diffsep_longform_workspace_bytes(K, S)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: C.c_void_p(t.data_ptr())
    one = torch.empty(4, device="cuda")

    def stitch():
        _lib.check(l.diffsep_longform_stitch(P(win), K, S, Tw, T, Tv, P(out), P(perm), None, P(ws), nbytes, st), l)

    def three_small():
        for _ in range(3):
            _lib.check(l.diffsep_randn(P(one), 1, 1, 0, st), l)

    res = dict(case="stitch", K=K, S=S, Tw=Tw, Tv=Tv, T=T, reps=args.reps, stitch=timed(stitch, args.reps, args.warmup),
               three_one_element_launches=timed(three_small, args.reps, args.warmup),
               stitch_via_ops=timed(lambda: ops.longform_stitch(win, T, Tv), args.reps, args.warmup))
    bytes_in, bytes_out = K * S * Tw * 4, S * T * 4
    starts = ops.longform_plan(T, Tw, Tv)
    gram_in = 2 * S * 4 * sum(starts[k] + Tw - starts[k + 1] for k in range(K - 1))  # both windows' rows over every overlap
    res.update(bytes_in=bytes_in, bytes_out=bytes_out, gram_bytes_read=gram_in,
               hbm_ms_once=round((bytes_in + bytes_out) / HBM_BYTES_PER_S * 1e3, 5))
    print(json.dumps(res), flush=True)


def bench_file(args):
    fs = 8000
    T = int(round(args.seconds * fs))
    m = DiffSepModel(default_config(nf=args.nf), dtype=args.dtype)
    table = [(n, s) for n, s, _ in param_table(m.score_model.cfg)]
    sd = synth.synth_state_dict(table, 7)
    m.score_model.load_state_dict({"backbone." + k: torch.from_numpy(v) for k, v in sd.items()})
    m.to("cuda:0")
    kw = {"N": args.N, "denoise": True, "intermediate": False, "corrector_steps": 1, "snr": 0.5, "schedule": None}
    reps = int(np.ceil(T / 32000))
    mix = torch.from_numpy(np.concatenate([synth.synth_mixture(i, T=32000)[0] for i in range(reps)], axis=-1)[:, :T]).cuda()
    walls = []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if args.no_chunk:
            out = sep_cli.separate_on_device(mix[None], m, kw, "cuda:0", lengths=[T], seeds=[1])
        else:
            out = m.separate_long(mix, int(round(args.chunk * fs)), int(round(args.chunk * fs / 8)), batch=args.batch, seed=1, **kw)
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
        print(json.dumps(dict(progress=len(walls), wall_s=round(walls[-1], 3))), flush=True)
    eng = m.score_model.engine()
    print(json.dumps(dict(case="file", seconds=args.seconds, T=T, chunk=None if args.no_chunk else args.chunk, nf=args.nf,
                          dtype=m.dtype, N=args.N, batch=args.batch, wall_s_all=[round(w, 3) for w in walls],
                          wall_s_last=round(walls[-1], 3), finite=bool(torch.isfinite(out).all()), shape=list(out.shape),
                          frames=eng.padded_frames(T if args.no_chunk else min(T, int(round(args.chunk * fs)))),
                          engine_device_MB=round(eng.device_bytes() / 2 ** 20, 1),
                          torch_max_allocated_MB=round(torch.cuda.max_memory_allocated() / 2 ** 20, 1))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["stitch", "file"])
    ap.add_argument("--reps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--chunk", type=float, default=4.0)
    ap.add_argument("--no-chunk", action="store_true")
    ap.add_argument("--nf", type=int, default=64)
    ap.add_argument("--dtype", default="f16")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("-N", type=int, default=30)
    args = ap.parse_args()
    torch.set_grad_enabled(False)
    if args.what == "stitch":
        args.reps = args.reps or 200
        bench_stitch(args)
    else:
        args.reps = args.reps or 3
        bench_file(args)


if __name__ == "__main__":
    main()
