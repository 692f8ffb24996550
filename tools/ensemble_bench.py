"""Cost of the reduction over posterior draws (csrc/ensemble.hip, ops.ensemble, DiffSepModel.separate_draws) on one GPU.

    python tools/ensemble_bench.py kernel [--reps 200] [--warmup 20] [--B 16] [--K 4] [--S 2] [--T 32000]
    python tools/ensemble_bench.py file [--files 4] [--K 4] [--nf 64] [--dtype f16] [-N 30] [--reps 3]

kernel: one diffsep_ensemble call (mean + spread + medoid draw: all five launches) on B x K draws of S sources and T samples
between two HIP events, median / min / max of --reps calls after --warmup calls; the same with only the mean asked for (four
launches); beside them five launches of a one-element kernel (diffsep_randn of one value: what five empty launches cost on this
stream).  bytes_min is what the passes must move at the least — the draws read once by the Gram pass and once by the reduce
pass, the medoid draw once more, the three [B][S][T] outputs written — and gbps = bytes_min / median, hbm_fraction = that over
the HBM figure of DESIGN.md's rooflines: a whole-call rate over peak (the time holds five launches and their gaps, and the
repeated call's draws may stay in the Infinity Cache), not a measured HBM rate and not a kernel's share of peak.
file: wall time, around a device synchronise, of DiffSepModel.separate_draws on --files synthetic 4 s mixtures with K draws
each (one engine call of files x K rows) on synthetic weights, next to the same rows through separate.separate_on_device
(files x K independent single draws: the engine work alone), and of ops.ensemble on that call's rows.  One JSON line per run.
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

from diffsep_amd import _lib, inflight, ops, synth  # noqa: E402
from diffsep_amd import separate as sep_cli  # noqa: E402
from diffsep_amd.engine import param_table  # noqa: E402
from diffsep_amd.pl_model import DiffSepModel, default_config  # noqa: E402

HBM_BYTES_PER_S = 8.0e12  # MI355X peak, the figure of DESIGN.md's rooflines


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


def bench_kernel(args):
    B, K, S, T = args.B, args.K, args.S, args.T
    draws = torch.randn(B, K, S, T, device="cuda")
    mean, std, pick = (torch.empty(B, S, T, device="cuda") for _ in range(3))
    perm = torch.empty(B, K, S, dtype=torch.int32, device="cuda")
    dist = torch.empty(B, K, dtype=torch.float64, device="cuda")
    medoid = torch.empty(B, dtype=torch.int32, device="cuda")
    l = _lib.lib()
    nbytes = l.diffsep_ensemble_workspace_bytes(B, K, S)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: C.c_void_p(t.data_ptr())
    one = torch.empty(4, device="cuda")

    def full():
        _lib.check(l.diffsep_ensemble(P(draws), None, None, B, K, S, T, P(mean), P(std), P(pick), P(perm), P(dist), P(medoid), None,
                                      P(ws), nbytes, st), l)

    def mean_only():
        _lib.check(l.diffsep_ensemble(P(draws), None, None, B, K, S, T, P(mean), None, None, P(perm), P(dist), P(medoid), None,
                                      P(ws), nbytes, st), l)

    def five_small():
        for _ in range(5):
            _lib.check(l.diffsep_randn(P(one), 1, 1, 0, st), l)

    row = S * T * 4
    bytes_full = B * (2 * K * row + row + 3 * row)  # Gram pass + reduce pass read the draws; the pick pass one draw; 3 outputs
    bytes_mean = B * (2 * K * row + row)
    res = dict(case="kernel", B=B, K=K, S=S, T=T, reps=args.reps, full=timed(full, args.reps, args.warmup),
               mean_only=timed(mean_only, args.reps, args.warmup), five_one_element_launches=timed(five_small, args.reps, args.warmup),
               via_ops=timed(lambda: ops.ensemble(draws, want_std=True, want_pick=True), args.reps, args.warmup),
               workspace_bytes=nbytes, bytes_min_full=bytes_full, bytes_min_mean_only=bytes_mean)
    for name, nb in (("full", bytes_full), ("mean_only", bytes_mean)):
        s = res[name]["ms_median"] * 1e-3
        res[name].update(gbps=round(nb / s / 1e9, 1), hbm_fraction=round(nb / s / HBM_BYTES_PER_S, 4),
                         hbm_ms_once=round(nb / HBM_BYTES_PER_S * 1e3, 5))
    print(json.dumps(res), flush=True)


def bench_file(args):
    T, F, K = 32000, args.files, args.K
    m = DiffSepModel(default_config(nf=args.nf), dtype=args.dtype)
    table = [(n, s) for n, s, _ in param_table(m.score_model.cfg)]
    sd = synth.synth_state_dict(table, 7)
    m.score_model.load_state_dict({"backbone." + k: torch.from_numpy(v) for k, v in sd.items()})
    m.to("cuda:0")
    kw = {"N": args.N, "denoise": True, "intermediate": False, "corrector_steps": 1, "snr": 0.5, "schedule": None}
    mix = torch.from_numpy(np.stack([synth.synth_mixture(i, T=T)[0] for i in range(F)])).cuda()  # [F, 1, T]
    seeds = list(range(1, F + 1))
    rep = mix.repeat_interleave(K, dim=0)
    rep_seeds = [s for f in seeds for s in inflight.draw_seeds(f, K)]

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    w_draws, w_rows, w_ens = [], [], []
    for _ in range(args.reps + 1):  # (the first round warms up: workspace plan, graph capture)
        t, (est, res) = wall(lambda: m.separate_draws(mix, K, seeds=seeds, rescale=sep_cli.scale_draws, check_finite=False, **kw))
        w_draws.append(t)
        t, rows = wall(lambda: sep_cli.separate_on_device(rep, m, kw, "cuda:0", lengths=[T] * (F * K), seeds=rep_seeds))
        w_rows.append(t)
        t, _ = wall(lambda: ops.ensemble(rows.view(F, K, *rows.shape[1:])))
        w_ens.append(t)
        print(json.dumps(dict(progress=len(w_draws), wall_s=round(w_draws[-1], 4))), flush=True)
    d, r, e = median(w_draws[1:]), median(w_rows[1:]), median(w_ens[1:])
    print(json.dumps(dict(case="file", files=F, K=K, T=T, nf=args.nf, dtype=m.dtype, N=args.N, separate_draws_s=round(d, 4),
                          rows_alone_s=round(r, 4), ensemble_wall_s=round(e, 6), files_per_s=round(F / d, 3),
                          rows_per_s_alone=round(F * K / r, 3), ensemble_share_of_call=round(e / d, 5),
                          finite=bool(torch.isfinite(est).all()), medoid=res.medoid.tolist())), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernel", "file"])
    ap.add_argument("--reps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--K", type=int, default=4)
    ap.add_argument("--S", type=int, default=2)
    ap.add_argument("--T", type=int, default=32000)
    ap.add_argument("--files", type=int, default=4)
    ap.add_argument("--nf", type=int, default=64)
    ap.add_argument("--dtype", default="f16")
    ap.add_argument("-N", type=int, default=30)
    args = ap.parse_args()
    torch.set_grad_enabled(False)
    if not torch.cuda.is_available():
        raise SystemExit("No GPU visible: a timing taken anywhere else says nothing")
    if args.what == "kernel":
        args.reps = args.reps or 200
        bench_kernel(args)
    else:
        args.reps = args.reps or 3
        bench_file(args)


if __name__ == "__main__":
    main()
