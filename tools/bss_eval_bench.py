"""Cost of the device BSS-eval SDR / SIR / SAR (diffsep_bss_eval, csrc/bss_eval.hip) on one GPU, beside the host form.

    python tools/bss_eval_bench.py [--sources 2] [--reps 20] [--warmup 3] [--host-threads 16] [--no-host]

One batch: B = 16, S = --sources, T = 32000, L = 512 (what evaluate --bss-eval hands over for a --batch 16 of 2 s at 16 kHz).
Device: the whole launch sequence of one ops.bss_eval call between two HIP events on the current stream, median / min / max of
--reps calls after --warmup calls, clocks as found.  Host: wall time of diffsep_amd.metrics.bss_eval_host over the same
utterances on --host-threads threads (one utterance per task), median of 3, and the single-thread cost of one utterance.
Prints one JSON line.  For the per-kernel split (correlation / fill / panel / update / finish) run it once under
`rocprofv3 --kernel-trace --stats -- python tools/bss_eval_bench.py --no-host --reps 10`.
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diffusion-separation_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from diffsep_amd import metrics, ops, synth  # noqa: E402

B, T, L = 16, 32000, 512


def inputs(S):
    ref = np.stack([synth.synth_mixture(i, T=T, fs=16000, n_src=max(S, 2))[1][:S] for i in range(B)]).astype(np.float32)
    est = np.stack([[0.8 * r + 0.2 * ref[i].sum(0) + 0.3 * np.std(r) * synth.normal(f"bench{s}", T, i) for s, r in enumerate(ref[i])]
                    for i in range(B)]).astype(np.float32)
    return ref, est


def median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sources", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    torch.set_grad_enabled(False)
    S = args.sources
    ref, est = inputs(S)
    ref_d, est_d = torch.from_numpy(ref).cuda(), torch.from_numpy(est).cuda()
    for _ in range(args.warmup):
        out = ops.bss_eval(ref_d, est_d, L, 100.0)[0]
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = ops.bss_eval(ref_d, est_d, L, 100.0)[0]
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    got = out.cpu().numpy()
    res = dict(B=B, S=S, T=T, L=L, reps=args.reps, device_ms_median=round(median(ms), 3), device_ms_min=round(min(ms), 3),
               device_ms_max=round(max(ms), 3), workspace_MB=round(ops.bss_eval_workspace_bytes(B, S, T, L) / 2 ** 20, 1),
               mean_sdr=round(float(got[:, 0].mean()), 6), mean_sir=round(float(got[:, 1].mean()), 6),
               mean_sar=round(float(got[:, 2].mean()), 6))
    if not args.no_host:
        one = lambda b: metrics.bss_eval_host(ref[b:b + 1], est[b:b + 1], L, clamp_db=100.0)
        t0 = time.perf_counter()
        one(0)
        single = time.perf_counter() - t0
        walls = []
        with ThreadPoolExecutor(max_workers=args.host_threads) as pool:
            for _ in range(3):
                t0 = time.perf_counter()
                vals = list(pool.map(one, range(B)))
                walls.append(time.perf_counter() - t0)
        host = np.stack([np.stack([v["sdr"][0], v["sir"][0], v["sar"][0]]) for v in vals])
        res.update(host_threads=args.host_threads, host_wall_ms_median=round(median(walls) * 1e3, 1),
                   host_wall_ms_all=[round(w * 1e3, 1) for w in walls], host_ms_one_utterance_alone=round(single * 1e3, 1),
                   max_abs_diff_db=float(np.nanmax(np.abs(got - host))))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
