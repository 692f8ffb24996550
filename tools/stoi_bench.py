"""Cost of the device STOI / ESTOI (diffsep_stoi, csrc/stoi.hip) on one GPU, beside the host path it can replace.

    python tools/stoi_bench.py [--reps 50] [--warmup 5] [--host-threads 16] [--no-host]

Two batches: B = 16, S = 2, T = 32000, fs = 8000 (the bench batch: 32 sources of 4 s) and B = 4, S = 2, T = 160000,
fs = 16000 (8 sources of 10 s); ESTOI and STOI.  Device: the whole launch sequence of one ops.stoi call between two HIP
events on the current stream, median / min / max of --reps calls after --warmup calls, clocks as found.  Host: wall time of
diffsep_amd.metrics.stoi over the same sources on --host-threads threads (what evaluate --stoi-on host does on its
loader pool), median of 3, and the single-thread cost per source.  Prints one JSON line per case.  For the per-kernel
split run it once under `rocprofv3 --kernel-trace --stats -- python tools/stoi_bench.py --no-host --reps 20`.
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

CASES = [dict(B=16, S=2, T=32000, fs=8000), dict(B=4, S=2, T=160000, fs=16000)]


def inputs(B, S, T, fs):
    ref = np.stack([synth.synth_mixture(i, T=T, fs=fs, n_src=S)[1] for i in range(B)]).astype(np.float32)
    est = np.stack([[r + 0.3 * np.std(r) * synth.normal(f"bench{s}", T, i) for s, r in enumerate(ref[i])]
                    for i in range(B)]).astype(np.float32)
    return ref, est


def median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    torch.set_grad_enabled(False)
    for case in CASES:
        B, S, T, fs = case["B"], case["S"], case["T"], case["fs"]
        ref, est = inputs(B, S, T, fs)
        ref_d, est_d = torch.from_numpy(ref).cuda(), torch.from_numpy(est).cuda()
        for extended in (True, False):
            for _ in range(args.warmup):
                out = ops.stoi(ref_d, est_d, fs, extended=extended)
            torch.cuda.synchronize()
            ms = []
            for _ in range(args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = ops.stoi(ref_d, est_d, fs, extended=extended)
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            res = dict(case, measure="ESTOI" if extended else "STOI", sources=B * S, reps=args.reps,
                       device_ms_median=round(median(ms), 4), device_ms_min=round(min(ms), 4), device_ms_max=round(max(ms), 4),
                       workspace_MB=round(ops.stoi_workspace_bytes(B, S, T, fs) / 2 ** 20, 1),
                       mean_value=round(float(out.mean()), 6))
            if not args.no_host:
                jobs = [(ref[b, s], est[b, s]) for b in range(B) for s in range(S)]
                ones = []
                for j in jobs[:4]:  # (the first call also imports scipy.signal: not counted)
                    t0 = time.perf_counter()
                    metrics.stoi(j[0], j[1], fs, extended)
                    ones.append(time.perf_counter() - t0)
                t_one = median(ones[1:])
                walls = []
                with ThreadPoolExecutor(max_workers=args.host_threads) as pool:
                    for _ in range(3):
                        t0 = time.perf_counter()
                        vals = list(pool.map(lambda j: metrics.stoi(j[0], j[1], fs, extended), jobs))
                        walls.append(time.perf_counter() - t0)
                res.update(host_threads=args.host_threads, host_wall_ms_median=round(median(walls) * 1e3, 2),
                           host_wall_ms_all=[round(w * 1e3, 2) for w in walls], host_ms_per_source_one_thread=round(t_one * 1e3, 2),
                           max_abs_diff=float(np.max(np.abs(out.cpu().numpy().reshape(-1) - np.asarray(vals)))))
            print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
