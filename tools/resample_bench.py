"""Cost of the device sample-rate converter (diffsep_resample, csrc/resample.hip) on one GPU, beside the host form.

    python tools/resample_bench.py [--reps 30] [--warmup 5] [--host-threads 16] [--no-host] [--seconds 4 60]
    python tools/resample_bench.py --cli [--files 64] [--nf 64]

Kernel part: 32 rows (B = 16, S = 2) of 4 s and of 60 s at 2/1, 1/2, 441/80 and 80/441, fp32 output.  Device: one ops.Resampler call
between two HIP events on the current stream, median / min / max of --reps calls after --warmup calls, clocks as found; the share
of the HBM floor = rows * 4 * (T_in + T_out) bytes at 8 TB/s over the median.  Host: what the tree offered before the kernel for
the same work, metrics.resample (scipy's resample_poly on the same filter) over the 32 rows on --host-threads threads plus the
two copies (device -> host of the input, host -> device of the float32 result), wall time, median of 3.  One JSON line per case.

--cli: `separate --resample file --batch 16 --streams 4` on --files 4 s files stored at 16 kHz against the same material stored at
8 kHz without the flag (synthetic weights of width --nf, default sampler): files per second of each whole run, of each run with
twice the files minus the run itself (the set-up cancels), and the resampler's share of a batch: one conversion down of
[16, 1, 64000] plus one up of [16, 2, 32000] between events, over the time a batch of 16 takes at the measured rate.
"""
import argparse
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diffusion-separation_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from diffsep_amd import metrics, ops, synth, wavio  # noqa: E402

ROWS = (16, 2)
RATES = [(8000, 16000), (16000, 8000), (8000, 44100), (44100, 8000)]  # p / q = 2/1, 1/2, 441/80, 80/441
HBM_BYTES_PER_S = 8e12


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
    return ms


def kernel_part(args):
    B, S = ROWS
    for seconds in args.seconds:
        for fs_in, fs_out in RATES:
            T = int(seconds * fs_in)
            rng = np.random.default_rng(fs_in + fs_out)
            x = rng.standard_normal((B, S, T)).astype(np.float32)
            xd = torch.from_numpy(x).cuda()
            rs = ops.Resampler(fs_in, fs_out)
            n = rs.length(T)
            out = torch.empty((B, S, n), dtype=torch.float32, device="cuda")
            ms = timed(lambda: rs(xd, out=out), args.reps, args.warmup)
            floor_us = B * S * 4 * (T + n) / HBM_BYTES_PER_S * 1e6
            taps = len(ops.resample_design(rs.p, rs.q))
            res = dict(p=rs.p, q=rs.q, seconds=seconds, rows=B * S, T_in=T, T_out=n, taps=taps, taps_per_output=-(-taps // rs.p),
                       reps=args.reps, device_us_median=round(median(ms) * 1e3, 2), device_us_min=round(min(ms) * 1e3, 2),
                       device_us_max=round(max(ms) * 1e3, 2), hbm_floor_us=round(floor_us, 2),
                       fraction_of_hbm_floor=round(floor_us / (median(ms) * 1e3), 4))
            if not args.no_host:
                def host():
                    h = xd.cpu().numpy().reshape(B * S, T)
                    with ThreadPoolExecutor(max_workers=args.host_threads) as pool:
                        y = list(pool.map(lambda r: metrics.resample(r.astype(np.float64), fs_out, fs_in).astype(np.float32), h))
                    return torch.from_numpy(np.stack(y)).cuda()
                host()
                walls = []
                for _ in range(3):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    y = host()
                    torch.cuda.synchronize()
                    walls.append(time.perf_counter() - t0)
                diff = float((y.reshape(B, S, n).double() - out.double()).abs().max())
                res.update(host_threads=args.host_threads, host_wall_ms_median=round(median(walls) * 1e3, 2),
                           host_wall_ms_all=[round(w * 1e3, 2) for w in walls], max_abs_diff_fp32_outputs=diff)
            print(json.dumps(res), flush=True)


def cli_part(args):
    from diffsep_amd import separate
    B, S = ROWS
    T8 = 32000
    down, up = ops.Resampler(16000, 8000), ops.Resampler(8000, 16000)
    with tempfile.TemporaryDirectory() as tmp:
        tmp = Path(tmp)
        walls = {}
        for count in (args.files, 2 * args.files):
            d16, d8 = tmp / f"in16_{count}", tmp / f"in8_{count}"
            d16.mkdir()
            d8.mkdir()
            for i in range(count):
                x16 = synth.synth_mixture(i, T=2 * T8, fs=16000)[0].astype(np.float32)
                wavio.save(d16 / f"utt{i:04d}.wav", torch.from_numpy(x16), 16000, bits=32)
                x8 = metrics.resample(x16[0].astype(np.float64), 8000, 16000).astype(np.float32)
                wavio.save(d8 / f"utt{i:04d}.wav", torch.from_numpy(x8)[None], 8000, bits=32)
            common = ["--synthetic-weights", str(args.nf), "--batch", "16", "--streams", "4", "--seed", "1"]
            for name, src, extra in (("16k_resample_file", d16, ["--resample", "file"]), ("8k_plain", d8, [])):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                separate.main([str(src), str(tmp / f"out_{name}_{count}")] + extra + common)
                torch.cuda.synchronize()
                walls[name, count] = time.perf_counter() - t0
        res = dict(files=args.files, nf=args.nf, seconds_per_file=4)
        for name in ("16k_resample_file", "8k_plain"):
            w1, w2 = walls[name, args.files], walls[name, 2 * args.files]
            res[name] = dict(wall_s=round(w1, 3), wall_s_twice_the_files=round(w2, 3), files_per_s_whole_run=round(args.files / w1, 2),
                             files_per_s_marginal=round(args.files / max(w2 - w1, 1e-9), 2))
    xd = torch.randn((B, 1, 2 * T8), device="cuda")
    sd = torch.randn((B, S, T8), device="cuda")
    ms = timed(lambda: (down(xd), up(sd)), 30, 5)
    batch_ms = B / res["16k_resample_file"]["files_per_s_marginal"] * 1e3
    res.update(resample_down_and_up_us_per_batch=round(median(ms) * 1e3, 2), batch_ms_at_marginal_rate=round(batch_ms, 2),
               resampler_share_of_a_batch=round(median(ms) / batch_ms, 5))
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--seconds", type=float, nargs="+", default=[4, 60])
    ap.add_argument("--cli", action="store_true")
    ap.add_argument("--files", type=int, default=64)
    ap.add_argument("--nf", type=int, default=64)
    args = ap.parse_args()
    torch.set_grad_enabled(False)
    if not torch.cuda.is_available():
        raise SystemExit("resample_bench needs the GPU: a timing taken elsewhere says nothing about it")
    cli_part(args) if args.cli else kernel_part(args)


if __name__ == "__main__":
    main()
