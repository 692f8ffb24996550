"""Cost of the probability-flow ODE sampler (Engine.ode_sample, sdes.get_ode_sampler) on one GPU.

    python tools/ode_bench.py [--nf 64] [--B 16] [--T 32000] [--rtol 1e-5] [--atol 1e-5] [--max-nfe 600]
                              [--dtypes f32,split,f16] [--reps 2] [--each | --fixed [--distance]]

Synthetic weights, synthetic mixtures, MixSDE.  Per engine dtype: nfev / accepted / rejected / status of the solve, the
wall time of one batch (median of --reps timed calls after one warm-up call), and the share of that time spent outside
the network evaluations.  That share is estimated as 1 - (nfev + denoise) * t_nfe / wall, with t_nfe the time of one
graph-replayed evaluation of the same (B, T) plan measured through a PC sampler run without corrector (N evaluations +
N light update kernels).  Prints one JSON line per dtype.

--each: the per-utterance sampler instead (Engine.ode_sample_each: one step controller per utterance, all sharing every
network evaluation).  Per dtype: the wall time of one ode_sample_each call on the batch (after one warm-up call) against
the SUM of the wall times of B calls of ode_sample on the utterances one by one (B = 1, the same seeds, after one warm-up
call of that plan), the evaluations the batch call ran (evals_run = the largest nfev), the utterances' nfev range and
whether every row of the batch call equals its B = 1 result bit for bit (expected on f32 only).

--fixed: the fixed-step sampler (Engine.ode_sample_fixed: Heun M = 30, 60 evaluations + denoise, and Euler M = 30, 30 + denoise)
next to the PC sampler of the same plan (N = 30, one corrector step: 60 evaluations) in the same process.  Per dtype, first one
batch at a time — --reps timed calls of each of the three, alternating, after two warm-up calls each: median wall, min - max,
and the wall per network evaluation — then --streams K (default 4) engines on K streams through inflight.Ring, --batches
batches each, the three again alternating: wall per batch and batches per second; and the local-error trace of Heun at M = 30 and
M = 120 (want_err).  The exponential integrators of the same entry ride along in every part: DDIM and DPM-Solver++ 2M at M = 30
(30 evaluations + denoise), and the trace of 2M (step minus its DDIM step).  --distance adds the rel RMS distance of ddim / dpmpp2m /
heun at M = 32, 64, 128 (no denoise) from the adaptive solve at --rtol / --atol (--max-nfe 0 lets it finish) from the same start
state.  Prints one JSON line per dtype.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diffusion-separation_amd"))

import torch  # noqa: E402

from diffsep_amd import _lib, ops, synth  # noqa: E402
from diffsep_amd.engine import Engine, pack_state_dict, param_table  # noqa: E402

DTYPES = {"f32": _lib.F32, "split": _lib.F32_SPLIT, "f16": _lib.F16, "bf16": _lib.BF16}
MIX = dict(kind=_lib.SDE_MIX, ndim=2, d_lambda=2.0, sigma_min=0.05, sigma_max=0.5)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, time.perf_counter() - t0


def bench_each(eng, mix_norm, args, name):
    B = mix_norm.shape[0]
    seeds = [1000 + 7 * b for b in range(B)]
    kw = dict(rtol=args.rtol, atol=args.atol, max_nfe=args.max_nfe)
    each = lambda: eng.ode_sample_each(mix_norm, MIX, seeds=seeds, **kw)  # noqa
    each()
    (out, infos, evals), wall_each = timed(each)
    one = [mix_norm[b:b + 1].contiguous() for b in range(B)]
    eng.ode_sample(one[0], MIX, seed=seeds[0], **kw)
    wall_solo, equal, solo_nfev = 0.0, True, []
    for b in range(B):
        (x, info), w = timed(lambda: eng.ode_sample(one[b], MIX, seed=seeds[b], **kw))
        wall_solo += w
        solo_nfev.append(info["nfev"])
        equal = equal and bool(torch.equal(x[0], out[b])) and info == infos[b]
    nfev = [i["nfev"] for i in infos]
    print(json.dumps(dict(mode="each", dtype=name, nf=args.nf, B=B, T=args.T, rtol=args.rtol, atol=args.atol,
                          max_nfe=args.max_nfe, evals_run=evals, nfev_min=min(nfev), nfev_max=max(nfev),
                          statuses=sorted({i["status"] for i in infos}), solo_nfev_sum=sum(solo_nfev),
                          finite=bool(torch.isfinite(out).all()), wall_each_ms=round(wall_each * 1e3, 1),
                          wall_solo_sum_ms=round(wall_solo * 1e3, 1), speedup=round(wall_solo / wall_each, 2),
                          rows_equal_solo=equal)), flush=True)


def bench_fixed(cfg, sd, mix_norm, args, name):
    from diffsep_amd import inflight
    K = max(1, args.streams)
    # engines before streams: HIP hands out hardware queues in stream-creation order (inflight.setup_workers)
    engines = [Engine(cfg, pack_state_dict(cfg, sd)) for _ in range(K)]
    for e in engines:
        e.reserve(mix_norm.shape[0], mix_norm.shape[2])
    streams = [torch.cuda.Stream() for _ in range(K)]
    runs = {"pc": (lambda e: e.pc_sample(mix_norm, MIX, N=30, corrector_steps=1, seed=1)[0], 60),
            "heun30": (lambda e: e.ode_sample_fixed(mix_norm, MIX, method="heun", steps=30, seed=1)[0], 61),
            "euler30": (lambda e: e.ode_sample_fixed(mix_norm, MIX, method="euler", steps=30, seed=1)[0], 31),
            "ddim30": (lambda e: e.ode_sample_fixed(mix_norm, MIX, method="ddim", steps=30, seed=1)[0], 31),
            "dpmpp2m30": (lambda e: e.ode_sample_fixed(mix_norm, MIX, method="dpmpp2m", steps=30, seed=1)[0], 31)}
    res = dict(mode="fixed", dtype=name, nf=args.nf, B=mix_norm.shape[0], T=args.T, streams=K, batches=args.batches,
               hw_queues=os.environ.get("GPU_MAX_HW_QUEUES"))
    walls = {k: [] for k in runs}
    for k, (fn, _) in runs.items():  # warm-up: plan, graph capture, buffers — on every engine
        for e in engines:
            fn(e)
            fn(e)
    torch.cuda.synchronize()
    for _ in range(max(1, args.reps)):
        for k, (fn, _) in runs.items():
            out, w = timed(lambda: fn(engines[0]))
            walls[k].append(w)
            res[k + "_finite"] = bool(torch.isfinite(out).all())
    for k, (_, evals) in runs.items():
        ws = sorted(walls[k])
        med = ws[len(ws) // 2]
        res[k] = dict(evals=evals, wall_ms=round(med * 1e3, 2), min_ms=round(ws[0] * 1e3, 2), max_ms=round(ws[-1] * 1e3, 2),
                      ms_per_eval=round(med * 1e3 / evals, 4))
    # the local-error trace of Heun: per step the largest over the utterances of rms(step - Euler step) / rms(y)
    for M in (30, 120):
        _, info = engines[0].ode_sample_fixed(mix_norm, MIX, method="heun", steps=M, seed=1, want_err=True)
        rel = (info["err"][:, :, 0] / info["err"][:, :, 1]).amax(dim=1).cpu()
        res[f"heun{M}_local_err"] = dict(max=round(float(rel.max()), 5), median=round(float(rel.median()), 5),
                                         first=[round(float(v), 5) for v in rel[:3]], last=[round(float(v), 5) for v in rel[-3:]],
                                         step_of_max=int(rel.argmax()))
    _, info = engines[0].ode_sample_fixed(mix_norm, MIX, method="dpmpp2m", steps=30, seed=1, want_err=True)
    rel = (info["err"][:, :, 0] / info["err"][:, :, 1]).amax(dim=1).cpu()  # rms(step - its DDIM step) / rms(y)
    res["dpmpp2m30_local_err"] = dict(max=round(float(rel.max()), 5), median=round(float(rel.median()), 5),
                                      first=[round(float(v), 5) for v in rel[:3]], last=[round(float(v), 5) for v in rel[-3:]],
                                      step_of_max=int(rel.argmax()))
    if args.distance:  # how far the fixed-grid solves end from the adaptive one (RK45 at --rtol / --atol), same start state
        z = torch.from_numpy(synth.synth_noise("ode_bench.distance", tuple(mix_norm.shape[:1]) + (2, args.T))).cuda()
        x_T = ops.sde_prior(MIX, mix_norm, z)
        ref, rinfo = engines[0].ode_sample(mix_norm, MIX, rtol=args.rtol, atol=args.atol, max_nfe=args.max_nfe, denoise=False,
                                           x_init=x_T)
        dist = dict(rk45_nfev=rinfo["nfev"], rk45_status=rinfo["status"])
        for method in ("ddim", "dpmpp2m", "heun"):
            for M in (32, 64, 128):
                out, _ = engines[0].ode_sample_fixed(mix_norm, MIX, method=method, steps=M, denoise=False, x_init=x_T)
                d = (out.double() - ref.double()).pow(2).mean().sqrt() / ref.double().pow(2).mean().sqrt()
                dist[f"{method}{M}"] = round(float(d), 5)
        res["distance_rel_rms"] = dist
    if K > 1:
        for e in engines:
            e.set_option("rw_quarter", 1)  # the throughput mode of the CLIs (DiffSepModel.set_throughput_mode)
        ring = {k: [] for k in runs}
        for rep_ in range(1 + max(1, args.reps)):  # (the first round warms the new option's graphs up and is dropped)
            for k, (fn, _) in runs.items():
                r = inflight.Ring(streams, lambda w, j, g: fn(engines[w]), lambda w, item: None)
                _, w = timed(lambda: r.run(list(range(args.batches))))
                if rep_:
                    ring[k].append(w)
        for k, (_, evals) in runs.items():
            ws = sorted(ring[k])
            med = ws[len(ws) // 2]
            res[k + "_inflight"] = dict(wall_per_batch_ms=round(med * 1e3 / args.batches, 2), batches_per_s=round(args.batches / med, 3),
                                        min_ms=round(ws[0] * 1e3 / args.batches, 2), max_ms=round(ws[-1] * 1e3 / args.batches, 2),
                                        ms_per_eval=round(med * 1e3 / args.batches / evals, 4))
    print(json.dumps(res), flush=True)
    for e in engines:
        e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nf", type=int, default=64)
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--T", type=int, default=32000)
    ap.add_argument("--rtol", type=float, default=1e-5)
    ap.add_argument("--atol", type=float, default=1e-5)
    ap.add_argument("--max-nfe", type=int, default=600)
    ap.add_argument("--dtypes", default="f32,split,f16")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--pc-steps", type=int, default=30)
    ap.add_argument("--each", action="store_true", help="one ode_sample_each call against the sum of B calls at B = 1")
    ap.add_argument("--fixed", action="store_true", help="the fixed-step sampler next to the PC sampler, alone and in flight")
    ap.add_argument("--streams", type=int, default=4, help="--fixed: engines / streams in flight")
    ap.add_argument("--batches", type=int, default=12, help="--fixed: batches per in-flight run")
    ap.add_argument("--distance", action="store_true",
                    help="--fixed: also the rel RMS distance of ddim / dpmpp2m / heun at M = 32, 64, 128 from the adaptive solve")
    args = ap.parse_args()
    torch.set_grad_enabled(False)
    mix = torch.from_numpy(synth.synth_batch(args.B, T=args.T)[0]).cuda()
    mix_norm, _, _ = ops.normalize_batch(mix)
    sd = None
    for name in args.dtypes.split(","):
        cfg = _lib.model_config(nf=args.nf, num_sources=2, dtype=DTYPES[name])
        if sd is None:
            sd = synth.synth_state_dict([(n, s) for n, s, _ in param_table(cfg)], 7)
        if args.fixed:
            bench_fixed(cfg, sd, mix_norm, args, name)
            torch.cuda.empty_cache()
            continue
        eng = Engine(cfg, pack_state_dict(cfg, sd))
        if args.each:
            bench_each(eng, mix_norm, args, name)
            eng.close()
            del eng
            torch.cuda.empty_cache()
            continue
        # one evaluation of this plan, graph-replayed: PC sampler without corrector
        eng.pc_sample(mix_norm, MIX, N=args.pc_steps, corrector="none", seed=1)
        _, t_pc = timed(lambda: eng.pc_sample(mix_norm, MIX, N=args.pc_steps, corrector="none", seed=1))
        t_nfe = t_pc / args.pc_steps
        run = lambda: eng.ode_sample(mix_norm, MIX, rtol=args.rtol, atol=args.atol, max_nfe=args.max_nfe, seed=3)  # noqa
        (out, info) = run()
        walls = []
        for _ in range(max(1, args.reps)):
            (out, info), w = timed(run)
            walls.append(w)
        wall = sorted(walls)[len(walls) // 2]
        outside = 1.0 - (info["nfev"] + 1) * t_nfe / wall
        print(json.dumps(dict(dtype=name, nf=args.nf, B=args.B, T=args.T, rtol=args.rtol, atol=args.atol,
                              max_nfe=args.max_nfe, **info, finite=bool(torch.isfinite(out).all()),
                              wall_ms=round(wall * 1e3, 1), ms_per_nfe=round(t_nfe * 1e3, 3),
                              share_outside_nfe=round(outside, 4), walls_ms=[round(w * 1e3, 1) for w in walls])),
              flush=True)
        eng.close()
        del eng
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
