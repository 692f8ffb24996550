"""One sha256 per output of every entry point that ends in a fixed-order float64 reduction (csrc/reduce_device.h), on fixed
seeded inputs at small shapes: run it on two builds of the library and compare the lists.

    python tools/reduce_ab.py [--out digests.txt]

Public ops / Engine API only, so the same file runs against an older tree (copy it there, or point DIFFSEP_LIB /
DIFFSEP_LIB_F16 at that tree's libraries).  Cases: stoi (fs 8000 / 16000, STOI and ESTOI) and composite (fs 8000 / 16000, with
frames) on B = 3, S = 2 with mixed lengths and a swapped perm; gram, normalize_batch, scale_output, sde_langevin_update;
ode_error_norm and ode_error_norm_each (RK45 error row); score_loss_reduce in each PIT mode at S = 2 and 3; longform_stitch
with its cross-Gram; one pc_sample with the Langevin corrector and one ode_sample on an nf = 16 engine; and the sums of an
all -0.0 signal (the one input class on which the sign of an exactly-zero total could tell two folds of the wave totals apart).
"""
import argparse
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diffusion-separation_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from diffsep_amd import _lib, ops, synth  # noqa: E402
from diffsep_amd.engine import Engine, pack_state_dict, param_table  # noqa: E402

LINES = []


def emit(name, *tensors):
    torch.cuda.synchronize()
    for i, t in enumerate(tensors):
        a = np.ascontiguousarray(t.detach().cpu().numpy())
        LINES.append(f"{hashlib.sha256(a.tobytes()).hexdigest()}  {name}[{i}] {a.dtype} {list(a.shape)}")
        print(LINES[-1], flush=True)


def randn(seed, *shape, dtype=torch.float32):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=dtype).cuda()


def mix_sde(S):
    return dict(kind=_lib.SDE_MIX, ndim=S, d_lambda=2.0, sigma_min=0.05, sigma_max=0.5)


def pair_metrics():
    B, S = 3, 2
    perm = [[0, 1], [1, 0], [1, 0]]
    for fs in (8000, 16000):
        T = 12000
        ref = np.stack([synth.synth_mixture(i, T=T, fs=fs, n_src=S)[1] for i in range(B)]).astype(np.float32)
        est = (ref[:, ::-1] + 0.3 * randn(fs, B, S, T).cpu().numpy()).astype(np.float32)
        ref_d, est_d = torch.from_numpy(ref).cuda(), torch.from_numpy(np.ascontiguousarray(est)).cuda()
        lens = [T, 9001, 7000]
        for extended in (True, False):
            emit(f"stoi fs={fs} extended={extended}", ops.stoi(ref_d, est_d, fs, extended=extended, lengths=lens, perm=perm))
        T = 8000
        out, fr = ops.composite(ref_d[..., :T], est_d[..., :T], fs=fs, lengths=[T, 6001, 5000], perm=perm, frames=True)
        emit(f"composite fs={fs}", out, fr)


def sde_sums():
    B, S, T = 3, 2, 3000
    ref, est = randn(1, B, S, T), randn(2, B, S, T)
    emit("gram", ops.gram(ref, est))
    mix = randn(3, B, 1, T) * 0.1 + 0.01
    emit("normalize_batch", *ops.normalize_batch(mix))
    emit("scale_output", ops.scale_output(mix, est))
    emit("sde_langevin_update", *ops.sde_langevin_update(0.5, ref, est, randn(4, B, S, T)))
    nz = torch.full((B, S, T), -0.0, device="cuda")
    emit("gram of -0.0 and +0.0", ops.gram(nz, torch.zeros_like(nz)))  # every addend of ref est^T is -0.0
    emit("normalize_batch of -0.0", *ops.normalize_batch(nz[:, :1].contiguous()))
    emit("scale_output of -0.0", ops.scale_output(nz[:, :1].contiguous(), nz))


def ode_norms():
    B, S, T = 3, 2, 4000
    K = [randn(10 + j, B, S, T) for j in range(7)]
    y = randn(20, B, S, T, dtype=torch.float64)
    y2 = y + 1e-3 * randn(21, B, S, T, dtype=torch.float64)
    E = _lib.ode_tableau("RK45")[3]
    emit("ode_error_norm", ops.ode_error_norm(mix_sde(S), K, E, -0.0123456789, y, 1e-5, 1e-5, y_new=y2))
    h, active, lens = [-0.0123456789, -0.02, -0.005], [1, 0, 1], [T, 3001, 2500]
    emit("ode_error_norm_each", ops.ode_error_norm_each(mix_sde(S), K, E, h, active, lens, y, 1e-5, 1e-5, y_new=y2))


def score_losses():
    B, T = 3, 5000
    for S in (2, 3):
        score, z, x0 = randn(30 + S, B, S, T), randn(40 + S, B, S, T), randn(50 + S, B, S, T)
        mix = x0.sum(dim=1, keepdim=True).contiguous()
        t = torch.tensor([0.1, 0.5, 0.9], device="cuda")
        for pit in (None, "true_mix", "mean0"):
            emit(f"score_loss_reduce S={S} pit={pit}",
                 *ops.score_loss_reduce(mix_sde(S), score, z, t, x0=x0, mix=mix, lengths=[T, 4001, 3000], pit=pit))


def longform():
    S, Tw, Tv, T = 3, 1024, 256, 5000
    K = len(ops.longform_plan(T, Tw, Tv))
    emit("longform_stitch", *ops.longform_stitch(randn(60, K, S, Tw), T, Tv, want_gram=True))


def samplers():
    NF, S, T, B = 16, 2, 4000, 2
    cfg = _lib.model_config(nf=NF, num_sources=S, spec_factor=0.33, dtype=_lib.F32)
    sd = synth.synth_state_dict([(n, s) for n, s, _ in param_table(cfg)], 7)
    eng = Engine(cfg, pack_state_dict(cfg, sd))
    mix = torch.from_numpy(synth.synth_batch(B, T=T)[0]).cuda()
    mix_norm = ops.normalize_batch(mix)[0]
    emit("pc_sample langevin", eng.pc_sample(mix_norm, mix_sde(S), N=2, corrector_steps=1, corrector="langevin", seed=1)[0])
    emit("ode_sample", eng.ode_sample(mix_norm, mix_sde(S), rtol=1e-3, atol=1e-3, seed=5)[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the digest list to this file")
    args = ap.parse_args()
    torch.set_grad_enabled(False)
    for case in (pair_metrics, sde_sums, ode_norms, score_losses, longform, samplers):
        case()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(LINES) + "\n")
    print(f"{len(LINES)} digests")


if __name__ == "__main__":
    main()
