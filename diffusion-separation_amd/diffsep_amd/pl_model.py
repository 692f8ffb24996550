"""DiffSepModel — inference members of the reference LightningModule (pl_model.py:95-759) re-hosted on
the HIP engine: checkpoint loading incl. the EMA swap (pl_model.py:642-670), normalize_batch (:81-92),
forward = score_fn (:407-409), get_pc_sampler (:687-759), separate (:148-164), and the forward values of the
denoising score-matching loss with validation_step / test_step (:166-247, 327-424, 429-448, 471-493, 540-573).
Backward passes, optimiser and EMA update are out of scope."""
import itertools
import math
import warnings

import torch

from . import ops, sdes
from .engine import SamplerTrace, param_table
from .score_models import ScoreModelNCSNpp
from .sdes import MixSDE, PriorMixSDE


def cfg_get(cfg, path, default=None):
    """Read 'a.b.c' from dicts / attribute objects / OmegaConf nodes alike."""
    cur = cfg
    for k in path.split("."):
        if cur is None:
            return default
        if isinstance(cur, dict):
            cur = cur.get(k, None)
        else:
            try:
                cur = cur[k]
            except Exception:
                cur = getattr(cur, k, None)
    return default if cur is None else cur


def normalize_batch(batch):
    """pl_model.py:81-88: mix [B,1,T] -> zero mean / unit (unbiased) std per utterance, std clamped at 1e-5.
    The reduction + scaling of the mixture run in the HIP kernel; the optional target only reuses mean/std."""
    mix, tgt = batch
    if mix.shape[1] != 1:
        raise ValueError("normalize_batch expects a single-channel mixture [B,1,T]")
    mix_n, mean, std = ops.normalize_batch(mix.contiguous().float())
    if tgt is not None:
        tgt = (tgt - mean) / std
    return (mix_n, tgt), mean, std


def denormalize_batch(x, mean, std):
    return x * std + mean


def enhancement_config(nf=128):
    """config/model/nr.yaml restated (values only): 16 kHz, nf 128, spec_factor 0.15, PriorMixSDE."""
    cfg = default_config(nf=nf, n_speakers=2, fs=16000, spec_factor=0.15)
    cfg["model"]["sde"] = {"_target_": "sdes.sdes.PriorMixSDE", "ndim": 2, "d_lambda": 2.0, "sigma_min": 0.05,
                           "sigma_max": 0.5, "N": 30}
    return cfg


def default_config(nf=64, n_speakers=2, fs=8000, spec_factor=0.33):
    """config/model/default.yaml restated as a plain dict (values only)."""
    return {"model": {
        "n_speakers": n_speakers, "fs": fs, "t_eps": 0.03,
        "score_model": {"num_sources": n_speakers,
                        "stft_args": {"n_fft": 510, "hop_length": 128, "center": True, "pad_mode": "constant"},
                        "backbone_args": {"nf": nf}, "transform": "exponent", "spec_abs_exponent": 0.5,
                        "spec_factor": spec_factor, "spec_trans_learnable": False},
        "sde": {"ndim": n_speakers, "d_lambda": 2.0, "sigma_min": 0.05, "sigma_max": 0.5, "N": 30},
        "sampler": {"N": 30, "snr": 0.5, "corrector_steps": 1}}}


# dtype="split": fp32 tensors, every matrix product as three bf16 MFMAs on the hi / lo bf16 halves of both operands
# (DIFFSEP_F32_SPLIT): 4e-5 relative RMS / >= 79 dB from the exact fp32 engine after 60 NFE at 1.9x its speed
# (tools/probes/split_probe.py) — the fast mode that meets the parity bar.
# dtype="hybrid": such a split-fp32 engine evaluates the score of the FIRST HYBRID_HEAD_STEPS reverse steps, the f16 engine
# the rest.  A score error enters the state scaled by the step size G(t)^2, which is ~100x larger at t = 1 than at
# t = 0.03, so the rounding of the EARLY steps is what separates a 16-bit trajectory from the fp32 one (measured on bf16 in
# round 2, tools/hybrid_probe.py: fp32 for the LAST 5 / 15 / 25 steps buys nothing, for the FIRST 5 / 10 / 15 it buys 9 / 14 /
# 17 dB).  With the f16 engine (tools/probes/hybrid_f16_probe.py; SI-SDR against the exact fp32 engine, mean / min dB at
# nf = 64 | nf = 128; time of one batch relative to f16 alone):
#   K = 0:  51.1 / 44.4 | 38.9 / 32.7   1.00        K = 5:  60.1 / 56.3 | 56.9 / 55.1   1.23
#   K = 2:  55.9 / 51.8 | 50.9 / 47.2   1.09        K = 7:  61.9 / 58.9 | 59.9 / 58.5   1.32
#   K = 3:  57.5 / 54.6 | 53.3 / 49.7   1.14        K = 10: 63.9 / 60.8 | 62.6 / 61.3   1.46
# (round-4 kernels.)  The criterion K = 5 was picked by — and is gated on, tests/test_fullsize_gpu.py — is >= 50 dB on EVERY
# utterance at both widths: at most 0.004 dB of SI-SDR at a 20 dB operating point, and a factor 3 inside the 1e-2 relative RMS bar
# against the CPU oracle (measured 3.2e-3 at nf = 128, T = 32000).  With the round-5 / 6 kernels (packed half-precision GroupNorm +
# SiLU in the streamed-weight convolution) K = 5 measures 59 / 54 dB at nf = 64 and 57 / 54 dB at nf = 128 (bench.py `precision`,
# `nf128.hybrid`): 1 - 2 dB under the table, same side of the criterion; K = 3 would not be (49.7 dB minimum at nf = 128 already with
# the round-4 kernels).
HYBRID_HEAD_STEPS = 5


class DiffSepModel:
    def __init__(self, config, dtype="auto", device=None, init_seed=0, head_steps=None):
        """dtype: "auto" (default) = "f16" for backbones up to nf = 64 and "hybrid" for wider ones — the rounding of a
        16-bit engine grows with the width (f16 alone: 50 dB from the fp32 result at nf = 64, 36 - 39 dB at the published
        nf = 128; hybrid: 60 / 57 dB at 1.23x the time); "f16" ( 16-bit tensors in IEEE half precision — the half-precision build of the library — 50 dB
        mean / 46 dB min from the fp32 result after 60 network evaluations, inside the 1e-3 RMS parity bar, at the speed of
        "bf16"), "bf16" (the same kernels on bfloat16 tensors: 32 dB / 25 dB), "f32" (exact fp32 MFMAs: parity with the
        reference to 1e-7), "split" (fp32 tensors, bf16x3 matrix products: parity to 4e-5 at twice the speed of "f32") or
        "hybrid": a "split" engine for the first head_steps reverse steps, f16 for the rest (extensions: the reference has
        one precision)."""
        self.config = config
        if dtype == "auto":
            dtype = "f16" if int(cfg_get(config, "model.score_model.backbone_args.nf", 128)) <= 64 else "hybrid"
        sm = dict(cfg_get(config, "model.score_model"))
        sm.pop("_target_", None)
        sm["stft_args"] = dict(sm["stft_args"])
        sm["backbone_args"] = {k: v for k, v in dict(sm["backbone_args"]).items()}
        self.dtype = dtype
        self.score_model = ScoreModelNCSNpp(dtype="f16" if dtype == "hybrid" else dtype, device=device,
                                            init_seed=init_seed, **sm)
        self.tail_model, self.head_steps = None, 0
        if dtype == "hybrid":
            # the split-precision head engine: the SAME parameters as score_model in another mode (a twin holds no weights)
            self.tail_model = self.score_model.twin("split", lib_kind="f16")
            self.head_steps = HYBRID_HEAD_STEPS if head_steps is None else int(head_steps)
        sd = dict(cfg_get(config, "model.sde"))
        target = str(sd.pop("_target_", "sdes.sdes.MixSDE"))
        if target.endswith("PriorMixSDE"):
            self.sde = PriorMixSDE(**sd)  # speech enhancement (config/model/nr.yaml:30-37)
        elif target.endswith("MixSDE"):
            self.sde = MixSDE(**sd)
        else:
            raise NotImplementedError(f"SDE '{target}' is not on the accelerated path (MixSDE / PriorMixSDE)")
        self.t_eps = cfg_get(config, "model.t_eps", 0.03)
        self.t_max = self.sde.T
        self.normalize_batch = normalize_batch
        self.denormalize_batch = denormalize_batch
        self.fallback_batches = 0  # sampler calls repeated on fallback_model() after non-finite samples
        # the loss members (pl_model.py:107-135), read with the reference's defaults
        self.valid_max_sep_batches = cfg_get(config, "model.valid_max_sep_batches", 1)
        self.time_sampling_strategy = cfg_get(config, "model.time_sampling_strategy", "uniform")
        self.init_hack = cfg_get(config, "model.init_hack", False)
        self.init_hack_p = cfg_get(config, "model.init_hack_p", 1.0 / self.sde.N)
        self.t_rev_init = cfg_get(config, "model.t_rev_init", 0.03)
        self.train_source_order = cfg_get(config, "model.train_source_order", "random")
        # torch.nn.MSELoss(): a scalar batch mean; reduction="none" (forced for init_hack 5 / 6 / 7): one value per utterance
        self.loss_per_utterance = self.init_hack in (5, 6, 7) or cfg_get(config, "model.loss.reduction", "mean") == "none"
        self.n_batches_est_done = 0
        self._loss_twins = {}

    # ---- checkpoint ----------------------------------------------------------------------
    @classmethod
    def load_from_checkpoint(cls, path, dtype="auto", device=None, use_ema=True, head_steps=None):
        """Lightning .ckpt / HF checkpoint.pt: {'state_dict', 'hyper_parameters': {'config'}, 'ema'}
        (pl_model.py:100,642-673).  Inference runs on the EMA shadow weights (pl_model.py:655-660)."""
        ckpt = torch.load(str(path), map_location="cpu", weights_only=False)
        config = ckpt["hyper_parameters"]["config"]
        model = cls(config, dtype=dtype, device=device, head_steps=head_steps)
        state = {k[len("score_model."):]: v for k, v in ckpt["state_dict"].items() if k.startswith("score_model.")}
        ema = ckpt.get("ema", None) if use_ema else None
        if ema is not None:
            shadow = ema["shadow_params"]
            names = ["backbone." + n for n, _, _ in param_table(model.score_model.cfg)]
            if len(shadow) == len(names) - 1:  # torch_ema tracks requires_grad params only: frozen Fourier W skipped
                names = [n for n in names if not n.endswith("all_modules.0.W")]
            if len(shadow) != len(names):
                raise ValueError(f"EMA has {len(shadow)} shadow params, model has {len(names)} parameters")
            for n, v in zip(names, shadow):
                if tuple(v.shape) != tuple(state[n].shape):
                    raise ValueError(f"EMA shadow parameter for '{n}' has shape {tuple(v.shape)}")
                state[n] = v
        model.load_state_dict(state)
        return model

    def to(self, device):
        """The device the engines live on.  The parameters stay host tensors (the engine holds the only device copy of the
        weights, repacked): this is not nn.Module.to — score_model.to(device) is, and the engines follow that as well."""
        if device != self.score_model.device:
            self.score_model.device = device
            self.score_model.weights_changed()
        # (tail_model and the fallback's score model are twins: they follow score_model's device and weights)
        return self

    def replica(self):
        """Another DiffSepModel over the SAME parameters with engines of its own (twins of score_model): what a caller that
        keeps several batches in flight on one GPU uses — one engine (weights repacked on the device + workspace) per HIP
        stream, one set of host parameters.  load_state_dict() / to() on this model reach every replica."""
        r = object.__new__(DiffSepModel)
        r.__dict__.update(self.__dict__)
        r.score_model = self.score_model.twin(self.score_model.cfg.dtype, self.score_model.lib_kind)
        r.tail_model = self.score_model.twin("split", lib_kind="f16") if self.tail_model is not None else None
        r._fallback, r.fallback_batches = None, 0
        return r

    def set_throughput_mode(self, on=True):
        """For callers with SEVERAL batches in flight on one GPU (evaluate / separate --streams K > 1, bench.py): engine option
        rw_quarter — a register-weight convolution whose blocks would get <= 4 tiles runs on a quarter of the CUs with four
        times the tiles per block, and the other batches' kernels take the rest of the chip (+2.5 % throughput at K = 4;
        one batch alone is 15 % slower in this mode, which is why it is not the engine's default).  Same arithmetic; a block's fp32
        partial sums of the GroupNorm statistics cover other tiles, so a 16-bit result moves at its own rounding level, as it does
        with the batch size (tests/test_round6_gpu.py); the fp32 / split engines are not touched."""
        self.score_model.set_engine_option("rw_quarter", int(bool(on)))
        return self

    def has_fallback(self):
        """Whether this mode has an overflow fallback at all — from the mode alone, without constructing it."""
        return self.dtype in ("f16", "fp16", "hybrid")

    def load_state_dict(self, state, strict=True):
        """Weights in the reference's score_model key layout ('backbone.all_modules....').  Every engine of the model follows:
        the hybrid head engine and the overflow fallback are twins of score_model (ScoreModelNCSNpp.twin), rebuilt from its
        parameters at their next use; the cached fallback object is dropped."""
        self.score_model.load_state_dict(state, strict=strict)
        self._fallback = None
        return self

    def fallback_model(self):
        """The parity-grade twin an f16 / hybrid run is repeated on when it returns non-finite samples: the same weights on a
        "split" engine (fp32 tensors — the range of fp32, 4e-5 from the fp32 result; a hybrid model's own head engine).  IEEE
        half precision ends at 65504 where bfloat16 and fp32 do not; an overflow anywhere in the network reaches the output as
        inf / NaN (residual trunk), which is what rerun_if_nonfinite looks for.  None for the modes without a range limit
        (bf16, f32, split).  (Round 3 fell back to bf16: finite, but 13 - 19 dB from the fp32 result at nf = 128.)"""
        if not self.has_fallback():
            return None
        if getattr(self, "_fallback", None) is None:
            fb = object.__new__(DiffSepModel)
            fb.__dict__.update(self.__dict__)
            fb.dtype, fb.tail_model, fb.head_steps, fb._fallback, fb.fallback_batches = "split", None, 0, None, 0
            fb.score_model = self.tail_model if self.tail_model is not None else self.score_model.twin("split")
            self._fallback = fb
        return self._fallback

    def rerun_if_nonfinite(self, result, rerun, what="a batch"):
        """THE overflow net of the 16-bit modes, in one place: get_pc_sampler wraps every sampler it returns in it, the
        asynchronous CLIs (evaluate, separate: several batches in flight) call it when they collect a batch.
        result = (x, nfe, ...) of a sampler of this model; rerun(fallback_model) -> the same request on the fallback.
        Finite: returned as is.  Otherwise the request is repeated on fallback_model() (counted in .fallback_batches, with
        a warning) — or FloatingPointError when the mode has no fallback or the repeat is non-finite too."""
        if bool(torch.isfinite(result[0]).all()):
            return result
        fb = self.fallback_model()
        if fb is None:
            raise FloatingPointError(f"non-finite samples for {what} (dtype {self.dtype})")
        warnings.warn(f"non-finite samples for {what} with dtype {self.dtype} (half precision overflows at 65504): "
                      f"repeating on the split-precision engine", RuntimeWarning, stacklevel=2)
        self.fallback_batches = getattr(self, "fallback_batches", 0) + 1
        again = rerun(fb)
        if not bool(torch.isfinite(again[0]).all()):
            raise FloatingPointError(f"non-finite samples for {what} on the split-precision engine too")
        return again

    def tail_engine(self):
        """the (split-)fp32 engine of dtype="hybrid" (None otherwise)"""
        return self.tail_model.engine() if self.tail_model is not None and self.head_steps > 0 else None

    def eval(self, no_ema=False):
        return self

    def engine(self):
        return self.score_model.engine()

    # ---- score function --------------------------------------------------------------------
    def forward(self, xt, time, mix):
        return self.score_model(xt, time, mix)

    __call__ = forward

    # ---- sampler factory (pl_model.py:687-759) ---------------------------------------------
    def get_ode_sampler(self, y, N=None, **kwargs):
        """sdes.get_ode_sampler on this model (reference sdes/__init__.py:193-278): eps defaults to t_eps, the denoise
        step's N to sde.N.  No overflow rerun: a 16-bit model's samples come back as they are (see the docstring of
        sdes.get_ode_sampler for the cost of 16-bit engines; dtype="hybrid" runs every evaluation on its split engine)."""
        sde = self.sde.copy()
        sde.N = self.sde.N if N is None else N
        kwargs = {"eps": self.t_eps, **kwargs}
        return sdes.get_ode_sampler(sde, self, y, **kwargs)

    def get_ode_fixed_sampler(self, y, N=None, check_finite=True, **kwargs):
        """sdes.get_ode_fixed_sampler on this model (extension): the probability-flow ODE on a fixed grid,
        one enqueued engine call of known cost.  eps defaults to t_eps, steps to the sampler's N, which is also the denoise
        step's N.  check_finite: as in get_pc_sampler — the overflow net of the 16-bit modes; a caller that keeps batches in
        flight passes False and calls rerun_if_nonfinite when it collects one."""
        sde = self.sde.copy()
        sde.N = self.sde.N if N is None else N
        kwargs = {"eps": self.t_eps, **kwargs}
        inner = sdes.get_ode_fixed_sampler(sde, self, y, **kwargs)
        if not check_finite or not self.has_fallback():
            return inner

        def checked(z=None, **_):
            def rerun(fb):
                again = sdes.get_ode_fixed_sampler(sde, fb, y, **kwargs)
                result = again(z)
                checked.info = again.info
                return result

            result = inner(z)
            checked.info = inner.info
            return self.rerun_if_nonfinite(result, rerun)

        checked.info = None
        return checked

    def get_pc_sampler(self, predictor_name, corrector_name, y, N=None, minibatch=None, schedule=None, check_finite=True,
                       **kwargs):
        """check_finite (extension): the returned sampler looks at its samples and repeats the request on fallback_model()
        when an f16 / hybrid run overflowed (rerun_if_nonfinite).  That look synchronises with the sampler's stream: a caller
        that keeps several batches in flight passes check_finite=False and calls rerun_if_nonfinite when it collects one.
        The tracing extensions snapshots= / target= of sdes.get_pc_sampler pass through: the returned sampler's .trace is the
        trace of its last call (with minibatch=: the minibatches' traces joined along the batch, and the third result the
        joined [(xt, xt_mean)]); an overflow re-run repeats the request with the same trace arguments and its trace replaces
        the first one.  So do x_init= / first_step= / last_step= (both ends of the sampler open): with
        minibatch= x_init is split along the batch, and an overflow re-run repeats the request with the same x_init."""
        sde = self.sde.copy()
        sde.N = self.sde.N if N is None else N
        kwargs = {"eps": self.t_eps, **kwargs}

        def make_on(model, y_part, kw):
            if schedule is None:
                return sdes.get_pc_sampler(predictor_name, corrector_name, sde=sde, score_fn=model, y=y_part, **kw)
            return sdes.get_pc_scheduled_sampler(predictor_name, corrector_name, sde=sde, score_fn=model, y=y_part,
                                                 schedule=schedule, **kw)

        def make(y_part, kw):
            inner = make_on(self, y_part, kw)
            if not check_finite or not self.has_fallback():  # (decided from the mode: the fallback is BUILT at the first overflow)
                return inner

            def rerun(fb):
                again = make_on(fb, y_part, kw)
                result = again()
                checked.trace = getattr(again, "trace", None)
                return result

            def checked():
                result = inner()
                checked.trace = getattr(inner, "trace", None)
                return self.rerun_if_nonfinite(result, rerun)

            checked.trace = None
            return checked

        if minibatch is None:
            return make(y, kwargs)

        seed0 = kwargs.pop("seed", None)
        if kwargs.get("lengths") is not None or kwargs.get("seeds") is not None:
            raise ValueError("lengths= / seeds= describe one engine batch; they cannot be combined with minibatch=")
        target, x_init = kwargs.get("target"), kwargs.get("x_init")

        def batched_sampling_fn():
            samples, ns, inter, traces = [], [], [], []
            for i in range(int(math.ceil(y.shape[0] / minibatch))):
                part = slice(i * minibatch, (i + 1) * minibatch)
                kw = dict(kwargs)
                # an explicit seed is advanced per minibatch: the same seed would give every minibatch of the same
                # shape the same device noise
                if seed0 is not None:
                    kw["seed"] = (int(seed0) + 0x9E3779B97F4A7C15 * i) % (1 << 64)
                if target is not None:
                    kw["target"] = target[part]
                if x_init is not None:
                    kw["x_init"] = x_init[part]
                sampler = make(y[part], kw)
                sample, n, *other = sampler()
                samples.append(sample)
                ns.append(n)
                if getattr(sampler, "trace", None) is not None:
                    traces.append(sampler.trace)
                elif other:
                    inter.append(other[0])
            samples = torch.cat(samples, dim=0)
            if traces:
                batched_sampling_fn.trace = SamplerTrace.cat(traces)
                return samples, ns, batched_sampling_fn.trace.intermediates()
            return (samples, ns, inter) if inter else (samples, ns)

        batched_sampling_fn.trace = None
        return batched_sampling_fn

    def separate(self, mix, sampler="pc", **kwargs):
        """sampler="pc" (the reference's call) or "ode-fixed" (extension: the fixed-step probability-flow solve; method=,
        steps=, schedule=, seed= ... of get_ode_fixed_sampler)"""
        (mix_n, _), mean, std = self.normalize_batch((mix, None))
        if sampler == "ode-fixed":
            est, _ = self.get_ode_fixed_sampler(mix_n, **kwargs)()
            return self.denormalize_batch(est, mean, std)
        if sampler != "pc":
            raise ValueError(f"separate: sampler must be 'pc' or 'ode-fixed', got '{sampler}'")
        skw = dict(cfg_get(self.config, "model.sampler", {}))
        skw.update(kwargs)
        est, *others = self.get_pc_sampler("reverse_diffusion", "ald2", mix_n, **skw)()
        return self.denormalize_batch(est, mean, std)

    def refine(self, mix, est, t_start=0.5, lengths=None, seeds=None, scale="ls", mean_from="mix", check_finite=True,
               sampler="pc", method="heun", steps=None, **sampler_kwargs):
        """Refine another separator's estimates (extension): est [B,S,T] is diffused forward to the step
        time ts[first] nearest below t_start with the SDE's own marginal (ops.warm_start: least-squares gains per file with
        scale "ls", the source average taken from the mixture with mean_from "mix"), and only the reverse steps [first, N) of the
        fused sampler run — (N - first) (corrector_steps + 1) network evaluations instead of N (corrector_steps + 1).  Per file
        it does what separate.separate_on_device does: mix [B,1,T] (a right-zero-padded batch of files of `lengths`) is
        normalised over each file's own samples, the result rescaled per file (separate.py:73-78).  seeds [B]: per-file device
        RNG seeds (default: one draw of torch's generator each); file b's perturbation is draw 0 of its seed — the prior draw of
        a full run — and its steps take the draws the full run's would.  Returns (sep [B,S,T], info): first_step, t (the start
        time), nfe, gains [B,S] float64 and fallback [B] int32 (1: the fit of that file met silent or proportional estimates
        and used gains of 1) — both left on the device, nothing is read back here.  check_finite: as in get_pc_sampler.
        sampler="ode-fixed" (DESIGN.md section 5l): a deterministic refinement — est is diffused to t_start ITSELF (no snapping to
        a step grid) and `steps` steps (default N) of `method` of the fixed-step probability-flow solve run from t_start down to
        eps (schedule= as in get_ode_fixed_sampler); info then holds t, nfe, method, steps, gains and fallback."""
        from .separate import scale_output
        if mix.dim() == 2:
            mix = mix[None]
        mix, est = mix.float().contiguous(), est.float().contiguous()
        B, _, T = mix.shape
        if tuple(est.shape) != (B, est.shape[1], T) or est.device != mix.device:
            raise ValueError("refine: est must be [B,S,T] on the mixture's device, with the mixture's B and T")
        lens = [T] * B if lengths is None else [int(L) for L in lengths]
        skw = dict(sampler_kwargs)
        N = self.sde.N if skw.get("N") is None else int(skw["N"])
        if sampler not in ("pc", "ode-fixed"):
            raise ValueError(f"refine: sampler must be 'pc' or 'ode-fixed', got '{sampler}'")
        fixed = sampler == "ode-fixed"
        if fixed:
            eps_ = skw.get("eps", self.t_eps)
            if not eps_ < float(t_start) <= self.sde.T:
                raise ValueError(f"refine: t_start = {t_start} must lie in (eps, T] = ({eps_}, {self.sde.T}]")
            first, t0 = None, float(t_start)
        else:
            ts = sdes.sampler_timesteps(N, skw.get("eps", self.t_eps), skw.get("schedule"), T=self.sde.T)
            first = sdes.first_step_for(t_start, ts)
            t0 = float(ts[first])
        mix_n = torch.zeros_like(mix)
        mean, std = (torch.empty(B, dtype=torch.float32, device=mix.device) for _ in range(2))
        for b, L in enumerate(lens):  # every file over ITS samples (pl_model.py:81-88), the tail left at zero
            (m_b, _), mu, sd = self.normalize_batch((mix[b:b + 1, :, :L], None))
            mix_n[b, :, :L], mean[b], std[b] = m_b[0], mu.reshape(()), sd.reshape(())
        if seeds is None:
            seeds = [int(torch.randint(0, 2 ** 62, (1,)).item()) for _ in range(B)]
        seeds = [int(s) for s in seeds]
        t = torch.full((B,), t0, dtype=torch.float32, device=mix.device)
        x_init, gains, fallback = ops.warm_start(self.sde, est, mix, mix_n, mean, std, t, scale=scale, mean_from=mean_from,
                                                 seeds=seeds, lengths=lens)
        if fixed:
            run = self.get_ode_fixed_sampler(mix_n, check_finite=check_finite, method=method, steps=steps, t_start=t0,
                                             **{**skw, "lengths": lens, "x_init": x_init})
            with torch.no_grad():
                sep, nfe = run()
            out = torch.zeros_like(sep)
            for b, L in enumerate(lens):
                out[b, :, :L] = scale_output(mix[b:b + 1, :, :L], sep[b:b + 1, :, :L])[0]
            return out, {"t": t0, "nfe": nfe, "method": method, "steps": run.info["steps"], "gains": gains, "fallback": fallback}
        sampler = self.get_pc_sampler("reverse_diffusion", "ald2", mix_n, check_finite=check_finite,
                                      **{**skw, "lengths": lens, "seeds": seeds, "x_init": x_init, "first_step": first})
        with torch.no_grad():
            sep, nfe, *_ = sampler()
        out = torch.zeros_like(sep)
        for b, L in enumerate(lens):
            out[b, :, :L] = scale_output(mix[b:b + 1, :, :L], sep[b:b + 1, :, :L])[0]
        return out, {"first_step": first, "t": t0, "nfe": nfe, "gains": gains, "fallback": fallback}

    def separate_long(self, mix, window, overlap, batch=16, seed=None, **sampler_kwargs):
        """A recording of any length as windows of the shape the engine is fast at (extension): mix
        [1,T] / [1,1,T] on the device is cut into the K windows of ops.longform_plan(T, window, overlap) (samples), up to
        `batch` windows share an engine call, and ops.longform_stitch aligns their source orders over the overlaps and
        cross-fades them on the device.  Every window is handled exactly as a file is (separate.separate_on_device): normalised
        over its own samples, sampled by the fused PC sampler with lengths= / seeds=, rescaled against its own stretch of the
        mixture.  Window k's device RNG seed is inflight.window_seeds(seed, K)[k]; seed None: one draw of torch's generator.
        T <= window: one window, the file through that same call.  Returns [1,S,T]; self.longform_info = {"starts", "perm"
        (device int32 [K,S]: output source i is row perm[k][i] of window k), "seeds", "K"}."""
        from . import inflight
        from .separate import separate_on_device
        if mix.dim() == 2:
            mix = mix[None]
        if mix.dim() != 3 or tuple(mix.shape[:2]) != (1, 1) or not mix.is_cuda:
            raise ValueError("separate_long: mix must be a [1,T] or [1,1,T] device tensor (one single-channel recording)")
        T = int(mix.shape[-1])
        starts = ops.longform_plan(T, window, overlap)
        K, L = len(starts), min(T, int(window))
        seeds = inflight.window_seeds(int(torch.randint(0, 2 ** 62, (1,)).item()) if seed is None else seed, K)
        batch = max(1, int(batch))
        parts = []
        for k0 in range(0, K, batch):
            ks = range(k0, min(K, k0 + batch))
            mb = torch.stack([mix[0, :, starts[k]:starts[k] + L] for k in ks])
            parts.append(separate_on_device(mb, self, sampler_kwargs, mix.device, lengths=[L] * len(ks),
                                            seeds=[seeds[k] for k in ks], check_finite=True))
        win = torch.cat(parts) if len(parts) > 1 else parts[0]
        if K == 1:
            out, perm = win, torch.arange(win.shape[1], dtype=torch.int32, device=win.device)[None]
        else:
            out, perm = ops.longform_stitch(win, T, overlap)
            out = out[None]
        self.longform_info = {"starts": starts, "perm": perm, "seeds": seeds, "K": K}
        return out

    def separate_draws(self, mix, K, lengths=None, seeds=None, out="mean", rescale=None, check_finite=True, want_std=False,
                       **sampler_kwargs):
        """K posterior draws per mixture, aligned and reduced on the device (extension).  Every call of
        the sampler is ONE random draw of the sources given the mixture, with its sources in an arbitrary order; this runs K of
        them per file in one engine call and hands back their mean (out="mean", the default), the draw nearest to the mean
        (out="medoid") or the mean together with all K draws in one source order (out="all").
        mix [F,1,T] (or [1,T]) on the device, right-zero-padded, file f being lengths[f] (default T) samples long; files of one
        call must share a padded frame count, as in every mixed-length engine call.  Each file is normalised once over its own
        samples and repeated K times in the batch; draw k of file f has the device RNG seed inflight.draw_seeds(seeds[f], K)[k]
        (seeds None: one draw of torch's generator per file), so draw 0 is what `separate` gives for the file under seeds[f].
        The rows of the fused PC sampler are first rescaled exactly as a single draw is — rescale(mix_f [1,1,n], rows
        [K,S,n]) -> [K,S,n], default: denormalize_batch with the file's mean and std, what `separate` does — and THEN aligned
        and reduced by ops.ensemble: the mean that comes back is the float64 mean of the very draws that come back, bit for
        bit.  check_finite: the overflow net of the 16-bit modes around the engine call, as in get_pc_sampler.
        Returns (estimate [F,S,T], ops.EnsembleResult) and with out="all" also the aligned draws [F,K,S,T]; tails beyond a
        length are zero.  self.draws_info = {"K", "seeds" (per file, per draw), "nfe"}."""
        from . import inflight
        if out not in ("mean", "medoid", "all"):
            raise ValueError(f"separate_draws: out = {out!r} (mean, medoid or all)")
        K = int(K)
        if not 1 <= K <= 32:
            raise ValueError(f"separate_draws: K = {K} draws (1..32)")
        if mix.dim() == 2:
            mix = mix[None]
        if mix.dim() != 3 or mix.shape[1] != 1 or not mix.is_cuda:
            raise ValueError("separate_draws: mix must be a [1,T] or [F,1,T] device tensor of single-channel mixtures")
        mix = mix.float().contiguous()
        F, _, T = mix.shape
        lengths = [T] * F if lengths is None else [int(n) for n in lengths]
        if seeds is None:
            seeds = [int(torch.randint(0, 2 ** 62, (1,)).item()) for _ in range(F)]
        if len(lengths) != F or len(seeds) != F:
            raise ValueError("separate_draws: lengths and seeds must have one entry per mixture")
        mix_n, stats = torch.zeros_like(mix), []
        for f, n in enumerate(lengths):  # every file normalised once, over ITS samples (pl_model.py:81-88)
            (m_f, _), mean, std = self.normalize_batch((mix[f:f + 1, :, :n], None))
            mix_n[f, :, :n] = m_f[0]
            stats.append((mean, std))
        dseeds = [inflight.draw_seeds(s, K) for s in seeds]
        skw = dict(cfg_get(self.config, "model.sampler", {}))
        skw.update(sampler_kwargs)
        sampler = self.get_pc_sampler("reverse_diffusion", "ald2", mix_n.repeat_interleave(K, dim=0), check_finite=check_finite,
                                      lengths=[n for n in lengths for _ in range(K)], seeds=[s for ds in dseeds for s in ds],
                                      **skw)
        with torch.no_grad():
            rows, nfe, *_ = sampler()
        draws = torch.zeros_like(rows)
        for f, n in enumerate(lengths):
            r = rows[f * K:(f + 1) * K, :, :n]
            draws[f * K:(f + 1) * K, :, :n] = self.denormalize_batch(r, *stats[f]) if rescale is None else \
                rescale(mix[f:f + 1, :, :n], r)
        draws = draws.view(F, K, *rows.shape[1:])
        res = ops.ensemble(draws, lengths=lengths, want_std=want_std, want_pick=out != "mean")
        self.draws_info = {"K": K, "seeds": dseeds, "nfe": nfe}
        if out == "all":
            return res.mean, res, res.aligned(draws)
        return (res.pick if out == "medoid" else res.mean), res

    # ---- denoising score-matching loss, forward values (pl_model.py:166-247, 327-424) --------------------------
    FORWARD_ONLY = ("the score-matching loss is implemented forward-only (diffsep_score_loss): backward passes, optimiser, EMA "
                    "update, gradient clipping and compute_score_loss_with_pit (train_source_order 'pit', init_hack 6) are "
                    "not part of this engine")

    def _loss_engine(self, dtype=None):
        """the engine the loss runs on: the model's configured precision, or (dtype=) a twin over the same parameters"""
        if dtype is None or dtype == self.dtype:
            return self.score_model.engine()
        if dtype not in self._loss_twins:
            self._loss_twins[dtype] = self.score_model.twin(dtype, lib_kind=self.score_model.engine().kind)
        return self._loss_twins[dtype].engine()

    def sample_time(self, x):
        """pl_model.py:166-177, B draws from torch's device generator"""
        n = x.shape[0]
        if self.time_sampling_strategy == "uniform":
            return x.new_zeros(n).uniform_(self.t_eps, self.t_max)
        if self.time_sampling_strategy == "varprop":
            return self.sde.sample_time_varprop(n, t_eps=self.t_eps, device=x.device)
        raise NotImplementedError(f"No sampling strategy {self.time_sampling_strategy}")

    def _prior_plan(self, target, time=None, select=None):
        """(time, beta [B] or None, redefine_z) of sample_prior for this model's init_hack (pl_model.py:192-245; every other
        value, the init_hack 5 / 6 / 7 of the train_step_init_* members among them, takes the plain branch :242-245)"""
        time = self.sample_time(target) if time is None else torch.as_tensor(time, dtype=torch.float32, device=target.device)
        T = self.sde.T
        Tm = T - self.t_rev_init
        if self.init_hack == 1:
            return time, (~(time < Tm)).float(), True
        if self.init_hack in (2, 3):
            return time, torch.clamp((time - Tm) / (T - Tm), min=0.0, max=1.0), self.init_hack == 3
        if self.init_hack == 4:
            sel = (torch.rand_like(time) < 1 / self.sde.N) if select is None else torch.as_tensor(select, device=time.device) > 0
            return torch.where(sel, torch.full_like(time, T), time), sel.float(), True
        return time, None, False

    def _seed(self):
        return int(torch.randint(0, 2 ** 62, (1,)).item())

    def sample_prior(self, mix, target, time=None, z=None, select=None):
        """(x_t, time, L, z) as the reference returns them (pl_model.py:179-247), every init_hack in {false, 1, 2, 3, 4} through
        ONE perturbation kernel (diffsep_sde_perturb); any other init_hack is the plain form, as in the reference.  time= / z= / select= inject the draws; otherwise the B-sized draws
        come from torch's device generator and z from the Philox kernel (seeded by torch's generator)."""
        mix, target = mix.float().contiguous(), target.float().contiguous()
        time, beta, redefine = self._prior_plan(target, time, select)
        smix = self.sde.sigma_mix(mix)
        x_t, z_out = ops.sde_perturb(self.sde.engine_config(), target, mix, time, z=z, sigma_mix=smix, beta=beta,
                                     redefine_z=redefine, seed=self._seed() if z is None else 0)
        return x_t, time, self.sde._std(time, mix), z_out

    def _reduce_batch(self, per_utt):
        per_utt = per_utt.float()
        return per_utt if self.loss_per_utterance else per_utt.mean()

    def compute_score_loss(self, mix, target, time=None, z=None, select=None, lengths=None, dtype=None, per_utterance=None):
        """The denoising score-matching loss mean((L score(x_t, t, mix) + z)^2) (pl_model.py:411-424) as ONE fused call:
        perturbation, one score evaluation on the engine, float64 reduction (diffsep_score_loss).  Returns what the
        reference's loss returns: a scalar batch mean for torch.nn.MSELoss(), one value per utterance for reduction="none"
        (per_utterance= overrides).  dtype= runs it on an fp32 / split twin instead of the model's configured precision.
        Measured against the fp32 engine (nf = 64, B = 16 x 4 s) the relative error of the 16-bit
        engines grows towards small t: f16 7.8e-4 at t = 1 and 2.0e-3 at t = 0.03, bf16 2.5e-3 and 8.6e-3 (largest per-utterance
        values); tests/test_score_loss_gpu.py gates them at 4e-3 / 2e-2."""
        mix, target = mix.float().contiguous(), target.float().contiguous()
        time, beta, redefine = self._prior_plan(target, time, select)
        out, _, _ = ops.score_loss(self._loss_engine(dtype), self.sde.engine_config(), mix, target, time, beta=beta, z=z,
                                   seed=self._seed() if z is None else 0, lengths=lengths, redefine_z=redefine)
        per = out[:, 0].float()
        if per_utterance is None:
            return self._reduce_batch(per)
        return per if per_utterance else per.mean()

    def _pit_loss(self, mix, target, time, z, pit, dtype):
        mix, target = mix.float().contiguous(), target.float().contiguous()
        beta = torch.ones_like(time) if pit == "true_mix" else None
        _, best, _ = ops.score_loss(self._loss_engine(dtype), self.sde.engine_config(), mix, target, time, beta=beta, z=z,
                                    seed=self._seed() if z is None else 0, pit=pit)
        return best.float()

    def compute_score_loss_init_hack_pit(self, mix, target, z=None, dtype=None):
        """pl_model.py:370-405 at t = T: min over source permutations of the loss with z_p = z0 + L^-1 (true_mix - mean_p).
        Every permutation's x_t is true_mix + L z0, so ONE score evaluation serves all S! of them (the reference runs S!)."""
        time = mix.new_ones(mix.shape[0], dtype=torch.float32) * self.sde.T
        return self._pit_loss(mix, target, time, z, "true_mix", dtype)

    @staticmethod
    def _shuffle_sources(x, perm=None):
        """shuffle_sources (pl_model.py:28-46); perm [B,S] injects the permutation"""
        if perm is None:
            perm = torch.argsort(x.new_zeros(x.shape[:2]).uniform_(), dim=1)
        perm = torch.as_tensor(perm, device=x.device).long()
        return torch.gather(x, 1, torch.broadcast_to(perm[..., None], x.shape))

    def compute_score_loss_with_pit_allthetime(self, mix, target, time=None, z=None, perm=None, dtype=None):
        """pl_model.py:327-368: x_t = mean_0 + L z0 of the shuffled target, min over permutations of the loss with
        z_p = z0 + L^-1 (mean_0 - mean_p); one score evaluation (the reference evaluates the same x_t S! times)."""
        time = self.sample_time(target) if time is None else torch.as_tensor(time, dtype=torch.float32, device=target.device)
        target = self._shuffle_sources(target.float(), perm)
        return self._pit_loss(mix, target, time, z, "mean0", dtype)

    def compute_score_loss_with_pit(self, mix, target):
        raise NotImplementedError(self.FORWARD_ONLY)

    def _train_step_init(self, mix, target, rest, pit_mask=None, **kw):
        pit = (mix.new_zeros(mix.shape[0]).uniform_() < self.init_hack_p) if pit_mask is None else \
            torch.as_tensor(pit_mask, device=mix.device).bool()
        losses = []
        if int(pit.sum()) > 0:
            losses.append(self.compute_score_loss_init_hack_pit(mix[pit], target[pit], dtype=kw.get("dtype")))
        if int(pit.sum()) != mix.shape[0]:
            losses.append(rest(mix[~pit], target[~pit]))
        return torch.cat(losses).mean()

    def train_step_init_5(self, mix, target, pit_mask=None, dtype=None):
        """the forward value of pl_model.py:429-448"""
        return self._train_step_init(mix, target, lambda m, t: self.compute_score_loss(
            m, self._shuffle_sources(t), dtype=dtype, per_utterance=True), pit_mask, dtype=dtype)

    def train_step_init_6(self, mix, target):
        raise NotImplementedError(self.FORWARD_ONLY)

    def train_step_init_7(self, mix, target, pit_mask=None, dtype=None):
        """the forward value of pl_model.py:471-493"""
        return self._train_step_init(mix, target, lambda m, t: self.compute_score_loss_with_pit_allthetime(m, t, dtype=dtype),
                                     pit_mask, dtype=dtype)

    def training_step(self, batch, batch_idx=0):
        raise NotImplementedError(self.FORWARD_ONLY)

    def on_validation_epoch_start(self):
        self.n_batches_est_done = 0

    on_test_epoch_start = on_validation_epoch_start

    def validation_step(self, batch, batch_idx=0, dataset_i=0, testing=False, **loss_kwargs):
        """pl_model.py:540-564 as forward values: returns {"val/score_loss": ...} and, for the first valid_max_sep_batches
        batches (every batch when testing), "val/si_sdr": SISDRLoss(zero_mean=True, clamp_db=30, sign_flip=True), mean-reduced,
        of the separated batch — from the Gram matrices of metrics.py (diffsep_gram).  The separation is ONE run of
        get_pc_sampler("reverse_diffusion", "ald2", ...) with the config's sampler arguments: the reference's separate()
        runs its sampler twice and returns the second, undenormalised result (quirk Q6), which is not reproduced."""
        from . import metrics
        mix, target = batch
        (mix_n, tgt_n), mean, std = self.normalize_batch((mix, target))
        if self.init_hack == 7:
            loss = self.train_step_init_7(mix_n, tgt_n)
        elif self.init_hack == 6:
            raise NotImplementedError(self.FORWARD_ONLY)
        elif self.init_hack == 5:
            loss = self.train_step_init_5(mix_n, tgt_n)
        else:
            loss = self.compute_score_loss(mix_n, tgt_n, **loss_kwargs)
        out = {"val/score_loss": loss}
        if testing or self.n_batches_est_done < self.valid_max_sep_batches:
            self.n_batches_est_done += 1
            skw = dict(cfg_get(self.config, "model.sampler", {}))
            est, *_ = self.get_pc_sampler("reverse_diffusion", "ald2", mix_n, **skw)()
            est = self.denormalize_batch(est, mean, std)
            out["val/si_sdr"] = metrics.si_sdr_loss(est, target.float(), zero_mean=True, clamp_db=30.0, sign_flip=True)
        return out

    def test_step(self, batch, batch_idx=0, dataset_i=None):
        return self.validation_step(batch, batch_idx, dataset_i=dataset_i, testing=True)
