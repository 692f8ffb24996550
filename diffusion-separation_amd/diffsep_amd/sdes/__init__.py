"""Sampler factories with the reference signatures (sdes/__init__.py:46-190).

get_pc_sampler(...) returns a closure `pc_sampler() -> (x, nfe[, intermediates])`; get_ode_sampler(...) returns
`ode_sampler(z=None) -> (x, nfe)`, the probability-flow ODE integrated by the engine's device-resident RK45 / RK23;
get_ode_fixed_sampler(...) the same ODE on a fixed grid at a cost known beforehand, enqueued like the PC sampler.  When score_fn is an
engine-backed model and the request is the default path (reverse_diffusion + ald2/none, no
intermediates) the whole loop runs as ONE engine call (hipGraph-replayed network evaluations, fused
update kernels, on-device Philox noise seeded from torch's generator); otherwise the generic
step-by-step loop below runs the same kernels through the predictor / corrector objects.
"""
import math

import torch

from .. import _lib

from .correctors import Corrector, CorrectorRegistry
from .predictors import Predictor, PredictorRegistry, ReverseDiffusionPredictor
from .sdes import MixSDE, PriorMixSDE, SDERegistry

__all__ = ["PredictorRegistry", "CorrectorRegistry", "SDERegistry", "Predictor", "Corrector", "MixSDE", "PriorMixSDE",
           "get_pc_sampler", "get_pc_scheduled_sampler", "get_ode_sampler", "get_ode_fixed_sampler", "ode_fixed_timesteps", "sampler_timesteps", "first_step_for"]


def _timesteps(sde, eps, schedule, device):
    """None -> linspace(T, eps, N) (sdes/__init__.py:175); scheduled samplers use N+1 points
    (sdes/__init__.py:91-111) but still step with dt = 1/N (reference quirk Q1)."""
    if schedule is None:
        return torch.linspace(sde.T, eps, sde.N, device=device)
    if schedule == "linear":
        return torch.linspace(sde.T, eps, sde.N + 1, device=device)
    if schedule == "log":
        return torch.logspace(math.log10(sde.T), math.log10(eps), sde.N + 1, base=10, device=device)
    if schedule == "revlog":
        return torch.logspace(math.log10(eps), math.log10(sde.T), sde.N + 1, base=10, device=device).flip(dims=(0,))
    raise NotImplementedError(f"Schedule '{schedule}' does not exist")


def sampler_timesteps(N, eps=3e-2, schedule=None, T=1.0):
    """The float32 times ts[0 .. N) at which the N reverse steps of a sampler run (host numpy): linspace(T, eps, N), or the first N
    points of a schedule's N + 1."""
    class _G:
        pass
    g = _G()
    g.T, g.N = T, int(N)
    return _timesteps(g, eps, schedule, "cpu").to(torch.float32).numpy()[:int(N)].copy()


def first_step_for(t_start, timesteps):
    """The reverse step a warm start at diffusion time t_start begins with: the smallest i with timesteps[i] <= t_start, on the
    float32 grid the sampler uses (timesteps: the descending step times, e.g. sampler_timesteps(N, eps, schedule)); the call then
    starts AT timesteps[i], never above t_start.  t_start >= T gives 0 (the whole run); t_start below the last step time raises
    ValueError.  Pure host code."""
    import numpy as np
    ts = np.asarray(timesteps.detach().cpu().numpy() if hasattr(timesteps, "detach") else timesteps, dtype=np.float32).reshape(-1)
    if ts.size == 0:
        raise ValueError("first_step_for: an empty grid")
    t = float(t_start)
    if not t >= float(ts[-1]):
        raise ValueError(f"first_step_for: t_start = {t_start} lies below the last step time {float(ts[-1])}: no step is left to run")
    return int(np.nonzero(ts.astype(np.float64) <= t)[0][0])


def _engine_of(score_fn):
    """The engine behind a score function: an engine-backed model (diffsep_amd's DiffSepModel / ScoreModelNCSNpp), or the
    REFERENCE's DiffSepModel holding a diffsep_amd ScoreModelNCSNpp as .score_model — its forward is nothing but
    `self.score_model(xt, time, mix)` (pl_model.py:407-409), so the fused sampler computes the same thing."""
    eng = getattr(score_fn, "engine", None)
    if eng is None:
        eng = getattr(getattr(score_fn, "score_model", None), "engine", None)
    return eng() if callable(eng) else eng


class _HybridScore:
    """score_fn of the step-by-step loop on a dtype="hybrid" model: the split-precision head model while .head is set (the
    first head_steps reverse steps), the 16-bit model after — the schedule the fused sampler runs inside one engine call."""

    def __init__(self, model):
        self.model, self.head, self.head_steps = model, True, int(getattr(model, "head_steps", 0))

    def __call__(self, xt, t, mix):
        return (self.model.tail_model if self.head else self.model.score_model)(xt, t, mix)


def _make_sampler(predictor_name, corrector_name, sde, score_fn, y, true_mean, denoise, eps, snr, corrector_steps,
                  probability_flow, intermediate, schedule, seed=None, lengths=None, seeds=None, snapshots=None, target=None,
                  x_init=None, first_step=0, last_step=None):
    predictor = PredictorRegistry.get_by_name(predictor_name)(sde, score_fn, probability_flow=probability_flow)
    corrector = CorrectorRegistry.get_by_name(corrector_name)(sde, score_fn, snr=snr, n_steps=corrector_steps)
    eng = _engine_of(score_fn)
    fused = (eng is not None and not intermediate and true_mean is None
             and predictor_name in ("reverse_diffusion", "euler_maruyama", "none")
             and corrector_name in ("ald2", "ald", "langevin", "none") and isinstance(sde, MixSDE)
             and not (corrector_name == "ald" and type(sde) is not MixSDE))

    traced = snapshots is not None or target is not None
    # both ends open, on either path: the steps [first, last) of the N-point grid, from x_init
    first, last = int(first_step), int(sde.N if last_step is None else last_step)
    if not 0 <= first < last <= sde.N:
        raise ValueError(f"the step range must satisfy 0 <= first_step < last_step <= N, got [{first}, {last}) of {sde.N}")
    if first > 0 and x_init is None:
        raise ValueError("first_step > 0 needs the state to start from (x_init=)")
    if not fused and (seed is not None or lengths is not None or seeds is not None or traced):
        # the step-by-step loop draws from torch's global generator like the reference (torch.manual_seed governs it),
        # has no notion of a zero-padded batch, and hands its states out itself (intermediate=True)
        raise ValueError("seed= / seeds= / lengths= / snapshots= / target= are extensions of the fused engine sampler; this request "
                         "(intermediate, true_mean or a user predictor / corrector) runs the generic loop")

    # dtype="hybrid" outside the fused sampler (intermediate=True, true_mean, a user-written predictor / corrector — calls the
    # reference supports on any model): the step-by-step loop keeps the schedule — the score of the first head_steps reverse
    # steps comes from the model's split-precision engine, the rest from its 16-bit engine — through a score function that
    # the loop switches per step.
    hybrid = None
    if not fused and getattr(score_fn, "tail_engine", lambda: None)() is not None:
        hybrid = _HybridScore(score_fn)
        predictor = PredictorRegistry.get_by_name(predictor_name)(sde, hybrid, probability_flow=probability_flow)
        corrector = CorrectorRegistry.get_by_name(corrector_name)(sde, hybrid, snr=snr, n_steps=corrector_steps)

    def pc_sampler():
        with torch.no_grad():
            ns = (last - first) * (corrector.n_steps + 1)
            if fused:
                # torch.manual_seed() governs reproducibility; seed=... (an extension) fixes the device RNG seed of
                # this sampler explicitly, e.g. when several samplers are driven from different threads
                s_ = int(torch.randint(0, 2 ** 62, (1,)).item()) if seed is None else int(seed)
                ts = None if schedule is None else _timesteps(sde, eps, schedule, "cpu").numpy()
                tail = getattr(score_fn, "tail_engine", lambda: None)()
                x, _, *tr = eng.pc_sample(y, sde.engine_config(), N=sde.N, corrector_steps=corrector.n_steps, snr=snr,
                                          eps=eps, denoise=denoise, predictor=predictor_name, corrector=corrector_name,
                                          seed=s_, timesteps=ts, lengths=lengths, seeds=seeds, tail=tail,
                                          head_steps=getattr(score_fn, "head_steps", 0) if tail is not None else 0,
                                          snapshots=snapshots, target=target, x_init=x_init, first_step=first,
                                          last_step=last if (last < sde.N or first > 0 or x_init is not None) else None)
                if traced:  # the tap of the fused sampler: the requested steps in the shape of `intermediate`
                    pc_sampler.trace = tr[0]
                    return x, ns, tr[0].intermediates()
                return x, ns
            im = []
            if x_init is not None:  # (no draw for the prior)
                xt = x_init
            else:
                xt = sde.prior_sampling((true_mean if true_mean is not None else y).shape,
                                        true_mean if true_mean is not None else y)
            ts = _timesteps(sde, eps, schedule, y.device)
            xt_mean = xt
            for i in range(first, last):
                if hybrid is not None:
                    hybrid.head = i < hybrid.head_steps
                vec_t = torch.ones(y.shape[0], device=y.device) * ts[i]
                xt, xt_mean = corrector.update_fn(xt, vec_t, y)
                if intermediate:
                    im.append((xt, xt_mean))
                xt, xt_mean = predictor.update_fn(xt, vec_t, y)
            res = xt_mean if (denoise and last == sde.N) else xt  # (a run that stops early hands out the state itself)
            return (res, ns, im) if intermediate else (res, ns)

    pc_sampler.trace = None
    return pc_sampler


def get_pc_sampler(predictor_name, corrector_name, sde, score_fn, y, true_mean=None, denoise=True, eps=3e-2, snr=0.1,
                   corrector_steps=1, probability_flow=False, intermediate=False, **kwargs):
    """Reference: sdes/__init__.py:132-190.  Extensions through **kwargs (fused engine path only): seed, and for a
    zero-padded batch of utterances of different lengths lengths=[B] (+ seeds=[B], per-utterance RNG seeds); snapshots=
    (a strictly ascending list of reverse steps, or "all") and / or target= ([B,S,T], zero beyond each length) trace the fused
    sampler (Engine.pc_sample): it then returns (x, ns, im), im = [(xt, xt_mean)] of the requested steps as intermediate=True
    would list them, and pc_sampler.trace (an engine.SamplerTrace) holds the steps and the Gram rows against the target.
    On BOTH paths (the fused call and the step-by-step loop, so a user-written predictor or corrector too): x_init= ([B,S,T], the
    state to start from: no prior sample is drawn), first_step= / last_step= (only the reverse steps [first_step, last_step) of
    the N-point grid run, each at its own time and with dt = 1/N; a run that stops before N returns the state x; ns counts the
    executed steps).  first_step_for(t_start, sampler_timesteps(N, eps)) turns a diffusion time into a step."""
    return _make_sampler(predictor_name, corrector_name, sde, score_fn, y, true_mean, denoise, eps, snr,
                         corrector_steps, probability_flow, intermediate, None, seed=kwargs.get("seed"),
                         lengths=kwargs.get("lengths"), seeds=kwargs.get("seeds"), snapshots=kwargs.get("snapshots"),
                         target=kwargs.get("target"), x_init=kwargs.get("x_init"), first_step=kwargs.get("first_step", 0),
                         last_step=kwargs.get("last_step"))


def get_pc_scheduled_sampler(predictor_name, corrector_name, sde, score_fn, y, denoise=True, true_mean=None, eps=3e-2,
                             snr=0.1, corrector_steps=1, probability_flow=False, intermediate=False,
                             schedule="linear", **kwargs):
    """Reference: sdes/__init__.py:46-129.  The extensions through **kwargs are get_pc_sampler's."""
    return _make_sampler(predictor_name, corrector_name, sde, score_fn, y, true_mean, denoise, eps, snr,
                         corrector_steps, probability_flow, intermediate, schedule, seed=kwargs.get("seed"),
                         lengths=kwargs.get("lengths"), seeds=kwargs.get("seeds"), snapshots=kwargs.get("snapshots"),
                         target=kwargs.get("target"), x_init=kwargs.get("x_init"), first_step=kwargs.get("first_step", 0),
                         last_step=kwargs.get("last_step"))


_ODE_KWARGS = ("first_step", "max_step", "max_nfe", "seed", "noise", "per_utterance", "lengths", "seeds")


def get_ode_sampler(sde, score_fn, y, inverse_scaler=None, denoise=True, rtol=1e-5, atol=1e-5, method="RK45", eps=3e-2,
                    device="cuda", **kwargs):
    """Reference: sdes/__init__.py:193-278 — the probability-flow ODE dx/dt = f(x,t) - 0.5 G(t)^2 score(x,t,y)
    (RSDE.sde with probability_flow=True) from t = sde.T down to eps with scipy's solve_ivp(method), then (denoise) one
    reverse_diffusion predictor step at eps without noise, its x_mean.  Here the whole solve is ONE engine call
    (Engine.ode_sample): scipy's RK45 / RK23 controller on the host, the state [B,S,T] real and resident on the device
    (fp64 solver state, fp32 network drift), every network evaluation a replayed hipGraph.  The batch is one ODE system
    with one error norm and one step size, as in the reference.  Differences from the reference:
    its ode_func reshapes the state to y.shape ([B,1,T], Q11) and casts it to complex64 (Q12), which makes it fail on
    DiffSep; neither is reproduced.

    method: "RK45" / "RK23" (other solve_ivp methods raise NotImplementedError); device: accepted and ignored.
    **kwargs: solve_ivp's first_step / max_step, and the extensions max_nfe (no step attempt starts that would take the
    evaluation count above it), seed (device RNG seed of the prior draw; default: drawn from torch's generator),
    noise ([B,S,T] draws of the prior) and per_utterance / lengths / seeds (below).  Anything else raises TypeError.

    Cost: every network evaluation runs on the score function's engine; on a dtype="hybrid" model all of them run on its
    split-precision engine.  A 16-bit (f16 / bf16) model runs as it is, and that is costly: the score's rounding noise
    (~3e-3 relative per evaluation) enters the embedded error estimate, which can shrink the step far below what the
    fp32 drift needs at tight tolerances — bound the work with max_nfe.

    per_utterance=True (extension; implied by lengths= or seeds=) runs Engine.ode_sample_each instead: every utterance of
    the batch is its own ODE system with its own step controller, all sharing each network evaluation.  lengths [B]: y is
    a zero-padded batch of utterances that share one padded frame count; seeds [B]: per-utterance seeds of the prior draw.
    On an fp32 engine utterance b then comes out bit for bit as a B = 1 sampler on it alone with seed seeds[b], wherever
    the network evaluation itself does not depend on the batch.  The
    sampler returns (x, evals_run), the network evaluations actually run (the largest nfev), and ode_sampler.info is
    the list of the utterances' info dicts.

    The returned ode_sampler(z=None) -> (x, nfe): z [B,S,T] is used as x_T when given (the reference documents z as the
    latent code and ignores it); nfe is solve_ivp's nfev (the denoise evaluation is not counted).  After a call,
    ode_sampler.info holds nfev, n_accepted, n_rejected, status (0 reached eps, -1 step too small, 1 max_nfe) and t_final.
    """
    if method not in _lib.ODE_METHODS:
        raise NotImplementedError(f"get_ode_sampler: method '{method}' is not implemented on the engine (RK45, RK23)")
    bad = sorted(set(kwargs) - set(_ODE_KWARGS))
    if bad:
        raise TypeError(f"get_ode_sampler() got unexpected keyword argument(s) {bad} (accepted: {list(_ODE_KWARGS)})")
    if not isinstance(sde, MixSDE):
        raise TypeError("get_ode_sampler: sde must be a MixSDE / PriorMixSDE")
    tail = getattr(score_fn, "tail_engine", None)
    eng = (tail() if callable(tail) else None) or _engine_of(score_fn)
    if eng is None:
        raise ValueError("get_ode_sampler: score_fn has no engine (an engine-backed DiffSepModel / ScoreModelNCSNpp is "
                         "needed; the ODE sampler has no host fallback)")
    seed, noise_ = kwargs.get("seed"), kwargs.get("noise")
    lengths, seeds = kwargs.get("lengths"), kwargs.get("seeds")
    each = bool(kwargs.get("per_utterance", False)) or lengths is not None or seeds is not None

    def ode_sampler(z=None, **_):
        with torch.no_grad():
            s_ = int(torch.randint(0, 2 ** 62, (1,)).item()) if seed is None else int(seed)
            if each:
                x, infos, evals = eng.ode_sample_each(y, sde.engine_config(), lengths=lengths, seeds=seeds, method=method,
                                                      rtol=rtol, atol=atol, eps=eps, first_step=kwargs.get("first_step"),
                                                      max_step=kwargs.get("max_step"), max_nfe=kwargs.get("max_nfe") or 0,
                                                      denoise=denoise, N=sde.N, x_init=z,
                                                      noise=noise_ if z is None else None, seed=s_)
                ode_sampler.info = infos
                if inverse_scaler is not None:
                    x = inverse_scaler(x)
                return x, evals
            x, info = eng.ode_sample(y, sde.engine_config(), method=method, rtol=rtol, atol=atol, eps=eps,
                                     first_step=kwargs.get("first_step"), max_step=kwargs.get("max_step"),
                                     max_nfe=kwargs.get("max_nfe") or 0, denoise=denoise, N=sde.N, x_init=z,
                                     noise=noise_ if z is None else None, seed=s_)
            ode_sampler.info = info
            if inverse_scaler is not None:
                x = inverse_scaler(x)
            return x, info["nfev"]

    ode_sampler.info = None
    return ode_sampler


def ode_fixed_timesteps(steps, eps=3e-2, schedule="linear", t_start=1.0):
    """The steps + 1 float64 times of a fixed-step solve from t_start down to eps (host numpy), by the rules of the scheduled
    samplers above with sde.T -> t_start and N -> steps: "linear", "log", "revlog"."""
    class _G:
        pass
    g = _G()
    g.T, g.N = float(t_start), int(steps)
    if schedule not in ("linear", "log", "revlog"):
        raise NotImplementedError(f"Schedule '{schedule}' does not exist")
    with torch.no_grad():
        prev = torch.get_default_dtype()
        try:
            torch.set_default_dtype(torch.float64)
            ts = _timesteps(g, eps, schedule, "cpu").to(torch.float64).numpy().copy()
        finally:
            torch.set_default_dtype(prev)
    ts[0], ts[-1] = float(t_start), float(eps)  # (10 ** log10(x) is x to rounding only: the ends are the caller's numbers)
    return ts


_ODE_FIXED_KWARGS = ("seed", "noise", "lengths", "seeds", "x_init", "want_err", "timesteps")


def get_ode_fixed_sampler(sde, score_fn, y, method="heun", steps=None, schedule=None, t_start=None, denoise=True, eps=3e-2,
                          **kwargs):
    """The probability-flow ODE of get_ode_sampler on a FIXED grid (no counterpart in the reference): `steps` steps (default
    sde.N) of method "euler" (steps network evaluations), "heun" / "midpoint" (2 steps), "rk4" (4 steps) or "ab2" (two-step
    Adams-Bashforth after a Heun step: steps + 1) from t_start (None: sde.T) down to eps, then (denoise) the reverse_diffusion
    step at eps without noise.  One engine call (Engine.ode_sample_fixed) that is ENQUEUED and does not block: no error norm is
    read back, so batches can be kept in flight as with the PC sampler.  Whether such a solve separates as well as the PC
    sampler at equal cost is not known (no trained checkpoint was available when this was written): this is the instrument.

    schedule: None (the uniform grid) or "linear" / "log" / "revlog" (ode_fixed_timesteps); timesteps= gives the steps + 1
    times directly.  Further **kwargs: seed, noise ([B,S,T] prior draws), x_init ([B,S,T], the state at t_start; needed when
    t_start < sde.T — ops.warm_start builds one), lengths / seeds (a zero-padded batch, per-utterance seeds), want_err (heun,
    midpoint, ab2: the local-error trace [steps,B,2] on the device, ode_sampler.info["err"]).  On a dtype="hybrid" model
    the evaluations of the first head_steps solver steps run on its split-precision engine.
    method "ddim" / "dpmpp2m" (DESIGN.md section 5m): the exponential integrators DDIM and DPM-Solver++ 2M, which integrate the
    linear drift and the noise schedule of both eigenspaces of the SDE in closed form and discretise only the network's data
    prediction — `steps` evaluations each, everything else as above; want_err with "dpmpp2m" (the step minus its DDIM step).
    Returns ode_sampler(z=None) -> (x, nfe); z [B,S,T] is used as the start state when given."""
    if method not in _lib.ODEF_METHODS and method not in _lib.EXPINT_METHODS:
        raise NotImplementedError(f"get_ode_fixed_sampler: method '{method}' is not implemented (one of "
                                  f"{sorted(_lib.ODEF_METHODS) + sorted(_lib.EXPINT_METHODS)})")
    bad = sorted(set(kwargs) - set(_ODE_FIXED_KWARGS))
    if bad:
        raise TypeError(f"get_ode_fixed_sampler() got unexpected keyword argument(s) {bad} (accepted: {list(_ODE_FIXED_KWARGS)})")
    if not isinstance(sde, MixSDE):
        raise TypeError("get_ode_fixed_sampler: sde must be a MixSDE / PriorMixSDE")
    eng = _engine_of(score_fn)
    if eng is None:
        raise ValueError("get_ode_fixed_sampler: score_fn has no engine (an engine-backed DiffSepModel / ScoreModelNCSNpp is "
                         "needed; the fixed-step ODE sampler has no host fallback)")
    M = int(sde.N if steps is None else steps)
    ts = kwargs.get("timesteps")
    if ts is not None and schedule is not None:
        raise ValueError("get_ode_fixed_sampler: schedule= and timesteps= are alternatives")
    if schedule is not None:
        ts = ode_fixed_timesteps(M, eps, schedule, sde.T if t_start is None else t_start)
    seed = kwargs.get("seed")

    def ode_sampler(z=None, **_):
        with torch.no_grad():
            s_ = int(torch.randint(0, 2 ** 62, (1,)).item()) if seed is None else int(seed)
            x0 = z if z is not None else kwargs.get("x_init")
            tail = getattr(score_fn, "tail_engine", lambda: None)()
            x, info = eng.ode_sample_fixed(y, sde.engine_config(), method=method, steps=M, t_start=t_start, eps=eps,
                                           timesteps=ts, denoise=denoise, N=sde.N, x_init=x0,
                                           noise=kwargs.get("noise") if x0 is None else None, seed=s_,
                                           lengths=kwargs.get("lengths"), seeds=kwargs.get("seeds"), tail=tail,
                                           head_steps=getattr(score_fn, "head_steps", 0) if tail is not None else 0,
                                           want_err=bool(kwargs.get("want_err", False)))
            ode_sampler.info = info
            return x, info["nfe"]

    ode_sampler.info = None
    return ode_sampler
