"""numpy float64 restatement of the exponential-integrator solve (DDIM, DPM-Solver++ 2M) for MixSDE / PriorMixSDE, written from
the definitions in include/diffsep_hip.h: the per-step coefficient table and the pass in its stated operation order.  Shared by
tests/test_expint_cpu.py and tests/test_expint_gpu.py; it calls nothing of the library."""
import numpy as np

CX_A, CD_A, W0_A, W1_A, CX_P, CD_P, W0_P, W1_P, AL_A, EV_A, AL_P, EV_P = range(12)
METHODS = {"ddim": 0, "dpmpp2m": 1}


def params(sde):
    """(d_lambda, sigma_min, sigma_max) as the library sees them: the C struct holds floats, widened as they are"""
    return tuple(float(np.float32(sde[k])) for k in ("d_lambda", "sigma_min", "sigma_max"))


def eig(sde, t):
    """ev1, ev2 of MixSDE._cov_eigval in float64"""
    lam, smin, smax = params(sde)
    r = smax / smin
    mult = smin * smin
    srp = r ** (2 * t)
    return mult * (srp - 1), mult * (srp - np.exp(-2.0 * lam * t)) / (1.0 + lam / np.log(r))


def alphas(sde, t):
    return np.exp(-0.0 * t), np.exp(-params(sde)[0] * t)


def g2(sde, t):
    """g(t)^2 of MixSDE.sde: (sigma_min r^t sqrt(2 ln r))^2"""
    _, smin, smax = params(sde)
    r = smax / smin
    return (smin * r ** t) ** 2 * 2 * np.log(r)


def uniform_grid(M, t0=1.0, eps=0.03):
    """the entry's own grid: t_i = t0 + (eps - t0) i / M for i < M, t_M = eps"""
    return np.array([t0 + (eps - t0) * i / M for i in range(M)] + [eps])


def log_grid(M, t0=1.0, eps=0.03):
    ts = np.logspace(np.log10(t0), np.log10(eps), M + 1)
    ts[0], ts[-1] = t0, eps
    return ts


def table(sde, method, ts):
    """[M, 12]: cx cd w0 w1 of eigenspace A, of eigenspace P, then alpha_A ev_A alpha_P ev_P at t_i"""
    ts = np.asarray(ts, np.float64)
    M = len(ts) - 1
    out = np.zeros((M, 12))
    ev = np.array([eig(sde, t) for t in ts])        # [M + 1, 2]
    al = np.array([alphas(sde, t) for t in ts])
    lam = np.log(al) - 0.5 * np.log(ev)
    for i in range(M):
        for j in range(2):
            h = lam[i + 1, j] - lam[i, j]
            w0, w1 = 1.0, 0.0
            if method == "dpmpp2m" and i >= 1:
                r = (lam[i, j] - lam[i - 1, j]) / h
                w0, w1 = 1.0 + 1.0 / (2.0 * r), -1.0 / (2.0 * r)
            out[i, 4 * j:4 * j + 4] = np.sqrt(ev[i + 1, j] / ev[i, j]), -al[i + 1, j] * np.expm1(-h), w0, w1
            out[i, AL_A + 2 * j], out[i, EV_A + 2 * j] = al[i, j], ev[i, j]
    return out


def _mean(a):
    """sum over the sources in the order s = 0, 1, ..., then one division by S (axis -2 of [..., S, T])"""
    acc = a[..., 0, :]
    for s in range(1, a.shape[-2]):
        acc = acc + a[..., s, :]
    return (acc / float(a.shape[-2]))[..., None, :]


def step(y, score, c, x0_prev=None, sigma_mix=None):
    """One pass in the operation order the kernel states.  y float64 [..., S, T], score float32 or float64 [..., S, T], c: one row
    of the table, x0_prev: float64 or None, sigma_mix float32 [..., T] or None.  -> (X0, y_new, d): d = step minus its DDIM
    step as the trace forms it (zeros without a previous X0)."""
    y = np.asarray(y, np.float64)
    sc = np.asarray(score).astype(np.float64)
    mx, ms = _mean(y), _mean(sc)
    if sigma_mix is None:
        q = 1.0
    else:
        sm = np.asarray(sigma_mix).astype(np.float64)[..., None, :]
        q = sm * sm
    eA, eP = c[EV_A] * q, c[EV_P] * q
    xa = (mx + eA * ms) / c[AL_A]
    x0 = xa + ((y - mx) + eP * (sc - ms)) / c[AL_P]
    mn = _mean(x0)
    dA = c[W0_A] * mn
    dP = c[W0_P] * (x0 - mn)
    d = np.zeros_like(y)
    if x0_prev is not None:
        mp = _mean(x0_prev)
        dA = dA + c[W1_A] * mp
        dP = dP + c[W1_P] * (x0_prev - mp)
        ga, gp = c[CD_A] * (c[W0_A] - 1.0), c[CD_P] * (c[W0_P] - 1.0)
        d = ga * (mn - mp) + gp * ((x0 - mn) - (x0_prev - mp))
    ya = c[CX_A] * mx + c[CD_A] * dA
    return x0, ya + (c[CX_P] * (y - mx) + c[CD_P] * dP), d


def solve(score_fn, y, tab, ts, method):
    """walk the table: score_fn(t_i, y) -> score; -> (final y, [(y_i, d_i) per step])"""
    x0_prev, trace = None, []
    for i in range(len(ts) - 1):
        x0, y_new, d = step(y, score_fn(ts[i], y), tab[i], x0_prev if (method == "dpmpp2m" and i >= 1) else None)
        trace.append((y, d))
        y, x0_prev = y_new, x0
    return y, trace
