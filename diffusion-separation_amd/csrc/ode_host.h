// ode_host.h — the host side of the probability-flow ODE sampler that needs no GPU: scipy's Butcher tableaux, what a solve
// derives from its diffsep_ode_config (OdePlan) and the adaptive step controller (OdeCtl), ported from scipy 1.15
// (integrate/_ivp/rk.py RungeKutta._step_impl, common.py select_initial_step / validate_tol, base.py OdeSolver.step, ivp.py
// solve_ivp's loop).  diffsep_ode_sample drives one OdeCtl, diffsep_ode_sample_each one per utterance (sampler.hip);
// tests/ode_ctl_main.cpp drives one on a small float64 system against scipy itself.  Below them: the plan of a fixed-step
// solve (OdeFixedPlan, diffsep_ode_sample_fixed; tests/ode_fixed_main.cpp walks it) and of an exponential-integrator solve
// (OdeExpintPlan, diffsep_ode_sample_expint; tests/expint_main.cpp walks it).  Plain C++17, no HIP.
#pragma once
#include <math.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/diffsep_hip.h"

#define DS_ODE_MAX_K 7  // Runge-Kutta stage derivatives held at once (RK45: 6 stages + FSAL)

// Butcher tableau of scipy.integrate's RK45 (method 0, Dormand-Prince) / RK23 (method 1, Bogacki-Shampine), as rk.py holds
// it: A [ns][ns] row-major, B [ns], C [ns], E [ns + 1]; any output may be null.  Returns -1 for an unknown method.
inline int ds_ode_tableau(int method, double* A, double* B, double* C, double* E, int* n_stages, int* error_order) {
  if (method == DIFFSEP_ODE_RK45) {  // Dormand-Prince 5(4)
    static const double a[6][6] = {
        {0, 0, 0, 0, 0, 0},
        {1.0 / 5, 0, 0, 0, 0, 0},
        {3.0 / 40, 9.0 / 40, 0, 0, 0, 0},
        {44.0 / 45, -56.0 / 15, 32.0 / 9, 0, 0, 0},
        {19372.0 / 6561, -25360.0 / 2187, 64448.0 / 6561, -212.0 / 729, 0, 0},
        {9017.0 / 3168, -355.0 / 33, 46732.0 / 5247, 49.0 / 176, -5103.0 / 18656, 0}};
    static const double b[6] = {35.0 / 384, 0, 500.0 / 1113, 125.0 / 192, -2187.0 / 6784, 11.0 / 84};
    static const double c[6] = {0, 1.0 / 5, 3.0 / 10, 4.0 / 5, 8.0 / 9, 1};
    static const double e[7] = {-71.0 / 57600, 0, 71.0 / 16695, -71.0 / 1920, 17253.0 / 339200, -22.0 / 525, 1.0 / 40};
    if (A) memcpy(A, a, sizeof(a));
    if (B) memcpy(B, b, sizeof(b));
    if (C) memcpy(C, c, sizeof(c));
    if (E) memcpy(E, e, sizeof(e));
    if (n_stages) *n_stages = 6;
    if (error_order) *error_order = 4;
    return 0;
  }
  if (method == DIFFSEP_ODE_RK23) {  // Bogacki-Shampine 3(2)
    static const double a[3][3] = {{0, 0, 0}, {1.0 / 2, 0, 0}, {0, 3.0 / 4, 0}};
    static const double b[3] = {2.0 / 9, 1.0 / 3, 4.0 / 9};
    static const double c[3] = {0, 1.0 / 2, 3.0 / 4};
    static const double e[4] = {5.0 / 72, -1.0 / 12, -1.0 / 9, 1.0 / 8};
    if (A) memcpy(A, a, sizeof(a));
    if (B) memcpy(B, b, sizeof(b));
    if (C) memcpy(C, c, sizeof(c));
    if (E) memcpy(E, e, sizeof(e));
    if (n_stages) *n_stages = 3;
    if (error_order) *error_order = 2;
    return 0;
  }
  return -1;
}

// What a solve derives from its diffsep_ode_config: the tableau (row s of A at A + s * DS_ODE_MAX_K), the tolerances as
// scipy uses them and the integration interval sde.T = 1 -> eps.
struct OdePlan {
  double A[DS_ODE_MAX_K * DS_ODE_MAX_K], B[DS_ODE_MAX_K], C[DS_ODE_MAX_K], E[DS_ODE_MAX_K + 1];
  int ns, eorder;
  double rtol, atol, max_step, eps;
  double t0, t_bound, dir, interval, err_exp;
  double first_step;  // <= 0: select_initial_step
  int max_nfe;        // 0: unbounded
};

// Fill and validate the plan (`who`: the entry point's name in the message); returns the message, empty when all is well.
inline std::string ode_plan_fill(OdePlan& p, const diffsep_ode_config& oc, const char* who) {
  const std::string w(who);
  memset(&p, 0, sizeof(p));
  double A0[6 * 6];
  if (ds_ode_tableau(oc.method, A0, p.B, p.C, p.E, &p.ns, &p.eorder) != 0)
    return w + ": method must be DIFFSEP_ODE_RK45 or DIFFSEP_ODE_RK23 (DOP853 / Radau / BDF / LSODA are not implemented)";
  for (int i = 0; i < p.ns; ++i)
    for (int j = 0; j < p.ns; ++j) p.A[i * DS_ODE_MAX_K + j] = A0[i * p.ns + j];
  if (!(oc.eps > 0.0 && oc.eps < 1.0)) return w + ": eps must be in (0, 1)";
  if (!(oc.atol >= 0.0 && oc.rtol >= 0.0)) return w + ": tolerances must be non-negative";
  if (!(oc.N >= 1 || !oc.denoise)) return w + ": the denoise step needs N >= 1";
  if (!(oc.max_nfe >= 0)) return w + ": max_nfe must be >= 0";
  // common.validate_tol: rtol below 100 machine epsilons is raised to it (scipy warns)
  p.rtol = std::max(oc.rtol, 100 * 2.220446049250313e-16);
  p.atol = oc.atol;
  p.max_step = (oc.max_step > 0.0) ? oc.max_step : INFINITY;
  p.eps = oc.eps;
  p.t0 = 1.0;  // sde.T = 1
  p.t_bound = oc.eps;
  p.dir = -1.0;
  p.interval = fabs(p.t_bound - p.t0);
  p.err_exp = -1.0 / (p.eorder + 1);
  p.first_step = oc.first_step;
  p.max_nfe = oc.max_nfe;
  if (!(oc.first_step <= 0.0 || oc.first_step <= p.interval))
    return w + ": first_step exceeds the interval (scipy: `first_step` exceeds bounds)";
  return std::string();
}

// One system's step controller.  The caller evaluates the right-hand side and the RMS norms; every decision is taken here:
//   while (c.begin_attempt(p)) { rk_step from c.t with c.h (stage s at c.stage_time(p, s)); c.end_attempt(p, error norm); }
struct OdeCtl {
  double t = 1.0, h_abs = 0.0, h = 0.0, t_new = 0.0, min_step = 0.0;
  int nfev = 0, n_acc = 0, n_rej = 0, status = 2;  // status 2: integrating; 0: reached t_bound; -1: step too small; 1: max_nfe
  bool new_step = true, rejected = false;

  // common.select_initial_step: h0 from d0 = norm(y0 / scale) and d1 = norm(f0 / scale) ...
  static double initial_h0(const OdePlan& p, double d0, double d1) {
    const double h0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * d0 / d1;
    return std::min(h0, p.interval);
  }
  // ... and the first h_abs from d1, h0 and norm((f1 - f0) / scale), f1 = f(t0 + h0 dir, y0 + h0 dir f0)
  void initial_step(const OdePlan& p, double d1, double norm_f1_f0, double h0) {
    const double d2 = norm_f1_f0 / h0;
    const double h1 = (d1 <= 1e-15 && d2 <= 1e-15) ? std::max(1e-6, h0 * 1e-3)
                                                   : pow(0.01 / std::max(d1, d2), 1.0 / (p.eorder + 1));
    h_abs = std::min(std::min(100 * h0, h1), std::min(p.interval, p.max_step));
  }
  // OdeSolver.step / _step_impl up to rk_step: false when the system attempts no (further) step — it had ended, or ends
  // here with status -1 or 1; otherwise h and t_new of this attempt are set.  (min_step is fixed when a step begins; the
  // two exits are tested before every attempt of it.)
  bool begin_attempt(const OdePlan& p) {
    if (status != 2) return false;
    if (new_step) {
      min_step = 10 * fabs(nextafter(t, p.dir * INFINITY) - t);
      if (h_abs > p.max_step) h_abs = p.max_step;
      else if (h_abs < min_step) h_abs = min_step;
      rejected = false;
      new_step = false;
    }
    if (h_abs < min_step) { status = -1; return false; }
    if (p.max_nfe > 0 && nfev + p.ns > p.max_nfe) { status = 1; return false; }
    h = h_abs * p.dir;
    t_new = t + h;
    if (p.dir * (t_new - p.t_bound) > 0) t_new = p.t_bound;
    h = t_new - t;
    h_abs = fabs(h);
    return true;
  }
  // the time of stage s of the attempt (s = ns: the FSAL evaluation at t + h)
  double stage_time(const OdePlan& p, int s) const { return s < p.ns ? t + p.C[s] * h : t + h; }
  // _step_impl after rk_step, with the attempt's error norm: true when the step is accepted (t advanced; status 0 at t_bound)
  bool end_attempt(const OdePlan& p, double err) {
    nfev += p.ns;
    if (err < 1) {
      double factor = err == 0 ? 10.0 : std::min(10.0, 0.9 * pow(err, p.err_exp));
      if (rejected) factor = std::min(1.0, factor);
      h_abs *= factor;
      t = t_new;
      ++n_acc;
      new_step = true;
      if (p.dir * (t - p.t_bound) >= 0) status = 0;
      return true;
    }
    h_abs *= std::max(0.2, 0.9 * pow(err, p.err_exp));
    rejected = true;
    ++n_rej;
    return false;
  }
};

// ------------------------------------------------------------------ fixed-step solves (diffsep_ode_sample_fixed)
// The same ODE on a grid the caller chooses: no error norm decides anything, so the whole solve is known before its first
// evaluation.  OdeFixedPlan is that knowledge — the grid, and the solve as a flat list of passes, one per network evaluation
// — and the driver in sampler.hip only walks it; tests/ode_fixed_main.cpp walks it on a small float64 system.
#define DS_ODEF_MAX_EVALS 16384  // steps x stages of one solve (the rows of the evaluation-time table)

struct OdeFixedConfig {  // the arguments of diffsep_ode_sample_fixed / _expint that shape the solve
  int method, steps;     // DIFFSEP_ODEF_* / DIFFSEP_EXPINT_*, M
  double t_start, eps;   // t_start <= 0: 1.0 (sde.T)
  int denoise, N;        // as diffsep_ode_config
};
using OdeExpintConfig = OdeFixedConfig;  // (the name the exponential-integrator side and its stand-alone program use)

// The grid of both fixed-grid solves: M + 1 times, strictly descending, inside (0, 1] — `timesteps` (M + 1 host times) or, with
// null, uniform from t_start to eps.  Returns the message (`who`: the entry point's name in it), empty when all is well.
// `refusal`: what the caller's method refuses of the request (its err_out rule), if anything; it ranks after the argument checks
// and before the grid's.  (The caller has bounded oc.steps from above.)
inline std::string ode_grid_fill(const OdeFixedConfig& oc, const double* timesteps, const char* who, std::vector<double>& t,
                                 const char* refusal = nullptr) {
  const std::string w(who);
  const int M = oc.steps;
  if (!(M >= 1)) return w + ": steps must be >= 1";
  if (!(oc.eps > 0.0 && oc.eps < 1.0)) return w + ": eps must be in (0, 1)";
  if (!(oc.N >= 1 || !oc.denoise)) return w + ": the denoise step needs N >= 1";
  if (refusal) return w + refusal;
  t.resize((size_t)M + 1);
  if (timesteps) {
    for (int i = 0; i <= M; ++i) t[i] = timesteps[i];
  } else {
    const double t0 = oc.t_start <= 0.0 ? 1.0 : oc.t_start;
    if (!(t0 > oc.eps)) return w + ": t_start must be above eps";
    for (int i = 0; i < M; ++i) t[i] = t0 + (oc.eps - t0) * i / M;
    t[M] = oc.eps;  // (t0 + (eps - t0) M / M rounds next to eps; the solve ends where the denoise step stands)
  }
  for (int i = 0; i <= M; ++i)
    if (!(t[i] > 0.0 && t[i] <= 1.0 && (i == 0 || t[i] < t[i - 1])))
      return w + ": the time grid must be strictly descending inside (0, 1]";
  return std::string();
}

// Explicit tableau of the one-step methods in OdePlan's layout (row s of A at A + s * DS_ODE_MAX_K) and, where the method
// has an embedded Euler step, D with  step - Euler step = h sum_j D[j] K_j  (has_d; Euler and RK4 have none).
// AB2 is no Runge-Kutta method: its first step is Heun's (this tableau), the others are built in ode_fixed_plan_fill.
inline int ds_odef_tableau(int method, double* A, double* B, double* C, double* D, int* ns, bool* has_d) {
  memset(A, 0, sizeof(double) * DS_ODE_MAX_K * DS_ODE_MAX_K);
  memset(B, 0, sizeof(double) * DS_ODE_MAX_K);
  memset(C, 0, sizeof(double) * DS_ODE_MAX_K);
  memset(D, 0, sizeof(double) * DS_ODE_MAX_K);
  *has_d = false;
  switch (method) {
    case DIFFSEP_ODEF_EULER:
      *ns = 1; B[0] = 1.0;
      return 0;
    case DIFFSEP_ODEF_HEUN:
    case DIFFSEP_ODEF_AB2:
      *ns = 2; C[1] = 1.0; A[1 * DS_ODE_MAX_K + 0] = 1.0; B[0] = 0.5; B[1] = 0.5;
      D[0] = -0.5; D[1] = 0.5; *has_d = true;
      return 0;
    case DIFFSEP_ODEF_MIDPOINT:
      *ns = 2; C[1] = 0.5; A[1 * DS_ODE_MAX_K + 0] = 0.5; B[1] = 1.0;
      D[0] = -1.0; D[1] = 1.0; *has_d = true;
      return 0;
    case DIFFSEP_ODEF_RK4:
      *ns = 4; C[1] = 0.5; C[2] = 0.5; C[3] = 1.0;
      A[1 * DS_ODE_MAX_K + 0] = 0.5; A[2 * DS_ODE_MAX_K + 1] = 0.5; A[3 * DS_ODE_MAX_K + 2] = 1.0;
      B[0] = 1.0 / 6; B[1] = 1.0 / 3; B[2] = 1.0 / 3; B[3] = 1.0 / 6;
      return 0;
  }
  return -1;
}

// One pass = what follows one network evaluation.  x is the evaluation's input (y itself at the first stage of a step):
//   K[kout] = f((float) t_eval, x)
//   mode 1:  x = fp32(y + (sum_{j < nk} c[j] K[j]) h)            the next evaluation's input
//   mode 2:  y_new = y + h sum_{j < nk} c[j] K[j]                the step; with err_nk > 0 the local-error pass
//            ||h sum_{j < err_nk} d[j] K[j]||_rms, ||y||_rms goes to slot `step`; then y <-> y_new, x = fp32(y),
//            and with swap_k01 K[0] <-> K[1] (AB2 keeps the previous step's drift in K[0])
// Sums run over j = 0, 1, ... in that order, as the device pass does.
struct OdeFixedPass {
  int step;       // the solver step the evaluation belongs to (which engine evaluates it: head_steps / tail_steps)
  double t_eval;
  int kout, mode, nk;
  double c[DS_ODE_MAX_K];
  double h;
  int err_nk;
  double d[DS_ODE_MAX_K];
  int swap_k01;
};

struct OdeFixedPlan {
  int method = 0, M = 0, n_evals = 0;
  bool has_err = false;    // the method has an embedded Euler step
  double eps = 0.0;
  int denoise = 0, N = 0;
  std::vector<double> t;   // the grid: M + 1 times, strictly descending, inside (0, 1]
  std::vector<OdeFixedPass> pass;  // n_evals passes
};

// Fill and validate (`who`: the entry point's name in the message; timesteps: M + 1 host times or null for the uniform
// grid t_start -> eps; want_err: the caller asks for the local-error trace); returns the message, empty when all is well.
inline std::string ode_fixed_plan_fill(OdeFixedPlan& p, const OdeFixedConfig& oc, const double* timesteps, bool want_err,
                                       const char* who) {
  const std::string w(who);
  p = OdeFixedPlan();
  double A[DS_ODE_MAX_K * DS_ODE_MAX_K], B[DS_ODE_MAX_K], C[DS_ODE_MAX_K], D[DS_ODE_MAX_K];
  int ns = 0;
  if (ds_odef_tableau(oc.method, A, B, C, D, &ns, &p.has_err) != 0)
    return w + ": method must be DIFFSEP_ODEF_EULER, HEUN, MIDPOINT, RK4 or AB2";
  const bool ab2 = oc.method == DIFFSEP_ODEF_AB2;
  const int M = oc.steps;
  if (!((long)M * ns <= DS_ODEF_MAX_EVALS)) return w + ": steps x stages must be <= 16384";
  const std::string bad = ode_grid_fill(oc, timesteps, who, p.t, (want_err && !p.has_err)
      ? ": err_out needs a method with an embedded Euler step (HEUN, MIDPOINT, AB2), not EULER or RK4" : nullptr);
  if (!bad.empty()) return bad;
  p.method = oc.method; p.M = M; p.eps = oc.eps; p.denoise = oc.denoise; p.N = oc.N;

  auto stage_pass = [&](int i, int s, double h) {  // the pass after stage s of Runge-Kutta step i
    OdeFixedPass q;
    memset(&q, 0, sizeof(q));
    q.step = i; q.t_eval = p.t[i] + C[s] * h; q.kout = s; q.h = h;
    if (s < ns - 1) {
      q.mode = 1; q.nk = s + 1;
      for (int j = 0; j <= s; ++j) q.c[j] = A[(s + 1) * DS_ODE_MAX_K + j];
    } else {
      q.mode = 2; q.nk = ns;
      for (int j = 0; j < ns; ++j) q.c[j] = B[j];
      if (p.has_err) { q.err_nk = ns; for (int j = 0; j < ns; ++j) q.d[j] = D[j]; }
    }
    p.pass.push_back(q);
  };
  for (int i = 0; i < M; ++i) {
    const double h = p.t[i + 1] - p.t[i];
    if (!ab2 || i == 0) {
      for (int s = 0; s < ns; ++s) stage_pass(i, s, h);
      continue;
    }
    // y_{n+1} = y_n + h_n ((1 + w/2) K_n - (w/2) K_{n-1}), w = h_n / h_{n-1}; K[0] = K_{n-1}, K[1] = K_n
    const double wr = h / (p.t[i] - p.t[i - 1]);
    OdeFixedPass q;
    memset(&q, 0, sizeof(q));
    q.step = i; q.t_eval = p.t[i]; q.kout = 1; q.mode = 2; q.nk = 2; q.h = h;
    q.c[0] = -(wr / 2); q.c[1] = 1.0 + wr / 2;
    q.err_nk = 2; q.d[0] = -(wr / 2); q.d[1] = wr / 2;
    q.swap_k01 = 1;
    p.pass.push_back(q);
  }
  p.n_evals = (int)p.pass.size();
  return std::string();
}

// ------------------------------------------------------------------ exponential integrators (diffsep_ode_sample_expint)
// DDIM and DPM-Solver++ 2M on the same grids.  A = 11^T / S and P = I - A commute with the mean matrix A + e^{-lambda t} P and
// with the perturbation's L(t) = sqrt(ev1) A + sqrt(ev2) P, so the probability-flow ODE splits into two scalar diffusions, one
// per eigenspace j in {A, P}:  alpha_A = 1, sigma_A^2 = ev1;  alpha_P = e^{-lambda t}, sigma_P^2 = ev2  (PriorMixSDE multiplies
// both sigma_j by sigma_mix[b,t]; it cancels out of every coefficient below and enters the data prediction only).  With the half
// log-SNR lam_j = ln alpha_j - 0.5 ln ev_j the linear drift and the noise schedule are integrated in closed form and only the
// network's data prediction X0 is discretised.  Everything here is float64; the SDE's float parameters are widened as they are.
#define DS_EXPINT_COEFS DIFFSEP_EXPINT_COEFS
enum {  // one row of the table: step i, from t_i to t_{i+1}
  DS_EI_CX_A = 0, DS_EI_CD_A, DS_EI_W0_A, DS_EI_W1_A,  // cx = sqrt(ev(t_{i+1}) / ev(t_i)), cd = -alpha(t_{i+1}) expm1(-h), w0, w1
  DS_EI_CX_P, DS_EI_CD_P, DS_EI_W0_P, DS_EI_W1_P,
  DS_EI_AL_A, DS_EI_EV_A, DS_EI_AL_P, DS_EI_EV_P  // alpha_j(t_i), ev_j(t_i): the data prediction at t_i
};

struct OdeExpintPlan {
  int method = 0, M = 0;
  double eps = 0.0;
  int denoise = 0, N = 0;
  std::vector<double> t;     // the grid: M + 1 times, strictly descending, inside (0, 1]
  std::vector<double> coef;  // [M][DS_EXPINT_COEFS]
};

// ev1, ev2 of MixSDE._cov_eigval (sdes/sdes.py:296-309) in float64, in its operation order
inline void ds_expint_eig(const diffsep_sde_config& s, double t, double& ev1, double& ev2) {
  const double r = (double)s.sigma_max / (double)s.sigma_min;
  const double mult = (double)s.sigma_min * (double)s.sigma_min;
  const double srp = pow(r, 2 * t);
  ev1 = mult * (srp - 1);
  ev2 = mult * (srp - exp(-2.0 * (double)s.d_lambda * t)) / (1.0 + (double)s.d_lambda / log(r));
}

// Fill and validate (`who`, timesteps as ode_fixed_plan_fill: the grid is ode_grid_fill's; want_err: the caller asks for the
// local-error trace); returns the message, empty when all is well.
inline std::string ode_expint_plan_fill(OdeExpintPlan& p, const OdeFixedConfig& oc, const diffsep_sde_config& sde,
                                        const double* timesteps, bool want_err, const char* who) {
  const std::string w(who);
  p = OdeExpintPlan();
  if (!(oc.method == DIFFSEP_EXPINT_DDIM || oc.method == DIFFSEP_EXPINT_DPMPP2M))
    return w + ": method must be DIFFSEP_EXPINT_DDIM or DIFFSEP_EXPINT_DPMPP2M";
  if (!(sde.kind == DIFFSEP_SDE_MIX || sde.kind == DIFFSEP_SDE_PRIORMIX))
    return w + ": the exponential integrators need a MixSDE or a PriorMixSDE (two eigenspaces with closed-form schedules)";
  const int M = oc.steps;
  if (!(M <= DS_ODEF_MAX_EVALS)) return w + ": steps must be <= 16384";
  const std::string bad = ode_grid_fill(oc, timesteps, who, p.t, (want_err && oc.method != DIFFSEP_EXPINT_DPMPP2M)
      ? ": err_out needs the second-order method (DPMPP2M: step minus its DDIM step), not DDIM" : nullptr);
  if (!bad.empty()) return bad;
  p.method = oc.method; p.M = M; p.eps = oc.eps; p.denoise = oc.denoise; p.N = oc.N;
  // per grid point and eigenspace: alpha, ev and the half log-SNR
  const double a[2] = {0.0, (double)sde.d_lambda};
  std::vector<double> al(2 * ((size_t)M + 1)), ev(al.size()), lam(al.size());
  for (int i = 0; i <= M; ++i) {
    double e[2];
    ds_expint_eig(sde, p.t[i], e[0], e[1]);
    if (!(e[0] > 0.0 && e[1] > 0.0))
      return w + ": ev_1 <= 0 (or ev_2 <= 0) at a grid point: the covariance eigenvalues must be positive (sigma_max > sigma_min)";
    for (int j = 0; j < 2; ++j) {
      al[2 * i + j] = exp(-a[j] * p.t[i]);
      ev[2 * i + j] = e[j];
      lam[2 * i + j] = log(al[2 * i + j]) - 0.5 * log(e[j]);
    }
  }
  p.coef.assign((size_t)M * DS_EXPINT_COEFS, 0.0);
  for (int i = 0; i < M; ++i) {
    double* c = p.coef.data() + (size_t)i * DS_EXPINT_COEFS;
    for (int j = 0; j < 2; ++j) {
      const double h = lam[2 * (i + 1) + j] - lam[2 * i + j];
      double* cj = c + 4 * j;
      cj[0] = sqrt(ev[2 * (i + 1) + j] / ev[2 * i + j]);
      cj[1] = -al[2 * (i + 1) + j] * expm1(-h);
      cj[2] = 1.0;
      cj[3] = 0.0;
      if (oc.method == DIFFSEP_EXPINT_DPMPP2M && i >= 1) {
        const double r = (lam[2 * i + j] - lam[2 * (i - 1) + j]) / h;
        cj[2] = 1.0 + 1.0 / (2.0 * r);
        cj[3] = -1.0 / (2.0 * r);
      }
      c[DS_EI_AL_A + 2 * j] = al[2 * i + j];
      c[DS_EI_EV_A + 2 * j] = ev[2 * i + j];
    }
  }
  return std::string();
}
