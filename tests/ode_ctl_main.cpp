// The step controller of the ODE sampler (csrc/ode_host.h: OdePlan, OdeCtl, the tableaux) on a small float64 system, with no GPU
// and no library: what tests/test_ode_ctl_cpu.py compares with scipy.integrate.solve_ivp on the same system.
//   ode_ctl_main METHOD(0 RK45 | 1 RK23) TOL(rtol = atol) FIRST_STEP(0: select_initial_step) MAX_STEP(0: none) MAX_NFE(0: none)
// integrates  y' = M y + 0.1 (i + 1) sin 3t + 5 (i + 1) tanh(40 (t - 0.5)),  y(1) = (1, -0.5, 0.25),  from t = 1 down to 0.03
// the way the device passes do (sums in sequence, RMS norms) and prints one JSON line: nfev, accepted, rejected, status, the
// accepted times and the final state — or {"refused": message} when the configuration is.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../diffusion-separation_amd/csrc/ode_host.h"

static const int N = 3;

static void fun(double t, const double* y, double* f) {
  static const double M[N][N] = {{-1.3, 2, 0}, {-2, -0.7, 0.5}, {0.1, -0.4, -2.1}};
  for (int i = 0; i < N; ++i) {
    double s = 0.0;
    for (int j = 0; j < N; ++j) s = s + M[i][j] * y[j];
    f[i] = s + 0.1 * (i + 1) * sin(3 * t) + 5.0 * (i + 1) * tanh(40 * (t - 0.5));
  }
}

// common.norm of v / (atol + max(|y|, |y2|) rtol)   (y2 null: |y| alone)
static double scaled_norm(const OdePlan& p, const double* v, const double* y, const double* y2) {
  double q = 0.0;
  for (int i = 0; i < N; ++i) {
    const double m = y2 ? fmax(fabs(y[i]), fabs(y2[i])) : fabs(y[i]);
    const double d = v[i] / (p.atol + m * p.rtol);
    q = q + d * d;
  }
  return sqrt(q) / sqrt((double)N);
}

int main(int argc, char** argv) {
  if (argc != 6) {
    fprintf(stderr, "usage: %s METHOD TOL FIRST_STEP MAX_STEP MAX_NFE\n", argv[0]);
    return 2;
  }
  diffsep_ode_config oc;
  memset(&oc, 0, sizeof(oc));
  oc.method = atoi(argv[1]);
  oc.rtol = oc.atol = atof(argv[2]);
  oc.eps = 0.03;
  oc.first_step = atof(argv[3]);
  oc.max_step = atof(argv[4]);
  oc.max_nfe = atoi(argv[5]);
  OdePlan p;
  const std::string bad = ode_plan_fill(p, oc, "ode_ctl_main");
  if (!bad.empty()) {
    printf("{\"refused\": \"%s\"}\n", bad.c_str());
    return 0;
  }
  const int ns = p.ns;
  double y[N] = {1.0, -0.5, 0.25}, ynew[N], K[DS_ODE_MAX_K][N], v[N];
  OdeCtl c;
  c.t = p.t0;
  fun(c.t, y, K[0]);
  ++c.nfev;
  if (p.first_step <= 0.0) {  // common.select_initial_step
    const double d0 = scaled_norm(p, y, y, nullptr), d1 = scaled_norm(p, K[0], y, nullptr);
    const double h0 = OdeCtl::initial_h0(p, d0, d1);
    for (int i = 0; i < N; ++i) v[i] = y[i] + h0 * p.dir * K[0][i];
    fun(p.t0 + h0 * p.dir, v, K[1]);
    ++c.nfev;
    for (int i = 0; i < N; ++i) v[i] = K[1][i] - K[0][i];
    c.initial_step(p, d1, scaled_norm(p, v, y, nullptr), h0);
  } else {
    c.h_abs = p.first_step;
  }
  std::vector<double> ts;
  while (c.begin_attempt(p)) {  // rk_step
    for (int s = 1; s <= ns; ++s) {
      const double* coef = s < ns ? p.A + s * DS_ODE_MAX_K : p.B;  // stage s < ns: row s of A over K[0..s); s = ns: y_new from B
      const int n = s < ns ? s : ns;
      for (int i = 0; i < N; ++i) {
        double acc = 0.0;
        for (int j = 0; j < n; ++j) acc = acc + coef[j] * K[j][i];
        v[i] = y[i] + acc * c.h;
      }
      if (s == ns) memcpy(ynew, v, sizeof(v));
      fun(c.stage_time(p, s), v, K[s]);
    }
    for (int i = 0; i < N; ++i) {  // _estimate_error: dot(K.T, E) * h
      double acc = 0.0;
      for (int j = 0; j <= ns; ++j) acc = acc + p.E[j] * K[j][i];
      v[i] = acc * c.h;
    }
    if (c.end_attempt(p, scaled_norm(p, v, y, ynew))) {
      memcpy(y, ynew, sizeof(y));
      memcpy(K[0], K[ns], sizeof(K[0]));
      ts.push_back(c.t);
    }
  }
  printf("{\"nfev\": %d, \"accepted\": %d, \"rejected\": %d, \"status\": %d, \"t\": [", c.nfev, c.n_acc, c.n_rej, c.status);
  for (size_t i = 0; i < ts.size(); ++i) printf("%s%.17g", i ? ", " : "", ts[i]);
  printf("], \"y\": [%.17g, %.17g, %.17g]}\n", y[0], y[1], y[2]);
  return 0;
}
