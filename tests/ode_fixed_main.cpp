// The plan of a fixed-step solve (csrc/ode_host.h: OdeFixedPlan, ode_fixed_plan_fill) walked on a small float64 system, with no
// GPU and no library: what tests/test_ode_fixed_cpu.py compares with its own numpy restatement of the methods.
//   ode_fixed_main METHOD(0 euler | 1 heun | 2 midpoint | 3 rk4 | 4 ab2) STEPS T_START EPS DENOISE N WANT_ERR [t_0 ... t_M]
// integrates  y' = a(t) M y,  a(t) = 1 + 2 t  (closed form: y = expm(M int a) y(t_0)),  y(t_0) = (1, -0.5, 0.25)  over the plan's grid
// by walking the pass list the way the device driver does (sums in sequence over K[0], K[1], ..., steps committed by swapping
// y and y_new) and prints one JSON line: the evaluation count, the grid, the state after every step, the local-error trace
// (RMS of the step minus its embedded Euler step, RMS of y_i) — or {"refused": message} when the plan is.
#include <stdio.h>
#include <stdlib.h>

#include <utility>
#include <vector>

#include "../diffusion-separation_amd/csrc/ode_host.h"

static const int N = 3;

static void fun(double t, const double* y, double* f) {
  static const double M[N][N] = {{-1.3, 2, 0}, {-2, -0.7, 0.5}, {0.1, -0.4, -2.1}};
  const double a = 1.0 + 2 * t;
  for (int i = 0; i < N; ++i) {
    double s = 0.0;
    for (int j = 0; j < N; ++j) s = s + M[i][j] * y[j];
    f[i] = a * s;
  }
}

static double rms(const double* v) {
  double q = 0.0;
  for (int i = 0; i < N; ++i) q = q + v[i] * v[i];
  return sqrt(q) / sqrt((double)N);
}

int main(int argc, char** argv) {
  if (argc < 8) {
    fprintf(stderr, "usage: %s METHOD STEPS T_START EPS DENOISE N WANT_ERR [t_0 ... t_M]\n", argv[0]);
    return 2;
  }
  OdeFixedConfig oc;
  oc.method = atoi(argv[1]);
  oc.steps = atoi(argv[2]);
  oc.t_start = atof(argv[3]);
  oc.eps = atof(argv[4]);
  oc.denoise = atoi(argv[5]);
  oc.N = atoi(argv[6]);
  const bool want_err = atoi(argv[7]) != 0;
  std::vector<double> grid;
  for (int i = 8; i < argc; ++i) grid.push_back(atof(argv[i]));
  if (!grid.empty() && (int)grid.size() != oc.steps + 1) {
    fprintf(stderr, "%s: %d grid times for %d steps\n", argv[0], (int)grid.size(), oc.steps);
    return 2;
  }
  OdeFixedPlan p;
  const std::string bad = ode_fixed_plan_fill(p, oc, grid.empty() ? nullptr : grid.data(), want_err, "ode_fixed_main");
  if (!bad.empty()) {
    printf("{\"refused\": \"%s\"}\n", bad.c_str());
    return 0;
  }
  std::vector<double> ya(N), yb(N);
  double *y = ya.data(), *ynew = yb.data();
  y[0] = 1.0; y[1] = -0.5; y[2] = 0.25;
  double Kbuf[DS_ODE_MAX_K][N];
  double* K[DS_ODE_MAX_K];
  for (int j = 0; j < DS_ODE_MAX_K; ++j) K[j] = Kbuf[j];
  double x[N], v[N];
  memcpy(x, y, sizeof(x));
  std::vector<double> states, errs;
  for (int r = 0; r < p.n_evals; ++r) {
    const OdeFixedPass& q = p.pass[r];
    fun(q.t_eval, x, K[q.kout]);
    for (int i = 0; i < N; ++i) {
      double acc = 0.0;
      for (int j = 0; j < q.nk; ++j) acc = acc + q.c[j] * K[j][i];
      v[i] = q.mode == 1 ? y[i] + acc * q.h : y[i] + q.h * acc;
    }
    if (q.mode == 1) {
      memcpy(x, v, sizeof(x));
      continue;
    }
    memcpy(ynew, v, sizeof(v));
    if (q.err_nk > 0) {
      for (int i = 0; i < N; ++i) {
        double acc = 0.0;
        for (int j = 0; j < q.err_nk; ++j) acc = acc + q.d[j] * K[j][i];
        v[i] = acc * q.h;
      }
      errs.push_back(rms(v));
      errs.push_back(rms(y));
    }
    std::swap(y, ynew);
    if (q.swap_k01) std::swap(K[0], K[1]);
    memcpy(x, y, sizeof(x));
    for (int i = 0; i < N; ++i) states.push_back(y[i]);
  }
  printf("{\"n_evals\": %d, \"steps\": %d, \"has_err\": %d, \"t\": [", p.n_evals, p.M, p.has_err ? 1 : 0);
  for (size_t i = 0; i < p.t.size(); ++i) printf("%s%.17g", i ? ", " : "", p.t[i]);
  printf("], \"t_eval\": [");
  for (int r = 0; r < p.n_evals; ++r) printf("%s%.17g", r ? ", " : "", p.pass[r].t_eval);
  printf("], \"step_of\": [");
  for (int r = 0; r < p.n_evals; ++r) printf("%s%d", r ? ", " : "", p.pass[r].step);
  printf("], \"y\": [");
  for (size_t i = 0; i < states.size(); ++i) printf("%s%.17g", i ? ", " : "", states[i]);
  printf("], \"err\": [");
  for (size_t i = 0; i < errs.size(); ++i) printf("%s%.17g", i ? ", " : "", errs[i]);
  printf("]}\n");
  return 0;
}
