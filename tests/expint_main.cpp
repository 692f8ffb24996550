// The plan of an exponential-integrator solve (csrc/ode_host.h: OdeExpintPlan, ode_expint_plan_fill) walked in float64 on the
// point-mass data distribution, with no GPU and no library: what tests/test_expint_cpu.py compares with its numpy restatement.
//   expint_main METHOD(0 ddim | 1 dpmpp2m) STEPS T_START EPS DENOISE N WANT_ERR KIND D_LAMBDA SIGMA_MIN SIGMA_MAX [t_0 ... t_M]
// Per eigenspace j in {A, P} one scalar u_j with the exact score of data concentrated at c_j:  score = -(u - alpha_j c_j) / ev_j,
// started at  u_j(t_0) = alpha_j(t_0) c_j + sqrt(ev_j(t_0)) z_j,  c = (0.7, -0.4), z = (0.3, -1.1).  Each step forms the data
// prediction X0 = (u + ev score) / alpha and takes  u' = cx u + cd (w0 X0 + w1 X0_prev)  from the plan's table.  Prints one JSON
// line: the grid, the table, the state after every step, the trace (step minus its DDIM step) — or {"refused": message}.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../diffusion-separation_amd/csrc/ode_host.h"

int main(int argc, char** argv) {
  if (argc < 12) {
    fprintf(stderr, "usage: %s METHOD STEPS T_START EPS DENOISE N WANT_ERR KIND D_LAMBDA SIGMA_MIN SIGMA_MAX [t_0 ... t_M]\n", argv[0]);
    return 2;
  }
  OdeExpintConfig oc;
  oc.method = atoi(argv[1]);
  oc.steps = atoi(argv[2]);
  oc.t_start = atof(argv[3]);
  oc.eps = atof(argv[4]);
  oc.denoise = atoi(argv[5]);
  oc.N = atoi(argv[6]);
  const bool want_err = atoi(argv[7]) != 0;
  diffsep_sde_config sde;
  memset(&sde, 0, sizeof(sde));
  sde.kind = atoi(argv[8]);
  sde.ndim = 2;
  sde.d_lambda = (float)atof(argv[9]);
  sde.sigma_min = (float)atof(argv[10]);
  sde.sigma_max = (float)atof(argv[11]);
  sde.avg_len = 510;
  std::vector<double> grid;
  for (int i = 12; i < argc; ++i) grid.push_back(atof(argv[i]));
  if (!grid.empty() && (int)grid.size() != oc.steps + 1) {
    fprintf(stderr, "%s: %d grid times for %d steps\n", argv[0], (int)grid.size(), oc.steps);
    return 2;
  }
  OdeExpintPlan p;
  const std::string bad = ode_expint_plan_fill(p, oc, sde, grid.empty() ? nullptr : grid.data(), want_err, "expint_main");
  if (!bad.empty()) {
    printf("{\"refused\": \"%s\"}\n", bad.c_str());
    return 0;
  }
  const double c0[2] = {0.7, -0.4}, z[2] = {0.3, -1.1};
  double u[2], prev[2] = {0.0, 0.0};
  {
    const double* r = p.coef.data();
    u[0] = r[DS_EI_AL_A] * c0[0] + sqrt(r[DS_EI_EV_A]) * z[0];
    u[1] = r[DS_EI_AL_P] * c0[1] + sqrt(r[DS_EI_EV_P]) * z[1];
  }
  std::vector<double> states, errs;
  for (int i = 0; i < p.M; ++i) {
    const double* r = p.coef.data() + (size_t)i * DS_EXPINT_COEFS;
    for (int j = 0; j < 2; ++j) {
      const double al = r[DS_EI_AL_A + 2 * j], ev = r[DS_EI_EV_A + 2 * j];
      const double* cj = r + 4 * j;
      const double score = -(u[j] - al * c0[j]) / ev;
      const double x0 = (u[j] + ev * score) / al;
      double d = cj[2] * x0;
      if (i >= 1) d = d + cj[3] * prev[j];
      errs.push_back(i >= 1 ? cj[1] * (cj[2] - 1.0) * (x0 - prev[j]) : 0.0);
      u[j] = cj[0] * u[j] + cj[1] * d;
      prev[j] = x0;
      states.push_back(u[j]);
    }
  }
  printf("{\"steps\": %d, \"t\": [", p.M);
  for (size_t i = 0; i < p.t.size(); ++i) printf("%s%.17g", i ? ", " : "", p.t[i]);
  printf("], \"coef\": [");
  for (size_t i = 0; i < p.coef.size(); ++i) printf("%s%.17g", i ? ", " : "", p.coef[i]);
  printf("], \"u\": [");
  for (size_t i = 0; i < states.size(); ++i) printf("%s%.17g", i ? ", " : "", states[i]);
  printf("], \"err\": [");
  for (size_t i = 0; i < errs.size(); ++i) printf("%s%.17g", i ? ", " : "", errs[i]);
  printf("]}\n");
  return 0;
}
