// sampler.hip — the two sampler drivers on the engine's resident state: the predictor-corrector sampler
// (sdes/__init__.py:166-188) and the probability-flow ODE sampler.  Host control flow only; every score evaluation is one
// run_nfe (engine.hip), every update a kernel of sde.hip / ode.hip.
#include "engine_host.h"

// torch.linspace(start, end, n) in float32 (ATen RangeFactories: symmetric fill around the midpoint)
static void linspace_f32(float start, float end, int n, float* out) {
  if (n == 1) { out[0] = start; return; }
  const float step = (end - start) / (float)(n - 1);
  const int half = n / 2;
  for (int i = 0; i < n; ++i) out[i] = (i < half) ? (start + step * (float)i) : (end - step * (float)(n - 1 - i));
}

// zero the tail t >= lens[b] of [B][rows][T] rows (mixture of a mixed-length batch)
__global__ __launch_bounds__(256) void mask_tail_kernel(float* __restrict__ v, int rows, long T,
                                                        const int* __restrict__ lens) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  const int b = blockIdx.y;
  if (t >= T || t < lens[b]) return;
  for (int r = 0; r < rows; ++r) v[((long)b * rows + r) * T + t] = 0.f;
}

int ds_launch_mask_tail(float* v, int B, int rows, long T, const int* lens, hipStream_t st) {
  hipLaunchKernelGGL(mask_tail_kernel, dim3(cdiv(T, 256), B), dim3(256), 0, st, v, rows, T, lens);
  DS_LAUNCH_CHECK();
  return 0;
}

// What both samplers ask of the SDE description (`who`: the entry point's name in the message)
static int check_sde(const diffsep_engine* e, const diffsep_sde_config* sde, const char* who) {
  const std::string w(who);
  DS_CHECK(sde->kind == DIFFSEP_SDE_MIX || sde->kind == DIFFSEP_SDE_PRIORMIX, w + ": unknown SDE kind");
  DS_CHECK(sde->kind == DIFFSEP_SDE_MIX || sde->avg_len >= 1, w + ": PriorMixSDE needs avg_len >= 1");
  DS_CHECK(sde->ndim == e->cfg.num_sources, w + ": sde.ndim != num_sources");
  return 0;
}
// PriorMixSDE: the per-sample noise scale from the envelope of the mixture in st_mix (sdes.py:477-489); MixSDE: none (null)
static int mixture_scale(diffsep_engine* e, const diffsep_sde_config* sde, int B, long T, hipStream_t st, const float** smix) {
  *smix = nullptr;
  if (sde->kind != DIFFSEP_SDE_PRIORMIX) return 0;
  if (ds_launch_sigma_mix(e->st_mix, e->st_smix, B, T, sde->avg_len, st)) return 1;
  *smix = e->st_smix;
  return 0;
}

extern "C" int32_t diffsep_pc_sample_ex(diffsep_engine* e, const diffsep_sde_config* sde,
                                        const diffsep_sampler_config* smp, const diffsep_sampler_ext* ext,
                                        const float* mix_norm, float* out, int32_t B, int64_t T, const float* noise,
                                        uint64_t seed, const float* timesteps_host, int32_t* nfe_out, void* stream) {
  DS_CHECK(e && sde && smp && mix_norm && out, "pc_sample: null argument");
  if (check_sde(e, sde, "pc_sample")) return 1;
  DS_CHECK(smp->N >= 1 && smp->N <= 4096, "pc_sample: N must be in [1,4096]");
  DS_CHECK(smp->predictor == DIFFSEP_PRED_REVERSE_DIFFUSION || smp->predictor == DIFFSEP_PRED_EULER_MARUYAMA ||
               smp->predictor == DIFFSEP_PRED_NONE,
           "pc_sample: predictor must be reverse_diffusion, euler_maruyama or none");
  DS_CHECK(smp->corrector == DIFFSEP_CORR_ALD2 || smp->corrector == DIFFSEP_CORR_NONE ||
               smp->corrector == DIFFSEP_CORR_ALD || smp->corrector == DIFFSEP_CORR_LANGEVIN,
           "pc_sample: corrector must be ald2, ald, langevin or none");
  DS_CHECK(smp->corrector != DIFFSEP_CORR_ALD || sde->kind == DIFFSEP_SDE_MIX,
           "pc_sample: the 'ald' corrector supports MixSDE only (sdes/correctors.py:64-67)");
  const int64_t* lengths = ext ? ext->lengths_host : nullptr;
  const uint64_t* seeds = ext ? ext->seeds_host : nullptr;
  diffsep_engine* tail = (ext && (ext->tail_steps > 0 || ext->head_steps > 0)) ? ext->tail_engine : nullptr;
  const int tail_steps = tail ? ext->tail_steps : 0;
  const int head_steps = tail ? ext->head_steps : 0;
  if (tail) {
    DS_CHECK(tail != e, "pc_sample: the tail engine must be a different engine");
    diffsep_model_config a = e->cfg, b2 = tail->cfg;
    a.dtype = b2.dtype = 0;
    DS_CHECK(memcmp(&a, &b2, sizeof(a)) == 0, "pc_sample: the tail engine must have the same architecture");
  }
  DS_CHECK(!lengths || smp->corrector != DIFFSEP_CORR_LANGEVIN,
           "pc_sample: the 'langevin' corrector couples the batch entries; it cannot run on a mixed-length batch");
  DS_CHECK(!seeds || !noise, "pc_sample: per-utterance seeds are for device noise (noise == NULL)");
  if (lengths) {
    const int Wp = diffsep_padded_frames(&e->cfg, T);
    for (int b = 0; b < B; ++b) {
      DS_CHECK(lengths[b] >= 1 && lengths[b] <= T, "pc_sample: utterance length outside [1, T]");
      DS_CHECK(diffsep_padded_frames(&e->cfg, lengths[b]) == Wp,
               "pc_sample: every utterance of a mixed-length batch must have the padded frame count of T");
    }
  }
  StreamScope sc_(e, stream);
  hipStream_t st = sc_.st;
  const int S = e->cfg.num_sources, N = smp->N;
  const int csteps = smp->corrector == DIFFSEP_CORR_NONE ? 0 : smp->corrector_steps;
  if (ensure_plan(e, B, T, st)) return 1;
  if (tail && ensure_plan(tail, B, T, st)) return 1;
  const size_t nst = (size_t)B * S * T;
  const SdeP sp = to_sdep(sde);
  // time steps -> device rows [N][B]
  std::vector<float> ts(N);
  if (timesteps_host) for (int i = 0; i < N; ++i) ts[i] = timesteps_host[i];
  else linspace_f32(1.0f, smp->eps, N, ts.data());
  if (e->ts_dev != ts || e->ts_B != B) {  // (same schedule as the last call: the device rows are already there)
    const size_t nrow = (size_t)N * B;
    float* pin;
    if (e->ts_pin.acquire(nrow, &pin)) return 1;
    for (int i = 0; i < N; ++i) for (int b = 0; b < B; ++b) pin[(size_t)i * B + b] = ts[i];
    DS_HIP(hipMemcpyAsync(e->st_ts, pin, nrow * 4, hipMemcpyHostToDevice, st));
    if (e->ts_pin.record(st)) return 1;
    e->ts_dev = ts;
    e->ts_B = B;
  }
  DS_HIP(hipMemcpyAsync(e->st_mix, mix_norm, (size_t)B * T * 4, hipMemcpyDeviceToDevice, st));
  const int* lens = nullptr;
  if (lengths || seeds) {  // per-utterance lengths / seeds -> device (pinned staging, stream-ordered)
    char* pin;
    if (e->ext_pin.acquire((size_t)B * 16, &pin)) return 1;
    unsigned long long* ps = reinterpret_cast<unsigned long long*>(pin);
    int* pl = reinterpret_cast<int*>(pin + (size_t)B * 8);
    for (int b = 0; b < B; ++b) {
      ps[b] = seeds ? seeds[b] : seed + 0x9E3779B97F4A7C15ull * (unsigned long long)b;  // (b = 0: the B = 1 stream of `seed`)
      pl[b] = lengths ? (int)lengths[b] : (int)T;
    }
    DS_HIP(hipMemcpyAsync(e->st_seeds, ps, (size_t)B * 8, hipMemcpyHostToDevice, st));
    DS_HIP(hipMemcpyAsync(e->st_lens, pl, (size_t)B * 4, hipMemcpyHostToDevice, st));
    if (e->ext_pin.record(st)) return 1;
    if (lengths) {
      lens = e->st_lens;
      hipLaunchKernelGGL(mask_tail_kernel, dim3(cdiv(T, 256), B), dim3(256), 0, st, e->st_mix, 1, (long)T, lens);
      DS_LAUNCH_CHECK();
    }
  }
  const bool batch_rng = !noise && (seeds || lengths);

  long draw = 0;
  auto next_noise = [&](const float** z) -> int {
    if (noise) { *z = noise + (size_t)draw * nst; }
    else {
      if (prof_launch(e, st, hbm_rec("randn (Philox4x32-10 + Box-Muller)", 4.0 * nst, B, 1, (int)T, S), [&]() {
            return batch_rng ? ds_launch_randn_batch(e->st_noise, B, S, T, (const uint64_t*)e->st_seeds, e->st_lens, (uint64_t)draw, st)
                             : ds_launch_randn(e->st_noise, (long)nst, seed, (uint64_t)draw, st);
          }))
        return 1;
      *z = e->st_noise;
    }
    ++draw;
    return 0;
  };
  const float* z = nullptr;
  if (next_noise(&z)) return 1;
  const float* smix = nullptr;
  if (mixture_scale(e, sde, B, T, st, &smix)) return 1;
  if (ds_launch_sde_prior(sp, e->st_mix, z, e->st_x, B, S, T, smix, st, lens)) return 1;
  DS_HIP(hipMemcpyAsync(e->st_xm, e->st_x, nst * 4, hipMemcpyDeviceToDevice, st));
  // one score evaluation of reverse step i: on this engine, or — in the last tail_steps steps — on the tail engine
  // (state and time step copied over, the score read from there)
  bool tail_ready = false;
  const float* score = e->st_score;
  auto eval_score = [&](int i) -> int {
    if (tail && (i >= N - tail_steps || i < head_steps)) {
      if (!tail_ready) {
        DS_HIP(hipMemcpyAsync(tail->st_mix, e->st_mix, (size_t)B * T * 4, hipMemcpyDeviceToDevice, st));
        tail_ready = true;
      }
      DS_HIP(hipMemcpyAsync(tail->st_x, e->st_x, nst * 4, hipMemcpyDeviceToDevice, st));
      DS_HIP(hipMemcpyAsync(tail->st_t, e->st_t, (size_t)B * 4, hipMemcpyDeviceToDevice, st));
      score = tail->st_score;
      return run_nfe(tail, B, T, st);
    }
    score = e->st_score;
    return run_nfe(e, B, T, st);
  };
  for (int i = 0; i < N; ++i) {
    DS_HIP(hipMemcpyAsync(e->st_t, e->st_ts + (size_t)i * B, (size_t)B * 4, hipMemcpyDeviceToDevice, st));
    for (int k = 0; k < csteps; ++k) {
      if (eval_score(i)) return 1;
      if (next_noise(&z)) return 1;
      if (smp->corrector == DIFFSEP_CORR_LANGEVIN) {
        if (ds_launch_langevin(smp->snr, e->st_x, score, z, e->st_x, e->st_xm, B, (long)S * T, e->st_lang, st))
          return 1;
      } else if (prof_launch(e, st, hbm_rec("sde_corrector (ald2 update)", 4.0 * nst * 5.0, B, 1, (int)T, S), [&]() {  // x, score, z in; x, x_mean out
                   return ds_launch_sde_corrector(sp, smp->snr, e->st_x, e->st_t, score, z, e->st_x, e->st_xm, B, S, T,
                                                  smix, smp->corrector == DIFFSEP_CORR_ALD ? 1 : 0, st, lens);
                 })) {
        return 1;
      }
    }
    if (smp->predictor != DIFFSEP_PRED_NONE) {
      // euler_maruyama (sdes/predictors.py:39-52) takes x + f*dt with the reverse drift f = drift - g^2 score and
      // noise g sqrt(dt): algebraically the reverse_diffusion step (dt = 1/N, G = g sqrt(dt)) — one kernel for both
      if (eval_score(i)) return 1;
      if (next_noise(&z)) return 1;
      if (prof_launch(e, st, hbm_rec("sde_predictor (reverse-diffusion update)", 4.0 * nst * 5.0, B, 1, (int)T, S), [&]() {
            return ds_launch_sde_predictor(sp, N, e->st_x, e->st_t, score, z, e->st_x, e->st_xm, B, S, T, smix, 0, st, lens);
          }))
        return 1;
    } else {
      DS_HIP(hipMemcpyAsync(e->st_xm, e->st_x, nst * 4, hipMemcpyDeviceToDevice, st));
    }
  }
  DS_HIP(hipMemcpyAsync(out, smp->denoise ? e->st_xm : e->st_x, nst * 4, hipMemcpyDeviceToDevice, st));
  if (nfe_out) *nfe_out = N * (csteps + 1);
  return 0;
}

extern "C" int32_t diffsep_pc_sample(diffsep_engine* e, const diffsep_sde_config* sde, const diffsep_sampler_config* smp,
                                     const float* mix_norm, float* out, int32_t B, int64_t T, const float* noise,
                                     uint64_t seed, const float* timesteps_host, int32_t* nfe_out, void* stream) {
  return diffsep_pc_sample_ex(e, sde, smp, nullptr, mix_norm, out, B, T, noise, seed, timesteps_host, nfe_out, stream);
}

// ------------------------------------------------------------------ probability-flow ODE sampler
// sdes.get_ode_sampler(...)() (reference sdes/__init__.py:193-278): scipy.integrate.solve_ivp(RK45 | RK23) on the
// probability-flow ODE, the controller ported from scipy 1.15 (integrate/_ivp/rk.py RungeKutta._step_impl, common.py
// select_initial_step / norm, base.py OdeSolver.step, ivp.py solve_ivp's loop) and run on the host; every stage is one
// graph-replayed network evaluation (run_nfe) + one fused pass (ode.hip), every step attempt one pinned readback of its
// error norm.
extern "C" int32_t diffsep_ode_sample(diffsep_engine* e, const diffsep_sde_config* sde, const diffsep_ode_config* oc,
                                      const float* mix_norm, const float* x_init, const float* noise, uint64_t seed,
                                      float* out, int32_t B, int64_t T, diffsep_ode_info* info, void* stream) {
  DS_CHECK(e && sde && oc && mix_norm && out, "ode_sample: null argument");
  if (check_sde(e, sde, "ode_sample")) return 1;
  DS_CHECK(B >= 1 && T >= 1, "ode_sample: empty batch");
  DS_CHECK(!(x_init && noise), "ode_sample: x_init and noise are alternatives");
  double Ab[DS_ODE_MAX_K * DS_ODE_MAX_K], Bb[DS_ODE_MAX_K], Cb[DS_ODE_MAX_K], Eb[DS_ODE_MAX_K + 1];
  int ns = 0, eorder = 0;
  DS_CHECK(ds_ode_tableau(oc->method, nullptr, nullptr, nullptr, nullptr, &ns, &eorder) == 0,
           "ode_sample: method must be DIFFSEP_ODE_RK45 or DIFFSEP_ODE_RK23 (DOP853 / Radau / BDF / LSODA are not implemented)");
  {
    double A0[6 * 6];
    ds_ode_tableau(oc->method, A0, Bb, Cb, Eb, nullptr, nullptr);
    for (int i = 0; i < ns; ++i) for (int j = 0; j < ns; ++j) Ab[i * DS_ODE_MAX_K + j] = A0[i * ns + j];
  }
  const double eps = oc->eps;
  DS_CHECK(eps > 0.0 && eps < 1.0, "ode_sample: eps must be in (0, 1)");
  DS_CHECK(oc->atol >= 0.0 && oc->rtol >= 0.0, "ode_sample: tolerances must be non-negative");
  DS_CHECK(oc->N >= 1 || !oc->denoise, "ode_sample: the denoise step needs N >= 1");
  DS_CHECK(oc->max_nfe >= 0, "ode_sample: max_nfe must be >= 0");
  // common.validate_tol: rtol below 100 machine epsilons is raised to it (scipy warns)
  const double rtol = std::max(oc->rtol, 100 * 2.220446049250313e-16), atol = oc->atol;
  const double max_step = (oc->max_step > 0.0) ? oc->max_step : INFINITY;
  const double t0 = 1.0, t_bound = eps, dir = -1.0, interval = std::fabs(t_bound - t0);  // sde.T = 1
  DS_CHECK(oc->first_step <= 0.0 || oc->first_step <= interval, "ode_sample: first_step exceeds the interval (scipy: `first_step` exceeds bounds)");

  StreamScope sc_(e, stream);
  hipStream_t st = sc_.st;
  const int S = e->cfg.num_sources;
  if (ensure_plan(e, B, T, st)) return 1;
  const size_t nst = (size_t)B * S * T;
  auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t need = 2 * al(nst * 8) + DS_ODE_MAX_K * al(nst * 4) + al(2 * DS_ODE_MAX_BLOCKS * 8) + 256;
  if (need > e->ode_cap) {
    if (e->ode_buf) {
      DS_HIP(hipDeviceSynchronize());
      DS_HIP(hipFree(e->ode_buf));
    }
    e->ode_buf = nullptr;
    e->ode_cap = 0;
    DS_HIP(hipMalloc((void**)&e->ode_buf, need));
    e->ode_cap = need;
  }
  double* pin;  // pinned readback of the two norms
  if (e->ode_pin.acquire(2, &pin)) return 1;
  char* p = e->ode_buf;
  double* y = (double*)p; p += al(nst * 8);
  double* ynew = (double*)p; p += al(nst * 8);
  float* K[DS_ODE_MAX_K];
  for (int j = 0; j < DS_ODE_MAX_K; ++j) { K[j] = (float*)p; p += al(nst * 4); }
  double* part = (double*)p; p += al(2 * DS_ODE_MAX_BLOCKS * 8);
  double* dnorm = (double*)p;
  const SdeP sp = to_sdep(sde);

  // x_T -> st_x (and y = x_T in fp64)
  DS_HIP(hipMemcpyAsync(e->st_mix, mix_norm, (size_t)B * T * 4, hipMemcpyDeviceToDevice, st));
  const float* smix = nullptr;
  if (mixture_scale(e, sde, B, T, st, &smix)) return 1;
  if (x_init) {
    DS_HIP(hipMemcpyAsync(e->st_x, x_init, nst * 4, hipMemcpyDeviceToDevice, st));
  } else {
    const float* z = noise;
    if (!z) {  // the PC sampler's prior draw of the same seed (its draw 0)
      if (ds_launch_randn(e->st_noise, (long)nst, seed, 0, st)) return 1;
      z = e->st_noise;
    }
    if (ds_launch_sde_prior(sp, e->st_mix, z, e->st_x, B, S, T, smix, st)) return 1;
  }
  if (ds_launch_ode_cast(e->st_x, y, (long)nst, st)) return 1;

  OdeArgs base;
  memset(&base, 0, sizeof(base));
  base.s = sp; base.x = e->st_x; base.score = e->st_score; base.smix = smix;
  base.rtol = rtol; base.atol = atol; base.part = part; base.B = B; base.S = S; base.T = T;
  base.kidx = -1;
  // the fused pass after the network evaluation at (float) t_eval: K[kout] = drift, then the combination `mode` of
  // K[0..nk) with coefficients c, written for the next evaluation at (float) t_next (mode 3: the error scale from
  // max(|y|, |y_new|), or from |y| alone in select_initial_step)
  auto pass = [&](int kout, double t_eval, int mode, int nk, const double* c, double h, double t_next, int* nblk,
                  bool scale_ynew = true) -> int {
    OdeArgs a = base;
    a.kout = kout >= 0 ? K[kout] : nullptr;
    a.t = (float)t_eval;
    a.kidx = (kout >= 0 && kout < nk) ? kout : -1;
    a.nk = nk;
    for (int j = 0; j < nk; ++j) { a.k[j] = K[j]; a.c[j] = c[j]; }
    a.h = h; a.mode = mode; a.y = y;
    if (mode == 1) a.xo = e->st_x;
    if (mode == 2) { a.yo = ynew; a.xo = e->st_x; }
    if (mode == 3 && scale_ynew) a.ynew = ynew;
    if (mode == 1 || mode == 2) { a.t_next_out = e->st_t; a.t_next = (float)t_next; }
    return prof_launch(e, st, hbm_rec("ode_stage (fused drift + RK stage)", 4.0 * nst * (2 + nk) + 8.0 * nst * (mode >= 2 ? 2 : 1), B, 1, (int)T, S),
                       [&]() { return ds_launch_ode_stage(a, st, nblk); });
  };
  // the two norms of the last mode-3 pass -> host (stream-ordered pinned readback, waited on by its event)
  auto read_norms = [&](int nblk, double* n0, double* n1) -> int {
    if (ds_launch_ode_norm_final(part, nblk, (long)nst, dnorm, st)) return 1;
    DS_HIP(hipMemcpyAsync(pin, dnorm, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
    if (e->ode_pin.record(st) || e->ode_pin.wait()) return 1;
    *n0 = pin[0];
    if (n1) *n1 = pin[1];
    return 0;
  };

  int nfev = 0, n_acc = 0, n_rej = 0, status = 2;
  double t = t0;
  if (ds_launch_fill(e->st_t, (float)t, B, st)) return 1;
  if (run_nfe(e, B, T, st)) return 1;
  ++nfev;
  double h_abs;
  const double one = 1.0;
  if (oc->first_step <= 0.0) {  // common.select_initial_step
    const double pm[2] = {-1.0, 1.0};
    int nb = 0;
    double d0, d1, d2;
    if (pass(0, t, 3, 1, &one, 1.0, 0.0, &nb, false)) return 1;  // K0 = f0; norm(f0 / scale), norm(y0 / scale)
    if (read_norms(nb, &d1, &d0)) return 1;
    double h0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * d0 / d1;
    h0 = std::min(h0, interval);
    OdeArgs a = base;  // y1 = y0 + h0 * direction * f0
    a.nk = 1; a.k[0] = K[0]; a.c[0] = 1.0; a.h = h0 * dir; a.mode = 1; a.y = y; a.xo = e->st_x;
    a.t_next_out = e->st_t; a.t_next = (float)(t0 + h0 * dir);
    if (ds_launch_ode_stage(a, st)) return 1;
    if (run_nfe(e, B, T, st)) return 1;
    ++nfev;
    if (pass(1, t0 + h0 * dir, 3, 2, pm, 1.0, 0.0, &nb, false)) return 1;  // norm((f1 - f0) / scale)
    if (read_norms(nb, &d2, nullptr)) return 1;
    d2 = d2 / h0;
    const double h1 = (d1 <= 1e-15 && d2 <= 1e-15) ? std::max(1e-6, h0 * 1e-3)
                                                   : std::pow(0.01 / std::max(d1, d2), 1.0 / (eorder + 1));
    h_abs = std::min(std::min(100 * h0, h1), std::min(interval, max_step));
  } else {
    if (pass(0, t, 0, 0, nullptr, 0.0, 0.0, nullptr)) return 1;  // K0 = f0
    h_abs = oc->first_step;
  }

  const double err_exp = -1.0 / (eorder + 1);
  for (;;) {  // solve_ivp: while status is None: solver.step()
    const double min_step = 10 * std::fabs(std::nextafter(t, dir * INFINITY) - t);
    if (h_abs > max_step) h_abs = max_step;
    else if (h_abs < min_step) h_abs = min_step;
    bool accepted = false, rejected = false;
    double t_new = t;
    while (!accepted) {
      if (h_abs < min_step) { status = -1; break; }
      if (oc->max_nfe > 0 && nfev + ns > oc->max_nfe) { status = 1; break; }
      double h = h_abs * dir;
      t_new = t + h;
      if (dir * (t_new - t_bound) > 0) t_new = t_bound;
      h = t_new - t;
      h_abs = std::fabs(h);
      // rk_step: stage s input fp32(y + dot(K[:s].T, A[s,:s]) h) at t + C[s] h; y_new; f_new = f(t + h, y_new)
      {
        OdeArgs a = base;
        a.nk = 1; a.k[0] = K[0]; a.c[0] = Ab[1 * DS_ODE_MAX_K]; a.h = h; a.mode = 1; a.y = y; a.xo = e->st_x;
        a.t_next_out = e->st_t; a.t_next = (float)(t + Cb[1] * h);
        if (prof_launch(e, st, hbm_rec("ode_stage (RK stage input)", 16.0 * nst, B, 1, (int)T, S),
                        [&]() { return ds_launch_ode_stage(a, st); }))
          return 1;
      }
      int nb = 0;
      for (int s = 1; s <= ns; ++s) {
        if (run_nfe(e, B, T, st)) return 1;
        ++nfev;
        const double ts = s < ns ? t + Cb[s] * h : t + h;
        if (s < ns - 1) {
          if (pass(s, ts, 1, s + 1, Ab + (s + 1) * DS_ODE_MAX_K, h, t + Cb[s + 1] * h, nullptr)) return 1;
        } else if (s == ns - 1) {
          if (pass(s, ts, 2, ns, Bb, h, t + h, nullptr)) return 1;
        } else {
          if (pass(s, ts, 3, ns + 1, Eb, h, 0.0, &nb)) return 1;
        }
      }
      double err;
      if (read_norms(nb, &err, nullptr)) return 1;
      if (err < 1) {
        double factor = err == 0 ? 10.0 : std::min(10.0, 0.9 * std::pow(err, err_exp));
        if (rejected) factor = std::min(1.0, factor);
        h_abs *= factor;
        accepted = true;
      } else {
        h_abs *= std::max(0.2, 0.9 * std::pow(err, err_exp));
        rejected = true;
        ++n_rej;
      }
    }
    if (!accepted) break;
    std::swap(y, ynew);  // y <- y_new, f <- f_new: pointer swaps, no copies
    std::swap(K[0], K[ns]);
    base.y = y;
    t = t_new;
    ++n_acc;
    if (dir * (t - t_bound) >= 0) { status = 0; break; }
  }

  // solution.y[:, -1] (the last accepted state) -> float32; optional denoise: x_mean of one reverse_diffusion step at
  // eps without noise (reference denoise_update_fn; dt = 1/N, quirk Q1)
  if (ds_launch_ode_round(y, e->st_x, (long)nst, st)) return 1;
  if (oc->denoise) {
    if (ds_launch_fill(e->st_t, (float)eps, B, st)) return 1;
    if (run_nfe(e, B, T, st)) return 1;
    if (ds_launch_sde_predictor(sp, oc->N, e->st_x, e->st_t, e->st_score, nullptr, e->st_xm, out, B, S, T, smix, 0, st))
      return 1;
  } else {
    DS_HIP(hipMemcpyAsync(out, e->st_x, nst * 4, hipMemcpyDeviceToDevice, st));
  }
  if (info) {
    info->nfev = nfev; info->n_accepted = n_acc; info->n_rejected = n_rej; info->status = status; info->t_final = t;
  }
  return 0;
}

// ------------------------------------------------------------------ ... with one step controller per utterance
// B copies of the controller above in lock step on a zero-padded batch: utterance b has its own t, h, error norm,
// accept / reject decisions and counts — the host arithmetic of diffsep_ode_sample, per utterance — and all utterances
// share every network evaluation.  One step attempt = one upload of its tables (h, active, the evaluation times of its
// stages: a row per pass, so that no pass waits for the host), n_stages evaluations of the whole batch, and one pinned
// readback of the 2 B norms.  The device takes the accepted steps itself (ode_commit_each_kernel: norm < 1, the host's
// own test on the same number).  An utterance whose status is set is frozen: its rows ride through the network, its
// state is not touched.
namespace {
struct OdeCtl {  // one utterance's controller (the locals of diffsep_ode_sample)
  double t, h_abs, h = 0.0, t_new = 0.0;
  int nfev = 0, n_acc = 0, n_rej = 0, status = 2;  // 2: integrating
  bool new_step = true, rejected = false;
  double min_step = 0.0;
};
}  // namespace

extern "C" int32_t diffsep_ode_sample_each(diffsep_engine* e, const diffsep_sde_config* sde, const diffsep_ode_config* oc,
                                           const diffsep_ode_ext* ext, const float* mix_norm, const float* x_init,
                                           const float* noise, uint64_t seed, float* out, int32_t B, int64_t T,
                                           diffsep_ode_info* infos, int32_t* evals_run, void* stream) {
  DS_CHECK(e && sde && oc && mix_norm && out, "ode_sample_each: null argument");
  if (check_sde(e, sde, "ode_sample_each")) return 1;
  DS_CHECK(B >= 1 && B <= 65535 && T >= 1 && T <= 0x7fffffffLL, "ode_sample_each: bad batch shape");
  DS_CHECK(!(x_init && noise), "ode_sample_each: x_init and noise are alternatives");
  const int64_t* lengths = ext ? ext->lengths_host : nullptr;
  const uint64_t* seeds = ext ? ext->seeds_host : nullptr;
  DS_CHECK(!seeds || !(noise || x_init), "ode_sample_each: per-utterance seeds are for device noise (noise == NULL, x_init == NULL)");
  if (lengths) {
    const int Wp = diffsep_padded_frames(&e->cfg, T);
    for (int b = 0; b < B; ++b) {
      DS_CHECK(lengths[b] >= 1 && lengths[b] <= T, "ode_sample_each: utterance length outside [1, T]");
      DS_CHECK(diffsep_padded_frames(&e->cfg, lengths[b]) == Wp,
               "ode_sample_each: every utterance of a mixed-length batch must have the padded frame count of T");
    }
  }
  double Ab[DS_ODE_MAX_K * DS_ODE_MAX_K], Bb[DS_ODE_MAX_K], Cb[DS_ODE_MAX_K], Eb[DS_ODE_MAX_K + 1];
  int ns = 0, eorder = 0;
  DS_CHECK(ds_ode_tableau(oc->method, nullptr, nullptr, nullptr, nullptr, &ns, &eorder) == 0,
           "ode_sample_each: method must be DIFFSEP_ODE_RK45 or DIFFSEP_ODE_RK23 (DOP853 / Radau / BDF / LSODA are not implemented)");
  {
    double A0[6 * 6];
    ds_ode_tableau(oc->method, A0, Bb, Cb, Eb, nullptr, nullptr);
    for (int i = 0; i < ns; ++i) for (int j = 0; j < ns; ++j) Ab[i * DS_ODE_MAX_K + j] = A0[i * ns + j];
  }
  const double eps = oc->eps;
  DS_CHECK(eps > 0.0 && eps < 1.0, "ode_sample_each: eps must be in (0, 1)");
  DS_CHECK(oc->atol >= 0.0 && oc->rtol >= 0.0, "ode_sample_each: tolerances must be non-negative");
  DS_CHECK(oc->N >= 1 || !oc->denoise, "ode_sample_each: the denoise step needs N >= 1");
  DS_CHECK(oc->max_nfe >= 0, "ode_sample_each: max_nfe must be >= 0");
  const double rtol = std::max(oc->rtol, 100 * 2.220446049250313e-16), atol = oc->atol;
  const double max_step = (oc->max_step > 0.0) ? oc->max_step : INFINITY;
  const double t0 = 1.0, t_bound = eps, dir = -1.0, interval = std::fabs(t_bound - t0);
  DS_CHECK(oc->first_step <= 0.0 || oc->first_step <= interval, "ode_sample_each: first_step exceeds the interval (scipy: `first_step` exceeds bounds)");

  StreamScope sc_(e, stream);
  hipStream_t st = sc_.st;
  const int S = e->cfg.num_sources;
  if (ensure_plan(e, B, T, st)) return 1;
  const size_t nst = (size_t)B * S * T;
  auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
  // device tables of one attempt: h [B] | ones [B] (fp64) | active [B] (int) | evaluation times [DS_ODE_MAX_K + 1][B] (fp32)
  const int n_trows = DS_ODE_MAX_K + 1;
  const size_t off_ones = (size_t)B * 8, off_act = (size_t)B * 16, off_tt = (size_t)B * 20;
  const size_t tab_bytes = (size_t)B * (20 + 4 * n_trows);
  const size_t need = 2 * al(nst * 8) + DS_ODE_MAX_K * al(nst * 4) + al((size_t)B * 2 * DS_ODE_MAX_BLOCKS * 8) +
                      al((size_t)B * 16) + al(tab_bytes);
  if (need > e->ode_cap) {
    if (e->ode_buf) {
      DS_HIP(hipDeviceSynchronize());
      DS_HIP(hipFree(e->ode_buf));
    }
    e->ode_buf = nullptr;
    e->ode_cap = 0;
    DS_HIP(hipMalloc((void**)&e->ode_buf, need));
    e->ode_cap = need;
  }
  double* pin;  // pinned readback of the 2 B norms
  if (e->ode_pin.acquire((size_t)2 * B, &pin)) return 1;
  char* p = e->ode_buf;
  double* y = (double*)p; p += al(nst * 8);
  double* ynew = (double*)p; p += al(nst * 8);
  float* K[DS_ODE_MAX_K];
  for (int j = 0; j < DS_ODE_MAX_K; ++j) { K[j] = (float*)p; p += al(nst * 4); }
  double* part = (double*)p; p += al((size_t)B * 2 * DS_ODE_MAX_BLOCKS * 8);
  double* dnorm = (double*)p; p += al((size_t)B * 16);
  char* tab = p;
  const double* d_h = (const double*)tab;
  const double* d_ones = (const double*)(tab + off_ones);
  const int* d_act = (const int*)(tab + off_act);
  const float* d_tt = (const float*)(tab + off_tt);
  const SdeP sp = to_sdep(sde);

  // mixture, lengths and seeds -> device; x_T -> st_x with a zero tail (and y = x_T in fp64)
  DS_HIP(hipMemcpyAsync(e->st_mix, mix_norm, (size_t)B * T * 4, hipMemcpyDeviceToDevice, st));
  {
    char* xp;
    if (e->ext_pin.acquire((size_t)B * 16, &xp)) return 1;
    unsigned long long* ps = reinterpret_cast<unsigned long long*>(xp);
    int* pl = reinterpret_cast<int*>(xp + (size_t)B * 8);
    for (int b = 0; b < B; ++b) {
      ps[b] = seeds ? seeds[b] : seed + 0x9E3779B97F4A7C15ull * (unsigned long long)b;  // (b = 0: the B = 1 stream of `seed`)
      pl[b] = lengths ? (int)lengths[b] : (int)T;
    }
    DS_HIP(hipMemcpyAsync(e->st_seeds, ps, (size_t)B * 8, hipMemcpyHostToDevice, st));
    DS_HIP(hipMemcpyAsync(e->st_lens, pl, (size_t)B * 4, hipMemcpyHostToDevice, st));
    if (e->ext_pin.record(st)) return 1;
  }
  const int* lens = e->st_lens;
  if (lengths && ds_launch_mask_tail(e->st_mix, B, 1, T, lens, st)) return 1;
  const float* smix = nullptr;
  if (mixture_scale(e, sde, B, T, st, &smix)) return 1;
  if (x_init) {
    DS_HIP(hipMemcpyAsync(e->st_x, x_init, nst * 4, hipMemcpyDeviceToDevice, st));
    if (lengths && ds_launch_mask_tail(e->st_x, B, S, T, lens, st)) return 1;
  } else {
    const float* z = noise;
    if (!z) {  // utterance b: the PC sampler's prior draw of its seed (draw 0 of the B = 1 stream)
      if (ds_launch_randn_batch(e->st_noise, B, S, T, (const uint64_t*)e->st_seeds, lens, 0, st)) return 1;
      z = e->st_noise;
    }
    if (ds_launch_sde_prior(sp, e->st_mix, z, e->st_x, B, S, T, smix, st, lens)) return 1;
  }
  if (ds_launch_ode_cast(e->st_x, y, (long)nst, st)) return 1;

  std::vector<OdeCtl> u(B);
  std::vector<int> act(B, 1);
  std::vector<double> hv(B, 1.0);
  std::vector<float> ttv((size_t)n_trows * B, (float)t0);
  // this attempt's tables -> device (the staging buffer is free again once the previous upload has gone through)
  auto upload = [&]() -> int {
    char* tp;
    if (e->ode_tab_pin.acquire(tab_bytes, &tp)) return 1;
    double* ph = reinterpret_cast<double*>(tp);
    double* po = reinterpret_cast<double*>(tp + off_ones);
    int* pa = reinterpret_cast<int*>(tp + off_act);
    for (int b = 0; b < B; ++b) { ph[b] = hv[b]; po[b] = 1.0; pa[b] = act[b]; }
    memcpy(tp + off_tt, ttv.data(), ttv.size() * 4);
    DS_HIP(hipMemcpyAsync(tab, tp, tab_bytes, hipMemcpyHostToDevice, st));
    return e->ode_tab_pin.record(st);
  };

  OdeEachArgs base;
  memset(&base, 0, sizeof(base));
  base.a.s = sp; base.a.x = e->st_x; base.a.score = e->st_score; base.a.smix = smix;
  base.a.rtol = rtol; base.a.atol = atol; base.a.part = part; base.a.B = B; base.a.S = S; base.a.T = T;
  base.a.kidx = -1; base.a.y = y;
  base.active = d_act; base.lens = lens;
  // the fused pass after the network evaluation at the times of table row `row` (kout >= 0: K[kout] = drift), the
  // combination `mode` of K[0..nk) with the step sizes of `htab`, written for the next evaluation at row + 1
  auto pass = [&](int kout, int row, int mode, int nk, const double* c, const double* htab, bool scale_ynew = true) -> int {
    OdeEachArgs a = base;
    a.a.kout = kout >= 0 ? K[kout] : nullptr;
    a.a.tt = d_tt + (size_t)row * B;
    a.a.kidx = (kout >= 0 && kout < nk) ? kout : -1;
    a.a.nk = nk;
    for (int j = 0; j < nk; ++j) { a.a.k[j] = K[j]; a.a.c[j] = c[j]; }
    a.a.mode = mode; a.h = htab;
    if (mode == 1) a.a.xo = e->st_x;
    if (mode == 2) { a.a.yo = ynew; a.a.xo = e->st_x; }
    if (mode == 3 && scale_ynew) a.a.ynew = ynew;
    if (mode == 1 || mode == 2) { a.a.t_next_out = e->st_t; a.tnext = d_tt + (size_t)(row + 1) * B; }
    return prof_launch(e, st, hbm_rec("ode_stage_each (fused drift + RK stage)", 4.0 * nst * (2 + nk) + 8.0 * nst * (mode >= 2 ? 2 : 1), B, 1, (int)T, S),
                       [&]() { return ds_launch_ode_stage_each(a, st); });
  };
  // the norms of the last mode-3 pass -> host; commit: the device takes the accepted steps before the host knows of them
  auto read_norms = [&](bool commit) -> int {
    if (ds_launch_ode_norm_final_each(part, lens, d_act, B, S, dnorm, st)) return 1;
    if (commit && ds_launch_ode_commit_each(y, ynew, K[0], K[ns], dnorm, d_act, B, S, T, st)) return 1;
    DS_HIP(hipMemcpyAsync(pin, dnorm, (size_t)2 * B * sizeof(double), hipMemcpyDeviceToHost, st));
    if (e->ode_pin.record(st) || e->ode_pin.wait()) return 1;
    return 0;
  };

  int evals = 0;
  for (int b = 0; b < B; ++b) u[b].t = t0;
  if (ds_launch_fill(e->st_t, (float)t0, B, st)) return 1;
  if (upload()) return 1;  // everyone active, row 0 = t0
  if (run_nfe(e, B, T, st)) return 1;
  ++evals;
  for (int b = 0; b < B; ++b) ++u[b].nfev;
  const double one = 1.0;
  if (oc->first_step <= 0.0) {  // common.select_initial_step, per utterance
    const double pm[2] = {-1.0, 1.0};
    std::vector<double> d0(B), d1(B), h0(B);
    if (pass(0, 0, 3, 1, &one, d_ones, false)) return 1;  // K0 = f0; norm(f0 / scale), norm(y0 / scale)
    if (read_norms(false)) return 1;
    for (int b = 0; b < B; ++b) {
      d1[b] = pin[2 * b]; d0[b] = pin[2 * b + 1];
      h0[b] = (d0[b] < 1e-5 || d1[b] < 1e-5) ? 1e-6 : 0.01 * d0[b] / d1[b];
      h0[b] = std::min(h0[b], interval);
      hv[b] = h0[b] * dir;
      ttv[(size_t)1 * B + b] = (float)(t0 + h0[b] * dir);
    }
    if (upload()) return 1;
    if (pass(-1, 0, 1, 1, &one, d_h)) return 1;  // y1 = y0 + h0 * direction * f0
    if (run_nfe(e, B, T, st)) return 1;
    ++evals;
    if (pass(1, 1, 3, 2, pm, d_ones, false)) return 1;  // norm((f1 - f0) / scale)
    if (read_norms(false)) return 1;
    for (int b = 0; b < B; ++b) {
      ++u[b].nfev;
      const double d2 = pin[2 * b] / h0[b];
      const double h1 = (d1[b] <= 1e-15 && d2 <= 1e-15) ? std::max(1e-6, h0[b] * 1e-3)
                                                        : std::pow(0.01 / std::max(d1[b], d2), 1.0 / (eorder + 1));
      u[b].h_abs = std::min(std::min(100 * h0[b], h1), std::min(interval, max_step));
    }
  } else {
    if (pass(0, 0, 0, 0, nullptr, nullptr)) return 1;  // K0 = f0
    for (int b = 0; b < B; ++b) u[b].h_abs = oc->first_step;
  }

  const double err_exp = -1.0 / (eorder + 1);
  for (;;) {  // one step attempt of every utterance that still integrates
    int n_active = 0;
    for (int b = 0; b < B; ++b) {
      OdeCtl& c = u[b];
      act[b] = 0;
      if (c.status != 2) continue;
      if (c.new_step) {  // solve_ivp: solver.step()
        c.min_step = 10 * std::fabs(std::nextafter(c.t, dir * INFINITY) - c.t);
        if (c.h_abs > max_step) c.h_abs = max_step;
        else if (c.h_abs < c.min_step) c.h_abs = c.min_step;
        c.rejected = false;
        c.new_step = false;
      }
      if (c.h_abs < c.min_step) { c.status = -1; continue; }
      if (oc->max_nfe > 0 && c.nfev + ns > oc->max_nfe) { c.status = 1; continue; }
      double h = c.h_abs * dir;
      c.t_new = c.t + h;
      if (dir * (c.t_new - t_bound) > 0) c.t_new = t_bound;
      h = c.t_new - c.t;
      c.h_abs = std::fabs(h);
      c.h = h;
      hv[b] = h;
      for (int s = 1; s < ns; ++s) ttv[(size_t)s * B + b] = (float)(c.t + Cb[s] * h);
      ttv[(size_t)ns * B + b] = (float)(c.t + h);
      act[b] = 1;
      ++n_active;
    }
    if (!n_active) break;
    if (upload()) return 1;
    // rk_step: stage s input fp32(y + dot(K[:s].T, A[s,:s]) h) at t + C[s] h; y_new; f_new = f(t + h, y_new)
    if (pass(-1, 0, 1, 1, Ab + 1 * DS_ODE_MAX_K, d_h)) return 1;
    for (int s = 1; s <= ns; ++s) {
      if (run_nfe(e, B, T, st)) return 1;
      ++evals;
      if (s < ns - 1) {
        if (pass(s, s, 1, s + 1, Ab + (s + 1) * DS_ODE_MAX_K, d_h)) return 1;
      } else if (s == ns - 1) {
        if (pass(s, s, 2, ns, Bb, d_h)) return 1;
      } else {
        if (pass(s, s, 3, ns + 1, Eb, d_h)) return 1;
      }
    }
    if (read_norms(true)) return 1;
    for (int b = 0; b < B; ++b) {
      if (!act[b]) continue;
      OdeCtl& c = u[b];
      c.nfev += ns;
      const double err = pin[2 * b];
      if (err < 1) {
        double factor = err == 0 ? 10.0 : std::min(10.0, 0.9 * std::pow(err, err_exp));
        if (c.rejected) factor = std::min(1.0, factor);
        c.h_abs *= factor;
        c.t = c.t_new;  // (y <- y_new, f <- f_new: taken on the device)
        ++c.n_acc;
        c.new_step = true;
        if (dir * (c.t - t_bound) >= 0) c.status = 0;
      } else {
        c.h_abs *= std::max(0.2, 0.9 * std::pow(err, err_exp));
        c.rejected = true;
        ++c.n_rej;
      }
    }
  }

  // the last accepted states -> float32; optional denoise as in diffsep_ode_sample, the tails staying zero
  if (ds_launch_ode_round(y, e->st_x, (long)nst, st)) return 1;
  if (oc->denoise) {
    if (ds_launch_fill(e->st_t, (float)eps, B, st)) return 1;
    if (run_nfe(e, B, T, st)) return 1;
    if (ds_launch_sde_predictor(sp, oc->N, e->st_x, e->st_t, e->st_score, nullptr, e->st_xm, out, B, S, T, smix, 0, st,
                                lengths ? lens : nullptr))
      return 1;
  } else {
    DS_HIP(hipMemcpyAsync(out, e->st_x, nst * 4, hipMemcpyDeviceToDevice, st));
  }
  if (infos)
    for (int b = 0; b < B; ++b) {
      infos[b].nfev = u[b].nfev; infos[b].n_accepted = u[b].n_acc; infos[b].n_rejected = u[b].n_rej;
      infos[b].status = u[b].status; infos[b].t_final = u[b].t;
    }
  if (evals_run) *evals_run = evals;
  return 0;
}
