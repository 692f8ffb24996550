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

// What every entry asks of the SDE description (`who`: the entry point's name in the message)
int check_sde(const diffsep_engine* e, const diffsep_sde_config* sde, const char* who) {
  const std::string w(who);
  DS_CHECK(sde->kind == DIFFSEP_SDE_MIX || sde->kind == DIFFSEP_SDE_PRIORMIX, w + ": unknown SDE kind");
  DS_CHECK(sde->kind == DIFFSEP_SDE_MIX || sde->avg_len >= 1, w + ": PriorMixSDE needs avg_len >= 1");
  DS_CHECK(sde->ndim == e->cfg.num_sources, w + ": sde.ndim != num_sources");
  return 0;
}
// PriorMixSDE: the per-sample noise scale from the envelope of the mixture in st_mix (sdes.py:477-489); MixSDE: none (null)
int mixture_scale(diffsep_engine* e, const diffsep_sde_config* sde, int B, long T, hipStream_t st, const float** smix) {
  *smix = nullptr;
  if (sde->kind != DIFFSEP_SDE_PRIORMIX) return 0;
  if (ds_launch_sigma_mix(e->st_mix, e->st_smix, B, T, sde->avg_len, st)) return 1;
  *smix = e->st_smix;
  return 0;
}

// What every entry asks of the batch extensions (diffsep_sampler_ext / diffsep_ode_ext, by field), before anything is
// enqueued: the other engine, seeds against host noise, the lengths of a zero-padded batch.  A null field is not checked.
int check_batch_ext(const diffsep_model_config* cfg, const char* who, int B, long T, const int64_t* lengths,
                    const uint64_t* seeds, const float* noise, const diffsep_engine* e, const diffsep_engine* tail) {
  const std::string w(who);
  if (tail) {
    const std::string must = w + ": the tail engine must ";
    DS_CHECK(tail != e, must + "be a different engine");
    diffsep_model_config a = e->cfg, b2 = tail->cfg;
    a.dtype = b2.dtype = 0;
    DS_CHECK(memcmp(&a, &b2, sizeof(a)) == 0, must + "have the same architecture");
  }
  DS_CHECK(!seeds || !noise, w + ": per-utterance seeds are for device noise (noise == NULL)");
  if (lengths) {
    const int Wp = diffsep_padded_frames(cfg, T);
    for (int b = 0; b < B; ++b) {
      DS_CHECK(lengths[b] >= 1 && lengths[b] <= T, w + ": utterance length outside [1, T]");
      DS_CHECK(diffsep_padded_frames(cfg, lengths[b]) == Wp,
               w + ": every utterance of a mixed-length batch must have the padded frame count of T");
    }
  }
  return 0;
}

namespace {
// The batch as the entries below see it on the device.  Which parts an entry uses decides the bits of its result, so each
// choice is an argument of the two functions that fill this.
struct SamplerBatch {
  const int* lens = nullptr;       // st_lens once uploaded (T where no lengths are given): what per-utterance passes read
  const int* tail_lens = nullptr;  // st_lens of a batch WITH lengths: what masks a tail
  const float* smix = nullptr;     // PriorMixSDE's noise scale
};

// The evaluation of one step's score: on e, or — in the first head_steps and last tail_steps of n_steps steps — on the other
// engine (mixture once, state and time every time copied over; the score read from there).
struct ScoreEval {
  diffsep_engine *e, *tail;
  int head_steps, tail_steps, n_steps, B;
  long T;
  size_t nst;
  hipStream_t st;
  bool tail_ready = false;
  const float* score;  // where the last evaluation left it
  // the other engine an extension names: none unless it gives it a step
  static diffsep_engine* other(const diffsep_sampler_ext* ext) {
    return (ext && (ext->tail_steps > 0 || ext->head_steps > 0)) ? ext->tail_engine : nullptr;
  }
  ScoreEval(diffsep_engine* e_, diffsep_engine* tail_, const diffsep_sampler_ext* ext, int n_steps_, int B_, long T_,
            size_t nst_, hipStream_t st_)
      : e(e_), tail(tail_), head_steps(tail_ ? ext->head_steps : 0), tail_steps(tail_ ? ext->tail_steps : 0),
        n_steps(n_steps_), B(B_), T(T_), nst(nst_), st(st_), score(e_->st_score) {}
  int eval(int i) {
    if (tail && (i >= n_steps - tail_steps || i < head_steps)) {
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
  }
};
}  // namespace

// mixture -> st_mix; with `upload` seeds (given, or seed + b * stride: b = 0 is the B = 1 stream of `seed`) and lengths (T
// where none are given) -> st_seeds, st_lens through pinned staging, stream-ordered; the mixture's tails zeroed
static int batch_mixture(diffsep_engine* e, SamplerBatch& sb, const float* mix_norm, int B, long T, const int64_t* lengths,
                         const uint64_t* seeds, uint64_t seed, bool upload, hipStream_t st) {
  DS_HIP(hipMemcpyAsync(e->st_mix, mix_norm, (size_t)B * T * 4, hipMemcpyDeviceToDevice, st));
  if (!upload) return 0;
  char* pin;
  if (e->ext_pin.acquire((size_t)B * 16, &pin)) return 1;
  unsigned long long* ps = reinterpret_cast<unsigned long long*>(pin);
  int* pl = reinterpret_cast<int*>(pin + (size_t)B * 8);
  for (int b = 0; b < B; ++b) {
    ps[b] = seeds ? seeds[b] : seed + 0x9E3779B97F4A7C15ull * (unsigned long long)b;
    pl[b] = lengths ? (int)lengths[b] : (int)T;
  }
  DS_HIP(hipMemcpyAsync(e->st_seeds, ps, (size_t)B * 8, hipMemcpyHostToDevice, st));
  DS_HIP(hipMemcpyAsync(e->st_lens, pl, (size_t)B * 4, hipMemcpyHostToDevice, st));
  if (e->ext_pin.record(st)) return 1;
  sb.lens = e->st_lens;
  sb.tail_lens = lengths ? e->st_lens : nullptr;
  return lengths ? ds_launch_mask_tail(e->st_mix, B, 1, T, sb.lens, st) : 0;
}

// sigma_mix, then the start state -> st_x: the caller's x_init with its tails zeroed like the mixture's, or the prior sample
// from z — null: from draw 0 of the device generator, the PC sampler's prior draw, keyed per utterance (st_seeds, st_lens)
// with batch_rng and by `seed` for the whole batch without.  prior_lens: the lengths the prior sample is cut to, if any.
static int batch_start(diffsep_engine* e, const diffsep_sde_config* sde, SamplerBatch& sb, int B, long T, const float* x_init,
                       const float* z, bool batch_rng, uint64_t seed, const int* prior_lens, hipStream_t st) {
  const int S = e->cfg.num_sources;
  const size_t nst = (size_t)B * S * T;
  if (mixture_scale(e, sde, B, T, st, &sb.smix)) return 1;
  if (x_init) {
    DS_HIP(hipMemcpyAsync(e->st_x, x_init, nst * 4, hipMemcpyDeviceToDevice, st));
    return sb.tail_lens ? ds_launch_mask_tail(e->st_x, B, S, T, sb.tail_lens, st) : 0;
  }
  if (!z) {
    if (batch_rng ? ds_launch_randn_batch(e->st_noise, B, S, T, (const uint64_t*)e->st_seeds, e->st_lens, 0, st)
                  : ds_launch_randn(e->st_noise, (long)nst, seed, 0, st))
      return 1;
    z = e->st_noise;
  }
  return ds_launch_sde_prior(to_sdep(sde), e->st_mix, z, e->st_x, B, S, T, sb.smix, st, prior_lens);
}

// The sampler, with an optional tap on its intermediate states (reference sdes/__init__.py:168-186, `intermediate`; the
// figure of evaluate.py:29-61 is drawn from them) and with both ends open: a caller-supplied state instead of the prior and a
// range [first_step, last_step) of the N reverse steps (diffsep_pc_sample_from; the three older entries forward to it with
// {NULL, 0, 0}).  In reverse step i, after the corrector step(s) and before the predictor — where the reference appends
// (xt, xt_mean) — one launch (sde.hip: trace_tap_kernel) copies the state of the chosen steps and adds up the Gram sums of
// every step against `target`.  The state lives on `e` whichever engine evaluates the score, and the tap is a stream launch
// between graph replays: the captured graphs are those of the untraced call.  With nothing to trace (n_snap == 0,
// target == NULL) and no range not one launch, copy or allocation is added: that is diffsep_pc_sample_ex.
// Steps are absolute indices of the N-point grid: step i runs at ts[i] with dt = 1/N and consumes the draws
// 1 + i (csteps + npred) ... of the device RNG (draw 0 is the prior's), whatever step the call starts at.
extern "C" int32_t diffsep_pc_sample_from(diffsep_engine* e, const diffsep_sde_config* sde,
                                          const diffsep_sampler_config* smp, const diffsep_sampler_ext* ext,
                                          const float* mix_norm, float* out, int32_t B, int64_t T, const float* noise,
                                          uint64_t seed, const float* timesteps_host, int32_t* nfe_out, int32_t n_snap,
                                          const int32_t* snap_steps_host, float* snap_x, float* snap_xm,
                                          const float* target, double* gram, const float* x_init, int32_t first_step,
                                          int32_t last_step, void* stream) {
  DS_CHECK(e && sde && smp && mix_norm && out, "pc_sample: null argument");
  if (check_sde(e, sde, "pc_sample")) return 1;
  DS_CHECK(smp->N >= 1 && smp->N <= 4096, "pc_sample: N must be in [1,4096]");
  const int first = first_step, last = last_step == 0 ? smp->N : last_step;
  DS_CHECK(first >= 0 && first < last && last <= smp->N,
           "pc_sample: the step range must satisfy 0 <= first_step < last_step <= N (last_step 0 = N)");
  DS_CHECK(first == 0 || x_init, "pc_sample: first_step > 0 needs the state to start from (x_init == NULL)");
  DS_CHECK(n_snap >= 0 && (n_snap == 0 || snap_steps_host), "pc_sample: n_snap snapshot steps are needed");
  DS_CHECK(n_snap == 0 || snap_x, "pc_sample: snapshots were requested without a buffer (snap_x == NULL)");
  for (int k = 0; k < n_snap; ++k)
    DS_CHECK(snap_steps_host[k] >= first && snap_steps_host[k] < last && (k == 0 || snap_steps_host[k] > snap_steps_host[k - 1]),
             "pc_sample: the snapshot steps must be strictly ascending and in [0, N), within the executed steps [first_step, last_step)");
  DS_CHECK(!target == !gram, "pc_sample: target and gram are given together or not at all");
  DS_CHECK(!(n_snap || target) || e->cfg.num_sources <= DS_MAX_SRC, "pc_sample: too many sources to trace");
  if (n_snap == 0) snap_x = snap_xm = nullptr;
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
  diffsep_engine* tail = ScoreEval::other(ext);
  DS_CHECK(!lengths || smp->corrector != DIFFSEP_CORR_LANGEVIN,
           "pc_sample: the 'langevin' corrector couples the batch entries; it cannot run on a mixed-length batch");
  if (check_batch_ext(&e->cfg, "pc_sample", B, T, lengths, seeds, noise, e, tail)) return 1;
  // (head_steps / tail_steps are absolute steps: a range that holds none of them never touches the other engine)
  if (tail && !(first < ext->head_steps || last > smp->N - ext->tail_steps)) tail = nullptr;
  StreamScope sc_(e, stream);
  hipStream_t st = sc_.st;
  const int S = e->cfg.num_sources, N = smp->N;
  const int csteps = smp->corrector == DIFFSEP_CORR_NONE ? 0 : smp->corrector_steps;
  const int npred = smp->predictor == DIFFSEP_PRED_NONE ? 0 : 1;
  if (ensure_plan(e, B, T, st)) return 1;
  if (tail && ensure_plan(tail, B, T, st)) return 1;
  const size_t nst = (size_t)B * S * T;
  const size_t ngram = (size_t)B * 3 * S * S;  // doubles of one row of `gram`
  int snap_next = 0;
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
  SamplerBatch sb;  // (seeds and lengths go up only when the extension gives one of them)
  if (batch_mixture(e, sb, mix_norm, B, T, lengths, seeds, seed, lengths || seeds, st)) return 1;
  const int* lens = sb.tail_lens;
  const bool batch_rng = !noise && (seeds || lengths);

  long draw = x_init ? 1 + (long)first * (csteps + npred) : 0;  // (a given state: draw 0, the prior's, is not generated)
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
  if (!x_init && next_noise(&z)) return 1;
  if (batch_start(e, sde, sb, B, T, x_init, z, batch_rng, seed, lens, st)) return 1;  // (z: drawn above, counted and profiled)
  const float* smix = sb.smix;
  DS_HIP(hipMemcpyAsync(e->st_xm, e->st_x, nst * 4, hipMemcpyDeviceToDevice, st));
  ScoreEval ev(e, tail, ext, N, B, T, nst, st);  // reverse step i is step i of N
  for (int i = first; i < last; ++i) {
    DS_HIP(hipMemcpyAsync(e->st_t, e->st_ts + (size_t)i * B, (size_t)B * 4, hipMemcpyDeviceToDevice, st));
    for (int k = 0; k < csteps; ++k) {
      if (ev.eval(i)) return 1;
      if (next_noise(&z)) return 1;
      if (smp->corrector == DIFFSEP_CORR_LANGEVIN) {
        if (ds_launch_langevin(smp->snr, e->st_x, ev.score, z, e->st_x, e->st_xm, B, (long)S * T, e->st_lang, st))
          return 1;
      } else if (prof_launch(e, st, hbm_rec("sde_corrector (ald2 update)", 4.0 * nst * 5.0, B, 1, (int)T, S), [&]() {  // x, score, z in; x, x_mean out
                   return ds_launch_sde_corrector(sp, smp->snr, e->st_x, e->st_t, ev.score, z, e->st_x, e->st_xm, B, S, T,
                                                  smix, smp->corrector == DIFFSEP_CORR_ALD ? 1 : 0, st, lens);
                 })) {
        return 1;
      }
    }
    if (snap_next < n_snap || target) {  // the tap: (x, x_mean) as the corrector left them
      const int k = (snap_next < n_snap && snap_steps_host[snap_next] == i) ? snap_next++ : -1;
      if (k >= 0 || target) {
        float* sx = k >= 0 ? snap_x + (size_t)k * nst : nullptr;
        float* sxm = (k >= 0 && snap_xm) ? snap_xm + (size_t)k * nst : nullptr;
        // without a corrector step the reference's "corrector" returns (x, x): st_xm still holds the last predictor's mean
        const float* xm = csteps > 0 ? e->st_xm : e->st_x;
        double* g = target ? gram + (size_t)i * ngram : nullptr;
        const double words = 1.0 + (target ? 1.0 : 0.0) + (sx ? 1.0 : 0.0) + (sxm ? 2.0 : 0.0);
        if (prof_launch(e, st, hbm_rec("trace_tap (state snapshot + Gram sums)", 4.0 * nst * words, B, 1, (int)T, S),
                        [&]() { return ds_launch_trace_tap(e->st_x, xm, target, sx, sxm, g, B, S, T, st); }))
          return 1;
      }
    }
    if (smp->predictor != DIFFSEP_PRED_NONE) {
      // euler_maruyama (sdes/predictors.py:39-52) takes x + f*dt with the reverse drift f = drift - g^2 score and
      // noise g sqrt(dt): algebraically the reverse_diffusion step (dt = 1/N, G = g sqrt(dt)) — one kernel for both
      if (ev.eval(i)) return 1;
      if (next_noise(&z)) return 1;
      if (prof_launch(e, st, hbm_rec("sde_predictor (reverse-diffusion update)", 4.0 * nst * 5.0, B, 1, (int)T, S), [&]() {
            return ds_launch_sde_predictor(sp, N, e->st_x, e->st_t, ev.score, z, e->st_x, e->st_xm, B, S, T, smix, 0, st, lens);
          }))
        return 1;
    } else {
      DS_HIP(hipMemcpyAsync(e->st_xm, e->st_x, nst * 4, hipMemcpyDeviceToDevice, st));
    }
  }
  // a run that stops before step N hands out the state x itself, whatever `denoise` says: it can be resumed from it
  DS_HIP(hipMemcpyAsync(out, (smp->denoise && last == N) ? e->st_xm : e->st_x, nst * 4, hipMemcpyDeviceToDevice, st));
  if (target && last == N && ds_launch_gram(target, out, gram + (size_t)N * ngram, B, S, T, st)) return 1;  // row N: the result itself
  if (nfe_out) *nfe_out = (last - first) * (csteps + 1);
  return 0;
}

extern "C" int32_t diffsep_pc_sample_trace(diffsep_engine* e, const diffsep_sde_config* sde,
                                           const diffsep_sampler_config* smp, const diffsep_sampler_ext* ext,
                                           const float* mix_norm, float* out, int32_t B, int64_t T, const float* noise,
                                           uint64_t seed, const float* timesteps_host, int32_t* nfe_out, int32_t n_snap,
                                           const int32_t* snap_steps_host, float* snap_x, float* snap_xm,
                                           const float* target, double* gram, void* stream) {
  return diffsep_pc_sample_from(e, sde, smp, ext, mix_norm, out, B, T, noise, seed, timesteps_host, nfe_out, n_snap,
                                snap_steps_host, snap_x, snap_xm, target, gram, nullptr, 0, 0, stream);
}

extern "C" int32_t diffsep_pc_sample_ex(diffsep_engine* e, const diffsep_sde_config* sde,
                                        const diffsep_sampler_config* smp, const diffsep_sampler_ext* ext,
                                        const float* mix_norm, float* out, int32_t B, int64_t T, const float* noise,
                                        uint64_t seed, const float* timesteps_host, int32_t* nfe_out, void* stream) {
  return diffsep_pc_sample_trace(e, sde, smp, ext, mix_norm, out, B, T, noise, seed, timesteps_host, nfe_out, 0, nullptr,
                                 nullptr, nullptr, nullptr, nullptr, stream);
}

extern "C" int32_t diffsep_pc_sample(diffsep_engine* e, const diffsep_sde_config* sde, const diffsep_sampler_config* smp,
                                     const float* mix_norm, float* out, int32_t B, int64_t T, const float* noise,
                                     uint64_t seed, const float* timesteps_host, int32_t* nfe_out, void* stream) {
  return diffsep_pc_sample_ex(e, sde, smp, nullptr, mix_norm, out, B, T, noise, seed, timesteps_host, nfe_out, stream);
}

// ------------------------------------------------------------------ probability-flow ODE sampler
// sdes.get_ode_sampler(...)() (reference sdes/__init__.py:193-278): scipy.integrate.solve_ivp(RK45 | RK23) on the
// probability-flow ODE.  scipy's controller runs on the host (ode_host.h: OdePlan, OdeCtl — one copy for both entries
// below); every stage is one graph-replayed network evaluation (run_nfe) + one fused pass (ode.hip), every step attempt one
// pinned readback of its error norm.
namespace {
// the solver's device state, carved from the engine's ODE buffer: y, y_new, K[], then per system (the whole batch, or each
// utterance) a partial-sum slab and two norms, then the entry's upload tables
struct OdeWork {
  double *y, *ynew;
  float* K[DS_ODE_MAX_K];
  double *part, *dnorm;
  char* tab;
};
}  // namespace

static int ode_workspace(diffsep_engine* e, size_t nst, int n_sys, size_t tab_bytes, OdeWork& w) {
  auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t part_bytes = al((size_t)n_sys * 2 * DS_ODE_MAX_BLOCKS * 8), norm_bytes = al((size_t)n_sys * 16);
  const size_t need = 2 * al(nst * 8) + DS_ODE_MAX_K * al(nst * 4) + part_bytes + norm_bytes + al(tab_bytes);
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
  char* p = e->ode_buf;
  w.y = (double*)p; p += al(nst * 8);
  w.ynew = (double*)p; p += al(nst * 8);
  for (int j = 0; j < DS_ODE_MAX_K; ++j) { w.K[j] = (float*)p; p += al(nst * 4); }
  w.part = (double*)p; p += part_bytes;
  w.dnorm = (double*)p; p += norm_bytes;
  w.tab = p;
  return 0;
}

// The fused pass after a network evaluation: K[kout] = drift (kout >= 0), then the combination `mode` of K[0..nk) with
// coefficients c, written for the next evaluation (mode 3: the error scale from max(|y|, |y_new|), or from |y| alone in
// select_initial_step).  The times and the step size are the caller's: scalars for the whole batch, tables per utterance.
static OdeArgs ode_pass_args(const diffsep_engine* e, const OdeArgs& base, const OdeWork& w, int kout, int mode, int nk,
                             const double* c, bool scale_ynew = true) {
  OdeArgs a = base;
  a.kout = kout >= 0 ? w.K[kout] : nullptr;
  a.kidx = (kout >= 0 && kout < nk) ? kout : -1;
  a.nk = nk;
  for (int j = 0; j < nk; ++j) { a.k[j] = w.K[j]; a.c[j] = c[j]; }
  a.mode = mode; a.y = w.y;
  if (mode == 1) a.xo = e->st_x;
  if (mode == 2) { a.yo = w.ynew; a.xo = e->st_x; }
  if (mode == 3 && scale_ynew) a.ynew = w.ynew;
  if (mode == 1 || mode == 2) a.t_next_out = e->st_t;
  return a;
}
static OdeArgs ode_base_args(const diffsep_engine* e, const SdeP& sp, const float* smix, const OdePlan& plan,
                             const OdeWork& w, int B, int S, long T) {
  OdeArgs base;
  memset(&base, 0, sizeof(base));
  base.s = sp; base.x = e->st_x; base.score = e->st_score; base.smix = smix;
  base.rtol = plan.rtol; base.atol = plan.atol; base.part = w.part; base.B = B; base.S = S; base.T = T;
  base.kidx = -1;
  return base;
}
static diffsep_engine::ProfRec ode_pass_rec(const char* name, size_t nst, int nk, int mode, int B, long T, int S) {
  return hbm_rec(name, 4.0 * nst * (2 + nk) + 8.0 * nst * (mode >= 2 ? 2 : 1), B, 1, (int)T, S);
}

// solution.y[:, -1] (the last accepted state) -> float32; optional denoise: x_mean of one reverse_diffusion step at eps
// without noise (reference denoise_update_fn; dt = 1/N, quirk Q1).  lens: the tails of a zero-padded batch stay zero.
static int ode_finish(diffsep_engine* e, const SdeP& sp, double eps, int denoise, int N, const float* smix, const double* y,
                      float* out, int B, int S, long T, const int* lens, hipStream_t st) {
  const size_t nst = (size_t)B * S * T;
  if (ds_launch_ode_round(y, e->st_x, (long)nst, st)) return 1;
  if (denoise) {
    if (ds_launch_fill(e->st_t, (float)eps, B, st)) return 1;
    if (run_nfe(e, B, T, st)) return 1;
    if (ds_launch_sde_predictor(sp, N, e->st_x, e->st_t, e->st_score, nullptr, e->st_xm, out, B, S, T, smix, 0, st, lens))
      return 1;
  } else {
    DS_HIP(hipMemcpyAsync(out, e->st_x, nst * 4, hipMemcpyDeviceToDevice, st));
  }
  return 0;
}
static void ode_info(const OdeCtl& c, diffsep_ode_info* info) {
  info->nfev = c.nfev; info->n_accepted = c.n_acc; info->n_rejected = c.n_rej; info->status = c.status; info->t_final = c.t;
}

extern "C" int32_t diffsep_ode_sample(diffsep_engine* e, const diffsep_sde_config* sde, const diffsep_ode_config* oc,
                                      const float* mix_norm, const float* x_init, const float* noise, uint64_t seed,
                                      float* out, int32_t B, int64_t T, diffsep_ode_info* info, void* stream) {
  DS_CHECK(e && sde && oc && mix_norm && out, "ode_sample: null argument");
  if (check_sde(e, sde, "ode_sample")) return 1;
  DS_CHECK(B >= 1 && T >= 1, "ode_sample: empty batch");
  DS_CHECK(!(x_init && noise), "ode_sample: x_init and noise are alternatives");
  OdePlan plan;
  const std::string bad = ode_plan_fill(plan, *oc, "ode_sample");
  DS_CHECK(bad.empty(), bad);
  const int ns = plan.ns;

  StreamScope sc_(e, stream);
  hipStream_t st = sc_.st;
  const int S = e->cfg.num_sources;
  if (ensure_plan(e, B, T, st)) return 1;
  const size_t nst = (size_t)B * S * T;
  OdeWork w;
  if (ode_workspace(e, nst, 1, 0, w)) return 1;
  double* pin;  // pinned readback of the two norms
  if (e->ode_pin.acquire(2, &pin)) return 1;
  const SdeP sp = to_sdep(sde);

  // x_T -> st_x (and y = x_T in fp64)
  SamplerBatch sb;  // (no extension: nothing is uploaded, the prior draw is the whole batch's, nothing is cut or masked)
  if (batch_mixture(e, sb, mix_norm, B, T, nullptr, nullptr, seed, false, st)) return 1;
  if (batch_start(e, sde, sb, B, T, x_init, noise, false, seed, nullptr, st)) return 1;
  const float* smix = sb.smix;
  if (ds_launch_ode_cast(e->st_x, w.y, (long)nst, st)) return 1;

  const OdeArgs base = ode_base_args(e, sp, smix, plan, w, B, S, T);
  // one pass after the evaluation at (float) t_eval, written for the next evaluation at (float) t_next; name: its profile
  // record (null: none)
  auto pass = [&](int kout, double t_eval, int mode, int nk, const double* c, double h, double t_next, int* nblk,
                  bool scale_ynew = true, const char* name = "ode_stage (fused drift + RK stage)") -> int {
    OdeArgs a = ode_pass_args(e, base, w, kout, mode, nk, c, scale_ynew);
    a.t = (float)t_eval; a.h = h; a.t_next = (float)t_next;
    if (!name) return ds_launch_ode_stage(a, st, nblk);
    const diffsep_engine::ProfRec rec = kout < 0 ? hbm_rec(name, 16.0 * nst, B, 1, (int)T, S) : ode_pass_rec(name, nst, nk, mode, B, T, S);
    return prof_launch(e, st, rec, [&]() { return ds_launch_ode_stage(a, st, nblk); });
  };
  // the two norms of the last mode-3 pass -> host (stream-ordered pinned readback, waited on by its event)
  auto read_norms = [&](int nblk, double* n0, double* n1) -> int {
    if (ds_launch_ode_norm_final(w.part, nblk, (long)nst, w.dnorm, st)) return 1;
    DS_HIP(hipMemcpyAsync(pin, w.dnorm, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
    if (e->ode_pin.record(st) || e->ode_pin.wait()) return 1;
    *n0 = pin[0];
    if (n1) *n1 = pin[1];
    return 0;
  };

  OdeCtl c;
  c.t = plan.t0;
  if (ds_launch_fill(e->st_t, (float)c.t, B, st)) return 1;
  if (run_nfe(e, B, T, st)) return 1;
  ++c.nfev;
  const double one = 1.0;
  int nb = 0;
  if (plan.first_step <= 0.0) {  // common.select_initial_step
    const double pm[2] = {-1.0, 1.0};
    double d0, d1, d2;
    if (pass(0, c.t, 3, 1, &one, 1.0, 0.0, &nb, false)) return 1;  // K0 = f0; norm(f0 / scale), norm(y0 / scale)
    if (read_norms(nb, &d1, &d0)) return 1;
    const double h0 = OdeCtl::initial_h0(plan, d0, d1), t1 = plan.t0 + h0 * plan.dir;
    if (pass(-1, 0.0, 1, 1, &one, h0 * plan.dir, t1, nullptr, true, nullptr)) return 1;  // y1 = y0 + h0 * direction * f0
    if (run_nfe(e, B, T, st)) return 1;
    ++c.nfev;
    if (pass(1, t1, 3, 2, pm, 1.0, 0.0, &nb, false)) return 1;  // norm((f1 - f0) / scale)
    if (read_norms(nb, &d2, nullptr)) return 1;
    c.initial_step(plan, d1, d2, h0);
  } else {
    if (pass(0, c.t, 0, 0, nullptr, 0.0, 0.0, nullptr)) return 1;  // K0 = f0
    c.h_abs = plan.first_step;
  }

  while (c.begin_attempt(plan)) {  // solve_ivp: while status is None: solver.step(), one attempt of a step per trip
    // rk_step: stage s input fp32(y + dot(K[:s].T, A[s,:s]) h) at t + C[s] h; y_new; f_new = f(t + h, y_new)
    if (pass(-1, 0.0, 1, 1, plan.A + 1 * DS_ODE_MAX_K, c.h, c.stage_time(plan, 1), nullptr, true, "ode_stage (RK stage input)"))
      return 1;
    for (int s = 1; s <= ns; ++s) {
      if (run_nfe(e, B, T, st)) return 1;
      const double ts = c.stage_time(plan, s);
      if (s < ns - 1) {
        if (pass(s, ts, 1, s + 1, plan.A + (s + 1) * DS_ODE_MAX_K, c.h, c.stage_time(plan, s + 1), nullptr)) return 1;
      } else if (s == ns - 1) {
        if (pass(s, ts, 2, ns, plan.B, c.h, c.stage_time(plan, ns), nullptr)) return 1;
      } else {
        if (pass(s, ts, 3, ns + 1, plan.E, c.h, 0.0, &nb)) return 1;
      }
    }
    double err;
    if (read_norms(nb, &err, nullptr)) return 1;
    if (c.end_attempt(plan, err)) {  // y <- y_new, f <- f_new: pointer swaps, no copies
      std::swap(w.y, w.ynew);
      std::swap(w.K[0], w.K[ns]);
    }
  }

  if (ode_finish(e, sp, oc->eps, oc->denoise, oc->N, smix, w.y, out, B, S, T, nullptr, st)) return 1;
  if (info) ode_info(c, info);
  return 0;
}

// ------------------------------------------------------------------ ... with one step controller per utterance
// B controllers in lock step on a zero-padded batch: utterance b has its own OdeCtl — its own t, h, error norm, accept /
// reject decisions and counts, the same code as diffsep_ode_sample's one — and all utterances share every network
// evaluation.  One step attempt = one upload of its tables (h, active, the evaluation times of its stages: a row per pass,
// so that no pass waits for the host), n_stages evaluations of the whole batch, and one pinned readback of the 2 B norms.
// The device takes the accepted steps itself (ode_commit_each_kernel: norm < 1, the host's own test on the same number).
// An utterance whose status is set is frozen: its rows ride through the network, its state is not touched.
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
  if (check_batch_ext(&e->cfg, "ode_sample_each", B, T, lengths, nullptr, nullptr, nullptr, nullptr)) return 1;  // (seeds: above)
  OdePlan plan;
  const std::string bad = ode_plan_fill(plan, *oc, "ode_sample_each");
  DS_CHECK(bad.empty(), bad);
  const int ns = plan.ns;

  StreamScope sc_(e, stream);
  hipStream_t st = sc_.st;
  const int S = e->cfg.num_sources;
  if (ensure_plan(e, B, T, st)) return 1;
  const size_t nst = (size_t)B * S * T;
  // device tables of one attempt: h [B] | ones [B] (fp64) | active [B] (int) | evaluation times [DS_ODE_MAX_K + 1][B] (fp32)
  const int n_trows = DS_ODE_MAX_K + 1;
  const size_t off_ones = (size_t)B * 8, off_act = (size_t)B * 16, off_tt = (size_t)B * 20;
  const size_t tab_bytes = (size_t)B * (20 + 4 * n_trows);
  OdeWork w;
  if (ode_workspace(e, nst, B, tab_bytes, w)) return 1;
  double* pin;  // pinned readback of the 2 B norms
  if (e->ode_pin.acquire((size_t)2 * B, &pin)) return 1;
  const double* d_h = (const double*)w.tab;
  const double* d_ones = (const double*)(w.tab + off_ones);
  const int* d_act = (const int*)(w.tab + off_act);
  const float* d_tt = (const float*)(w.tab + off_tt);
  const SdeP sp = to_sdep(sde);

  // mixture, lengths and seeds -> device; x_T -> st_x with a zero tail (and y = x_T in fp64)
  // (always uploaded; the prior draw always keyed per utterance — utterance b: draw 0 of the B = 1 stream of its seed — and
  // the prior sample always cut to the lengths, T where none are given)
  SamplerBatch sb;
  if (batch_mixture(e, sb, mix_norm, B, T, lengths, seeds, seed, true, st)) return 1;
  if (batch_start(e, sde, sb, B, T, x_init, noise, true, seed, sb.lens, st)) return 1;
  const int* lens = sb.lens;
  const float* smix = sb.smix;
  if (ds_launch_ode_cast(e->st_x, w.y, (long)nst, st)) return 1;
  std::vector<OdeCtl> u(B);
  std::vector<int> act(B, 1);
  std::vector<double> hv(B, 1.0);
  std::vector<float> ttv((size_t)n_trows * B, (float)plan.t0);
  // this attempt's tables -> device (the staging buffer is free again once the previous upload has gone through)
  auto upload = [&]() -> int {
    char* tp;
    if (e->ode_tab_pin.acquire(tab_bytes, &tp)) return 1;
    double* ph = reinterpret_cast<double*>(tp);
    double* po = reinterpret_cast<double*>(tp + off_ones);
    int* pa = reinterpret_cast<int*>(tp + off_act);
    for (int b = 0; b < B; ++b) { ph[b] = hv[b]; po[b] = 1.0; pa[b] = act[b]; }
    memcpy(tp + off_tt, ttv.data(), ttv.size() * 4);
    DS_HIP(hipMemcpyAsync(w.tab, tp, tab_bytes, hipMemcpyHostToDevice, st));
    return e->ode_tab_pin.record(st);
  };

  const OdeArgs base = ode_base_args(e, sp, smix, plan, w, B, S, T);
  // one pass after the evaluation at the times of table row `row`, with the step sizes of `htab`, written for the next
  // evaluation at row + 1
  auto pass = [&](int kout, int row, int mode, int nk, const double* c, const double* htab, bool scale_ynew = true) -> int {
    OdeEachArgs a;
    a.a = ode_pass_args(e, base, w, kout, mode, nk, c, scale_ynew);
    a.a.tt = d_tt + (size_t)row * B;
    a.h = htab; a.active = d_act; a.lens = lens;
    a.tnext = a.a.t_next_out ? d_tt + (size_t)(row + 1) * B : nullptr;
    return prof_launch(e, st, ode_pass_rec("ode_stage_each (fused drift + RK stage)", nst, nk, mode, B, T, S),
                       [&]() { return ds_launch_ode_stage_each(a, st); });
  };
  // the norms of the last mode-3 pass -> host; commit: the device takes the accepted steps before the host knows of them
  auto read_norms = [&](bool commit) -> int {
    if (ds_launch_ode_norm_final_each(w.part, lens, d_act, B, S, w.dnorm, st)) return 1;
    if (commit && ds_launch_ode_commit_each(w.y, w.ynew, w.K[0], w.K[ns], w.dnorm, d_act, B, S, T, st)) return 1;
    DS_HIP(hipMemcpyAsync(pin, w.dnorm, (size_t)2 * B * sizeof(double), hipMemcpyDeviceToHost, st));
    if (e->ode_pin.record(st) || e->ode_pin.wait()) return 1;
    return 0;
  };

  int evals = 0;
  for (int b = 0; b < B; ++b) u[b].t = plan.t0;
  if (ds_launch_fill(e->st_t, (float)plan.t0, B, st)) return 1;
  if (upload()) return 1;  // everyone active, row 0 = t0
  if (run_nfe(e, B, T, st)) return 1;
  ++evals;
  for (int b = 0; b < B; ++b) ++u[b].nfev;
  const double one = 1.0;
  if (plan.first_step <= 0.0) {  // common.select_initial_step, per utterance
    const double pm[2] = {-1.0, 1.0};
    std::vector<double> d1(B), h0(B);
    if (pass(0, 0, 3, 1, &one, d_ones, false)) return 1;  // K0 = f0; norm(f0 / scale), norm(y0 / scale)
    if (read_norms(false)) return 1;
    for (int b = 0; b < B; ++b) {
      d1[b] = pin[2 * b];
      h0[b] = OdeCtl::initial_h0(plan, pin[2 * b + 1], d1[b]);
      hv[b] = h0[b] * plan.dir;
      ttv[(size_t)1 * B + b] = (float)(plan.t0 + h0[b] * plan.dir);
    }
    if (upload()) return 1;
    if (pass(-1, 0, 1, 1, &one, d_h)) return 1;  // y1 = y0 + h0 * direction * f0
    if (run_nfe(e, B, T, st)) return 1;
    ++evals;
    if (pass(1, 1, 3, 2, pm, d_ones, false)) return 1;  // norm((f1 - f0) / scale)
    if (read_norms(false)) return 1;
    for (int b = 0; b < B; ++b) {
      ++u[b].nfev;
      u[b].initial_step(plan, d1[b], pin[2 * b], h0[b]);
    }
  } else {
    if (pass(0, 0, 0, 0, nullptr, nullptr)) return 1;  // K0 = f0
    for (int b = 0; b < B; ++b) u[b].h_abs = plan.first_step;
  }

  for (;;) {  // one step attempt of every utterance that still integrates
    int n_active = 0;
    for (int b = 0; b < B; ++b) {
      OdeCtl& c = u[b];
      act[b] = c.begin_attempt(plan) ? 1 : 0;
      if (!act[b]) continue;
      hv[b] = c.h;
      for (int s = 1; s <= ns; ++s) ttv[(size_t)s * B + b] = (float)c.stage_time(plan, s);
      ++n_active;
    }
    if (!n_active) break;
    if (upload()) return 1;
    // rk_step: stage s input fp32(y + dot(K[:s].T, A[s,:s]) h) at t + C[s] h; y_new; f_new = f(t + h, y_new)
    if (pass(-1, 0, 1, 1, plan.A + 1 * DS_ODE_MAX_K, d_h)) return 1;
    for (int s = 1; s <= ns; ++s) {
      if (run_nfe(e, B, T, st)) return 1;
      ++evals;
      if (s < ns - 1) {
        if (pass(s, s, 1, s + 1, plan.A + (s + 1) * DS_ODE_MAX_K, d_h)) return 1;
      } else if (s == ns - 1) {
        if (pass(s, s, 2, ns, plan.B, d_h)) return 1;
      } else {
        if (pass(s, s, 3, ns + 1, plan.E, d_h)) return 1;
      }
    }
    if (read_norms(true)) return 1;
    for (int b = 0; b < B; ++b)
      if (act[b]) u[b].end_attempt(plan, pin[2 * b]);  // (y <- y_new, f <- f_new: taken on the device)
  }

  if (ode_finish(e, sp, oc->eps, oc->denoise, oc->N, smix, w.y, out, B, S, T, sb.tail_lens, st)) return 1;
  if (infos)
    for (int b = 0; b < B; ++b) ode_info(u[b], &infos[b]);
  if (evals_run) *evals_run = evals;
  return 0;
}

// ------------------------------------------------------------------ ... on a fixed grid, enqueued like the PC sampler
// The plan (ode_host.h: OdeFixedPlan) knows every evaluation time, step size and coefficient before the first evaluation, so
// this entry uploads its tables once and walks the pass list: one network evaluation (on e, or on the tail engine for the
// steps ext names) + one per-utterance pass each, steps committed by pointer swap.  Nothing is read back and nothing waits.
extern "C" int32_t diffsep_ode_sample_fixed(diffsep_engine* e, const diffsep_sde_config* sde, int32_t method, int32_t steps,
                                            double t_start, double eps, int32_t denoise, int32_t N,
                                            const diffsep_sampler_ext* ext, const float* mix_norm, const float* x_init,
                                            const float* noise, uint64_t seed, const double* timesteps_host, float* out,
                                            double* err_out, int32_t B, int64_t T, int32_t* nfe_out, void* stream) {
  DS_CHECK(e && sde && mix_norm && out, "ode_sample_fixed: null argument");
  if (check_sde(e, sde, "ode_sample_fixed")) return 1;
  DS_CHECK(B >= 1 && B <= 65535 && T >= 1 && T <= 0x7fffffffLL, "ode_sample_fixed: bad batch shape");
  DS_CHECK(!(x_init && noise), "ode_sample_fixed: x_init and noise are alternatives");
  const OdeFixedConfig fc{method, steps, t_start, eps, denoise, N};
  OdeFixedPlan plan;
  const std::string bad = ode_fixed_plan_fill(plan, fc, timesteps_host, err_out != nullptr, "ode_sample_fixed");
  DS_CHECK(bad.empty(), bad);
  DS_CHECK(plan.t[0] >= 1.0 || x_init, "ode_sample_fixed: a grid that starts below 1 needs the state to start from (x_init == NULL)");
  const int M = plan.M, n_evals = plan.n_evals;
  const int64_t* lengths = ext ? ext->lengths_host : nullptr;
  const uint64_t* seeds = ext ? ext->seeds_host : nullptr;
  diffsep_engine* tail = ScoreEval::other(ext);
  if (check_batch_ext(&e->cfg, "ode_sample_fixed", B, T, lengths, seeds, noise, e, tail)) return 1;

  StreamScope sc_(e, stream);
  hipStream_t st = sc_.st;
  const int S = e->cfg.num_sources;
  if (ensure_plan(e, B, T, st)) return 1;
  if (tail && ensure_plan(tail, B, T, st)) return 1;
  const size_t nst = (size_t)B * S * T;
  // device tables of the whole solve: h [M][B] (fp64) | evaluation times [n_evals + 1][B] (fp32) | active [B] (int)
  const size_t off_tt = (size_t)M * B * 8, off_act = off_tt + (size_t)(n_evals + 1) * B * 4;
  const size_t tab_bytes = off_act + (size_t)B * 4;
  OdeWork w;
  if (ode_workspace(e, nst, err_out ? B : 0, tab_bytes, w)) return 1;
  const double* d_h = (const double*)w.tab;
  const float* d_tt = (const float*)(w.tab + off_tt);
  const int* d_act = (const int*)(w.tab + off_act);
  const SdeP sp = to_sdep(sde);
  {
    char* tp;
    if (e->ode_tab_pin.acquire(tab_bytes, &tp)) return 1;
    double* ph = reinterpret_cast<double*>(tp);
    float* pt = reinterpret_cast<float*>(tp + off_tt);
    int* pa = reinterpret_cast<int*>(tp + off_act);
    for (int i = 0; i < M; ++i)
      for (int b = 0; b < B; ++b) ph[(size_t)i * B + b] = plan.t[i + 1] - plan.t[i];
    for (int r = 0; r <= n_evals; ++r)
      for (int b = 0; b < B; ++b) pt[(size_t)r * B + b] = (float)(r < n_evals ? plan.pass[r].t_eval : plan.t[M]);
    for (int b = 0; b < B; ++b) pa[b] = 1;
    DS_HIP(hipMemcpyAsync(w.tab, tp, tab_bytes, hipMemcpyHostToDevice, st));
    if (e->ode_tab_pin.record(st)) return 1;
  }

  // mixture, lengths and seeds -> device; the start state -> st_x with a zero tail (and y in fp64)
  // (always uploaded; the prior draw keyed as the PC sampler keys it, the prior sample cut only to lengths that are given)
  SamplerBatch sb;
  if (batch_mixture(e, sb, mix_norm, B, T, lengths, seeds, seed, true, st)) return 1;
  if (batch_start(e, sde, sb, B, T, x_init, noise, seeds || lengths, seed, sb.tail_lens, st)) return 1;
  const int *lens = sb.lens, *tail_lens = sb.tail_lens;
  const float* smix = sb.smix;
  if (ds_launch_ode_cast(e->st_x, w.y, (long)nst, st)) return 1;

  OdeArgs base;
  memset(&base, 0, sizeof(base));
  base.s = sp; base.x = e->st_x; base.smix = smix;
  base.rtol = 0.0; base.atol = 1.0; base.part = w.part; base.B = B; base.S = S; base.T = T;
  base.kidx = -1;
  ScoreEval ev(e, tail, ext, M, B, T, nst, st);  // every stage of solver step i of M counts as step i

  DS_HIP(hipMemcpyAsync(e->st_t, d_tt, (size_t)B * 4, hipMemcpyDeviceToDevice, st));
  for (int r = 0; r < n_evals; ++r) {
    const OdeFixedPass& p = plan.pass[r];
    if (ev.eval(p.step)) return 1;
    OdeEachArgs a;
    a.a = ode_pass_args(e, base, w, p.kout, p.mode, p.nk, p.c);
    a.a.score = ev.score;
    a.a.tt = d_tt + (size_t)r * B;
    a.h = d_h + (size_t)p.step * B; a.active = d_act; a.lens = lens;
    a.tnext = d_tt + (size_t)(r + 1) * B;
    if (prof_launch(e, st, ode_pass_rec("ode_stage_each (fused drift + RK stage)", nst, p.nk, p.mode, B, T, S),
                    [&]() { return ds_launch_ode_stage_each(a, st); }))
      return 1;
    if (p.mode != 2) continue;
    if (err_out && p.err_nk > 0) {  // ||step - Euler step||_rms and ||y_i||_rms of every utterance -> slot [step][b]
      OdeEachArgs q;
      q.a = ode_pass_args(e, base, w, -1, 3, p.err_nk, p.d, false);
      q.h = a.h; q.active = d_act; q.lens = lens; q.tnext = nullptr;
      if (prof_launch(e, st, ode_pass_rec("ode_stage_each (local error of a fixed step)", nst, p.err_nk, 3, B, T, S),
                      [&]() { return ds_launch_ode_stage_each(q, st); }))
        return 1;
      if (ds_launch_ode_norm_final_each(w.part, lens, d_act, B, S, err_out + (size_t)p.step * B * 2, st)) return 1;
    }
    std::swap(w.y, w.ynew);  // y <- y_new
    if (p.swap_k01) std::swap(w.K[0], w.K[1]);
  }

  if (ode_finish(e, sp, eps, denoise, N, smix, w.y, out, B, S, T, tail_lens, st)) return 1;
  if (nfe_out) *nfe_out = n_evals;
  return 0;
}

// ------------------------------------------------------------------ ... by exponential integrators (DDIM, DPM-Solver++ 2M)
// The plan (ode_host.h: OdeExpintPlan) holds the grid and the per-step coefficient rows; the driver follows the fixed-step one
// above: one upload of the time table, then per solver step one network evaluation (on e, or on the tail engine) and ONE pass
// (ode.hip, ode_expint_each_kernel) that forms the data prediction and takes the step.  The two X0 histories are fp64 views of
// the stage-derivative buffers K[0..1] and K[2..3], swapped by pointer like y and y_new.  Nothing is read back.
extern "C" int32_t diffsep_ode_sample_expint(diffsep_engine* e, const diffsep_sde_config* sde, int32_t method, int32_t steps,
                                             double t_start, double eps, int32_t denoise, int32_t N,
                                             const diffsep_sampler_ext* ext, const float* mix_norm, const float* x_init,
                                             const float* noise, uint64_t seed, const double* timesteps_host, float* out,
                                             double* err_out, int32_t B, int64_t T, int32_t* nfe_out, void* stream) {
  DS_CHECK(e && sde && mix_norm && out, "ode_sample_expint: null argument");
  if (check_sde(e, sde, "ode_sample_expint")) return 1;
  DS_CHECK(B >= 1 && B <= 65535 && T >= 1 && T <= 0x7fffffffLL, "ode_sample_expint: bad batch shape");
  DS_CHECK(!(x_init && noise), "ode_sample_expint: x_init and noise are alternatives");
  const OdeFixedConfig xc{method, steps, t_start, eps, denoise, N};
  OdeExpintPlan plan;
  const std::string bad = ode_expint_plan_fill(plan, xc, *sde, timesteps_host, err_out != nullptr, "ode_sample_expint");
  DS_CHECK(bad.empty(), bad);
  DS_CHECK(plan.t[0] >= 1.0 || x_init, "ode_sample_expint: a grid that starts below 1 needs the state to start from (x_init == NULL)");
  const int M = plan.M;
  const int64_t* lengths = ext ? ext->lengths_host : nullptr;
  const uint64_t* seeds = ext ? ext->seeds_host : nullptr;
  diffsep_engine* tail = ScoreEval::other(ext);
  if (check_batch_ext(&e->cfg, "ode_sample_expint", B, T, lengths, seeds, noise, e, tail)) return 1;

  StreamScope sc_(e, stream);
  hipStream_t st = sc_.st;
  const int S = e->cfg.num_sources;
  if (ensure_plan(e, B, T, st)) return 1;
  if (tail && ensure_plan(tail, B, T, st)) return 1;
  const size_t nst = (size_t)B * S * T;
  // device tables of the whole solve: evaluation times [M + 1][B] (fp32) | active [B] (int)
  const size_t off_act = (size_t)(M + 1) * B * 4;
  const size_t tab_bytes = off_act + (size_t)B * 4;
  OdeWork w;
  if (ode_workspace(e, nst, err_out ? B : 0, tab_bytes, w)) return 1;
  static_assert(DS_ODE_MAX_K >= 4, "the X0 histories take K[0..1] and K[2..3]");
  double* x0_new = reinterpret_cast<double*>(w.K[0]);   // (K[j + 1] - K[j] >= 4 nst bytes, 256-byte aligned: ode_workspace)
  double* x0_prev = reinterpret_cast<double*>(w.K[2]);
  const float* d_tt = (const float*)w.tab;
  const int* d_act = (const int*)(w.tab + off_act);
  const SdeP sp = to_sdep(sde);
  {
    char* tp;
    if (e->ode_tab_pin.acquire(tab_bytes, &tp)) return 1;
    float* pt = reinterpret_cast<float*>(tp);
    int* pa = reinterpret_cast<int*>(tp + off_act);
    for (int i = 0; i <= M; ++i)
      for (int b = 0; b < B; ++b) pt[(size_t)i * B + b] = (float)plan.t[i];
    for (int b = 0; b < B; ++b) pa[b] = 1;
    DS_HIP(hipMemcpyAsync(w.tab, tp, tab_bytes, hipMemcpyHostToDevice, st));
    if (e->ode_tab_pin.record(st)) return 1;
  }

  // mixture, lengths and seeds -> device; the start state -> st_x with a zero tail (and y in fp64)
  // (always uploaded; the prior draw keyed as the PC sampler keys it, the prior sample cut only to lengths that are given)
  SamplerBatch sb;
  if (batch_mixture(e, sb, mix_norm, B, T, lengths, seeds, seed, true, st)) return 1;
  if (batch_start(e, sde, sb, B, T, x_init, noise, seeds || lengths, seed, sb.tail_lens, st)) return 1;
  const int *lens = sb.lens, *tail_lens = sb.tail_lens;
  const float* smix = sb.smix;
  if (ds_launch_ode_cast(e->st_x, w.y, (long)nst, st)) return 1;

  ScoreEval ev(e, tail, ext, M, B, T, nst, st);

  DS_HIP(hipMemcpyAsync(e->st_t, d_tt, (size_t)B * 4, hipMemcpyDeviceToDevice, st));
  for (int i = 0; i < M; ++i) {
    if (ev.eval(i)) return 1;
    ExpintArgs a;
    memset(&a, 0, sizeof(a));
    a.y = w.y; a.score = ev.score; a.smix = smix;
    a.x0p = (method == DIFFSEP_EXPINT_DPMPP2M && i >= 1) ? x0_prev : nullptr;
    a.x0o = x0_new; a.yo = w.ynew; a.xo = e->st_x;
    ds_expint_set_coef(a, plan.coef.data() + (size_t)i * DS_EXPINT_COEFS);
    a.part = err_out ? w.part : nullptr;
    a.tnext = d_tt + (size_t)(i + 1) * B; a.t_next_out = e->st_t; a.active = d_act; a.lens = lens;
    a.B = B; a.S = S; a.T = T;
    if (prof_launch(e, st, hbm_rec("ode_expint_each (data prediction + exponential-integrator step)", 40.0 * nst, B, 1, (int)T, S),
                    [&]() { return ds_launch_ode_expint_each(a, st); }))
      return 1;
    if (err_out && ds_launch_ode_norm_final_each(w.part, lens, d_act, B, S, err_out + (size_t)i * B * 2, st)) return 1;
    std::swap(w.y, w.ynew);        // y <- y'
    std::swap(x0_new, x0_prev);    // the X0 just written is the next step's previous one
  }

  if (ode_finish(e, sp, eps, denoise, N, smix, w.y, out, B, S, T, tail_lens, st)) return 1;
  if (nfe_out) *nfe_out = M;
  return 0;
}
