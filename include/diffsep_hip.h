/*
 * diffsep_hip.h — C-ABI of the MI355X-native reverse-diffusion separation engine.
 *
 * This is the drop-in boundary for the ONE hot path of fakufaku/diffusion-separation:
 *   separate.py / evaluate.py -> DiffSepModel.get_pc_sampler -> sdes.get_pc_sampler
 *   -> {ald2 corrector, reverse_diffusion predictor} -> ScoreModelNCSNpp (STFT -> NCSN++ -> iSTFT).
 * The reference has no C-ABI/FFI of its own on this path: its plug points are
 * Python call signatures.  Each entry point below cites the reference interface it replaces
 * (paths relative to the reference repository root).
 *
 * Conventions
 *   - plain C types, raw DEVICE pointers (e.g. torch.Tensor.data_ptr()), sizes as int / int64_t;
 *   - every function returns 0 on success, non-zero on failure; diffsep_last_error() returns a
 *     thread-local message; no C++ exception crosses this boundary;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); all work is
 *     asynchronous on it, the caller synchronises;
 *   - waveforms are float32 [B, S, T] / [B, 1, T] contiguous, exactly as the reference passes them;
 *   - image-like activations at the unit-op level are NHWC ("pixel-major") with an explicit pixel
 *     stride `ld` (elements): element (b,h,w,c) lives at ((b*H + h)*W + w)*ld + c.  dtype is
 *     DIFFSEP_F32 or DIFFSEP_BF16 (16-bit storage), C and ld multiples of 8;
 *   - the library is built twice from the same sources and exports this same interface both times:
 *     libdiffsep_hip.so stores the 16-bit tensors (code DIFFSEP_BF16) as raw bfloat16 bits,
 *     libdiffsep_hip_f16.so (-DDS_HALF_F16) as IEEE half precision: the same kernels and speed with 11
 *     instead of 8 significand bits (one score evaluation 2.4e-3 instead of 2.5e-2 from fp32).
 *     diffsep_version() names the build.  Handles and 16-bit buffers of one build mean nothing to the other;
 *   - an engine handle is bound to the device that was current at creation, owns the repacked
 *     weights + workspace, and is not thread-safe (the reference is one Python thread per process
 *     per GPU: evaluate_mp.py:339,510-513).  The parameter-table queries (diffsep_param_count / _info /
 *     _total) share ONE process-wide cache of the last architecture asked about: call them from one
 *     thread at a time.
 */
#ifndef DIFFSEP_HIP_H
#define DIFFSEP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DIFFSEP_F32 0
#define DIFFSEP_BF16 1
/* fp32 tensors and fp32 everywhere except the matrix products: every MFMA k-block runs as three bf16 MFMAs on the
 * hi / lo bf16 halves of both operands (hi*hi + hi*lo + lo*hi, fp32 accumulation: products good to ~2^-17 instead of
 * 2^-24), ~2x the speed of DIFFSEP_F32.  Accepted by diffsep_engine_create and by the unit convolution / attention
 * entry points; tensors are fp32 exactly as for DIFFSEP_F32. */
#define DIFFSEP_F32_SPLIT 2
#define DIFFSEP_F64 4 /* float64 rows: an output type of diffsep_resample only (3 is the Python binding's name for the half build) */

#define DIFFSEP_SDE_MIX 0      /* sdes/sdes.py:180-349  MixSDE      */
#define DIFFSEP_SDE_PRIORMIX 1 /* sdes/sdes.py:352-590  PriorMixSDE */

#define DIFFSEP_PRED_REVERSE_DIFFUSION 0 /* sdes/predictors.py:55-66 */
#define DIFFSEP_PRED_EULER_MARUYAMA 1    /* sdes/predictors.py:39-52 */
#define DIFFSEP_PRED_NONE 2              /* sdes/predictors.py:69-77 */

#define DIFFSEP_CORR_ALD2 0     /* sdes/correctors.py:94-128  */
#define DIFFSEP_CORR_NONE 1     /* sdes/correctors.py:131-141 */
#define DIFFSEP_CORR_ALD 2      /* sdes/correctors.py:58-91 (MixSDE only) */
#define DIFFSEP_CORR_LANGEVIN 3 /* sdes/correctors.py:35-55 (one step size for the whole batch) */

#define DIFFSEP_ODE_RK45 0 /* scipy.integrate.RK45 (Dormand-Prince 5(4)), the reference's default (sdes/__init__.py:193-278) */
#define DIFFSEP_ODE_RK23 1 /* scipy.integrate.RK23 (Bogacki-Shampine 3(2)) */
#define DIFFSEP_ODE_WORKSPACE_BYTES 16384 /* workspace of the error-norm unit entry: per-block fp64 partial sums */

typedef struct diffsep_engine diffsep_engine; /* opaque */
typedef struct diffsep_resampler diffsep_resampler; /* opaque (sample-rate conversion, below) */

/* Hyper-parameters of ScoreModelNCSNpp + its NCSNpp backbone.
 * Replaces: models/score_models.py:11-39 (ctor kwargs), models/ncsnpp.py:45-70 (ctor defaults),
 * config/model/default.yaml:14-31. */
typedef struct {
  int32_t nf;               /* backbone_args.nf (64 default.yaml:25; 128 icassp-separation.yaml:16) */
  int32_t num_sources;      /* S; backbone in = 2S+2, out = 2S (score_models.py:24-26) */
  int32_t n_levels;         /* len(ch_mult) = 7 */
  int32_t ch_mult[8];       /* (1,1,2,2,2,2,2) */
  int32_t num_res_blocks;   /* 2 */
  int32_t attn_resolution;  /* 16 (tested against the frequency axis, ncsnpp.py:367,415) */
  int32_t n_fft;            /* 510 -> image height n_fft/2+1 = 256 */
  int32_t hop;              /* 128 */
  float spec_abs_exponent;  /* 0.5 */
  float spec_factor;        /* 0.33 (0.15 published) */
  int32_t dtype;            /* DIFFSEP_F32 (exact), DIFFSEP_F32_SPLIT (parity-grade, 2x faster) or DIFFSEP_BF16 (16-bit storage: throughput) */
} diffsep_model_config;

/* sdes/sdes.py:217-240 (MixSDE ctor), :397-450 (PriorMixSDE ctor). */
typedef struct {
  int32_t kind; /* DIFFSEP_SDE_* */
  int32_t ndim; /* number of sources */
  float d_lambda, sigma_min, sigma_max;
  int32_t avg_len; /* PriorMixSDE only: length of the mix^2 moving average (510, sdes.py:383) */
} diffsep_sde_config;

/* sdes/__init__.py:132-145 (get_pc_sampler kwargs) + pl_model.py:687-701. */
typedef struct {
  int32_t N;               /* reverse steps */
  int32_t corrector_steps; /* n_steps of the corrector */
  float snr;               /* corrector step size */
  float eps;               /* t_eps: last time step */
  int32_t denoise;         /* return x_mean of the last predictor step */
  int32_t predictor;       /* DIFFSEP_PRED_* */
  int32_t corrector;       /* DIFFSEP_CORR_* */
} diffsep_sampler_config;

const char* diffsep_last_error(void);
const char* diffsep_version(void);

/* ---- parameter table: the canonical weight order is the reference state_dict order of
 * ScoreModelNCSNpp.backbone (models/ncsnpp.py:106-308: all_modules.{i}.*, then output_layer.*,
 * see SURVEY.md Appendix A).  The host assembles one flat float32 blob in this order. ---- */
int32_t diffsep_param_count(const diffsep_model_config* cfg);
/* name: e.g. "all_modules.4.Conv_0.weight"; shape: up to 4 dims (reference layout, e.g. OIHW);
 * offset: position (in floats) inside the flat blob. */
int32_t diffsep_param_info(const diffsep_model_config* cfg, int32_t idx, char* name, int32_t name_cap,
                           int64_t shape[4], int32_t* ndim, int64_t* offset);
int64_t diffsep_param_total(const diffsep_model_config* cfg);

/* Create from HOST weights (EMA already applied by the caller: pl_model.py:655-660).
 * Replaces DiffSepModel.__init__/load_from_checkpoint + .to(device) (separate.py:44-48). */
int32_t diffsep_engine_create(const diffsep_model_config* cfg, const float* weights_host, int64_t n_floats,
                              diffsep_engine** out);
void diffsep_engine_destroy(diffsep_engine* e);
/* bytes of device memory currently held (weights + workspace). */
int64_t diffsep_engine_device_bytes(const diffsep_engine* e);
/* Size the workspace for batches of up to B utterances of T samples now (the engine otherwise grows it on demand, and
 * hipFree / hipMalloc synchronise the whole device — i.e. every other stream).  Host-side counterpart in the
 * reference: none (torch's caching allocator). */
int32_t diffsep_engine_reserve(diffsep_engine* e, int32_t B, int64_t T, void* stream);
/* Debug aid: the engine's workspace arena (sampler state, then one forward's activations in launch order from
 * fwd_base).  Lets a test snapshot every intermediate tensor of a forward; no reference counterpart. */
int32_t diffsep_engine_debug_arena(const diffsep_engine* e, void** base, int64_t* bytes, int64_t* fwd_base);
/* Debug / test aid (engine option "track_tensors" = 1, eager forwards: diffsep_score_forward): for every activation tensor of the
 * last forward, in allocation order, out[4 i ..] = {largest finite |value|, number of non-finite values, rows H, channels C};
 * *n = number of tensors (out may be NULL to query).  How far the half-precision engines are from 65504. */
int32_t diffsep_engine_debug_absmax(diffsep_engine* e, double* out, int32_t cap, int32_t* n);
/* Debug / test aid (engine option "trace" = 1, eager forwards: diffsep_score_forward, diffsep_backbone_forward): one record per
 * tensor or side array the last forward WROTE, in launch order, of the query-then-fill form of diffsep_engine_debug_absmax
 * (fields / names may be NULL to query *n; at most cap records are written).
 * fields[DIFFSEP_TRACE_FIELDS i ..] = {mod, B, H, W, C, ld, f32, offset, stats}: mod = index of the module in the all_modules
 * order, -1 outside it; the tensor is [B][H][W][C] with leading dimension ld, fp32 when f32 != 0 and of the engine's storage type
 * otherwise; offset = its byte offset in the arena of diffsep_engine_debug_arena (-1: the caller's own buffer); stats = byte offset
 * in the arena of its [B][C][2] int64 GroupNorm accumulators (they live in the statistics region at the start of the forward's
 * allocations), or -1.
 * names[DIFFSEP_TRACE_NAME_BYTES i ..] = three NUL-terminated strings at +0, +16 and +32: kind = the step that wrote it ("stft",
 * "fourier", "linear", "conv", "gn_apply", "gn_finalize", "gn_stats", "gemm", "softmax", "attn_fused"); role = what the tensor is
 * to its block ("x0", "emb", "t1", "temb", "proj", "conv_in", "h0m", "xr", "h1p", "h1", "skip", "outp", "out", "scale", "shift",
 * "h", "q", "k", "vt", "scores", "probs", "o", "pd", "combine", "pu", "pnew", "y"); kernel = what diffsep_last_conv_kernel()
 * reported after a convolution or fused-attention launch ("" otherwise).
 * Inputs are not recorded: which tensors a step should have read is the checker's business (tests/netcheck.py).  Off by default;
 * with the option off a forward launches exactly what it launches without this entry. */
#define DIFFSEP_TRACE_FIELDS 9
#define DIFFSEP_TRACE_NAME_BYTES 160
int32_t diffsep_engine_debug_trace(const diffsep_engine* e, int64_t* fields, char* names, int32_t cap, int32_t* n);
/* frames F = 1 + (T + n_fft - hop)/hop and padded width W = 64*ceil(F/64) for T samples
 * (score_models.py:83-91,107-112). Pure host arithmetic. */
int32_t diffsep_num_frames(const diffsep_model_config* cfg, int64_t T);
int32_t diffsep_padded_frames(const diffsep_model_config* cfg, int64_t T);

/* score_fn(x, t, mix): DiffSepModel.forward (pl_model.py:407-409) -> ScoreModelNCSNpp.forward
 * (models/score_models.py:126-138).  xt [B,S,T], t [B], mix [B,1,T], out [B,S,T]; all device f32. */
int32_t diffsep_score_forward(diffsep_engine* e, const float* xt, const float* t, const float* mix, float* out,
                              int32_t B, int64_t T, void* stream);

/* backbone only: NCSNpp.forward (models/ncsnpp.py:319-478) on an already-packed NHWC input
 * x [B,256,W,Cpad] (dtype of the engine, BEFORE the 2x-1 of ncsnpp.py:347-349), t [B] f32;
 * y [B,256,W,Cpad_out].  Used by parity tests to isolate the network from the STFT front end. */
int32_t diffsep_backbone_forward(diffsep_engine* e, const void* x, const float* t, void* y, int32_t B, int32_t W,
                                 void* stream);

/* The whole sampler: sdes.get_pc_sampler(...)() (sdes/__init__.py:132-190) as called from
 * DiffSepModel.get_pc_sampler (pl_model.py:687-711) with score_fn = the engine.
 *   mix_norm [B,1,T] : output of normalize_batch (pl_model.py:81-88);
 *   out      [B,S,T] : x_mean of the last predictor step if denoise else x (sdes/__init__.py:183);
 *   noise            : NULL -> on-device Philox N(0,1) draws keyed by `seed`; otherwise
 *                      [1 + N*(corrector_steps+1)][B][S][T] float32 draws consumed in the
 *                      reference's RNG order: prior, then per step corrector
 *                      draw(s), predictor draw;
 *   timesteps        : NULL -> torch.linspace(T=1, eps, N) semantics (sdes/__init__.py:175);
 *                      otherwise N+1 HOST floats for the scheduled sampler
 *                      (sdes/__init__.py:91-111; dt is still 1/N — reference quirk Q1);
 *   nfe_out          : N*(corrector_steps+1) (sdes/__init__.py:184), may be NULL. */
int32_t diffsep_pc_sample(diffsep_engine* e, const diffsep_sde_config* sde, const diffsep_sampler_config* smp,
                          const float* mix_norm, float* out, int32_t B, int64_t T, const float* noise,
                          uint64_t seed, const float* timesteps_host, int32_t* nfe_out, void* stream);

/* Extensions of the sampler call that have no counterpart in the reference (which runs one utterance at a time in
 * one precision: evaluate.py:348-376).  All fields optional (zero / NULL = diffsep_pc_sample behaviour).
 *   lengths_host [B]  : utterance b has lengths_host[b] <= T samples; the batch is zero-padded to T and every
 *                       utterance must have the padded frame count of T (diffsep_padded_frames).  Samples beyond an
 *                       utterance's length stay exactly zero through the whole sampler, so each utterance comes out
 *                       bit-for-bit as a B = 1 call on it alone with the same seed (fp32 engine; within the
 *                       GroupNorm-sum rounding of the weight-stationary bf16 kernel otherwise).  The 'langevin'
 *                       corrector couples the batch entries and is refused with lengths.
 *   seeds_host [B]    : per-utterance Philox seeds (with noise == NULL): utterance b draws exactly what a B = 1 call
 *                       with seed = seeds_host[b] draws, whatever batch it rides in.  Without it `seed` keys the
 *                       whole batch as in diffsep_pc_sample (with lengths: utterance b uses seed + b * 0x9E3779B97F4A7C15).
 *   tail_engine       : a second engine of the same architecture and weights (an fp32 or split-fp32 engine behind a bf16 one) that
 *                       evaluates the score of the FIRST head_steps and / or the LAST tail_steps reverse steps (their
 *                       corrector and predictor evaluations).  A score error enters the state scaled by the step size
 *                       G(t)^2, ~100x larger at t = 1 than at t = eps: it is the early steps whose precision decides
 *                       how closely the bf16 sampler follows the fp32 one (tools/hybrid_probe.py). */
typedef struct {
  const int64_t* lengths_host;
  const uint64_t* seeds_host;
  diffsep_engine* tail_engine;
  int32_t tail_steps;
  int32_t head_steps;
} diffsep_sampler_ext;
int32_t diffsep_pc_sample_ex(diffsep_engine* e, const diffsep_sde_config* sde, const diffsep_sampler_config* smp,
                             const diffsep_sampler_ext* ext, const float* mix_norm, float* out, int32_t B, int64_t T,
                             const float* noise, uint64_t seed, const float* timesteps_host, int32_t* nfe_out,
                             void* stream);

/* diffsep_pc_sample_ex with a tap on the intermediate states of the reverse diffusion: what the reference's sampler returns
 * with intermediate=True (sdes/__init__.py:168-186: `(xt, xt_mean)` appended after the corrector and before the predictor of
 * every step) and what evaluate.py:29-61 draws its `fig/<split>/evo_NNN.pdf` from.  In reverse step i, at that same place, one
 * launch of one 1024-thread block per utterance makes one pass over the state:
 *   snap_steps_host [n_snap] : HOST, the steps to copy, strictly ascending, each in [0, N);
 *   snap_x, snap_xm          : [n_snap][B][S][T] device f32: x (and x_mean; snap_xm may be NULL) of those steps.  Without a
 *                              corrector step (corrector none, or corrector_steps 0) x_mean is x, as in the reference's loop;
 *   target                   : [B][S][T] device f32, or NULL.  It must be ZERO beyond each utterance's length (the state's tail
 *                              is, so that the tails add nothing to the sums);
 *   gram                     : [N+1][B][3][S][S] device float64, given with target or not at all.  Row i < N is bit for bit
 *                              diffsep_gram(target, x of step i) (the same per-thread stride and reduction order), row N is
 *                              diffsep_gram(target, out): the SI-SDR / SI-SIR / SI-SAR of every step follow on the host.
 * The state lives on `e` whichever engine evaluates a step (ext->tail_engine), and `out` is bit for bit that of the untraced
 * call.  Refused with an error text before anything is enqueued: steps unordered, repeated or out of range; n_snap > 0 with
 * snap_x NULL; exactly one of target / gram.  With n_snap == 0 and target == NULL this IS diffsep_pc_sample_ex: not one
 * launch, copy or allocation more. */
int32_t diffsep_pc_sample_trace(diffsep_engine* e, const diffsep_sde_config* sde, const diffsep_sampler_config* smp,
                                const diffsep_sampler_ext* ext, const float* mix_norm, float* out, int32_t B, int64_t T,
                                const float* noise, uint64_t seed, const float* timesteps_host, int32_t* nfe_out,
                                int32_t n_snap, const int32_t* snap_steps_host, float* snap_x, float* snap_xm,
                                const float* target, double* gram, void* stream);

/* diffsep_pc_sample_trace with both ends of the sampler open: a state to start from instead of the prior sample, and a range
 * of the N reverse steps.  The reference starts only at t = T from prior_sampling (sdes/__init__.py:166-188); what it offers
 * for an intermediate start is SDE.marginal_prob (sdes/sdes.py:322-324, PriorMixSDE :515-532), as its training uses it in
 * sample_prior (pl_model.py:179-247): diffsep_warm_start below builds x_init from it.  This is the most general sampler entry;
 * the three above forward to it with x_init = NULL, first_step = 0, last_step = 0 and enqueue exactly what they always did.
 * All steps are ABSOLUTE indices of the N-point grid:
 *   last_step == 0 means N; the steps i in [first_step, last_step) run, step i at time ts[i] of the same grid (linspace(1, eps, N)
 *   or timesteps_host) with dt = 1/N (quirk Q1) and with the draws 1 + i (c + p) ... 1 + (i + 1)(c + p) - 1 of `noise` / of the
 *   device RNG (c = corrector steps, 0 for corrector none; p = 1 unless predictor none; draw 0 is the prior's), so that a run
 *   over [0, k) followed by a run over [k, N) from its result is bit for bit the run over [0, N);
 *   ext->head_steps / tail_steps keep meaning absolute steps: a range that holds none of them never touches ext->tail_engine;
 *   x_init [B,S,T] device f32, or NULL: copied into the state in place of the prior sample (draw 0 is then not generated; with
 *   ext->lengths_host its tail is zeroed like the mixture's).  first_step > 0 needs it;
 *   out: with last_step < N the state x itself, whatever smp->denoise says (it can be resumed from); with last_step == N as above;
 *   nfe_out = (last_step - first_step) (corrector steps + 1);
 *   snap_steps_host must lie in [first_step, last_step); of gram [N+1][B][3][S][S] the rows first_step .. last_step - 1 are
 *   written, and row N only when last_step == N; every other row is left as it was.
 * Refused with an error text before anything is enqueued, `out` untouched: a range outside 0 <= first_step < last_step <= N,
 * first_step > 0 with x_init == NULL, a snapshot step outside the range, and everything diffsep_pc_sample_trace refuses. */
int32_t diffsep_pc_sample_from(diffsep_engine* e, const diffsep_sde_config* sde, const diffsep_sampler_config* smp,
                               const diffsep_sampler_ext* ext, const float* mix_norm, float* out, int32_t B, int64_t T,
                               const float* noise, uint64_t seed, const float* timesteps_host, int32_t* nfe_out,
                               int32_t n_snap, const int32_t* snap_steps_host, float* snap_x, float* snap_xm,
                               const float* target, double* gram, const float* x_init, int32_t first_step,
                               int32_t last_step, void* stream);

/* The probability-flow ODE sampler: sdes.get_ode_sampler(...)() (sdes/__init__.py:193-278), i.e.
 * scipy.integrate.solve_ivp(method = RK45 | RK23) on dx/dt = f(x,t) - 0.5 G(t)^2 score(x,t,mix) (RSDE.sde with
 * probability_flow, sdes/sdes.py:130-160) from t = 1 down to eps, the whole batch [B,S,T] as ONE system (one error
 * norm, one step size), followed by the optional denoise step.  The controller is scipy's (rk.py / common.py, scipy
 * 1.15): select_initial_step, the embedded error norm ||h K^T E / (atol + max(|y|,|y_new|) rtol)||_rms, accept if < 1,
 * factor min(10, 0.9 err^(-1/(p+1))) (at most 1 after a rejection), reject factor max(0.2, 0.9 err^(-1/(p+1))), last
 * step clipped onto eps, stop when the step falls below 10 ulp(t).  State in fp64, stage derivatives in fp32.
 *   mix_norm [B,1,T], out [B,S,T] (device float32);
 *   x_init   : NULL -> x_T = prior sample (noise [B,S,T] given, or on-device Philox draws keyed by `seed`: the draws of
 *              the PC sampler's prior with the same seed); otherwise the caller's x_T [B,S,T] (the reference's `z`);
 *   info     : may be NULL.  nfev is scipy's solution.nfev (the denoise evaluation is not counted).
 * Buffers: y, y_new, 7 K and a partial-sum slab, allocated at the first call (diffsep_engine_device_bytes grows then;
 * the workspace of the PC sampler does not change).  No mixed-length batches (diffsep_ode_sample_each), no tail engine. */
typedef struct {
  double rtol, atol;   /* solve_ivp tolerances (reference default 1e-5 / 1e-5) */
  double eps;          /* t_bound: integrate from 1 down to eps (3e-2) */
  double first_step;   /* <= 0: select_initial_step (one more evaluation) */
  double max_step;     /* <= 0 or inf: unbounded */
  int32_t method;      /* DIFFSEP_ODE_* */
  int32_t max_nfe;     /* 0: unbounded; otherwise no step attempt starts that would take nfev above it (status 1) */
  int32_t denoise;     /* one reverse_diffusion predictor step at eps without noise, its x_mean (dt = 1/N: quirk Q1) */
  int32_t N;           /* sde.N of that denoise step */
} diffsep_ode_config;
typedef struct {
  int32_t nfev;        /* network evaluations of the solver (scipy's nfev) */
  int32_t n_accepted, n_rejected;
  int32_t status;      /* 0 reached eps, -1 step size below 10 ulp(t) (scipy's failure), 1 max_nfe reached */
  double t_final;      /* time of the returned state (before the denoise step) */
} diffsep_ode_info;
int32_t diffsep_ode_sample(diffsep_engine* e, const diffsep_sde_config* sde, const diffsep_ode_config* ode,
                           const float* mix_norm, const float* x_init, const float* noise, uint64_t seed, float* out,
                           int32_t B, int64_t T, diffsep_ode_info* info, void* stream);
/* The same sampler with ONE STEP CONTROLLER PER UTTERANCE (no counterpart in the reference, whose evaluate.py:348-376 runs
 * sdes.get_ode_sampler (sdes/__init__.py:193-278) on one utterance at a time, where "the batch is one system" and "every
 * utterance is its own system" are the same thing).  The batch [B,S,T] is B independent ODE systems solved in lock step:
 * utterance b keeps its own t, h, error norm, accept / reject decisions and counts, exactly as diffsep_ode_sample computes
 * them for it alone, and all utterances share every network evaluation (one step attempt = n_stages evaluations of the whole
 * batch with a per-utterance time).  An utterance that has reached eps (or failed, or hit max_nfe) is frozen: its rows ride
 * through the remaining evaluations, its state is not touched.  Given the same network evaluations, row b of `out` inside
 * its length is bit-for-bit what diffsep_ode_sample returns for that utterance alone (B = 1, T = lengths[b], the same
 * seed), whatever batch, position or padded width it rides in: the norms are summed in the B = 1 order of an utterance of
 * that length.  So it is wherever the fp32 engine's evaluation does not depend on the batch (the reach of
 * diffsep_sampler_ext.lengths_host's guarantee; DESIGN.md section 5b has the measurement); the 16-bit engines are not
 * bit-independent of the batch, so there the decisions may differ too.
 *   ext (may be NULL, both fields optional):
 *     lengths_host [B] : as in diffsep_sampler_ext — within [1, T], all with the padded frame count of T; the mixture's tail
 *                        is masked, the state's tail stays exactly zero and enters no norm (n = S * lengths[b]);
 *     seeds_host [B]   : per-utterance Philox seeds of the prior draw (noise == NULL and x_init == NULL); without it
 *                        utterance b uses seed + b * 0x9E3779B97F4A7C15, as the PC sampler does;
 *   x_init / noise     : as in diffsep_ode_sample, their tails zeroed;
 *   infos [B]          : may be NULL; the counts utterance b would have had alone;
 *   evals_run          : may be NULL; network evaluations of the batch actually run = max_b infos[b].nfev (the denoise
 *                        evaluation is not counted).
 * One pinned readback of 2 B norms per step attempt; the call blocks on it.  Buffers as diffsep_ode_sample, plus one
 * partial-sum slab per utterance and the per-attempt tables. */
typedef struct {
  const int64_t* lengths_host;
  const uint64_t* seeds_host;
} diffsep_ode_ext;
int32_t diffsep_ode_sample_each(diffsep_engine* e, const diffsep_sde_config* sde, const diffsep_ode_config* ode,
                                const diffsep_ode_ext* ext, const float* mix_norm, const float* x_init,
                                const float* noise, uint64_t seed, float* out, int32_t B, int64_t T,
                                diffsep_ode_info* infos, int32_t* evals_run, void* stream);
/* The same ODE on a FIXED GRID with a budget the caller chooses (no counterpart in the reference, whose only ODE solve is the
 * adaptive one above; the right-hand side is the reference's: RSDE.sde with probability_flow, sdes/sdes.py:130-160, as
 * sdes/__init__.py:193-278 hands it to solve_ivp).  No error norm decides anything, so the call enqueues the whole solve on
 * `stream` and returns: no readback, no event wait, no stream synchronisation — like diffsep_pc_sample_from, and with its
 * extensions.  One network evaluation + one fused pass (csrc/ode.hip, the per-utterance form) per stage.
 *   method, steps (M) : DIFFSEP_ODEF_EULER (M evaluations), HEUN and MIDPOINT (2 M), RK4 (4 M: the classic tableau) or AB2
 *                       (M + 1): y_{n+1} = y_n + h_n ((1 + w/2) K_n - (w/2) K_{n-1}), w = h_n / h_{n-1}, after a first Heun step
 *                       whose K_0 is kept;
 *   t_start, eps      : the grid t_i = t_start + (eps - t_start) i / M, i < M, and t_M = eps; t_start <= 0 means 1.0 (sde.T);
 *   timesteps_host    : NULL, or M + 1 HOST float64 times that replace that grid: strictly descending, inside (0, 1].
 *                       h_i = t_{i+1} - t_i exactly (a true integration: the dt = 1/N of quirk Q1 is the denoise step's only);
 *                       stage s of step i is evaluated at (float)(t_i + C[s] h_i), state in fp64, K in fp32, as above;
 *   denoise, N        : as diffsep_ode_config: one reverse_diffusion predictor step at eps without noise, its x_mean;
 *   x_init / noise / seed : the prior as in diffsep_ode_sample — the caller's state, or the prior sample from noise [B,S,T],
 *                       or from draw 0 of the PC sampler's device generator under seed / ext->seeds_host.  A grid that starts
 *                       below 1 needs x_init (diffsep_warm_start builds one at any time);
 *   ext (may be NULL) : lengths_host — B independent zero-padded rows: row b inside its length is bit for bit the call on that
 *                       utterance alone (B = 1, T = lengths[b], same seed) wherever the fp32 network evaluation does not depend
 *                       on the batch, and its tail is zero; seeds_host — per-utterance seeds of the prior draw (unused with
 *                       x_init); tail_engine with head_steps / tail_steps counted in SOLVER STEPS of this grid: every stage
 *                       evaluation of the first head_steps and the last tail_steps steps runs on it (state and time copied
 *                       over, the state lives on e; the denoise evaluation is e's).  A range that holds no such step never
 *                       touches it;
 *   err_out           : NULL, or device float64 [M][B][2] (HEUN, MIDPOINT, AB2): per step i and utterance b the RMS over the
 *                       utterance of (step - embedded Euler step) = h (K1 - K0) / 2, h (K1 - K0), h (w/2)(K_n - K_{n-1}), and the
 *                       RMS of y_i; fixed-order fp64 sums (the error-norm pass with rtol = 0, atol = 1), nothing read back.
 *                       With NULL not one launch, copy or allocation is added and `out` is the same bits;
 *   nfe_out           : the evaluation count above, known before the call (the denoise evaluation is not counted).
 * Refused with an error text before anything is enqueued: an unknown method, steps < 1, steps x stages > 16384, a grid that
 * is not strictly descending inside (0, 1], eps outside (0, 1), t_start <= eps, denoise with N < 1, err_out with EULER or
 * RK4, x_init together with noise, a start below 1 without x_init, seeds with noise, and the length checks of
 * diffsep_pc_sample_from.  Buffers: those of diffsep_ode_sample plus the uploaded tables (evaluation times [M x stages + 1][B],
 * h [M][B], active, lengths: one upload through a pinned stage before the first evaluation) and, with err_out, one partial-sum
 * slab per utterance.
 * (The solve's shape is passed as plain arguments, not as a struct: host code keeps them in OdeFixedConfig, csrc/ode_host.h.) */
#define DIFFSEP_ODEF_EULER 0
#define DIFFSEP_ODEF_HEUN 1
#define DIFFSEP_ODEF_MIDPOINT 2
#define DIFFSEP_ODEF_RK4 3
#define DIFFSEP_ODEF_AB2 4
int32_t diffsep_ode_sample_fixed(diffsep_engine* e, const diffsep_sde_config* sde, int32_t method, int32_t steps,
                                 double t_start, double eps, int32_t denoise, int32_t N, const diffsep_sampler_ext* ext,
                                 const float* mix_norm, const float* x_init, const float* noise, uint64_t seed,
                                 const double* timesteps_host, float* out, double* err_out, int32_t B, int64_t T,
                                 int32_t* nfe_out, void* stream);
/* The same ODE by EXPONENTIAL INTEGRATORS on the same grids: DDIM (first order) and DPM-Solver++ 2M (second-order multistep, step 0
 * a DDIM step), M network evaluations each (no counterpart in the reference; the SDE is the reference's, sdes/sdes.py:180-349).
 * A = 11^T / S and P = I - A commute with the mean matrix A + e^{-lambda t} P and with L(t) = sqrt(ev1) A + sqrt(ev2) P
 * (MixSDE._cov_eigval, sdes/sdes.py:296-309), so the ODE is two scalar diffusions, one per eigenspace j in {A, P}:
 * alpha_A = 1, sigma_A^2 = ev1; alpha_P = e^{-lambda t}, sigma_P^2 = ev2 (times sigma_mix[b,t]^2 for PriorMixSDE).  The linear drift
 * and the noise schedule are integrated in closed form; only the network's data prediction is discretised.  Per step i from t_i
 * to t_{i+1}, float64 on the host from the SDE's float parameters widened as they are, with a_A = 0, a_P = d_lambda:
 *   alpha_j(t) = exp(-a_j t), ev_j(t) as _cov_eigval, lam_j = ln alpha_j - 0.5 ln ev_j, h_j = lam_j(t_{i+1}) - lam_j(t_i),
 *   cx_j = sqrt(ev_j(t_{i+1}) / ev_j(t_i)), cd_j = -alpha_j(t_{i+1}) expm1(-h_j), w0_j = 1, w1_j = 0, and for DPMPP2M at i >= 1
 *   r_j = h_j(i-1) / h_j(i), w0_j = 1 + 1 / (2 r_j), w1_j = -1 / (2 r_j).
 * diffsep_expint_coefficients writes that table (host memory, no GPU needed): coef_out [steps][DIFFSEP_EXPINT_COEFS] =
 *   cx_A cd_A w0_A w1_A | cx_P cd_P w0_P w1_P | alpha_A(t_i) ev_A(t_i) alpha_P(t_i) ev_P(t_i)
 * for the grid diffsep_ode_sample_fixed builds from (steps, t_start, eps) or takes from timesteps_host, with its refusals in its
 * words, and: an SDE kind that is neither MixSDE nor PriorMixSDE, a grid point where ev_1 <= 0, steps > 16384.
 * The pass (csrc/ode.hip, one launch per step, per-utterance form), per time sample, every sum and product rounded on its own in
 * float64 in the order written (sums over the sources run s = 0, 1, ..., then one division by S):
 *   mx = mean_s y_s, ms = mean_s score_s, q = sigma_mix[b,t]^2 (widened, then squared; 1 for MixSDE),
 *   X0_s = (mx + (ev_A q) ms) / alpha_A + ((y_s - mx) + (ev_P q) (score_s - ms)) / alpha_P          (Tweedie at t_i)
 *   mX0n = mean_s X0_s, mX0p = mean_s X0p_s (the previous step's X0; without one both w1 terms are absent)
 *   y'_s = (cx_A mx + cd_A (w0_A mX0n + w1_A mX0p)) + (cx_P (y_s - mx) + cd_P (w0_P (X0_s - mX0n) + w1_P (X0p_s - mX0p)))
 * and the next network input is fp32(y'), evaluated at (float) t_{i+1}.
 * diffsep_ode_sample_expint: the argument list, the grid, x_init / noise / seed, ext (lengths, seeds, tail engine counted in solver
 * steps), denoise, the enqueued call without readback and the refusals of diffsep_ode_sample_fixed; nfe_out = steps.
 *   err_out : NULL, or device float64 [M][B][2] (DPMPP2M only): per step and utterance the RMS of (step - its DDIM step) =
 *             (cd_A (w0_A - 1)) (mX0n - mX0p) + (cd_P (w0_P - 1)) ((X0_s - mX0n) - (X0p_s - mX0p)), an exact 0 at step 0, and the RMS
 *             of y_i; summed in the same launch into fixed-order fp64 partials, one small final launch per step.  With NULL not
 *             one launch, copy or allocation is added and `out` is the same bits.
 * Buffers: those of diffsep_ode_sample_fixed; the two X0 histories live in its stage-derivative buffers.
 * diffsep_expint_update_each: the pass on caller buffers.  y, x0_prev (NULL: no previous X0), x0_out, y_new_out float64 [B,S,T];
 * score, x_out float32 [B,S,T]; sigma_mix [B,T] for PriorMixSDE, else NULL; coef: HOST, one row of the table; active, lengths:
 * DEVICE int32 [B] as in diffsep_ode_stage_update_each (inactive rows untouched, t >= lengths[b] never read and the three outputs
 * written as exact zeros there); norms_out NULL, or device float64 [B][2] with workspace >= B * DIFFSEP_ODE_WORKSPACE_BYTES: the
 * two values of err_out.  No output may alias an input. */
#define DIFFSEP_EXPINT_DDIM 0
#define DIFFSEP_EXPINT_DPMPP2M 1
#define DIFFSEP_EXPINT_COEFS 12
int32_t diffsep_ode_sample_expint(diffsep_engine* e, const diffsep_sde_config* sde, int32_t method, int32_t steps,
                                  double t_start, double eps, int32_t denoise, int32_t N, const diffsep_sampler_ext* ext,
                                  const float* mix_norm, const float* x_init, const float* noise, uint64_t seed,
                                  const double* timesteps_host, float* out, double* err_out, int32_t B, int64_t T,
                                  int32_t* nfe_out, void* stream);
int32_t diffsep_expint_coefficients(const diffsep_sde_config* sde, int32_t method, int32_t steps, double t_start, double eps,
                                    const double* timesteps_host, double* coef_out);
int32_t diffsep_expint_update_each(const diffsep_sde_config* sde, const double* y, const float* score, const float* sigma_mix,
                                   const double* x0_prev, const double* coef, const int32_t* active, const int32_t* lengths,
                                   double* x0_out, double* y_new_out, float* x_out, double* norms_out, int32_t B, int32_t S,
                                   int64_t T, void* workspace, int64_t workspace_bytes, void* stream);
/* Butcher tableau of RK45 / RK23 exactly as scipy's rk.py holds it (sdes/__init__.py:193-278 -> solve_ivp): A [ns][ns]
 * row-major, B [ns], C [ns], E [ns+1]; every pointer may be NULL (host memory, no GPU needed). */
int32_t diffsep_ode_tableau(int32_t method, double* A, double* B, double* C, double* E, int32_t* n_stages,
                            int32_t* error_order);
/* The two passes of the ODE sampler as unit entries (sdes/__init__.py:193-278; the sampler launches them on its own
 * state).  State [B,S,T]: x, score, K[j] float32; y, y_new fp64.  K is a HOST array of n_k (<= 7) device pointers.
 *   k_out >= 0: K[k_out] = f(x,t) - 0.5 G(t)^2 score (t [B] device; sigma_mix [B,T] for PriorMixSDE, else NULL),
 *              computed in the operation order of diffsep_sde_coefficients + diffsep_sde_reverse_drift(probability_flow);
 *   acc = sum_{j < n_k} coef[j] K[j] (fp64, in order j = 0, 1, ...);
 * stage_update: y_new_out == NULL: x_out = fp32(y + acc h) (the next stage input; x_out may be x);
 *               otherwise y_new_out = y + h acc and x_out (may be NULL) = fp32(y_new_out).  n_k = 0: the drift only.
 * error_norm:   norms_out[0] = ||acc h / sc||_rms, norms_out[1] = ||y / sc||_rms (device fp64 [2]),
 *               sc = atol + max(|y|, |y_new|) rtol (y_new NULL: atol + |y| rtol); fixed-order fp64 reduction. */
int32_t diffsep_ode_stage_update(const diffsep_sde_config* sde, const float* x, const float* t, const float* score,
                                 const float* sigma_mix, const double* y, float* const* K, const double* coef,
                                 int32_t n_k, int32_t k_out, double h, float* x_out, double* y_new_out, int32_t B,
                                 int32_t S, int64_t T, void* stream);
int32_t diffsep_ode_error_norm(const diffsep_sde_config* sde, const float* x, const float* t, const float* score,
                               const float* sigma_mix, const double* y, const double* y_new, float* const* K,
                               const double* coef, int32_t n_k, int32_t k_out, double h, double rtol, double atol,
                               double* norms_out, int32_t B, int32_t S, int64_t T, void* workspace,
                               int64_t workspace_bytes, void* stream);

/* The two passes with per-utterance tables, as diffsep_ode_sample_each launches them (sdes/__init__.py:193-278 per
 * utterance).  h [B] (fp64), active [B] and lengths [B] (int32) are DEVICE arrays; everything else as above.
 *   active[b] == 0 : nothing of utterance b is read or written (its norms keep their value);
 *   t >= lengths[b]: never read; K[k_out], x_out and y_new_out are written as exact zeros there;
 *   norms_out [B][2]: the two norms of utterance b over its S * lengths[b] values, summed in the order
 *                     diffsep_ode_error_norm uses for B = 1, T = lengths[b] (whatever B, b and T are);
 *   workspace      : >= B * DIFFSEP_ODE_WORKSPACE_BYTES. */
int32_t diffsep_ode_stage_update_each(const diffsep_sde_config* sde, const float* x, const float* t, const float* score,
                                      const float* sigma_mix, const double* y, float* const* K, const double* coef,
                                      int32_t n_k, int32_t k_out, const double* h, const int32_t* active,
                                      const int32_t* lengths, float* x_out, double* y_new_out, int32_t B, int32_t S,
                                      int64_t T, void* stream);
int32_t diffsep_ode_error_norm_each(const diffsep_sde_config* sde, const float* x, const float* t, const float* score,
                                    const float* sigma_mix, const double* y, const double* y_new, float* const* K,
                                    const double* coef, int32_t n_k, int32_t k_out, const double* h,
                                    const int32_t* active, const int32_t* lengths, double rtol, double atol,
                                    double* norms_out, int32_t B, int32_t S, int64_t T, void* workspace,
                                    int64_t workspace_bytes, void* stream);

/* Use hipGraph replay of the per-NFE launch sequence inside diffsep_pc_sample (default 1). */
int32_t diffsep_engine_set_graph(diffsep_engine* e, int32_t enable);

/* Options (no counterpart in the reference: A/B switches, test aids and the bound of the graph cache).
 * Process-wide defaults of the kernel-dispatch switches "no_rw", "no_rw128", "rw_small", "no_rw_res" (0 / 1): read from the
 * environment variables DIFFSEP_NO_RW, DIFFSEP_NO_RW128, DIFFSEP_RW_SMALL, DIFFSEP_NO_RW_RES ONCE, changed here; they apply to
 * the unit entry points (diffsep_conv2d, ...) and are copied by every engine created afterwards. */
int32_t diffsep_set_option(const char* name, int64_t value);
/* Per engine: the same four switches, plus "graph_cache" (captured graphs kept, least recently used evicted; default 12),
 * "dbg_alloc" (log workspace allocations) and "ablate" (measurement aid: bit mask of launch classes that are skipped — the
 * results are garbage).  Synchronises the device and drops the engine's captured graphs. */
int32_t diffsep_engine_set_option(diffsep_engine* e, const char* name, int64_t value);
/* Current value of an engine option, "graphs_cached" = number of captured graphs held; -1 for an unknown name. */
int64_t diffsep_engine_get_option(const diffsep_engine* e, const char* name);

/* Measurement hook (bench.py): between begin and end every MFMA conv/GEMM launch of the engine is
 * bracketed by HIP events on its launch stream (graph replay bypassed).  Outputs are 12-entry arrays
 * indexed by kernel class: 3x3 {8x32 tile x 64 cout, 8x32 x 32, 8x8 x 64}, then the same
 * tiles for 1x1 / GEMM, the weight-stationary 64 -> 64 3x3 kernel, the small-image 3x3 kernel, the register-weight
 * 3x3 kernel (conv3x3_rw.hip), the fused attention block (attn_fused.hip), the streamed-weight 3x3 kernel (conv3x3_sw.hip) and
 * its split-precision sibling (conv3x3_sws.hip) — TWELVE entries: summed algorithmic flops, summed milliseconds, launch counts and (bytes, nullable)
 * summed algorithmic HBM bytes = every operand read once + the output written once. */
#define DIFFSEP_NUM_KERNEL_CLASSES 12
int32_t diffsep_engine_profile_begin(diffsep_engine* e);
/* Writes DIFFSEP_NUM_KERNEL_CLASSES entries per array — the caller's buffers must hold that many (ABI note: the count was 9
 * until round 3 and 10 until round 5; a caller compiled against an older header must use the _n form below or be rebuilt). */
int32_t diffsep_engine_profile_end(diffsep_engine* e, double* flops, double* ms, int64_t* launches, double* bytes);
/* The same with the capacity of the caller's arrays stated: writes min(n_classes, DIFFSEP_NUM_KERNEL_CLASSES) entries per
 * array and never more; *n_written (nullable) receives that number. */
int32_t diffsep_engine_profile_end_n(diffsep_engine* e, int32_t n_classes, double* flops, double* ms, int64_t* launches,
                                     double* bytes, int32_t* n_written);
int32_t diffsep_num_kernel_classes(void);
/* The launches of that span one by one (call after profile_end; out may be NULL to query *n): the kernel instantiation
 * with its template arguments, the problem shape, algorithmic flops / bytes and the measured duration.  Round 5: the
 * HBM-bound launches of the path (GroupNorm apply / FIR x2 resampling, STFT, iSTFT, SDE updates, RNG) are bracketed too and
 * appear here with cls = -1, flops = 0, Cin = channels, bytes = algorithmic HBM bytes (inputs read once, outputs written once);
 * they are not part of the per-class arrays of profile_end. */
typedef struct diffsep_prof_record {
  char kernel[128];
  int32_t B, H, W, Cin, Cout, taps, skip_cin, has_res, cls, _pad;
  double flops, bytes;
  double ms;
} diffsep_prof_record;
int32_t diffsep_engine_profile_records(diffsep_engine* e, diffsep_prof_record* out, int32_t cap, int32_t* n);

/* ------------------------------------------------------------------ unit entry points
 * (used by the parity tests; the engine calls the same launchers internally). */

/* Time embedding of the backbone: temb[B][4 nf] = Linear_2(SiLU(Linear_1(GaussianFourierProjection(log t)))).
 * Replaces: models/ncsnpp.py:324-343 (all_modules[0..2]), models/ncsnpp_utils/layerspp.py:37-47 (the projection).
 * fourier_w [nf] (the frozen W, scale included), w1 [4 nf][2 nf], b1 [4 nf], w2 [4 nf][4 nf], b2 [4 nf] (nn.Linear layout),
 * all float32 device pointers; workspace >= B * 6 nf floats. */
int32_t diffsep_time_embedding(const float* t, const float* fourier_w, const float* w1, const float* b1, const float* w2,
                               const float* b2, float* temb, int32_t B, int32_t nf, void* workspace,
                               int64_t workspace_bytes, void* stream);

/* The wide Dense_0 projection of the backbone in isolation: y[B][sum O_i] = act(x) W^T + bias, act = SiLU when silu_in != 0,
 * for n_blocks nn.Linear weight blocks [O_i][K] stored one after the other in w (every ResnetBlockBigGANpp's Dense_0 at once,
 * layerspp.py:311-312), through the launchers the engine uses: each block is transposed into the concatenation [K][sum O_i] in
 * the workspace, then one product runs over all of them.  x [B][K], w [sum O_i][K], bias [sum O_i] or NULL, y: float32 device
 * pointers; out_ch_host [n_blocks]: host array of the O_i; K a multiple of 4, at most 1024; workspace >= K * sum O_i floats. */
int32_t diffsep_dense_projection(const float* x, const float* w, const float* bias, const int32_t* out_ch_host,
                                 int32_t n_blocks, float* y, int32_t B, int32_t K, int32_t silu_in, void* workspace,
                                 int64_t workspace_bytes, void* stream);

/* upfirdn2d with the [1,3,3,1] FIR, factor 2: upsample_2d / downsample_2d
 * (models/ncsnpp_utils/up_or_down_sampling.py:206-273; native op op/upfirdn2d.cpp:12-23,
 * op/upfirdn2d_kernel.cu:107-207).  up!=0: [B,H,W,C] -> [B,2H,2W,C]; else -> [B,H/2,W/2,C]. */
int32_t diffsep_upfirdn2d(const void* x, void* y, int32_t B, int32_t H, int32_t W, int32_t C, int32_t ldx,
                          int32_t ldy, int32_t up, int32_t dtype, void* stream);

/* y = act(GroupNorm(x)) with G = min(C/4,32), eps, affine (layerspp.py:264-266,292,313);
 * act: 0 none (attention GN, layerspp.py:78) / 1 SiLU.  resample: 0 none / 1 FIR up / 2 FIR down
 * applied to act(GN(x)) (layerspp.py:294-299); xr (nullable) receives the same resampling of raw x. */
int32_t diffsep_groupnorm_act(const void* x, const float* gamma, const float* beta, void* y, void* xr, int32_t B,
                              int32_t H, int32_t W, int32_t C, int32_t ldx, int32_t ldy, int32_t ldxr,
                              int32_t groups, float eps, int32_t act, int32_t resample, int32_t dtype,
                              void* workspace, int64_t workspace_bytes, void* stream);
/* ... with split (as above) and the network's output layer applied on the fly (ow != NULL; all device pointers): x is then the
 * last pyramid tensor [B,256,W,Cpad] and every pixel becomes v[c] = (sum_{k < ow_cin} ow[c][k] x[k]) / tdiv[b] + ob[c] first.
 * ow [2S][ow_cin] f32, ob [2S] f32, tdiv [B] f32, 2S <= ow_cin <= 8 (anything else is refused).  ow == NULL: ob, tdiv
 * and ow_cin are ignored.  Name left behind: "istft_fused_kernel<NS,EM>" (NS = 2 at S = 2, else 1; EM = 0 | 1 | 2: exponent 0.5 |
 * 1 | other) or the route's last kernel "istft_ola_kernel". */
int32_t diffsep_istft_unpack_ex(const void* x, float* out, int32_t B, int32_t S, int64_t T, int32_t n_fft,
                                int32_t hop, float exponent, float factor, int32_t W, int32_t Cpad, int32_t dtype,
                                void* workspace, int64_t workspace_bytes, void* stream, int32_t split, const float* ow,
                                const float* ob, const float* tdiv, int32_t ow_cin);

/* 3x3 (pad 1) or 1x1 convolution, NHWC, implicit GEMM on MFMA:
 * y = (conv(x, w) + bias[co] + bias_b[b,co] + res) * out_scale     (layers.py:112-119,141-156;
 * the fused terms are layerspp.py:306-323).  w: [Cout][taps][Cin] in `dtype` (taps = ky*3+kx). */
int32_t diffsep_conv2d(const void* x, const void* w, const float* bias, const float* bias_b, const void* res,
                       void* y, int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t ksize,
                       int32_t ldx, int32_t ldr, int32_t ldy, float out_scale, int32_t dtype, void* stream);

/* GroupNorm statistics only: per-(b,c) scale = rstd*gamma, shift = beta - mean*scale ([B][C] fp32), optionally
 * over the in-place channel concat cat([x, x2]) (x holds C1 channels).  The convolutions consume them. */
int32_t diffsep_groupnorm_stats(const void* x, const void* x2, int32_t C1, const float* gamma, const float* beta,
                                float* scale, float* shift, int32_t B, int32_t H, int32_t W, int32_t C, int32_t ldx,
                                int32_t ldx2, int32_t groups, float eps, int32_t dtype, void* workspace,
                                int64_t workspace_bytes, void* stream);

/* diffsep_conv2d with the producer-side fusions the engine uses: the input may be cat([x, x2], C) read in
 * place (ncsnpp.py:411) and act(GroupNorm(.)) (layerspp.py:292,313) is applied to it on the fly from
 * per-(b,c) scale/shift (gn_act: 0 none, 1 SiLU); zero padding is applied AFTER the activation. */
int32_t diffsep_conv2d_fused(const void* x, const void* x2, int32_t C1, const float* gn_scale, const float* gn_shift,
                             int32_t gn_act, const void* w, const float* bias, const float* bias_b, const void* res,
                             void* y, int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t ksize,
                             int32_t ldx, int32_t ldx2, int32_t ldr, int32_t ldy, float out_scale, int32_t dtype,
                             int64_t* stats, int32_t w_chunk, const int64_t* gn_acc1, const int64_t* gn_acc2,
                             const float* gn_gamma, const float* gn_beta, int32_t gn_groups, void* stream);
/* `w_chunk` = 0: w is [Cout][k*k][Cin_pad]; = kc = diffsep_conv2d_chunk(ksize, dtype): w is chunk-major
 * [Cin_pad / kc][k*k][Cout][kc] (the layout the engine keeps its weights in: one K stage of the kernel is then
 * contiguous in memory and is fetched in full 128-byte lines). */
int32_t diffsep_conv2d_chunk(int32_t ksize, int32_t dtype);
/* The general one-tap launch of csrc/conv_mfma.hip (batched NT GEMM), as the unfused attention path assembles it for Q K^T, P V
 * and V^T:  Y[b, m, n] = ((sum_k A[b | shared, m, k] * Bt[b | shared, n, k]) / div_b[b] + bias + res[b, m, n]) * out_scale.
 * a [B | 1][M][lda], bt dense [B | 1][N][K] (a_batched / bt_batched = 0: one matrix shared by the batch), res [B][M][ldr] or NULL,
 * y [B][M][ldy]; bias fp32 [N] (bias_mode 0, along n) or [M] (bias_mode 1, along m) or NULL; div_b fp32 [B] or NULL.  K, lda, ldr,
 * ldy multiples of 8, ldr / ldy >= N rounded up to 8.  Columns [N, N rounded up to 8) of y are written as zeros (res must hold
 * zeros there), columns beyond are not touched.  dtype: DIFFSEP_F32, DIFFSEP_F32_SPLIT or DIFFSEP_BF16. */
int32_t diffsep_gemm_nt(const void* a, const void* bt, const float* bias, const float* div_b, const void* res, void* y, int32_t B,
                        int32_t M, int32_t N, int32_t K, int32_t lda, int32_t ldr, int32_t ldy, int32_t a_batched,
                        int32_t bt_batched, int32_t bias_mode, float out_scale, int32_t dtype, void* stream);
/* Name, with its template arguments, of the kernel instantiation that the calling thread's last convolution launch ran
 * (thread-local; "" before the first launch).  The fused attention kernel counts as one, from the unit entry point and from
 * the engine's block code alike: "attn_fused_kernel<LT>" with LT = 1, 2, 4, 8 tiles of 32 pixels.  So does every GroupNorm-apply /
 * FIR resampling launch of csrc/norm.hip: "gn_apply_kernel<MODE,affine|raw>", "gn_resample2x2_kernel<T,MODE>",
 * "gn_fir_down_strip_kernel<RS>", "gn_fir_down_tiled_kernel<RS>", "gn_resample_up_tiled_kernel<T>" (T = f32 | bf16 | f16). */
const char* diffsep_last_conv_kernel(void);
/* GroupNorm scale / shift [B][C1 + C2] fp32 from the int64 channel-sum accumulators [B][C][2] that the convolutions' `stats`
 * fill (acc2 nullable: the in-place concat of two tensors); npix = H * W of the tensor.  The expression, and the float-rounded
 * 1 / (npix * C / groups), that the convolutions evaluate when they are given `gn_acc1` instead of `gn_scale` / `gn_shift`:
 * both tables hold the same bits (tests/test_gn_table_gpu.py). */
int32_t diffsep_gn_finalize_acc(const int64_t* acc1, int32_t C1, const int64_t* acc2, int32_t C2, int32_t B, int64_t npix,
                                int32_t groups, float eps, const float* gamma, const float* beta, float* scale, float* shift,
                                void* stream);
/* The GroupNorm-apply / FIR x2 resampling kernels (csrc/norm.hip) as units on a CALLER'S table: y = FIR(act(x * scale[b,c] +
 * shift[b,c])) and xr = FIR(x) (mode 0: no FIR, no xr; 1: x2 up; 2: x2 down; zero padding of BOTH tensors after the activation),
 * x [B][H][W][ldx], y / xr [B][H'][W'][ldy / ldxr], C channels written, the other lanes untouched.  scale = shift = y = NULL: the
 * pyramid's pure FIR of x into xr.  act: 0 none, 1 SiLU.  The launch leaves its kernel's name in diffsep_last_conv_kernel().
 * route = DIFFSEP_GN_AUTO: the kernel the dispatch picks for the shape (what the engine runs).  Any other code forces that kernel
 * wherever its SHAPE preconditions hold — an error otherwise — and lifts only the dispatch's size thresholds:
 *   BLOCK2X2 (gn_resample2x2_kernel): table; up, or down with H % 4 == 0 and W % 4 == 0
 *   DOWN_STRIP4 / 8 (gn_fir_down_strip_kernel<4 | 8>): 16-bit, table, down, W % 4 == 0
 *   DOWN_TILED4 / 8 (gn_fir_down_tiled_kernel<4 | 8>): libdiffsep_hip_f16.so only, 16-bit, table, down, W % 32 == 0, C % 64 == 0,
 *                                                      ldx, ldy, ldxr multiples of 8
 *   UP_TILED (gn_resample_up_tiled_kernel): table, up, C % 64 == 0 */
#define DIFFSEP_GN_AUTO 0
#define DIFFSEP_GN_APPLY 1
#define DIFFSEP_GN_BLOCK2X2 2
#define DIFFSEP_GN_DOWN_STRIP4 3
#define DIFFSEP_GN_DOWN_STRIP8 4
#define DIFFSEP_GN_DOWN_TILED4 5
#define DIFFSEP_GN_DOWN_TILED8 6
#define DIFFSEP_GN_UP_TILED 7
int32_t diffsep_gn_apply(const void* x, const float* scale, const float* shift, void* y, void* xr, int32_t B, int32_t H, int32_t W,
                         int32_t C, int32_t ldx, int32_t ldy, int32_t ldxr, int32_t act, int32_t mode, int32_t dtype, int32_t route,
                         void* stream);
/* The dispatch alone, nothing launched (host arithmetic; needs no device when cus > 0): the kernel name that
 * diffsep_gn_apply(route = DIFFSEP_GN_AUTO) would leave in diffsep_last_conv_kernel() for this launch on a device of `cus` compute
 * units (<= 0: the current device's).  NULL (and diffsep_last_error) on a shape the entry point refuses. */
const char* diffsep_gn_route_name(int32_t mode, int32_t affine, int32_t dtype, int32_t B, int32_t H, int32_t W, int32_t C,
                                  int32_t ldx, int32_t ldy, int32_t ldxr, int32_t has_xr, int32_t cus);
/* The streamed-weight 3x3 kernel (csrc/conv3x3_sw.hip; the 128-cout layers with 192 / 256 input channels or a folded 1x1 skip
 * on up to 256 raw channels: ncsnpp.py:409-417, layerspp.py:291-323) as a unit, whatever the dispatch would pick.  Dense NHWC
 * 16-bit tensors: x [B][H][W][C1 or Cin], x2 (nullable) the other Cin - C1 channels; act(GroupNorm(.)) from per-(b, c)
 * scale / shift when gn_scale != NULL (SiLU), raw input otherwise; optional folded skip y += sw * cat([sx, sx2]) on RAW channels;
 * y [B][H][W][Cout] = (conv + bias + bias_b[b]) * out_scale; `stats` as in diffsep_conv2d_fused.  w_frag / sw_frag: the
 * [Cout][3 x 3][Cin] / [Cout][sCin] weights in FRAGMENT-major order — element (cout, tap, cin) at diffsep_frag_index(cout, tap,
 * cin, taps, Cout): one k-step (64-channel chunk, tap, 16-channel block) of all couts is contiguous, cout group by cout group,
 * so that a wave's 1 KB load instruction is one MFMA B-operand.
 * dtype = DIFFSEP_F32_SPLIT: the split mode's sibling (csrc/conv3x3_sws.hip; sdes/__init__.py:166-188 runs on it in the head of a
 * hybrid run): fp32 tensors, Cout = 64 / 128 / 256, every product as three bfloat16 MFMAs on hi / lo planes; w_frag / sw_frag
 * are then PAIRS of bfloat16 planes (hi = bf16(w), lo = bf16(w - hi)) at diffsep_frag_index_split(cout, tap, cin, taps, Cout,
 * plane).  `res` (nullable, no skip beside it; 16-bit: Cout = 128): residual [B][H][W][Cout] added before out_scale — it rides
 * through the matrix cores against `ident_frag`, the fragment copy (of that mode) of the Cout x Cout identity (taps = 1).
 * 16-bit tile shapes: 8 x 32 pixels x 128 couts, 4 x 32 x 128 where H % 8 != 0 (and, in the engine, on levels with fewer 8-row
 * tiles than compute units), 8 x 32 x 64 for the one 64-cout layer the register-weight kernel does not hold (Cin = 192).
 * gn_acc1 (nullable, instead of gn_scale / gn_shift; gn_acc2 for x2), gn_gamma, gn_beta, gn_groups: GroupNorm of the input from
 * its producers' accumulators, as in diffsep_conv2d_fused. */
int32_t diffsep_conv3x3_streamed(const void* x, const void* x2, int32_t C1, const float* gn_scale, const float* gn_shift,
                                 const void* w_frag, const float* bias, const float* bias_b, const void* sx, const void* sx2,
                                 int32_t sC1, int32_t sCin, const void* sw_frag, void* y, int32_t B, int32_t H, int32_t W,
                                 int32_t Cin, int32_t Cout, float out_scale, int32_t dtype, int64_t* stats, const void* res,
                                 const void* ident_frag, const int64_t* gn_acc1, const int64_t* gn_acc2, const float* gn_gamma,
                                 const float* gn_beta, int32_t gn_groups, void* stream);
/* The register-weight 3x3 kernel (csrc/conv3x3_rw.hip) as a unit, whatever the dispatch would choose, with its folded 1x1 skip:
 * dense NHWC 16-bit tensors, 64 / cat -> 64 or 128 -> 128 couts, H >= 32, H % 8 == 0, W % 32 == 0.  w as in diffsep_conv2d_fused
 * (row-major, or chunk-major with w_chunk); sx (+ sx2, split at sC1) [B][H][W][sCin] raw skip channels (64 / 128, 192 at
 * 64 -> 64) against sw [Cout][sCin] row-major, added before out_scale; res (nullable, no skip beside it) likewise. */
int32_t diffsep_conv3x3_regweight(const void* x, const void* x2, int32_t C1, const float* gn_scale, const float* gn_shift,
                                  const void* w, int32_t w_chunk, const float* bias, const float* bias_b, const void* sx,
                                  const void* sx2, int32_t sC1, int32_t sCin, const void* sw, const void* res, void* y, int32_t B,
                                  int32_t H, int32_t W, int32_t Cin, int32_t Cout, float out_scale, int32_t dtype, int64_t* stats,
                                  void* stream);
/* The fused attention kernel (csrc/attn_fused.hip) as a unit: x, y dense [B][L][C] 16-bit, C = 128, L = 16 .. 256 by 16; wqk
 * (= Wk^T Wq), wv, wo in the order of diffsep_frag_index(row, 0, column, 1, C); bqk = Wk^T b_q, bv, bo [C] fp32.  GroupNorm of x
 * (no activation) from gn_acc [B][C][2] + gn_gamma / gn_beta / gn_groups, or from gn_scale / gn_shift [B][C] when gn_acc is NULL.
 * stats (nullable): accumulators of y. */
int32_t diffsep_attn_fused(const void* x, const int64_t* gn_acc, const float* gn_gamma, const float* gn_beta, int32_t gn_groups,
                           const float* gn_scale, const float* gn_shift, const void* wqk, const void* wv, const void* wo,
                           const float* bqk, const float* bv, const float* bo, void* y, int64_t* stats, int32_t B, int32_t L,
                           int32_t C, void* stream);
int64_t diffsep_frag_index(int32_t cout, int32_t tap, int32_t cin, int32_t taps, int32_t Cout);
int64_t diffsep_frag_index_split(int32_t cout, int32_t tap, int32_t cin, int32_t taps, int32_t Cout, int32_t plane);
/* `stats` (nullable): channel-sum accumulators of the OUTPUT for the next GroupNorm, [B][Cout][2] int64 fixed point
 * (sum * 2^24, sum of squares * 2^16; exact to 6e-8 / 1.5e-5 per tile, no overflow while the per-image sum of
 * squares of a channel stays below 1.4e14).  Every block ADDS its tile's totals with integer atomics (associative:
 * bit-reproducible), the caller zeroes the buffer first — so no separate pass over the tensor is needed
 * (layerspp.py:313: GroupNorm_1 follows Conv_0).
 * `gn_acc1` (nullable, instead of gn_scale / gn_shift): such accumulators of x (and gn_acc2 of x2) plus the
 * GroupNorm affine parameters gamma / beta [Cin] and the group count; the kernel derives scale / shift itself
 * (eps = 1e-6, statistics over H * W * Cin / groups elements per group). */

/* ResnetBlockBigGANpp.forward (layerspp.py:291-323) through the engine's own block code (GroupNorm + SiLU fused into
 * the convolutions' input staging, FIR up / down of both branches in one pass, Conv_2 folded into Conv_1, temb
 * projection Dense_0(act(temb))): x [B,H,W,in_ch] NHWC (dtype), temb [B,temb_dim] f32 -> y [B,H',W',out_ch].
 * params_host: the block's parameters as one float32 blob in reference state_dict order (GroupNorm_0.{weight,bias},
 * Conv_0.{weight,bias}, Dense_0.{weight,bias}, GroupNorm_1.{weight,bias}, Conv_1.{weight,bias}[, Conv_2.{weight,
 * bias} when in_ch != out_ch or up or down]).  Test aid: builds a one-module engine per call and synchronises. */
int32_t diffsep_resblock_forward(int32_t in_ch, int32_t out_ch, int32_t up, int32_t down, int32_t temb_dim,
                                 int32_t dtype, const float* params_host, int64_t n_floats, const void* x,
                                 const float* temb, void* y, int32_t B, int32_t H, int32_t W, void* stream);
/* AttnBlockpp.forward (layerspp.py:76-92) through the engine's block code: x, y [B,H,W,C] NHWC (dtype);
 * params_host = GroupNorm_0.{weight,bias}, NIN_0.{W,b} .. NIN_3.{W,b} as one float32 blob.  Test aid. */
int32_t diffsep_attnblock_forward(int32_t channels, int32_t dtype, const float* params_host, int64_t n_floats,
                                  const void* x, void* y, int32_t B, int32_t H, int32_t W, void* stream);

/* AttnBlockpp core (layerspp.py:83-87): o = softmax(q k^T * C^-0.5) v over L = H*W tokens.
 * q,k [B,L,C] (ld), vt [B,C,Lp] (V transposed, Lp = L rounded up to 8), o [B,L,C];
 * ws >= B*L*Lp*(2*elt) bytes.  QK^T and PV run on MFMA. */
int32_t diffsep_attention(const void* q, const void* k, const void* vt, void* o, int32_t B, int32_t L, int32_t C,
                          int32_t ld, int32_t dtype, void* workspace, int64_t workspace_bytes, void* stream);

/* pre_process (score_models.py:107-116) + the 2x-1 of ncsnpp.py:347-349: cat(xt, mix) -> right pad
 * n_fft-hop -> STFT(n_fft, hop, periodic Hann, center, zero pad) -> |z|^e e^{j angle} * factor ->
 * [re x S+1 | im x S+1] channels -> zero-pad frames to W (then 2x-1).
 * xt [B,S,T], mix [B,1,T] f32 -> y [B, n_fft/2+1, W, Cpad] (dtype), Cpad = roundup(2S+2, 8).
 * centered_shift != 0 applies 2x-1 (what the engine does); 0 leaves the packed spectrogram.
 * ws >= 2*((B*(S+1)*F + 8)*512*4 + 256) bytes (windowed frames + transposed spectrum of the DFT GEMM). */
int32_t diffsep_stft_pack(const float* xt, const float* mix, void* y, int32_t B, int32_t S, int64_t T,
                          int32_t n_fft, int32_t hop, float exponent, float factor, int32_t W, int32_t Cpad,
                          int32_t centered_shift, int32_t dtype, void* workspace, int64_t workspace_bytes,
                          void* stream);
/* ... with split != 0: the DFT matrix product of the three-launch route with bf16x3 products (what the bf16 and split engines
 * pass); the fused kernel (16-bit y, n_fft 510, hop 128, Cpad 8, W % 32 == 0) ignores it.  The launch leaves its kernel's name in
 * diffsep_last_conv_kernel(): "stft_fused_kernel<S+1>", or the route's last kernel "stft_pack_kernel<f32|bf16|f16>". */
int32_t diffsep_stft_pack_ex(const float* xt, const float* mix, void* y, int32_t B, int32_t S, int64_t T,
                             int32_t n_fft, int32_t hop, float exponent, float factor, int32_t W, int32_t Cpad,
                             int32_t centered_shift, int32_t dtype, void* workspace, int64_t workspace_bytes,
                             void* stream, int32_t split);

/* post_process (score_models.py:118-124): unpad frames -> channels to complex -> z/|factor| ->
 * |z|^(1/e) e^{j angle} -> iSTFT -> crop to T.  x [B,256,W,Cpad] (first 2S channels used) -> out [B,S,T];
 * ws >= 2*(B*S*F*512*4 + 256) bytes (decompressed bins + inverse-DFT frames). */
int32_t diffsep_istft_unpack(const void* x, float* out, int32_t B, int32_t S, int64_t T, int32_t n_fft,
                             int32_t hop, float exponent, float factor, int32_t W, int32_t Cpad, int32_t dtype,
                             void* workspace, int64_t workspace_bytes, void* stream);

/* PriorMixSDE._std_sigma_mix (sdes/sdes.py:477-489): sigma_mix[b,t] = 0.5*sqrt(clamp(avg_pool1d(mix^2, avg_len,
 * stride 1, pad avg_len/2), 1e-4)); mix [B,1,T] -> sigma_mix [B,T].  The three updates below take it as their
 * `sigma_mix` argument for kind = DIFFSEP_SDE_PRIORMIX (time-varying std, sdes.py:451-470,515-532) and NULL
 * for MixSDE. */
int32_t diffsep_sde_sigma_mix(const float* mix, float* sigma_mix, int32_t B, int64_t T, int32_t avg_len, void* stream);
/* MixSDE.prior_sampling (sdes/sdes.py:334-346) / PriorMixSDE.prior_sampling (:564-587):
 * x_T = 0.5*y (bcast) + L(T) @ z. */
int32_t diffsep_sde_prior(const diffsep_sde_config* sde, const float* y, const float* z, float* x, int32_t B,
                          int32_t S, int64_t T, const float* sigma_mix, void* stream);
/* AnnealedLangevinDynamics2.update_fn body for one step given the score
 * (sdes/correctors.py:115-126). t [B] device. */
int32_t diffsep_sde_corrector_update(const diffsep_sde_config* sde, float snr, const float* x, const float* t,
                                     const float* score, const float* z, float* x_out, float* x_mean_out,
                                     int32_t B, int32_t S, int64_t T, const float* sigma_mix, int32_t variant,
                                     void* stream); /* variant: 0 = ald2, 1 = ald (sdes/correctors.py:58-91) */
/* ReverseDiffusionPredictor.update_fn given the score (sdes/predictors.py:60-66 ->
 * sdes/sdes.py:163-171,93-107,275-284); dt = 1/N.  EulerMaruyamaPredictor (predictors.py:39-52) is the same
 * update.  probability_flow != 0: RSDE.discretize with half the score term and no noise (sdes.py:165-171). */
int32_t diffsep_sde_predictor_update(const diffsep_sde_config* sde, int32_t N, const float* x, const float* t,
                                     const float* score, const float* z, float* x_out, float* x_mean_out,
                                     int32_t B, int32_t S, int64_t T, const float* sigma_mix,
                                     int32_t probability_flow, void* stream);
/* ---- the SDE object surface a user-written Predictor / Corrector reaches through the reference API.  The fused
 * sampler never calls these; diffsep_amd/sdes/sdes.py builds sde() / marginal_prob() / mult_std() / discretize() /
 * reverse() on them. ----
 * SDE.sde (MixSDE sdes/sdes.py:275-284, PriorMixSDE :451-470) scaled for SDE.discretize (:93-107):
 *   drift_out [B,S,T] = f_scale * (-lambda P x);  diffusion_out = g_scale * g(t) [B]  (MixSDE)
 *                                                              or g_scale * g(t) sigma_mix [B,S,T] (PriorMixSDE).
 *   sde(): f_scale = g_scale = 1; discretize(): f_scale = dt, g_scale = sqrt(dt), dt = 1/N (quirk Q1). */
int32_t diffsep_sde_coefficients(const diffsep_sde_config* sde, const float* x, const float* t, const float* sigma_mix,
                                 float* drift_out, float* diffusion_out, int32_t B, int32_t S, int64_t T, float f_scale,
                                 float g_scale, void* stream);
/* MixSDE._mean (sdes/sdes.py:286-294): (A + exp(-lambda t) P) x0, the mean of marginal_prob (:322-324). */
int32_t diffsep_sde_mean(const diffsep_sde_config* sde, const float* x0, const float* t, float* mean_out, int32_t B,
                         int32_t S, int64_t T, void* stream);
/* MixSDE._std (sdes/sdes.py:315-320) -> std_out [B,S,S]; PriorMixSDE._std (:515-532, sigma_mix != NULL) ->
 * std_out [B,S,S,T]: the second member of marginal_prob. */
int32_t diffsep_sde_std(const diffsep_sde_config* sde, const float* t, const float* sigma_mix, float* std_out, int32_t B,
                        int32_t S, int64_t T, void* stream);
/* MixSDE.mult_std (std @ x, sdes/sdes.py:326-328; per_sample = 0, std [B,S,S]) / PriorMixSDE.mult_std
 * (einsum "bcdt,bdt->bct", :534-537; per_sample = 1, std [B,S,S,T]) for any dense std. */
int32_t diffsep_sde_mult_std(const float* std, const float* x, float* out, int32_t B, int32_t S, int64_t T,
                             int32_t per_sample, void* stream);
/* MixSDE.mult_std_inv (torch.linalg.solve(std, x), sdes/sdes.py:330-332; per_sample = 0, std [B,S,S]) /
 * PriorMixSDE.mult_std_inv (:534-558; per_sample = 1, std [B,S,S,T]) for any dense std: the reference's explicit 2x2 formula
 * for S = 2 with a per-sample std, LU with partial pivoting in registers otherwise.  (The fused loss kernels below do not
 * solve: for the SDE's own std the inverse is A / sqrt(ev1) + Pn / sqrt(ev2), divided by sigma_mix.) */
int32_t diffsep_sde_mult_std_inv(const float* std, const float* x, float* out, int32_t B, int32_t S, int64_t T,
                                 int32_t per_sample, void* stream);
/* RSDE.discretize (sdes/sdes.py:163-171) given the forward discretisation: rev_f = f - G^2 score (x 0.5 when
 * probability_flow); G is [B] (g_full = 0) or [B, n_per_batch] (g_full = 1). */
int32_t diffsep_sde_reverse_drift(const float* f, const float* G, const float* score, float* rev_f_out, int32_t B,
                                  int64_t n_per_batch, int32_t g_full, int32_t probability_flow, void* stream);

/* LangevinCorrector.update_fn body for one step (sdes/correctors.py:43-53): step = 2 (snr <||z_b||> / <||g_b||>)^2
 * from batch-mean norms, x_mean = x + step g, x = x_mean + sqrt(2 step) z.  x etc. are [B, n_per_batch];
 * ws >= 16*B + 16 bytes. */
int32_t diffsep_sde_langevin_update(float snr, const float* x, const float* score, const float* z, float* x_out,
                                    float* x_mean_out, int32_t B, int64_t n_per_batch, void* workspace,
                                    int64_t workspace_bytes, void* stream);

/* normalize_batch (pl_model.py:81-88): per-utterance mean / unbiased std (clamped 1e-5) over (1,T).
 * mix [B,1,T] -> mix_norm; mean,std [B] (nullable). */
int32_t diffsep_normalize_batch(const float* mix, float* mix_norm, float* mean, float* std, int32_t B, int64_t T,
                                void* stream);
/* scale_output (separate.py:73-78): alpha = <mix,sep>/sum(sep^2+1e-10); sep*alpha, in place. */
int32_t diffsep_scale_output(const float* mix, float* sep, int32_t B, int32_t S, int64_t T, void* stream);

/* Gram matrices of references and estimates for the separation metrics (evaluate.py:103-132:
 * fast_bss_eval.si_bss_eval_sources(ref, est, zero_mean=False, compute_permutation=True)): out [B][3][S][S] float64 =
 * { ref ref^T, ref est^T, est est^T }.  SI-SDR / SI-SIR / SI-SAR and the best permutation follow from these alone. */
int32_t diffsep_gram(const float* ref, const float* est, double* out, int32_t B, int32_t S, int64_t T, void* stream);

/* STOI / ESTOI of every source of a zero-padded batch (evaluate.py:113-130: pystoi's stoi(ref, est, fs, extended) per source;
 * C. H. Taal, R. C. Hendriks, R. Heusdens, J. Jensen, "An Algorithm for Intelligibility Prediction of Time-Frequency Weighted
 * Noisy Speech", IEEE TASLP 2011; J. Jensen, C. H. Taal, "An Algorithm for Predicting the Intelligibility of Speech Masked by
 * Modulated Noise Maskers", IEEE/ACM TASLP 2016).  ref, est [B,S,T] float32; out [B][S] float64: estimate row perm[b][i]
 * (NULL: i) scored against reference row i over the first lengths[b] (NULL: T) samples, in float64 from the samples on:
 * polyphase resampling to 10 kHz (Kaiser-windowed sinc, 60 dB), silent-frame removal (40 dB), 15 one-third octave bands of
 * 256-sample Hann frames, 30-frame segments; fewer than 30 frames left: 1e-5.  extended != 0: ESTOI.  lengths, perm: device
 * int32.  Row (b, i) does not depend on the rest of the batch or on the stream (fixed-order reductions).  fs: any rate whose
 * reduced 10000 / fs = p / q has p, q <= 1000 (8000, 10000, 16000, 44100, 48000 ...); others are refused.
 * Caller-owned workspace of diffsep_stoi_workspace_bytes(B, S, T, fs) bytes (host arithmetic only; -1 and an error message for
 * a bad shape or rate). */
int64_t diffsep_stoi_workspace_bytes(int32_t B, int32_t S, int64_t T, int32_t fs);
int32_t diffsep_stoi(const float* ref, const float* est, double* out, int32_t B, int32_t S, int64_t T,
                     const int32_t* lengths, const int32_t* perm, int32_t fs, int32_t extended, void* workspace,
                     int64_t workspace_bytes, void* stream);

/* Ingredients of the Hu & Loizou composite measures CSIG / CBAK / COVL for every source of a zero-padded batch
 * (evaluate_covl.py:18-54 eval_composite; :358-408 llr with :62-95 lpcoeff; :155-355 wss; :106-152 SSNR): the log-likelihood
 * ratio, the weighted spectral slope and the segmental SNR.  ref, est [B,S,T] float32; estimate row perm[b][i] (NULL: i) is
 * scored against reference row i over the first lengths[b] (NULL: T) samples, in float64 from the samples on.  fs = 16000
 * (30 ms frames of 480 samples, 1024-point spectrum, LPC order 16) or 8000 (240, 512, 10); frames start every win / 4
 * samples, n = max(0, (len - win) div (win / 4)) of them, under the window 0.5 (1 - cos(2 pi j / (win + 1))), j = 1..win.
 *   LLR  per frame: log of the ratio of the two LPC residual energies on the reference's autocorrelation (Levinson-Durbin
 *        with the max(1e-15, E) guard, both quadratic forms floored at 1e-10); the reference's float32 casts are NOT
 *        reproduced;
 *   WSS  per frame: 25 Gaussian critical bands on the power spectrum, dB with a 1e-10 floor, 24 slopes, Klatt's weights
 *        from the nearest peak (Kmax 20, Klocmax 1), sum W dslope^2 / sum W;
 *   segSNR per frame: 10 log10(E_ref / (E_diff + 1e-10) + 1e-10) clamped to [-10, 35] after removing each signal's mean
 *        and scaling the estimate by max|ref| / max|est| (LLR and WSS see the original samples).
 * out [B][S][4] float64 = { mean of the m = round-half-even(0.95 n) smallest frame LLRs, the same of the frame WSS, mean
 * segSNR over all frames, n }; n = 0: NaN, NaN, NaN, 0.  frames_out (nullable) [B][S][3][frames_cap] = per-frame { llr, wss,
 * segsnr } in frame order, entries beyond n untouched; frames_cap >= the frame count of T when given.  lengths, perm: device
 * int32.  Row (b, i) does not depend on the rest of the batch or on the stream (fixed-order reductions, no atomics);
 * asynchronous on stream, no host readback.  S in 1..3.  A refusal returns non-zero with a message and writes nothing.
 * Caller-owned workspace of diffsep_composite_workspace_bytes(B, S, T, fs) bytes (host arithmetic only; -1 and an error
 * message for a bad shape or rate, or for more frames per row than the on-device ranking takes: 65536). */
int64_t diffsep_composite_workspace_bytes(int32_t B, int32_t S, int64_t T, int32_t fs);
int32_t diffsep_composite(const float* ref, const float* est, double* out, double* frames_out, int64_t frames_cap,
                          int32_t B, int32_t S, int64_t T, const int32_t* lengths, const int32_t* perm, int32_t fs,
                          void* workspace, int64_t workspace_bytes, void* stream);

/* BSS-eval SDR / SIR / SAR with a time-invariant distortion filter of L taps for every utterance of a zero-padded batch
 * (mir_eval.separation.bss_eval_sources; fast_bss_eval.bss_eval_sources(ref, est, filter_length=L), the package that
 * evaluate.py:103-132 imports for the scale-invariant forms).  ref, est [B,S,T] float32; the first lengths[b] (NULL: T)
 * samples count and samples beyond them are never read; float64 from the samples on.  With A_i the (n + L - 1) x L matrix
 * whose column tau is reference i delayed by tau, A = [A_0 ... A_{S-1}] and P_i, P the orthogonal projections onto their
 * column spans: s_target = P_i e_j, e_interf = P e_j - P_i e_j, e_artif = e_j - P e_j.  Computed from correlations:
 *   c_ik(l) = sum_m r_i[m] r_k[m + l], |l| < L;   R[(i,tau),(k,tau')] = c_ik(tau - tau')  (S L x S L, block Toeplitz);
 *   b_j[(i,tau)] = sum_m r_i[m - tau] e_j[m];   E_j = sum e_j^2;   q_ij = b_ij^T R_ii^-1 b_ij;   Q_j = b_j^T R^-1 b_j
 *   SDR[i][j] = 10 log10(q_ij / (E_j - q_ij)),  SIR[i][j] = 10 log10(q_ij / (Q_j - q_ij)),  SAR[j] = 10 log10(Q_j / (E_j - Q_j))
 * by direct time-domain sums and dense Cholesky factorisations (no approximation).  A denominator <= 0 gives +inf (S = 1:
 * every SIR, exactly).  A non-positive Cholesky pivot (a silent reference) makes what depends on that factorisation NaN: of
 * R_ii, row i of the SDR and SIR tables; of R, every SIR and SAR of the utterance; no other utterance is touched and the
 * call returns normally.  clamp_db > 0 clamps every value that is not NaN, the infinite ones included, to [-clamp_db,
 * clamp_db]; 0: no clamp.  perm (device int32 [B][S], entries clamped to [0, S)) NULL: the permutation of largest summed
 * clamped SDR[i][perm[i]], NaN counting as -inf, the earliest in lexicographic order on a tie (the enumeration of
 * diffsep_longform_stitch and diffsep_ensemble).  out [B][3][S] = { SDR[i][perm[i]], SIR[i][perm[i]], SAR[perm[i]] };
 * pair_out (nullable) [B][2][S][S] = the SDR and SIR tables [i][j]; perm_out (nullable) [B][S] = the permutation used.
 * S in 1..3, L in 1..1024, B S <= 65535, T < 2^31; n < L is legal (the missing lags are zero).  Asynchronous on stream, no
 * host readback.  Every sum has a fixed order that depends on n and L alone (no atomics): row b is bit for bit what the call
 * gives for that utterance alone, at any padded T, in any batch, on any stream.  A refusal (shape, a null ref / est / out /
 * workspace, clamp_db < 0, workspace_bytes too small, a workspace not 8-byte aligned) is decided before the first device
 * call, returns non-zero with a message naming the argument and writes nothing.
 * Caller-owned workspace of diffsep_bss_eval_workspace_bytes(B, S, T, L) bytes (host arithmetic only; -1 and a message for a
 * refused shape): with J = 2 S^2 + S correlation rows and C = ceil(T / 2048) time chunks, four pieces, each rounded up to
 * 256 bytes:  8 B J C L  +  8 B J L  +  8 B ((S L + S) S L + (S - 1)(L + S) L)  +  4 B S
 * (S = 3, L = 512: 23.1 MB per utterance for the systems and their right-hand sides). */
int64_t diffsep_bss_eval_workspace_bytes(int32_t B, int32_t S, int64_t T, int32_t L);
int32_t diffsep_bss_eval(const float* ref, const float* est, double* out, double* pair_out, int32_t* perm_out, int32_t B,
                         int32_t S, int64_t T, const int32_t* lengths, const int32_t* perm, int32_t L, double clamp_db,
                         void* workspace, int64_t workspace_bytes, void* stream);

/* Band-limited sample-rate conversion of fp32 rows by a reduced ratio p / q (fs_out / fs_in) with an odd-length FIR
 * h[0 .. 2 L] in float64, applied as given — the zero-stuffed direct form, centred:
 *   y[m] = sum_j h[m q + L - p j] (double)x[j],  0 <= j < len, tap index in [0, 2 L],  0 <= m < n_out = ceil(len p / q),
 * what scipy.signal.resample_poly(x, p, q, window=h / p) computes.  Float64 throughout, each term entering by one fused
 * multiply-add (the product is not rounded on its own: an unfused float64 reference agrees within the summation bound, bit for
 * bit only where every sum is exact), one rounding at the end for fp32 output; every output is summed in a fixed order that depends on p, q and L only (no atomics): a row comes out bit for
 * bit the same alone, inside any batch and on any stream.
 * Host arithmetic only, no device needed:
 *   diffsep_resample_ratio   p / q = fs_out / fs_in reduced; refuses (non-zero, message) rates <= 0 and max(p, q) > 1000;
 *   diffsep_resample_length  ceil(n p / q), or -1 and a message for n < 0, p, q < 1 or an n p beyond 64 bits;
 *   diffsep_resample_design  the project's filter for a reduced p / q (Octave's resample design: Kaiser-windowed sinc, 60 dB
 *                            rejection, L = ceil(52 / (28.714 / (20 max(p, q)))), taps summing to p; p = q = 1: the one tap 1.0):
 *                            returns 2 L + 1 and fills taps_out (NULL: the count only), or -1 and a message (p / q not reduced
 *                            or beyond 1000, cap < 2 L + 1).
 * diffsep_resampler_create builds the polyphase-ordered tap table on the current device from the CALLER's taps (any odd-length
 * FIR); it refuses null taps, an even or zero ntaps, ntaps > 2^17 and a p / q that is not reduced or beyond 1000.  The handle
 * is read-only afterwards: any number of streams may use it at once.  diffsep_resampler_destroy frees it (NULL: no-op).
 * diffsep_resample — x [rows][ldx] fp32 -> y [rows][ldy] of out_dtype (DIFFSEP_F32 or DIFFSEP_F64); rows r with
 * r div rows_per_length = g count lengths[g] samples (device int32, clamped to [0, T]; NULL: T everywhere).  Every column
 * below ceil(T p / q) is written, those from the row's own n_out on as zeros (a valid zero-padded batch); columns from
 * ceil(T p / q) on are left alone.  lengths_out (nullable device int32) receives each group's n_out.  Asynchronous on
 * `stream`, no host readback, no workspace.  Refusals (null pointers, an unknown out_dtype, T outside 1 .. 2^31 - 1, ldx < T,
 * ldy < ceil(T p / q), rows outside 1 .. 65535, rows_per_length < 1, a handle of another device) return non-zero with a message
 * and write nothing. */
int32_t diffsep_resample_ratio(int32_t fs_in, int32_t fs_out, int32_t* p, int32_t* q);
int64_t diffsep_resample_length(int64_t n, int32_t p, int32_t q);
int32_t diffsep_resample_design(int32_t p, int32_t q, double* taps_out, int32_t cap);
int32_t diffsep_resampler_create(int32_t p, int32_t q, const double* taps, int32_t ntaps, diffsep_resampler** out);
void diffsep_resampler_destroy(diffsep_resampler* r);
int32_t diffsep_resample(const diffsep_resampler* r, const float* x, int64_t ldx, void* y, int64_t ldy, int32_t rows, int64_t T,
                         const int32_t* lengths, int32_t rows_per_length, int32_t* lengths_out, int32_t out_dtype, void* stream);

/* Long recordings: a file of T samples as K windows of Tw samples with a nominal overlap of Tv, stitched on the device.
 * The plan (host arithmetic only, no device needed): refused (-1 and a message) unless T >= 1, Tv >= 1 and 3 Tv <= Tw.
 * T <= Tw: K = 1, starts = {0}, the one window is the file itself (T samples).  Otherwise hop = Tw - Tv,
 * K = 1 + ceil((T - Tw) / hop), starts[k] = k hop for k < K - 1 and starts[K - 1] = T - Tw: the last window is shifted back to
 * end at T, so every window is full length.  Windows k and k + 1 overlap on [starts[k + 1], starts[k] + Tw): Tv samples, more
 * for the last pair only.  Their seam is the n = min(Tv, overlap) samples from starts[k + 1] + (overlap - n) / 2 on; seams
 * never intersect, and a sample outside every seam belongs to exactly one window (the one between its neighbouring seams).
 * diffsep_longform_plan returns K and fills starts_out when it is non-NULL (cap < K is refused).  diffsep_longform_locate
 * says where sample t comes from, by the arithmetic the blend kernel uses: window *k alone (*n = 0), or offset *j of the
 * *n-sample seam of windows *k and *k + 1.
 * diffsep_longform_stitch — win [K][S][Tw] -> out [S][T], asynchronous on `stream`, no host readback, three launches; K must be
 * the plan's K (K = 1: the first T samples of the one window's rows).  Sources come out of a separator in arbitrary order per
 * window, so windows are aligned before they are cross-faded:
 *   cross-Gram  C_k[i][j] = sum over the overlap of win[k][i] win[k + 1][j]: products exact in float64, float64 sums in a fixed
 *               order (no atomics: the result does not depend on the stream, on co-resident work or on repetition);
 *               gram_out [K - 1][S][S] (nullable) receives them;
 *   permutation r_k = the permutation maximising sum_i C_k[i][r(i)] (= least squared distance over the overlap), candidates in
 *               lexicographic order with a strict >: a tie, an all-silent overlap included, keeps the earliest (the identity);
 *               g_0 = identity, g_{k+1}[i] = r_k[g_k[i]]; perm_out [K][S] = g: output source i is row g_k[i] of window k;
 *   blend       every out[i][t] written exactly once (no pre-zeroing): the owning window's sample, or inside a seam
 *               a + (b - a) r, r = (j + 0.5f) / n, each operation rounded to float32 on its own — where the two windows
 *               agree bit for bit the output is that value bit for bit.
 * S in 1..3.  Refusals (S, K, a refused plan, a workspace below diffsep_longform_workspace_bytes(K, S), null pointers) return
 * non-zero with a message and write nothing.  Alignment sees the overlap only: a source silent through a whole overlap leaves
 * that pair's decision to the tie rule or to noise. */
int32_t diffsep_longform_plan(int64_t T, int64_t Tw, int64_t Tv, int64_t* starts_out, int32_t cap);
int32_t diffsep_longform_locate(int64_t T, int64_t Tw, int64_t Tv, int64_t t, int32_t* k_out, int64_t* j_out, int64_t* n_out);
int64_t diffsep_longform_workspace_bytes(int32_t K, int32_t S);
int32_t diffsep_longform_stitch(const float* win, int32_t K, int32_t S, int64_t Tw, int64_t T, int64_t Tv, float* out,
                                int32_t* perm_out, double* gram_out, void* workspace, int64_t workspace_bytes, void* stream);

/* Posterior draws: K draws of every utterance of a zero-padded batch, brought to one source order and reduced on the device
 * (extension: the reference returns one draw per call and has no counterpart).  draws [B][K][S][T] float32; anchor [B][S][T]
 * or NULL = draw 0 of each utterance; lengths device int32 [B] or NULL (= T); n = lengths[b].  Asynchronous on `stream`, no
 * host readback, no floating-point atomics; five launches (four without pick_out).  For utterance b:
 *   cross-Gram  C[k][i][j] = sum_{t<n} (double)a[i][t] (double)d[k][j][t], a = the anchor: products exact in float64, sums in the
 *               fixed order of the block reductions, the 32 block partials of an entry folded in index order;
 *               gram_out [B][K][S][S] (nullable) receives them;
 *   permutation r_k = the permutation maximising sum_i C[k][i][r(i)] (= least squared distance to the anchor), candidates in
 *               lexicographic order with a strict >: a tie, an all-silent draw included, keeps the identity — the rule of
 *               diffsep_longform_stitch, the same code.  With anchor == NULL r_0 is the identity by construction (draw 0 is
 *               not searched against itself).  perm_out [B][K][S] = r: aligned source i of draw k is its row r_k[i],
 *               v_k[i][t] = d[k][r_k[i]][t];
 *   mean        m[i][t] = (((v_0 + v_1) + ...) + v_{K-1}) / K in float64, mean_out = (float)m;
 *   spread      std_out (nullable) = (float)sqrt(sum_k (v_k - m)^2 / K), the population form, k ascending, each operation
 *               rounded on its own in float64;
 *   distance    dist_out [B][K]: dist[k] = sum_{i, t<n} (v_k[i][t] - m[i][t])^2 in float64 against the unrounded m, in a fixed
 *               order (block partials folded source-major);
 *   medoid      medoid_out [B] = argmin_k dist[k], scanning from k = 0 with a strict <; pick_out (nullable) = v_medoid, bit for
 *               bit.
 * Samples at t >= n are never read; mean_out, std_out and pick_out [B][S][T] are written as exact +0.0 there (no pre-zeroing).
 * Every output of utterance b is bit for bit what the call gives for that utterance alone (B = 1, T = n), in any batch, at any
 * padded width, on any stream: the partition of the time axis into blocks is a function of n alone.  Rows are read with 16-byte
 * loads where all base pointers are 16-byte aligned and T is a multiple of 4, sample by sample otherwise and at ragged ends; the
 * two paths give the same bits.  K in 1..32, S in 1..3, B in 1..65535, 1 <= T < 2^31.  Refusals (K, S, B, T, a null required
 * pointer, a workspace below diffsep_ensemble_workspace_bytes(B, K, S) or not 8-byte aligned) are checked before the first
 * device call, return non-zero with a message that names the argument, and write nothing.
 * diffsep_ensemble_workspace_bytes: host arithmetic only; -1 and a message for a refused shape. */
int64_t diffsep_ensemble_workspace_bytes(int32_t B, int32_t K, int32_t S);
int32_t diffsep_ensemble(const float* draws, const float* anchor, const int32_t* lengths, int32_t B, int32_t K, int32_t S,
                         int64_t T, float* mean_out, float* std_out, float* pick_out, int32_t* perm_out, double* dist_out,
                         int32_t* medoid_out, double* gram_out, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- warm start: from another separator's estimates to the x_init of diffsep_pc_sample_from at a chosen diffusion time.  The
 * reference holds the pieces and no such call: normalize_batch((mix, tgt)) (pl_model.py:81-88) and the forward marginal
 * SDE.marginal_prob (sdes/sdes.py:322-324: MixSDE._mean :286-294 and _std :315-320; PriorMixSDE._std :515-532), which its training
 * draws from in DiffSepModel.sample_prior (pl_model.py:179-247).  Two launches, asynchronous on `stream`, nothing read back:
 *   fit (scale = DIFFSEP_WARM_SCALE_LS): per utterance over its own n = lengths[b] samples, in float64 from the fp32 samples, the
 *     Gram matrix of the estimates and their inner products with the RAW mixture; gains = argmin_g || mix - sum_s g_s est_s ||^2 by
 *     Cholesky.  A pivot <= 2^-40 trace / S (a silent estimate, two proportional estimates) sets every gain of that utterance to 1
 *     and fallback_out[b] = 1 (otherwise 0).  DIFFSEP_WARM_SCALE_NONE: no pass, gains exactly 1.
 *   apply and perturb, one pass over [B,S,T]:
 *     x0_i = (gain_i est_i - mean_b) / std_b;   m = mix_norm / S (DIFFSEP_WARM_MEAN_MIX) or mean_s x0 (DIFFSEP_WARM_MEAN_ESTIMATE:
 *     marginal_prob exactly);   x_init_i = m + exp(-lambda t_b)(x0_i - m) + (a mean_s z + p (z_i - mean_s z)) [sigma_mix],
 *     a = sqrt(ev1(t_b)), p = sqrt(ev2(t_b)).
 *   est [B,S,T], mix [B,1,T] (raw; needed by the fit only), mix_norm [B,1,T] (needed by DIFFSEP_WARM_MEAN_MIX only), mean, std, t [B]
 *   (device f32; mean / std as diffsep_normalize_batch returns them, one time per utterance), sigma_mix [B,T] for PriorMixSDE and
 *   NULL for MixSDE.  z [B,S,T], or NULL: generated in the kernel, bit for bit draw 0 (stream id 0) of
 *   diffsep_randn_batch(seeds, lengths) when seeds (device [B]) is given, of diffsep_randn(B S T values, seed) otherwise — the draw
 *   the sampler's prior would have used, so that a warm-started sampler call consumes a subset of the full call's draws.
 *   lengths (device int32 [B], nullable): samples at or beyond lengths[b] are never summed and x_init is exactly zero there.
 *   x_init [B,S,T] f32, gains_out [B][S] float64, fallback_out [B] int32: all required.
 * Sums in the fixed order of the library's float64 block reductions, no atomics: every output row of utterance b is bit for bit
 * that of the call on it alone (B = 1, T = n), in any batch, at any padded width, on any stream.  S in 1..3, B in 1..65535,
 * 1 <= T < 2^31.  Refusals (shape, a null required pointer, z together with seeds, sigma_mix against the SDE kind, a workspace
 * below diffsep_warm_start_workspace_bytes(B, S) or not 8-byte aligned with scale = ls) come before the first device call and
 * write nothing.  diffsep_warm_start_workspace_bytes: host arithmetic only; -1 and a message for a refused shape. */
#define DIFFSEP_WARM_SCALE_NONE 0
#define DIFFSEP_WARM_SCALE_LS 1
#define DIFFSEP_WARM_MEAN_MIX 0
#define DIFFSEP_WARM_MEAN_ESTIMATE 1
int64_t diffsep_warm_start_workspace_bytes(int32_t B, int32_t S);
int32_t diffsep_warm_start(const diffsep_sde_config* sde, const float* est, const float* mix, const float* mix_norm,
                           const float* mean, const float* std, const float* t, const float* z, const float* sigma_mix,
                           const int32_t* lengths, const uint64_t* seeds, uint64_t seed, int32_t scale, int32_t mean_from,
                           float* x_init, double* gains_out, int32_t* fallback_out, int32_t B, int32_t S, int64_t T,
                           void* workspace, int64_t workspace_bytes, void* stream);

/* ---- the denoising score-matching loss (forward values only): DiffSepModel.sample_prior (pl_model.py:179-247),
 * compute_score_loss (:411-424), compute_score_loss_init_hack_pit (:370-405), compute_score_loss_with_pit_allthetime
 * (:327-368).  With true_mix = mix / S, mean = (A + exp(-lambda t) Pn) x0 and L the marginal std (times sigma_mix for
 * PriorMixSDE):
 * perturb — sample_prior for init_hack in {false, 1, 2, 3, 4} in one pass:
 *   x_t = beta true_mix + (1 - beta) mean + L z,   z_out = z + (redefine_z ? beta L^-1 (true_mix - mean) : 0)
 *   x0 [B,S,T], mix [B,1,T] (both normalised), t [B], beta [B] (NULL: 0), sigma_mix [B,T] (PriorMixSDE) or NULL;
 *   z [B,S,T], or NULL: Philox draws of the stream (seed, stream_id) laid out as [B,S,T], the bits of diffsep_randn with the
 *   same keys; z_out may be z.  lengths (device int32 [B], nullable): samples at or beyond lengths[b] come out exactly zero.
 *   beta = 0: plain; hack 1: beta = (t >= T - t_rev_init), redefine; hack 2: beta = clamp((t - Tm) / (T - Tm), 0, 1);
 *   hack 3: the same, redefine; hack 4: beta = select (t already set to T there), redefine. */
int32_t diffsep_sde_perturb(const diffsep_sde_config* sde, const float* x0, const float* mix, const float* t, const float* z,
                            const float* sigma_mix, const float* beta, int32_t redefine_z, const int32_t* lengths,
                            uint64_t seed, uint64_t stream_id, float* x_t, float* z_out, int32_t B, int32_t S, int64_t T,
                            void* stream);
/* loss_reduce — out [B][P] float64 = mean over (s, t < lengths[b]) of ((L score)[s,t] + z_p[s,t])^2 (pl_model.py:418-422).
 *   pit_mode DIFFSEP_PIT_NONE: P = 1, z_p = z.  Otherwise P = S!, the source permutations in itertools.permutations order, and
 *   z_p = z + L^-1 (anchor - mean_p), mean_p the marginal mean of x0[:, p, :]; anchor = true_mix (DIFFSEP_PIT_TRUE_MIX,
 *   pl_model.py:383-401) or the mean of the unpermuted target (DIFFSEP_PIT_MEAN0, :347-364).  x0 and mix may be NULL without
 *   PIT.  Per-sample arithmetic in fp32, squares and sums in float64; per-block partial sums in the caller's workspace, then
 *   one finishing block per utterance: row b depends neither on the batch it rides in, nor on the stream, nor on repetition.
 *   best [B] float64 = min over p, argbest [B] int32 (first minimum); coef_out [B][3] float32 = (exp(-lambda t), sqrt(ev1),
 *   sqrt(ev2)) as the kernels use them; all three nullable.  Workspace: diffsep_score_loss_workspace_bytes (host arithmetic
 *   only; -1 and a message for a bad shape). */
#define DIFFSEP_PIT_NONE 0
#define DIFFSEP_PIT_TRUE_MIX 1
#define DIFFSEP_PIT_MEAN0 2
int64_t diffsep_score_loss_workspace_bytes(int32_t B, int32_t S, int64_t T);
int32_t diffsep_score_loss_reduce(const diffsep_sde_config* sde, const float* score, const float* z, const float* x0,
                                  const float* mix, const float* t, const float* sigma_mix, const int32_t* lengths,
                                  int32_t pit_mode, double* out, double* best, int32_t* argbest, float* coef_out, int32_t B,
                                  int32_t S, int64_t T, void* workspace, int64_t workspace_bytes, void* stream);
/* perturb -> one score evaluation on the engine -> loss_reduce, asynchronous on `stream` with no host synchronisation in
 * between: compute_score_loss and the two PIT forms, which here cost ONE network evaluation (every permutation sees the same
 * x_t).  mix_norm [B,1,T], target [B,S,T] (normalised), t [B], beta [B] (nullable), z [B,S,T] or NULL (Philox draws keyed by
 * seed, stream id 0).  lengths_host [B] (nullable) follows the rule of diffsep_sampler_ext: every utterance must have the padded
 * frame count of T, otherwise the call is refused; each row then equals the B = 1 call on that utterance alone (fp32 engine).
 * out [B][P], best / argbest as above; x_t_out, score_out [B,S,T]: nullable debug outputs. */
typedef struct {
  int32_t pit_mode;   /* DIFFSEP_PIT_* */
  int32_t redefine_z; /* the noise redefinition of init_hack 1, 3, 4 (without PIT) */
} diffsep_loss_config;
int32_t diffsep_score_loss(diffsep_engine* e, const diffsep_sde_config* sde, const diffsep_loss_config* cfg,
                           const float* mix_norm, const float* target, const float* t, const float* beta, const float* z,
                           uint64_t seed, const int64_t* lengths_host, double* out, double* best, int32_t* argbest,
                           float* x_t_out, float* score_out, int32_t B, int64_t T, void* workspace, int64_t workspace_bytes,
                           void* stream);
/* The argument checks of the call above that need no GPU (number of sources, pit_mode, lengths against the padded frame count
 * of T, workspace size), from the model configuration alone; the call runs them first. */
int32_t diffsep_score_loss_validate(const diffsep_model_config* cfg, const diffsep_loss_config* loss, int32_t B, int64_t T,
                                    const int64_t* lengths_host, int64_t workspace_bytes);

/* on-device standard normal draws (Philox4x32-10 + Box-Muller); used when noise == NULL. */
int32_t diffsep_randn(float* out, int64_t n, uint64_t seed, uint64_t stream_id, void* stream);
/* the same for a zero-padded batch of utterances with their own seeds and lengths (device arrays [B]): row (b, s) of
 * out [B,S,T] holds values s*len_b .. (s+1)*len_b - 1 of the stream diffsep_randn(seed_b, stream_id) draws, then zeros. */
int32_t diffsep_randn_batch(float* out, int32_t B, int32_t S, int64_t T, const uint64_t* seeds, const int32_t* lengths,
                            uint64_t stream_id, void* stream);

/* float32 <-> engine dtype conversion helper for the tests (n elements); dtype codes DIFFSEP_F32 and DIFFSEP_BF16 (the 16-bit
 * storage format of the build) only, any other is an error. */
int32_t diffsep_convert(const void* src, void* dst, int64_t n, int32_t src_dtype, int32_t dst_dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DIFFSEP_HIP_H */
