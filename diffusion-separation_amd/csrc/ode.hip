// ode.hip — the passes of the probability-flow ODE sampler (reference sdes/__init__.py:193-278: get_ode_sampler, i.e.
// scipy.integrate.solve_ivp(method="RK45" / "RK23") on  dx/dt = f(x,t) - 0.5 g(t)^2 score(x,t,mix), sdes/sdes.py:130-160).
//
// The solver state y / y_new is fp64 (scipy holds its state in float64), the stage derivatives K_j are fp32 (they are the
// network's float32 drift, which is what scipy stores after its float64 round trip), and a stage input is
// fp32(y + (sum_j a_j K_j) h) formed in fp64: the very numbers scipy's rk_step hands the reference's ode_func.
// One thread item = V consecutive time indices of one utterance x all sources (the drift couples the sources through
// their mean): ode_item is what every pass computes for it, with float4 / 2 x double2 accesses when the rows allow it.
// Two kernels walk the items — the whole batch as one system (ode_stage_kernel) and one system per utterance of a
// zero-padded batch (ode_stage_each_kernel) — and share the item body, the block-partials tail and the final tree (both
// in the fixed order of reduce_device.h), so that what an utterance computes is the same code whichever entry it came through.
// A third kernel (ode_expint_each_kernel) is the one pass of the exponential integrators DDIM / DPM-Solver++ 2M, per utterance.
// Contraction is off in this file: every sum and product rounds on its own, like numpy's, so that the stage inputs
// can be reproduced bit for bit in float64 on the host (tests/test_ode_gpu.py).
#include <string.h>

#include <algorithm>

#include "common.h"
#include "reduce_device.h"  // the fixed-order fp64 block totals of the error norms
#include "../../include/diffsep_hip.h"

#pragma clang fp contract(off)

// ------------------------------------------------------------------ loads / stores of V consecutive elements (VEC: V = 4, 16-byte aligned)
template <int V, bool VEC> __device__ inline void ldf(const float* p, float* v) {
  if constexpr (VEC) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
#pragma unroll
    for (int i = 0; i < V; ++i) v[i] = p[i];
  }
}
template <int V, bool VEC> __device__ inline void stf(float* p, const float* v) {
  if constexpr (VEC) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int i = 0; i < V; ++i) p[i] = v[i];
  }
}
template <int V, bool VEC> __device__ inline void ldd(const double* p, double* v) {
  if constexpr (VEC) {
    const double2 q0 = reinterpret_cast<const double2*>(p)[0], q1 = reinterpret_cast<const double2*>(p)[1];
    v[0] = q0.x; v[1] = q0.y; v[2] = q1.x; v[3] = q1.y;
  } else {
#pragma unroll
    for (int i = 0; i < V; ++i) v[i] = p[i];
  }
}
template <int V, bool VEC> __device__ inline void std_(double* p, const double* v) {
  if constexpr (VEC) {
    reinterpret_cast<double2*>(p)[0] = make_double2(v[0], v[1]);
    reinterpret_cast<double2*>(p)[1] = make_double2(v[2], v[3]);
  } else {
#pragma unroll
    for (int i = 0; i < V; ++i) p[i] = v[i];
  }
}

// ------------------------------------------------------------------ the fused pass (see OdeArgs in common.h)
// One item: samples t0 .. t0 + V of utterance b, all sources; the drift at time t_eval, the combination with step size h.
// Mode 3 adds the item's squares to q0, q1.
template <int V, bool VEC>
__device__ inline void ode_item(const OdeArgs& a, int b, long t0, float t_eval, double h, double& q0, double& q1) {
  const int S = a.S;
  const long T = a.T;
  float kd[DS_MAX_SRC][V];
  if (a.kout) {
    // the drift of sde_coeff_kernel (f, g through the same helpers), then rev_f = f - g g score 0.5 in the operation
    // order of sde_reverse_kernel (RSDE.sde with probability_flow = True, sdes/sdes.py:130-160)
    float xv[DS_MAX_SRC][V];
#pragma unroll
    for (int s = 0; s < DS_MAX_SRC; ++s)
      if (s < S) ldf<V, VEC>(a.x + ((long)b * S + s) * T + t0, xv[s]);
    const float g0 = sde_g_of_t(a.s, t_eval);
#pragma unroll
    for (int v = 0; v < V; ++v) {
      float xs[DS_MAX_SRC], f[DS_MAX_SRC];
#pragma unroll
      for (int s = 0; s < DS_MAX_SRC; ++s) xs[s] = s < S ? xv[s][v] : 0.f;
      sde_mix_drift(a.s, xs, f, S);
#pragma unroll
      for (int s = 0; s < DS_MAX_SRC; ++s)
        if (s < S) kd[s][v] = f[s];
    }
#pragma unroll
    for (int s = 0; s < DS_MAX_SRC; ++s) {
      if (s >= S) continue;
      const long o = ((long)b * S + s) * T + t0;
      float sc[V];
      ldf<V, VEC>(a.score + o, sc);
#pragma unroll
      for (int v = 0; v < V; ++v) {
        const float g = a.smix ? g0 * a.smix[(long)b * T + t0 + v] : g0;
        kd[s][v] = kd[s][v] - g * g * sc[v] * 0.5f;
      }
      stf<V, VEC>(a.kout + o, kd[s]);
    }
  }
  if (a.mode == 0) return;
#pragma unroll
  for (int s = 0; s < DS_MAX_SRC; ++s) {
    if (s >= S) continue;
    const long o = ((long)b * S + s) * T + t0;
    double yv[V], acc[V];
    ldd<V, VEC>(a.y + o, yv);
#pragma unroll
    for (int v = 0; v < V; ++v) acc[v] = 0.0;
    for (int j = 0; j < a.nk; ++j) {
      float kv[V];
      if (j == a.kidx) {
#pragma unroll
        for (int v = 0; v < V; ++v) kv[v] = kd[s][v];
      } else {
        ldf<V, VEC>(a.k[j] + o, kv);
      }
      const double cj = a.c[j];
#pragma unroll
      for (int v = 0; v < V; ++v) acc[v] = acc[v] + cj * (double)kv[v];
    }
    if (a.mode == 1) {  // rk_step: fun(t + c h, y + dot(K[:s].T, a[:s]) * h)
      float xo[V];
#pragma unroll
      for (int v = 0; v < V; ++v) xo[v] = (float)(yv[v] + acc[v] * h);
      stf<V, VEC>(a.xo + o, xo);
    } else if (a.mode == 2) {  // rk_step: y_new = y + h * dot(K[:-1].T, B)
      double yn[V];
      float xo[V];
#pragma unroll
      for (int v = 0; v < V; ++v) {
        yn[v] = yv[v] + h * acc[v];
        xo[v] = (float)yn[v];
      }
      std_<V, VEC>(a.yo + o, yn);
      if (a.xo) stf<V, VEC>(a.xo + o, xo);
    } else {  // _estimate_error_norm: norm(dot(K.T, E) * h / (atol + max(|y|, |y_new|) rtol))
      double yn[V];
      if (a.ynew) ldd<V, VEC>(a.ynew + o, yn);
#pragma unroll
      for (int v = 0; v < V; ++v) {
        const double m = a.ynew ? fmax(fabs(yv[v]), fabs(yn[v])) : fabs(yv[v]);
        const double scale = a.atol + m * a.rtol;
        const double d = (acc[v] * h) / scale;
        const double dy = yv[v] / scale;
        q0 = q0 + d * d;
        q1 = q1 + dy * dy;
      }
    }
  }
}

// per-block partials of a mode-3 pass in the fixed order of reduce_device.h (no float atomics) -> part[2 blk + q].
// Every thread of the block calls it.
__device__ inline void ode_block_partials(double q0, double q1, double* part) {
  __shared__ double sh[2][4];
  const double q[2] = {q0, q1};
  const double r = ds_block_totals_d<4, 2>(q, 2, sh);
  if (threadIdx.x < 2) part[2 * blockIdx.x + threadIdx.x] = r;
}

// the final tree of one block over nblk partials: strided sums, then the block total in the same order;
// out[q] = sqrt(sum) / sqrt(n)   (common.norm: ||x||_2 / sqrt(x.size))
__device__ inline void ode_norm_tree(const double* __restrict__ part, int nblk, long n, double* __restrict__ out) {
  __shared__ double sh[2][4];
  double r[2] = {0.0, 0.0};
  for (int i = threadIdx.x; i < nblk; i += 256) { r[0] = r[0] + part[2 * i]; r[1] = r[1] + part[2 * i + 1]; }
  const double s = ds_block_totals_d<4, 2>(r, 2, sh);
  if (threadIdx.x < 2) out[threadIdx.x] = sqrt(s) / sqrt((double)n);
}

// the whole batch as one system: items of all utterances in one sequence, grid-stride over a capped grid
template <int V>
__global__ __launch_bounds__(256) void ode_stage_kernel(OdeArgs a) {
  const long TV = a.T / V;
  const long items = (long)a.B * TV;
  if (a.t_next_out && blockIdx.x == 0)
    for (int i = threadIdx.x; i < a.B; i += 256) a.t_next_out[i] = a.t_next;
  double q0 = 0.0, q1 = 0.0;
  for (long it = (long)blockIdx.x * 256 + threadIdx.x; it < items; it += (long)gridDim.x * 256) {
    const int b = (int)(it / TV);
    ode_item<V, V == 4>(a, b, (it - (long)b * TV) * V, a.tt ? a.tt[b] : a.t, a.h, q0, q1);
  }
  if (a.mode == 3) ode_block_partials(q0, q1, a.part);
}

__global__ __launch_bounds__(256) void ode_norm_final_kernel(const double* __restrict__ part, int nblk, long n,
                                                             double* __restrict__ out) {
  ode_norm_tree(part, nblk, n, out);
}

__global__ __launch_bounds__(256) void ode_cast_kernel(const float* __restrict__ x, double* __restrict__ y, long n) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) y[i] = (double)x[i];
}
__global__ __launch_bounds__(256) void ode_round_kernel(const double* __restrict__ y, float* __restrict__ x, long n) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) x[i] = (float)y[i];
}

static bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
// float4 / double2 accesses: rows of a multiple of 4 samples and every tensor 16-byte aligned
static bool ode_vec(const OdeArgs& a) {
  bool vec = a.T % 4 == 0;
  const void* ps[] = {a.x, a.score, a.kout, a.y, a.ynew, a.yo, a.xo};
  for (const void* p : ps) vec = vec && al16(p);
  for (int j = 0; j < a.nk; ++j) vec = vec && al16(a.k[j]);
  return vec;
}
// what both stage launches ask of their arguments (`who`: "ode" / "ode each" in the message)
static int ode_check(const OdeArgs& a, const char* who) {
  const std::string w(who);
  DS_CHECK(a.S >= 1 && a.S <= DS_MAX_SRC && a.B >= 1 && a.T >= 1, w + ": bad shape");
  DS_CHECK(a.nk >= 0 && a.nk <= DS_ODE_MAX_K && a.kidx < a.nk && (a.kidx < 0 || a.kout), w + ": bad stage combination");
  DS_CHECK(a.mode >= 0 && a.mode <= 3, w + ": bad mode");
  DS_CHECK(!a.kout || (a.x && a.score && (a.tt || a.t > 0.f)), w + ": the drift needs x, t and the score");
  DS_CHECK(a.mode == 0 || a.y, w + ": the stage combination needs y");
  DS_CHECK(a.mode != 1 || a.xo, w + ": stage mode needs x_out");
  DS_CHECK(a.mode != 2 || a.yo, w + ": y_new mode needs y_new_out");
  DS_CHECK(a.mode != 3 || a.part, w + ": error mode needs the partial-sum slab");
  for (int j = 0; j < a.nk; ++j) DS_CHECK(j == a.kidx || a.k[j], w + ": null stage derivative");
  return 0;
}

int ds_launch_ode_stage(const OdeArgs& a, hipStream_t st, int* nblk) {
  if (ode_check(a, "ode")) return 1;
  const bool vec = ode_vec(a);
  const long items = (long)a.B * (a.T / (vec ? 4 : 1));
  const int nb = (int)std::min<long>(cdiv(items, 256), DS_ODE_MAX_BLOCKS);
  if (vec) hipLaunchKernelGGL(ode_stage_kernel<4>, dim3(nb), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(ode_stage_kernel<1>, dim3(nb), dim3(256), 0, st, a);
  DS_LAUNCH_CHECK();
  if (nblk) *nblk = nb;
  return 0;
}
int ds_launch_ode_norm_final(const double* part, int nblk, long n, double* out, hipStream_t st) {
  hipLaunchKernelGGL(ode_norm_final_kernel, dim3(1), dim3(256), 0, st, part, nblk, n, out);
  DS_LAUNCH_CHECK();
  return 0;
}
int ds_launch_ode_cast(const float* x, double* y, long n, hipStream_t st) {
  const int nb = (int)std::min<long>(cdiv(n, 256), 4096);
  hipLaunchKernelGGL(ode_cast_kernel, dim3(nb), dim3(256), 0, st, x, y, n);
  DS_LAUNCH_CHECK();
  return 0;
}
int ds_launch_ode_round(const double* y, float* x, long n, hipStream_t st) {
  const int nb = (int)std::min<long>(cdiv(n, 256), 4096);
  hipLaunchKernelGGL(ode_round_kernel, dim3(nb), dim3(256), 0, st, y, x, n);
  DS_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------ one step controller per utterance
// The same pass on a zero-padded batch of utterances that are B independent ODE systems (diffsep_ode_sample_each): the
// step size, the times, whether the utterance still integrates and its length come from device tables [B].  What utterance
// b computes — every stage input, and the summation tree of its two norms — is what ode_stage_kernel +
// ode_norm_final_kernel compute for it alone (B = 1, T = lens[b]): a thread item is 4 consecutive samples x all sources
// when lens[b] % 4 == 0 and one sample otherwise, nb = min(cdiv(items, 256), DS_ODE_MAX_BLOCKS) blocks of the row's grid
// stride over the items with a stride of nb * 256, and the partials are reduced in the same order.  None of that depends
// on B, b or the padded T; rows that are not 16-byte aligned (T % 4 != 0) keep the item shape and load by element.

// the items of utterance b that block blockIdx.x of its nb blocks owns, with the utterance's own t and h
template <int V, bool VEC>
__device__ inline void ode_each_items(const OdeEachArgs& e, int b, long len, long nb, double& q0, double& q1) {
  const OdeArgs& a = e.a;
  const float t_eval = a.kout ? a.tt[b] : 0.f;
  const double h = a.mode ? e.h[b] : 0.0;
  for (long it = (long)blockIdx.x * 256 + threadIdx.x; it < len / V; it += nb * 256)
    ode_item<V, VEC>(a, b, it * V, t_eval, h, q0, q1);
}

// blocks of an utterance's row of the grid that its summation tree needs: min(cdiv(items, 256), DS_ODE_MAX_BLOCKS)
__device__ inline long ode_each_blocks(long len) {
  const long items = len % 4 == 0 ? len / 4 : len;
  const long nb = (items + 255) / 256;
  return nb < DS_ODE_MAX_BLOCKS ? nb : DS_ODE_MAX_BLOCKS;
}

// grid (min(cdiv(T, 256), DS_ODE_MAX_BLOCKS), B): row b of the grid is utterance b; vec: ode_vec of the padded batch
__global__ __launch_bounds__(256) void ode_stage_each_kernel(OdeEachArgs e, int vec) {
  const OdeArgs& a = e.a;
  const int b = blockIdx.y;
  if (!e.active[b]) return;
  const int S = a.S;
  const long T = a.T, len = e.lens[b];
  if (len < 1 || len > T) return;  // (the drivers check the lengths on the host; a bad table entry touches nothing)
  if (e.tnext && blockIdx.x == 0 && threadIdx.x == 0) a.t_next_out[b] = e.tnext[b];
  const long nb = ode_each_blocks(len);
  double q0 = 0.0, q1 = 0.0;
  if (blockIdx.x < nb) {
    if (len % 4 != 0) ode_each_items<1, false>(e, b, len, nb, q0, q1);
    else if (vec) ode_each_items<4, true>(e, b, len, nb, q0, q1);
    else ode_each_items<4, false>(e, b, len, nb, q0, q1);
  }
  // the zero tail of what this pass writes (every block of the row)
  const long tail = T - len;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < tail * S; i += (long)gridDim.x * 256) {
    const int s = (int)(i / tail);
    const long o = ((long)b * S + s) * T + len + (i - (long)s * tail);
    if (a.kout) a.kout[o] = 0.f;
    if ((a.mode == 1 || a.mode == 2) && a.xo) a.xo[o] = 0.f;
    if (a.mode == 2) a.yo[o] = 0.0;
  }
  if (a.mode == 3 && blockIdx.x < nb) ode_block_partials(q0, q1, a.part + (long)b * 2 * DS_ODE_MAX_BLOCKS);
}

// grid (B): the final tree on the slab of utterance b with its own block count and n = S lens[b]
__global__ __launch_bounds__(256) void ode_norm_final_each_kernel(const double* __restrict__ part_all,
                                                                  const int* __restrict__ lens,
                                                                  const int* __restrict__ active, int S,
                                                                  double* __restrict__ norms) {
  const int b = blockIdx.x;
  if (!active[b]) return;
  const long len = lens[b];
  if (len < 1) return;
  ode_norm_tree(part_all + (long)b * 2 * DS_ODE_MAX_BLOCKS, (int)ode_each_blocks(len), (long)S * len, norms + 2 * b);
}

// grid (x, B): the accepted utterances take their step (whole rows: the tails of y_new and K[ns] are zero like those of y, K[0])
__global__ __launch_bounds__(256) void ode_commit_each_kernel(double* __restrict__ y, const double* __restrict__ ynew,
                                                              float* __restrict__ k0, const float* __restrict__ kns,
                                                              const double* __restrict__ norms,
                                                              const int* __restrict__ active, long n) {
  const int b = blockIdx.y;
  if (!active[b] || !(norms[2 * b] < 1.0)) return;
  const long o = (long)b * n;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    y[o + i] = ynew[o + i];
    k0[o + i] = kns[o + i];
  }
}

int ds_launch_ode_stage_each(const OdeEachArgs& e, hipStream_t st) {
  const OdeArgs& a = e.a;
  if (ode_check(a, "ode each")) return 1;
  DS_CHECK(a.B <= 65535 && a.T <= 0x7fffffffL, "ode each: bad shape");
  DS_CHECK(e.active && e.lens && (a.mode == 0 || e.h), "ode each: the tables h, active and lengths are needed");
  DS_CHECK(!a.kout || a.tt, "ode each: the drift needs x, t [B] and the score");
  DS_CHECK(!e.tnext || a.t_next_out, "ode each: t_next needs its output");
  const int nb = (int)std::min<long>(cdiv(a.T, 256), DS_ODE_MAX_BLOCKS);
  hipLaunchKernelGGL(ode_stage_each_kernel, dim3(nb, a.B), dim3(256), 0, st, e, ode_vec(a) ? 1 : 0);
  DS_LAUNCH_CHECK();
  return 0;
}
int ds_launch_ode_norm_final_each(const double* part, const int* lens, const int* active, int B, int S, double* norms,
                                  hipStream_t st) {
  hipLaunchKernelGGL(ode_norm_final_each_kernel, dim3(B), dim3(256), 0, st, part, lens, active, S, norms);
  DS_LAUNCH_CHECK();
  return 0;
}
int ds_launch_ode_commit_each(double* y, const double* ynew, float* k0, const float* kns, const double* norms,
                              const int* active, int B, int S, long T, hipStream_t st) {
  const long n = (long)S * T;
  const int nb = (int)std::min<long>(cdiv(n, 256), 1024);
  hipLaunchKernelGGL(ode_commit_each_kernel, dim3(nb, B), dim3(256), 0, st, y, ynew, k0, kns, norms, active, n);
  DS_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------ exponential integrators: one step of DDIM / DPM-Solver++ 2M
// The pass after the network evaluation at t_i (diffsep_ode_sample_expint): data prediction and step in one sweep, 40 bytes per
// element (y, X0_prev and the score in; X0, y' and fp32(y') out).  Per time sample, in float64, every sum and product rounded on
// its own (contraction is off), in exactly this order — sums over the sources run s = 0, 1, ... and are then divided by S:
//   mx = (sum_s y_s) / S,  ms = (sum_s (double) score_s) / S,  mp = (sum_s X0p_s) / S
//   q = (double) sigma_mix * (double) sigma_mix  (1 without sigma_mix),  eA = ev_A * q,  eP = ev_P * q
//   xa = (mx + eA * ms) / alpha_A
//   X0_s = xa + ((y_s - mx) + eP * ((double) score_s - ms)) / alpha_P
//   mn = (sum_s X0_s) / S
//   dA = w0_A * mn [+ w1_A * mp],  ya = cx_A * mx + cd_A * dA
//   dP_s = w0_P * (X0_s - mn) [+ w1_P * (X0p_s - mp)]
//   y'_s = ya + (cx_P * (y_s - mx) + cd_P * dP_s)
// ([...]: with a previous X0 only), and for the trace  d_s = ga * (mn - mp) + gp * ((X0_s - mn) - (X0p_s - mp))  (0 without a
// previous X0), q0 += d_s^2, q1 += y_s^2 over the item's samples v = 0 .. V, sources innermost.
template <int V, bool VEC>
__device__ inline void expint_item(const ExpintArgs& a, int b, long t0, double& q0, double& q1) {
  const int S = a.S;
  const long T = a.T;
  const bool prev = a.x0p != nullptr;
  double yv[DS_MAX_SRC][V], pv[DS_MAX_SRC][V];
  float sv[DS_MAX_SRC][V], smv[V];
#pragma unroll
  for (int s = 0; s < DS_MAX_SRC; ++s) {
    if (s >= S) continue;
    const long o = ((long)b * S + s) * T + t0;
    ldd<V, VEC>(a.y + o, yv[s]);
    ldf<V, VEC>(a.score + o, sv[s]);
    if (prev) ldd<V, VEC>(a.x0p + o, pv[s]);
  }
  if (a.smix) ldf<V, VEC>(a.smix + (long)b * T + t0, smv);
  const double dS = (double)S;
  const double* c = a.c;
#pragma unroll
  for (int v = 0; v < V; ++v) {
    double mx = 0.0, ms = 0.0, mp = 0.0;
#pragma unroll
    for (int s = 0; s < DS_MAX_SRC; ++s) {
      if (s >= S) continue;
      mx = mx + yv[s][v];
      ms = ms + (double)sv[s][v];
      if (prev) mp = mp + pv[s][v];
    }
    mx = mx / dS;
    ms = ms / dS;
    mp = mp / dS;
    double q = 1.0;
    if (a.smix) q = (double)smv[v] * (double)smv[v];
    const double eA = c[DS_EI_EV_A] * q, eP = c[DS_EI_EV_P] * q;
    const double xa = (mx + eA * ms) / c[DS_EI_AL_A];
    double x0[DS_MAX_SRC], mn = 0.0;
#pragma unroll
    for (int s = 0; s < DS_MAX_SRC; ++s) {
      if (s >= S) continue;
      x0[s] = xa + ((yv[s][v] - mx) + eP * ((double)sv[s][v] - ms)) / c[DS_EI_AL_P];
      mn = mn + x0[s];
    }
    mn = mn / dS;
    double dA = c[DS_EI_W0_A] * mn;
    if (prev) dA = dA + c[DS_EI_W1_A] * mp;
    const double ya = c[DS_EI_CX_A] * mx + c[DS_EI_CD_A] * dA;
#pragma unroll
    for (int s = 0; s < DS_MAX_SRC; ++s) {
      if (s >= S) continue;
      double dP = c[DS_EI_W0_P] * (x0[s] - mn);
      if (prev) dP = dP + c[DS_EI_W1_P] * (pv[s][v] - mp);
      const double yn = ya + (c[DS_EI_CX_P] * (yv[s][v] - mx) + c[DS_EI_CD_P] * dP);
      if (a.part) {
        const double d = prev ? a.ga * (mn - mp) + a.gp * ((x0[s] - mn) - (pv[s][v] - mp)) : 0.0;
        q0 = q0 + d * d;
        q1 = q1 + yv[s][v] * yv[s][v];
      }
      pv[s][v] = x0[s];
      yv[s][v] = yn;
      sv[s][v] = (float)yn;
    }
  }
#pragma unroll
  for (int s = 0; s < DS_MAX_SRC; ++s) {
    if (s >= S) continue;
    const long o = ((long)b * S + s) * T + t0;
    std_<V, VEC>(a.x0o + o, pv[s]);
    std_<V, VEC>(a.yo + o, yv[s]);
    stf<V, VEC>(a.xo + o, sv[s]);
  }
}

template <int V, bool VEC>
__device__ inline void expint_each_items(const ExpintArgs& a, int b, long len, long nb, double& q0, double& q1) {
  for (long it = (long)blockIdx.x * 256 + threadIdx.x; it < len / V; it += nb * 256) expint_item<V, VEC>(a, b, it * V, q0, q1);
}

// grid (min(cdiv(T, 256), DS_ODE_MAX_BLOCKS), B): row b of the grid is utterance b, walked as ode_stage_each_kernel walks it
// (the same items, blocks and partial-sum tree per utterance, whatever B, b and the padded T are); vec: expint_vec
__global__ __launch_bounds__(256) void ode_expint_each_kernel(ExpintArgs a, int vec) {
  const int b = blockIdx.y;
  if (!a.active[b]) return;
  const int S = a.S;
  const long T = a.T, len = a.lens[b];
  if (len < 1 || len > T) return;  // (the driver checks the lengths on the host; a bad table entry touches nothing)
  if (a.tnext && blockIdx.x == 0 && threadIdx.x == 0) a.t_next_out[b] = a.tnext[b];
  const long nb = ode_each_blocks(len);
  double q0 = 0.0, q1 = 0.0;
  if (blockIdx.x < nb) {
    if (len % 4 != 0) expint_each_items<1, false>(a, b, len, nb, q0, q1);
    else if (vec) expint_each_items<4, true>(a, b, len, nb, q0, q1);
    else expint_each_items<4, false>(a, b, len, nb, q0, q1);
  }
  // the zero tail of the three outputs (every block of the row)
  const long tail = T - len;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < tail * S; i += (long)gridDim.x * 256) {
    const int s = (int)(i / tail);
    const long o = ((long)b * S + s) * T + len + (i - (long)s * tail);
    a.x0o[o] = 0.0;
    a.yo[o] = 0.0;
    a.xo[o] = 0.f;
  }
  if (a.part && blockIdx.x < nb) ode_block_partials(q0, q1, a.part + (long)b * 2 * DS_ODE_MAX_BLOCKS);
}

// float4 / double2 accesses: rows of a multiple of 4 samples and every tensor 16-byte aligned
static bool expint_vec(const ExpintArgs& a) {
  bool vec = a.T % 4 == 0;
  const void* ps[] = {a.y, a.score, a.smix, a.x0p, a.x0o, a.yo, a.xo};
  for (const void* p : ps) vec = vec && al16(p);
  return vec;
}

int ds_launch_ode_expint_each(const ExpintArgs& a, hipStream_t st) {
  DS_CHECK(a.S >= 1 && a.S <= DS_MAX_SRC && a.B >= 1 && a.B <= 65535 && a.T >= 1 && a.T <= 0x7fffffffL, "expint each: bad shape");
  DS_CHECK(a.y && a.score && a.x0o && a.yo && a.xo, "expint each: y, the score and the three outputs are needed");
  DS_CHECK(a.active && a.lens, "expint each: the tables active and lengths are needed");
  DS_CHECK(!a.tnext || a.t_next_out, "expint each: t_next needs its output");
  DS_CHECK((const double*)a.x0o != a.x0p && (const double*)a.x0o != a.y && (const double*)a.yo != a.y &&
               (const double*)a.yo != a.x0p && a.x0o != a.yo,
           "expint each: an output aliases an input or another output");
  DS_CHECK(a.c[DS_EI_AL_A] > 0.0 && a.c[DS_EI_AL_P] > 0.0, "expint each: bad coefficient row (alpha <= 0)");
  const int nb = (int)std::min<long>(cdiv(a.T, 256), DS_ODE_MAX_BLOCKS);
  hipLaunchKernelGGL(ode_expint_each_kernel, dim3(nb, a.B), dim3(256), 0, st, a, expint_vec(a) ? 1 : 0);
  DS_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------ C-ABI: tableau + unit entry points
extern "C" int32_t diffsep_expint_coefficients(const diffsep_sde_config* sde, int32_t method, int32_t steps, double t_start,
                                               double eps, const double* timesteps_host, double* coef_out) {
  DS_CHECK(sde && coef_out, "expint_coefficients: null argument");
  const OdeExpintConfig oc{method, steps, t_start, eps, 0, 0};
  OdeExpintPlan plan;
  const std::string bad = ode_expint_plan_fill(plan, oc, *sde, timesteps_host, false, "expint_coefficients");
  DS_CHECK(bad.empty(), bad);
  memcpy(coef_out, plan.coef.data(), plan.coef.size() * sizeof(double));
  return 0;
}

extern "C" int32_t diffsep_expint_update_each(const diffsep_sde_config* sde, const double* y, const float* score,
                                              const float* sigma_mix, const double* x0_prev, const double* coef,
                                              const int32_t* active, const int32_t* lengths, double* x0_out,
                                              double* y_new_out, float* x_out, double* norms_out, int32_t B, int32_t S,
                                              int64_t T, void* workspace, int64_t workspace_bytes, void* stream) {
  DS_CHECK(sde && coef, "expint_update_each: null argument");
  DS_CHECK((sde->kind == DIFFSEP_SDE_PRIORMIX) == (sigma_mix != nullptr),
           "expint_update_each: PriorMixSDE with sigma_mix, MixSDE without");
  DS_CHECK(!norms_out || (workspace && B >= 1 && workspace_bytes >= (int64_t)B * DIFFSEP_ODE_WORKSPACE_BYTES),
           "expint_update_each: norms_out needs a workspace >= B * DIFFSEP_ODE_WORKSPACE_BYTES");
  ExpintArgs a;
  memset(&a, 0, sizeof(a));
  a.y = y; a.score = score; a.smix = sigma_mix; a.x0p = x0_prev;
  a.x0o = x0_out; a.yo = y_new_out; a.xo = x_out;
  ds_expint_set_coef(a, coef);
  a.part = norms_out ? (double*)workspace : nullptr;
  a.active = active; a.lens = lengths;
  a.B = B; a.S = S; a.T = T;
  if (ds_launch_ode_expint_each(a, (hipStream_t)stream)) return 1;
  if (norms_out) return ds_launch_ode_norm_final_each(a.part, lengths, active, B, S, norms_out, (hipStream_t)stream);
  return 0;
}

extern "C" int32_t diffsep_ode_tableau(int32_t method, double* A, double* B, double* C, double* E, int32_t* n_stages,
                                       int32_t* error_order) {
  int ns = 0, eo = 0;
  DS_CHECK(ds_ode_tableau(method, A, B, C, E, &ns, &eo) == 0, "ode_tableau: method must be RK45 (0) or RK23 (1)");
  if (n_stages) *n_stages = ns;
  if (error_order) *error_order = eo;
  return 0;
}

static int unit_args(OdeArgs& a, const diffsep_sde_config* sde, const float* x, const float* t, const float* score,
                     const float* sigma_mix, const double* y, const float* const* K, const double* coef, int32_t n_k,
                     int32_t k_out, double h, int32_t B, int32_t S, int64_t T) {
  DS_CHECK(n_k >= 0 && n_k <= DS_ODE_MAX_K && k_out < DS_ODE_MAX_K && (n_k == 0 || (K && coef)) &&
               (k_out < 0 || (K && K[k_out])),
           "ode unit: bad stage list");
  memset(&a, 0, sizeof(a));
  if (sde) a.s = SdeP{sde->kind, sde->ndim, sde->d_lambda, sde->sigma_min, sde->sigma_max};
  DS_CHECK(k_out < 0 || (sde && (sde->kind == 1) == (sigma_mix != nullptr)),
           "ode unit: the drift needs the SDE (PriorMixSDE with sigma_mix, MixSDE without)");
  a.x = x; a.score = score; a.tt = t; a.smix = sigma_mix;
  a.kout = k_out >= 0 ? const_cast<float*>(K[k_out]) : nullptr;
  a.kidx = k_out < n_k ? k_out : -1;
  a.nk = n_k;
  for (int j = 0; j < n_k; ++j) { a.k[j] = K[j]; a.c[j] = coef[j]; }
  a.h = h; a.y = y; a.B = B; a.S = S; a.T = T;
  return 0;
}

extern "C" int32_t diffsep_ode_stage_update(const diffsep_sde_config* sde, const float* x, const float* t,
                                            const float* score, const float* sigma_mix, const double* y,
                                            float* const* K, const double* coef, int32_t n_k, int32_t k_out, double h,
                                            float* x_out, double* y_new_out, int32_t B, int32_t S, int64_t T,
                                            void* stream) {
  OdeArgs a;
  if (unit_args(a, sde, x, t, score, sigma_mix, y, K, coef, n_k, k_out, h, B, S, T)) return 1;
  DS_CHECK(k_out < 0 || t, "ode_stage_update: null t");
  a.mode = n_k == 0 ? 0 : (y_new_out ? 2 : 1);
  a.xo = x_out; a.yo = y_new_out;
  return ds_launch_ode_stage(a, (hipStream_t)stream);
}

extern "C" int32_t diffsep_ode_error_norm(const diffsep_sde_config* sde, const float* x, const float* t,
                                          const float* score, const float* sigma_mix, const double* y,
                                          const double* y_new, float* const* K, const double* coef, int32_t n_k,
                                          int32_t k_out, double h, double rtol, double atol, double* norms_out,
                                          int32_t B, int32_t S, int64_t T, void* workspace, int64_t workspace_bytes,
                                          void* stream) {
  OdeArgs a;
  if (unit_args(a, sde, x, t, score, sigma_mix, y, K, coef, n_k, k_out, h, B, S, T)) return 1;
  DS_CHECK(k_out < 0 || t, "ode_error_norm: null t");
  DS_CHECK(norms_out && workspace && workspace_bytes >= DIFFSEP_ODE_WORKSPACE_BYTES && n_k >= 1,
           "ode_error_norm: bad argument (workspace >= DIFFSEP_ODE_WORKSPACE_BYTES)");
  a.mode = 3;
  a.ynew = y_new; a.rtol = rtol; a.atol = atol; a.part = (double*)workspace;
  int nb = 0;
  if (ds_launch_ode_stage(a, (hipStream_t)stream, &nb)) return 1;
  return ds_launch_ode_norm_final(a.part, nb, (long)B * S * T, norms_out, (hipStream_t)stream);
}

// the per-utterance passes (h, active, lengths: device tables [B]); see ds_launch_ode_stage_each
static int unit_each(OdeEachArgs& e, const double* h, const int32_t* active, const int32_t* lengths, const char* who) {
  DS_CHECK(h && active && lengths, std::string(who) + ": null table (h, active, lengths are device arrays [B])");
  e.h = h; e.active = active; e.lens = lengths; e.tnext = nullptr;
  return 0;
}

extern "C" int32_t diffsep_ode_stage_update_each(const diffsep_sde_config* sde, const float* x, const float* t,
                                                 const float* score, const float* sigma_mix, const double* y,
                                                 float* const* K, const double* coef, int32_t n_k, int32_t k_out,
                                                 const double* h, const int32_t* active, const int32_t* lengths,
                                                 float* x_out, double* y_new_out, int32_t B, int32_t S, int64_t T,
                                                 void* stream) {
  OdeEachArgs e;
  if (unit_args(e.a, sde, x, t, score, sigma_mix, y, K, coef, n_k, k_out, 0.0, B, S, T)) return 1;
  if (unit_each(e, h, active, lengths, "ode_stage_update_each")) return 1;
  DS_CHECK(k_out < 0 || t, "ode_stage_update_each: null t");
  e.a.mode = n_k == 0 ? 0 : (y_new_out ? 2 : 1);
  e.a.xo = x_out; e.a.yo = y_new_out;
  return ds_launch_ode_stage_each(e, (hipStream_t)stream);
}

extern "C" int32_t diffsep_ode_error_norm_each(const diffsep_sde_config* sde, const float* x, const float* t,
                                               const float* score, const float* sigma_mix, const double* y,
                                               const double* y_new, float* const* K, const double* coef, int32_t n_k,
                                               int32_t k_out, const double* h, const int32_t* active,
                                               const int32_t* lengths, double rtol, double atol, double* norms_out,
                                               int32_t B, int32_t S, int64_t T, void* workspace,
                                               int64_t workspace_bytes, void* stream) {
  OdeEachArgs e;
  if (unit_args(e.a, sde, x, t, score, sigma_mix, y, K, coef, n_k, k_out, 0.0, B, S, T)) return 1;
  if (unit_each(e, h, active, lengths, "ode_error_norm_each")) return 1;
  DS_CHECK(k_out < 0 || t, "ode_error_norm_each: null t");
  DS_CHECK(norms_out && workspace && B >= 1 && workspace_bytes >= (int64_t)B * DIFFSEP_ODE_WORKSPACE_BYTES && n_k >= 1,
           "ode_error_norm_each: bad argument (workspace >= B * DIFFSEP_ODE_WORKSPACE_BYTES)");
  e.a.mode = 3;
  e.a.ynew = y_new; e.a.rtol = rtol; e.a.atol = atol; e.a.part = (double*)workspace;
  if (ds_launch_ode_stage_each(e, (hipStream_t)stream)) return 1;
  return ds_launch_ode_norm_final_each(e.a.part, lengths, active, B, S, norms_out, (hipStream_t)stream);
}
