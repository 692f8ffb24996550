// engine_host.h — private to the engine's host sources (arch.hip, engine.hip, sampler.hip, unit.hip): the architecture
// description, the engine struct and the few helpers that more than one of them calls.  Nothing here is part of the C-ABI.
#pragma once
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "../../include/diffsep_hip.h"
#include "common.h"

#pragma GCC visibility push(hidden)  // (C++ names that carry a diffsep_ type stay out of the libraries' dynamic symbol table)

// ------------------------------------------------------------------ architecture description (arch.hip)
struct PRef { long off = -1; long numel = 0; };  // into the flat fp32 blob
struct ParamInfo { std::string name; int ndim; int64_t shape[4]; long off; };

enum ModKind { MK_FOURIER, MK_LINEAR, MK_CONV3, MK_RES, MK_ATTN, MK_COMBINE, MK_GN };

struct Module {
  ModKind kind;
  int in_ch = 0, out_ch = 0;
  int in_c1 = 0;  // residual blocks of the up path read an in-place concat: channels of its first source (0 = none)
  bool up = false, down = false, has_conv2 = false;
  int temb_off = 0;  // offset of this block's Dense_0 output inside the concatenated projection
  // fp32 parameter references
  PRef w0, b0;        // Fourier W / Linear / Conv (3x3 or 1x1) / GN gamma,beta
  PRef gn0_w, gn0_b, conv0_w, conv0_b, dense_w, dense_b, gn1_w, gn1_b, conv1_w, conv1_b, conv2_w, conv2_b;
  PRef nin_w[4], nin_b[4];
  // packed (engine dtype) weight offsets in elements
  long pk0 = -1, pk1 = -1, pk2 = -1, pk_nin[4] = {-1, -1, -1, -1};
  // second copies of Conv_0 / Conv_1 / Conv_2 in the register-weight kernel's fragment-major order (16-bit engines, the shapes
  // that kernel takes: ds_rw_frag_shape), -1 = none
  long pf0 = -1, pf1 = -1, pf2 = -1;
  // split engines: the copies are hi / lo plane pairs (ds_sws_frag_index); pf_id = that copy of the identity matrix, which the
  // residual of a block without Conv_2 meets as a folded skip (conv3x3_sws.hip)
  long pf_id = -1;
  // cat(128, 128) -> 128 blocks whose convolutions run as two 128-channel launches (res_block): fragment-major copies of the
  // two halves of Conv_0, of the first half of Conv_2, and the second half of Conv_2 packed for a stand-alone 1x1 launch
  long pf0a = -1, pf0b = -1, pf2a = -1, pk2b = -1;
  // attention block, fused kernel (attn_fused.hip; 128 channels only): fragment-major copies [0] = Wk^T Wq (query and key
  // projections folded at engine creation), [2] = Wv, [3] = Wo; ab_off = this block's Wk^T b_q in the engine's d_attn_b
  long pf_nin[4] = {-1, -1, -1, -1};
  long ab_off = -1;
};

struct Arch {
  std::vector<Module> mods;
  std::vector<ParamInfo> params;
  PRef out_w, out_b;
  long pk_out = -1;
  long total = 0;       // floats in the blob
  long pack_total = 0;  // elements in the packed weight buffer
  int dense_total = 0;  // sum of out_ch over residual blocks
  long attn_bias_total = 0;  // floats of folded attention biases (Module::ab_off)
  int chan_in = 0, chan_out = 0, cpad_in = 0, cpad_out = 0;
};

static inline int rup8(int c) { return (c + 7) & ~7; }

struct ArchBuilder {
  Arch& A;
  // which fragment-major weight copies get a slot in the pack buffer: bit 0 = the shapes of the 16-bit kernels (conv3x3_rw / _sw,
  // the fused attention block), bit 1 = the shapes of the split-precision kernel (conv3x3_sws).  An exact-fp32 engine reads none
  // of them (0); the unit entry points build their one-module engines with every copy (3).
  int frag;
  explicit ArchBuilder(Arch& a, int frag_mask = 3) : A(a), frag(frag_mask) {}
  bool frag_wanted(int taps, int cin, int cout) const {
    return ((frag & 1) && (ds_rw_frag_shape(taps, cin, cout) || ds_sw_frag_shape(taps, cin, cout))) ||
           ((frag & 2) && ds_sws_frag_shape(taps, cin, cout));
  }
  PRef add(const std::string& name, std::initializer_list<int64_t> shp) {
    ParamInfo p;
    p.name = name;
    p.ndim = (int)shp.size();
    long n = 1;
    int i = 0;
    for (auto s : shp) { p.shape[i++] = s; n *= s; }
    for (; i < 4; ++i) p.shape[i] = 1;
    p.off = A.total;
    A.params.push_back(p);
    PRef r;
    r.off = A.total;
    r.numel = n;
    A.total += n;
    return r;
  }
  long pack(long o, int taps, int cin) {
    long r = A.pack_total;
    A.pack_total += o * taps * (long)rup8(cin);
    A.pack_total = (A.pack_total + 63) & ~63L;
    return r;
  }
  std::string pfx() const { return "all_modules." + std::to_string(A.mods.size()) + "."; }
  void fourier(int nf) {
    Module m; m.kind = MK_FOURIER; m.out_ch = nf;
    m.w0 = add(pfx() + "W", {nf});
    A.mods.push_back(m);
  }
  void linear(int in, int out) {
    Module m; m.kind = MK_LINEAR; m.in_ch = in; m.out_ch = out;
    m.w0 = add(pfx() + "weight", {out, in});
    m.b0 = add(pfx() + "bias", {out});
    A.mods.push_back(m);
  }
  void conv3(int in, int out) {
    Module m; m.kind = MK_CONV3; m.in_ch = in; m.out_ch = out;
    m.w0 = add(pfx() + "weight", {out, in, 3, 3});
    m.b0 = add(pfx() + "bias", {out});
    m.pk0 = pack(out, 9, in);
    A.mods.push_back(m);
  }
  void gn(int c) {
    Module m; m.kind = MK_GN; m.in_ch = m.out_ch = c;
    m.w0 = add(pfx() + "weight", {c});
    m.b0 = add(pfx() + "bias", {c});
    A.mods.push_back(m);
  }
  void res(int in, int out, bool up, bool down, int temb_dim, int in_c1 = 0) {
    Module m; m.kind = MK_RES; m.in_ch = in; m.out_ch = out; m.up = up; m.down = down; m.in_c1 = in_c1;
    const std::string p = pfx();
    m.gn0_w = add(p + "GroupNorm_0.weight", {in});
    m.gn0_b = add(p + "GroupNorm_0.bias", {in});
    m.conv0_w = add(p + "Conv_0.weight", {out, in, 3, 3});
    m.conv0_b = add(p + "Conv_0.bias", {out});
    m.dense_w = add(p + "Dense_0.weight", {out, temb_dim});
    m.dense_b = add(p + "Dense_0.bias", {out});
    m.gn1_w = add(p + "GroupNorm_1.weight", {out});
    m.gn1_b = add(p + "GroupNorm_1.bias", {out});
    m.conv1_w = add(p + "Conv_1.weight", {out, out, 3, 3});
    m.conv1_b = add(p + "Conv_1.bias", {out});
    m.has_conv2 = (in != out) || up || down;
    if (m.has_conv2) {
      m.conv2_w = add(p + "Conv_2.weight", {out, in, 1, 1});
      m.conv2_b = add(p + "Conv_2.bias", {out});
      m.pk2 = pack(out, 1, in);
    }
    m.pk0 = pack(out, 9, in);
    m.pk1 = pack(out, 9, out);
    if (frag_wanted(9, in, out)) m.pf0 = pack(out, 9, in);
    if (frag_wanted(9, out, out)) m.pf1 = pack(out, 9, out);
    if (m.has_conv2 && frag_wanted(1, in, out)) m.pf2 = pack(out, 1, in);
    if (!m.has_conv2 && (((frag & 2) && ds_sws_frag_shape(1, out, out)) || ((frag & 1) && ds_sw_frag_shape(1, out, out))))
      m.pf_id = pack(out, 1, out);
    if ((frag & 1) && in == 256 && in_c1 == 128 && out == 128 && !up && !down) {
      m.pf0a = pack(out, 9, 128); m.pf0b = pack(out, 9, 128); m.pf2a = pack(out, 1, 128); m.pk2b = pack(out, 1, 128);
    }
    m.temb_off = A.dense_total;
    A.dense_total += out;
    A.mods.push_back(m);
  }
  void attn(int c) {
    Module m; m.kind = MK_ATTN; m.in_ch = m.out_ch = c;
    const std::string p = pfx();
    m.gn0_w = add(p + "GroupNorm_0.weight", {c});
    m.gn0_b = add(p + "GroupNorm_0.bias", {c});
    for (int i = 0; i < 4; ++i) {
      m.nin_w[i] = add(p + "NIN_" + std::to_string(i) + ".W", {c, c});
      m.nin_b[i] = add(p + "NIN_" + std::to_string(i) + ".b", {c});
      m.pk_nin[i] = pack(c, 1, c);
      if ((frag & 1) && c == 128 && i != 1) m.pf_nin[i] = pack(c, 1, c);
    }
    if (c == 128) { m.ab_off = A.attn_bias_total; A.attn_bias_total += c; }
    A.mods.push_back(m);
  }
  void combine(int d1, int d2) {
    Module m; m.kind = MK_COMBINE; m.in_ch = d1; m.out_ch = d2;
    const std::string p = pfx();
    m.w0 = add(p + "Conv_0.weight", {d2, d1, 1, 1});
    m.b0 = add(p + "Conv_0.bias", {d2});
    m.pk0 = pack(d2, 1, d1);
    A.mods.push_back(m);
  }
};
int build_arch(const diffsep_model_config& c, Arch& A, int frag_mask = 3);

// Which weights the engine keeps chunk-major: every conv whose input channels are a multiple of 64 and whose concat
// split (c1 channels from the first source, 0 = no concat) falls on a chunk boundary
static inline int weight_chunk(int taps, int cin, int c1, int dtype) {
  const int kc = ds_conv_chunk(taps, dtype);
  return (cin % 64 == 0 && c1 % kc == 0) ? kc : 0;
}
// Conv_2 of a block is folded into its second 3x3 convolution when that one runs on a 64-cout tile
static inline bool fuse_skip(const Module& m) { return m.has_conv2 && m.out_ch > 32; }
// boundary dtype -> the storage type the kernels see + the split flag (DS_F32_SPLIT: fp32 tensors, bf16x3 MFMA products)
struct DtypeSplit { int dtype, split; };
static inline DtypeSplit split_dtype(int boundary) {
  return {boundary == DS_F32_SPLIT ? DS_F32 : boundary, boundary == DS_F32_SPLIT ? 1 : 0};
}
// GroupNorm(num_groups = min(C / 4, 32)) and the reciprocal of one group's element count over npix pixels
static inline int gn_group_count(int C) { return (C / 4 < 32) ? C / 4 : 32; }
static inline float gn_inv_count(long npix, int C, int groups) { return (float)(1.0 / ((double)npix * (C / groups))); }
static inline SdeP to_sdep(const diffsep_sde_config* s) { return SdeP{s->kind, s->ndim, s->d_lambda, s->sigma_min, s->sigma_max}; }

// ------------------------------------------------------------------ engine
struct Tn {  // NHWC view; optionally the in-place channel concat of two tensors (C1 channels from p, rest from p2)
  void* p = nullptr;
  int C = 0, ld = 0, H = 0, W = 0;
  void* p2 = nullptr;
  int C1 = 0, ld2 = 0;
  // channel-sum accumulators filled by the producing conv ([B][C][2] fixed-point int64, common.h), or null
  long long* sa = nullptr;
  long long* sa2 = nullptr;
};
// the tensor part of a launch description: every batch stride is that of a dense [H][W][ld] image
static inline long image_bs(const Tn& t, int ld) { return (long)t.H * t.W * ld; }
static inline void conv_input(ConvArgs& a, const Tn& x) {  // (+ the problem's H, W, Cin)
  a.x = x.p; a.x_bs = image_bs(x, x.ld); a.ldx = x.ld;
  a.x2 = x.p2; a.x2_bs = image_bs(x, x.ld2); a.ldx2 = x.ld2; a.C1 = x.C1;
  a.H = x.H; a.W = x.W; a.Cin = x.C;
}
static inline void conv_skip_input(ConvArgs& a, const Tn& sx) {
  a.sx = sx.p; a.sx_bs = image_bs(sx, sx.ld); a.ldsx = sx.ld;
  a.sx2 = sx.p2; a.sx2_bs = image_bs(sx, sx.ld2); a.ldsx2 = sx.ld2; a.sC1 = sx.C1; a.sCin = sx.C;
}
static inline void conv_residual(ConvArgs& a, const Tn& r) { a.res = r.p; a.res_bs = image_bs(r, r.ld); a.ldr = r.ld; }
static inline void conv_output(ConvArgs& a, const Tn& y) { a.y = y.p; a.y_bs = image_bs(y, y.ld); a.ldy = y.ld; }

// Pinned host staging for small stream-ordered copies (a pageable hipMemcpyAsync + stream sync was measured waiting for the
// work of OTHER streams: 200 ms per new utterance length with four samplers in flight) + the event of its last use
struct PinnedStage {
  char* p = nullptr;
  size_t cap = 0;  // elements
  hipEvent_t ev = nullptr;
  bool rec = false;
  PinnedStage() = default;
  PinnedStage(const PinnedStage&) = delete;
  ~PinnedStage() { if (ev) hipEventDestroy(ev); if (p) hipHostFree(p); }
  int wait() { if (rec) DS_HIP(hipEventSynchronize(ev)); return 0; }  // until the last recorded copy is through the buffer
  // wait, grow to n elements (never below 4096, never shrinking), hand out the buffer
  template <typename T>
  int acquire(size_t n, T** out) {
    if (wait()) return 1;
    if (n > cap) {
      if (p) DS_HIP(hipHostFree(p));
      p = nullptr;
      cap = 0;
      const size_t grown = n < 4096 ? 4096 : n;
      DS_HIP(hipHostMalloc((void**)&p, grown * sizeof(T), hipHostMallocDefault));
      cap = grown;
    }
    if (!ev) DS_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    *out = reinterpret_cast<T*>(p);
    return 0;
  }
  int record(hipStream_t st) { DS_HIP(hipEventRecord(ev, st)); rec = true; return 0; }
};

struct diffsep_engine {
  diffsep_engine() = default;
  diffsep_engine(const diffsep_engine&) = delete;
  ~diffsep_engine();  // releases everything below (the caller has made sure that no work of the engine is in flight)
  diffsep_model_config cfg;
  Arch arch;
  int esz = 4;
  float* d_blob = nullptr;
  char* d_pack = nullptr;
  float* d_dense_w = nullptr;
  float* d_dense_b = nullptr;
  float* d_attn_b = nullptr;  // folded query / key biases of the fused attention blocks
  float* d_tab = nullptr;
  // arena
  char* arena = nullptr;
  size_t cap = 0, top = 0, fwd_base = 0;
  size_t stats_need = 0, stats_used = 0;  // GroupNorm accumulator region of one forward (sized by the dry run)
  char* stats_ptr = nullptr;
  bool dry = false;
  int planB = -1;
  long planT = -1;
  // sampler state (inside the arena, below fwd_base)
  float *st_x = nullptr, *st_xm = nullptr, *st_score = nullptr, *st_t = nullptr, *st_noise = nullptr,
        *st_ts = nullptr, *st_mix = nullptr, *st_smix = nullptr, *st_lang = nullptr;
  int* st_lens = nullptr;             // per-utterance lengths of a mixed-length batch (diffsep_sampler_ext)
  unsigned long long* st_seeds = nullptr;
  PinnedStage ext_pin;                // staging of (seeds, lengths)
  // The captured graphs (one NFE: (st_x, st_t, st_mix) -> st_score) of the plans seen so far, keyed by (B, T): every plan lays
  // its tensors out in the ONE arena, so a graph stays valid until the arena is reallocated.  cur_graph = the current plan's
  // entry (null: not captured yet).
  // The cache is an LRU of graph_cap plans (option "graph_cache", default 12: a CLI meets a handful of (batch, width bucket)
  // pairs; the Python API passes raw signal lengths, and a loop over utterances of distinct lengths must not keep one graph of
  // several hundred nodes per length for ever).
  struct GraphRec { hipGraph_t g; hipGraphExec_t x; uint64_t used; };
  std::map<std::pair<int, long>, GraphRec> graphs;
  GraphRec* cur_graph = nullptr;
  int graph_cap = 12;
  uint64_t graph_tick = 0;
  int use_graph = 1;
  unsigned opts = 0;      // DS_OPT_* dispatch switches of this engine's launches (copied from the process defaults at creation)
  unsigned ablate = 0;    // option "ablate" (measurement aid, tools/ablate_bench.py): launch classes that are SKIPPED
  bool warmed = false;
  int64_t weight_bytes = 0;
  // work never runs on the legacy null stream (it cannot be captured): a NULL `stream` argument is
  // mapped to this private stream, ordered against the null stream with events on both sides.
  hipStream_t own = nullptr;
  hipEvent_t ev_in = nullptr, ev_out = nullptr;
  PinnedStage ts_pin;         // staging of the time-step upload
  std::vector<float> ts_dev;  // time steps currently in st_ts (for ts_B batch rows): re-uploaded only when they change
  int ts_B = 0;
  bool had_arena = false;
  bool dbg_alloc = false;  // DIFFSEP_DBG_ALLOC=1: log every arena allocation (offset, bytes) to stderr
  // option "track_tensors": every activation tensor of a forward is recorded so that diffsep_engine_debug_absmax can scan them
  // (the range margin of half-precision storage: tests/test_round5_gpu.py); off by default, eager forwards only
  bool track_tensors = false;
  struct Tracked { void* p; long n; int H, W, C; };
  std::vector<Tracked> tracked;
  // option "trace": every tensor and side array an eager forward WRITES gets a record (diffsep_engine_debug_trace; the
  // checker is tests/netcheck.py).  trace_on = the option, tracing = inside diffsep_score_forward / diffsep_backbone_forward with
  // the option on (graph capture and the samplers never record), trace_mod = the module the forward is in (-1 outside the list).
  // Host bookkeeping only: no launch decision reads any of it.
  bool trace_on = false, tracing = false;
  int trace_mod = -1;
  struct TraceRec {
    const char* kind; const char* role; std::string kernel;
    int mod, B, H, W, C, ld, f32; long long off, stats_off;
  };
  std::vector<TraceRec> trace;
  // DIFFSEP_F32_SPLIT: fp32 tensors, every MFMA product as 3 bf16 MFMAs on hi / lo halves (cfg.dtype stays DS_F32)
  int split = 0;
  // optional per-launch timing of the MFMA kernels (HIP events on the launch stream)
  bool prof = false;
  struct ProfRec {  // (cls: kernel class of profile_end's arrays; -1: reported through profile_records only)
    hipEvent_t a = nullptr, b = nullptr; double flops = 0.0, bytes = 0.0; int cls = -1; const char* kernel = nullptr;
    int B = 0, H = 0, W = 0, Cin = 0, Cout = 0, taps = 0, sCin = 0, res = 0; float ms = 0.f;
  };
  std::vector<ProfRec> prof_done;  // the records of the last profile_begin .. profile_end span, with their times
  std::vector<ProfRec> prof_recs;
  std::vector<hipEvent_t> ev_pool;
  // probability-flow ODE sampler (diffsep_ode_sample): y, y_new (fp64), K[7] (fp32), the partial-sum slab and the two
  // norms, in one allocation made at the first ODE call (outside the arena: the PC sampler's plan does not change)
  char* ode_buf = nullptr;
  size_t ode_cap = 0;
  PinnedStage ode_pin;  // readback of the norms
  PinnedStage ode_tab_pin;  // diffsep_ode_sample_each: staging of the per-utterance tables of one step attempt
};

// One launch (or launch sequence) `body` on st, bracketed by two events when the engine is inside a profile_begin .. profile_end
// span: r carries what the caller knows of it (flops, bytes = the ALGORITHMIC HBM bytes: every input read once, every output
// written once; class; a static kernel name; shape)
static inline hipEvent_t prof_event(diffsep_engine* e) {
  if (!e->ev_pool.empty()) { hipEvent_t v = e->ev_pool.back(); e->ev_pool.pop_back(); return v; }
  hipEvent_t v = nullptr;
  hipEventCreate(&v);
  return v;
}
template <typename F>
static int prof_launch(diffsep_engine* e, hipStream_t st, diffsep_engine::ProfRec r, F&& body) {
  if (!e->prof) return body();
  r.a = prof_event(e); r.b = prof_event(e);
  hipEventRecord(r.a, st);
  const int rc = body();
  hipEventRecord(r.b, st);
  e->prof_recs.push_back(r);
  return rc;
}
// the record of an HBM-bound launch (GroupNorm apply / FIR resampling, STFT / iSTFT, SDE and ODE updates, RNG)
static inline diffsep_engine::ProfRec hbm_rec(const char* name, double bytes, int B, int H, int W, int C) {
  diffsep_engine::ProfRec r;
  r.kernel = name; r.bytes = bytes; r.B = B; r.H = H; r.W = W; r.Cin = C;
  return r;
}

struct StreamScope {
  diffsep_engine* e; hipStream_t user; hipStream_t st;
  StreamScope(diffsep_engine* e_, void* s) : e(e_), user((hipStream_t)s), st((hipStream_t)s) {
    if (!user) {
      // the private stream is only created for callers on the null stream: HIP maps streams onto its few hardware
      // queues in creation order, and streams nobody uses would alias the caller's streams onto one queue
      if (!e->own) hipStreamCreateWithFlags(&e->own, hipStreamNonBlocking);
      st = e->own;
      hipEventRecord(e->ev_in, nullptr);
      hipStreamWaitEvent(st, e->ev_in, 0);
    }
  }
  ~StreamScope() {
    if (!user) {
      hipEventRecord(e->ev_out, st);
      hipStreamWaitEvent(nullptr, e->ev_out, 0);
    }
  }
};

// arch.hip: device copies of the fp32 blob and of every weight in the layouts the kernels read (`what` names the blob in the
// size error)
int upload_weights(diffsep_engine* e, const float* weights_host, int64_t n_floats, const char* what);
// engine.hip
float* e_f32(diffsep_engine* e, size_t n);
int stats_begin(diffsep_engine* e, hipStream_t st);
int res_block(diffsep_engine* e, const Module& m, const Tn& x, const float* temb_proj, int B, Tn& out, hipStream_t st);
int attn_block(diffsep_engine* e, const Module& m, const Tn& x, int B, Tn& out, hipStream_t st);
int attention_core(const Tn& q, const void* k, const void* vt, const Tn& o, int B, void* scores, void* probs, int dtype,
                   hipStream_t st, int split = 0);
int ensure_plan(diffsep_engine* e, int B, long T, hipStream_t st);
int run_nfe(diffsep_engine* e, int B, long T, hipStream_t st);
// sampler.hip: zero the tail t >= lens[b] of [B][rows][T] rows (the mixture of a mixed-length batch)
int ds_launch_mask_tail(float* v, int B, int rows, long T, const int* lens, hipStream_t st);
// sampler.hip: what every entry asks of the SDE description and of the batch extensions (`who`: the entry's name in the
// message; a null extension field is not checked, and the lengths need no engine), and PriorMixSDE's noise scale of st_mix
int check_sde(const diffsep_engine* e, const diffsep_sde_config* sde, const char* who);
int check_batch_ext(const diffsep_model_config* cfg, const char* who, int B, long T, const int64_t* lengths,
                    const uint64_t* seeds, const float* noise, const diffsep_engine* e, const diffsep_engine* tail);
int mixture_scale(diffsep_engine* e, const diffsep_sde_config* sde, int B, long T, hipStream_t st, const float** smix);

#pragma GCC visibility pop
