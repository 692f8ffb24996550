// engine.hip — the engine itself: options, the workspace arena, the forward of NCSN++ (models/ncsnpp.py:319-478) as a
// launch sequence, the plan of a (B, T) batch and its captured graph (eager or hipGraph replay), per-launch profiling.
// Everything that touches data is a HIP kernel from the sibling files; this file only sequences launches.  The architecture
// table and the weight upload are in arch.hip, the samplers in sampler.hip, the unit entry points in unit.hip.
#include "engine_host.h"

// ------------------------------------------------------------------ error string
static thread_local std::string g_err;
void ds_set_error(const std::string& s) { g_err = s; }
extern "C" const char* diffsep_last_error(void) { return g_err.c_str(); }
extern "C" const char* diffsep_version(void) {
    // which build of the library this is: 16-bit tensors stored as bfloat16 or (-DDS_HALF_F16) as IEEE half precision
#ifdef DS_HALF_F16
    return "diffsep-hip 0.3 (gfx950, 16-bit storage f16)";
#else
    return "diffsep-hip 0.3 (gfx950, 16-bit storage bf16)";
#endif
}

// ------------------------------------------------------------------ process-wide options, device properties
// The dispatch switches (common.h DS_OPT_*): option name, the environment variable that sets its process default (or null), bit.
// The environment is read ONCE (never inside a launch decision); diffsep_set_option changes the defaults for engines created
// later and for the unit entry points.
static const struct { const char* name; const char* env; unsigned bit; } kOpts[] = {
    {"no_rw", "DIFFSEP_NO_RW", DS_OPT_NO_RW},
    {"no_rw128", "DIFFSEP_NO_RW128", DS_OPT_NO_RW128},
    {"rw_small", "DIFFSEP_RW_SMALL", DS_OPT_RW_SMALL},
    {"no_rw_res", "DIFFSEP_NO_RW_RES", DS_OPT_NO_RW_RES},
    {"no_rw_helper", nullptr, DS_OPT_NO_RW_HELPER},
    {"no_wfrag", nullptr, DS_OPT_NO_WFRAG},
    {"no_attn_fused", nullptr, DS_OPT_NO_ATTN_FUSED},
    {"no_stft_fused", "DIFFSEP_NO_STFT_FUSED", DS_OPT_NO_STFT_FUSED},
    {"rw_half", "DIFFSEP_RW_HALF", DS_OPT_RW_HALF},
    {"rw_quarter", "DIFFSEP_RW_QUARTER", DS_OPT_RW_QUARTER},
    {"rw_big_half", "DIFFSEP_RW_BIG_HALF", DS_OPT_RW_BIG_HALF},
    {"no_split256", nullptr, DS_OPT_NO_SPLIT256},
    {"no_sw", "DIFFSEP_NO_SW", DS_OPT_NO_SW},
    {"no_sws", "DIFFSEP_NO_SWS", DS_OPT_NO_SWS},
    {"no_sw_rows4", "DIFFSEP_NO_SW_ROWS4", DS_OPT_NO_SW_ROWS4},
    {"sw_rows4", nullptr, DS_OPT_SW_ROWS4},
    {"no_sw_rw", "DIFFSEP_NO_SW_RW", DS_OPT_NO_SW_RW}};
static std::atomic<unsigned> g_opts{0};  // (read by every thread that creates an engine or calls a unit entry point)
static std::once_flag g_opts_once;
unsigned ds_default_opts() {
  std::call_once(g_opts_once, [] {
    for (const auto& o : kOpts) {
      const char* v = o.env ? getenv(o.env) : nullptr;
      if (v && *v && strcmp(v, "0") != 0) g_opts |= o.bit;
    }
  });
  return g_opts;
}
int ds_num_cus() {
  static std::atomic<int> cus[32];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 32) dev = 0;
  int c = cus[dev].load(std::memory_order_relaxed);
  if (c <= 0) {
    hipDeviceProp_t prop;
    c = hipGetDeviceProperties(&prop, dev) == hipSuccess ? prop.multiProcessorCount : 0;
    if (c <= 0) c = 256;
    cus[dev].store(c, std::memory_order_relaxed);
  }
  return c;
}
static int opt_bit(const char* name, unsigned* bit) {
  for (const auto& o : kOpts)
    if (!strcmp(name, o.name)) { *bit = o.bit; return 0; }
  return 1;
}
extern "C" int32_t diffsep_set_option(const char* name, int64_t value) {
  DS_CHECK(name, "set_option: null name");
  unsigned bit = 0;
  if (opt_bit(name, &bit)) { ds_set_error(std::string("set_option: unknown option '") + name + "'"); return 1; }
  ds_default_opts();
  if (value) g_opts.fetch_or(bit); else g_opts.fetch_and(~bit);
  return 0;
}

// ------------------------------------------------------------------ arena
static Tn cat_view(const Tn& a, const Tn& b) {
  Tn t = a;
  t.C = a.C + b.C; t.C1 = a.C; t.p2 = b.p; t.ld2 = b.ld;
  t.sa2 = b.sa;
  return t;
}

static void* e_alloc(diffsep_engine* e, size_t bytes) {
  const size_t a = (e->top + 255) & ~(size_t)255;
  e->top = a + bytes;
  if (e->dry) return (void*)(uintptr_t)(a + 256);  // fake non-null
  if (e->dbg_alloc) fprintf(stderr, "[diffsep alloc] %zu %zu\n", a, bytes);
  return e->arena + a;
}
// GroupNorm accumulators live in one region at the start of a forward's allocations: ONE fill launch per forward
// zeroes them all (they are filled by integer atomics)
static long long* e_alloc_stats(diffsep_engine* e, size_t bytes) {
  const size_t a = (e->stats_used + 255) & ~(size_t)255;
  e->stats_used = a + bytes;
  if (e->dry) { if (e->stats_used > e->stats_need) e->stats_need = e->stats_used; return (long long*)(uintptr_t)256; }
  if (e->stats_used > e->stats_need) { ds_set_error("internal: GroupNorm accumulator region overflow"); return nullptr; }
  return (long long*)(e->stats_ptr + a);
}
int stats_begin(diffsep_engine* e, hipStream_t st) {  // call right after e->top = e->fwd_base
  e->stats_used = 0;
  if (e->dry) { e->stats_need = 0; return 0; }
  e->stats_ptr = (char*)e_alloc(e, e->stats_need);
  // zeroed by a kernel, not hipMemsetAsync: as a captured memset NODE it made every engine but the first return
  // different samples when the graph was replayed on another stream (B >= 4; profiles/experiments/README.md)
  if (e->stats_need && ds_launch_fill((float*)e->stats_ptr, 0.f, (long)(e->stats_need / 4), st)) return 1;
  return 0;
}
static Tn e_tensor(diffsep_engine* e, int B, int H, int W, int C) {
  Tn t;
  t.C = C; t.ld = C; t.H = H; t.W = W;
  t.p = e_alloc(e, (size_t)B * H * W * C * e->esz);
  if (e->track_tensors && !e->dry) e->tracked.push_back({t.p, (long)B * H * W * C, H, W, C});
  return t;
}
float* e_f32(diffsep_engine* e, size_t n) { return (float*)e_alloc(e, n * 4); }
// ---- option "trace": one record per tensor / side array a step has just written (outputs only; engine_host.h)
static void trace_raw(diffsep_engine* e, const char* kind, const char* role, const void* p, int B, int H, int W, int C, int ld,
                      int f32, const long long* sa, const char* kernel = "") {
  if (!e->tracing || e->dry) return;
  const char* a = e->arena;
  const char* q = (const char*)p;
  const long long off = (a && q >= a && q < a + e->cap) ? (long long)(q - a) : -1;
  e->trace.push_back({kind, role, kernel ? kernel : "", e->trace_mod, B, H, W, C, ld, f32, off,
                      sa ? (long long)((const char*)sa - e->stats_ptr) : -1});
}
static void trace_tn(diffsep_engine* e, const char* kind, const char* role, const Tn& t, int B, const char* kernel = "") {
  trace_raw(e, kind, role, t.p, B, t.H, t.W, t.C, t.ld, 0, t.sa, kernel);
}
static void trace_f32(diffsep_engine* e, const char* kind, const char* role, const float* p, int B, int n) {
  trace_raw(e, kind, role, p, B, 1, 1, n, n, 1, nullptr);
}
static const float* P(diffsep_engine* e, const PRef& r) { return e->d_blob + r.off; }
static const void* PK(diffsep_engine* e, long off) { return e->d_pack + off * e->esz; }
static const void* PKF(diffsep_engine* e, long off) { return off >= 0 ? e->d_pack + off * e->esz : nullptr; }

// option "ablate" (a measurement aid: what would the step cost if these launches were free?): bit 0 = every convolution /
// GEMM of the <= 16-row levels (attention included), 1 / 2 / 5 / 6 = those of the 32 / 64 / 128 / 256-row level, 3 = the
// gn_apply / FIR resampling kernels, 4 = gn_finalize, 7 = the STFT / iSTFT passes.  Results are garbage by construction.
static bool ablated(const diffsep_engine* e, int H) {
  if (!e->ablate) return false;
  const unsigned bit = H <= 16 ? 1u : H == 32 ? 2u : H == 64 ? 4u : H == 128 ? 32u : H == 256 ? 64u : 0u;
  return (e->ablate & bit) != 0;
}

// ---- launch helpers (skip when dry)
// GroupNorm of a conv input: either materialised per-(b,c) scale / shift arrays, or (lazy) the producers'
// accumulators + affine parameters, from which the consuming conv builds the table itself (no launch)
struct GnAff {
  float* scale = nullptr; float* shift = nullptr;
  const long long* acc1 = nullptr; const long long* acc2 = nullptr;
  const float* gamma = nullptr; const float* beta = nullptr; int groups = 0; float inv_count = 0.f;
};
struct SkipConv { const Tn* x; const void* w; int chunk; const void* w_frag; };  // fused 1x1 skip convolution on the raw block input
// One convolution launch.  x, w, Cout and taps are required; every other operand is optional and off by default.
struct Conv {
  const Tn& x;
  const void* w;  // packed [Cout][taps][Cin] (chunk-major where weight_chunk says so)
  int Cout, taps;
  Conv(const Tn& x_, const void* w_, int Cout_, int taps_) : x(x_), w(w_), Cout(Cout_), taps(taps_) {}
  const void* w_frag = nullptr;      // fragment-major copy of w (PKF)
  const void* ident_frag = nullptr;  // ... of the identity, for a residual that the kernel meets as a folded skip
  const float* bias = nullptr;       // [Cout]
  const float* bias_b = nullptr;     // + a per-batch bias [B][bias_b_ld] (stride 0: a second [Cout] bias)
  int bias_b_ld = 0;
  const float* div_b = nullptr;      // per-batch divisor of the accumulator
  const Tn* res = nullptr;           // residual, added before `scale`
  float scale = 1.f;
  const GnAff* gn = nullptr;         // the input is SiLU(GroupNorm(x))
  const SkipConv* skip = nullptr;
  bool want_stats = false;           // the output gets GroupNorm accumulators (y.sa)
  const char* role = "out";          // what the output is to its block (option "trace")
};
// The launcher's view of a Conv writing into y (no launch, no allocation: stats_acc is conv()'s to set)
static ConvArgs conv_args(const diffsep_engine* e, const Conv& c, const Tn& y, int B) {
  const Tn& x = c.x;
  ConvArgs a;
  memset(&a, 0, sizeof(a));
  a.B = B; a.Cout = c.Cout; a.taps = c.taps; a.dtype = e->cfg.dtype; a.split = e->split; a.opts = e->opts;
  conv_input(a, x);
  if (c.gn) {
    a.gn_scale = c.gn->scale; a.gn_shift = c.gn->shift; a.gn_act = 1;
    if (c.gn->acc1) {
      a.gn_acc1 = c.gn->acc1; a.gn_acc2 = c.gn->acc2; a.gn_gamma = c.gn->gamma; a.gn_beta = c.gn->beta;
      a.gn_groups = c.gn->groups; a.gn_inv_count = c.gn->inv_count; a.gn_eps = 1e-6f;
    }
  }
  a.w = c.w; a.w_bs = 0; a.w_chunked = weight_chunk(c.taps, x.C, x.p2 ? x.C1 : 0, e->cfg.dtype);
  const bool use_frag = (e->cfg.dtype == DS_BF16 || (e->cfg.dtype == DS_F32 && e->split)) && !(e->opts & DS_OPT_NO_WFRAG);
  a.w_frag = use_frag ? c.w_frag : nullptr;
  a.ident_frag = use_frag ? c.ident_frag : nullptr;
  a.bias = c.bias; a.bias_b = c.bias_b; a.bias_b_ld = c.bias_b_ld; a.bias_mode = 0; a.div_b = c.div_b;
  if (c.res) conv_residual(a, *c.res);
  a.out_scale = c.scale;
  conv_output(a, y);
  if (c.skip) {
    conv_skip_input(a, *c.skip->x);
    a.sw = c.skip->w; a.sw_chunked = c.skip->chunk;
    a.sw_frag = use_frag ? c.skip->w_frag : nullptr;
  }
  return a;
}
static int conv(diffsep_engine* e, const Conv& c, Tn& y, int B, hipStream_t st) {
  ConvArgs a = conv_args(e, c, y, B);
  if (c.want_stats) {  // the consumer's GroupNorm reads these partials instead of re-reading the tensor
    y.sa = e_alloc_stats(e, (size_t)B * c.Cout * 2 * sizeof(long long));
    if (!y.sa) return 1;
    a.stats_acc = y.sa;
  }
  const ConvPlan p = ds_conv_plan(a);  // (the one plan of this launch: its kernel, its profile class)
  DS_CHECK(!a.sx || p.skip_ok, "internal: fused skip conv on an unsupported tile");
  if (c.want_stats && e->dbg_alloc && !e->dry)
    fprintf(stderr, "[diffsep stats] %ld Cin %d Cout %d taps %d HxW %dx%d res %d skip %d bias_b %d cfg %d\n",
            (long)((char*)y.sa - e->stats_ptr), a.Cin, c.Cout, c.taps, a.H, a.W, c.res != nullptr, c.skip != nullptr,
            c.bias_b != nullptr, p.cls);
  if (e->dry || ablated(e, a.H)) return 0;
  if (!e->prof) {
    const int rc = ds_launch_conv(a, p, st);
    trace_tn(e, "conv", c.role, y, B, ds_last_conv_kernel());
    return rc;
  }
  diffsep_engine::ProfRec r;
  r.flops = 2.0 * ((double)a.taps * a.Cin + (a.sx ? a.sCin : 0)) * a.Cout * (double)a.H * a.W * a.B;
  {  // algorithmic HBM bytes: input (+ fused skip input) + output (+ residual) once each, weights once
    const double esz = a.dtype == DS_F32 ? 4.0 : 2.0;
    r.bytes = esz * ((double)a.B * a.H * a.W *
                         ((double)a.Cin + a.Cout + (a.res ? a.Cout : 0) + (a.sx ? a.sCin : 0)) +
                     ((double)a.taps * a.Cin + (a.sx ? a.sCin : 0)) * a.Cout);
  }
  r.cls = p.cls;
  r.B = a.B; r.H = a.H; r.W = a.W; r.Cin = a.Cin; r.Cout = a.Cout; r.taps = a.taps; r.sCin = a.sx ? a.sCin : 0; r.res = a.res != nullptr;
  const int rc = prof_launch(e, st, r, [&]() { return ds_launch_conv(a, p, st); });
  e->prof_recs.back().kernel = ds_last_conv_kernel();  // (the instantiation the dispatch chose)
  trace_tn(e, "conv", c.role, y, B, ds_last_conv_kernel());
  return rc;
}

static int gn_stats(diffsep_engine* e, const Tn& x, const float* gamma, const float* beta, int B, GnAff& aff,
                    hipStream_t st, bool lazy = false) {
  const int groups = gn_group_count(x.C);
  aff = GnAff();
  const bool have_acc = x.sa && (!x.p2 || x.sa2);
  if (have_acc && lazy && x.C <= 512) {  // the consuming conv computes scale / shift in its prologue
    // (its LDS table holds 512 channels; wider inputs take the materialised arrays below)
    aff.acc1 = x.sa; aff.acc2 = x.sa2; aff.gamma = gamma; aff.beta = beta; aff.groups = groups;
    aff.inv_count = gn_inv_count((long)x.H * x.W, x.C, groups);
    return 0;
  }
  aff.scale = e_f32(e, (size_t)B * x.C);
  aff.shift = e_f32(e, (size_t)B * x.C);
  if (have_acc) {
    if (e->dry || (e->ablate & 16u)) return 0;
    trace_f32(e, "gn_finalize", "scale", aff.scale, B, x.C);
    trace_f32(e, "gn_finalize", "shift", aff.shift, B, x.C);
    return ds_launch_gn_finalize_acc(x.sa, x.p2 ? x.C1 : x.C, x.sa2, x.p2 ? x.C - x.C1 : 0, B, (long)x.H * x.W, groups,
                                     1e-6f, gamma, beta, aff.scale, aff.shift, st);
  }
  void* ws = e_alloc(e, (size_t)ds_gn_workspace_bytes(B, x.H, x.W, x.C));
  if (e->dry) return 0;
  trace_f32(e, "gn_stats", "scale", aff.scale, B, x.C);
  trace_f32(e, "gn_stats", "shift", aff.shift, B, x.C);
  return ds_launch_gn_stats(x.p, x.ld, x.p2, x.ld2, x.C1, B, x.H, x.W, x.C, groups, 1e-6f, gamma, beta, ws, aff.scale,
                            aff.shift, e->cfg.dtype, st);
}
static int gn_apply(diffsep_engine* e, const Tn& x, const GnAff* aff, const Tn* y, const Tn* xr, int B, int act,
                    int mode, hipStream_t st) {
  if (e->dry || (e->ablate & 8u)) return 0;
  // algorithmic bytes: x read once; each output (act(GN(x)) and / or raw x, resampled: x 4 up, / 4 down) written once
  const double esz = e->cfg.dtype == DS_F32 ? 4.0 : 2.0, nin = (double)B * x.H * x.W * x.C;
  const double fo = mode == 1 ? 4.0 : (mode == 2 ? 0.25 : 1.0);
  const double bytes = esz * nin * (1.0 + fo * ((y ? 1 : 0) + (xr ? 1 : 0)));
  const char* name = mode == 1 ? (aff ? "gn_fir_up (GroupNorm + SiLU + FIR x2 up of act and raw)" : "fir_up (pyramid)")
                               : (mode == 2 ? (aff ? "gn_fir_down (GroupNorm + SiLU + FIR x2 down of act and raw)" : "fir_down (pyramid)")
                                            : "gn_apply (GroupNorm affine + SiLU)");
  return prof_launch(e, st, hbm_rec(name, bytes, B, x.H, x.W, x.C), [&]() {
    return ds_launch_gn_apply(x.p, x.ld, aff ? aff->scale : nullptr, aff ? aff->shift : nullptr, x.C, y ? y->p : nullptr,
                              y ? y->ld : 0, xr ? xr->p : nullptr, xr ? xr->ld : 0, B, x.H, x.W, act, mode, e->cfg.dtype,
                              st);
  });
}

static const float kInvSqrt2 = 0.70710678118654752440f;

// Conv_1 of a block with Conv_2 (1x1 on the raw, possibly resampled block input `skip_src`; layerspp.py:317-318) folded in as
// extra K through its centre tap: no separate launch, no skip tensor in HBM
static int conv1_folded_skip(diffsep_engine* e, const Module& m, const Tn& h1, const Tn& skip_src, const GnAff& a1, Tn& out,
                             int B, hipStream_t st) {
  const SkipConv sk = {&skip_src, PK(e, m.pk2), weight_chunk(9, m.in_ch, m.in_c1, e->cfg.dtype), PKF(e, m.pf2)};
  Conv c(h1, PK(e, m.pk1), m.out_ch, 9);
  c.w_frag = PKF(e, m.pf1); c.gn = &a1; c.skip = &sk; c.scale = kInvSqrt2; c.want_stats = true;
  c.bias = P(e, m.conv1_b); c.bias_b = P(e, m.conv2_b);  // conv bias + Conv_2 bias: the second as a "per-batch" bias with stride 0
  return conv(e, c, out, B, st);
}

// ResnetBlockBigGANpp.forward  layerspp.py:291-323.  act(GN(.)) is never materialised for the plain blocks:
// both 3x3 convs apply it while staging their input tile; x may be an in-place concat view.
int res_block(diffsep_engine* e, const Module& m, const Tn& x, const float* temb_proj, int B, Tn& out,
              hipStream_t st) {
  DS_CHECK(x.C == m.in_ch, "internal: resblock channel mismatch");
  const int mode = m.up ? 1 : (m.down ? 2 : 0);
  const int Ho = m.up ? 2 * x.H : (m.down ? x.H / 2 : x.H);
  const int Wo = m.up ? 2 * x.W : (m.down ? x.W / 2 : x.W);
  GnAff a0, a1;
  const float* temb = temb_proj + m.temb_off;  // this block's Dense_0(act(temb)), row stride dense_total
  // cat(128, 128) -> 128 on a level with at least one 4 x 32 tile per CU (nf = 128 at 256^2 / 128^2), 16-bit: no register-weight
  // kernel holds 256 input channels (section 8 of DESIGN.md), but conv(cat(a, b)) = conv_a(a) + conv_b(b) and no GroupNorm group
  // straddles the seam (256 / 32 = 8 channels per group): each convolution runs as TWO 128 -> 128 register-weight launches, the
  // second taking the first's result as its residual (one more storage rounding of a partial sum).  Conv_0: 850 -> 593 us at
  // 256^2; Conv_1 + the 256-channel 1x1 skip: the first half of the skip folded as before, the second as a 1x1 launch.
  // Only from 128 rows up: at 64^2 (where nf = 64 has these blocks) the register-weight launches carry their weight prologue for
  // two tiles per block and the pair is SLOWER than the generic tile (61.5 + 50.0 against 49.3 + 42.6 us per block in the graph).
  // Round 5, with the streamed-weight kernel (conv3x3_sw.hip; stand-alone, B = 16): Conv_0 as ONE launch 659 us at 256^2 against
  // 269 + 318 for the pair, 155 against 77 + 89 at 128^2 — the pair stays at 256 rows; Conv_1 with the WHOLE 256-channel skip
  // folded 438 us at 256^2 against 319 + 193 (3x3 with half of the skip + the 1x1 launch on the other half), 103 against 91 + 47 at
  // 128^2 — one launch at every size.  Option no_sw: the route of round 4.
  if (e->cfg.dtype == DS_BF16 && mode == 0 && x.p2 && m.pf0a >= 0 && x.C1 == 128 && x.sa && x.sa2 &&
      x.H >= ((e->opts & DS_OPT_NO_SW) ? 128 : 256) && !(e->opts & (DS_OPT_NO_SPLIT256 | DS_OPT_NO_WFRAG))) {
    Tn xa = x, xb = x;
    xa.C = 128; xa.p2 = nullptr; xa.C1 = 0; xa.ld2 = 0; xa.sa2 = nullptr;
    xb.p = x.p2; xb.ld = x.ld2; xb.C = 128; xb.p2 = nullptr; xb.C1 = 0; xb.ld2 = 0; xb.sa = x.sa2; xb.sa2 = nullptr;
    GnAff ga, gb;
    ga.acc1 = xa.sa; ga.gamma = P(e, m.gn0_w); ga.beta = P(e, m.gn0_b);
    ga.groups = gn_group_count(x.C) / 2;  // (of the 128-channel half)
    ga.inv_count = gn_inv_count((long)x.H * x.W, x.C, gn_group_count(x.C));
    gb = ga; gb.acc1 = xb.sa; gb.gamma = ga.gamma + 128; gb.beta = ga.beta + 128;
    Conv c0a(xa, PK(e, m.pk0), m.out_ch, 9);
    c0a.w_frag = PKF(e, m.pf0a); c0a.gn = &ga; c0a.bias = P(e, m.conv0_b); c0a.bias_b = temb; c0a.bias_b_ld = e->arch.dense_total;
    // ... and only where the register-weight kernel's rule takes such a half (whole tiles, one 4 x 32 tile per CU, no_rw / no_rw128
    // off; the streamed-weight kernel may still come first) — without rw_small, the unit tests' way past the tile counts
    Tn h1p; h1p.C = h1p.ld = m.out_ch; h1p.H = Ho; h1p.W = Wo;  // (its shape is all the plan reads)
    ConvArgs half = conv_args(e, c0a, h1p, B); half.opts &= ~DS_OPT_RW_SMALL;
    if (ds_conv_plan(half).rw_ok) {
      h1p = e_tensor(e, B, Ho, Wo, m.out_ch);
      Tn h1 = e_tensor(e, B, Ho, Wo, m.out_ch);
      const long half0 = 4L * 9 * m.out_ch * 32;  // chunk-major [Cin / 32][9][Cout][32]: the first source = the first 4 chunks
      c0a.role = "h1p";
      if (conv(e, c0a, h1p, B, st)) return 1;
      Conv c0b(xb, PK(e, m.pk0 + half0), m.out_ch, 9);
      c0b.w_frag = PKF(e, m.pf0b); c0b.gn = &gb; c0b.res = &h1p; c0b.want_stats = true; c0b.role = "h1";
      if (conv(e, c0b, h1, B, st)) return 1;
      if (gn_stats(e, h1, P(e, m.gn1_w), P(e, m.gn1_b), B, a1, st, true)) return 1;
      out = e_tensor(e, B, Ho, Wo, m.out_ch);
      if (!(e->opts & DS_OPT_NO_SW) && m.pf2 >= 0) return conv1_folded_skip(e, m, h1, x, a1, out, B, st);
      Tn outp = e_tensor(e, B, Ho, Wo, m.out_ch);
      const SkipConv sk = {&xa, PK(e, m.pk2), weight_chunk(9, 128, 0, e->cfg.dtype), PKF(e, m.pf2a)};
      Conv c1(h1, PK(e, m.pk1), m.out_ch, 9);
      c1.w_frag = PKF(e, m.pf1); c1.gn = &a1; c1.skip = &sk; c1.bias = P(e, m.conv1_b); c1.bias_b = P(e, m.conv2_b);
      c1.role = "outp";
      if (conv(e, c1, outp, B, st)) return 1;
      Conv c2b(xb, PK(e, m.pk2b), m.out_ch, 1);
      c2b.res = &outp; c2b.scale = kInvSqrt2; c2b.want_stats = true;
      return conv(e, c2b, out, B, st);
    }
  }
  if (gn_stats(e, x, P(e, m.gn0_w), P(e, m.gn0_b), B, a0, st, mode == 0)) return 1;  // resampling needs the arrays
  Tn h1 = e_tensor(e, B, Ho, Wo, m.out_ch);
  Tn xr = x, h0m;
  if (mode) {
    DS_CHECK(x.p2 == nullptr, "internal: resampling block on a concat view");
    h0m = e_tensor(e, B, Ho, Wo, m.in_ch);
    xr = e_tensor(e, B, Ho, Wo, m.in_ch);
    if (gn_apply(e, x, &a0, &h0m, &xr, B, 1, mode, st)) return 1;
    trace_tn(e, "gn_apply", "h0m", h0m, B, ds_last_conv_kernel());
    trace_tn(e, "gn_apply", "xr", xr, B, ds_last_conv_kernel());
  }
  if (!m.has_conv2) DS_CHECK(xr.p2 == nullptr, "internal: identity skip on a concat view");
  Conv c0(mode ? h0m : x, PK(e, m.pk0), m.out_ch, 9);  // (a resampling block's input is already act(GN(.)), resampled)
  c0.w_frag = PKF(e, m.pf0); c0.gn = mode ? nullptr : &a0; c0.want_stats = true; c0.role = "h1";
  c0.bias = P(e, m.conv0_b); c0.bias_b = temb; c0.bias_b_ld = e->arch.dense_total;
  if (conv(e, c0, h1, B, st)) return 1;
  if (gn_stats(e, h1, P(e, m.gn1_w), P(e, m.gn1_b), B, a1, st, true)) return 1;
  out = e_tensor(e, B, Ho, Wo, m.out_ch);
  if (m.has_conv2 && fuse_skip(m)) return conv1_folded_skip(e, m, h1, xr, a1, out, B, st);  // (conv() checks the tile takes it)
  Tn skip = xr;
  if (m.has_conv2) {  // narrow blocks (<= 32 couts use the 32-cout tile, which has no skip path): separate 1x1 launch
    skip = e_tensor(e, B, Ho, Wo, m.out_ch);
    Conv c2(xr, PK(e, m.pk2), m.out_ch, 1);
    c2.bias = P(e, m.conv2_b); c2.role = "skip";
    if (conv(e, c2, skip, B, st)) return 1;
  }
  Conv c1(h1, PK(e, m.pk1), m.out_ch, 9);
  c1.w_frag = PKF(e, m.pf1); c1.ident_frag = m.has_conv2 ? nullptr : PKF(e, m.pf_id);
  c1.gn = &a1; c1.bias = P(e, m.conv1_b); c1.res = &skip; c1.scale = kInvSqrt2; c1.want_stats = true;
  return conv(e, c1, out, B, st);
}

// attention core shared with the unit entry point: o = softmax(q k^T C^-1/2) v for q, o = [B][L][C] views (H = 1, W = L)
int attention_core(const Tn& q, const void* k, const void* vt, const Tn& o, int B, void* scores, void* probs, int dtype,
                   hipStream_t st, int split) {
  const int L = q.W, C = q.C, Lp = rup8(L);
  Tn s = q, p = q;  // scores and probabilities: [B][L][Lp]
  s.p = scores; p.p = probs; s.ld = p.ld = Lp; p.C = Lp;
  ConvArgs a;
  memset(&a, 0, sizeof(a));
  a.dtype = dtype; a.split = split; a.B = B; a.taps = 1; a.bias_mode = 0;
  // scores[b, i, j] = sum_c q[b,i,c] k[b,j,c] * C^-0.5
  conv_input(a, q);
  a.w = k; a.w_bs = (long)L * C;
  conv_output(a, s);
  a.Cout = L;
  a.out_scale = 1.0f / sqrtf((float)C);
  if (ds_launch_conv(a, st)) return 1;
  if (ds_launch_softmax(scores, probs, (long)B * L, L, Lp, dtype, st)) return 1;
  // o[b, i, c] = sum_j P[b,i,j] vt[b,c,j]
  conv_input(a, p);
  a.w = vt; a.w_bs = (long)C * Lp;
  conv_output(a, o);
  a.Cout = C;
  a.out_scale = 1.f;
  return ds_launch_conv(a, st);
}

// AttnBlockpp.forward  layerspp.py:76-92
int attn_block(diffsep_engine* e, const Module& m, const Tn& x, int B, Tn& out, hipStream_t st) {
  const int C = m.in_ch, L = x.H * x.W, Lp = rup8(L);
  DS_CHECK(x.C == C, "internal: attention channel mismatch");
  if (ds_attn_fused_eligible(e->cfg.dtype, C, L) && !x.p2 && m.pf_nin[0] >= 0 && !(e->opts & DS_OPT_NO_ATTN_FUSED)) {
    // the whole block in one launch (attn_fused.hip): GroupNorm from the producer's accumulators (a tensor without them — the
    // unit entry point — gets the statistics kernels first), projections, softmax attention, output projection, residual,
    // statistics for the consumer
    GnAff ga;
    if (!x.sa && gn_stats(e, x, P(e, m.gn0_w), P(e, m.gn0_b), B, ga, st)) return 1;
    out = e_tensor(e, B, x.H, x.W, C);
    out.sa = e_alloc_stats(e, (size_t)B * C * 2 * sizeof(long long));
    if (!out.sa) return 1;
    if (e->dry || ablated(e, x.H)) return 0;
    AttnFusedArgs a;
    memset(&a, 0, sizeof(a));
    a.x = x.p; a.x_bs = (long)L * x.ld; a.ldx = x.ld;
    a.gn_acc = x.sa; a.gn_scale = ga.scale; a.gn_shift = ga.shift; a.gn_gamma = P(e, m.gn0_w); a.gn_beta = P(e, m.gn0_b);
    a.gn_groups = gn_group_count(C); a.gn_inv_count = gn_inv_count(L, C, a.gn_groups); a.gn_eps = 1e-6f;
    a.wqk = PKF(e, m.pf_nin[0]); a.wv = PKF(e, m.pf_nin[2]); a.wo = PKF(e, m.pf_nin[3]);
    a.bqk = e->d_attn_b + m.ab_off; a.bv = P(e, m.nin_b[2]); a.bo = P(e, m.nin_b[3]);
    a.y = out.p; a.y_bs = (long)L * out.ld; a.ldy = out.ld;
    a.stats = out.sa;
    a.B = B; a.L = L; a.C = C;
    diffsep_engine::ProfRec r;  // (per-launch timing like the convolutions)
    // V^T, Q' and the output projection (2 L C^2 each), scores and P V (2 L^2 C each); input + output + three matrices once
    r.flops = (double)B * (6.0 * L * C * C + 4.0 * (double)L * L * C);
    r.bytes = (double)e->esz * (2.0 * B * L * C + 3.0 * C * C);
    r.cls = DS_CLS_ATTN; r.B = B; r.H = x.H; r.W = x.W; r.Cin = C; r.Cout = C; r.taps = 1; r.res = 1;
    r.kernel = "attn_fused_kernel";
    const int rc = prof_launch(e, st, r, [&]() { return ds_launch_attn_fused(a, st); });
    trace_tn(e, "attn_fused", "out", out, B, ds_last_conv_kernel());
    return rc;
  }
  GnAff a0;
  if (gn_stats(e, x, P(e, m.gn0_w), P(e, m.gn0_b), B, a0, st)) return 1;
  Tn h = e_tensor(e, B, x.H, x.W, C);
  if (gn_apply(e, x, &a0, &h, nullptr, B, 0, 0, st)) return 1;
  trace_tn(e, "gn_apply", "h", h, B, ds_last_conv_kernel());
  Tn q = e_tensor(e, B, x.H, x.W, C), k = e_tensor(e, B, x.H, x.W, C);
  Conv cq(h, PK(e, m.pk_nin[0]), C, 1), ck(h, PK(e, m.pk_nin[1]), C, 1);
  cq.bias = P(e, m.nin_b[0]); ck.bias = P(e, m.nin_b[1]); cq.role = "q"; ck.role = "k";
  if (conv(e, cq, q, B, st) || conv(e, ck, k, B, st)) return 1;
  // V^T[b, c, l] = sum_c' Wv[c', c] h[b, l, c'] + b[c]: A = packed Wv^T ([C][C]), Bt = h, bias along rows
  void* vt = e_alloc(e, (size_t)B * C * Lp * e->esz);
  void* scores = e_alloc(e, (size_t)B * L * Lp * e->esz);
  void* probs = e_alloc(e, (size_t)B * L * Lp * e->esz);
  Tn o = e_tensor(e, B, x.H, x.W, C);
  out = e_tensor(e, B, x.H, x.W, C);
  if (!e->dry && !ablated(e, x.H)) {
    Tn wv, vtn;  // A = Wv^T shared by the batch ([C][C]), output V^T [B][C][Lp]
    wv.p = const_cast<void*>(PK(e, m.pk_nin[2])); wv.C = wv.ld = C; wv.H = 1; wv.W = C;
    vtn.p = vt; vtn.ld = Lp; vtn.H = 1; vtn.W = C;
    ConvArgs a;
    memset(&a, 0, sizeof(a));
    a.dtype = e->cfg.dtype; a.split = e->split; a.B = B; a.taps = 1; a.out_scale = 1.f;
    conv_input(a, wv);
    a.x_bs = 0;
    a.w = h.p; a.w_bs = (long)L * C;
    a.bias = P(e, m.nin_b[2]); a.bias_mode = 1;
    conv_output(a, vtn);
    a.Cout = L;
    if (ds_launch_conv(a, st)) return 1;
    Tn qv = q, ov = o;  // [B][L][C] GEMM views
    qv.H = ov.H = 1; qv.W = ov.W = L;
    if (attention_core(qv, k.p, vt, ov, B, scores, probs, e->cfg.dtype, st, e->split)) return 1;
    trace_raw(e, "gemm", "vt", vt, B, 1, C, L, Lp, 0, nullptr);          // V^T [B][C][Lp]
    trace_raw(e, "gemm", "scores", scores, B, 1, L, L, Lp, 0, nullptr);  // [B][L][Lp]
    trace_raw(e, "softmax", "probs", probs, B, 1, L, Lp, Lp, 0, nullptr);  // (the padding columns [L, Lp) are written too: zeros)
    trace_tn(e, "gemm", "o", o, B);
  }
  // (the dry run must see this call too: it sizes the accumulator region)
  Conv co(o, PK(e, m.pk_nin[3]), C, 1);
  co.bias = P(e, m.nin_b[3]); co.res = &x; co.scale = kInvSqrt2; co.want_stats = true;
  return conv(e, co, out, B, st);
}

// NCSNpp.forward  ncsnpp.py:319-478.  x0: packed input AFTER 2x-1, [B,H,W,cpad_in]; y: [B,H,W,cpad_out]
// pyr_out != null: stop before the output layer and hand back the last pyramid tensor (the caller's iSTFT applies
// `output_layer(pyramid / t)` while unpacking)
static int net_forward(diffsep_engine* e, const Tn& x0, const float* t, const Tn& y, int B, hipStream_t st,
                       Tn* pyr_out = nullptr) {
  const Arch& A = e->arch;
  const diffsep_model_config& c = e->cfg;
  const int nf = c.nf;
  size_t mi = 0;
  e->trace_mod = -1;
  // (the module the forward enters, for option "trace")
  auto next = [&]() -> const Module& { e->trace_mod = (int)mi; return A.mods[mi++]; };
  // ---- time embedding (ncsnpp.py:324-343) and every block's Dense_0(act(temb)) (layerspp.py:311-312)
  float* emb = e_f32(e, (size_t)B * 2 * nf);
  float* t1 = e_f32(e, (size_t)B * 4 * nf);
  float* temb = e_f32(e, (size_t)B * 4 * nf);
  float* proj = e_f32(e, (size_t)B * A.dense_total);
  const Module& mf = A.mods[mi++];
  const Module& l1 = A.mods[mi++];
  const Module& l2 = A.mods[mi++];
  if (!e->dry) {
    if (ds_launch_fourier(t, P(e, mf.w0), emb, B, nf, st)) return 1;
    if (ds_launch_linear(emb, P(e, l1.w0), P(e, l1.b0), t1, B, 2 * nf, 4 * nf, 0, st)) return 1;
    if (ds_launch_linear(t1, P(e, l2.w0), P(e, l2.b0), temb, B, 4 * nf, 4 * nf, 1, st)) return 1;
    if (ds_launch_linear_t(temb, e->d_dense_w, e->d_dense_b, proj, B, 4 * nf, A.dense_total, 1, st)) return 1;
    trace_f32(e, "fourier", "emb", emb, B, 2 * nf);
    trace_f32(e, "linear", "t1", t1, B, 4 * nf);
    trace_f32(e, "linear", "temb", temb, B, 4 * nf);
    trace_f32(e, "linear", "proj", proj, B, A.dense_total);
  }
  // ---- input conv
  const Module& cin = A.mods[mi++];
  std::vector<Tn> hs;
  {
    Tn h = e_tensor(e, B, x0.H, x0.W, nf);
    Conv ci(x0, PK(e, cin.pk0), nf, 9);
    ci.bias = P(e, cin.b0); ci.want_stats = true; ci.role = "conv_in";
    e->trace_mod = (int)mi - 1;
    if (conv(e, ci, h, B, st)) return 1;
    hs.push_back(h);
  }
  Tn pyr_in = x0;
  const int L = c.n_levels;
  Tn h;
  for (int i = 0; i < L; ++i) {
    for (int k = 0; k < c.num_res_blocks; ++k) {
      if (res_block(e, next(), hs.back(), proj, B, h, st)) return 1;
      if (h.H == c.attn_resolution) {
        DS_CHECK(mi < A.mods.size() && A.mods[mi].kind == MK_ATTN, "attention placement mismatch (image height)");
        Tn ha;
        if (attn_block(e, next(), h, B, ha, st)) return 1;
        h = ha;
      }
      hs.push_back(h);
    }
    if (i != L - 1) {
      if (res_block(e, next(), hs.back(), proj, B, h, st)) return 1;
      // input pyramid: FIR down, Combine = conv1x1(pyr) + h   (ncsnpp.py:383-386, layerspp.py:52-57)
      Tn pd = e_tensor(e, B, pyr_in.H / 2, pyr_in.W / 2, pyr_in.C);
      const Module& cm = next();
      if (gn_apply(e, pyr_in, nullptr, nullptr, &pd, B, 0, 2, st)) return 1;
      trace_tn(e, "gn_apply", "pd", pd, B, ds_last_conv_kernel());
      pyr_in = pd;
      DS_CHECK(cm.kind == MK_COMBINE, "internal: expected Combine");
      Tn hc = e_tensor(e, B, h.H, h.W, h.C);
      Conv cc(pyr_in, PK(e, cm.pk0), h.C, 1);
      cc.bias = P(e, cm.b0); cc.res = &h; cc.want_stats = true; cc.role = "combine";
      if (conv(e, cc, hc, B, st)) return 1;
      hs.push_back(hc);
    }
  }
  h = hs.back();
  Tn t2;
  if (res_block(e, next(), h, proj, B, t2, st)) return 1;
  if (attn_block(e, next(), t2, B, h, st)) return 1;
  if (res_block(e, next(), h, proj, B, t2, st)) return 1;
  h = t2;

  Tn pyramid;
  bool have_pyr = false;
  for (int i = L - 1; i >= 0; --i) {
    for (int k = 0; k < c.num_res_blocks + 1; ++k) {
      const Tn s = hs.back();
      hs.pop_back();
      const Tn cat = cat_view(h, s);  // torch.cat([h, hs.pop()], dim=1) read in place (ncsnpp.py:411)
      Tn hn2;
      if (res_block(e, next(), cat, proj, B, hn2, st)) return 1;
      h = hn2;
    }
    if (h.H == c.attn_resolution) {
      DS_CHECK(mi < A.mods.size() && A.mods[mi].kind == MK_ATTN, "attention placement mismatch (image height)");
      Tn ha;
      if (attn_block(e, next(), h, B, ha, st)) return 1;
      h = ha;
    }
    // output pyramid (ncsnpp.py:419-440): conv3x3(act(GN(h))) [+ FIR up of the previous pyramid]
    const Module& g = A.mods[mi++];  // (GroupNorm of the pyramid head: no launch of its own)
    const Module& cv = next();
    DS_CHECK(g.kind == MK_GN && cv.kind == MK_CONV3, "internal: expected pyramid GN + conv");
    hipStream_t sp = st;  // (the pyramid chain on a side stream was measured 6 % slower: profiles/experiments)
    GnAff ga;
    if (gn_stats(e, h, P(e, g.w0), P(e, g.b0), B, ga, sp, true)) return 1;
    Tn pnew = e_tensor(e, B, h.H, h.W, A.cpad_in);
    Conv cp(h, PK(e, cv.pk0), A.chan_in, 9);
    cp.bias = P(e, cv.b0); cp.gn = &ga; cp.role = "pnew";
    Tn pu;
    if (have_pyr) {
      pu = e_tensor(e, B, h.H, h.W, A.cpad_in);
      if (gn_apply(e, pyramid, nullptr, nullptr, &pu, B, 0, 1, sp)) return 1;
      trace_tn(e, "gn_apply", "pu", pu, B, ds_last_conv_kernel());
      cp.res = &pu;
    }
    if (conv(e, cp, pnew, B, sp)) return 1;
    pyramid = pnew;
    have_pyr = true;
    if (i != 0) {
      Tn hu;
      if (res_block(e, next(), h, proj, B, hu, st)) return 1;
      h = hu;
    }
  }
  DS_CHECK(hs.empty() && mi == A.mods.size(), "internal: module walk did not consume all modules");
  // h = pyramid / t ; out = output_layer(h)   (ncsnpp.py:472-477)
  e->trace_mod = -1;
  if (pyr_out) { *pyr_out = pyramid; return 0; }
  Tn yy = y;
  Conv co(pyramid, PK(e, A.pk_out), A.chan_out, 1);
  co.bias = P(e, A.out_b); co.div_b = t; co.role = "y";
  return conv(e, co, yy, B, st);
}

// ScoreModelNCSNpp.forward  score_models.py:126-138
static int score_forward_impl(diffsep_engine* e, const float* xt, const float* t, const float* mix, float* out, int B,
                              long T, hipStream_t st) {
  const diffsep_model_config& c = e->cfg;
  const int W = diffsep_padded_frames(&c, T), H = c.n_fft / 2 + 1, S = c.num_sources;
  e->top = e->fwd_base;
  e->tracked.clear();
  if (stats_begin(e, st)) return 1;
  Tn x0 = e_tensor(e, B, H, W, e->arch.cpad_in);
  Tn y = e_tensor(e, B, H, W, e->arch.cpad_out);
  // the DFT GEMMs work on fp32 frames in every mode: exact fp32 MFMAs for the fp32 engine, bf16x3 products (4e-5, far
  // below the bf16 rounding of the packed spectrogram) for the split and the bf16 engine
  const int dft_split = e->split || c.dtype == DS_BF16;
  float* ws_f = (float*)e_alloc(e, (size_t)ds_stft_workspace_bytes(B, S, T, c.n_fft, c.hop));
  float* frames = (float*)e_alloc(e, (size_t)ds_istft_workspace_bytes(B, S, T, c.n_fft, c.hop));
  const double esz_t = c.dtype == DS_F32 ? 4.0 : 2.0;
  if (!e->dry && !(e->ablate & 128u))
    if (prof_launch(e, st, hbm_rec("stft (frame + real-DFT GEMM + compress / pack)",
                                   4.0 * B * (S + 1) * (double)T + esz_t * B * H * (double)W * e->arch.cpad_in, B, H, W, e->arch.cpad_in), [&]() {
          return ds_launch_stft_pack(xt, mix, x0.p, B, S, T, c.n_fft, c.hop, c.spec_abs_exponent, c.spec_factor, W,
                                     e->arch.cpad_in, 1, c.dtype, e->d_tab, ws_f, st, dft_split);
        }))
      return 1;
  trace_tn(e, "stft", "x0", x0, B);
  Tn pyr;
  if (net_forward(e, x0, t, y, B, st, &pyr)) return 1;
  if (!e->dry && !(e->ablate & 128u))
    if (prof_launch(e, st, hbm_rec("istft (unpack / decompress + inverse-DFT GEMM + overlap-add)",
                                   esz_t * B * H * (double)W * pyr.ld + 4.0 * B * S * (double)T, B, H, W, pyr.ld), [&]() {
          return ds_launch_istft(pyr.p, out, B, S, T, c.n_fft, c.hop, c.spec_abs_exponent, c.spec_factor, W, pyr.ld, c.dtype,
                                 e->d_tab, frames, st, dft_split, P(e, e->arch.out_w), P(e, e->arch.out_b), t, e->arch.chan_in);
        }))
      return 1;
  return 0;
}

// ------------------------------------------------------------------ plans and their captured graphs
static void destroy_graph(diffsep_engine::GraphRec& r) {
  if (r.x) hipGraphExecDestroy(r.x);
  if (r.g) hipGraphDestroy(r.g);
  r.x = nullptr; r.g = nullptr;
}
// Forget every captured graph (the arena moved, graphs were switched off, the engine goes away).  The caller has made sure
// that none of them is still executing.
static void drop_graph(diffsep_engine* e) {
  for (auto& kv : e->graphs) destroy_graph(kv.second);
  e->graphs.clear();
  e->cur_graph = nullptr;
}

// The sampler state at the bottom of the arena (a dry run sizes it, like a forward)
static void layout_state(diffsep_engine* e, int B, long T) {
  const size_t nst = (size_t)B * e->cfg.num_sources * T;
  e->top = 0;
  e->st_x = (float*)e_alloc(e, nst * 4);
  e->st_xm = (float*)e_alloc(e, nst * 4);
  e->st_score = (float*)e_alloc(e, nst * 4);
  e->st_noise = (float*)e_alloc(e, nst * 4);
  e->st_t = (float*)e_alloc(e, (size_t)B * 4);
  e->st_mix = (float*)e_alloc(e, (size_t)B * T * 4);
  e->st_smix = (float*)e_alloc(e, (size_t)B * T * 4);
  e->st_ts = (float*)e_alloc(e, 4096 * (size_t)B * 4);
  e->st_lang = (float*)e_alloc(e, 16 * (size_t)B + 64);
  e->st_lens = (int*)e_alloc(e, (size_t)B * 4);
  e->st_seeds = (unsigned long long*)e_alloc(e, (size_t)B * 8);
}

// Size the arena for (B, T): sampler state + one forward's bump allocations.
int ensure_plan(diffsep_engine* e, int B, long T, hipStream_t st) {
  if (e->planB == B && e->planT == T && e->arena) return 0;
  DS_CHECK(B >= 1 && T >= 1, "empty batch or signal");
  // a plan seen before keeps its captured graph (one per (B, T): evaluate / separate alternate between a few widths and
  // the short last batch of each); only the layout and the zero padding of the arena are re-established below
  e->cur_graph = nullptr;
  e->planB = -1;  // (no plan until this one stands: the state pointers are about to change)
  e->planT = -1;
  e->dry = true;
  layout_state(e, B, T);
  e->fwd_base = (e->top + 255) & ~(size_t)255;
  const int rc = score_forward_impl(e, nullptr, nullptr, nullptr, nullptr, B, T, st);
  e->dry = false;
  if (rc) return 1;
  const size_t need = e->top + e->stats_need + 8192;
  if (need > e->cap) {
    DS_HIP(hipStreamSynchronize(st));
    drop_graph(e);  // their addresses die with the old arena (nothing is in flight after the synchronisation)
    if (e->arena) DS_HIP(hipFree(e->arena));
    e->tracked.clear();  // (track_tensors: those pointers were into the old arena)
    e->arena = nullptr;
    e->cap = 0;
    // (hipFree / hipMalloc synchronise the whole device: grow with headroom so that a stream of utterances of
    // slowly increasing length does not reallocate — and stall every other stream — at each new maximum)
    const size_t grown = e->had_arena ? need + need / 4 : need;
    DS_HIP(hipMalloc((void**)&e->arena, grown));
    e->cap = grown;
    e->had_arena = true;
  }
  DS_HIP(hipMemsetAsync(e->arena, 0, e->cap, st));  // channel / K padding must read as zero
  layout_state(e, B, T);
  e->planB = B;
  e->planT = T;
  {
    auto it = e->graphs.find(std::make_pair(B, T));
    if (it != e->graphs.end()) {
      e->cur_graph = &it->second;
      it->second.used = ++e->graph_tick;
    }
  }
  e->ts_dev.clear();
  // a new plan is captured at its first score evaluation (hipFuncSetAttribute inside the launchers is not a stream
  // operation and is legal during capture)
  e->warmed = true;
  return 0;
}

int run_nfe(diffsep_engine* e, int B, long T, hipStream_t st) {
  // one score evaluation on the resident state: (st_x, st_t, st_mix) -> st_score
  if (e->use_graph && e->warmed && !e->prof) {
    if (!e->cur_graph) {
      DS_HIP(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
      const int rc = score_forward_impl(e, e->st_x, e->st_t, e->st_mix, e->st_score, B, T, st);
      diffsep_engine::GraphRec r{nullptr, nullptr, 0};
      const hipError_t ce = hipStreamEndCapture(st, &r.g);
      if (rc || ce != hipSuccess || !r.g) {
        destroy_graph(r);
        e->use_graph = 0;  // fall back to eager launches of the same kernels
        if (rc) return 1;
      } else {
        const hipError_t ie = hipGraphInstantiate(&r.x, r.g, nullptr, nullptr, 0);
        if (ie != hipSuccess) destroy_graph(r);
        DS_HIP(ie);
        if ((int)e->graphs.size() >= e->graph_cap) {  // evict the least recently used plan's graph
          // (its last replay may still be running — on this stream or, if the engine was driven from another stream in an
          // earlier call, on that one: eviction is rare, wait for the device before destroying the executable)
          const hipError_t se = hipDeviceSynchronize();
          if (se != hipSuccess) destroy_graph(r);
          DS_HIP(se);
          while ((int)e->graphs.size() >= e->graph_cap) {
            auto lru = e->graphs.begin();
            for (auto it = e->graphs.begin(); it != e->graphs.end(); ++it)
              if (it->second.used < lru->second.used) lru = it;
            destroy_graph(lru->second);
            e->graphs.erase(lru);
          }
        }
        r.used = ++e->graph_tick;
        e->cur_graph = &(e->graphs[std::make_pair(B, (long)T)] = r);
      }
    }
    if (e->cur_graph) {
      DS_HIP(hipGraphLaunch(e->cur_graph->x, st));
      return 0;
    }
  }
  const int rc = score_forward_impl(e, e->st_x, e->st_t, e->st_mix, e->st_score, B, T, st);
  e->warmed = true;  // the first eager pass also sets the kernels' LDS attributes (not capturable)
  return rc;
}

// ------------------------------------------------------------------ engine life cycle, options, profiling
extern "C" int32_t diffsep_engine_create(const diffsep_model_config* cfg, const float* weights_host, int64_t n_floats,
                                         diffsep_engine** out) {
  DS_CHECK(cfg && weights_host && out, "engine_create: null argument");
  DS_CHECK(cfg->dtype == DS_F32 || cfg->dtype == DS_BF16 || cfg->dtype == DS_F32_SPLIT,
           "engine_create: dtype must be DIFFSEP_F32, DIFFSEP_BF16 or DIFFSEP_F32_SPLIT");
  std::unique_ptr<diffsep_engine> e(new diffsep_engine());  // (every early return below releases what the engine holds by then)
  e->cfg = *cfg;
  const DtypeSplit ds = split_dtype(cfg->dtype);  // storage and every non-MFMA kernel of a split engine: plain fp32
  e->cfg.dtype = ds.dtype; e->split = ds.split;
  // fragment-major weight copies only for the kernels this engine can dispatch to (an exact-fp32 engine: none)
  if (build_arch(e->cfg, e->arch, e->cfg.dtype == DS_BF16 ? 1 : (e->split ? 2 : 0))) return 1;
  const Arch& A = e->arch;
  if (upload_weights(e.get(), weights_host, n_floats, "engine_create: weight blob")) return 1;
  e->weight_bytes = (int64_t)A.total * 4 + (int64_t)A.pack_total * e->esz + (int64_t)A.dense_total * (4 * cfg->nf + 1) * 4;
  if (ds_build_stft_table(cfg->n_fft, &e->d_tab)) return 1;
  if (const char* sv = getenv("DIFFSEP_DBG_ALLOC")) e->dbg_alloc = atoi(sv) != 0;  // (read once, at creation)
  e->opts = ds_default_opts();
  DS_HIP(hipEventCreateWithFlags(&e->ev_in, hipEventDisableTiming));
  DS_HIP(hipEventCreateWithFlags(&e->ev_out, hipEventDisableTiming));
  *out = e.release();
  return 0;
}

diffsep_engine::~diffsep_engine() {
  drop_graph(this);
  hipFree(d_blob); hipFree(d_pack); hipFree(d_dense_w); hipFree(d_dense_b); hipFree(d_attn_b); hipFree(d_tab);
  hipFree(arena); hipFree(ode_buf);  // (hipFree(null) is a no-op)
  if (own) hipStreamDestroy(own);
  if (ev_in) hipEventDestroy(ev_in);
  if (ev_out) hipEventDestroy(ev_out);
  for (auto& r : prof_recs) { hipEventDestroy(r.a); hipEventDestroy(r.b); }  // (a span that profile_end never closed)
  for (hipEvent_t v : ev_pool) hipEventDestroy(v);
}
extern "C" void diffsep_engine_destroy(diffsep_engine* e) { delete e; }
extern "C" int32_t diffsep_engine_reserve(diffsep_engine* e, int32_t B, int64_t T, void* stream) {
  DS_CHECK(e && B >= 1 && T >= 1, "reserve: bad argument");
  // size the workspace for a B x T batch now: plans of that size or smaller never reallocate afterwards
  // (hipFree / hipMalloc synchronise the whole device, i.e. every other stream's work)
  // (on the caller's stream — the null stream included: no private stream is created here, see StreamScope)
  hipStream_t st = (hipStream_t)stream;
  if (ensure_plan(e, B, T, st)) return 1;
  DS_HIP(hipStreamSynchronize(st));  // the workspace is zeroed before any other stream may use the plan
  return 0;
}
// Largest finite |value| and number of non-finite values of every activation tensor of the LAST eager forward (option
// "track_tensors" on): out[i] = {max |v|, non-finite count, H, C} for tensor i in allocation order.  Debug / test aid.
__global__ __launch_bounds__(256) void absmax_kernel(const void* __restrict__ p, long n, int f32, unsigned* __restrict__ out) {
  float m = 0.f;
  unsigned bad = 0;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const float v = f32 ? reinterpret_cast<const float*>(p)[i] : h2f(reinterpret_cast<const bf16_t*>(p)[i]);
    if (v != v || fabsf(v) > 3.0e38f) ++bad; else m = fmaxf(m, fabsf(v));
  }
  atomicMax(out, __float_as_uint(m));
  if (bad) atomicAdd(out + 1, bad);
}
extern "C" int32_t diffsep_engine_debug_absmax(diffsep_engine* e, double* out, int32_t cap, int32_t* n) {
  DS_CHECK(e && n, "debug_absmax: null argument");
  *n = (int32_t)e->tracked.size();
  if (!out || cap <= 0) return 0;
  const int cnt = *n < cap ? *n : cap;
  unsigned* d = nullptr;
  DS_HIP(hipMalloc(&d, (size_t)cnt * 8 + 8));
  DS_HIP(hipMemset(d, 0, (size_t)cnt * 8 + 8));
  for (int i = 0; i < cnt; ++i) {
    const auto& t = e->tracked[i];
    long nb = (t.n + 255) / 256;
    if (nb > 1024) nb = 1024;
    hipLaunchKernelGGL(absmax_kernel, dim3((unsigned)nb), dim3(256), 0, nullptr, t.p, t.n, e->cfg.dtype == DS_F32 ? 1 : 0, d + 2 * i);
  }
  std::vector<unsigned> hbuf((size_t)cnt * 2);
  DS_HIP(hipDeviceSynchronize());
  DS_HIP(hipMemcpy(hbuf.data(), d, (size_t)cnt * 8, hipMemcpyDeviceToHost));
  hipFree(d);
  for (int i = 0; i < cnt; ++i) {
    float m;
    memcpy(&m, &hbuf[2 * i], 4);
    out[4 * i] = m; out[4 * i + 1] = hbuf[2 * i + 1]; out[4 * i + 2] = e->tracked[i].H; out[4 * i + 3] = e->tracked[i].C;
  }
  return 0;
}
extern "C" int32_t diffsep_engine_debug_arena(const diffsep_engine* e, void** base, int64_t* bytes, int64_t* fwd_base) {
  DS_CHECK(e && base && bytes && fwd_base, "debug_arena: null argument");
  *base = e->arena; *bytes = (int64_t)e->cap; *fwd_base = (int64_t)e->fwd_base;
  return 0;
}
extern "C" int32_t diffsep_engine_debug_trace(const diffsep_engine* e, int64_t* fields, char* names, int32_t cap, int32_t* n) {
  DS_CHECK(e && n, "debug_trace: null argument");
  *n = (int32_t)e->trace.size();
  const long long sb = e->stats_ptr && e->arena ? (long long)(e->stats_ptr - e->arena) : 0;
  for (int i = 0; i < *n && i < cap; ++i) {
    const auto& r = e->trace[i];
    if (fields) {
      const int64_t v[DIFFSEP_TRACE_FIELDS] = {r.mod, r.B, r.H, r.W, r.C, r.ld, r.f32, r.off, r.stats_off >= 0 ? sb + r.stats_off : -1};
      memcpy(fields + (size_t)DIFFSEP_TRACE_FIELDS * i, v, sizeof(v));
    }
    if (names) {
      char* o = names + (size_t)DIFFSEP_TRACE_NAME_BYTES * i;
      memset(o, 0, DIFFSEP_TRACE_NAME_BYTES);
      snprintf(o, 16, "%s", r.kind);
      snprintf(o + 16, 16, "%s", r.role);
      snprintf(o + 32, DIFFSEP_TRACE_NAME_BYTES - 32, "%s", r.kernel.c_str());
    }
  }
  return 0;
}
extern "C" int64_t diffsep_engine_device_bytes(const diffsep_engine* e) {
  return e ? e->weight_bytes + (int64_t)e->cap + (int64_t)e->ode_cap : 0;
}
extern "C" int32_t diffsep_engine_set_graph(diffsep_engine* e, int32_t enable) {
  DS_CHECK(e, "null engine");
  e->use_graph = enable;
  if (!enable) drop_graph(e);
  return 0;
}

extern "C" int32_t diffsep_engine_set_option(diffsep_engine* e, const char* name, int64_t value) {
  DS_CHECK(e && name, "engine_set_option: null argument");
  unsigned bit = 0;
  if (!strcmp(name, "graph_cache")) {
    DS_CHECK(value >= 1 && value <= 4096, "engine_set_option: graph_cache must be in [1, 4096]");
    e->graph_cap = (int)value;
  } else if (!strcmp(name, "ablate")) {
    e->ablate = (unsigned)value;
  } else if (!strcmp(name, "dbg_alloc")) {
    e->dbg_alloc = value != 0;
    return 0;  // (a log switch: no launch decision depends on it)
  } else if (!strcmp(name, "no_stft_fused")) {
    // stft.hip reads the PROCESS default (ds_default_opts): an engine-level value would be accepted and do nothing
    ds_set_error("engine_set_option: 'no_stft_fused' is a process-level option (diffsep_set_option / DIFFSEP_NO_STFT_FUSED)");
    return 1;
  } else if (!strcmp(name, "trace")) {  // (host bookkeeping: no launch decision depends on it, plans and graphs stay)
    e->trace_on = value != 0;
    e->trace.clear();
    return 0;
  } else if (!strcmp(name, "track_tensors")) {
    e->track_tensors = value != 0;
    e->tracked.clear();
    return 0;
  } else if (!opt_bit(name, &bit)) {
    e->opts = value ? (e->opts | bit) : (e->opts & ~bit);
  } else {
    ds_set_error(std::string("engine_set_option: unknown option '") + name + "'");
    return 1;
  }
  // the captured graphs froze the old launch decisions (and the cache may now be over its cap): forget them all — and the plan:
  // a dispatch switch may change what a forward allocates (tensors, GroupNorm accumulators), so the next call sizes it again
  DS_HIP(hipDeviceSynchronize());
  drop_graph(e);
  e->planB = -1;
  e->planT = -1;
  return 0;
}
extern "C" int64_t diffsep_engine_get_option(const diffsep_engine* e, const char* name) {
  if (!e || !name) return -1;
  unsigned bit = 0;
  if (!strcmp(name, "graph_cache")) return e->graph_cap;
  if (!strcmp(name, "graphs_cached")) return (int64_t)e->graphs.size();
  if (!strcmp(name, "ablate")) return e->ablate;
  if (!strcmp(name, "trace")) return e->trace_on ? 1 : 0;
  if (!opt_bit(name, &bit)) return (e->opts & bit) ? 1 : 0;
  return -1;
}

// Per-launch timing of the MFMA contraction kernels inside the real launch sequence: between profile_begin and profile_end every
// conv/GEMM launch is bracketed by HIP events on its stream (graph replay is bypassed meanwhile).  The arrays are indexed by
// kernel class (DS_CLS_*, common.h).  flops = algorithmic 2*taps*Cin*Cout*H*W*B (unpadded).
extern "C" int32_t diffsep_engine_profile_begin(diffsep_engine* e) {
  DS_CHECK(e, "null engine");
  e->prof = true;
  e->prof_recs.clear();
  return 0;
}
static_assert(DS_NCLS == DIFFSEP_NUM_KERNEL_CLASSES, "header and engine agree on the number of kernel classes");
extern "C" int32_t diffsep_num_kernel_classes(void) { return DS_NCLS; }
extern "C" int32_t diffsep_engine_profile_end(diffsep_engine* e, double* flops, double* ms, int64_t* launches,
                                               double* bytes) {
  return diffsep_engine_profile_end_n(e, DS_NCLS, flops, ms, launches, bytes, nullptr);
}
extern "C" int32_t diffsep_engine_profile_end_n(diffsep_engine* e, int32_t n_classes, double* flops, double* ms,
                                                 int64_t* launches, double* bytes, int32_t* n_written) {
  DS_CHECK(e && flops && ms && launches && n_classes >= 0, "profile_end: null argument");
  DS_HIP(hipDeviceSynchronize());
  const int ncls = n_classes < DS_NCLS ? n_classes : DS_NCLS;
  if (n_written) *n_written = ncls;
  for (int i = 0; i < ncls; ++i) { flops[i] = 0; ms[i] = 0; launches[i] = 0; if (bytes) bytes[i] = 0; }
  e->prof_done.clear();
  for (auto& r : e->prof_recs) {
    float t = 0.f;
    hipEventElapsedTime(&t, r.a, r.b);
    r.ms = t;
    e->prof_done.push_back(r);
    if (r.cls >= 0 && r.cls < ncls) {  // (cls -1: the HBM-bound launches, reported through profile_records only)
      flops[r.cls] += r.flops;
      if (bytes) bytes[r.cls] += r.bytes;
      ms[r.cls] += t;
      launches[r.cls] += 1;
    }
    e->ev_pool.push_back(r.a);
    e->ev_pool.push_back(r.b);
  }
  e->prof_recs.clear();
  e->prof = false;
  return 0;
}

// The launches of the last profile_begin .. profile_end span one by one (call after profile_end): kernel instantiation
// with its template arguments, problem shape, algorithmic flops / bytes, duration.
extern "C" int32_t diffsep_engine_profile_records(diffsep_engine* e, diffsep_prof_record* out, int32_t cap, int32_t* n) {
  DS_CHECK(e && n, "profile_records: null argument");
  *n = (int32_t)e->prof_done.size();
  if (!out) return 0;
  for (int i = 0; i < *n && i < cap; ++i) {
    const auto& r = e->prof_done[i];
    diffsep_prof_record& o = out[i];
    memset(&o, 0, sizeof(o));
    snprintf(o.kernel, sizeof(o.kernel), "%s", r.kernel ? r.kernel : "");
    o.B = r.B; o.H = r.H; o.W = r.W; o.Cin = r.Cin; o.Cout = r.Cout; o.taps = r.taps; o.skip_cin = r.sCin; o.has_res = r.res;
    o.cls = r.cls; o.flops = r.flops; o.bytes = r.bytes; o.ms = r.ms;
  }
  return 0;
}

// option "trace": the records of the forward that begins here replace the last one's; nothing else records (run_nfe, capture)
struct TraceScope {
  diffsep_engine* e;
  explicit TraceScope(diffsep_engine* e_) : e(e_) { e->trace.clear(); e->trace_mod = -1; e->tracing = e->trace_on; }
  ~TraceScope() { e->tracing = false; }
};
extern "C" int32_t diffsep_score_forward(diffsep_engine* e, const float* xt, const float* t, const float* mix,
                                         float* out, int32_t B, int64_t T, void* stream) {
  DS_CHECK(e && xt && t && mix && out, "score_forward: null argument");
  StreamScope sc_(e, stream);
  hipStream_t st = sc_.st;
  if (ensure_plan(e, B, T, st)) return 1;
  const TraceScope ts_(e);
  return score_forward_impl(e, xt, t, mix, out, B, T, st);
}

extern "C" int32_t diffsep_backbone_forward(diffsep_engine* e, const void* x, const float* t, void* y, int32_t B,
                                            int32_t W, void* stream) {
  DS_CHECK(e && x && t && y, "backbone_forward: null argument");
  DS_CHECK(W >= 64 && W % 64 == 0, "backbone_forward: W must be a positive multiple of 64");
  StreamScope sc_(e, stream);
  hipStream_t st = sc_.st;
  // plan sized through the equivalent signal length: F = W frames  <=>  T = (W-1)*hop - (n_fft-hop) + hop - 1
  const long T = (long)(W - 1) * e->cfg.hop - (e->cfg.n_fft - e->cfg.hop) + e->cfg.hop - 1;
  DS_CHECK(diffsep_padded_frames(&e->cfg, T) == W, "internal: width/length mapping");
  if (ensure_plan(e, B, T, st)) return 1;
  const int H = e->cfg.n_fft / 2 + 1;
  const TraceScope ts_(e);
  e->top = e->fwd_base;
  if (stats_begin(e, st)) return 1;
  Tn xin; xin.p = (void*)x; xin.C = xin.ld = e->arch.cpad_in; xin.H = H; xin.W = W;
  Tn x0 = e_tensor(e, B, H, W, e->arch.cpad_in);
  float* sc = e_f32(e, (size_t)B * e->arch.cpad_in);
  float* sh = e_f32(e, (size_t)B * e->arch.cpad_in);
  if (ds_launch_fill(sc, 2.f, (long)B * e->arch.cpad_in, st)) return 1;
  if (ds_launch_fill(sh, -1.f, (long)B * e->arch.cpad_in, st)) return 1;
  GnAff aff{sc, sh};
  if (gn_apply(e, xin, &aff, &x0, nullptr, B, 0, 0, st)) return 1;  // x = 2x - 1 (ncsnpp.py:347-349)
  trace_tn(e, "gn_apply", "x0", x0, B, ds_last_conv_kernel());
  Tn yo; yo.p = y; yo.C = yo.ld = e->arch.cpad_out; yo.H = H; yo.W = W;
  return net_forward(e, x0, t, yo, B, st);
}
