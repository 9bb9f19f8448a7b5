// Nature-CNN policy/value tower on gfx950: forward, backward fused with the
// K-FAC input-factor statistics, and the sampled-loss output statistics.
//
// Reference: envs/atari/model.py:77-217 (graph), :219-246 (K-FAC layer
// registration), nn.py:37-126 (layer math), policies.py:146-158 and
// baselines.py:55-69 (predictive distributions), objectives.py:78 (the
// tf.gradients of the shared loss).  See include/acmi.h for the contract.
#include <math.h>
#include <stdlib.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <atomic>
#include <vector>

#include "gemm.hpp"
#include "gemm3.hpp"
#include "conv1u8.hpp"
#include "convt3.hpp"
#include "convfwd3.hpp"
#include "band.hpp"
#include "tower.hpp"
#include "fc4roll.hpp"
#include "convt2.hpp"
#include "stepper.hpp"
#include "towersplit.hpp"

namespace acmi {

// Arithmetic modes.  Process-wide defaults (acmi_set_*_mode; initial values from
// the environment) and the modes in effect for the calling thread's current
// entry point: a net's own (acmi_net_t gemm_mode / forward_mode /
// conv_stats_mode, each mode + 1) or the defaults (ModeScope).
//   gemm:  ACMI_GEMM_X3 = 16-bit split operands (f16x2 / bf16x3, f32-accurate),
//          ACMI_GEMM_F32 = v_mfma_f32_32x32x2_f32; ACMI_GEMM ("f32" / "x3"), default x3
//   conv stats: pixel-pair band reduction (band.hpp, x3 only) or patch rows; ACMI_BAND ("0": patches)
//   forward: the conv tower's precision; ACMI_FORWARD ("bf16" / "f32")
static int s_gemm_mode = [] {
  const char* e = getenv("ACMI_GEMM");
  return (e && e[0] == 'f') ? ACMI_GEMM_F32 : ACMI_GEMM_X3;
}();
static int s_conv_stats_mode = [] {
  const char* e = getenv("ACMI_BAND");
  return (e && e[0] == '0') ? ACMI_CONV_STATS_PATCHES : ACMI_CONV_STATS_BAND;
}();
static int s_forward_mode = [] {
  const char* e = getenv("ACMI_FORWARD");
  return (e && e[0] == 'b') ? ACMI_FWD_BF16 : ACMI_FWD_F32;
}();
thread_local int g_gemm_mode = s_gemm_mode;
thread_local int g_conv_stats_mode = s_conv_stats_mode;
thread_local int g_forward_mode = s_forward_mode;

// a net's mode fields (0: the process default) are valid
static bool net_modes_ok(const acmi_net_t* n) {
  if (!n) return true;
  const int g = n->gemm_mode ? n->gemm_mode - 1 : s_gemm_mode;
  const int f = n->forward_mode ? n->forward_mode - 1 : s_forward_mode;
  const int c = n->conv_stats_mode ? n->conv_stats_mode - 1 : s_conv_stats_mode;
  return (g == ACMI_GEMM_F32 || g == ACMI_GEMM_X3) && (f == ACMI_FWD_F32 || f == ACMI_FWD_BF16) &&
         (c == ACMI_CONV_STATS_PATCHES || c == ACMI_CONV_STATS_BAND) && (f == ACMI_FWD_F32 || g == ACMI_GEMM_X3);
}
// the modes of one entry point's call, restored when it returns (thread-local:
// calls on different threads with different nets do not interfere)
struct ModeScope {
  int g, f, c;
  explicit ModeScope(const acmi_net_t* n) : g(g_gemm_mode), f(g_forward_mode), c(g_conv_stats_mode) {
    g_gemm_mode = n && n->gemm_mode ? n->gemm_mode - 1 : s_gemm_mode;
    g_forward_mode = n && n->forward_mode ? n->forward_mode - 1 : s_forward_mode;
    g_conv_stats_mode = n && n->conv_stats_mode ? n->conv_stats_mode - 1 : s_conv_stats_mode;
  }
  ~ModeScope() {
    g_gemm_mode = g;
    g_forward_mode = f;
    g_conv_stats_mode = c;
  }
};

static thread_local char g_err[512];
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

// ---------------------------------------------------------------------------
// launch-site profiling: HIP events recorded on the launch stream around one
// chosen kernel (acmi_prof_enable), summed by acmi_prof_collect.
// ---------------------------------------------------------------------------
static int g_prof_site = 0;
static int g_prof_cap = 0;
static int g_prof_n = 0;
static hipEvent_t* g_prof_ev = nullptr;  // 2 * cap events

static void prof_begin(int site, hipStream_t s) {
  if (site != g_prof_site || g_prof_n >= g_prof_cap) return;
  (void)hipEventRecord(g_prof_ev[2 * g_prof_n], s);
}
static void prof_end(int site, hipStream_t s) {
  if (site != g_prof_site || g_prof_n >= g_prof_cap) return;
  (void)hipEventRecord(g_prof_ev[2 * g_prof_n + 1], s);
  ++g_prof_n;
}

// ---------------------------------------------------------------------------
// layout
// ---------------------------------------------------------------------------
struct Layout {
  int A, C3;
  long long off[12];  // W, b per layer
  long long total;
  long long K[6], N[6];
  long long din[6], dout[6];
  long long stat_off[11], stat_total;
  long long rows_per_img[6];  // output locations per image (conv L, fc 1)
};

static bool make_layout(int A, int C3, Layout* L) {
  if (A < 1 || A > 64 || (C3 != 32 && C3 != 64)) return false;
  L->A = A;
  L->C3 = C3;
  const long long K[6] = {8 * 8 * 4, 4 * 4 * 32, 3 * 3 * 64, 49LL * C3, 512, 512};
  const long long N[6] = {32, 64, C3, 512, A, 1};
  const long long R[6] = {400, 81, 49, 1, 1, 1};
  long long o = 0;
  for (int l = 0; l < 6; ++l) {
    L->K[l] = K[l];
    L->N[l] = N[l];
    L->din[l] = K[l] + 1;
    L->dout[l] = N[l];
    L->rows_per_img[l] = R[l];
    L->off[2 * l] = o;
    o += K[l] * N[l];
    L->off[2 * l + 1] = o;
    o += N[l];
  }
  L->total = o;
  long long s = 0;
  for (int f = 0; f < 5; ++f) {
    L->stat_off[f] = s;
    s += L->din[f] * L->din[f];
  }
  for (int l = 0; l < 6; ++l) {
    L->stat_off[5 + l] = s;
    s += L->dout[l] * L->dout[l];
  }
  L->stat_total = s;
  return true;
}

bool get_layout(int A, int C3, Layout* L) { return make_layout(A, C3, L); }

// ---------------------------------------------------------------------------
// small helpers
// ---------------------------------------------------------------------------
// acmi_acts_t's masks: all three or none
static bool masks_ok(const acmi_acts_t* a) { return (a->m1 && a->m2 && a->m3) || (!a->m1 && !a->m2 && !a->m3); }

inline int roundup4(int x) { return (x + 3) & ~3; }

}  // namespace acmi

#include "forward.hpp"  // the forward: its kernels, fc4's split plan, the heads / tail launcher, forward_dispatch
#include "splitk.hpp"  // the split-K reduction: finalizes, plans, wgrad_layer / gcov_layer, workspace sizes

#include "backward.hpp"  // the update's backward: argument check, workspace views, dX chains, wgrad / G factors

using namespace acmi;

extern "C" {

const char* acmi_last_error(void) { return g_err; }
int acmi_abi_version(void) { return ACMI_ABI_VERSION; }
int acmi_abi_struct_sizes(int64_t* sizes, int n) {
  const int64_t all[5] = {(int64_t)sizeof(acmi_net_t), (int64_t)sizeof(acmi_acts_t), (int64_t)sizeof(acmi_bwd_t),
                          (int64_t)sizeof(acmi_env_state_t), (int64_t)sizeof(acmi_rollout_io_t)};
  if (!sizes || n < 0) return 0;
  const int k = n < 5 ? n : 5;
  for (int i = 0; i < k; ++i) sizes[i] = all[i];
  return k;
}

int acmi_set_gemm_mode(int mode) {
  ACMI_REQUIRE(mode == ACMI_GEMM_F32 || mode == ACMI_GEMM_X3, ACMI_ERR_ARG,
               "acmi_set_gemm_mode: unknown mode %d", mode);
  ACMI_REQUIRE(mode == ACMI_GEMM_X3 || s_forward_mode == ACMI_FWD_F32, ACMI_ERR_ARG,
               "acmi_set_gemm_mode: f32 gemm mode has no bf16 forward (acmi_set_forward_mode(ACMI_FWD_F32) first)");
  s_gemm_mode = g_gemm_mode = mode;
  return ACMI_OK;
}
int acmi_get_gemm_mode(void) { return s_gemm_mode; }

int acmi_set_forward_mode(int mode) {
  ACMI_REQUIRE(mode == ACMI_FWD_F32 || mode == ACMI_FWD_BF16, ACMI_ERR_ARG, "acmi_set_forward_mode: bad mode %d",
               mode);
  // the bf16 arithmetic exists only in the fused tower (tower.hpp): refuse a mode
  // the forward could not honour instead of silently computing in f32
  ACMI_REQUIRE(mode == ACMI_FWD_F32 || s_gemm_mode == ACMI_GEMM_X3, ACMI_ERR_ARG,
               "acmi_set_forward_mode: bf16 forward needs the fused tower (x3 gemm mode)");
  s_forward_mode = g_forward_mode = mode;
  return ACMI_OK;
}
int acmi_get_forward_mode(void) { return s_forward_mode; }

int acmi_set_conv_stats_mode(int mode) {
  ACMI_REQUIRE(mode == ACMI_CONV_STATS_PATCHES || mode == ACMI_CONV_STATS_BAND, ACMI_ERR_ARG,
               "acmi_set_conv_stats_mode: unknown mode %d", mode);
  s_conv_stats_mode = g_conv_stats_mode = mode;
  return ACMI_OK;
}
int acmi_get_conv_stats_mode(void) { return s_conv_stats_mode; }


int acmi_band_info(int layer, int C3, int64_t rows, int64_t* info) {
  ACMI_REQUIRE(info && (layer == 1 || layer == 2) && (C3 == 32 || C3 == 64) && rows > 0, ACMI_ERR_ARG,
               "acmi_band_info: bad arguments");
  const BandPlan* p = layer == 1 ? band_host_plan(20, 20, 32, 4, 4, 2, 64) : band_host_plan(9, 9, 64, 3, 3, 1, C3);
  ACMI_REQUIRE(p, ACMI_ERR_ARG, "acmi_band_info: no plan");
  int nc, ch;
  band_chunks(rows, (int)p->groups.size(), &nc, &ch);
  info[0] = p->ntiles;
  info[1] = (int64_t)p->groups.size();
  info[2] = nc;
  info[3] = ch;
  int units = 0;
  for (const BandGroup& G : p->groups) {
    int t = 0;
    for (int w = 0; w < 8; ++w) t += (G.ra[w][0] >= 0) + (G.ra[w][1] >= 0);
    units += (t + 3) / 4;
  }
  info[4] = units;  // sum over groups of the busiest SIMD's sub-tiles
  return ACMI_OK;
}

int64_t acmi_param_count(int A, int C3) {
  Layout L;
  if (!make_layout(A, C3, &L)) return -1;
  return L.total;
}

int acmi_param_offsets(int A, int C3, int64_t* off) {
  Layout L;
  ACMI_REQUIRE(off && make_layout(A, C3, &L), ACMI_ERR_ARG, "bad A=%d/C3=%d", A, C3);
  for (int i = 0; i < 12; ++i) off[i] = L.off[i];
  return ACMI_OK;
}

int acmi_kfac_layout(int A, int C3, int64_t* din, int64_t* dout, int64_t* so, int64_t* total) {
  Layout L;
  ACMI_REQUIRE(make_layout(A, C3, &L), ACMI_ERR_ARG, "bad A=%d/C3=%d", A, C3);
  for (int l = 0; l < 6; ++l) {
    if (din) din[l] = L.din[l];
    if (dout) dout[l] = L.dout[l];
  }
  for (int f = 0; f < 11; ++f)
    if (so) so[f] = L.stat_off[f];
  if (total) *total = L.stat_total;
  return ACMI_OK;
}

int64_t acmi_conv_prep_bytes(int C3) {
  if (C3 != 32 && C3 != 64) return -1;
  return dispatch_c3(C3, [](auto c3) { return (int64_t)PrepView<decltype(c3)::value>::bytes(); });
}

// two zeroed runs of 16-byte words in one launch
__global__ __launch_bounds__(256) void zero2_kernel(uint4* a, long long na, uint4* b, long long nb) {
  const uint4 z = make_uint4(0u, 0u, 0u, 0u);
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < na + nb; i += (long long)gridDim.x * 256) {
    if (i < na) a[i] = z;
    else b[i - na] = z;
  }
}

// acmi_conv_prepare's two dependent passes, each one launch over block ranges:
//   bounds: the tower's header (tower_stats_body, 64 blocks) and max |W2| of conv2's
//     input-gradient weights (convt2_wmax_body, kPrepWmaxBlocks), atomicMax into
//     the zeroed words;
//   split: the a3 bound from the final a2 bound (tower_stats3_body, four columns per
//     block), then the f16x2 fragments of the tower, of conv2's input gradient and
//     of fc4 (each scaled by a bound of the first pass)
constexpr int kPrepWmaxBlocks = 32;
struct PrepArgs {
  const float *w1, *b1, *w2, *b2, *w3, *b3, *w4;
  int C3, K4;
  char* tower;       // TowerPrep<C3>
  unsigned* hdr;     // its bounds header
  char* ct2;         // CT2 block
  char* fc4;         // fc4 fragments
  int nb3, nbt, nbc;  // split-pass block counts: stats3, tower, convt2 (fc4, then convt3 after)
  int nbf;            // fc4's
  char* ct3;          // conv3 input-gradient fragments (CT3Prep)
};
__global__ __launch_bounds__(256) void conv_prep_bounds_kernel(PrepArgs a) {
  const int b = blockIdx.x;
  if (b < 64) tower_stats_body(a.w1, a.b1, a.w2, a.b2, a.w3, 576 * a.C3, a.w4, a.K4 * 512, a.hdr, b);
  else convt2_wmax_body(a.w2, a.ct2, b - 64, kPrepWmaxBlocks);
}
__global__ __launch_bounds__(256) void conv_prep_split_kernel(PrepArgs a) {
  int b = blockIdx.x;
  if (b < a.nb3) {
    const int co = 4 * b + (threadIdx.x >> 6);
    if (co < a.C3) tower_stats3_body(a.w3, a.b3, a.C3, a.hdr, co);
  } else if ((b -= a.nb3) < a.nbt) {
    tower_prep_body(a.w1, a.w2, a.w3, a.C3, a.tower, a.hdr, b);
  } else if ((b -= a.nbt) < a.nbc) {
    convt2_prep_body(a.w2, a.ct2, b);
  } else if ((b -= a.nbc) < a.nbf) {
    fc4_prep_body(a.w4, a.K4, a.fc4, a.hdr, b);
  } else {
    b -= a.nbf;
    if (a.C3 == 32) convt3_prep_body<32>(a.w3, a.ct3, a.hdr + kTowMaxW3, b);
    else convt3_prep_body<64>(a.w3, a.ct3, a.hdr + kTowMaxW3, b);
  }
}

int acmi_conv_prepare(const acmi_net_t* net, void* prep, acmi_stream_t stream) {
  ACMI_REQUIRE(net_modes_ok(net), ACMI_ERR_ARG, "acmi_conv_prepare: bad acmi_net_t mode fields");
  const ModeScope mode_scope(net);
  Layout L;
  ACMI_REQUIRE(net && net->params && prep && make_layout(net->num_actions, net->conv3_filters, &L),
               ACMI_ERR_ARG, "acmi_conv_prepare: bad arguments");
  ACMI_REQUIRE((uintptr_t)prep % 16 == 0, ACMI_ERR_ARG, "acmi_conv_prepare: prep must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  return dispatch_c3(L.C3, [&](auto c3) -> int {
    constexpr int C3 = decltype(c3)::value;
    const PrepView<C3> v{prep};
    // the atomicMax targets -- the tower's bounds header and conv2 input gradient's
    // max |W2| words -- zeroed by one launch, then the tower's f16x2 fragments
    static_assert(TowerPrep<C3>::HDR_BYTES % 16 == 0 && (CT2::BYTES - CT2::FRAG_BYTES) % 16 == 0 &&
                      TowerPrep<C3>::HDR % 16 == 0 && CT2::FRAG_BYTES % 16 == 0,
                  "16-byte runs");
    hipLaunchKernelGGL(zero2_kernel, dim3(64), dim3(256), 0, s, reinterpret_cast<uint4*>(v.hdr()),
                       TowerPrep<C3>::HDR_BYTES / 16, reinterpret_cast<uint4*>(v.ct2() + CT2::FRAG_BYTES),
                       (CT2::BYTES - CT2::FRAG_BYTES) / 16);
    const float* P = net->params;
    const int K4 = 49 * C3;
    const int nbf = K4 / 16 * 16 * 64 / 256;
    const int nb3p = CT3Prep<C3>::KSTEPS * 2 * 64 / 256;
    PrepArgs a{P + L.off[0], P + L.off[1], P + L.off[2], P + L.off[3], P + L.off[4], P + L.off[5], P + L.off[6],
               C3, K4, v.tower(), v.hdr(), v.ct2(), v.fc4(),
               C3 / 4, (16 + 64 + 36 * (C3 / 32)) * 64 / 256 + 1, CT2::NKS * 4 * 64 / 256, nbf, v.ct3()};
    hipLaunchKernelGGL(conv_prep_bounds_kernel, dim3(64 + kPrepWmaxBlocks), dim3(256), 0, s, a);
    hipLaunchKernelGGL(conv_prep_split_kernel, dim3(a.nb3 + a.nbt + a.nbc + nbf + nb3p), dim3(256), 0, s, a);
    ACMI_LAUNCH_CHECK("acmi_conv_prepare");
    return ACMI_OK;
  });
}

int acmi_forward(const acmi_net_t* net, const uint8_t* obs, int64_t img_stride, int B,
                 const acmi_acts_t* acts, int want_value, acmi_stream_t stream) {
  ACMI_REQUIRE(net_modes_ok(net), ACMI_ERR_ARG, "acmi_forward: bad acmi_net_t mode fields");
  const ModeScope mode_scope(net);
  return forward_dispatch(net, obs, img_stride, B, acts, want_value, 1, stream);
}

/* Rollout variant: batch row b is image (b*act_img_stride) of the activation
 * buffers (env-major [N][T] storage; pointers pre-offset by step t). */
int acmi_forward_strided(const acmi_net_t* net, const uint8_t* obs, int64_t img_stride, int B,
                         const acmi_acts_t* acts, int want_value, int64_t act_img_stride,
                         acmi_stream_t stream) {
  ACMI_REQUIRE(net_modes_ok(net), ACMI_ERR_ARG, "acmi_forward_strided: bad acmi_net_t mode fields");
  const ModeScope mode_scope(net);
  return forward_dispatch(net, obs, img_stride, B, acts, want_value, act_img_stride, stream, nullptr,
                          "acmi_forward_strided");
}

// acmi_rollout_step / acmi_rollout_step_masked (legal: nullptr / one word per env)
static int rollout_step_impl(const acmi_net_t* net, const uint8_t* obs, int64_t img_stride, int B,
                             const acmi_acts_t* acts, int64_t act_img_stride, const acmi_rollout_io_t* io,
                             const uint32_t* legal, acmi_stream_t stream) {
  ACMI_REQUIRE(net_modes_ok(net), ACMI_ERR_ARG, "acmi_rollout_step: bad acmi_net_t mode fields");
  const ModeScope mode_scope(net);
  ACMI_REQUIRE(io && io->actions && io->bad_rows && io->obs_out && io->rewards && io->terminals &&
                   io->episode_rewards && io->ld >= 1 && io->out_stride % 16 == 0 &&
                   img_stride % 16 == 0 && io->row_offset >= 0 && net,
               ACMI_ERR_ARG, "acmi_rollout_step: bad arguments");
  ACMI_REQUIRE(net->num_actions < kMaxHeads, ACMI_ERR_ARG,
               "acmi_rollout_step: num_actions=%d, the fused step takes at most %d (its tail holds the A + 1 heads "
               "in %d floats of LDS); step wider action sets with acmi_forward_strided + acmi_sample_actions_dev + "
               "acmi_env_step",
               net->num_actions, kMaxHeads - 1, kMaxHeads);
  TailArgs ta{*io, obs, (long long)img_stride, legal};
  return forward_dispatch(net, obs, img_stride, B, acts, 1, act_img_stride, stream, &ta);
}

int acmi_rollout_step(const acmi_net_t* net, const uint8_t* obs, int64_t img_stride, int B,
                      const acmi_acts_t* acts, int64_t act_img_stride, const acmi_rollout_io_t* io,
                      acmi_stream_t stream) {
  return rollout_step_impl(net, obs, img_stride, B, acts, act_img_stride, io, nullptr, stream);
}

int acmi_rollout_step_masked(const acmi_net_t* net, const uint8_t* obs, int64_t img_stride, int B,
                             const acmi_acts_t* acts, int64_t act_img_stride, const acmi_rollout_io_t* io,
                             const uint32_t* legal, acmi_stream_t stream) {
  ACMI_REQUIRE(net, ACMI_ERR_ARG, "acmi_rollout_step_masked: null net");
  ACMI_REQUIRE_MASK("acmi_rollout_step_masked", legal, net->num_actions);
  return rollout_step_impl(net, obs, img_stride, B, acts, act_img_stride, io, legal, stream);
}

int acmi_game_pend_ints(void) { return (int)(sizeof(GamePend) / 4); }
int64_t acmi_rollout_game_io_bytes(void) { return (int64_t)sizeof(acmi_rollout_game_io_t); }

int acmi_rollout_step_games(const acmi_net_t* net, const uint8_t* obs, int64_t img_stride, int B,
                            const acmi_acts_t* acts, int64_t act_img_stride, const acmi_rollout_game_io_t* gio,
                            const uint32_t* legal, acmi_stream_t stream) {
  ACMI_REQUIRE(net_modes_ok(net), ACMI_ERR_ARG, "acmi_rollout_step_games: bad acmi_net_t mode fields");
  const ModeScope mode_scope(net);
  ACMI_REQUIRE(net && gio, ACMI_ERR_ARG, "acmi_rollout_step_games: null net / io");
  const acmi_rollout_io_t* io = &gio->io;
  ACMI_REQUIRE(io->actions && io->bad_rows && io->obs_out && io->rewards && io->terminals && io->episode_rewards &&
                   io->ld >= 1 && io->out_stride >= 84 * 84 * 4 && io->out_stride % 16 == 0 &&
                   img_stride % 16 == 0 && io->row_offset >= 0 && io->env_offset >= 0,
               ACMI_ERR_ARG, "acmi_rollout_step_games: bad arguments");
  const acmi_game_state_t& gs = gio->state;
  ACMI_REQUIRE(gs.episode && gs.step && gs.total && gs.done && gs.vars && gs.game >= 0 && gs.game < kNumDeviceGames,
               ACMI_ERR_ARG, "acmi_rollout_step_games: bad game state (null array or no such game)");
  ACMI_REQUIRE((gio->rules.episodic_life == 0 || gio->rules.episodic_life == 1) && gio->rules.max_steps >= 0 &&
                   gio->rules.max_steps <= BREAKOUT_MAX_STEPS,
               ACMI_ERR_ARG, "acmi_rollout_step_games: rules: episodic_life 0 or 1, max_steps 0..2000");
  ACMI_REQUIRE(net->num_actions < kMaxHeads, ACMI_ERR_ARG,
               "acmi_rollout_step_games: num_actions=%d, the fused step takes at most %d; step wider action sets "
               "with acmi_forward_strided + acmi_sample_actions_dev + acmi_game_step_mixed",
               net->num_actions, kMaxHeads - 1);
  ACMI_REQUIRE(B > kSplitMaxB || !(io->next_acts || io->tower_done) || gio->pend, ACMI_ERR_ARG,
               "acmi_rollout_step_games: the split form (B <= %d with step fusion) needs the pending area",
               kSplitMaxB);
  ACMI_REQUIRE((uintptr_t)gio->pend % 16 == 0, ACMI_ERR_ARG, "acmi_rollout_step_games: pend must be 16-byte aligned");
  GameTailArgs ta{*io, obs, (long long)img_stride, legal,
                  GameCall{gs, gio->games, gio->bad_envs, gio->rules, io->env_seed}, gio->truncated,
                  reinterpret_cast<GamePend*>(gio->pend)};
  return forward_dispatch<GameEnv>(net, obs, img_stride, B, acts, 1, act_img_stride, stream, &ta);
}

int64_t acmi_forward_ws_floats(int B) {
  if (B <= 0) return 0;
  int nz, chunk;
  fc4_plan(B, 49 * 64, &nz, &chunk);
  int nz2, chunk2;
  fc4_plan(B, 49 * 32, &nz2, &chunk2);
  // + the split rollout step's pending env states (forward_impl)
  return (long long)std::max(nz, nz2) * (B + 1) * 512 +
         (B <= kSplitMaxB ? (long long)B * (long long)(sizeof(PendState) / 4) : 0);
}

int64_t acmi_backward_ws_floats(int B, int A, int C3) {
  Layout L;
  if (!make_layout(A, C3, &L) || B < 0) return -1;
  return std::max(bwd_prefix_floats(B), stats_prefix_floats(B, A)) + bwd_partial_floats(B, A, C3);
}

// The update's entry points: check_update_args (backward.hpp; every error before
// any launch), the call's modes, one dispatch on C3.
int acmi_backward(const acmi_net_t* net, const uint8_t* obs, int64_t img_stride, int B,
                  const acmi_acts_t* acts, const acmi_bwd_t* bwd, float* grads,
                  float* a_stats, float* ws, int64_t ws_floats, acmi_stream_t stream) {
  Layout L;
  const UpdateArgs u{"acmi_backward", /*nonnull*/ acts && bwd && grads && ws && obs, /*masks*/ acts,
                     /*with_obs*/ true, obs, /*obs8*/ a_stats != nullptr, img_stride, bwd, /*distinct*/ true,
                     {ws_floats, ws_floats}};
  const int rc = check_update_args(net, B, u, &L);
  if (rc) return rc;
  const ModeScope mode_scope(net);
  return dispatch_c3(L.C3, [&](auto c3) {
    constexpr int C3 = decltype(c3)::value;
    return backward_impl<C3>(L, net->params, obs, img_stride, B, acts, bwd, grads, a_stats, ws, ws_floats,
                             (hipStream_t)stream, PrepView<C3>{net->conv_prep});
  });
}

int acmi_backward_stacked(const acmi_net_t* net, const uint8_t* obs, int64_t img_stride, int B,
                          const acmi_acts_t* acts, const acmi_bwd_t* bwd, float* grads, float* a_stats,
                          float* ws, int64_t ws_floats, const acmi_bwd_t* bwd_s, uint32_t seed,
                          uint32_t row_offset, uint32_t counter, float* ws_s, int64_t ws_s_floats,
                          acmi_stream_t stream) {
  Layout L;
  const bool nonnull = acts && bwd && bwd_s && grads && a_stats && ws && ws_s && obs;
  const bool distinct = nonnull && ws != ws_s && bwd->d1 != bwd_s->d1 && bwd->d2 != bwd_s->d2 &&
                        bwd->d3 != bwd_s->d3 && bwd->d4 != bwd_s->d4;
  const UpdateArgs u{"acmi_backward_stacked", nonnull, /*masks*/ acts, /*with_obs*/ true, obs, /*obs8*/ true,
                     img_stride, bwd, distinct, {ws_floats, ws_s_floats}};
  const int rc = check_update_args(net, B, u, &L);
  if (rc) return rc;
  const ModeScope mode_scope(net);
  return dispatch_c3(L.C3, [&](auto c3) {
    constexpr int C3 = decltype(c3)::value;
    return backward_stacked_impl<C3>(L, net->params, obs, img_stride, B, acts, bwd, grads, a_stats, ws, ws_floats,
                                     bwd_s, seed, row_offset, counter, ws_s, ws_s_floats, (hipStream_t)stream,
                                     PrepView<C3>{net->conv_prep});
  });
}

int acmi_kfac_output_stats_finish(const acmi_net_t* net, int B, const acmi_acts_t* acts, const acmi_bwd_t* bwd_s,
                                  float* g_stats, float* ws_s, int64_t ws_s_floats, acmi_stream_t stream) {
  Layout L;
  const UpdateArgs u{"acmi_kfac_output_stats_finish", /*nonnull*/ acts && bwd_s && g_stats && ws_s, /*masks*/ nullptr,
                     /*with_obs*/ false, nullptr, false, 0, nullptr, /*distinct*/ true, {ws_s_floats, ws_s_floats}};
  const int rc = check_update_args(net, B, u, &L);
  if (rc) return rc;
  const ModeScope mode_scope(net);
  // what acmi_backward_stacked left in bwd_s and in this workspace
  const StatsWs w(ws_s, ws_s_floats, B, L.A);
  return g_factors(L, B, bwd_s, g_stats, w, conv2_dx_grams_d1(net->conv_prep != nullptr, B, w), (hipStream_t)stream);
}

int acmi_stream_wait_backward_dx(acmi_stream_t stream) {
  hipEvent_t* ev = dx_done_event();
  ACMI_REQUIRE(ev && hipStreamWaitEvent((hipStream_t)stream, *ev, 0) == hipSuccess, ACMI_ERR_HIP,
               "acmi_stream_wait_backward_dx failed");
  return ACMI_OK;
}

// acmi_kfac_output_stats / acmi_kfac_output_stats_masked (legal: nullptr / one word per row)
static int output_stats_entry(const char* fn, const acmi_net_t* net, int B, const acmi_acts_t* acts,
                              const acmi_bwd_t* bwd, uint32_t seed, uint32_t row_offset,
                              uint32_t counter, float* g_stats, float* ws, int64_t ws_floats,
                              const uint32_t* legal, acmi_stream_t stream) {
  Layout L;
  const UpdateArgs u{fn, /*nonnull*/ acts && bwd && g_stats && ws, /*masks*/ acts, /*with_obs*/ false, nullptr, false,
                     0, nullptr, /*distinct*/ true, {ws_floats, ws_floats}};
  const int rc = check_update_args(net, B, u, &L);
  if (rc) return rc;
  const ModeScope mode_scope(net);
  return dispatch_c3(L.C3, [&](auto c3) {
    constexpr int C3 = decltype(c3)::value;
    return output_stats_impl<C3>(L, net->params, B, acts, bwd, seed, row_offset, counter, g_stats, ws, ws_floats,
                                 (hipStream_t)stream, PrepView<C3>{net->conv_prep}, legal);
  });
}

int acmi_kfac_output_stats(const acmi_net_t* net, int B, const acmi_acts_t* acts,
                           const acmi_bwd_t* bwd, uint32_t seed, uint32_t row_offset,
                           uint32_t counter, float* g_stats, float* ws, int64_t ws_floats,
                           acmi_stream_t stream) {
  return output_stats_entry("acmi_kfac_output_stats", net, B, acts, bwd, seed, row_offset, counter, g_stats, ws,
                            ws_floats, nullptr, stream);
}

int acmi_kfac_output_stats_masked(const acmi_net_t* net, int B, const acmi_acts_t* acts,
                                  const acmi_bwd_t* bwd, uint32_t seed, uint32_t row_offset,
                                  uint32_t counter, const uint32_t* legal, float* g_stats, float* ws,
                                  int64_t ws_floats, acmi_stream_t stream) {
  ACMI_REQUIRE(net, ACMI_ERR_ARG, "acmi_kfac_output_stats_masked: null net");
  ACMI_REQUIRE_MASK("acmi_kfac_output_stats_masked", legal, net->num_actions);
  return output_stats_entry("acmi_kfac_output_stats_masked", net, B, acts, bwd, seed, row_offset, counter, g_stats,
                            ws, ws_floats, legal, stream);
}

int acmi_prof_enable(int site, int capacity) {
  ACMI_REQUIRE(site >= 0 && capacity >= 0 && capacity <= 65536, ACMI_ERR_ARG,
               "acmi_prof_enable: bad site/capacity");
  if (g_prof_ev) {
    for (int i = 0; i < 2 * g_prof_cap; ++i) (void)hipEventDestroy(g_prof_ev[i]);
    delete[] g_prof_ev;
    g_prof_ev = nullptr;
  }
  g_prof_site = 0;
  g_prof_cap = 0;
  g_prof_n = 0;
  if (site == 0 || capacity == 0) return ACMI_OK;
  g_prof_ev = new hipEvent_t[2 * capacity];
  for (int i = 0; i < 2 * capacity; ++i) {
    if (hipEventCreate(&g_prof_ev[i]) != hipSuccess) {
      set_error("acmi_prof_enable: hipEventCreate failed");
      return ACMI_ERR_HIP;
    }
  }
  g_prof_site = site;
  g_prof_cap = capacity;
  return ACMI_OK;
}

int acmi_prof_collect(double* total_ms, int* count) {
  ACMI_REQUIRE(total_ms && count, ACMI_ERR_ARG, "acmi_prof_collect: null argument");
  double t = 0.0;
  for (int i = 0; i < g_prof_n; ++i) {
    if (hipEventSynchronize(g_prof_ev[2 * i + 1]) != hipSuccess) {
      set_error("acmi_prof_collect: hipEventSynchronize failed");
      return ACMI_ERR_HIP;
    }
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, g_prof_ev[2 * i], g_prof_ev[2 * i + 1]);
    t += ms;
  }
  *total_ms = t;
  *count = g_prof_n;
  g_prof_n = 0;
  return ACMI_OK;
}

// conv2's input-gradient kernels on caller-given buffers (test_gpu_convt2_resident.py):
// mode 0 the staging store + Gram forms, 1 the stacked form, 2 the resident forms
int acmi_debug_convt2(const acmi_net_t* net, int mode, const float* d2a, const float* d2b, const uint32_t* m1,
                      float* d1, int B, float* gram_part, const uint32_t* d2max_a, const uint32_t* d2max_b,
                      uint32_t* d1max, acmi_stream_t stream) {
  ACMI_REQUIRE(net_modes_ok(net), ACMI_ERR_ARG, "acmi_debug_convt2: bad acmi_net_t mode fields");
  const ModeScope mode_scope(net);
  ACMI_REQUIRE(net && net->conv_prep && d2a && d2b && m1 && d1 && gram_part && d2max_a && d2max_b && d1max && B > 0 &&
                   mode >= 0 && mode <= 2,
               ACMI_ERR_ARG, "acmi_debug_convt2: bad arguments");
  const char* p2 = dispatch_c3(net->conv3_filters, [&](auto c3) -> const char* {
    return PrepView<decltype(c3)::value>{net->conv_prep}.ct2();
  });
  hipStream_t s = (hipStream_t)stream;
  const float* act1 = reinterpret_cast<const float*>(m1);
  if (mode == 0) {
    hipLaunchKernelGGL((convt2_kernel<false, true>), dim3(convt2_store_blocks(B)), dim3(256), 0, s, p2, d2a, act1, d1,
                       B, nullptr, d2max_a, d1max, nullptr, nullptr);
    hipLaunchKernelGGL((convt2_kernel<true, true>), dim3(convt2_gram_blocks(B)), dim3(256), 0, s, p2, d2b, act1,
                       nullptr, B, gram_part, d2max_b, nullptr, nullptr, nullptr);
  } else if (mode == 1) {
    hipLaunchKernelGGL((convt2_kernel<true, true, true>), dim3(convt2_gram_blocks(B)), dim3(256), 0, s, p2, d2a,
                       act1, d1, B, gram_part, d2max_a, d1max, d2b, d2max_b);
  } else {
    const dim3 grid(convt2_resident_blocks(B)), block(CT2R::THREADS);
    hipLaunchKernelGGL((convt2_resident_kernel<false, true>), grid, block, 0, s, p2, d2a, act1, d1, B, nullptr,
                       d2max_a, d1max, convt2_resident_teams(B));
    hipLaunchKernelGGL((convt2_resident_kernel<true, true>), grid, block, 0, s, p2, d2b, act1, nullptr, B, gram_part,
                       d2max_b, nullptr, convt2_resident_teams(B));
  }
  ACMI_LAUNCH_CHECK("acmi_debug_convt2");
  return ACMI_OK;
}

int acmi_debug_convt2_form(int form) {
  return g_convt2_form.exchange(form < 0 ? -1 : form != 0, std::memory_order_relaxed);
}

int acmi_debug_ws_flushes(void) {
  return g_ws_flushes.exchange(0);
}

// Host-only check of the launch planners (no GPU): every sub-tile of the
// upper triangle of P^T P and every (P, dY) sub-tile is produced by sym_plan's
// groups, each column's sum by exactly one wave, for K = 64..max_k; and
// plan_rounds' chunks cover the rows exactly.  0 = ok, else the failing K.
int acmi_selftest_plans(int max_k) {
  for (int K = 64; K <= max_k; K += 32) {
    SymPlan p;
    if (!sym_plan(K, 64, &p)) continue;  // shape falls back to the 128x128 tiles
    const int J = K + 64;
    std::vector<unsigned char> cov((size_t)K * J, 0);
    std::vector<int> cs(J, 0);
    for (int g = 0; g < p.ngroups; ++g)
      for (int w = 0; w < 4; ++w) {
        if (p.g[g].wa[w] < 0) continue;
        const int a = p.g[g].base[p.g[g].wa[w]], b = p.g[g].base[p.g[g].wb[w]];
        if (a < 0 || b < 0 || a >= K) return K;
        for (int i = a; i < a + 64 && i < K; ++i)
          for (int j = b; j < b + 64 && j < J; ++j) cov[(size_t)i * J + j] = 1;
        if (a == 0)
          for (int j = b; j < b + 64 && j < J; ++j) cs[j]++;
      }
    for (int i = 0; i < K; ++i)
      for (int j = i; j < J; ++j)
        if (!cov[(size_t)i * J + j]) return K;
    for (int j = 0; j < J; ++j)
      if (cs[j] < 1) return K;
  }
  // six-slab groups (symred6_kernel): every needed sub-tile exactly once, at
  // most 16 per group and 2 per wave, each column's sum by exactly one wave
  for (int K : {512, 576})
    for (int cp : {8, 32, 64}) {
      SymPlan6 p;
      if (!sym_plan6(K, cp, &p)) return -(K + cp);
      const int nb = K / 64;
      std::vector<int> cov((size_t)(nb + 1) * (nb + 1), 0), cs(nb + 1, 0);
      for (int g = 0; g < p.ngroups; ++g) {
        int n = 0;
        for (int w = 0; w < 8; ++w)
          for (int t = 0; t < 2; ++t) {
            const int ra = p.g[g].ra[w][t], cb = p.g[g].cb[w][t];
            if (ra < 0) {
              if (t == 0 && p.g[g].ra[w][1] >= 0) return -(K + cp);  // tile 1 without tile 0
              continue;
            }
            ++n;
            const int a = p.g[g].base[ra], b = p.g[g].base[cb];
            if (a < 0 || b < 0 || a % 64 || a >= K || b < a) return -(K + cp);
            cov[(size_t)(a / 64) * (nb + 1) + b / 64]++;
            if (a == 0) cs[b / 64]++;
            // a half-width (dY) tile in slot 0 needs slot 1 half as well (kernel variants)
            if (t == 1 && p.g[g].base[p.g[g].cb[w][0]] == K && b != K) return -(K + cp);
          }
        if (n > 16) return -(K + cp);
      }
      for (int a = 0; a < nb; ++a)
        for (int b = a; b <= nb; ++b)
          if (cov[(size_t)a * (nb + 1) + b] != 1) return -(K + cp);
      for (int b = 0; b <= nb; ++b)
        if (cs[b] != 1) return -(K + cp);
    }
  // greedy six-slab groups (fc4 and the other K): every needed sub-tile exactly once,
  // at most 16 per group, a half-width tile never in slot 0 under a full one, each
  // column slab's sum by exactly one (0, b) tile
  for (int K : {1568, 512, 576})
    for (int cp : {512, 64, 8}) {
      SymPlan6 p;
      if (!sym_plan6_greedy(K, cp, &p)) return -(K + cp + 1);
      const int J = K + cp, ns = (J + 63) / 64, nbp = (K + 63) / 64;
      std::vector<int> cov((size_t)ns * ns, 0), cs(ns, 0);
      for (int g = 0; g < p.ngroups; ++g) {
        int n = 0;
        for (int w = 0; w < 8; ++w) {
          bool half0 = false;
          for (int t = 0; t < 2; ++t) {
            const int ra = p.g[g].ra[w][t], cb = p.g[g].cb[w][t];
            if (ra < 0) {
              if (t == 0 && p.g[g].ra[w][1] >= 0) return -(K + cp + 1);
              continue;
            }
            ++n;
            const int a = p.g[g].base[ra], b = p.g[g].base[cb];
            const bool half = b + 32 >= J;
            if (t == 0) half0 = half;
            else if (half0 && !half) return -(K + cp + 1);
            if (a % 64 || b % 64 || a >= K || b < a || b >= J) return -(K + cp + 1);
            cov[(size_t)(a / 64) * ns + b / 64]++;
            if (a == 0) cs[b / 64]++;
          }
        }
        if (n > 16) return -(K + cp + 1);
      }
      for (int a = 0; a < nbp; ++a)
        for (int b = a; b < ns; ++b)
          if (cov[(size_t)a * ns + b] != 1) return -(K + cp + 1);
      for (int b = 0; b < ns; ++b)
        if (cs[b] != 1) return -(K + cp + 1);
    }
  for (long long rows : {1000LL, 4096000LL, 829440LL, 501760LL, 10240LL}) {
    for (int live : {1, 3, 11, 14, 90}) {
      int nc, ch;
      plan_rounds(rows, live, 1024, &nc, &ch);
      if (ch % 32 != 0 || (long long)nc * ch < rows || (long long)(nc - 1) * ch >= rows) return -1;
    }
  }
  // band plans (conv2, conv3 at C3 = 32 / 64): exact cover, column-sum owners,
  // and the fold tables reproduce the patch-row sums (host emulation in double)
  const int bshape[3][7] = {{20, 20, 32, 4, 4, 2, 64}, {9, 9, 64, 3, 3, 1, 32}, {9, 9, 64, 3, 3, 1, 64}};
  for (int i = 0; i < 3; ++i) {
    const int* b = bshape[i];
    const BandPlan* p = band_host_plan(b[0], b[1], b[2], b[3], b[4], b[5], b[6]);
    if (!p || band_plan_check(*p) != 0 || band_plan_emulate(*p) > 1e-12) return -(1000 + i);
    for (long long rows : {1LL, 37LL, 10240LL, 20480LL}) {
      int nc, ch;
      band_chunks(rows, (int)p->groups.size(), &nc, &ch);
      if (ch % 16 != 0 || (long long)nc * ch < rows || (long long)(nc - 1) * ch >= rows) return -(1010 + i);
    }
  }
  // fc4's split counts (forward.hpp): each has a compiled heads / tail kernel, and
  // the rollout batches get the counts the fused tails are compiled for
  if (!fc4_counts_ok()) return -3000;
  return 0;
}

int acmi_gemm_f32(const float* A, const float* B, float* C, int M, int N, int K,
                  acmi_stream_t stream) {
  ACMI_REQUIRE(A && B && C && M > 0 && N > 0 && K > 0 && K % 4 == 0 && N % 4 == 0,
               ACMI_ERR_ARG, "acmi_gemm_f32: need K%%4==0, N%%4==0");
  RowsAsK<DenseRows> opA{DenseRows{A, K, M, K}};
  MatI<true> opB{B, N, K, N};
  EpiStore epi{C, N};
  launch_gemm<128, 128, 32, 2, 2, false, false>(opA, opB, epi, M, N, K, 1, 0,
                                                (hipStream_t)stream);
  ACMI_LAUNCH_CHECK("acmi_gemm_f32");
  return ACMI_OK;
}

}  // extern "C"
