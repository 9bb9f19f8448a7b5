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
// d4 = (dhead [W_pi | w_v]^T) * relu'(a4): A+1 MACs per output, elementwise
// over [B][512] (memory-bound); the k-ordered fmaf chain is the f32 MFMA's.
// amax (nullable): max |d4| published for fc4's f16x2 input gradient, once per
// block (common.hpp amax_update; every thread reaches the block reduction,
// out-of-range ones contribute 0)
__device__ __forceinline__ void block_amax256(unsigned* amax, float m) {
  __shared__ float red[4];
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) amax_update(amax, fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])));
}
__device__ __forceinline__ float absmax4f(float4 r) {
  return fmaxf(fmaxf(fabsf(r.x), fabsf(r.y)), fmaxf(fabsf(r.z), fabsf(r.w)));
}

__global__ __launch_bounds__(256) void heads_dx_kernel(const float* dhead, int ldh, int B, const float* wpi,
                                                       const float* wv, int A, const float* a4, float* d4,
                                                       unsigned* amax) {
  // 4 consecutive outputs per thread (float4 a4 / d4)
  const long long q0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const bool ok = q0 < (long long)B * 128;
  const long long q = ok ? q0 : 0;
  const int m = (int)(q >> 7), j0 = (int)(q & 127) * 4;
  const float* g = dhead + (long long)m * ldh;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int a = 0; a < A; ++a) {
    const float ga = g[a];
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] = __builtin_fmaf(ga, wpi[(j0 + e) * A + a], acc[e]);
  }
  const float gv = g[A];  // (wv is not 16-byte aligned for every A: scalar loads)
#pragma unroll
  for (int e = 0; e < 4; ++e) acc[e] = __builtin_fmaf(gv, wv[j0 + e], acc[e]);
  const float4 x = *reinterpret_cast<const float4*>(a4 + q * 4);
  // masks as multiplies by 0/1 of the computed sums (a select with a load
  // operand would be turned into a branch around the load)
  float4 o;
  o.x = acc[0] * (float)(x.x > 0.f);
  o.y = acc[1] * (float)(x.y > 0.f);
  o.z = acc[2] * (float)(x.z > 0.f);
  o.w = acc[3] * (float)(x.w > 0.f);
  if (ok) *reinterpret_cast<float4*>(d4 + q * 4) = o;
  if (amax) block_amax256(amax, ok ? absmax4f(o) : 0.f);
}

// Breakout's A = 4 (16-byte aligned W_pi rows, dhead rows of ldh % 4 == 0): the
// four W_pi rows and the dhead row as float4 loads (7 loads a thread instead of 26),
// the same k-ordered fmaf chain per output
__global__ __launch_bounds__(256) void heads_dx4_kernel(const float* dhead, int ldh, int B, const float* wpi,
                                                        const float* wv, const float* a4, float* d4,
                                                        unsigned* amax) {
  const long long q0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const bool ok = q0 < (long long)B * 128;
  const long long q = ok ? q0 : 0;
  const int m = (int)(q >> 7), j0 = (int)(q & 127) * 4;
  const float* g = dhead + (long long)m * ldh;
  const float4 g4 = *reinterpret_cast<const float4*>(g);
  const float gv = g[4];
  const float4* w4 = reinterpret_cast<const float4*>(wpi + j0 * 4);
  const float4 x = *reinterpret_cast<const float4*>(a4 + q * 4);
  float o[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float4 w = w4[e];
    float acc = __builtin_fmaf(g4.x, w.x, 0.f);
    acc = __builtin_fmaf(g4.y, w.y, acc);
    acc = __builtin_fmaf(g4.z, w.z, acc);
    acc = __builtin_fmaf(g4.w, w.w, acc);
    o[e] = __builtin_fmaf(gv, wv[j0 + e], acc);
  }
  float4 r;
  r.x = o[0] * (float)(x.x > 0.f);
  r.y = o[1] * (float)(x.y > 0.f);
  r.z = o[2] * (float)(x.z > 0.f);
  r.w = o[3] * (float)(x.w > 0.f);
  if (ok) *reinterpret_cast<float4*>(d4 + q * 4) = r;
  if (amax) block_amax256(amax, ok ? absmax4f(r) : 0.f);
}

// acmi_acts_t's masks: all three or none
static bool masks_ok(const acmi_acts_t* a) { return (a->m1 && a->m2 && a->m3) || (!a->m1 && !a->m2 && !a->m3); }

inline int roundup4(int x) { return (x + 3) & ~3; }

// (Measured and removed: conv2's input gradient on the dY-im2col-in-LDS kernel
// of convt3.hpp, 939 / 620 us per launch at M = 10240 against 444 on gemm3 -- its
// f32 dY image leaves one block per CU; conv1 / conv2 forwards on convfwd3.hpp,
// 26.5 / 82 us at 512 images against 26.5 / 30.  conv3's input gradient and
// forward keep those kernels: 231 -> 186 us, 19.6 -> 18.7 us.)

}  // namespace acmi

#include "forward.hpp"  // the forward: its kernels, fc4's split plan, the heads / tail launcher, forward_dispatch
#include "splitk.hpp"  // the split-K reduction: finalizes, plans, wgrad_layer / gcov_layer, workspace sizes

namespace acmi {

// Recorded on the backward's stream right after its input-gradient chain (per
// device): acmi_stream_wait_backward_dx lets the sampled-loss chain on another
// stream start there, next to the weight-gradient reductions instead of next to
// the (memory-bound) input gradients.
static hipEvent_t* dx_done_event() {
  static hipEvent_t ev[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
  if (!ev[dev] && hipEventCreateWithFlags(&ev[dev], hipEventDisableTiming) != hipSuccess) {
    ev[dev] = nullptr;
    return nullptr;
  }
  return &ev[dev];
}
// ---------------------------------------------------------------------------
// backward (dX chain) shared by the loss backward and the sampled backward
// ---------------------------------------------------------------------------
// the chain up to d2: heads -> d4, fc4 -> d3, conv3 -> d2
template <int C3>
static int dx_chain_pre(const Layout& L, const float* P, int B, const acmi_acts_t* a,
                        const acmi_bwd_t* bw, const float* dhead, int ldh,
                        hipStream_t s, const char* prep, unsigned* dxs) {
  // dxs: kBandScratch words of scratch (band.hpp layout): the dX epilogues publish
  // max |d3|, |d2| there, the f16x2 consumers (convt2, the band reductions) scale
  // by them
  ACMI_REQUIRE(dxs, ACMI_ERR_ARG, "dx_chain: no scratch");
  ACMI_REQUIRE(hipMemsetAsync(dxs, 0, kBandScratch * sizeof(unsigned), s) == hipSuccess, ACMI_ERR_HIP,
               "dx_chain: scratch reset failed");
  // heads -> d4 = (dhead W_h^T) * relu'(a4)
  if (L.A == 4 && ldh % 4 == 0 && (uintptr_t)(P + L.off[8]) % 16 == 0 && (uintptr_t)dhead % 16 == 0)
    hipLaunchKernelGGL(heads_dx4_kernel, dim3(cdiv((long long)B * 128, 256)), dim3(256), 0, s, dhead,
                       ldh, B, P + L.off[8], P + L.off[10], a->a4, bw->d4, dxs + kBsMaxD4);
  else
    hipLaunchKernelGGL(heads_dx_kernel, dim3(cdiv((long long)B * 128, 256)), dim3(256), 0, s, dhead,
                       ldh, B, P + L.off[8], P + L.off[10], L.A, a->a4, bw->d4, dxs + kBsMaxD4);
  // max |W3|, |W4| for the f16x2 operands below: from the prepared weights'
  // header, else computed here
  const unsigned* hdr = prep ? reinterpret_cast<const unsigned*>(prep + TowerPrep<C3>::HDR) : nullptr;
  const unsigned* w3max = hdr ? hdr + kTowMaxW3 : dxs + kBsMaxW3;
  const unsigned* w4max = hdr ? hdr + kTowMaxW4 : dxs + kBsMaxW4;
  if (!hdr && g_gemm_mode == ACMI_GEMM_X3) {
    hipLaunchKernelGGL(absmax_kernel, dim3(16), dim3(256), 0, s, P + L.off[4], (long long)576 * C3,
                       dxs + kBsMaxW3);
    hipLaunchKernelGGL(absmax_kernel, dim3(64), dim3(256), 0, s, P + L.off[6], (long long)49 * C3 * 512,
                       dxs + kBsMaxW4);
  }
  {  // fc4 -> d3 = (d4 W4^T) * relu'(a3)
    const int K3 = 49 * C3;
    RowsAsK<DenseRows> opA{DenseRows{bw->d4, 512, B, 512}};
    MatTK<true> opB{P + L.off[6], 512, 512, K3};
    // f16x2 on 128 x 64 tiles, BK = 32 (per launch at M = 10240: 89.8 us; 64 x 128
    // 107, 128 x 128 96.6, 64 x 128 / BK 32 97.1, 256 x 128 127.7; bf16x3 64 x 128 132)
    auto run = [&](auto epi) {
      if (g_gemm_mode == ACMI_GEMM_X3)
        launch_gemm3_f16<128, 64, 32, 2, 1>(opA, opB, epi, B, K3, 512, dxs + kBsMaxD4, w4max, s);
      else
        launch_mm<64, 128, 32, 1, 2, false, false, 16>(opA, opB, epi, B, K3, 512, 1, 0, s);
    };
    // ReLU'(a3) from the mask bits when the forward wrote them
    prof_begin(ACMI_PROF_FC4_DX, s);
    if (a->m3) run(EpiReluGrad<true>{bw->d3, reinterpret_cast<const float*>(a->m3), K3, dxs + kBsMaxD3});
    else run(EpiReluGrad<false>{bw->d3, a->a3, K3, dxs + kBsMaxD3});
    prof_end(ACMI_PROF_FC4_DX, s);
  }
  // conv input gradients as transposed products: rows = (phase, channel) of
  // the weights, columns = (super-)pixels gathering dY (EpiConvT, float4 rows)
  {  // conv3 -> d2 (stride 1: one phase)
    // its weights pre-split in the prepared buffer (after fc4's, acmi_conv_prep_bytes)
    const char* ct3p = prep ? prep + TowerPrep<C3>::BYTES + CT2::BYTES + fc4_prep_bytes(49 * C3) : nullptr;
    using Src = ConvTRows<9, 9, 3, 3, 1, C3>;
    using W = ConvTWeights<3, 3, 1, 64, C3>;
    W opA{P + L.off[4]};
    RowsAsK<Src> opB{Src{bw->d3, B * Src::L}};
    auto run = [&](auto epi) {
      if (g_gemm_mode == ACMI_GEMM_X3)
        // f16x2 operands: the scales of max |W3| and of max |d3| (the fc4 dX epilogue's)
        launch_convt_x3<9, 9, 3, 3, 1, 64, C3, 256>(P + L.off[4], ct3p, bw->d3, B, epi, w3max, dxs + kBsMaxD3, s);
      else
        launch_mm<64, 128, 16, 1, 2, false, false, 16>(opA, opB, epi, W::N, B * Src::L, Src::COLS, 1, 0, s);
    };
    prof_begin(ACMI_PROF_CONV3_DX, s);
    if (a->m2) run(EpiConvT<9, 9, 1, 64, true>{bw->d2, reinterpret_cast<const float*>(a->m2), dxs + kBsMaxD2});
    else run(EpiConvT<9, 9, 1, 64>{bw->d2, a->a2, dxs + kBsMaxD2});
    prof_end(ACMI_PROF_CONV3_DX, s);
  }
  ACMI_LAUNCH_CHECK("dx_chain");
  return ACMI_OK;
}

// which form of conv2's input gradient dx_conv2 launches (acmi_debug_convt2_form):
// -1 = by the tile-count thresholds of convt2.hpp, 0 = staging, 1 = resident
static std::atomic<int> g_convt2_form{-1};
static bool convt2_use_resident(int B, bool gram) {
  const int f = g_convt2_form.load(std::memory_order_relaxed);
  return f < 0 ? convt2_resident_default(B, gram) : f != 0;
}

// conv2's input gradient, from d2 (max |d2| in dxs): the loss chain stores the
// masked d1 (gram_part null), the sampled chain reduces it to conv1's G-factor
// Gram partials (*gram_done set when it did)
template <int C3>
static int dx_conv2(const Layout& L, const float* P, int B, const acmi_acts_t* a, const acmi_bwd_t* bw,
                    hipStream_t s, const char* prep, float* gram_part, bool* gram_done, unsigned* dxs) {
  if (gram_done) *gram_done = false;
  {  // conv2 -> d1 (stride 2: the four phases of a 2x2 super-pixel are the
     // 4 x 32 rows of one product over the 10x10 super-pixels)
    using Src = ConvTRows<20, 20, 4, 4, 2, 64>;
    using W = ConvTWeights<4, 4, 2, 32, 64>;
    W opA{P + L.off[2]};
    RowsAsK<Src> opB{Src{bw->d2, B * Src::L}};
    // (max |d1|: conv1's f16x2 weight gradient; ReLU'(a1) from the mask bits when written)
    const float* act1 = a->m1 ? reinterpret_cast<const float*>(a->m1) : a->a1;
    prof_begin(ACMI_PROF_CONV2_DX, s);
    const char* p2 = prep ? prep + TowerPrep<C3>::BYTES : nullptr;
    if (p2 && g_gemm_mode == ACMI_GEMM_X3) {
      // pre-split weights, four phases per wave (convt2.hpp); the sampled-loss
      // chain reduces d1 to its Gram partials instead of storing it
      auto go = [&](auto GRAMc, auto MASKc) {
        constexpr bool GR = decltype(GRAMc)::value, MK = decltype(MASKc)::value;
        if (convt2_use_resident(B, GR))  // W2^T resident in LDS (large batches; the same bits)
          hipLaunchKernelGGL((convt2_resident_kernel<GR, MK>), dim3(convt2_resident_blocks(B)), dim3(CT2R::THREADS),
                             0, s, p2, bw->d2, act1, GR ? nullptr : bw->d1, B, GR ? gram_part : nullptr,
                             dxs + kBsMaxD2, GR ? nullptr : dxs + kBsMaxD1, convt2_resident_teams(B));
        else if (GR)
          hipLaunchKernelGGL((convt2_kernel<GR, MK>), dim3(convt2_gram_blocks(B)), dim3(256), 0, s, p2, bw->d2,
                             act1, nullptr, B, gram_part, dxs + kBsMaxD2, nullptr);
        else
          hipLaunchKernelGGL((convt2_kernel<GR, MK>), dim3(convt2_store_blocks(B)), dim3(256), 0, s, p2,
                             bw->d2, act1, bw->d1, B, nullptr, dxs + kBsMaxD2, dxs + kBsMaxD1);
      };
      using T = std::true_type;
      using F = std::false_type;
      if (gram_part) {
        if (a->m1) go(T{}, T{});
        else go(T{}, F{});
        if (gram_done) *gram_done = true;
      } else {
        if (a->m1) go(F{}, T{});
        else go(F{}, F{});
      }
    } else if (a->m1) {
      launch_mm<128, 128, 16, 2, 2, false, false, 16>(
          opA, opB, EpiConvT<20, 20, 2, 32, true>{bw->d1, act1, dxs + kBsMaxD1}, W::N, B * Src::L, Src::COLS, 1, 0, s);
    } else {
      launch_mm<128, 128, 16, 2, 2, false, false, 16>(opA, opB, EpiConvT<20, 20, 2, 32>{bw->d1, act1, dxs + kBsMaxD1},
                                                      W::N, B * Src::L, Src::COLS, 1, 0, s);
    }
    prof_end(ACMI_PROF_CONV2_DX, s);
  }
  ACMI_LAUNCH_CHECK("dx_conv2");
  return ACMI_OK;
}

template <int C3>
static int dx_chain(const Layout& L, const float* P, int B, const acmi_acts_t* a,
                    const acmi_bwd_t* bw, const float* dhead, int ldh,
                    hipStream_t s, const char* prep = nullptr, float* gram_part = nullptr,
                    bool* gram_done = nullptr, unsigned* dxs = nullptr) {
  const int rc = dx_chain_pre<C3>(L, P, B, a, bw, dhead, ldh, s, prep, dxs);
  if (rc) return rc;
  return dx_conv2<C3>(L, P, B, a, bw, s, prep, gram_part, gram_done, dxs);
}

template <int C3>
static int backward_impl(const Layout& L, const float* P, const uint8_t* obs,
                         long long img_stride, int B, const acmi_acts_t* a,
                         const acmi_bwd_t* bw, float* grads, float* astat,
                         float* ws, long long ws_cap, hipStream_t s, const char* prep,
                         bool dx_done = false) {
  // dx_done: the caller ran the dX chain into bw / the scratch (backward_stacked_impl)
  const bool st = astat != nullptr;
  // conv1's weight gradient is fused into the A-factor pass (bf16x3 mode; it needs
  // d1, so the pass follows the dX chain).  (Measured and removed: the A factor on a
  // library side stream next to the dX chain, 5.69 vs 5.64 ms per update -- the i8
  // gather competes with the symmetric reductions for L2 and LDS; the A factor
  // before the dX chain.)
  const bool fuse_c1 = st && g_gemm_mode == ACMI_GEMM_X3;
  // operand-scale scratch (band.hpp) first: the dX epilogues publish max |d3|,
  // |d2| into it; then the conv1 A-factor integers; the partial region is the rest
  unsigned* bscr = reinterpret_cast<unsigned*>(ws);
  const long long prefix = bwd_prefix_floats(B);
  float* part = ws + prefix;
  const long long avail = ws_cap - prefix;
  const bool band = band_on(st);
  int rc = ACMI_OK;
  if (!dx_done) {
    rc = dx_chain<C3>(L, P, B, a, bw, bw->dhead, bw->ldh, s, prep, nullptr, nullptr, bscr);
    if (rc) return rc;
    hipEvent_t* ev = dx_done_event();
    ACMI_REQUIRE(ev && hipEventRecord(*ev, s) == hipSuccess, ACMI_ERR_HIP, "acmi_backward: dX event record failed");
  }
  float* wpart_c1 = nullptr;  // conv1's fused weight-gradient partials (in the A-factor workspace)
  if (st) {
    prof_begin(ACMI_PROF_CONV1_AFACTOR, s);
    const int rc0 = conv1_afactor_u8(obs, img_stride, B, astat + L.stat_off[0],
                                     reinterpret_cast<int*>(ws + kBandScratch), afactor_ws_floats(B), s,
                                     fuse_c1 ? bw->d1 : nullptr, &wpart_c1, bscr + kBsMaxD1);
    prof_end(ACMI_PROF_CONV1_AFACTOR, s);
    if (rc0) return rc0;
  }
  // the conv1, heads and fc4 finalizes deferred into one launch: each layer's
  // partials in their own range of the partial region
  PartRanges<WgradSet> ra{part, avail, s};
  if (st && fuse_c1) {  // the conv1 weight gradient came with the A factor: reduce its chunks
    const long long rows = 400LL * B;
    WgradDesc d{wpart_c1, conv1_afactor_fused_chunks(rows), 256, 32, 0, 32, grads + L.off[0], 32,
                nullptr, nullptr, (int)rows, 1.0f / 255.0f};
    ra.add(d, 0);
  }
  // heads: X = a4 (512), dY = dhead (A+1 columns: pi | v)
  rc = wgrad_layer(DenseRows{a->a4, 512, B, 512}, 512, B, bw->dhead, bw->ldh, L.A + 1, st, ra, grads + L.off[8],
                   L.A, grads + L.off[10], st ? astat + L.stat_off[4] : nullptr);
  if (rc) return rc;
  // fc4: X = a3 flat; f16x2 with the prepared weights' a3 bound and max |d4|
  // (published by the dX chain's heads kernel)
  const unsigned* a3b =
      prep ? reinterpret_cast<const unsigned*>(prep + TowerPrep<C3>::HDR) + kTowMaxA3 : nullptr;
  rc = wgrad_layer(DenseRows{a->a3, 49 * C3, B, 49 * C3}, 49 * C3, B, bw->d4, 512, 512, st, ra, grads + L.off[6],
                   512, nullptr, st ? astat + L.stat_off[3] : nullptr, 0, 1.f, a3b, a3b ? bscr + kBsMaxD4 : nullptr);
  if (rc) return rc;
  ra.flush();
  // conv3 / conv2: pixel-pair band reductions over the dense activation rows
  // (band.hpp, the whole partial region), or the patches of a2 / a1 (each
  // patch-row layer's finalize launched straight after it)
  // a1 / a2 bounds from the weights (max |d2|, |d3| came with the dX chain): the
  // prepared weights' header holds them (tower_stats_body, the same sums as
  // band_bounds_kernel), else computed here
  const unsigned* xb = prep ? reinterpret_cast<const unsigned*>(prep + TowerPrep<C3>::HDR) : nullptr;
  const unsigned* a1b = xb ? xb + kTowMaxA1 : bscr + kBsMaxA1;
  const unsigned* a2b = xb ? xb + kTowMaxA2 : bscr + kBsMaxA2;
  if (band) {
    if (!xb)
      hipLaunchKernelGGL(band_bounds_kernel, dim3(64), dim3(256), 0, s, P + L.off[0], P + L.off[1], P + L.off[2],
                         P + L.off[3], bscr);
    rc = band_layer(a->a2, 9, 9, 64, 3, 3, 1, bw->d3, C3, B, part, avail, grads + L.off[4],
                    astat + L.stat_off[2], 1.f, a2b, bscr + kBsMaxD3, s);
  } else
    rc = wgrad_layer(ConvRows<float, 9, 9, 64, 3, 3, 1>{a->a2, 81 * 64, B * 49}, 576, 49LL * B, bw->d3, C3, C3, st,
                     ra, grads + L.off[4], C3, nullptr, st ? astat + L.stat_off[2] : nullptr);
  if (rc) return rc;
  ra.flush();
  if (band)
    rc = band_layer(a->a1, 20, 20, 32, 4, 4, 2, bw->d2, 64, B, part, avail, grads + L.off[2],
                    astat + L.stat_off[1], 1.f, a1b, bscr + kBsMaxD2, s, ACMI_PROF_CONV2_WGRAD);
  else
    rc = wgrad_layer(ConvRows<float, 20, 20, 32, 4, 4, 2>{a->a1, 400 * 32, B * 81}, 512, 81LL * B, bw->d2, 64, 64,
                     st, ra, grads + L.off[2], 64, nullptr, st ? astat + L.stat_off[1] : nullptr,
                     ACMI_PROF_CONV2_WGRAD);
  if (rc) return rc;
  ra.flush();
  // conv1: weight gradient on the f32 engine from the raw u8 patches; its A factor
  // from the u8 frames on the i8 matrix cores (exact integer sums, afactor_u8.hip)
  if (!fuse_c1)
    rc = wgrad_layer(ConvRows<uint8_t, 84, 84, 4, 8, 8, 4>{obs, (uint32_t)img_stride, B * 400}, 256, 400LL * B,
                     bw->d1, 32, 32, false, ra, grads + L.off[0], 32, nullptr, nullptr, ACMI_PROF_CONV1_WGRAD,
                     1.0f / 255.0f);
  if (rc) return rc;
  ra.flush();
  ACMI_LAUNCH_CHECK("wgrad_layer");
  return ACMI_OK;
}

// sampled-loss output gradients at the heads (kfac "gradients" mode):
// g_pi = softmax(z) - onehot(y), y ~ Cat(z);  g_v = V - y_v = -eps, eps~N(0,1)
// MASKED (acmi_kfac_output_stats_masked): y ~ Cat over the row's legal set S with
// the same key, p - onehot(y) on S and +0 elsewhere (stepper.hpp legal_at)
template <bool MASKED>
__global__ void sampled_head_grad_kernel(const float* logits, int ld, int B, int A, uint32_t seed, uint32_t row0,
                                         uint32_t ctr, float* g, int ldg, const uint32_t* legal) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= B) return;
  const float* z = logits + (long long)m * ld;
  const uint32_t lg = MASKED ? legal_bits(legal[m], A) : 0xFFFFFFFFu;
  const RowMaxSum ms = row_max_sum<MASKED>(z, A, lg);
  const float mx = ms.mx, se = ms.se;
  // keyed by the global row: a data-parallel shard draws what the full batch would
  const uint32_t h = key4(seed, 0u, ctr, row0 + (uint32_t)m);
  const float u = u01(h);
  // inverse CDF draw
  const float target = u * se;
  float c = 0.f;
  int y = ms.last;
  for (int a = 0; a < A; ++a) {
    if (!legal_at<MASKED>(lg, a)) continue;
    c += expf(z[a] - mx);
    if (target < c) { y = a; break; }
  }
  float* gr = g + (long long)m * ldg;
  for (int a = 0; a < A; ++a)
    gr[a] = legal_at<MASKED>(lg, a) ? expf(z[a] - mx) / se - (a == y ? 1.f : 0.f) : 0.f;
  // The drawn action's column p_y - 1 carries p_y's rounding, 2^-24 absolute: on a
  // saturated row that is 0 or one ulp of 1 where the column is 1e-8 .. 1e-30, and the
  // policy head's G factor of a batch of such rows would be rounding noise.  Where the
  // OTHER members hold less than 2^-7 of the sum (the subtraction would lose more
  // than 7 of the 24 bits) the column is formed from them instead, -rest / se, to
  // f32 relative accuracy.  Every other row keeps the subtraction (within 2^-17 of
  // the column there), so runs whose policies are not saturated reproduce bit for bit.
  float rest = 0.f;
  for (int a = 0; a < A; ++a)
    if (a != y && legal_at<MASKED>(lg, a)) rest += expf(z[a] - mx);
  if (y >= 0 && rest > 0.f && rest < se * 0.0078125f) gr[y] = -rest / se;
  // Box-Muller from two further counters
  const float u1 = u01(mix32(h ^ 0x68e31da4U)) + (1.0f / 33554432.0f);
  const float u2 = u01(mix32(h ^ 0xb5297a4dU));
  const float eps = sqrtf(-2.f * logf(u1)) * cosf(6.2831853071795864f * u2);
  gr[A] = -eps;
  for (int a = A + 1; a < ldg; ++a) gr[a] = 0.f;
}
// legal (nullable): per-row legal-action words
static void launch_sampled_head_grad(const float* logits, int ld, int B, int A, uint32_t seed, uint32_t row0,
                                     uint32_t ctr, float* g, int ldg, const uint32_t* legal, hipStream_t s) {
  const auto kern = legal ? sampled_head_grad_kernel<true> : sampled_head_grad_kernel<false>;
  hipLaunchKernelGGL(kern, dim3(cdiv(B, 128)), dim3(128), 0, s, logits, ld, B, A, seed, row0, ctr, g, ldg, legal);
}

template <int C3>
static int output_stats_impl(const Layout& L, const float* P, int B,
                             const acmi_acts_t* a, const acmi_bwd_t* bw,
                             uint32_t seed, uint32_t row0, uint32_t ctr,
                             float* gstat, float* ws, long long ws_cap,
                             hipStream_t s, const char* prep, int stage = 0,
                             const uint32_t* legal = nullptr) {
  // legal (nullable): per-row legal-action words, the masked head gradients
  // stage: 0 the whole chain; 2 only the G factors, from what backward_stacked_impl
  // left in bw (d2..d4) and in this workspace (scratch maxima, conv1's Gram partials)
  const int ldg = (int)head_grad_ldg(L.A);
  // [the dX chain's scratch (operand-scale maxima) | ghead [B][ldg] | partials]
  unsigned* dxs = reinterpret_cast<unsigned*>(ws);
  float* ghead = ws + kBandScratch;
  const long long prefix = stats_prefix_floats(B, L.A);
  float* part = ws + prefix;
  const long long cap = ws_cap - prefix;
  bool g1_done = false;
  const bool g1_fits = (long long)convt2_gram_blocks(B) * 33 * 32 <= cap;
  int rc = ACMI_OK;
  if (stage == 0) {
    launch_sampled_head_grad(a->logits, a->ld_logits, B, L.A, seed, row0, ctr, ghead, ldg, legal, s);
    rc = dx_chain<C3>(L, P, B, a, bw, ghead, ldg, s, prep, g1_fits ? part : nullptr, &g1_done, dxs);
    if (rc) return rc;
  } else {
    g1_done = g1_fits && prep && g_gemm_mode == ACMI_GEMM_X3;  // (dx_conv2's Gram predicate)
  }
  // the G factors' finalizes deferred into one launch: every Gram's partials in
  // their own range of the workspace
  PartRanges<CovSet> ra{part, cap, s};
  if (g1_done) {  // G of conv1's output from the conv2 dX kernel's per-block Gram partials (the first range)
    const int nc = convt2_gram_blocks(B);
    const long long floats = (long long)nc * 33 * 32;
    const float* g1_part = ra.begin(floats);
    ra.add(g1_part, nc, 32, 32, gstat + L.stat_off[5 + 0], (int)(400LL * B), 1);
    rc = ra.end(floats);
    if (rc) return rc;
  }
  // heads: G_pi (A x A) from the first A columns, G_v = element (A, A)
  rc = gcov_layer(ghead, ldg, L.A + 1, B, L.A, ra, gstat + L.stat_off[5 + 4], gstat + L.stat_off[5 + 5], L.A);
  if (rc) return rc;
  // (the dX chain above published max |d4| and max |d2| into dxs)
  rc = gcov_layer(bw->d4, 512, 512, B, 512, ra, gstat + L.stat_off[5 + 3], nullptr, -1, dxs + kBsMaxD4);
  if (rc) return rc;
  rc = gcov_layer(bw->d3, C3, C3, 49LL * B, C3, ra, gstat + L.stat_off[5 + 2]);
  if (rc) return rc;
  rc = gcov_layer(bw->d2, 64, 64, 81LL * B, 64, ra, gstat + L.stat_off[5 + 1], nullptr, -1, dxs + kBsMaxD2);
  if (rc) return rc;
  if (!g1_done) rc = gcov_layer(bw->d1, 32, 32, 400LL * B, 32, ra, gstat + L.stat_off[5 + 0]);
  if (rc) return rc;
  ra.flush();
  ACMI_LAUNCH_CHECK("G factor finalize");
  return ACMI_OK;
}

// acmi_backward + the input-gradient half of acmi_kfac_output_stats, with conv2's
// input gradient of both chains as ONE launch (convt2_kernel MIX: one W2^T
// stream, the loss chain's tiles storing d1, the sampled chain's reducing
// conv1's G-factor Gram); the G factors follow in output_stats_impl stage 2.
// Bit-identical to the two calls.
template <int C3>
static int backward_stacked_impl(const Layout& L, const float* P, const uint8_t* obs, long long img_stride, int B,
                                 const acmi_acts_t* a, const acmi_bwd_t* bw, float* grads, float* astat, float* ws,
                                 long long ws_cap, const acmi_bwd_t* bws, uint32_t seed, uint32_t row0, uint32_t ctr,
                                 float* wss, long long wss_cap, hipStream_t s, const char* prep) {
  unsigned* bscr = reinterpret_cast<unsigned*>(ws);
  int rc = dx_chain_pre<C3>(L, P, B, a, bw, bw->dhead, bw->ldh, s, prep, bscr);
  if (rc) return rc;
  // the sampled chain's head gradients and its chain up to d2 (output_stats_impl's layout)
  const int ldg = (int)head_grad_ldg(L.A);
  unsigned* dxs = reinterpret_cast<unsigned*>(wss);
  float* ghead = wss + kBandScratch;
  float* part_s = wss + stats_prefix_floats(B, L.A);
  const long long cap_s = wss_cap - stats_prefix_floats(B, L.A);
  launch_sampled_head_grad(a->logits, a->ld_logits, B, L.A, seed, row0, ctr, ghead, ldg, nullptr, s);
  rc = dx_chain_pre<C3>(L, P, B, a, bws, ghead, ldg, s, prep, dxs);
  if (rc) return rc;
  const bool g1_fits = (long long)convt2_gram_blocks(B) * 33 * 32 <= cap_s;
  if (prep && g_gemm_mode == ACMI_GEMM_X3 && g1_fits) {
    const char* p2 = prep + TowerPrep<C3>::BYTES;
    const float* act1 = a->m1 ? reinterpret_cast<const float*>(a->m1) : a->a1;
    prof_begin(ACMI_PROF_CONV2_DX, s);
    if (a->m1)
      hipLaunchKernelGGL((convt2_kernel<true, true, true>), dim3(convt2_gram_blocks(B)), dim3(256), 0, s, p2, bw->d2,
                         act1, bw->d1, B, part_s, bscr + kBsMaxD2, bscr + kBsMaxD1, bws->d2, dxs + kBsMaxD2);
    else
      hipLaunchKernelGGL((convt2_kernel<true, false, true>), dim3(convt2_gram_blocks(B)), dim3(256), 0, s, p2, bw->d2,
                         act1, bw->d1, B, part_s, bscr + kBsMaxD2, bscr + kBsMaxD1, bws->d2, dxs + kBsMaxD2);
    prof_end(ACMI_PROF_CONV2_DX, s);
    ACMI_LAUNCH_CHECK("stacked conv2 dX");
  } else {  // the two launches (no prepared weights / f32 mode / a workspace without room for the Gram)
    rc = dx_conv2<C3>(L, P, B, a, bw, s, prep, nullptr, nullptr, bscr);
    if (rc) return rc;
    bool g1_done = false;
    rc = dx_conv2<C3>(L, P, B, a, bws, s, prep, g1_fits ? part_s : nullptr, &g1_done, dxs);
    if (rc) return rc;
  }
  {
    hipEvent_t* ev = dx_done_event();
    ACMI_REQUIRE(ev && hipEventRecord(*ev, s) == hipSuccess, ACMI_ERR_HIP, "acmi_backward: dX event record failed");
  }
  return backward_impl<C3>(L, P, obs, img_stride, B, a, bw, grads, astat, ws, ws_cap, s, prep, true);
}

}  // namespace acmi

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
  // the tower's conv weights, then conv2's input-gradient weights (convt2.hpp)
  // and fc4's weights (fc4roll.hpp)
  // and conv3's input-gradient weights (convt3.hpp)
  return C3 == 32   ? TowerPrep<32>::BYTES + CT2::BYTES + fc4_prep_bytes(49 * 32) + CT3Prep<32>::BYTES
         : C3 == 64 ? TowerPrep<64>::BYTES + CT2::BYTES + fc4_prep_bytes(49 * 64) + CT3Prep<64>::BYTES
                    : -1;
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
  const long long o2 = L.C3 == 32 ? TowerPrep<32>::BYTES : TowerPrep<64>::BYTES;
  const long long oh = L.C3 == 32 ? TowerPrep<32>::HDR : TowerPrep<64>::HDR;
  // the atomicMax targets -- the tower's bounds header and conv2 input gradient's
  // max |W2| words -- zeroed by one launch, then the tower's f16x2 fragments
  static_assert(TowerPrep<32>::HDR_BYTES % 16 == 0 && (CT2::BYTES - CT2::FRAG_BYTES) % 16 == 0 &&
                    TowerPrep<32>::HDR % 16 == 0 && TowerPrep<64>::HDR % 16 == 0 && CT2::FRAG_BYTES % 16 == 0,
                "16-byte runs");
  hipLaunchKernelGGL(zero2_kernel, dim3(64), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<uint4*>(static_cast<char*>(prep) + oh), TowerPrep<32>::HDR_BYTES / 16,
                     reinterpret_cast<uint4*>(static_cast<char*>(prep) + o2 + CT2::FRAG_BYTES),
                     (CT2::BYTES - CT2::FRAG_BYTES) / 16);
  const float* P = net->params;
  char* base = static_cast<char*>(prep);
  const int K4 = 49 * L.C3;
  const int nbf = K4 / 16 * 16 * 64 / 256;
  const int nb3p = (L.C3 == 32 ? CT3Prep<32>::KSTEPS : CT3Prep<64>::KSTEPS) * 2 * 64 / 256;
  PrepArgs a{P + L.off[0], P + L.off[1], P + L.off[2], P + L.off[3], P + L.off[4], P + L.off[5], P + L.off[6],
             L.C3, K4, base, reinterpret_cast<unsigned*>(base + oh), base + o2, base + o2 + CT2::BYTES,
             L.C3 / 4, (16 + 64 + 36 * (L.C3 / 32)) * 64 / 256 + 1, CT2::NKS * 4 * 64 / 256, nbf,
             base + o2 + CT2::BYTES + fc4_prep_bytes(K4)};
  hipLaunchKernelGGL(conv_prep_bounds_kernel, dim3(64 + kPrepWmaxBlocks), dim3(256), 0, (hipStream_t)stream, a);
  hipLaunchKernelGGL(conv_prep_split_kernel, dim3(a.nb3 + a.nbt + a.nbc + nbf + nb3p), dim3(256), 0,
                     (hipStream_t)stream, a);
  ACMI_LAUNCH_CHECK("acmi_conv_prepare");
  return ACMI_OK;
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
  return forward_dispatch(net, obs, img_stride, B, acts, want_value, act_img_stride, stream);
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

int acmi_backward(const acmi_net_t* net, const uint8_t* obs, int64_t img_stride, int B,
                  const acmi_acts_t* acts, const acmi_bwd_t* bwd, float* grads,
                  float* a_stats, float* ws, int64_t ws_floats, acmi_stream_t stream) {
  ACMI_REQUIRE(net_modes_ok(net), ACMI_ERR_ARG, "acmi_backward: bad acmi_net_t mode fields");
  const ModeScope mode_scope(net);
  Layout L;
  ACMI_REQUIRE(net && acts && bwd && grads && ws && obs, ACMI_ERR_ARG,
               "acmi_backward: null argument");
  ACMI_REQUIRE(masks_ok(acts), ACMI_ERR_ARG, "acmi_backward: ReLU masks m1..m3 must be all set or all NULL");
  ACMI_REQUIRE(make_layout(net->num_actions, net->conv3_filters, &L), ACMI_ERR_ARG,
               "acmi_backward: bad net");
  ACMI_REQUIRE(B > 0 && img_stride >= 84 * 84 * 4 && img_stride % 4 == 0, ACMI_ERR_ARG,
               "acmi_backward: bad B / img_stride");
  ACMI_REQUIRE(bwd->ldh >= net->num_actions + 1 && bwd->ldh % 4 == 0, ACMI_ERR_ARG,
               "acmi_backward: ldh must be >= A+1 and a multiple of 4 (zero padded)");
  ACMI_REQUIRE(spans32(B, img_stride, 84 * 84 * 4) && spans32(B, 400 * 32, 400 * 32), ACMI_ERR_ARG,
               "acmi_backward: batch spans >= 2^31 elements (B=%d)", B);
  const long long need = acmi_backward_ws_floats(B, net->num_actions, net->conv3_filters);
  ACMI_REQUIRE(ws_floats >= need, ACMI_ERR_WS, "acmi_backward: workspace of %lld floats < %lld",
               (long long)ws_floats, need);
  hipStream_t s = (hipStream_t)stream;
  if (L.C3 == 32)
    return backward_impl<32>(L, net->params, obs, img_stride, B, acts, bwd, grads, a_stats, ws,
                             ws_floats, s, static_cast<const char*>(net->conv_prep));
  return backward_impl<64>(L, net->params, obs, img_stride, B, acts, bwd, grads, a_stats, ws,
                           ws_floats, s, static_cast<const char*>(net->conv_prep));
}

int acmi_backward_stacked(const acmi_net_t* net, const uint8_t* obs, int64_t img_stride, int B,
                          const acmi_acts_t* acts, const acmi_bwd_t* bwd, float* grads, float* a_stats,
                          float* ws, int64_t ws_floats, const acmi_bwd_t* bwd_s, uint32_t seed,
                          uint32_t row_offset, uint32_t counter, float* ws_s, int64_t ws_s_floats,
                          acmi_stream_t stream) {
  ACMI_REQUIRE(net_modes_ok(net), ACMI_ERR_ARG, "acmi_backward_stacked: bad acmi_net_t mode fields");
  const ModeScope mode_scope(net);
  Layout L;
  ACMI_REQUIRE(net && acts && bwd && bwd_s && grads && a_stats && ws && ws_s && obs, ACMI_ERR_ARG,
               "acmi_backward_stacked: null argument");
  ACMI_REQUIRE(masks_ok(acts), ACMI_ERR_ARG, "acmi_backward_stacked: ReLU masks m1..m3 must be all set or all NULL");
  ACMI_REQUIRE(make_layout(net->num_actions, net->conv3_filters, &L), ACMI_ERR_ARG, "acmi_backward_stacked: bad net");
  ACMI_REQUIRE(B > 0 && img_stride >= 84 * 84 * 4 && img_stride % 4 == 0, ACMI_ERR_ARG,
               "acmi_backward_stacked: bad B / img_stride");
  ACMI_REQUIRE(bwd->ldh >= net->num_actions + 1 && bwd->ldh % 4 == 0, ACMI_ERR_ARG,
               "acmi_backward_stacked: ldh must be >= A+1 and a multiple of 4 (zero padded)");
  ACMI_REQUIRE(spans32(B, img_stride, 84 * 84 * 4) && spans32(B, 400 * 32, 400 * 32), ACMI_ERR_ARG,
               "acmi_backward_stacked: batch spans >= 2^31 elements (B=%d)", B);
  ACMI_REQUIRE(ws != ws_s && bwd->d1 != bwd_s->d1 && bwd->d2 != bwd_s->d2 && bwd->d3 != bwd_s->d3 &&
                   bwd->d4 != bwd_s->d4,
               ACMI_ERR_ARG, "acmi_backward_stacked: the two chains need their own workspaces and d1..d4");
  const long long need = acmi_backward_ws_floats(B, net->num_actions, net->conv3_filters);
  ACMI_REQUIRE(ws_floats >= need && ws_s_floats >= need, ACMI_ERR_WS,
               "acmi_backward_stacked: workspaces of %lld / %lld floats < %lld", (long long)ws_floats,
               (long long)ws_s_floats, need);
  hipStream_t s = (hipStream_t)stream;
  const char* prep = static_cast<const char*>(net->conv_prep);
  if (L.C3 == 32)
    return backward_stacked_impl<32>(L, net->params, obs, img_stride, B, acts, bwd, grads, a_stats, ws, ws_floats,
                                     bwd_s, seed, row_offset, counter, ws_s, ws_s_floats, s, prep);
  return backward_stacked_impl<64>(L, net->params, obs, img_stride, B, acts, bwd, grads, a_stats, ws, ws_floats,
                                   bwd_s, seed, row_offset, counter, ws_s, ws_s_floats, s, prep);
}

int acmi_kfac_output_stats_finish(const acmi_net_t* net, int B, const acmi_acts_t* acts, const acmi_bwd_t* bwd_s,
                                  float* g_stats, float* ws_s, int64_t ws_s_floats, acmi_stream_t stream) {
  ACMI_REQUIRE(net_modes_ok(net), ACMI_ERR_ARG, "acmi_kfac_output_stats_finish: bad acmi_net_t mode fields");
  const ModeScope mode_scope(net);
  Layout L;
  ACMI_REQUIRE(net && acts && bwd_s && g_stats && ws_s, ACMI_ERR_ARG, "acmi_kfac_output_stats_finish: null argument");
  ACMI_REQUIRE(make_layout(net->num_actions, net->conv3_filters, &L), ACMI_ERR_ARG, "bad net");
  ACMI_REQUIRE(B > 0 && spans32(B, 400 * 32, 400 * 32), ACMI_ERR_ARG, "bad B");
  const long long need = acmi_backward_ws_floats(B, net->num_actions, net->conv3_filters);
  ACMI_REQUIRE(ws_s_floats >= need, ACMI_ERR_WS, "acmi_kfac_output_stats_finish: workspace of %lld floats < %lld",
               (long long)ws_s_floats, need);
  hipStream_t s = (hipStream_t)stream;
  const char* prep = static_cast<const char*>(net->conv_prep);
  if (L.C3 == 32)
    return output_stats_impl<32>(L, net->params, B, acts, bwd_s, 0, 0, 0, g_stats, ws_s, ws_s_floats, s, prep, 2);
  return output_stats_impl<64>(L, net->params, B, acts, bwd_s, 0, 0, 0, g_stats, ws_s, ws_s_floats, s, prep, 2);
}

int acmi_stream_wait_backward_dx(acmi_stream_t stream) {
  hipEvent_t* ev = dx_done_event();
  ACMI_REQUIRE(ev && hipStreamWaitEvent((hipStream_t)stream, *ev, 0) == hipSuccess, ACMI_ERR_HIP,
               "acmi_stream_wait_backward_dx failed");
  return ACMI_OK;
}

// acmi_kfac_output_stats / acmi_kfac_output_stats_masked (legal: nullptr / one word per row)
static int output_stats_entry(const acmi_net_t* net, int B, const acmi_acts_t* acts,
                              const acmi_bwd_t* bwd, uint32_t seed, uint32_t row_offset,
                              uint32_t counter, float* g_stats, float* ws, int64_t ws_floats,
                              const uint32_t* legal, acmi_stream_t stream) {
  ACMI_REQUIRE(net_modes_ok(net), ACMI_ERR_ARG, "acmi_kfac_output_stats: bad acmi_net_t mode fields");
  const ModeScope mode_scope(net);
  Layout L;
  ACMI_REQUIRE(net && acts && bwd && g_stats && ws, ACMI_ERR_ARG,
               "acmi_kfac_output_stats: null argument");
  ACMI_REQUIRE(make_layout(net->num_actions, net->conv3_filters, &L), ACMI_ERR_ARG, "bad net");
  ACMI_REQUIRE(B > 0 && spans32(B, 400 * 32, 400 * 32), ACMI_ERR_ARG, "bad B");
  ACMI_REQUIRE(masks_ok(acts), ACMI_ERR_ARG, "acmi_kfac_output_stats: ReLU masks m1..m3 must be all set or all NULL");
  const long long need = acmi_backward_ws_floats(B, net->num_actions, net->conv3_filters);
  ACMI_REQUIRE(ws_floats >= need, ACMI_ERR_WS, "acmi_kfac_output_stats: workspace of %lld floats < %lld",
               (long long)ws_floats, need);
  hipStream_t s = (hipStream_t)stream;
  if (L.C3 == 32)
    return output_stats_impl<32>(L, net->params, B, acts, bwd, seed, row_offset, counter,
                                 g_stats, ws, ws_floats, s, static_cast<const char*>(net->conv_prep), 0, legal);
  return output_stats_impl<64>(L, net->params, B, acts, bwd, seed, row_offset, counter, g_stats,
                               ws, ws_floats, s, static_cast<const char*>(net->conv_prep), 0, legal);
}

int acmi_kfac_output_stats(const acmi_net_t* net, int B, const acmi_acts_t* acts,
                           const acmi_bwd_t* bwd, uint32_t seed, uint32_t row_offset,
                           uint32_t counter, float* g_stats, float* ws, int64_t ws_floats,
                           acmi_stream_t stream) {
  return output_stats_entry(net, B, acts, bwd, seed, row_offset, counter, g_stats, ws, ws_floats, nullptr, stream);
}

int acmi_kfac_output_stats_masked(const acmi_net_t* net, int B, const acmi_acts_t* acts,
                                  const acmi_bwd_t* bwd, uint32_t seed, uint32_t row_offset,
                                  uint32_t counter, const uint32_t* legal, float* g_stats, float* ws,
                                  int64_t ws_floats, acmi_stream_t stream) {
  ACMI_REQUIRE(net, ACMI_ERR_ARG, "acmi_kfac_output_stats_masked: null net");
  ACMI_REQUIRE_MASK("acmi_kfac_output_stats_masked", legal, net->num_actions);
  return output_stats_entry(net, B, acts, bwd, seed, row_offset, counter, g_stats, ws, ws_floats, legal, stream);
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

// Host-only check of the launch planners (no GPU): every sub-tile of the
// upper triangle of P^T P and every (P, dY) sub-tile is produced by sym_plan's
// groups, each column's sum by exactly one wave, for K = 64..max_k; and
// plan_rounds' chunks cover the rows exactly.  0 = ok, else the failing K.
int acmi_debug_convt2(const acmi_net_t* net, int mode, const float* d2a, const float* d2b, const uint32_t* m1,
                      float* d1, int B, float* gram_part, const uint32_t* d2max_a, const uint32_t* d2max_b,
                      uint32_t* d1max, acmi_stream_t stream) {
  ACMI_REQUIRE(net_modes_ok(net), ACMI_ERR_ARG, "acmi_debug_convt2: bad acmi_net_t mode fields");
  const ModeScope mode_scope(net);
  ACMI_REQUIRE(net && net->conv_prep && d2a && d2b && m1 && d1 && gram_part && d2max_a && d2max_b && d1max && B > 0 &&
                   mode >= 0 && mode <= 2,
               ACMI_ERR_ARG, "acmi_debug_convt2: bad arguments");
  const char* p2 = static_cast<const char*>(net->conv_prep) +
                   (net->conv3_filters == 32 ? TowerPrep<32>::BYTES : TowerPrep<64>::BYTES);
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
