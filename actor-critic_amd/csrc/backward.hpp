// The update's backward path (net.hip's acmi_backward / acmi_backward_stacked /
// acmi_kfac_output_stats[_masked] / acmi_kfac_output_stats_finish): the argument
// check the entry points share, the two workspace views, the input-gradient (dX)
// chain heads -> d4 -> d3 -> d2 -> d1 of the loss and of the sampled loss, the
// weight gradients with the K-FAC A factors, the sampled head gradients with the
// G factors, and the stacked form that runs conv2's input gradient of both chains
// as one launch.
//
// Part of net.hip's translation unit: it is included after forward.hpp (dispatch_c3,
// spans32, PrepView) and splitk.hpp (wgrad_layer / gcov_layer, PartRanges, the
// prefix sizes), and uses net.hip's Layout, masks_ok, net_modes_ok and mode globals.
#pragma once

#include <atomic>
#include <type_traits>

#include "band.hpp"
#include "convt2.hpp"
#include "convt3.hpp"
#include "gemm.hpp"
#include "gemm3.hpp"
#include "prepview.hpp"
#include "stepper.hpp"

namespace acmi {

// ---------------------------------------------------------------------------
// what the five entry points check before anything is launched
// ---------------------------------------------------------------------------
// fn: the entry point's name, in every message.  nonnull: its own pointer
// arguments.  The backward entries (with_obs) take observations and a loss chain
// (bwd: its ldh); the output-statistics entries do not.  masks (nullable): the
// acmi_acts_t whose ReLU masks must be all set or all NULL.  Argument errors come
// before ACMI_ERR_WS: every workspace in ws_floats holds acmi_backward_ws_floats.
struct UpdateArgs {
  const char* fn;
  bool nonnull;
  const acmi_acts_t* masks;
  bool with_obs;
  const uint8_t* obs;
  bool obs8;  // conv1's A factor runs (a_stats): 8-byte patch loads (afactor_u8.hip)
  long long img_stride;
  const acmi_bwd_t* bwd;
  bool distinct;  // acmi_backward_stacked: the two chains' buffers differ
  long long ws_floats[2];
};
static int check_update_args(const acmi_net_t* net, int B, const UpdateArgs& u, Layout* L) {
  ACMI_REQUIRE(net_modes_ok(net), ACMI_ERR_ARG, "%s: bad acmi_net_t mode fields", u.fn);
  ACMI_REQUIRE(net && u.nonnull, ACMI_ERR_ARG, "%s: null argument", u.fn);
  const bool masks = !u.masks || masks_ok(u.masks);
  if (u.with_obs) ACMI_REQUIRE(masks, ACMI_ERR_ARG, "%s: ReLU masks m1..m3 must be all set or all NULL", u.fn);
  ACMI_REQUIRE(make_layout(net->num_actions, net->conv3_filters, L), ACMI_ERR_ARG, "%s: bad net", u.fn);
  if (u.with_obs) {
    ACMI_REQUIRE(B > 0 && u.img_stride >= 84 * 84 * 4 && u.img_stride % 4 == 0, ACMI_ERR_ARG,
                 "%s: bad B / img_stride", u.fn);
    // the widest load from obs: uint32 (conv1's weight gradient from the u8 patches,
    // ConvRows<uint8_t>::stage), 8 bytes with the conv1 A factor
    const int al = u.obs8 ? 8 : 4;
    ACMI_REQUIRE((uintptr_t)u.obs % al == 0 && u.img_stride % al == 0, ACMI_ERR_ARG,
                 "%s: obs and img_stride must be multiples of %d bytes%s", u.fn, al,
                 u.obs8 ? " (with a_stats: the conv1 A factor loads 8 bytes)" : "");
    ACMI_REQUIRE(u.bwd->ldh >= net->num_actions + 1 && u.bwd->ldh % 4 == 0, ACMI_ERR_ARG,
                 "%s: ldh must be >= A+1 and a multiple of 4 (zero padded)", u.fn);
    ACMI_REQUIRE(spans32(B, u.img_stride, 84 * 84 * 4) && spans32(B, 400 * 32, 400 * 32), ACMI_ERR_ARG,
                 "%s: batch spans >= 2^31 elements (B=%d)", u.fn, B);
    ACMI_REQUIRE(u.distinct, ACMI_ERR_ARG, "%s: the two chains need their own workspaces and d1..d4", u.fn);
  } else {
    ACMI_REQUIRE(B > 0 && spans32(B, 400 * 32, 400 * 32), ACMI_ERR_ARG, "%s: bad B", u.fn);
    ACMI_REQUIRE(masks, ACMI_ERR_ARG, "%s: ReLU masks m1..m3 must be all set or all NULL", u.fn);
  }
  const long long need = acmi_backward_ws_floats(B, L->A, L->C3);
  ACMI_REQUIRE(u.ws_floats[0] >= need && u.ws_floats[1] >= need, ACMI_ERR_WS, "%s: workspace of %lld floats < %lld",
               u.fn, std::min(u.ws_floats[0], u.ws_floats[1]), need);
  return ACMI_OK;
}

// ---------------------------------------------------------------------------
// the two layouts of the update's workspace (splitk.hpp: one size for both)
// ---------------------------------------------------------------------------
// Both start with kBandScratch words of scratch (band.hpp layout): the dX chain's
// epilogues publish max |d4| .. |d1| there, the f16x2 consumers (convt2, the band
// reductions, the wide Grams) scale by them.  The partial region is the rest.
struct BwdWs {  // [scratch | conv1 A-factor ints | partials]
  unsigned* scr;
  int* afactor;
  long long afactor_ints;
  float* part;
  long long cap;
  BwdWs(float* ws, long long ws_floats, int B)
      : scr(reinterpret_cast<unsigned*>(ws)), afactor(reinterpret_cast<int*>(ws + kBandScratch)),
        afactor_ints(afactor_ws_floats(B)), part(ws + bwd_prefix_floats(B)), cap(ws_floats - bwd_prefix_floats(B)) {}
};
struct StatsWs {  // [scratch | sampled head gradients ghead [B][ldg] | partials]
  unsigned* scr;
  float* ghead;
  int ldg;
  float* part;
  long long cap;
  StatsWs(float* ws, long long ws_floats, int B, int A)
      : scr(reinterpret_cast<unsigned*>(ws)), ghead(ws + kBandScratch), ldg((int)head_grad_ldg(A)),
        part(ws + stats_prefix_floats(B, A)), cap(ws_floats - stats_prefix_floats(B, A)) {}
};

// conv1's G factor from conv2 dX: the per-block Gram partials [33][32] that
// convt2's GRAM forms leave at the start of the sampled chain's partial region
static long long conv1_gram_floats(int B) { return (long long)convt2_gram_blocks(B) * 33 * 32; }
// conv2's input gradient of the sampled chain reduces d1 to those partials instead
// of storing it: with prepared weights, in x3 mode, when they fit.  The ONE rule
// for the kernel form launched (dx_conv2, backward_stacked_impl) and for the
// finalize that reads them (g_factors).
static bool conv2_dx_grams_d1(bool prepared, int B, const StatsWs& w) {
  return prepared && g_gemm_mode == ACMI_GEMM_X3 && conv1_gram_floats(B) <= w.cap;
}

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
static int record_dx_done(hipStream_t s) {
  hipEvent_t* ev = dx_done_event();
  ACMI_REQUIRE(ev && hipEventRecord(*ev, s) == hipSuccess, ACMI_ERR_HIP, "acmi_backward: dX event record failed");
  return ACMI_OK;
}

// f(masked, x): ReLU' of a layer from the mask bits the forward wrote (masked =
// std::true_type, x the words) or from its activations (std::false_type)
template <class F>
static __forceinline__ void with_relu_src(const uint32_t* mask, const float* act, F&& f) {
  if (mask) f(std::true_type{}, reinterpret_cast<const float*>(mask));
  else f(std::false_type{}, act);
}

// ---------------------------------------------------------------------------
// backward (dX chain) shared by the loss backward and the sampled backward
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

// the chain up to d2: heads -> d4, fc4 -> d3, conv3 -> d2
template <int C3>
static int dx_chain_pre(const Layout& L, const float* P, int B, const acmi_acts_t* a,
                        const acmi_bwd_t* bw, const float* dhead, int ldh,
                        hipStream_t s, const PrepView<C3>& prep, unsigned* dxs) {
  // dxs: the chain's scratch words (BwdWs / StatsWs scr)
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
  const bool hdr = prep.hdr() != nullptr;
  const unsigned* w3max = hdr ? prep.bound(kTowMaxW3) : dxs + kBsMaxW3;
  const unsigned* w4max = hdr ? prep.bound(kTowMaxW4) : dxs + kBsMaxW4;
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
    prof_begin(ACMI_PROF_FC4_DX, s);
    with_relu_src(a->m3, a->a3, [&](auto masked, const float* x) {
      run(EpiReluGrad<decltype(masked)::value>{bw->d3, x, K3, dxs + kBsMaxD3});
    });
    prof_end(ACMI_PROF_FC4_DX, s);
  }
  // conv input gradients as transposed products: rows = (phase, channel) of
  // the weights, columns = (super-)pixels gathering dY (EpiConvT, float4 rows)
  {  // conv3 -> d2 (stride 1: one phase), its weights pre-split in the prepared buffer
    using Src = ConvTRows<9, 9, 3, 3, 1, C3>;
    using W = ConvTWeights<3, 3, 1, 64, C3>;
    W opA{P + L.off[4]};
    RowsAsK<Src> opB{Src{bw->d3, B * Src::L}};
    auto run = [&](auto epi) {
      if (g_gemm_mode == ACMI_GEMM_X3)
        // f16x2 operands: the scales of max |W3| and of max |d3| (the fc4 dX epilogue's)
        launch_convt_x3<9, 9, 3, 3, 1, 64, C3, 256>(P + L.off[4], prep.ct3(), bw->d3, B, epi, w3max, dxs + kBsMaxD3,
                                                    s);
      else
        launch_mm<64, 128, 16, 1, 2, false, false, 16>(opA, opB, epi, W::N, B * Src::L, Src::COLS, 1, 0, s);
    };
    prof_begin(ACMI_PROF_CONV3_DX, s);
    with_relu_src(a->m2, a->a2, [&](auto masked, const float* x) {
      run(EpiConvT<9, 9, 1, 64, decltype(masked)::value>{bw->d2, x, dxs + kBsMaxD2});
    });
    prof_end(ACMI_PROF_CONV3_DX, s);
  }
  ACMI_LAUNCH_CHECK("dx_chain");
  return ACMI_OK;
}

// (Measured and removed: conv2's input gradient on the dY-im2col-in-LDS kernel
// of convt3.hpp, 939 / 620 us per launch at M = 10240 against 444 on gemm3 -- its
// f32 dY image leaves one block per CU; conv1 / conv2 forwards on convfwd3.hpp,
// 26.5 / 82 us at 512 images against 26.5 / 30.  conv3's input gradient and
// forward keep those kernels: 231 -> 186 us, 19.6 -> 18.7 us.)

// which form of conv2's input gradient dx_conv2 launches (acmi_debug_convt2_form):
// -1 = by the tile-count thresholds of convt2.hpp, 0 = staging, 1 = resident
static std::atomic<int> g_convt2_form{-1};
static bool convt2_use_resident(int B, bool gram) {
  const int f = g_convt2_form.load(std::memory_order_relaxed);
  return f < 0 ? convt2_resident_default(B, gram) : f != 0;
}

// conv2's input gradient, from d2 (max |d2| in dxs): the loss chain stores the
// masked d1 (gram null); the sampled chain (gram: its workspace) reduces it to
// conv1's G-factor Gram partials where conv2_dx_grams_d1 says so
template <int C3>
static int dx_conv2(const Layout& L, const float* P, int B, const acmi_acts_t* a, const acmi_bwd_t* bw,
                    hipStream_t s, const PrepView<C3>& prep, const StatsWs* gram, unsigned* dxs) {
  // conv2 -> d1 (stride 2: the four phases of a 2x2 super-pixel are the
  // 4 x 32 rows of one product over the 10x10 super-pixels)
  using Src = ConvTRows<20, 20, 4, 4, 2, 64>;
  using W = ConvTWeights<4, 4, 2, 32, 64>;
  W opA{P + L.off[2]};
  RowsAsK<Src> opB{Src{bw->d2, B * Src::L}};
  const char* p2 = prep.ct2();
  float* gram_part = gram && conv2_dx_grams_d1(p2 != nullptr, B, *gram) ? gram->part : nullptr;
  prof_begin(ACMI_PROF_CONV2_DX, s);
  // (max |d1|: conv1's f16x2 weight gradient; ReLU'(a1) from the mask bits when written)
  with_relu_src(a->m1, a->a1, [&](auto masked, const float* act1) {
    constexpr bool MK = decltype(masked)::value;
    if (p2 && g_gemm_mode == ACMI_GEMM_X3) {
      // pre-split weights, four phases per wave (convt2.hpp); the sampled-loss
      // chain reduces d1 to its Gram partials instead of storing it
      auto go = [&](auto GRAMc) {
        constexpr bool GR = decltype(GRAMc)::value;
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
      if (gram_part) go(std::true_type{});
      else go(std::false_type{});
    } else {
      launch_mm<128, 128, 16, 2, 2, false, false, 16>(opA, opB, EpiConvT<20, 20, 2, 32, MK>{bw->d1, act1, dxs + kBsMaxD1},
                                                      W::N, B * Src::L, Src::COLS, 1, 0, s);
    }
  });
  prof_end(ACMI_PROF_CONV2_DX, s);
  ACMI_LAUNCH_CHECK("dx_conv2");
  return ACMI_OK;
}

template <int C3>
static int dx_chain(const Layout& L, const float* P, int B, const acmi_acts_t* a, const acmi_bwd_t* bw,
                    const float* dhead, int ldh, hipStream_t s, const PrepView<C3>& prep, const StatsWs* gram,
                    unsigned* dxs) {
  const int rc = dx_chain_pre<C3>(L, P, B, a, bw, dhead, ldh, s, prep, dxs);
  if (rc) return rc;
  return dx_conv2<C3>(L, P, B, a, bw, s, prep, gram, dxs);
}

// The weight gradients and the A factors, after the loss chain's dX (d1..d4 in bw,
// the maxima in w.scr)
template <int C3>
static int wgrad_chain(const Layout& L, const float* P, const uint8_t* obs, long long img_stride, int B,
                       const acmi_acts_t* a, const acmi_bwd_t* bw, float* grads, float* astat, const BwdWs& w,
                       hipStream_t s, const PrepView<C3>& prep) {
  const bool st = astat != nullptr;
  // conv1's weight gradient is fused into the A-factor pass (bf16x3 mode; it needs
  // d1, so the pass follows the dX chain).  (Measured and removed: the A factor on a
  // library side stream next to the dX chain, 5.69 vs 5.64 ms per update -- the i8
  // gather competes with the symmetric reductions for L2 and LDS; the A factor
  // before the dX chain.)
  const bool fuse_c1 = st && g_gemm_mode == ACMI_GEMM_X3;
  unsigned* bscr = w.scr;
  float* part = w.part;
  const long long avail = w.cap;
  const bool band = band_on(st);
  int rc = ACMI_OK;
  float* wpart_c1 = nullptr;  // conv1's fused weight-gradient partials (in the A-factor workspace)
  if (st) {
    prof_begin(ACMI_PROF_CONV1_AFACTOR, s);
    const int rc0 = conv1_afactor_u8(obs, img_stride, B, astat + L.stat_off[0], w.afactor, w.afactor_ints, s,
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
  const unsigned* a3b = prep.bound(kTowMaxA3);
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
  const bool xb = prep.hdr() != nullptr;
  const unsigned* a1b = xb ? prep.bound(kTowMaxA1) : bscr + kBsMaxA1;
  const unsigned* a2b = xb ? prep.bound(kTowMaxA2) : bscr + kBsMaxA2;
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

// acmi_backward: the loss chain's dX, the dX event, then the weight gradients
template <int C3>
static int backward_impl(const Layout& L, const float* P, const uint8_t* obs, long long img_stride, int B,
                         const acmi_acts_t* a, const acmi_bwd_t* bw, float* grads, float* astat, float* ws,
                         long long ws_cap, hipStream_t s, const PrepView<C3>& prep) {
  const BwdWs w(ws, ws_cap, B);
  int rc = dx_chain<C3>(L, P, B, a, bw, bw->dhead, bw->ldh, s, prep, nullptr, w.scr);
  if (rc) return rc;
  rc = record_dx_done(s);
  if (rc) return rc;
  return wgrad_chain<C3>(L, P, obs, img_stride, B, a, bw, grads, astat, w, s, prep);
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
// into w.ghead; legal (nullable): per-row legal-action words
static void launch_sampled_head_grad(const acmi_acts_t* a, int B, int A, uint32_t seed, uint32_t row0, uint32_t ctr,
                                     const StatsWs& w, const uint32_t* legal, hipStream_t s) {
  const auto kern = legal ? sampled_head_grad_kernel<true> : sampled_head_grad_kernel<false>;
  hipLaunchKernelGGL(kern, dim3(cdiv(B, 128)), dim3(128), 0, s, a->logits, a->ld_logits, B, A, seed, row0, ctr,
                     w.ghead, w.ldg, legal);
}

// The G factors from what a sampled chain left in bw (d1..d4) and in its workspace
// (the head gradients, the scratch maxima, and -- conv1_from_gram, the value of
// conv2_dx_grams_d1 for that chain -- conv1's Gram partials in place of d1)
static int g_factors(const Layout& L, int B, const acmi_bwd_t* bw, float* gstat, const StatsWs& w,
                     bool conv1_from_gram, hipStream_t s) {
  const int C3 = L.C3;
  // the G factors' finalizes deferred into one launch: every Gram's partials in
  // their own range of the workspace
  PartRanges<CovSet> ra{w.part, w.cap, s};
  int rc = ACMI_OK;
  if (conv1_from_gram) {  // the conv2 dX kernel's per-block Gram partials (the first range)
    const int nc = convt2_gram_blocks(B);
    const long long floats = conv1_gram_floats(B);
    const float* g1_part = ra.begin(floats);
    ra.add(g1_part, nc, 32, 32, gstat + L.stat_off[5 + 0], (int)(400LL * B), 1);
    rc = ra.end(floats);
    if (rc) return rc;
  }
  // heads: G_pi (A x A) from the first A columns, G_v = element (A, A)
  rc = gcov_layer(w.ghead, w.ldg, L.A + 1, B, L.A, ra, gstat + L.stat_off[5 + 4], gstat + L.stat_off[5 + 5], L.A);
  if (rc) return rc;
  // (the dX chain published max |d4| and max |d2| into the scratch)
  rc = gcov_layer(bw->d4, 512, 512, B, 512, ra, gstat + L.stat_off[5 + 3], nullptr, -1, w.scr + kBsMaxD4);
  if (rc) return rc;
  rc = gcov_layer(bw->d3, C3, C3, 49LL * B, C3, ra, gstat + L.stat_off[5 + 2]);
  if (rc) return rc;
  rc = gcov_layer(bw->d2, 64, 64, 81LL * B, 64, ra, gstat + L.stat_off[5 + 1], nullptr, -1, w.scr + kBsMaxD2);
  if (rc) return rc;
  if (!conv1_from_gram) rc = gcov_layer(bw->d1, 32, 32, 400LL * B, 32, ra, gstat + L.stat_off[5 + 0]);
  if (rc) return rc;
  ra.flush();
  ACMI_LAUNCH_CHECK("G factor finalize");
  return ACMI_OK;
}

// acmi_kfac_output_stats[_masked]: the sampled head gradients, their dX chain, the
// G factors.  legal (nullable): per-row legal-action words
template <int C3>
static int output_stats_impl(const Layout& L, const float* P, int B, const acmi_acts_t* a, const acmi_bwd_t* bw,
                             uint32_t seed, uint32_t row0, uint32_t ctr, float* gstat, float* ws, long long ws_cap,
                             hipStream_t s, const PrepView<C3>& prep, const uint32_t* legal) {
  const StatsWs w(ws, ws_cap, B, L.A);
  launch_sampled_head_grad(a, B, L.A, seed, row0, ctr, w, legal, s);
  const int rc = dx_chain<C3>(L, P, B, a, bw, w.ghead, w.ldg, s, prep, &w, w.scr);
  if (rc) return rc;
  return g_factors(L, B, bw, gstat, w, conv2_dx_grams_d1(prep.base != nullptr, B, w), s);
}

// acmi_backward + the input-gradient half of acmi_kfac_output_stats, with conv2's
// input gradient of both chains as ONE launch (convt2_kernel MIX: one W2^T
// stream, the loss chain's tiles storing d1, the sampled chain's reducing
// conv1's G-factor Gram); the G factors follow in acmi_kfac_output_stats_finish
// (g_factors).  Bit-identical to the two calls.
template <int C3>
static int backward_stacked_impl(const Layout& L, const float* P, const uint8_t* obs, long long img_stride, int B,
                                 const acmi_acts_t* a, const acmi_bwd_t* bw, float* grads, float* astat, float* ws,
                                 long long ws_cap, const acmi_bwd_t* bws, uint32_t seed, uint32_t row0, uint32_t ctr,
                                 float* wss, long long wss_cap, hipStream_t s, const PrepView<C3>& prep) {
  const BwdWs w(ws, ws_cap, B);
  const StatsWs v(wss, wss_cap, B, L.A);
  int rc = dx_chain_pre<C3>(L, P, B, a, bw, bw->dhead, bw->ldh, s, prep, w.scr);
  if (rc) return rc;
  // the sampled chain's head gradients and its chain up to d2
  launch_sampled_head_grad(a, B, L.A, seed, row0, ctr, v, nullptr, s);
  rc = dx_chain_pre<C3>(L, P, B, a, bws, v.ghead, v.ldg, s, prep, v.scr);
  if (rc) return rc;
  if (conv2_dx_grams_d1(prep.base != nullptr, B, v)) {
    prof_begin(ACMI_PROF_CONV2_DX, s);
    with_relu_src(a->m1, a->a1, [&](auto masked, const float* act1) {
      hipLaunchKernelGGL((convt2_kernel<true, decltype(masked)::value, true>), dim3(convt2_gram_blocks(B)), dim3(256),
                         0, s, prep.ct2(), bw->d2, act1, bw->d1, B, v.part, w.scr + kBsMaxD2, w.scr + kBsMaxD1,
                         bws->d2, v.scr + kBsMaxD2);
    });
    prof_end(ACMI_PROF_CONV2_DX, s);
    ACMI_LAUNCH_CHECK("stacked conv2 dX");
  } else {  // the two launches (no prepared weights / f32 mode / a workspace without room for the Gram)
    rc = dx_conv2<C3>(L, P, B, a, bw, s, prep, nullptr, w.scr);
    if (rc) return rc;
    rc = dx_conv2<C3>(L, P, B, a, bws, s, prep, &v, v.scr);
    if (rc) return rc;
  }
  rc = record_dx_done(s);
  if (rc) return rc;
  return wgrad_chain<C3>(L, P, obs, img_stride, B, a, bw, grads, astat, w, s, prep);
}

}  // namespace acmi
