// The split-K reduction of the update (net.hip's weight gradients, A factors and
// G factors): every layer writes per-chunk partials [nchunk][I+1][J] into a range
// of the caller's workspace, and a "finalize" sums the chunks in a fixed order
// into the output -- bit-identical for every legal workspace size.  Here: the
// finalize descriptors, bodies and the two task-set kernels, the narrow streaming
// Gram, the plans, wgrad_layer / gcov_layer, the range allocator they share and
// the workspace-size helpers.
//
// Part of net.hip's translation unit: it is included after the mode globals
// (g_gemm_mode, g_conv_stats_mode), prof_begin / prof_end and roundup4 that it uses.
#pragma once

#include <algorithm>
#include <atomic>
#include <type_traits>

#include "band.hpp"
#include "conv1u8.hpp"
#include "gemm.hpp"
#include "gemm3.hpp"

namespace acmi {

// ---------------------------------------------------------------------------
// split-K weight-gradient / factor reduction
// ---------------------------------------------------------------------------
// part: [nchunk][I+1][J] with J = kp + cout_pad + (kp ? 1 : 0).
// grad (layer [W;b], (K+1) x cout, optionally split into two column groups
// for the fused heads) and astat ((K+1)^2, symmetric, / rows).
struct WgradDesc {
  const float* part;
  int nchunk;
  int I;  // = K
  int J;
  int kp;       // 0 or K
  int cout;
  float* gradA;  // columns [0, nsplit)
  int nsplit;
  float* gradB;  // columns [nsplit, cout)
  float* astat;  // nullable
  int rows;
  float wscale;  // applied to the weight rows (a < K) of the gradient
};

// One block = 32 consecutive outputs x 8 chunk groups: group g sums chunks
// g, g+8, ... in order (4 loads in flight), then the 8 group sums are added in
// group order -- a fixed order (deterministic) with 8x the loads in flight of one
// thread per output.  Outputs: the gradient rows (K+1) x cout, then the upper
// triangle of the A factor (written to both halves).
constexpr int kFinGroups = 8;
__device__ __forceinline__ float chunk_sum_group(const float* p, int n, long long cs, int g) {
  float s = 0.f;
  for (int c0 = g; c0 < n; c0 += 4 * kFinGroups) {
    float v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int c = c0 + u * kFinGroups;
      v[u] = p[(long long)(c < n ? c : g) * cs];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) s += (c0 + u * kFinGroups < n) ? v[u] : 0.f;
  }
  return s;
}

__device__ __forceinline__ void finalize_wgrad_body(const WgradDesc& d, int bx, float (*red)[32]) {
  const int K = d.I;
  const long long ngrad = (long long)(K + 1) * d.cout;
  const long long nstat = d.astat ? (long long)(K + 1) * (K + 1) : 0;
  const int el = threadIdx.x & 31, g = threadIdx.x >> 5;
  const long long idx = (long long)bx * 32 + el;
  const long long cs = (long long)(d.I + 1) * d.J;  // chunk stride
  // the partial this output sums (nullptr: nothing to sum)
  const float* p = nullptr;
  int a = 0, b = 0, n = 0;
  if (idx < ngrad) {
    a = (int)(idx / d.cout);
    n = (int)(idx - (long long)a * d.cout);
    const int row = a < K ? a : d.I;
    p = d.part + (long long)row * d.J + d.kp + n;
  } else if (idx < ngrad + nstat) {
    const long long e = idx - ngrad;
    a = (int)(e / (K + 1));
    b = (int)(e - (long long)a * (K + 1));
    // column K (the homogeneous coordinate) = sum of P = column-sum row
    if (a <= b && a != K) p = b < K ? d.part + (long long)a * d.J + b : d.part + (long long)d.I * d.J + a;
  }
  red[g][el] = p ? chunk_sum_group(p, d.nchunk, cs, g) : 0.f;
  __syncthreads();
  if (g != 0 || idx >= ngrad + nstat) return;
  float s = 0.f;
#pragma unroll
  for (int q = 0; q < kFinGroups; ++q) s += red[q][el];
  if (idx < ngrad) {
    if (a < K) s *= d.wscale;
    if (n < d.nsplit) d.gradA[(long long)a * d.nsplit + n] = s;
    else d.gradB[(long long)a * (d.cout - d.nsplit) + (n - d.nsplit)] = s;
  } else {
    if (a > b) return;
    if (a == K) s = (float)d.rows;
    s *= 1.0f / (float)d.rows;
    d.astat[(long long)a * (K + 1) + b] = s;
    d.astat[(long long)b * (K + 1) + a] = s;
  }
}

// Gradient outputs (d.astat == nullptr) of a partial with few chunks (<= 8): one
// thread per output instead of 32 outputs x 8 chunk groups per block (7 of the 8
// groups idle at one chunk: the fc4 gradient's 803 K outputs were 25 K blocks).
// The same sums in the same order: group g holds chunk g alone (0 + p[g]), the
// groups added in order from 0.
__device__ __forceinline__ void finalize_grad_thread_body(const WgradDesc& d, int bx) {
  const int K = d.I;
  const long long idx = (long long)bx * 256 + threadIdx.x;
  if (idx >= (long long)(K + 1) * d.cout) return;
  const int a = (int)(idx / d.cout), n = (int)(idx - (long long)a * d.cout);
  const float* p = d.part + (long long)(a < K ? a : d.I) * d.J + d.kp + n;
  const long long cs = (long long)(d.I + 1) * d.J;
  float v[kFinGroups];
#pragma unroll
  for (int g = 0; g < kFinGroups; ++g) v[g] = p[(long long)(g < d.nchunk ? g : 0) * cs];
  float s = 0.f;
#pragma unroll
  for (int g = 0; g < kFinGroups; ++g) s += g < d.nchunk ? 0.f + v[g] : 0.f;
  if (a < K) s *= d.wscale;
  if (n < d.nsplit) d.gradA[(long long)a * d.nsplit + n] = s;
  else d.gradB[(long long)a * (d.cout - d.nsplit) + (n - d.nsplit)] = s;
}
__device__ __forceinline__ bool fin_thread_ok(const WgradDesc& d) { return !d.astat && d.nchunk <= kFinGroups; }
inline int fin_blocks(const WgradDesc& d) {
  const long long total = (long long)(d.I + 1) * d.cout + (d.astat ? (long long)(d.I + 1) * (d.I + 1) : 0);
  return (int)(!d.astat && d.nchunk <= kFinGroups ? cdiv(total, 256) : cdiv(total, 32));
}

// The A factor of a split-K wgrad partial ((K+1)^2, symmetric): one block per
// 32x32 tile of the upper triangle; each element sums its chunks in exactly
// finalize_wgrad_body's order (chunk group g = c mod 8 in chunk order, then
// the groups in order), is stored at (a, b) and, through an LDS transpose, at
// (b, a) -- both halves written by coalesced rows (the element-per-thread
// mirror store of finalize_wgrad_body is a 4-byte scatter with stride K+1).
__device__ __forceinline__ void finalize_afactor_body(const WgradDesc& d, int ntile, int bx, float (*tr)[33]) {
  const int K = d.I, K1 = K + 1;
  // upper-triangle tile (ta <= tb) of linear index bx
  int t = bx, ta = 0;
  while (t >= ntile - ta) t -= ntile - ta, ++ta;
  const int tb = ta + t;
  const long long cs = (long long)(d.I + 1) * d.J;
  const int c = threadIdx.x & 31, r0 = threadIdx.x >> 5;
  const float inv = 1.0f / (float)d.rows;
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int r = r0 + 8 * it;
    const int a = 32 * ta + r, b = 32 * tb + c;
    float v = 0.f;
    if (a < K1 && b < K1 && a <= b) {
      if (a == K) {
        v = (float)d.rows * inv;  // rows * fl(1/rows), as finalize_wgrad_body (1 - 2^-24 for some rows)
      } else {
        const float* p = b < K ? d.part + (long long)a * d.J + b : d.part + (long long)d.I * d.J + a;
        float s = 0.f;
        for (int g = 0; g < kFinGroups; ++g) {
          float sg = 0.f;
          for (int ch = g; ch < d.nchunk; ch += kFinGroups) sg += p[(long long)ch * cs];
          s += sg;
        }
        v = s * inv;
      }
      d.astat[(long long)a * K1 + b] = v;
    }
    tr[r][c] = v;
  }
  __syncthreads();
#pragma unroll
  for (int it = 0; it < 4; ++it) {  // (b, a) for a < b: row b of the output reads column b of the tile
    const int r = r0 + 8 * it;     // row offset inside tile tb
    const int b = 32 * tb + r, a = 32 * ta + c;
    if (a < K1 && b < K1 && a < b) d.astat[(long long)b * K1 + a] = tr[c][r];
  }
}
inline int afactor_tiles(const WgradDesc& d) { return cdiv(d.I + 1, 32); }

// One or several layers' weight-gradient / A-factor finalizes as one launch
// (each layer's split-K partials in their own workspace range): task k owns
// blocks [blk0, blk0 of k+1) and runs finalize_wgrad_body or
// finalize_grad_thread_body (kind 0) or finalize_afactor_body (kind 1).
struct WgradTask {
  WgradDesc d;
  int kind, ntile, blk0;
};
struct WgradSet {
  static constexpr int kTasks = 6;
  static constexpr const char* kWhat = "layer";  // (PartRanges' messages)
  int n = 0;
  int blocks = 0;
  WgradTask t[kTasks];
  void add(const WgradDesc& d, int kind) {
    const int nt = kind == 1 ? afactor_tiles(d) : 0;
    t[n++] = WgradTask{d, kind, nt, blocks};
    blocks += kind == 1 ? nt * (nt + 1) / 2 : fin_blocks(d);
  }
  void launch(hipStream_t s) const;
};
__global__ __launch_bounds__(256) void finalize_wgrad_multi_kernel(WgradSet S) {
  __shared__ float red[kFinGroups][32];
  __shared__ float tr[32][33];
  int k = 0;
  while (k + 1 < S.n && (int)blockIdx.x >= S.t[k + 1].blk0) ++k;
  const WgradTask& T = S.t[k];
  const int b = blockIdx.x - T.blk0;
  if (T.kind == 0) {
    if (fin_thread_ok(T.d)) finalize_grad_thread_body(T.d, b);
    else finalize_wgrad_body(T.d, b, red);
  } else {
    finalize_afactor_body(T.d, T.ntile, b, tr);
  }
}
inline void WgradSet::launch(hipStream_t s) const {
  hipLaunchKernelGGL(finalize_wgrad_multi_kernel, dim3(blocks), dim3(256), 0, s, *this);
}

// G factor: part [nchunk][I+1][J] (I == J == n, no colsum row used); out is
// sub x sub, taken from the top-left of the n x n product, / rows.  Every body
// sums the chunks in a fixed order, so the result is deterministic; each is
// followed by the blocks it takes.
struct CovTask {
  const float* part;
  float* out;
  int nchunk, n, sub, rows, kind, a, blk0;
};

// kind 0: thread per upper-triangle element (few chunks): consecutive threads
// read consecutive partials, the value is written to both halves
__device__ __forceinline__ void finalize_cov_thread_body(const CovTask& T, int bx) {
  const long long cs = (long long)(T.n + 1) * T.n;
  const int idx = bx * 256 + threadIdx.x;
  if (idx >= T.sub * T.sub) return;
  const int a = idx / T.sub, c = idx - a * T.sub;
  if (a > c) return;
  const float v = chunk_sum(T.part + (long long)a * T.n + c, T.nchunk, cs) * (1.0f / (float)T.rows);
  T.out[a * T.sub + c] = v;
  T.out[c * T.sub + a] = v;
}
inline int cov_thread_blocks(int sub) { return cdiv(sub * sub, 256); }

// kind 3: kind 0's sums on 32 x 32 upper-triangle tiles, both halves written by
// coalesced rows through an LDS transpose (kind 0's mirror store is a 4-byte
// scatter with stride sub: the 512-wide G factor's half)
__device__ __forceinline__ void finalize_cov_tile_body(const CovTask& T, int bx, float (*tr)[33]) {
  const long long cs = (long long)(T.n + 1) * T.n;
  const int ntile = (T.sub + 31) / 32;
  int t = bx, ta = 0;
  while (t >= ntile - ta) t -= ntile - ta, ++ta;
  const int tb = ta + t;
  const int c = threadIdx.x & 31, r0 = threadIdx.x >> 5;
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int r = r0 + 8 * it;
    const int a = 32 * ta + r, cc = 32 * tb + c;
    float v = 0.f;
    if (a < T.sub && cc < T.sub && a <= cc) {
      v = chunk_sum(T.part + (long long)a * T.n + cc, T.nchunk, cs) * (1.0f / (float)T.rows);
      T.out[a * T.sub + cc] = v;
    }
    tr[r][c] = v;
  }
  __syncthreads();
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int r = r0 + 8 * it;
    const int bb = 32 * tb + r, a = 32 * ta + c;
    if (a < T.sub && bb < T.sub && a < bb) T.out[bb * T.sub + a] = tr[c][r];
  }
}
inline int cov_tile_blocks(int sub) {
  const int nt = cdiv(sub, 32);
  return nt * (nt + 1) / 2;
}

// kind 1: wave per element (many chunks: the lanes split the chunks, then a
// butterfly), 4 elements per block; kind 2: G of the value head, element
// (T.a, T.a) of the heads product, by the block's first wave
__device__ __forceinline__ void finalize_cov_wave_body(const CovTask& T, int bx) {
  const long long cs = (long long)(T.n + 1) * T.n;
  const int idx = T.kind == 1 ? bx * 4 + (threadIdx.x >> 6) : 0;
  const int lane = threadIdx.x & 63;
  if (idx >= T.sub * T.sub || (T.kind == 2 && threadIdx.x >= 64)) return;
  int lo, hi;
  if (T.kind == 1) {
    const int a = idx / T.sub, c = idx - a * T.sub;
    lo = a < c ? a : c, hi = a < c ? c : a;
  } else {
    lo = hi = T.a;
  }
  const float* p = T.part + (long long)lo * T.n + hi;
  float v = 0.f;
  for (int c = lane; c < T.nchunk; c += 64) v += p[c * cs];
  v = wave_sum(v);
  if (lane == 0) T.out[idx] = v * (1.0f / (float)T.rows);
}
inline int cov_wave_blocks(int kind, int sub) { return kind == 1 ? cdiv(sub * sub, 4) : 1; }

// The sampled-loss chain's G-factor finalizes as ONE launch after all its Grams
// (each Gram's partials in its own workspace range): task k owns blocks
// [blk0, blk0 of k+1) and runs the body of its kind.
struct CovSet {
  static constexpr int kTasks = 8;
  static constexpr const char* kWhat = "Gram";  // (PartRanges' messages)
  int n = 0;
  int blocks = 0;
  CovTask t[kTasks];
  void add(const float* part, int nchunk, int n_, int sub, float* out, int rows, int kind, int a = 0) {
    t[n++] = CovTask{part, out, nchunk, n_, sub, rows, kind, a, blocks};
    blocks += kind == 0 ? cov_thread_blocks(sub) : kind == 3 ? cov_tile_blocks(sub) : cov_wave_blocks(kind, sub);
  }
  void launch(hipStream_t s) const;
};
__global__ __launch_bounds__(256) void finalize_cov_multi_kernel(CovSet S) {
  __shared__ float tr[32][33];
  int k = 0;
  while (k + 1 < S.n && (int)blockIdx.x >= S.t[k + 1].blk0) ++k;
  const CovTask& T = S.t[k];
  const int b = blockIdx.x - T.blk0;
  if (T.kind == 3) finalize_cov_tile_body(T, b, tr);
  else if (T.kind == 0) finalize_cov_thread_body(T, b);
  else finalize_cov_wave_body(T, b);
}
inline void CovSet::launch(hipStream_t s) const {
  hipLaunchKernelGGL(finalize_cov_multi_kernel, dim3(blocks), dim3(256), 0, s, *this);
}

// G = D^T D for narrow D (n <= NP, NP in {32, 64}) straight from global memory:
// each wave streams row pairs (lane l: row 2q + (l>>5), column l&31 [+32]) as
// the A and B fragments of v_mfma_f32_32x32x2_f32 (the Gram tile is D^T D of
// the same registers).  Two register sets of UNR k-steps: the next group's
// loads are issued before this group's MFMAs.  The block's 4 waves are summed
// into one LDS image in wave order (deterministic) and stored as
// part[chunk][NP+1][NP] (summed by finalize_cov_thread_body / finalize_cov_wave_body).
template <int NP>
__global__ __launch_bounds__(256) void gram_small_kernel(const float* D, int ld, int n,
                                                        long long rows, long long chunk,
                                                        float* part) {
  constexpr int T = NP / 32;           // column tiles
  constexpr int NT = T * (T + 1) / 2;  // upper-triangle tile pairs
  constexpr int UNR = 8;
  __shared__ float red[NP * NP];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int h = lane >> 5, c = lane & 31;
  const long long r0 = (long long)blockIdx.x * chunk;
  const long long r1 = min(rows, r0 + chunk);
  f32x16 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  const float* zero = zero_run();
  auto load = [&](long long base, float (&v)[UNR][T]) {
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const long long row = base + 8 * u + h;
#pragma unroll
      for (int t = 0; t < T; ++t) {
        const int col = c + 32 * t;
        const bool ok = row < r1 && col < n;
        v[u][t] = *(ok ? D + row * ld + col : zero);
      }
    }
  };
  auto mma = [&](const float (&v)[UNR][T]) {
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      int t = 0;
#pragma unroll
      for (int x = 0; x < T; ++x)
#pragma unroll
        for (int y = x; y < T; ++y, ++t)
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(v[u][x], v[u][y], acc[t], 0, 0, 0);
    }
  };
  float va[UNR][T], vb[UNR][T];
  long long base = r0 + 2 * wave;
  load(base, va);
  for (; base < r1; base += 16 * UNR) {
    load(base + 8 * UNR, vb);
    mma(va);
    if (base + 8 * UNR >= r1) break;
    load(base + 16 * UNR, va);
    mma(vb);
  }
  // acc[t][r]: tile (x, y), row 32x + (r&3) + 8(r>>2) + 4h, column 32y + c
  for (int w = 0; w < 4; ++w) {
    if (wave == w) {
      int t = 0;
#pragma unroll
      for (int x = 0; x < T; ++x)
#pragma unroll
        for (int y = x; y < T; ++y, ++t)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int i = 32 * x + (r & 3) + 8 * (r >> 2) + 4 * h, j = 32 * y + c;
            const float prev_ij = w ? red[i * NP + j] : 0.f;
            red[i * NP + j] = prev_ij + acc[t][r];
            if (x != y) {
              const float prev_ji = w ? red[j * NP + i] : 0.f;
              red[j * NP + i] = prev_ji + acc[t][r];
            }
          }
    }
    __syncthreads();
  }
  float* out = part + (long long)blockIdx.x * (NP + 1) * NP;
  for (int e = threadIdx.x; e < NP * NP; e += 256) out[e] = red[e];
}

// split-K reductions fill whole rounds of resident blocks (plan_rounds):
// MI355X has 256 CUs; blocks per CU follow from each config's LDS image
constexpr int kCUs = 256;

static bool band_on(bool with_stats) {
  return with_stats && g_gemm_mode == ACMI_GEMM_X3 && g_conv_stats_mode == ACMI_CONV_STATS_BAND;
}

struct WgradPlan {
  int I, J, kp, cout_pad, nc, ch;
  bool slabs;  // symred_kernel (slab groups) instead of 128x128 live tiles
  bool six;    // bf16x3 six-slab groups (symred6_kernel)
  bool six_greedy = false;  // ... with the greedy plan for any K (fc4)
  SymPlan sp;
  SymPlan6 sp6;
  long long floats;
};

static WgradPlan wgrad_plan(int K, int cout, bool with_stats, long long rows, bool u8 = false,
                            int mode = g_gemm_mode) {
  WgradPlan p;
  p.cout_pad = roundup4(cout);
  p.kp = with_stats ? K : 0;
  p.I = K;
  // no homogeneous column: the A factor's last column (sum of P) is the
  // column-sum row's P part, by symmetry
  p.J = p.kp + p.cout_pad;
  p.slabs = with_stats && sym_plan(K, p.cout_pad, &p.sp);  // (f32 patch sources only)
  p.six = p.slabs && mode == ACMI_GEMM_X3 && sym_plan6(K, p.cout_pad, &p.sp6);
  // fc4 (K = 1568, no four-slab plan): greedy six-slab groups instead of 128x128 tiles
  p.six_greedy = !p.slabs && !u8 && with_stats && mode == ACMI_GEMM_X3 && K % 4 == 0 &&
                 sym_plan6_greedy(K, p.cout_pad, &p.sp6);
  if (p.six_greedy) p.six = true;
  if (u8)  // conv1 weight gradient: conv1_wgrad_u8/x3_kernel, one 256x32 block per chunk
    conv1_wgrad_u8_plan(rows, &p.nc, &p.ch, mode);
  else if (p.six_greedy)  // many groups: one round of blocks, few chunks (partials stay small)
    plan_rounds(rows, p.sp6.ngroups, kCUs, &p.nc, &p.ch, 2048);
  else if (p.six)  // one 512-thread block per CU (2 x 64 accumulators per wave)
    plan_rounds(rows, p.sp6.ngroups, kCUs, &p.nc, &p.ch);
  else if (p.slabs)  // f32 slab groups (in x3 mode every slab plan that runs, K = 512 / 576, is a six-slab one)
    plan_rounds(rows, p.sp.ngroups, kCUs * std::min(8, 160 * 1024 / symred_lds_bytes<16>()), &p.nc,
                &p.ch);
  else if (with_stats)
    plan_rounds(rows, live_tiles<128, 128>(p.I, p.J, K),
                kCUs * gemm_blocks_per_cu<128, 128, 16, false, false>(), &p.nc, &p.ch);
  else
    plan_rounds(rows, live_tiles<128, 32>(p.I, p.J, 0),
                kCUs * gemm_blocks_per_cu<128, 32, 32, false, false>(), &p.nc, &p.ch);
  p.floats = (long long)p.nc * (p.I + 1) * p.J;
  return p;
}

struct GcovPlan {
  int np, nc, ch;
  long long floats;
};

// narrow Gram: chunks of >= 512 rows, at most 2048 blocks (8 per CU)
static void gram_plan(long long rows, int* nc, long long* chunk) {
  long long n = std::min<long long>(2048, std::max<long long>(1, rows / 512));
  long long ch = (rows + n - 1) / n;
  ch = (ch + 63) / 64 * 64;
  *chunk = ch;
  *nc = (int)((rows + ch - 1) / ch);
}

static GcovPlan gcov_plan(int n, long long rows) {
  GcovPlan p;
  p.np = roundup4(n);
  plan_rounds(rows, live_tiles<64, 64>(p.np, p.np, p.np),
              kCUs * gemm_blocks_per_cu<64, 64, 32, false, false>(), &p.nc, &p.ch);
  p.floats = (long long)p.nc * (p.np + 1) * p.np;
  return p;
}

// the partial floats gcov_layer will need (its two paths' plans)
static long long gcov_need(int n, long long rows) {
  if (n <= 32) {
    int nc;
    long long ch;
    gram_plan(rows, &nc, &ch);
    return (long long)nc * 33 * 32;
  }
  return gcov_plan(n, rows).floats;
}

// The partial region of one entry point, handed out in ranges: every layer (Gram)
// of a finalize set (Set: WgradSet / CovSet) writes its split-K partials into a
// range of its own and adds its finalize tasks; flush() launches the set.
static std::atomic<int> g_ws_flushes{0};  // acmi_debug_ws_flushes
template <class Set>
struct PartRanges {
  float* base;
  long long cap;
  hipStream_t s;
  Set set{};
  long long off = 0, need = 0;
  // launch the finalizes added so far; the ranges start over
  void flush() {
    if (set.n) set.launch(s);
    set = Set();
    off = 0;
  }
  // the range (room() floats) for a plan of need_ floats: after the others, or --
  // when the plan does not fit there -- a new first range after the set so far is
  // finalized (at workspaces near the minimum; acmi_debug_ws_flushes counts it)
  float* begin(long long need_) {
    need = need_;
    if (off > 0 && need > cap - off) g_ws_flushes.fetch_add(1), flush();
    else if (set.n + 2 > Set::kTasks) flush();
    return base + off;
  }
  long long room() const { return cap - off; }
  template <class... Args>
  void add(const Args&... task) { set.add(task...); }
  // the layer reports what it wrote, which must be that plan
  int end(long long used) {
    ACMI_REQUIRE(used == need, ACMI_ERR_ARG, "internal: a %s used %lld partial floats against its planned %lld",
                 Set::kWhat, used, need);
    off += (used + 3) / 4 * 4;
    return ACMI_OK;
  }
};

// Launch [P;1]^T [P | dY] (with_stats; the 1 row is the column-sum row) or
// [P;1]^T [dY] over rows into the next range of ra, and add its finalize (one
// task, or two) to ra's set.
template <class Src>
static int wgrad_layer(const Src& src, int K, long long rows, const float* dy,
                       int ldy, int cout, bool with_stats, PartRanges<WgradSet>& ra,
                       float* gradA, int nsplit, float* gradB, float* astat, int site = 0,
                       float wscale = 1.f, const unsigned* pmax = nullptr, const unsigned* ymax = nullptr) {
  constexpr bool kU8 = !std::is_same<typename Src::elem_t, float>::value;
  const int mode = g_gemm_mode;
  const WgradPlan pl = wgrad_plan(K, cout, with_stats, rows, kU8, mode);
  const int I = pl.I, J = pl.J, kp = pl.kp, nc = pl.nc, ch = pl.ch;
  hipStream_t s = ra.s;
  float* part = ra.begin(pl.floats);
  RowsAsI<Src> opA{src};
  CatRowsI<Src> opB{src, kp, dy, ldy, cout, pl.cout_pad, (int)rows};
  if constexpr (!std::is_same<typename Src::elem_t, float>::value)
    ACMI_REQUIRE(!with_stats, ACMI_ERR_ARG, "u8 patch sources take the integer A-factor path");
  ACMI_REQUIRE(pl.floats <= ra.room(), ACMI_ERR_WS, "wgrad workspace too small (%lld > %lld)",
               pl.floats, ra.room());
  EpiPartial epi{part, I, J};
  prof_begin(site, s);
  if constexpr (std::is_same<typename Src::elem_t, float>::value) {
    if (pl.six)  // six-slab groups, bf16x3 split operands (f16x2 with published bounds)
      launch_symred6(opB, epi, pl.sp6, I, J, (int)rows, nc, ch, s, pmax, ymax, kp);
    else if (pl.slabs)  // slab groups over the upper triangle of P^T P and the dY columns
      launch_symred<16>(opB, epi, pl.sp, I, J, (int)rows, nc, ch, s);
    else if (with_stats)  // 128x128 live tiles (fc4: K not a multiple of 64)
      launch_mm<128, 128, 16, 2, 2, true, true, 16>(opA, opB, epi, I, J, (int)rows, nc, ch, s, K);
    else
      launch_mm<128, 32, 32, 1, 1, true, true, 32>(opA, opB, epi, I, J, (int)rows, nc, ch, s);
  } else {  // u8 patches (conv1): weight gradient only, bytes in LDS
    ACMI_REQUIRE(K == 256 && cout == 32 && ldy == 32, ACMI_ERR_ARG, "conv1 weight gradient shape");
    launch_conv1_wgrad_u8(src, dy, (int)rows, nc, ch, epi, s);
  }
  prof_end(site, s);
  // few chunks (fc4): the A factor on upper-triangle tiles mirrored through LDS;
  // many (the heads' 80): one output per 8 threads, chunk groups in parallel
  const bool tiles = astat && nc <= kFinGroups;
  WgradDesc d{part, nc, I, J, kp, cout, gradA, nsplit, gradB, tiles ? nullptr : astat, (int)rows, wscale};
  ra.add(d, 0);
  if (tiles) {
    d.astat = astat;
    ra.add(d, 1);
  }
  ACMI_LAUNCH_CHECK("wgrad_layer");
  return ra.end(pl.floats);
}

// G = g^T g / rows for g [rows][ld] (first n columns), via split-K into the next
// range of ra, its finalize added to ra's set; gmax: the published max |g| (bit
// pattern) -- the wide Grams then run on f16x2 split operands (three MFMAs per
// product instead of bf16x3's six)
static int gcov_layer(const float* g, int ld, int n, long long rows, int sub,
                      PartRanges<CovSet>& ra, float* out, float* out_v = nullptr, int v_index = -1,
                      const unsigned* gmax = nullptr) {
  hipStream_t s = ra.s;
  float* part = ra.begin(gcov_need(n, rows));
  int np, nc;
  if (n <= 32) {  // narrow: streaming Gram kernel (f32 MFMA; 64 wide runs faster on the split-K
                  // bf16x3 GEMM below: conv2's G factor 82 + 25 -> 59 + 16 us)
    np = 32;
    long long ch;
    gram_plan(rows, &nc, &ch);
    ACMI_REQUIRE((long long)nc * (np + 1) * np <= ra.room(), ACMI_ERR_WS, "gcov workspace too small");
    hipLaunchKernelGGL(gram_small_kernel<32>, dim3(nc), dim3(256), 0, s, g, ld, n, rows, ch, part);
  } else {
    const GcovPlan pl = gcov_plan(n, rows);
    np = pl.np;
    nc = pl.nc;
    DenseRows src{g, ld, (int)rows, np};
    RowsAsI<DenseRows> op{src};
    ACMI_REQUIRE(pl.floats <= ra.room(), ACMI_ERR_WS, "gcov workspace too small");
    EpiPartial epi{part, np, np};
    if (gmax && g_gemm_mode == ACMI_GEMM_X3)
      launch_gemm3_f16_splitk<64, 64, 16, 1, 1>(op, op, epi, np, np, (int)rows, nc, (int)pl.ch, gmax, gmax, s, np);
    else
      launch_mm<64, 64, 32, 1, 1, true, false, 16>(op, op, epi, np, np, (int)rows, nc, pl.ch, s, np);
  }
  // few chunks: a thread per element (wide factors on LDS-transposed tiles); many: a wave
  ra.add(part, nc, np, sub, out, (int)rows, nc <= 64 ? (sub >= 64 ? 3 : 0) : 1);
  if (out_v) ra.add(part, nc, np, 1, out_v, (int)rows, 2, v_index);
  ACMI_LAUNCH_CHECK("gcov_layer");
  return ra.end((long long)nc * (np + 1) * np);
}

// the split-K partial region's minimum: the largest partial over all layers (with
// stats, both gemm modes, both Gram paths, the band reductions)
static long long bwd_partial_floats(int B, int A, int C3) {
  long long m = 0;
  const long long rowsL[5] = {400LL * B, 81LL * B, 49LL * B, B, B};
  const int Ks[5] = {256, 512, 576, 49 * C3, 512};
  const int co[5] = {32, 64, C3, 512, A + 1};
  for (int l = 0; l < 5; ++l) {
    for (int mode : {ACMI_GEMM_F32, ACMI_GEMM_X3})
      m = std::max(m, wgrad_plan(Ks[l], co[l], true, rowsL[l], false, mode).floats);
    for (int mode : {ACMI_GEMM_F32, ACMI_GEMM_X3})
      m = std::max(m, wgrad_plan(Ks[l], co[l], false, rowsL[l], l == 0, mode).floats);
    // G factors of the same layer's output
    if (co[l] <= 64) {  // (the 64-wide streaming Gram no longer runs; its term keeps acmi_backward_ws_floats)
      int nc;
      long long ch;
      gram_plan(rowsL[l], &nc, &ch);
      const long long np = co[l] <= 32 ? 32 : 64;
      m = std::max(m, nc * (np + 1) * np);
    }
    m = std::max(m, gcov_plan(co[l], rowsL[l]).floats);
  }
  // band reductions of conv2 / conv3 (rows = images)
  m = std::max(m, band_ws_floats(band_host_plan(20, 20, 32, 4, 4, 2, 64), B));
  m = std::max(m, band_ws_floats(band_host_plan(9, 9, 64, 3, 3, 1, C3), B));
  return (m + 63) / 64 * 64;
}

static long long afactor_ws_floats(int B) { return conv1_afactor_ws_ints(400LL * B); }

// Workspace of acmi_backward / acmi_kfac_output_stats (one size for both):
//   backward:      [scratch kBandScratch | conv1 A-factor ints | partials ...]
//   output stats:  [scratch kBandScratch | sampled head gradients B x ldg | partials ...]
// (prefixes rounded to 256 B); the partial region is the rest of the caller's
// buffer, at least bwd_partial_floats.  backward.hpp's BwdWs / StatsWs are the
// views of the two layouts, by these prefix sizes.
static long long head_grad_ldg(int A) { return roundup4(A + 1) < 8 ? 8 : roundup4(A + 1); }
static long long bwd_prefix_floats(int B) { return kBandScratch + (afactor_ws_floats(B) + 63) / 64 * 64; }
static long long stats_prefix_floats(int B, int A) { return kBandScratch + ((long long)B * head_grad_ldg(A) + 63) / 64 * 64; }

}  // namespace acmi
