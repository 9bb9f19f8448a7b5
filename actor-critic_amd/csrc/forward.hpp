// The forward (net.hip's acmi_forward / acmi_forward_strided / acmi_rollout_step[_games]):
// the per-layer epilogue and mask kernel, the heads kernel and the rollout tails
// (alone, fused with the next step's tower, split over kSplitParts workgroups),
// fc4's split plan with the table of split counts that have a compiled heads /
// tail kernel, the launcher that picks one of them, forward_impl and
// forward_dispatch.
//
// Part of net.hip's translation unit: it is included after the mode globals
// (g_gemm_mode, g_forward_mode), prof_begin / prof_end, Layout and masks_ok that it uses.
// dispatch_c3, by which every entry point of the translation unit picks its C3
// instantiation, is defined here.
#pragma once

#include <algorithm>
#include <iterator>
#include <type_traits>
#include <utility>

#include "conv1u8.hpp"
#include "convfwd3.hpp"
#include "fc4roll.hpp"
#include "games.hpp"
#include "gemm.hpp"
#include "gemm3.hpp"
#include "prepview.hpp"
#include "stepper.hpp"
#include "tower.hpp"
#include "towersplit.hpp"

namespace acmi {

// ReLU' bit masks from the f32 activations, for the per-layer forward (the tower
// writes them itself): word k of image b (wpi words per image, one per 32
// channels) = bits (act > 0) of its 32 floats; images st apart in both buffers
__global__ void act_mask_kernel(const float* act, int B, int wpi, long long st, uint32_t* mask) {
  const long long w = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= (long long)B * wpi) return;
  const long long b = w / wpi, k = w - b * wpi;
  const float4* src = reinterpret_cast<const float4*>(act + (b * st * wpi + k) * 32);
  uint32_t bits = 0;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const float4 v = src[q];
    bits |= (uint32_t)(v.x > 0.f) << (4 * q) | (uint32_t)(v.y > 0.f) << (4 * q + 1) |
            (uint32_t)(v.z > 0.f) << (4 * q + 2) | (uint32_t)(v.w > 0.f) << (4 * q + 3);
  }
  mask[b * st * wpi + k] = bits;
}

// conv/fc epilogue with an image remap so the rollout can write step t of an
// env-major [N][T][rows] activation buffer in place.
struct EpiAct {
  float* out;
  const float* bias;
  int cols;         // output channels (row length)
  int L;            // output rows per image
  long long img_stride;  // floats between consecutive images in `out`
  float scale = 1.f;     // conv1: 1/255 (its A operand is the raw u8 pixels)
  __device__ __forceinline__ float aux(int, int j) const { return bias[j]; }
  __device__ __forceinline__ void store(int i, int j, float v, float b) const {
    const uint32_t img = (uint32_t)i / (uint32_t)L;
    const uint32_t p = (uint32_t)i - img * (uint32_t)L;
    out[(long long)img * img_stride + (long long)p * cols + j] = fmaxf(__builtin_fmaf(v, scale, b), 0.f);
  }
};


// Fused rollout tail (acmi_rollout_step): one workgroup per env b -- a4 from
// fc4's split-K slabs (or as stored), the A+1 heads, the categorical draw and
// the env step, with the arithmetic of heads_kernel / sample_kernel /
// env_step_kernel (same per-element orders), so the fused step is bit-identical
// to the three launches it replaces.
// legal (acmi_rollout_step_masked; nullptr: unmasked): env b's legal-action word
// at legal[b] -- one more load on the thread that draws, nothing else changes
struct TailArgs {
  acmi_rollout_io_t io;
  const uint8_t* obs;
  long long img_stride;
  const uint32_t* legal = nullptr;
};
constexpr int kMaxHeads = 32;

// The env a tail steps is a policy (rollout_tail_body's Env): its kernel arguments
// (Args: io, obs, img_stride, legal as in TailArgs, plus its own), the pre-step state it
// loads ahead of the heads (Pre, with the stack words in old[]), the whole-block step,
// the split form's part step and its pending entry (Pend), and the host's half of the
// pending contract (pend_area, commit).  SynthEnv is the synthetic stepper of
// stepper.hpp (acmi_rollout_step); GameEnv the device games of games.hpp
// (acmi_rollout_step_games).
struct SynthEnv {
  using Args = TailArgs;
  using Pre = EnvPre;
  using Pend = PendState;
  using Commit = Fc4Commit;
  static __device__ __forceinline__ void prefetch(const Args& ta, int row, Pre& pre) {
    env_prefetch(ta.io.state, row, ta.obs + (long long)row * ta.img_stride, pre);
  }
  static __device__ __forceinline__ void step_block(const Args& ta, int row, uint32_t action, const Pre& pre,
                                                    uint4* mirror) {
    const acmi_rollout_io_t& io = ta.io;
    env_step_block_pre(io.state, row, (uint32_t)(io.env_offset + row), io.env_seed, action, pre,
                       io.obs_out + (long long)row * io.out_stride, io.rewards, io.terminals,
                       io.episode_rewards, io.ld, mirror);
  }
  static __device__ __forceinline__ void step_part(const Args& ta, int row, uint32_t action, int spart,
                                                   uint4* mirror, bool writer, Pend* pend) {
    const acmi_rollout_io_t& io = ta.io;
    env_step_part(io.state, row, (uint32_t)(io.env_offset + row), io.env_seed, action,
                  ta.obs + (long long)row * ta.img_stride, split_word_lo(spart), split_word_hi(spart),
                  split_own_lo(spart), split_own_hi(spart), io.obs_out + (long long)row * io.out_stride,
                  io.obs_copy ? io.obs_copy + (long long)row * io.out_stride : nullptr, mirror, writer, io.rewards,
                  io.terminals, io.episode_rewards, io.ld, pend);
  }
  // the pending states sit after fc4's slabs in the forward workspace
  // (acmi_forward_ws_floats reserves them at B <= kSplitMaxB)
  static Pend* pend_area(const Args&, const acmi_acts_t* a, int nz, int B) {
    return a->ws_floats >= (long long)nz * (B + 1) * 512 + (long long)B * (sizeof(PendState) / 4)
               ? reinterpret_cast<PendState*>(a->ws + (long long)nz * (B + 1) * 512)
               : nullptr;
  }
  static Commit commit(const Args* ta, Pend* pend, int B) {
    return Commit{pend, ta ? ta->io.state : acmi_env_state_t{}, pend ? B : 0};
  }
};

// acmi_rollout_step_games: io.state is not read; the game is read per env from
// game.games where that is given -- a run-time test of the pointer, one kernel per
// form ("Fused step").  pend: the caller's pending area (host side only).
struct GameTailArgs {
  acmi_rollout_io_t io;
  const uint8_t* obs;
  long long img_stride;
  const uint32_t* legal;
  GameCall game;
  uint8_t* truncated;
  GamePend* pend;
};
struct GameFc4Commit {
  GamePend* pend;
  acmi_game_state_t st;
  int B;
  __device__ __forceinline__ void run() const { game_commit_pending(st, pend, B); }
};
struct GameEnv {
  using Args = GameTailArgs;
  using Pre = GamePre;
  using Pend = GamePend;
  using Commit = GameFc4Commit;
  static __device__ __forceinline__ GameOut outs(const Args& ta) {
    return GameOut{ta.io.rewards, ta.io.terminals, ta.truncated, ta.io.episode_rewards, ta.io.ld};
  }
  static __device__ __forceinline__ void prefetch(const Args& ta, int row, Pre& pre) {
    game_prefetch<true>(ta.game, row, ta.obs + (long long)row * ta.img_stride, pre);
  }
  static __device__ __forceinline__ void step_block(const Args& ta, int row, uint32_t action, const Pre& pre,
                                                    uint4* mirror) {
    game_step_block_pre<true>(ta.game, row, (uint32_t)(ta.io.env_offset + row), action, pre,
                              ta.io.obs_out + (long long)row * ta.io.out_stride, outs(ta), mirror);
  }
  static __device__ __forceinline__ void step_part(const Args& ta, int row, uint32_t action, int spart,
                                                   uint4* mirror, bool writer, Pend* pend) {
    const acmi_rollout_io_t& io = ta.io;
    game_step_part(ta.game, row, (uint32_t)(io.env_offset + row), action, ta.obs + (long long)row * ta.img_stride,
                   split_word_lo(spart), split_word_hi(spart), split_own_lo(spart), split_own_hi(spart),
                   io.obs_out + (long long)row * io.out_stride,
                   io.obs_copy ? io.obs_copy + (long long)row * io.out_stride : nullptr, mirror, writer, outs(ta),
                   pend);
  }
  static Pend* pend_area(const Args& ta, const acmi_acts_t*, int, int) { return ta.pend; }
  static Commit commit(const Args* ta, Pend* pend, int B) {
    return Commit{pend, ta ? ta->game.st : acmi_game_state_t{}, pend ? B : 0};
  }
};
static_assert(kGameWords == kEnvWords && kGameFrameWords == FRAME_WORDS && kGameThreads == kEnvThreads,
              "the tails file the stacks of either env with one loop");
// sx [512], sl [kMaxHeads], s_action: the block's scratch in LDS; mirror
// (nullable): the new stack also goes there (the fused next-step tower's image)
// SPLIT (towersplit.hpp): one of kSplitParts workgroups of env `row` (part `spart`):
// the heads and the draw are computed by every part (the same arithmetic, so the
// same action), only part 0 stores them; the env step builds the stack words the
// part's tower needs (env_step_part) and the post-step state goes to pend.
template <int NZ, bool SPLIT = false, class Env = SynthEnv>
__device__ __forceinline__ void rollout_tail_body(
    const float* part, int nz, const float* b4, float* a4, long long a4_stride, int B,
    const float* wpi, const float* bpi, const float* wv, const float* bv, int A, float* logits,
    long long l_stride, float* value, long long v_stride, const typename Env::Args& ta, float* sx, float* sl,
    int& s_action, uint4* mirror, int row = -1, int spart = 0, typename Env::Pend* pend = nullptr) {
  if (row < 0) row = blockIdx.x;
  const bool writer = spart == 0;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  typename Env::Pre pre;  // the env's state and current stack: in flight during the heads
  if constexpr (!SPLIT) Env::prefetch(ta, row, pre);
  if (!SPLIT && ta.io.obs_copy) {  // the stacks this step read, filed where the batch keeps them
    uint4* cp = reinterpret_cast<uint4*>(ta.io.obs_copy + (long long)row * ta.io.out_stride);
#pragma unroll
    for (int i = 0; i < kEnvWords; ++i) {
      const int g = threadIdx.x + kEnvThreads * i;
      if (g < FRAME_WORDS) cp[g] = pre.old[i];
    }
  }
  // head a's weight for a4 element lane + 64 e (a == A: the value head); the
  // wave's first two heads are loaded now, beside the slab and stack loads
  auto head_w = [&](int a, int e) {
    const int ai = a < A ? a : 0;
    return a < A ? wpi[(lane + 64 * e) * A + ai] : wv[lane + 64 * e];
  };
  float hw[2][8];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int e = 0; e < 8; ++e) hw[h][e] = head_w(min(wave + 4 * h, A), e);  // (unused past A)
  float* x = a4 + (long long)row * a4_stride;
  if (NZ > 0) {
    // both columns' NZ slab loads issued before the (fixed-order) sums
    const long long zs = (long long)(B + 1) * 512;
    float pv[2][NZ > 0 ? NZ : 1];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int z = 0; z < NZ; ++z) pv[h][z] = part[z * zs + (long long)row * 512 + threadIdx.x + 256 * h];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int j = threadIdx.x + 256 * h;
      float acc = 0.f;
#pragma unroll
      for (int z = 0; z < NZ; ++z) acc += pv[h][z];
      const float v = fmaxf(acc + b4[j], 0.f);
      if (writer) x[j] = v;
      sx[j] = v;
    }
  } else {
    for (int j = threadIdx.x; j < 512; j += 256) sx[j] = x[j];
  }
  __syncthreads();
  float xv[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) xv[e] = sx[lane + 64 * e];
  auto head = [&](int a, const float (&w)[8]) {  // head a (a == A: the value head)
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) s += xv[e] * w[e];
    s = wave_sum(s);
    if (lane == 0) sl[a] = s + (a < A ? bpi[a] : bv[0]);
  };
  if (wave <= A) head(wave, hw[0]);
  if (wave + 4 <= A) head(wave + 4, hw[1]);
  for (int a = wave + 8; a <= A; a += 4) {
    float w[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) w[e] = head_w(a, e);
    head(a, w);
  }
  __syncthreads();
  const acmi_rollout_io_t& io = ta.io;
  if (threadIdx.x == 0) {
    if (writer) {
      for (int a = 0; a < A; ++a) logits[(long long)row * l_stride + a] = sl[a];
      if (value) value[(long long)row * v_stride] = sl[A];
    }
    const uint32_t ctr = io.counter + (io.counter_dev ? *io.counter_dev : 0u);
    bool bad;
    const uint32_t grow = (uint32_t)(row + io.row_offset);
    const int y = ta.legal ? sample_row<true>(sl, A, io.seed, io.stream_id, ctr, grow, nullptr, 0, &bad, ta.legal[row])
                           : sample_row<false>(sl, A, io.seed, io.stream_id, ctr, grow, nullptr, 0, &bad);
    if (writer) {
      if (bad) atomicAdd(io.bad_rows, 1);
      io.actions[(long long)row * io.ld] = y;
    }
    s_action = y;
  }
  __syncthreads();
  if constexpr (SPLIT) Env::step_part(ta, row, (uint32_t)s_action, spart, mirror, writer, pend);
  else Env::step_block(ta, row, (uint32_t)s_action, pre, mirror);
}

template <int NZ, class Env = SynthEnv>
__global__ __launch_bounds__(256) void rollout_tail_kernel(
    const float* part, int nz, const float* b4, float* a4, long long a4_stride, int B,
    const float* wpi, const float* bpi, const float* wv, const float* bv, int A, float* logits,
    long long l_stride, float* value, long long v_stride, typename Env::Args ta) {
  __shared__ float sx[512];
  __shared__ float sl[kMaxHeads];
  __shared__ int s_action;
  rollout_tail_body<NZ, false, Env>(part, nz, b4, a4, a4_stride, B, wpi, bpi, wv, bv, A, logits, l_stride, value,
                                    v_stride, ta, sx, sl, s_action, nullptr);
}

// The rollout tail of step t fused with the conv tower of step t + 1 (the
// acmi_rollout_io_t next_acts contract): the env step leaves the new stack in
// the tower's LDS image as well as in obs_out, the tower then runs on it --
// one launch and one image round trip fewer per step, the same arithmetic.
// The tail's scratch sits in the tower's a1 region (unused until conv1's
// epilogue).  Two blocks per CU, like the tower.
struct NextTower {
  const float *b1, *b2, *b3;
  float *a1, *a2, *a3;
  long long st;
  const char* prep;
  uint32_t *m1, *m2, *m3;
};
template <int NZ, int C3, bool H16, class Env = SynthEnv>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void rollout_tail_tower_kernel(
    const float* part, int nz, const float* b4, float* a4, long long a4_stride, int B,
    const float* wpi, const float* bpi, const float* wv, const float* bv, int A, float* logits,
    long long l_stride, float* value, long long v_stride, typename Env::Args ta, NextTower nt) {
  __shared__ __attribute__((aligned(16))) char lds[kTowLds + kTowScr];
  float* sx = reinterpret_cast<float*>(lds + kTowObs);
  int* s_action = reinterpret_cast<int*>(sx + 512 + kMaxHeads);
  rollout_tail_body<NZ, false, Env>(part, nz, b4, a4, a4_stride, B, wpi, bpi, wv, bv, A, logits, l_stride, value,
                                    v_stride, ta, sx, sx + 512, *s_action, reinterpret_cast<uint4*>(lds));
  __syncthreads();  // the image in LDS; the tail's scratch free again
  tower_body<C3, H16, true>(nullptr, 0, nt.b1, nt.b2, nt.b3, nt.a1, nt.a2, nt.a3, nt.st, nt.prep, nt.m1, nt.m2,
                            nt.m3, lds, blockIdx.x);
}

// The split rollout step (small batches, towersplit.hpp): kSplitParts workgroups
// per env -- the tail (redundant heads / draw, the env step's words each part's
// tower needs, the post-step state into pend) and then part j of the next
// step's conv tower.  The pending states are committed by the next step's fc4
// launch (fc4_roll_kernel: env_commit_pending), the first launch after this one.
template <int NZ, int C3, bool H16, class Env = SynthEnv>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void rollout_tail_split_kernel(
    const float* part, int nz, const float* b4, float* a4, long long a4_stride, int B,
    const float* wpi, const float* bpi, const float* wv, const float* bv, int A, float* logits,
    long long l_stride, float* value, long long v_stride, typename Env::Args ta, NextTower nt,
    typename Env::Pend* pend) {
  __shared__ __attribute__((aligned(16))) char lds[kSpLds];
  const int n = blockIdx.x / kSplitParts, j = blockIdx.x - n * kSplitParts;
  float* sx = reinterpret_cast<float*>(lds + kSpImg);  // the tail's scratch in the a1 image
  int* s_action = reinterpret_cast<int*>(sx + 512 + kMaxHeads);
  rollout_tail_body<NZ, true, Env>(part, nz, b4, a4, a4_stride, B, wpi, bpi, wv, bv, A, logits, l_stride, value,
                                   v_stride, ta, sx, sx + 512, *s_action, reinterpret_cast<uint4*>(lds), n, j, pend);
  __syncthreads();  // the image rows in LDS; the tail's scratch free again
  tower_part_body<C3, H16>(j, nt.b1, nt.b2, nt.b3, nt.a1, nt.a2, nt.a3, nt.st, nt.prep, nt.m1, nt.m2, nt.m3, lds, n);
}
// the split tower alone (small batches without a fused tail: step 0, the bootstrap
// forward): part j loads the input rows 8j .. 8j+35 of image n
template <int C3, bool H16>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void tower_split_kernel(
    const uint8_t* obs, long long img_stride, NextTower nt) {
  __shared__ __attribute__((aligned(16))) char lds[kSpLds];
  const int n = blockIdx.x / kSplitParts, j = blockIdx.x - n * kSplitParts;
  const uint4* src = reinterpret_cast<const uint4*>(obs + n * img_stride);
  uint4* dst = reinterpret_cast<uint4*>(lds);
  const int g0 = split_word_lo(j), g1 = split_word_hi(j);
  constexpr int NW = (36 * 21 + 255) / 256;
  uint4 v[NW];
#pragma unroll
  for (int i = 0; i < NW; ++i) {
    const int g = g0 + (int)threadIdx.x + 256 * i;
    v[i] = src[g < g1 ? g : g0];
  }
#pragma unroll
  for (int i = 0; i < NW; ++i) {
    const int g = g0 + (int)threadIdx.x + 256 * i;
    if (g < g1) dst[g] = v[i];
  }
  __syncthreads();
  tower_part_body<C3, H16>(j, nt.b1, nt.b2, nt.b3, nt.a1, nt.a2, nt.a3, nt.st, nt.prep, nt.m1, nt.m2, nt.m3, lds, n);
}

// policy/value heads, one wave per row: the 512-long dot products of a4 with
// the A+1 head columns, lane-strided partial sums + a butterfly (fixed order).
// With part != nullptr the row of a4 is first finalised from fc4's split-K
// partial slabs [nz][B+1][512] (relu(sum_z + b4), fixed z order) and stored.
template <int NZ>
__global__ __launch_bounds__(256) void heads_kernel(const float* part, int nz, const float* b4,
                                                    float* a4, long long a4_stride, int B,
                                                    const float* wpi, const float* bpi,
                                                    const float* wv, const float* bv, int A,
                                                    float* logits, long long l_stride,
                                                    float* value, long long v_stride) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= B) return;
  float* x = a4 + (long long)row * a4_stride;
  float xv[8];
  if (NZ > 0) {
    // all NZ x 8 slab loads are issued before the (fixed-order) sums
    const long long zs = (long long)(B + 1) * 512;
    float v[NZ > 0 ? NZ : 1][8];
#pragma unroll
    for (int z = 0; z < NZ; ++z)
#pragma unroll
      for (int e = 0; e < 8; ++e) v[z][e] = part[z * zs + (long long)row * 512 + lane + 64 * e];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int j = lane + 64 * e;
      float acc = 0.f;
#pragma unroll
      for (int z = 0; z < NZ; ++z) acc += v[z][e];
      xv[e] = fmaxf(acc + b4[j], 0.f);
      x[j] = xv[e];
    }
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) xv[e] = x[lane + 64 * e];
  }
  for (int a = 0; a < A; ++a) {
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) s += xv[e] * wpi[(lane + 64 * e) * A + a];
    s = wave_sum(s);
    if (lane == 0) logits[(long long)row * l_stride + a] = s + bpi[a];
  }
  if (value) {
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) s += xv[e] * wv[lane + 64 * e];
    s = wave_sum(s);
    if (lane == 0) value[(long long)row * v_stride] = s + bv[0];
  }
}

// split factor for fc4 at small batch (64 x 128 tiles over 512 columns; 4 / 6 /
// 12 / 16 chunks measured no better than 8)
// (ktile: the split GEMM's K-tile, a chunk is a multiple of it)
static void fc4_plan(int B, int K, int ktile, int* nz, int* chunk) {
  // the split cap at batches <= 128 is 16: the chain of k-steps per chunk, not
  // the slab traffic, sets fc4's time there (14 / 16 measured best)
  const int maxsp = B <= 128 ? 16 : 8;
  const int blocks = cdiv(B, 64) * 4;
  int sp = blocks >= 256 ? 1 : std::min(maxsp, cdiv(256 * maxsp / 8, blocks));
  int ch = (cdiv(K, sp) + ktile - 1) / ktile * ktile;
  *chunk = ch;
  *nz = cdiv(K, ch);
}
// the plan in the calling thread's gemm mode
static void fc4_plan(int B, int K, int* nz, int* chunk) {
  fc4_plan(B, K, g_gemm_mode == ACMI_GEMM_X3 ? 16 : 32, nz, chunk);
}

// The split counts with a compiled heads_kernel / rollout_tail_kernel (0: no
// split): every count the plan produces (fc4_counts_ok, run by acmi_selftest_plans).
constexpr int kHeadCounts[] = {0, 2, 3, 4, 5, 6, 7, 8, 13, 14, 16};
// The fused tail + next tower needs the x3 tower (k-tile 16) and is compiled at
// the counts the plan gives there: 8 at the rollout batch (129 .. 576 images) and
// the small-batch count (<= 128 images: K = 1568 / 3136 in chunks of 7 / 13
// k16-steps), the only one with a split form (kSplitMaxB images at the most).
constexpr int small_count(int C3) { return C3 == 32 ? 14 : 16; }
constexpr bool fused_count(int C3, int nz) { return nz == 8 || nz == small_count(C3); }
static_assert(kSplitMaxB <= 128, "the split step runs at the small-batch count");

// f(std::integral_constant<int, NZ>) for the table's NZ == nz; false: not in the table
template <class F, size_t... I>
static __forceinline__ bool with_head_count(int nz, F&& f, std::index_sequence<I...>) {
  return ((nz == kHeadCounts[I] && (f(std::integral_constant<int, kHeadCounts[I]>{}), true)) || ...);
}
template <class F>
static __forceinline__ bool with_head_count(int nz, F&& f) {
  return with_head_count(nz, f, std::make_index_sequence<std::size(kHeadCounts)>{});
}

// the plan against the table and the fused counts, over every batch up to 8192
static bool fc4_counts_ok() {
  for (int C3 : {32, 64})
    for (int ktile : {16, 32})
      for (int B = 1; B <= 8192; ++B) {
        int nz, chunk;
        fc4_plan(B, 49 * C3, ktile, &nz, &chunk);
        if (nz != 1 && !with_head_count(nz, [](auto) {})) return false;
        if (ktile == 16 && B <= 576 && nz != (B <= 128 ? small_count(C3) : 8)) return false;
      }
  return true;
}

// The arguments every heads / tail kernel starts with, by type; launch passes them
// in the kernels' order and appends the family's own (TailArgs, NextTower, PendState*).
struct HeadArgs {
  const float *part, *b4, *wpi, *bpi, *wv, *bv;
  float *a4, *logits, *value;
  long long a4_stride, l_stride, v_stride;
  int nz, B, A;
  template <auto Kernel, class... Extra>
  __forceinline__ void launch(dim3 grid, hipStream_t s, const Extra&... extra) const {
    hipLaunchKernelGGL(Kernel, grid, dim3(256), 0, s, part, nz, b4, a4, a4_stride, B, wpi, bpi, wv, bv, A, logits,
                       l_stride, value, v_stride, extra...);
  }
};

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------
template <int C3, class Env = SynthEnv>
static int forward_impl(const Layout& L, const float* P, const uint8_t* obs,
                        long long img_stride, int B, const acmi_acts_t* a,
                        int want_value, long long act_img_stride,
                        hipStream_t s, const typename Env::Args* tail = nullptr, const void* prep = nullptr,
                        const char* fn = "acmi_forward") {
  // act_img_stride: images between consecutive batch rows in the activation
  // buffers (1 = contiguous; T = rollout step t of an env-major buffer).
  const long long st = act_img_stride;
  // conv1 -> conv2 -> conv3 as one fused kernel per image (tower.hpp, f16x2 on
  // acmi_conv_prepare's fragments) in x3 mode; the per-layer kernels below in f32
  // mode, without prepared weights or for unaligned images
  const bool tower =
      g_gemm_mode == ACMI_GEMM_X3 && prep && (uintptr_t)obs % 16 == 0 && img_stride % 16 == 0;
  ACMI_REQUIRE(tower || g_forward_mode == ACMI_FWD_F32, ACMI_ERR_ARG,
               "%s: the 16-bit forward needs the fused tower: net->conv_prep and 16-byte aligned observations / "
               "image stride",
               fn);
  // step fusion (acmi_rollout_io_t): this step's tower ran in the previous
  // step's tail; the next step's tower runs in this step's tail
  const bool tower_done = tail && tail->io.tower_done;
  const acmi_acts_t* nxt = tail ? tail->io.next_acts : nullptr;
  ACMI_REQUIRE(tower || (!tower_done && !nxt), ACMI_ERR_ARG,
               "rollout step fusion needs the fused tower (x3 gemm mode, conv_prep, 16-byte aligned images)");
  ACMI_REQUIRE(!tail || !tail->io.obs_copy || ((uintptr_t)tail->io.obs_copy % 16 == 0 && tail->io.out_stride % 16 == 0),
               ACMI_ERR_ARG, "acmi_rollout_step: obs_copy must be 16-byte aligned");
  ACMI_REQUIRE(!nxt || (nxt->a1 && nxt->a2 && nxt->a3 && masks_ok(nxt) && tail->io.next_act_stride >= 1 &&
                        (uintptr_t)tail->io.obs_out % 16 == 0 && tail->io.out_stride % 16 == 0),
               ACMI_ERR_ARG, "acmi_rollout_step: bad next_acts / next_act_stride / obs_out alignment");
  // small batches: each image's tower over kSplitParts workgroups (towersplit.hpp)
  auto tower_any = [&](const uint8_t* o, long long ostride, float* a1, float* a2, float* a3, long long ast,
                       uint32_t* m1, uint32_t* m2, uint32_t* m3) {
    const bool h16 = g_forward_mode == ACMI_FWD_BF16;
    if (B <= kSplitMaxB) {
      const NextTower nt{P + L.off[1], P + L.off[3], P + L.off[5], a1, a2, a3, ast,
                         static_cast<const char*>(prep), m1, m2, m3};
      if (h16)
        hipLaunchKernelGGL((tower_split_kernel<C3, true>), dim3(B * kSplitParts), dim3(256), 0, s, o, ostride, nt);
      else
        hipLaunchKernelGGL((tower_split_kernel<C3, false>), dim3(B * kSplitParts), dim3(256), 0, s, o, ostride, nt);
    } else {
      launch_tower<C3>(o, ostride, B, P, L.off, a1, a2, a3, ast, prep, s, h16, m1, m2, m3);
    }
  };
  if (tower) {
    // the three convs fused per image (16-byte image loads)
    if (!tower_done) {
      prof_begin(ACMI_PROF_CONV1_FWD, s);
      tower_any(obs, img_stride, a->a1, a->a2, a->a3, st, a->m1, a->m2, a->m3);
      prof_end(ACMI_PROF_CONV1_FWD, s);
    }
  } else {
  {  // conv1: [B,84,84,4]u8 -> [B,20,20,32]; the u8 patches stay bytes in LDS
    using Src = ConvRows<uint8_t, 84, 84, 4, 8, 8, 4>;
    MatI<true> w{P + L.off[0], 32, 256, 32};
    EpiAct epi{a->a1, P + L.off[1], 32, 400, st * 400 * 32, 1.0f / 255.0f};
    prof_begin(ACMI_PROF_CONV1_FWD, s);
    launch_conv1_fwd_u8<32>(Src{obs, (uint32_t)img_stride, B * 400}, w, epi, B * 400, 256, s);
    prof_end(ACMI_PROF_CONV1_FWD, s);
  }
  {  // conv2: -> [B,9,9,64]
    using Src = ConvRows<float, 20, 20, 32, 4, 4, 2>;
    RowsAsK<Src> opA{Src{a->a1, (uint32_t)(st * 400 * 32), B * 81}};
    MatI<true> opB{P + L.off[2], 64, 512, 64};
    EpiAct epi{a->a2, P + L.off[3], 64, 81, st * 81 * 64};
    if (B <= 2048)
      launch_mm<64, 64, 32, 1, 1, false, false, 32>(opA, opB, epi, B * 81, 64, 512, 1, 0, s);
    else
      launch_mm<128, 64, 32, 2, 1, false, false, 16>(opA, opB, epi, B * 81, 64, 512, 1, 0, s);
  }
  {  // conv3: -> [B,7,7,C3]
    using Src = ConvRows<float, 9, 9, 64, 3, 3, 1>;
    RowsAsK<Src> opA{Src{a->a2, (uint32_t)(st * 81 * 64), B * 49}};
    MatI<true> opB{P + L.off[4], C3, 576, C3};
    EpiAct epi{a->a3, P + L.off[5], C3, 49, st * 49 * C3};
    if (g_gemm_mode == ACMI_GEMM_X3)
      launch_convf_x3<float, 9, 9, 64, 3, 3, 1, C3, 2, 64>(a->a2, st * 81 * 64, B, P + L.off[4], epi, s);
    else if constexpr (C3 == 32)
      // (f32 MFMA: the 128x32 bf16x3 tile needs BK = 32 and fits 2 blocks per CU;
      // measured slower than this at B = 512, 21.1 vs 19.6 us)
      launch_gemm<128, 32, 32, 1, 1, false, false>(opA, opB, epi, B * 49, C3, 576, 1, 0, s);
    else
      launch_mm<128, 64, 32, 2, 1, false, false, 16>(opA, opB, epi, B * 49, C3, 576, 1, 0, s);
  }
  if (a->m1) {  // the ReLU' masks the tower would have written
    hipLaunchKernelGGL(act_mask_kernel, dim3(cdiv((long long)B * 400, 256)), dim3(256), 0, s, a->a1, B, 400, st, a->m1);
    hipLaunchKernelGGL(act_mask_kernel, dim3(cdiv((long long)B * 162, 256)), dim3(256), 0, s, a->a2, B, 162, st, a->m2);
    hipLaunchKernelGGL(act_mask_kernel, dim3(cdiv((long long)B * 49 * C3 / 32, 256)), dim3(256), 0, s, a->a3, B,
                       49 * C3 / 32, st, a->m3);
  }
  }  // per-layer convs
  // fc4: [B,49*C3] -> [B,512]
  const int K4 = 49 * C3;
  // rows are images; with an image stride the dense row stride is st*K4
  RowsAsK<DenseRows> opA4{DenseRows{a->a3, (int)(st * K4), B, K4}};
  MatI<true> opB4{P + L.off[6], 512, K4, 512};
  int nz, chunk;
  fc4_plan(B, K4, &nz, &chunk);
  const bool split = nz > 1 && a->ws && a->ws_floats >= (long long)nz * (B + 1) * 512;
  const PrepView<C3> pv{prep};
  const char* w4p = pv.fc4();
  // the split rollout step's pending env states (Env::pend_area: after fc4's slabs in
  // the forward workspace, or the caller's buffer); only with the rollout fc4 kernel,
  // the one launch that commits them
  const bool fc4_roll = split && g_gemm_mode == ACMI_GEMM_X3 && w4p && fc4_roll_ok(a->a3, st * K4, K4, chunk);
  typename Env::Pend* pend = fc4_roll && tail && B <= kSplitMaxB ? Env::pend_area(*tail, a, nz, B) : nullptr;
  if (split) {
    // small (rollout) batches: split K over chunks; the heads kernel reduces
    // the slabs in fixed order and applies bias + relu
    // every rollout step with a pending area commits the entries flagged there
    // (the previous fused step's; also, at step 0, those a rollout abandoned
    // between fused steps left behind -- the flag is cleared on commit)
    const typename Env::Commit cm = Env::commit(tail, pend, B);
    if (!(fc4_roll &&
          launch_fc4_roll(a->a3, st * K4, B, K4, w4p, nz, chunk, a->ws, pv.hdr(), s, cm))) {
      // (no fused tower without the rollout fc4: no split step, nothing pending)
      EpiPartial epi{a->ws, B, 512};
      launch_mm<64, 128, 32, 1, 2, true, false, 16>(opA4, opB4, epi, B, 512, K4, nz, chunk, s);
    }
  } else {
    EpiAct epi{a->a4, P + L.off[7], 512, 1, st * 512};
    launch_mm<64, 128, 32, 1, 2, false, false, 16>(opA4, opB4, epi, B, 512, K4, 1, 0, s);
  }
  // heads: [B,512] -> logits [B,A], value [B]
  const HeadArgs ha{split ? a->ws : nullptr, P + L.off[7], P + L.off[8], P + L.off[9], P + L.off[10], P + L.off[11],
                    a->a4, a->logits, want_value ? a->value : nullptr, st * 512, st * a->ld_logits, st, nz, B, L.A};
  NextTower ntw{};
  if (nxt) ntw = NextTower{P + L.off[1], P + L.off[3], P + L.off[5], nxt->a1, nxt->a2, nxt->a3,
                          tail->io.next_act_stride, static_cast<const char*>(prep), nxt->m1, nxt->m2, nxt->m3};
  const bool h16 = g_forward_mode == ACMI_FWD_BF16;
  // the fused tail + next tower at the rollout's split-K counts (fused_count); any
  // other (or no) split runs the tail and then the next step's tower as two launches
  // (small batches run the 16-wave tower, which the fused tail does not host)
  const bool fuse_next = nxt && split && fused_count(C3, nz);
  const bool launched = with_head_count(split ? nz : 0, [&](auto count) {
    constexpr int NZ = decltype(count)::value;
    auto fused = [&](auto half) {  // with pending states the split form, at its one count
      constexpr bool H16 = decltype(half)::value;
      if constexpr (NZ == small_count(C3))
        if (pend)
          return ha.launch<rollout_tail_split_kernel<NZ, C3, H16, Env>>(dim3(B * kSplitParts), s, *tail, ntw, pend);
      ha.launch<rollout_tail_tower_kernel<NZ, C3, H16, Env>>(dim3(B), s, *tail, ntw);
    };
    if (!tail) ha.launch<heads_kernel<NZ>>(dim3(cdiv(B, 4)), s);
    else if (!fuse_next) ha.launch<rollout_tail_kernel<NZ, Env>>(dim3(B), s, *tail);
    else if constexpr (fused_count(C3, NZ)) h16 ? fused(std::true_type{}) : fused(std::false_type{});
  });
  ACMI_REQUIRE(launched, ACMI_ERR_ARG, "fc4 split factor %d out of range", nz);
  if (nxt && !fuse_next)  // the next step's tower on the stacks the tail just wrote
    tower_any(tail->io.obs_out, tail->io.out_stride, nxt->a1, nxt->a2, nxt->a3, tail->io.next_act_stride, nxt->m1,
              nxt->m2, nxt->m3);
  ACMI_LAUNCH_CHECK("acmi_forward");
  return ACMI_OK;
}

// The GEMM operand loaders address with 32-bit element offsets (gemm_ops.hpp):
// every buffer a launch reads must span < 2^31 elements.
static bool spans32(long long rows, long long stride, long long per_row) {
  return rows <= 0 || (rows - 1) * stride + per_row < (1LL << 31);
}

// f(std::integral_constant<int, C3>) for a layout's C3 (make_layout: 32 or 64)
template <class F>
static __forceinline__ auto dispatch_c3(int C3, F&& f) {
  return C3 == 32 ? f(std::integral_constant<int, 32>{}) : f(std::integral_constant<int, 64>{});
}

template <class Env = SynthEnv>
static int forward_dispatch(const acmi_net_t* net, const uint8_t* obs, int64_t img_stride,
                            int B, const acmi_acts_t* acts, int want_value,
                            long long act_stride, acmi_stream_t stream,
                            const typename Env::Args* tail = nullptr, const char* fn = "acmi_forward") {
  // fn: the entry point's name, in every message.  Every argument error comes
  // before anything is enqueued (forward_impl's own are ahead of its launches).
  Layout L;
  ACMI_REQUIRE(net && acts && obs && net->params, ACMI_ERR_ARG, "%s: null argument", fn);
  ACMI_REQUIRE(make_layout(net->num_actions, net->conv3_filters, &L), ACMI_ERR_ARG,
               "%s: bad A=%d/C3=%d", fn, net->num_actions, net->conv3_filters);
  ACMI_REQUIRE(B >= 0 && img_stride >= 84 * 84 * 4 && img_stride % 4 == 0, ACMI_ERR_ARG,
               "%s: bad B=%d / img_stride=%lld (>= 28224, a multiple of 4)", fn, B, (long long)img_stride);
  // the per-layer conv1 loads patch pixels as uint32 (ConvRows<uint8_t>::stage)
  ACMI_REQUIRE((uintptr_t)obs % 4 == 0, ACMI_ERR_ARG, "%s: obs must be 4-byte aligned", fn);
  ACMI_REQUIRE(acts->a1 && acts->a2 && acts->a3 && acts->a4 && acts->logits &&
                   acts->ld_logits >= net->num_actions && (!want_value || acts->value),
               ACMI_ERR_ARG, "%s: bad activation buffers", fn);
  ACMI_REQUIRE(masks_ok(acts), ACMI_ERR_ARG, "%s: ReLU masks m1..m3 must be all set or all NULL", fn);
  ACMI_REQUIRE(act_stride >= 1, ACMI_ERR_ARG, "%s: bad activation stride", fn);
  ACMI_REQUIRE(spans32(B, img_stride, 84 * 84 * 4) && spans32(B, act_stride * 400 * 32, 400 * 32),
               ACMI_ERR_ARG, "%s: batch spans >= 2^31 elements (B=%d)", fn, B);
  if (B == 0) return ACMI_OK;
  hipStream_t s = (hipStream_t)stream;
  return dispatch_c3(L.C3, [&](auto c3) {
    return forward_impl<decltype(c3)::value, Env>(L, net->params, obs, img_stride, B, acts, want_value, act_stride, s,
                                                  tail, net->conv_prep, fn);
  });
}

}  // namespace acmi
