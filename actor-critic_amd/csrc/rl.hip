// Rollout-side and loss-side kernels: categorical sampling, n-step targets,
// A2C and PPO losses + head gradients, row gather, first-order optimizers, batched synthetic Atari
// stepper with the reference's frame-stack / auto-reset / episode-info
// semantics.  Contracts and reference citations: include/acmi.h.
#include <math.h>

#include "common.hpp"
#include "stepper.hpp"

namespace acmi {

// ---------------------------------------------------------------------------
// sampling (policies.py:86 Categorical.sample / :87 mode)
// ---------------------------------------------------------------------------
// row_offset: global row index of local row 0 (a batch sampled in pieces draws
// the same uniforms as in one launch)
// ctr_dev (nullable): device counter base added to ctr (graph-replayed rollouts)
// MASKED: legal[m] is row m's legal-action word (stepper.hpp legal_at); the
// unmasked instantiations take legal = nullptr and never read it.
template <bool MASKED>
__global__ void sample_kernel(const float* logits, int ld, int B, int A, uint32_t seed, uint32_t sid, uint32_t ctr,
                              const uint32_t* ctr_dev, uint32_t row_offset, const float* uniforms, int mode,
                              int32_t* actions, int32_t* bad, const uint32_t* legal) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= B) return;
  if (ctr_dev) ctr += *ctr_dev;
  bool bad_row;
  const int y = sample_row<MASKED>(logits + (long long)m * ld, A, seed, sid, ctr, (uint32_t)m + row_offset,
                                   uniforms ? uniforms + m : nullptr, mode, &bad_row,
                                   MASKED ? legal[m] : 0xFFFFFFFFu);
  if (bad_row) atomicAdd(bad, 1);
  actions[m] = y;
}

// A row's log-softmax and entropy over its legal set S (all of 0..A-1 unmasked):
//   mx = max_S z, se = sum_S expf(z - mx), lse = mx + logf(se), H = -sum_S p log p
// in ascending a -- the one statement of the arithmetic every loss kernel shares.
// log pi(a) = z[a] - lse while |mx| < 8: lse < 8 + log 64 there, so its rounding to
// f32 puts at most half an ulp of 16, 1e-6, into a log-probability.  Past that the
// rounding of lse grows with |mx| (5e-4 at logits near 1e4), and the maximum is
// subtracted from the logit BEFORE the log of the sum, (z[a] - mx) - logf(se): the
// difference z - mx is exact or rounded at its own size, and with se >= 1 (the
// maximum's own term) log pi <= 0 and H >= 0 whatever the logits.  (One form for every
// row would do; rows of ordinary logits keep the first so that runs reproduce bit for
// bit.)
struct RowLse {
  float mx, lz, lse;  // the maximum over S, logf(se), their sum
};
template <bool MASKED>
__device__ __forceinline__ RowLse row_lse(const float* z, int A, uint32_t lg) {
  const RowMaxSum ms = row_max_sum<MASKED>(z, A, lg);
  const float lz = logf(ms.se);
  return RowLse{ms.mx, lz, ms.mx + lz};
}
__device__ __forceinline__ float row_logp(float z, const RowLse& l) {
  return fabsf(l.mx) < 8.f ? z - l.lse : (z - l.mx) - l.lz;
}
template <bool MASKED>
__device__ __forceinline__ float row_entropy(const float* z, int A, uint32_t lg, const RowLse& lse) {
  float H = 0.f;
  for (int a = 0; a < A; ++a) {
    if (!legal_at<MASKED>(lg, a)) continue;
    const float lp = row_logp(z[a], lse);
    H -= expf(lp) * lp;
  }
  return H;
}
// MASKED: is `act` a member of S?  (an empty S has no member)
template <bool MASKED>
__device__ __forceinline__ bool action_ok(uint32_t lg, int act, int A) {
  if constexpr (MASKED) return act >= 0 && act < A && ((lg >> act) & 1u) != 0u;
  return true;
}

// per-row entropy and log pi(a) (Categorical.entropy / log_prob, policies.py:87-89)
// MASKED: over S; log pi of an action outside S is -inf (an empty S: H = 0)
template <bool MASKED>
__global__ void categorical_kernel(const float* logits, int ld, int B, int A, const int32_t* actions, float* ent,
                                   float* lpa, const uint32_t* legal) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= B) return;
  const float* z = logits + (long long)m * ld;
  const uint32_t lg = MASKED ? legal_bits(legal[m], A) : 0xFFFFFFFFu;
  const RowLse lse = row_lse<MASKED>(z, A, lg);
  if (ent) ent[m] = row_entropy<MASKED>(z, A, lg, lse);
  if (lpa && actions) {
    const int act = actions[m];
    lpa[m] = action_ok<MASKED>(lg, act, A) ? row_logp(z[act], lse) : -INFINITY;
  }
}

// ---------------------------------------------------------------------------
// n-step targets (objectives.py:178-214), one thread per (env, step), reverse-free:
// target[t] = sum_{i=t..stop} r_i * gp[i-t]  (ascending i, mul+add, no FMA)
// ---------------------------------------------------------------------------
// TRUNC (acmi_returns_trunc): a terminal flagged in tr still ends the sum but keeps a
// bootstrap, from the value of the step after it (the lazy auto-reset's observation);
// the TRUNC = false instantiation takes tr = nullptr and never reads it
template <bool TRUNC>
__global__ void returns_kernel(const float* r, const uint8_t* d, const uint8_t* tr, const float* v, const float* vb,
                               int N, int T, const float* gp, const float* bp, float* tgt, float* adv) {
  // the first terminal at or after t ends the sum
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long long)N * T) return;
  const int n = (int)(idx / T), t = (int)(idx - (long long)n * T);
  const float* rn = r + (long long)n * T;
  const uint8_t* dn = d + (long long)n * T;
  int next_term = T;  // index of the first terminal >= t (T = none)
  for (int i = T - 1; i >= t; --i)
    if (dn[i]) next_term = i;
  const int stop = next_term < T ? next_term : T - 1;
  float acc = 0.f;
  for (int i = t; i <= stop; ++i) acc = __fadd_rn(acc, __fmul_rn(rn[i], gp[i - t]));
  float boot = next_term < T ? 0.f : __fmul_rn(bp[T - t], vb[n]);
  if (TRUNC) {
    if (next_term < T && tr[(long long)n * T + stop] != 0) {
      const float vnext = stop + 1 < T ? v[(long long)n * T + stop + 1] : vb[n];
      boot = __fmul_rn(bp[stop + 1 - t], vnext);
    }
  }
  const float target = __fadd_rn(acc, boot);
  tgt[idx] = target;
  adv[idx] = __fsub_rn(target, v[idx]);
}

// ---------------------------------------------------------------------------
// GAE(lambda) targets (Schulman et al. 2016; an option beyond the reference,
// whose targets are the n-step returns above): one thread per env, reverse scan
//   delta_t = r_t + gamma V_{t+1} (1 - d_t) - V_t,   V_T = V_boot
//   A_t = delta_t + gamma lambda (1 - d_t) A_{t+1},  target_t = A_t + V_t
// with the operation order fixed (__f*_rn: no contraction) so the numpy float32
// restatement (oracle.gae_f32) is bit-exact.  lambda = 1 equals the n-step
// target in exact arithmetic.
// ---------------------------------------------------------------------------
// TRUNC (acmi_gae_trunc): boot = live || truncated_t keeps gamma V_{t+1} in delta_t at
// a truncated terminal; the lambda chain is cut at every terminal all the same
template <bool TRUNC>
__global__ void gae_kernel(const float* r, const uint8_t* d, const uint8_t* tr, const float* v, const float* vb,
                           int N, int T, float gamma, float gl, float* tgt, float* adv) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  float next_v = vb[n], last = 0.f;
  for (int t = T - 1; t >= 0; --t) {
    const long long i = (long long)n * T + t;
    const bool live = d[i] == 0;
    bool boot = live;
    if (TRUNC) boot = live || tr[i] != 0;
    const float vi = v[i];
    const float delta = __fsub_rn(__fadd_rn(r[i], boot ? __fmul_rn(gamma, next_v) : 0.f), vi);
    last = __fadd_rn(delta, live ? __fmul_rn(gl, last) : 0.f);
    adv[i] = last;
    tgt[i] = __fadd_rn(last, vi);
    next_v = vi;
  }
}

// ---------------------------------------------------------------------------
// V-trace targets (Espeholt et al. 2018; beyond the reference): GAE's scan with
// clipped importance weights of the current policy against the behaviour policy.
// A block covers E whole envs (E*T <= VTRACE_BLOCK when T allows it), two phases:
//   1. one thread per (env, step) of the block's envs: log pi(a) by row_lse /
//      row_logp (categorical_kernel's statements: the same bits), D = logp - blogp,
//      w = expf(D), rho = min(rho_bar, w) -> rho[] (global), 0 where D is a NaN.
//      c = min(c_bar, w) is min(c_bar, rho) because rho_bar >= c_bar: only rho travels.
//   2. after one barrier, one thread per env: the reverse scan
//        delta_t = rho_t ((r_t + (boot ? gamma V_{t+1} : 0)) - V_t)
//        acc_t   = delta_t + (live ? ((gamma lambda) c_t) acc_{t+1} : 0)
//        vs_t    = acc_t + V_t                                   -> targets
//        nextv   = live ? vs_{t+1} : (truncated_t ? V_{t+1} : 0)
//        adv_t   = rho_t ((r_t + gamma nextv) - V_t)
//      (vs_T = V_T = v_boot; live / boot as gae_kernel) with the operation order fixed
//      (__f*_rn), so vtrace_f32 (actorcritic/vtrace.py) restates it bit for bit and
//      rho = c = 1 gives gae_kernel's targets.
// The block reads only rho values that its own threads wrote: the barrier orders them.
// ---------------------------------------------------------------------------
constexpr int VTRACE_BLOCK = 256;

template <bool MASKED, bool TRUNC>
__global__ void __launch_bounds__(VTRACE_BLOCK)
    vtrace_kernel(const float* logits, int ld, int A, const int32_t* actions, const float* blogp, const float* r,
                  const uint8_t* d, const uint8_t* tr, const float* v, const float* vb, int N, int T, int E,
                  float gamma, float gl, float rho_bar, float c_bar, const uint32_t* legal, int32_t* bad_rows,
                  float* tgt, float* adv, float* rho, float* logp_out) {
  const int n0 = blockIdx.x * E;  // (the grid is cdiv(N, E) blocks: n0 < N)
  const int envs = N - n0 < E ? N - n0 : E;
  const long long row0 = (long long)n0 * T;
  const int rows = envs * T;  // (<= VTRACE_BLOCK, or one env's T)
  for (int k = threadIdx.x; k < rows; k += VTRACE_BLOCK) {
    const long long m = row0 + k;
    const float* z = logits + m * ld;
    const uint32_t lg = MASKED ? legal_bits(legal[m], A) : 0xFFFFFFFFu;
    const RowLse lse = row_lse<MASKED>(z, A, lg);
    const int act = actions[m];
    const bool ok = action_ok<MASKED>(lg, act, A);
    const float lp = ok ? row_logp(z[act], lse) : -INFINITY;
    if (!ok && bad_rows) atomicAdd(bad_rows, 1);
    const float w = expf(__fsub_rn(lp, blogp[m]));
    // a NaN (by its bits: both log-probabilities -inf, or a NaN logit) weighs nothing
    const bool nan = (__float_as_uint(w) & 0x7fffffffu) > 0x7f800000u;
    rho[m] = nan ? 0.f : fminf(rho_bar, w);
    if (logp_out) logp_out[m] = lp;
  }
  __syncthreads();
  if ((int)threadIdx.x >= envs) return;
  const int n = n0 + threadIdx.x;
  float next_v = vb[n], next_vs = vb[n], acc = 0.f;
  for (int t = T - 1; t >= 0; --t) {
    const long long i = (long long)n * T + t;
    const bool live = d[i] == 0;
    bool trunc = false;
    if (TRUNC) trunc = !live && tr[i] != 0;
    const bool boot = live || trunc;
    const float vi = v[i], ri = r[i], rh = rho[i];
    const float c = fminf(c_bar, rh);
    const float delta = __fmul_rn(rh, __fsub_rn(__fadd_rn(ri, boot ? __fmul_rn(gamma, next_v) : 0.f), vi));
    acc = __fadd_rn(delta, live ? __fmul_rn(__fmul_rn(gl, c), acc) : 0.f);
    const float vs = __fadd_rn(acc, vi);
    const float nextv = live ? next_vs : (trunc ? next_v : 0.f);
    adv[i] = __fmul_rn(rh, __fsub_rn(__fadd_rn(ri, __fmul_rn(gamma, nextv)), vi));
    tgt[i] = vs;
    next_v = vi;
    next_vs = vs;
  }
}

// ---------------------------------------------------------------------------
// advantage normalisation (an option beyond the reference): batch moments in
// double, two fixed-order passes; normalise with the (all-reduced) moments
// ---------------------------------------------------------------------------
constexpr int MOM_BLOCKS = 256;

__global__ void adv_moments_partial_kernel(const float* a, long long M, double* part) {
  __shared__ double red[2][4];
  double s = 0.0, q = 0.0;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < M;
       i += (long long)gridDim.x * blockDim.x) {
    const double x = a[i];
    s += x;
    q += x * x;
  }
  s = wave_sum_d(s);
  q = wave_sum_d(q);
  if ((threadIdx.x & 63) == 0) red[0][threadIdx.x >> 6] = s, red[1][threadIdx.x >> 6] = q;
  __syncthreads();
  if (threadIdx.x == 0) {
    part[2 * blockIdx.x] = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    part[2 * blockIdx.x + 1] = red[1][0] + red[1][1] + red[1][2] + red[1][3];
  }
}

__global__ void adv_moments_final_kernel(const double* part, int nb, double* out) {
  double s = 0.0, q = 0.0;  // one wave, lane-strided then butterfly
  for (int i = threadIdx.x; i < nb; i += 64) s += part[2 * i], q += part[2 * i + 1];
  s = wave_sum_d(s);
  q = wave_sum_d(q);
  if (threadIdx.x == 0) out[0] = s, out[1] = q;
}

__global__ void adv_normalize_kernel(float* a, long long M, const double* mom, double count, double eps) {
  const double mean = mom[0] / count;
  const double var = fmax(mom[1] / count - mean * mean, 0.0);
  const double inv = 1.0 / (sqrt(var) + eps);
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < M;
       i += (long long)gridDim.x * blockDim.x)
    a[i] = (float)(((double)a[i] - mean) * inv);
}

// ---------------------------------------------------------------------------
// per-group reward scaling by the running std of the discounted return (an
// option beyond the reference; baselines' VecNormalize(ret=True), one set of
// statistics per game).  acmi.h states the maths.  Three launches an update:
//   retnorm_scan_kernel    one thread per env: forward scan of R = gamma R + r
//                          (float32, no contraction) from carry[n], the env's
//                          (sum u, sum u^2) in double into ws[n][2]
//   retnorm_groups_kernel  one wave per group: lane-strided over the envs in
//                          ascending order, then the butterfly -- fixed order,
//                          no atomics on the sums
//   retnorm_apply_kernel   ONE block: thread g merges group g's (summed over
//                          ranks) moments into stats[g] (Chan), a barrier, then
//                          every thread scales.  One block because stats is
//                          updated in place and every scale must see the merged
//                          value: a second block could not tell which it read.
//                          The batch is N*T floats (10240 at 512 x 20).
// An env whose group id is >= G is counted in bad_envs, joins no group, keeps
// its rewards as they are; its carry advances all the same.
// ---------------------------------------------------------------------------
constexpr int RETNORM_MAX_GROUPS = 64;
constexpr int RETNORM_SCAN_BLOCK = 256;
constexpr int RETNORM_APPLY_BLOCK = 1024;

__global__ void retnorm_scan_kernel(const float* r, const uint8_t* d, const uint8_t* groups, int N, int T, int G,
                                    float gamma, float* carry, double* part, int32_t* bad_envs) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  float R = carry[n];
  double s = 0.0, q = 0.0;
  for (int t = 0; t < T; ++t) {
    const long long i = (long long)n * T + t;
    R = __fadd_rn(__fmul_rn(R, gamma), r[i]);
    const double u = R;
    s += u;
    q += u * u;  // (u*u is exact in double: a fused multiply-add rounds the same sum)
    if (d[i] != 0) R = 0.f;
  }
  carry[n] = R;
  part[2LL * n] = s;
  part[2LL * n + 1] = q;
  if (groups[n] >= G && bad_envs != nullptr) atomicAdd(bad_envs, 1);
}

// The group reduction of the per-env partials part[n][NS + NM] (retnorm's moments, the
// episode statistics below), one wave per group g: the lanes walk the envs lane-strided in
// ascending order and take those of the group, then the butterfly.  Columns 0..NS-1 are
// summed, columns NS.. are maximised (from -inf); every lane holds the result in v.
// -> the number of envs of the group (exact).
template <int NS, int NM>
__device__ __forceinline__ double group_reduce(const double* part, const uint8_t* groups, int N, int g,
                                               double (&v)[NS + NM]) {
  constexpr int W = NS + NM;
  double c = 0.0;
#pragma unroll
  for (int k = 0; k < W; ++k) v[k] = k < NS ? 0.0 : -INFINITY;
  for (int n = threadIdx.x; n < N; n += 64) {
    if (groups[n] == g) {
      const double* p = part + (long long)W * n;
      c += 1.0;
#pragma unroll
      for (int k = 0; k < NS; ++k) v[k] += p[k];
#pragma unroll
      for (int k = NS; k < W; ++k) v[k] = fmax(v[k], p[k]);
    }
  }
  c = wave_sum_d(c);
#pragma unroll
  for (int k = 0; k < NS; ++k) v[k] = wave_sum_d(v[k]);
#pragma unroll
  for (int k = NS; k < W; ++k) v[k] = wave_max_d(v[k]);
  return c;
}

__global__ void retnorm_groups_kernel(const double* part, const uint8_t* groups, int N, int T, double* moments) {
  const int g = blockIdx.x;  // one wave per group
  double v[2];
  const double c = group_reduce<2, 0>(part, groups, N, g, v);
  if (threadIdx.x == 0) moments[3 * g] = c * (double)T, moments[3 * g + 1] = v[0], moments[3 * g + 2] = v[1];
}

__global__ void __launch_bounds__(RETNORM_APPLY_BLOCK)
    retnorm_apply_kernel(const float* r, const uint8_t* groups, int N, int T, int G, const double* moments,
                         double* stats, double eps, float clip, float* out, float* inv_out) {
  __shared__ float inv[RETNORM_MAX_GROUPS];
  const int g = threadIdx.x;
  if (g < G) {
    double n = stats[3 * g], mean = stats[3 * g + 1], M2 = stats[3 * g + 2];
    const double c = moments[3 * g], s = moments[3 * g + 1], q = moments[3 * g + 2];
    if (c > 0.0) {
      const double mb = s / c;
      const double M2b = fmax(q - s * s / c, 0.0);
      const double tot = n + c;
      const double dl = mb - mean;
      mean += dl * c / tot;
      M2 += M2b + dl * dl * n * c / tot;
      n = tot;
      stats[3 * g] = n, stats[3 * g + 1] = mean, stats[3 * g + 2] = M2;
    }
    const float v = n > 0.0 ? (float)(1.0 / sqrt(M2 / n + eps)) : 1.0f;
    inv[g] = v;
    if (inv_out != nullptr) inv_out[g] = v;
  }
  __syncthreads();
  const long long M = (long long)N * T;
  // elementwise (out may be r); element i = e*T + t, with (e, t) stepped along with i: no divide a turn
  const int de = RETNORM_APPLY_BLOCK / T, dt = RETNORM_APPLY_BLOCK % T;
  int e = (int)threadIdx.x / T, t = (int)threadIdx.x % T;
  for (long long i = threadIdx.x; i < M; i += RETNORM_APPLY_BLOCK) {
    const int ge = groups[e];
    const float x = r[i];
    float v = x;
    if (ge < G) {
      v = __fmul_rn(x, inv[ge]);
      if (clip > 0.f) v = v > clip ? clip : (v < -clip ? -clip : v);  // (a NaN stays a NaN)
    }
    out[i] = v;
    e += de, t += dt;
    if (t >= T) t -= T, ++e;
  }
}

// ---------------------------------------------------------------------------
// episode statistics per group (an option beyond the reference): returns and
// lengths of the episodes that ended in a rollout, accumulated on the device.
// acmi.h states the semantics.  Two launches a call, retnorm_scan's shape:
//   epstats_scan_kernel    one thread per env: walks the env's T episode
//                          rewards, counts its steps from length_carry[n], the
//                          env's eight partials into ws[n][8]
//   epstats_groups_kernel  one wave per group: group_reduce (sums 0..3, maxima
//                          4..7), lane 0 merges into acc[g]
// "No episode" is a NaN by its BITS: a comparison x != x is the optimiser's
// to fold.
// ---------------------------------------------------------------------------
constexpr int EPSTATS_COLS = 8;

__global__ void epstats_scan_kernel(const float* ep, const uint8_t* groups, int N, int T, int G,
                                    int32_t* length_carry, double* part, int32_t* bad_envs) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  int len = length_carry[n];
  double c = 0.0, s = 0.0, q = 0.0, sl = 0.0;
  double rmax = -INFINITY, rmin = -INFINITY, lmax = -INFINITY, lmin = -INFINITY;  // (the minima negated)
  for (int t = 0; t < T; ++t) {
    const float x = ep[(long long)n * T + t];
    ++len;
    if ((__float_as_uint(x) & 0x7fffffffu) <= 0x7f800000u) {  // not a NaN: an episode ended here
      const double r = x, l = len;
      c += 1.0;
      s += r;
      q += r * r;  // (r*r is exact in double: a fused multiply-add rounds the same sum)
      sl += l;
      rmax = fmax(rmax, r), rmin = fmax(rmin, -r);
      lmax = fmax(lmax, l), lmin = fmax(lmin, -l);
      len = 0;
    }
  }
  length_carry[n] = len;
  double* p = part + (long long)EPSTATS_COLS * n;
  p[0] = c, p[1] = s, p[2] = q, p[3] = sl;
  p[4] = rmax, p[5] = rmin, p[6] = lmax, p[7] = lmin;
  if (groups[n] >= G && bad_envs != nullptr) atomicAdd(bad_envs, 1);
}

__global__ void epstats_groups_kernel(const double* part, const uint8_t* groups, int N, double* acc) {
  const int g = blockIdx.x;  // one wave per group
  double v[EPSTATS_COLS];
  group_reduce<4, 4>(part, groups, N, g, v);
  if (threadIdx.x == 0) {
    double* a = acc + EPSTATS_COLS * g;
#pragma unroll
    for (int k = 0; k < 4; ++k) a[k] += v[k];
#pragma unroll
    for (int k = 4; k < EPSTATS_COLS; ++k) a[k] = fmax(a[k], v[k]);
  }
}

// ---------------------------------------------------------------------------
// A2C and PPO losses + head gradients: one thread per row, the row's policy
// arithmetic and the block's sums stated once for both
// ---------------------------------------------------------------------------
constexpr int LOSS_BLOCK = 256;
constexpr int A2C_SUMS = 3;  // policy term, entropy, value loss
constexpr int PPO_SUMS = 5;  // surrogate, entropy, value loss, old_logp - logp, clipped rows

// The policy part of a good row: lse and H over S, lpa = log pi(act), and the columns
//   g[k] = dL/dz_k = -inv [w (onehot_k - p_k) - beta p_k (log p_k + H)]  on S, +0 outside it.
// weight(lpa) gives w, the policy term's weight (A2C: adv; PPO: r adv where the
// unclipped term is active, r = exp(lpa - old_logp)); with w = adv, PPO's columns
// are A2C's bit for bit because they are these statements.
struct RowPolicy {
  RowLse lse;
  float H, lpa;
};
template <bool MASKED, class Weight>
__device__ __forceinline__ RowPolicy policy_row(const float* z, int A, uint32_t lg, int act, float beta, float inv,
                                                float* g, Weight weight) {
  RowPolicy r;
  r.lse = row_lse<MASKED>(z, A, lg);
  r.H = row_entropy<MASKED>(z, A, lg, r.lse);
  r.lpa = row_logp(z[act], r.lse);
  const float w = weight(r.lpa);
  for (int a = 0; a < A; ++a) {
    if (!legal_at<MASKED>(lg, a)) {
      g[a] = 0.f;
      continue;
    }
    const float lp = row_logp(z[a], r.lse);
    const float p = expf(lp);
    const float oh = a == act ? 1.f : 0.f;
    g[a] = -inv * (w * (oh - p) - beta * p * (lp + r.H));
  }
  return r;
}

// A block's K sums into part[block][K] (every thread of the block calls it): a wave
// butterfly, then thread k adds sum k's wave partials in ascending wave order
template <int K>
__device__ __forceinline__ void block_sums(float (&s)[K], float* part) {
  __shared__ float red[K][LOSS_BLOCK / 64];
#pragma unroll
  for (int k = 0; k < K; ++k) s[k] = wave_sum(s[k]);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int k = 0; k < K; ++k) red[k][w] = s[k];
  __syncthreads();
  if (threadIdx.x < K) {
    float a = 0.f;
    for (int i = 0; i < LOSS_BLOCK / 64; ++i) a += red[threadIdx.x][i];
    part[blockIdx.x * K + threadIdx.x] = a;
  }
}

// A2C (objectives.py:123-154, :78).
// MASKED: the softmax, entropy and policy columns over S (columns outside S are
// +0); a bad row -- S empty or the taken action outside S -- adds nothing to the
// policy and entropy sums, gets zero policy columns, keeps its value term and
// counts in bad_rows (nullable).
template <bool MASKED>
__global__ void a2c_loss_kernel(const float* logits, int ld, const float* values, const int32_t* actions,
                                const float* targets, const float* adv, int M, int A, float beta, float vcoef,
                                float gscale, float* dhead, int ldh, float* part, const uint32_t* legal,
                                int32_t* bad_rows) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  float s[A2C_SUMS] = {0.f, 0.f, 0.f};
  if (m < M) {
    const float* z = logits + (long long)m * ld;
    const uint32_t lg = MASKED ? legal_bits(legal[m], A) : 0xFFFFFFFFu;
    const int act = actions[m];
    const bool ok = action_ok<MASKED>(lg, act, A);
    const float ad = adv[m];
    const float diff = targets[m] - values[m];
    s[2] = 0.5f * diff * diff;
    // dL/dz_k = -(1/M)[adv (onehot_k - p_k) - beta p_k (log p_k + H)]
    const float inv = gscale / (float)M;
    float* g = dhead + (long long)m * ldh;
    if (ok) {
      const RowPolicy rp = policy_row<MASKED>(z, A, lg, act, beta, inv, g, [&](float lpa) {
        s[0] = ad * lpa;
        return ad;
      });
      s[1] = rp.H;
    } else {
      for (int a = 0; a < A; ++a) g[a] = 0.f;
      if (bad_rows) atomicAdd(bad_rows, 1);
    }
    // d(vcoef * L_v)/dV = vcoef * (V - target) / M
    g[A] = vcoef * inv * (values[m] - targets[m]);
    for (int a = A + 1; a < ldh; ++a) g[a] = 0.f;
  }
  block_sums(s, part);
}

// PPO clipped surrogate (Schulman et al. 2017; beyond the reference): with old_logp
// from categorical_kernel on the same logits r is exactly 1 and dhead is
// a2c_loss_kernel's, bit for bit.
// MASKED: as a2c_loss_kernel; a bad row adds nothing to the surrogate, entropy,
// KL and clipped-row sums either.
template <bool MASKED>
__global__ void ppo_loss_kernel(const float* logits, int ld, const float* values, const int32_t* actions,
                                const float* old_logp, const float* old_values, const float* targets,
                                const float* adv, int M, int A, float clip_eps, float vclip, float beta,
                                float vcoef, float gscale, float* dhead, int ldh, float* part,
                                const uint32_t* legal, int32_t* bad_rows) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  float s[PPO_SUMS] = {0.f, 0.f, 0.f, 0.f, 0.f};
  if (m < M) {
    const float* z = logits + (long long)m * ld;
    const uint32_t lg = MASKED ? legal_bits(legal[m], A) : 0xFFFFFFFFu;
    const int act = actions[m];
    const bool ok = action_ok<MASKED>(lg, act, A);
    const float ad = adv[m];
    const float v = values[m], tg = targets[m];
    const float diff = tg - v;
    s[2] = 0.5f * diff * diff;
    bool val_on = true;
    if (vclip > 0.f) {
      const float vo = old_values[m];
      const float dv = v - vo;
      // only a value that left the range can lose its gradient: inside it Vc is V
      if (fabsf(dv) > vclip) {
        const float dc = tg - (vo + fminf(fmaxf(dv, -vclip), vclip));
        const float sc = 0.5f * dc * dc;
        if (sc > s[2]) {
          s[2] = sc;
          val_on = false;
        }
      }
    }
    const float inv = gscale / (float)M;
    float* g = dhead + (long long)m * ldh;
    if (ok) {
      // dL/dz_k = -(1/M)[adv r (onehot_k - p_k) [unclipped] - beta p_k (log p_k + H)]
      const RowPolicy rp = policy_row<MASKED>(z, A, lg, act, beta, inv, g, [&](float lpa) {
        const float olp = old_logp[m];
        const float r = expf(lpa - olp);
        const float rc = fminf(fmaxf(r, 1.f - clip_eps), 1.f + clip_eps);
        const float s1 = r * ad, s2 = rc * ad;
        // the unclipped term is the active minimum (ties: r inside the range, s1 == s2)
        const bool pol_on = s1 <= s2;
        s[0] = pol_on ? s1 : s2;
        s[3] = olp - lpa;
        s[4] = fabsf(r - 1.f) > clip_eps ? 1.f : 0.f;
        return pol_on ? s1 : 0.f;
      });
      s[1] = rp.H;
    } else {
      for (int a = 0; a < A; ++a) g[a] = 0.f;
      if (bad_rows) atomicAdd(bad_rows, 1);
    }
    // d(vcoef * L_v)/dV = vcoef * (V - target) / M where the unclipped square is active
    const float gv = vcoef * inv * (values[m] - targets[m]);
    g[A] = val_on ? gv : 0.f;
    for (int a = A + 1; a < ldh; ++a) g[a] = 0.f;
  }
  block_sums(s, part);
}

// K = A2C_SUMS / PPO_SUMS: out[0..2] = policy loss, value loss, mean entropy; PPO
// adds out[3] = mean(old_logp - logp) and the clipped fraction
template <int K>
__global__ void loss_final_kernel(const float* part, int nb, int M, float beta, float scale, float* out,
                                  float* clip_frac_out) {
  // one wave: deterministic fixed-order sums
  float s[K];
  for (int k = 0; k < K; ++k) s[k] = 0.f;
  for (int i = threadIdx.x; i < nb; i += 64)
    for (int k = 0; k < K; ++k) s[k] += part[i * K + k];
  for (int k = 0; k < K; ++k) s[k] = wave_sum(s[k]);
  if (threadIdx.x == 0) {
    // scale = 1/world_size: the SUM all-reduce of the update buffer then leaves
    // the global means (every rank holds M rows)
    const float mean_pl = s[0] / (float)M;
    const float mean_h = s[1] / (float)M;
    out[0] = scale * -(mean_pl + beta * mean_h);
    out[1] = scale * (s[2] / (float)M);
    out[2] = scale * mean_h;
    if constexpr (K == PPO_SUMS) {
      out[3] = scale * (s[3] / (float)M);
      if (clip_frac_out) clip_frac_out[0] = scale * (s[4] / (float)M);
    }
  }
}

// ---------------------------------------------------------------------------
// row gather (PPO's shuffled minibatches; beyond the reference): a pure copy.
// One block per output row: its 256 threads move the image's 1764 16-byte
// words (lane-contiguous: 1 KiB per wave instruction; all of a thread's loads
// are issued before its first store), thread 0 the row's <= 8 four-byte vector
// elements.  An index outside [0, src_rows) zero-fills the row and counts it.
// Without an image (obs == nullptr): one thread per row.
// ---------------------------------------------------------------------------
constexpr int GATHER_MAX_VECS = 8;
constexpr int GATHER_BLOCK = 256;
constexpr int GATHER_WORDS_PER_THREAD = (FRAME_WORDS + GATHER_BLOCK - 1) / GATHER_BLOCK;  // 7

struct GatherVecs {
  const uint32_t* src[GATHER_MAX_VECS];
  uint32_t* dst[GATHER_MAX_VECS];
};

__device__ __forceinline__ void gather_row_vectors(const GatherVecs& v, int nvec, long long r, long long i,
                                                   bool ok) {
#pragma unroll
  for (int k = 0; k < GATHER_MAX_VECS; ++k)
    if (k < nvec) v.dst[k][r] = ok ? v.src[k][i] : 0u;
}

__global__ __launch_bounds__(GATHER_BLOCK) void gather_rows_kernel(
    const uint8_t* obs, long long img_stride, long long src_rows, const int32_t* index, long long rows,
    uint8_t* obs_out, long long out_stride, int nvec, GatherVecs vecs, int32_t* bad) {
  if (!obs) {
    const long long r = (long long)blockIdx.x * GATHER_BLOCK + threadIdx.x;
    if (r >= rows) return;
    const long long i = index[r];
    const bool ok = i >= 0 && i < src_rows;
    gather_row_vectors(vecs, nvec, r, i, ok);
    if (!ok && bad) atomicAdd(bad, 1);
    return;
  }
  const long long r = blockIdx.x;  // (the grid is exactly `rows` blocks)
  const long long i = index[r];
  const bool ok = i >= 0 && i < src_rows;  // uniform over the block
  uint4* out = reinterpret_cast<uint4*>(obs_out + r * out_stride);
  uint4 w[GATHER_WORDS_PER_THREAD];
  if (ok) {
    const uint4* in = reinterpret_cast<const uint4*>(obs + i * img_stride);
#pragma unroll
    for (int u = 0; u < GATHER_WORDS_PER_THREAD; ++u) {
      const int g = threadIdx.x + u * GATHER_BLOCK;
      if (g < FRAME_WORDS) w[u] = in[g];
    }
  } else {
#pragma unroll
    for (int u = 0; u < GATHER_WORDS_PER_THREAD; ++u) w[u] = make_uint4(0u, 0u, 0u, 0u);
  }
#pragma unroll
  for (int u = 0; u < GATHER_WORDS_PER_THREAD; ++u) {
    const int g = threadIdx.x + u * GATHER_BLOCK;
    if (g < FRAME_WORDS) out[g] = w[u];
  }
  if (threadIdx.x == 0) {
    gather_row_vectors(vecs, nvec, r, i, ok);
    if (!ok && bad) atomicAdd(bad, 1);
  }
}

// ---------------------------------------------------------------------------
// deterministic global sum of squares / dot product (two passes)
// ---------------------------------------------------------------------------
constexpr int RED_BLOCKS = 512;

__global__ void dot_partial_kernel(const float* x, const float* y, long long n, float* part) {
  __shared__ float red[4];
  float s = 0.f;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (long long)gridDim.x * blockDim.x)
    s += x[i] * y[i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

__device__ float block_final_sum(const float* part, int nb) {
  // called by one full block of 256: fixed-order reduction
  __shared__ float red[4];
  float s = 0.f;
  for (int i = threadIdx.x; i < nb; i += blockDim.x) s += part[i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  const float tot = red[0] + red[1] + red[2] + red[3];
  __syncthreads();
  return tot;
}

// scale[0] = clip factor (TF clip_by_global_norm), scale[1] = global norm
__global__ void clip_scale_kernel(const float* part, int nb, float clip_norm, float* scale,
                                  float* norm_out) {
  const float ss = block_final_sum(part, nb);
  if (threadIdx.x == 0) {
    const float gn = sqrtf(ss);
    float sc = 1.f;
    if (clip_norm > 0.f) sc = clip_norm * fminf(1.f / gn, 1.f / clip_norm);
    scale[0] = sc;
    scale[1] = gn;
    if (norm_out) norm_out[0] = gn;
  }
}

__global__ void momentum_kernel(float* p, float* acc, const float* g, long long n, float lr,
                                float mom, const float* scale) {
  const float sc = scale[0];
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (long long)gridDim.x * blockDim.x) {
    const float a = mom * acc[i] + g[i] * sc;
    acc[i] = a;
    p[i] -= lr * a;
  }
}

__global__ void rmsprop_kernel(float* p, float* ms, float* mom, const float* g, long long n,
                               float lr, float decay, float momentum, float eps,
                               const float* scale) {
  const float sc = scale[0];
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (long long)gridDim.x * blockDim.x) {
    const float gi = g[i] * sc;
    const float m2 = decay * ms[i] + (1.f - decay) * gi * gi;
    ms[i] = m2;
    const float mo = momentum * mom[i] + lr * gi / sqrtf(m2 + eps);
    mom[i] = mo;
    p[i] -= mo;
  }
}

// TF1 AdamOptimizer: lr_t = lr sqrt(1 - b2^t) / (1 - b1^t) comes from the host
__global__ void adam_kernel(float* p, float* m, float* v, const float* g, long long n, float lr_t,
                            float beta1, float beta2, float eps, const float* scale) {
  const float sc = scale[0];
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (long long)gridDim.x * blockDim.x) {
    const float gi = g[i] * sc;
    const float mi = beta1 * m[i] + (1.f - beta1) * gi;
    const float vi = beta2 * v[i] + (1.f - beta2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    p[i] -= lr_t * mi / (sqrtf(vi) + eps);
  }
}

// ---------------------------------------------------------------------------
// batched synthetic Atari stepper (multi_env.py:121-137 + wrappers.py:201-235
// + wrappers.py:263-323).  One workgroup per env; 1764 words of 4 pixels.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void env_reset_kernel(acmi_env_state_t st, int env_offset,
                                                        uint32_t seed, uint8_t* obs,
                                                        long long stride) {
  const int n = blockIdx.x;
  const uint32_t e = (uint32_t)(env_offset + n);
  const GameParams gp = game_params(env_game(st, n));
  const uint32_t base = key4(seed ^ gp.salt, e, 0u, RESET_TAG);
  uint4* out = reinterpret_cast<uint4*>(obs + (long long)n * stride);
  for (int g = threadIdx.x; g < FRAME_WORDS; g += blockDim.x) {
    const uint32_t w = word_hash(base, (uint32_t)g);
    uint4 o;
    o.x = (w & 255u) * 0x01010101u;
    o.y = ((w >> 8) & 255u) * 0x01010101u;
    o.z = ((w >> 16) & 255u) * 0x01010101u;
    o.w = (w >> 24) * 0x01010101u;
    out[g] = o;
  }
  if (threadIdx.x == 0) {
    st.episode[n] = 0;
    st.step[n] = 0;
    st.length[n] = episode_length(seed, e, 0u, gp);
    st.total[n] = 0.f;
    st.done[n] = 0;
  }
}

__global__ __launch_bounds__(256) void env_step_kernel(
    acmi_env_state_t st, int env_offset, uint32_t seed, const int32_t* actions,
    const uint8_t* obs_in, long long in_stride, uint8_t* obs_out, long long out_stride,
    float* rewards, uint8_t* terminals, float* ep_rewards, long long ld) {
  const int n = blockIdx.x;
  env_step_block(st, n, (uint32_t)(env_offset + n), seed, (uint32_t)actions[n],
                 obs_in + (long long)n * in_stride, obs_out + (long long)n * out_stride, rewards,
                 terminals, ep_rewards, ld);
}

}  // namespace acmi

using namespace acmi;

extern "C" {

int acmi_sample_actions(const float* logits, int ld, int B, int A, uint32_t seed,
                        uint32_t stream_id, uint32_t counter, const float* uniforms, int mode,
                        int32_t* actions, int32_t* bad_rows, acmi_stream_t stream) {
  return acmi_sample_actions_at(logits, ld, B, A, seed, stream_id, counter, 0, uniforms, mode,
                                actions, bad_rows, stream);
}

int acmi_sample_actions_at(const float* logits, int ld, int B, int A, uint32_t seed,
                           uint32_t stream_id, uint32_t counter, int row_offset,
                           const float* uniforms, int mode, int32_t* actions, int32_t* bad_rows,
                           acmi_stream_t stream) {
  return acmi_sample_actions_dev(logits, ld, B, A, seed, stream_id, nullptr, counter, row_offset,
                                 uniforms, mode, actions, bad_rows, stream);
}

// The launchers below serve an unmasked / non-truncating entry point and its _masked /
// _trunc twin: legal, bad_rows and truncated are nullable (null: the unmasked kernel),
// name is the entry point that was called (error text).
static int sample_launch(const char* name, const float* logits, int ld, int B, int A, uint32_t seed,
                         uint32_t stream_id, const uint32_t* counter_dev, uint32_t counter_add, int row_offset,
                         const float* uniforms, int mode, const uint32_t* legal, int32_t* actions,
                         int32_t* bad_rows, acmi_stream_t stream) {
  ACMI_REQUIRE(logits && actions && bad_rows && B >= 0 && A >= 1 && ld >= A && row_offset >= 0,
               ACMI_ERR_ARG, "%s: bad arguments", name);
  if (B == 0) return ACMI_OK;
  const auto kern = legal ? sample_kernel<true> : sample_kernel<false>;
  hipLaunchKernelGGL(kern, dim3(cdiv(B, 256)), dim3(256), 0, (hipStream_t)stream, logits, ld, B, A, seed,
                     stream_id, counter_add, counter_dev, (uint32_t)row_offset, uniforms, mode, actions, bad_rows,
                     legal);
  ACMI_LAUNCH_CHECK(name);
  return ACMI_OK;
}

int acmi_sample_actions_dev(const float* logits, int ld, int B, int A, uint32_t seed,
                            uint32_t stream_id, const uint32_t* counter_dev, uint32_t counter_add,
                            int row_offset, const float* uniforms, int mode, int32_t* actions,
                            int32_t* bad_rows, acmi_stream_t stream) {
  return sample_launch("acmi_sample_actions", logits, ld, B, A, seed, stream_id, counter_dev, counter_add,
                       row_offset, uniforms, mode, nullptr, actions, bad_rows, stream);
}

int acmi_sample_actions_masked(const float* logits, int ld, int B, int A, uint32_t seed,
                               uint32_t stream_id, const uint32_t* counter_dev, uint32_t counter_add,
                               int row_offset, const float* uniforms, int mode, const uint32_t* legal,
                               int32_t* actions, int32_t* bad_rows, acmi_stream_t stream) {
  ACMI_REQUIRE_MASK("acmi_sample_actions_masked", legal, A);
  return sample_launch("acmi_sample_actions_masked", logits, ld, B, A, seed, stream_id, counter_dev, counter_add,
                       row_offset, uniforms, mode, legal, actions, bad_rows, stream);
}

static int categorical_launch(const char* name, const float* logits, int ld, int B, int A, const int32_t* actions,
                              const uint32_t* legal, float* entropy, float* log_prob, acmi_stream_t stream) {
  ACMI_REQUIRE(logits && B >= 0 && A >= 1 && ld >= A && (entropy || log_prob) && (!log_prob || actions),
               ACMI_ERR_ARG, "%s: bad arguments", name);
  if (B == 0) return ACMI_OK;
  const auto kern = legal ? categorical_kernel<true> : categorical_kernel<false>;
  hipLaunchKernelGGL(kern, dim3(cdiv(B, 256)), dim3(256), 0, (hipStream_t)stream, logits, ld, B, A, actions,
                     entropy, log_prob, legal);
  ACMI_LAUNCH_CHECK(name);
  return ACMI_OK;
}

int acmi_categorical(const float* logits, int ld, int B, int A, const int32_t* actions,
                     float* entropy, float* log_prob, acmi_stream_t stream) {
  return categorical_launch("acmi_categorical", logits, ld, B, A, actions, nullptr, entropy, log_prob, stream);
}

int acmi_categorical_masked(const float* logits, int ld, int B, int A, const int32_t* actions,
                            const uint32_t* legal, float* entropy, float* log_prob, acmi_stream_t stream) {
  ACMI_REQUIRE_MASK("acmi_categorical_masked", legal, A);
  return categorical_launch("acmi_categorical_masked", logits, ld, B, A, actions, legal, entropy, log_prob, stream);
}

static int returns_launch(const char* name, const float* rewards, const uint8_t* terminals,
                          const uint8_t* truncated, const float* values, const float* v_boot, int N, int T,
                          const float* gamma_pow, const float* boot_pow, float* targets, float* adv,
                          acmi_stream_t stream) {
  ACMI_REQUIRE(rewards && terminals && values && v_boot && gamma_pow && boot_pow && targets &&
                   adv && N >= 0 && T >= 1,
               ACMI_ERR_ARG, "%s: bad arguments", name);
  if (N == 0) return ACMI_OK;
  const auto kern = truncated ? returns_kernel<true> : returns_kernel<false>;
  hipLaunchKernelGGL(kern, dim3(cdiv((long long)N * T, 256)), dim3(256), 0, (hipStream_t)stream, rewards,
                     terminals, truncated, values, v_boot, N, T, gamma_pow, boot_pow, targets, adv);
  ACMI_LAUNCH_CHECK(name);
  return ACMI_OK;
}

int acmi_returns(const float* rewards, const uint8_t* terminals, const float* values,
                 const float* v_boot, int N, int T, const float* gamma_pow,
                 const float* boot_pow, float* targets, float* adv, acmi_stream_t stream) {
  return returns_launch("acmi_returns", rewards, terminals, nullptr, values, v_boot, N, T, gamma_pow, boot_pow,
                        targets, adv, stream);
}

int acmi_returns_trunc(const float* rewards, const uint8_t* terminals, const uint8_t* truncated,
                       const float* values, const float* v_boot, int N, int T, const float* gamma_pow,
                       const float* boot_pow, float* targets, float* adv, acmi_stream_t stream) {
  ACMI_REQUIRE(truncated, ACMI_ERR_ARG, "acmi_returns_trunc: bad arguments");
  return returns_launch("acmi_returns_trunc", rewards, terminals, truncated, values, v_boot, N, T, gamma_pow,
                        boot_pow, targets, adv, stream);
}

static int gae_launch(const char* name, const float* rewards, const uint8_t* terminals, const uint8_t* truncated,
                      const float* values, const float* v_boot, int N, int T, float gamma, float lambda,
                      float* targets, float* adv, acmi_stream_t stream) {
  ACMI_REQUIRE(rewards && terminals && values && v_boot && targets && adv && N >= 0 && T >= 1 &&
                   lambda >= 0.f && lambda <= 1.f,
               ACMI_ERR_ARG, "%s: bad arguments", name);
  if (N == 0) return ACMI_OK;
  const auto kern = truncated ? gae_kernel<true> : gae_kernel<false>;
  hipLaunchKernelGGL(kern, dim3(cdiv(N, 64)), dim3(64), 0, (hipStream_t)stream, rewards, terminals, truncated,
                     values, v_boot, N, T, gamma, gamma * lambda, targets, adv);
  ACMI_LAUNCH_CHECK(name);
  return ACMI_OK;
}

int acmi_gae(const float* rewards, const uint8_t* terminals, const float* values, const float* v_boot,
             int N, int T, float gamma, float lambda, float* targets, float* adv, acmi_stream_t stream) {
  return gae_launch("acmi_gae", rewards, terminals, nullptr, values, v_boot, N, T, gamma, lambda, targets, adv,
                    stream);
}

int acmi_gae_trunc(const float* rewards, const uint8_t* terminals, const uint8_t* truncated, const float* values,
                   const float* v_boot, int N, int T, float gamma, float lambda, float* targets, float* adv,
                   acmi_stream_t stream) {
  ACMI_REQUIRE(truncated, ACMI_ERR_ARG, "acmi_gae_trunc: bad arguments");
  return gae_launch("acmi_gae_trunc", rewards, terminals, truncated, values, v_boot, N, T, gamma, lambda, targets,
                    adv, stream);
}

int acmi_vtrace(const float* logits, int ld, int A, const int32_t* actions, const float* behaviour_logp,
                const float* rewards, const uint8_t* terminals, const uint8_t* truncated, const float* values,
                const float* v_boot, int N, int T, float gamma, float lambda, float rho_bar, float c_bar,
                const uint32_t* legal, int32_t* bad_rows, float* targets, float* adv, float* rho, float* log_prob,
                acmi_stream_t stream) {
  ACMI_REQUIRE(logits && actions && behaviour_logp && rewards && terminals && values && v_boot && targets && adv &&
                   rho,
               ACMI_ERR_ARG, "acmi_vtrace: a required pointer is NULL");
  ACMI_REQUIRE(N >= 0 && T >= 0 && A >= 1 && ld >= A && (long long)N * T <= INT32_MAX, ACMI_ERR_ARG,
               "acmi_vtrace: N=%d, T=%d must not be negative (N*T below 2^31), A=%d at least 1 and ld=%d at least A",
               N, T, A, ld);
  ACMI_REQUIRE(!legal || A <= 32, ACMI_ERR_ARG, "acmi_vtrace: num_actions=%d, a legal-action mask holds at most 32",
               A);
  // (written so that a NaN fails each of them)
  ACMI_REQUIRE(lambda >= 0.f && lambda <= 1.f && c_bar > 0.f && rho_bar >= c_bar, ACMI_ERR_ARG,
               "acmi_vtrace: lambda=%g outside [0, 1], c_bar=%g not positive or rho_bar=%g below c_bar",
               (double)lambda, (double)c_bar, (double)rho_bar);
  if (N == 0 || T == 0) return ACMI_OK;
  const int E = T < VTRACE_BLOCK ? VTRACE_BLOCK / T : 1;  // whole envs per block
  const auto kern = legal ? (truncated ? vtrace_kernel<true, true> : vtrace_kernel<true, false>)
                          : (truncated ? vtrace_kernel<false, true> : vtrace_kernel<false, false>);
  hipLaunchKernelGGL(kern, dim3(cdiv(N, E)), dim3(VTRACE_BLOCK), 0, (hipStream_t)stream, logits, ld, A, actions,
                     behaviour_logp, rewards, terminals, truncated, values, v_boot, N, T, E, gamma, gamma * lambda,
                     rho_bar, c_bar, legal, bad_rows, targets, adv, rho, log_prob);
  ACMI_LAUNCH_CHECK("acmi_vtrace");
  return ACMI_OK;
}

int64_t acmi_adv_moments_ws_doubles(int64_t M) { (void)M; return 2LL * MOM_BLOCKS; }

int acmi_adv_moments(const float* adv, int64_t M, double* ws, double* moments, acmi_stream_t stream) {
  ACMI_REQUIRE(adv && ws && moments && M >= 1, ACMI_ERR_ARG, "acmi_adv_moments: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(adv_moments_partial_kernel, dim3(MOM_BLOCKS), dim3(256), 0, s, adv, (long long)M, ws);
  hipLaunchKernelGGL(adv_moments_final_kernel, dim3(1), dim3(64), 0, s, ws, MOM_BLOCKS, moments);
  ACMI_LAUNCH_CHECK("acmi_adv_moments");
  return ACMI_OK;
}

int acmi_adv_normalize(float* adv, int64_t M, const double* moments, double count, double eps,
                       acmi_stream_t stream) {
  ACMI_REQUIRE(adv && moments && M >= 1 && count >= 1.0 && eps >= 0.0, ACMI_ERR_ARG,
               "acmi_adv_normalize: bad arguments");
  hipLaunchKernelGGL(adv_normalize_kernel, dim3(std::min<long long>(cdiv(M, 256), 1024)), dim3(256), 0,
                     (hipStream_t)stream, adv, (long long)M, moments, count, eps);
  ACMI_LAUNCH_CHECK("acmi_adv_normalize");
  return ACMI_OK;
}

int64_t acmi_retnorm_ws_doubles(int64_t N) { return N < 1 ? 0 : 2 * N; }

int acmi_retnorm_scan(const float* rewards, const uint8_t* terminals, const uint8_t* groups, int N, int T, int G,
                      float gamma, float* carry, double* ws, double* moments, int32_t* bad_envs,
                      acmi_stream_t stream) {
  ACMI_REQUIRE(rewards && terminals && groups && carry && ws && moments, ACMI_ERR_ARG,
               "acmi_retnorm_scan: a required pointer is NULL");
  ACMI_REQUIRE(N >= 1 && T >= 1 && G >= 1 && G <= RETNORM_MAX_GROUPS, ACMI_ERR_ARG,
               "acmi_retnorm_scan: N=%d, T=%d must be at least 1 and G=%d in 1..%d", N, T, G, RETNORM_MAX_GROUPS);
  ACMI_REQUIRE(gamma >= 0.f && gamma <= 1.f, ACMI_ERR_ARG, "acmi_retnorm_scan: gamma=%g outside [0, 1]",
               (double)gamma);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(retnorm_scan_kernel, dim3(cdiv(N, RETNORM_SCAN_BLOCK)), dim3(RETNORM_SCAN_BLOCK), 0, s, rewards,
                     terminals, groups, N, T, G, gamma, carry, ws, bad_envs);
  hipLaunchKernelGGL(retnorm_groups_kernel, dim3(G), dim3(64), 0, s, ws, groups, N, T, moments);
  ACMI_LAUNCH_CHECK("acmi_retnorm_scan");
  return ACMI_OK;
}

int acmi_retnorm_apply(const float* rewards, const uint8_t* groups, int N, int T, int G, const double* moments,
                       double* stats, double eps, float clip, float* out, float* inv_out, acmi_stream_t stream) {
  ACMI_REQUIRE(rewards && groups && moments && stats && out, ACMI_ERR_ARG,
               "acmi_retnorm_apply: a required pointer is NULL");
  ACMI_REQUIRE(N >= 1 && T >= 1 && G >= 1 && G <= RETNORM_MAX_GROUPS, ACMI_ERR_ARG,
               "acmi_retnorm_apply: N=%d, T=%d must be at least 1 and G=%d in 1..%d", N, T, G, RETNORM_MAX_GROUPS);
  ACMI_REQUIRE(eps >= 0.0 && clip == clip, ACMI_ERR_ARG, "acmi_retnorm_apply: eps=%g must not be negative, clip=%g",
               eps, (double)clip);
  hipLaunchKernelGGL(retnorm_apply_kernel, dim3(1), dim3(RETNORM_APPLY_BLOCK), 0, (hipStream_t)stream, rewards,
                     groups, N, T, G, moments, stats, eps, clip, out, inv_out);
  ACMI_LAUNCH_CHECK("acmi_retnorm_apply");
  return ACMI_OK;
}

int64_t acmi_epstats_ws_doubles(int64_t N) { return N < 1 ? 0 : EPSTATS_COLS * N; }

int acmi_epstats_update(const float* episode_rewards, const uint8_t* groups, int N, int T, int G,
                        int32_t* length_carry, double* ws, double* acc, int32_t* bad_envs, acmi_stream_t stream) {
  ACMI_REQUIRE(episode_rewards && groups && length_carry && ws && acc, ACMI_ERR_ARG,
               "acmi_epstats_update: a required pointer is NULL");
  ACMI_REQUIRE(N >= 1 && T >= 1 && G >= 1 && G <= RETNORM_MAX_GROUPS, ACMI_ERR_ARG,
               "acmi_epstats_update: N=%d, T=%d must be at least 1 and G=%d in 1..%d", N, T, G, RETNORM_MAX_GROUPS);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(epstats_scan_kernel, dim3(cdiv(N, RETNORM_SCAN_BLOCK)), dim3(RETNORM_SCAN_BLOCK), 0, s,
                     episode_rewards, groups, N, T, G, length_carry, ws, bad_envs);
  hipLaunchKernelGGL(epstats_groups_kernel, dim3(G), dim3(64), 0, s, ws, groups, N, acc);
  ACMI_LAUNCH_CHECK("acmi_epstats_update");
  return ACMI_OK;
}

int64_t acmi_a2c_loss_ws_floats(int M) { return (long long)A2C_SUMS * cdiv(M, LOSS_BLOCK) + 16; }

static int a2c_loss_launch(const char* name, const float* logits, int ld, const float* values,
                           const int32_t* actions, const float* targets, const float* adv, int M, int A, float beta,
                           float vcoef, float grad_scale, float* dhead, int ldh, float* ws, float* loss_out,
                           const uint32_t* legal, int32_t* bad_rows, acmi_stream_t stream) {
  ACMI_REQUIRE(logits && values && actions && targets && adv && dhead && ws && loss_out &&
                   M > 0 && A >= 1 && ld >= A && ldh >= A + 1,
               ACMI_ERR_ARG, "%s: bad arguments", name);
  const int nb = cdiv(M, LOSS_BLOCK);
  hipStream_t s = (hipStream_t)stream;
  const auto kern = legal ? a2c_loss_kernel<true> : a2c_loss_kernel<false>;
  hipLaunchKernelGGL(kern, dim3(nb), dim3(LOSS_BLOCK), 0, s, logits, ld, values, actions, targets, adv, M, A, beta,
                     vcoef, grad_scale, dhead, ldh, ws, legal, bad_rows);
  hipLaunchKernelGGL(loss_final_kernel<A2C_SUMS>, dim3(1), dim3(64), 0, s, ws, nb, M, beta, grad_scale, loss_out,
                     nullptr);
  ACMI_LAUNCH_CHECK(name);
  return ACMI_OK;
}

int acmi_a2c_loss(const float* logits, int ld, const float* values, const int32_t* actions,
                  const float* targets, const float* adv, int M, int A, float beta, float vcoef,
                  float grad_scale, float* dhead, int ldh, float* ws, float* loss_out,
                  acmi_stream_t stream) {
  return a2c_loss_launch("acmi_a2c_loss", logits, ld, values, actions, targets, adv, M, A, beta, vcoef, grad_scale,
                         dhead, ldh, ws, loss_out, nullptr, nullptr, stream);
}

int acmi_a2c_loss_masked(const float* logits, int ld, const float* values, const int32_t* actions,
                         const float* targets, const float* adv, int M, int A, float beta, float vcoef,
                         float grad_scale, float* dhead, int ldh, float* ws, float* loss_out,
                         const uint32_t* legal, int32_t* bad_rows, acmi_stream_t stream) {
  ACMI_REQUIRE_MASK("acmi_a2c_loss_masked", legal, A);
  return a2c_loss_launch("acmi_a2c_loss_masked", logits, ld, values, actions, targets, adv, M, A, beta, vcoef,
                         grad_scale, dhead, ldh, ws, loss_out, legal, bad_rows, stream);
}

int64_t acmi_ppo_loss_ws_floats(int M) { return (long long)PPO_SUMS * cdiv(M, LOSS_BLOCK) + 16; }

static int ppo_loss_launch(const char* name, const float* logits, int ld, const float* values,
                           const int32_t* actions, const float* old_logp, const float* old_values,
                           const float* targets, const float* adv, int M, int A, float clip_eps, float vclip,
                           float beta, float vcoef, float grad_scale, float* dhead, int ldh, float* ws,
                           float* loss_out, float* clip_frac_out, const uint32_t* legal, int32_t* bad_rows,
                           acmi_stream_t stream) {
  ACMI_REQUIRE(logits && values && actions && old_logp && targets && adv && dhead && ws &&
                   loss_out && M > 0 && A >= 1 && ld >= A && ldh >= A + 1 && clip_eps > 0.f &&
                   (old_values || !(vclip > 0.f)),
               ACMI_ERR_ARG, "%s: bad arguments", name);
  const int nb = cdiv(M, LOSS_BLOCK);
  hipStream_t s = (hipStream_t)stream;
  const auto kern = legal ? ppo_loss_kernel<true> : ppo_loss_kernel<false>;
  hipLaunchKernelGGL(kern, dim3(nb), dim3(LOSS_BLOCK), 0, s, logits, ld, values, actions, old_logp, old_values,
                     targets, adv, M, A, clip_eps, vclip, beta, vcoef, grad_scale, dhead, ldh, ws, legal, bad_rows);
  hipLaunchKernelGGL(loss_final_kernel<PPO_SUMS>, dim3(1), dim3(64), 0, s, ws, nb, M, beta, grad_scale, loss_out,
                     clip_frac_out);
  ACMI_LAUNCH_CHECK(name);
  return ACMI_OK;
}

int acmi_ppo_loss(const float* logits, int ld, const float* values, const int32_t* actions,
                  const float* old_logp, const float* old_values, const float* targets,
                  const float* adv, int M, int A, float clip_eps, float vclip, float beta,
                  float vcoef, float grad_scale, float* dhead, int ldh, float* ws, float* loss_out,
                  float* clip_frac_out, acmi_stream_t stream) {
  return ppo_loss_launch("acmi_ppo_loss", logits, ld, values, actions, old_logp, old_values, targets, adv, M, A,
                         clip_eps, vclip, beta, vcoef, grad_scale, dhead, ldh, ws, loss_out, clip_frac_out, nullptr,
                         nullptr, stream);
}

int acmi_ppo_loss_masked(const float* logits, int ld, const float* values, const int32_t* actions,
                         const float* old_logp, const float* old_values, const float* targets,
                         const float* adv, int M, int A, float clip_eps, float vclip, float beta,
                         float vcoef, float grad_scale, float* dhead, int ldh, float* ws, float* loss_out,
                         float* clip_frac_out, const uint32_t* legal, int32_t* bad_rows,
                         acmi_stream_t stream) {
  ACMI_REQUIRE_MASK("acmi_ppo_loss_masked", legal, A);
  return ppo_loss_launch("acmi_ppo_loss_masked", logits, ld, values, actions, old_logp, old_values, targets, adv, M,
                         A, clip_eps, vclip, beta, vcoef, grad_scale, dhead, ldh, ws, loss_out, clip_frac_out,
                         legal, bad_rows, stream);
}

int acmi_gather_rows(const uint8_t* obs, int64_t img_stride, int64_t src_rows, const int32_t* index,
                     int64_t rows, uint8_t* obs_out, int64_t out_stride, int nvec,
                     const void* const* vec_src, void* const* vec_dst, int32_t* bad_rows,
                     acmi_stream_t stream) {
  constexpr int64_t kRowBytes = (int64_t)FRAME_WORDS * 16;
  ACMI_REQUIRE(index && rows >= 0 && rows <= INT32_MAX && src_rows >= 0 && nvec >= 0 &&
                   nvec <= GATHER_MAX_VECS && (nvec == 0 || (vec_src && vec_dst)),
               ACMI_ERR_ARG, "acmi_gather_rows: bad arguments");
  GatherVecs vecs = {};
  for (int k = 0; k < nvec; ++k) {
    ACMI_REQUIRE(vec_src[k] && vec_dst[k] && (uintptr_t)vec_src[k] % 4 == 0 && (uintptr_t)vec_dst[k] % 4 == 0,
                 ACMI_ERR_ARG, "acmi_gather_rows: vector %d null or misaligned", k);
    vecs.src[k] = static_cast<const uint32_t*>(vec_src[k]);
    vecs.dst[k] = static_cast<uint32_t*>(vec_dst[k]);
  }
  if (obs)
    ACMI_REQUIRE(obs_out && img_stride >= kRowBytes && out_stride >= kRowBytes && img_stride % 16 == 0 &&
                     out_stride % 16 == 0 && (uintptr_t)obs % 16 == 0 && (uintptr_t)obs_out % 16 == 0,
                 ACMI_ERR_ARG, "acmi_gather_rows: obs, obs_out and the strides (>= %lld) must be 16-byte aligned",
                 (long long)kRowBytes);
  if (rows == 0 || (!obs && nvec == 0)) return ACMI_OK;
  const unsigned grid = obs ? (unsigned)rows : (unsigned)cdiv(rows, GATHER_BLOCK);
  hipLaunchKernelGGL(gather_rows_kernel, dim3(grid), dim3(GATHER_BLOCK), 0, (hipStream_t)stream, obs,
                     (long long)img_stride, (long long)src_rows, index, (long long)rows, obs_out,
                     (long long)out_stride, nvec, vecs, bad_rows);
  ACMI_LAUNCH_CHECK("acmi_gather_rows");
  return ACMI_OK;
}

int64_t acmi_opt_ws_floats(int64_t n) { (void)n; return RED_BLOCKS + 16; }

static int clip_prologue(const float* g, long long n, float clip_norm, float* ws,
                         float* norm_out, hipStream_t s) {
  hipLaunchKernelGGL(dot_partial_kernel, dim3(RED_BLOCKS), dim3(256), 0, s, g, g, n, ws);
  hipLaunchKernelGGL(clip_scale_kernel, dim3(1), dim3(256), 0, s, ws, RED_BLOCKS, clip_norm,
                     ws + RED_BLOCKS, norm_out);
  ACMI_LAUNCH_CHECK("clip_by_global_norm");
  return ACMI_OK;
}

int acmi_momentum_apply(float* params, float* accum, const float* grads, int64_t n, float lr,
                        float momentum, float clip_norm, float* ws, float* norm_out,
                        acmi_stream_t stream) {
  ACMI_REQUIRE(params && accum && grads && ws && n > 0, ACMI_ERR_ARG,
               "acmi_momentum_apply: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  int rc = clip_prologue(grads, n, clip_norm, ws, norm_out, s);
  if (rc) return rc;
  hipLaunchKernelGGL(momentum_kernel, dim3(std::min<long long>(cdiv(n, 256), 2048)), dim3(256),
                     0, s, params, accum, grads, (long long)n, lr, momentum, ws + RED_BLOCKS);
  ACMI_LAUNCH_CHECK("acmi_momentum_apply");
  return ACMI_OK;
}

int acmi_rmsprop_apply(float* params, float* ms, float* mom, const float* grads, int64_t n,
                       float lr, float decay, float momentum, float eps, float clip_norm,
                       float* ws, float* norm_out, acmi_stream_t stream) {
  ACMI_REQUIRE(params && ms && mom && grads && ws && n > 0, ACMI_ERR_ARG,
               "acmi_rmsprop_apply: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  int rc = clip_prologue(grads, n, clip_norm, ws, norm_out, s);
  if (rc) return rc;
  hipLaunchKernelGGL(rmsprop_kernel, dim3(std::min<long long>(cdiv(n, 256), 2048)), dim3(256),
                     0, s, params, ms, mom, grads, (long long)n, lr, decay, momentum, eps,
                     ws + RED_BLOCKS);
  ACMI_LAUNCH_CHECK("acmi_rmsprop_apply");
  return ACMI_OK;
}

int acmi_adam_apply(float* params, float* m, float* v, const float* grads, int64_t n, float lr_t,
                    float beta1, float beta2, float eps, float clip_norm, float* ws,
                    float* norm_out, acmi_stream_t stream) {
  ACMI_REQUIRE(params && m && v && grads && ws && n > 0, ACMI_ERR_ARG,
               "acmi_adam_apply: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  int rc = clip_prologue(grads, n, clip_norm, ws, norm_out, s);
  if (rc) return rc;
  hipLaunchKernelGGL(adam_kernel, dim3(std::min<long long>(cdiv(n, 256), 2048)), dim3(256), 0, s,
                     params, m, v, grads, (long long)n, lr_t, beta1, beta2, eps, ws + RED_BLOCKS);
  ACMI_LAUNCH_CHECK("acmi_adam_apply");
  return ACMI_OK;
}

int acmi_env_reset(const acmi_env_state_t* st, int N, int env_offset, uint32_t seed,
                   uint8_t* obs_out, int64_t out_stride, acmi_stream_t stream) {
  ACMI_REQUIRE(st && obs_out && N >= 0 && out_stride >= 84 * 84 * 4 && out_stride % 16 == 0,
               ACMI_ERR_ARG, "acmi_env_reset: bad arguments");
  if (N == 0) return ACMI_OK;
  hipLaunchKernelGGL(env_reset_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, *st,
                     env_offset, seed, obs_out, (long long)out_stride);
  ACMI_LAUNCH_CHECK("acmi_env_reset");
  return ACMI_OK;
}

int acmi_env_step(const acmi_env_state_t* st, int N, int env_offset, uint32_t seed,
                  const int32_t* actions, const uint8_t* obs_in, int64_t in_stride,
                  uint8_t* obs_out, int64_t out_stride, float* rewards, uint8_t* terminals,
                  float* episode_rewards, int64_t ld, acmi_stream_t stream) {
  ACMI_REQUIRE(st && actions && obs_in && obs_out && rewards && terminals && episode_rewards &&
                   N >= 0 && in_stride % 16 == 0 && out_stride % 16 == 0 && ld >= 1,
               ACMI_ERR_ARG, "acmi_env_step: bad arguments");
  if (N == 0) return ACMI_OK;
  hipLaunchKernelGGL(env_step_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, *st,
                     env_offset, seed, actions, obs_in, (long long)in_stride, obs_out,
                     (long long)out_stride, rewards, terminals, episode_rewards,
                     (long long)ld);
  ACMI_LAUNCH_CHECK("acmi_env_step");
  return ACMI_OK;
}

}  // extern "C"
