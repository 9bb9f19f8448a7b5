// Update diagnostics (an option beyond the reference): what one parameter
// update did, as per-group double accumulators a log line reads with one copy.
// include/acmi.h states the semantics; actorcritic/update_diag.py restates them
// in numpy.  Every sum is a double sum in an order fixed by the arguments alone
// (partials in a workspace, one reducing kernel, the wave butterfly; the only
// atomics are the integer counters bad_envs / bad_rows): same bytes in, same
// bytes out.  Nothing here is on the step path: the calls run on logging
// updates, over M*A <= 10240*64 logits and the 0.87 M parameters.
//
//   acmi_diag_value     diag_value_envs_kernel    one thread per env: its T rows
//                                                 ascending, 5 sums into ws[n][5]
//                       diag_value_groups_kernel  one wave per group: the envs
//                                                 lane-strided, ascending, then
//                                                 the butterfly
//   acmi_diag_policy    diag_policy_rows_kernel   one thread per row: KL and H in
//                                                 double into ws[m][3]
//                       diag_policy_groups_kernel one wave per group, as above,
//                                                 over each env's T rows
//   acmi_diag_segments  diag_seg_parts_kernel     block (k, s): slice k of the 64
//                                                 slices of segment s (the slice
//                                                 length follows from the offsets
//                                                 alone) into ws[s][k][4]
//                       diag_seg_final_kernel     one wave per segment: lane k
//                                                 takes slice k, the butterfly
#include <limits.h>
#include <math.h>

#include "common.hpp"

namespace acmi {

constexpr int DIAG_MAX_GROUPS = 64;
constexpr int DIAG_BLOCK = 256;
constexpr int DIAG_VALUE_PART = 5;   // sum v, sum y, sum y^2, sum e, sum e^2
constexpr int DIAG_POLICY_PART = 3;  // counted (1 or 0), KL, H
constexpr int DIAG_SEG_SLICES = 64;  // slices of a segment = lanes of the final wave
constexpr int DIAG_SEG_MAX = 65535;  // (the grid's y extent)

__device__ __forceinline__ int diag_group(const uint8_t* groups, int n) { return groups != nullptr ? groups[n] : 0; }

__global__ void diag_value_envs_kernel(const float* v, const float* y, const uint8_t* groups, int N, int T, int G,
                                       double* part, int32_t* bad_envs) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  double sv = 0.0, sy = 0.0, qy = 0.0, se = 0.0, qe = 0.0;
  for (int t = 0; t < T; ++t) {
    const long long i = (long long)n * T + t;
    const double vd = v[i], yd = y[i];
    const double e = yd - vd;
    sv += vd;
    sy += yd;
    qy += yd * yd;            // (exact in double: a fused multiply-add rounds the same sum)
    se += e;
    qe += __dmul_rn(e, e);    // (not exact: the product is rounded, then added, as numpy does)
  }
  double* p = part + (long long)DIAG_VALUE_PART * n;
  p[0] = sv, p[1] = sy, p[2] = qy, p[3] = se, p[4] = qe;
  if (diag_group(groups, n) >= G && bad_envs != nullptr) atomicAdd(bad_envs, 1);
}

__global__ void diag_value_groups_kernel(const double* part, const uint8_t* groups, int N, int T, double* acc) {
  const int g = blockIdx.x;  // one wave per group
  double c = 0.0, s[DIAG_VALUE_PART];
#pragma unroll
  for (int k = 0; k < DIAG_VALUE_PART; ++k) s[k] = 0.0;
  for (int n = threadIdx.x; n < N; n += 64) {
    if (diag_group(groups, n) == g) {
      const double* p = part + (long long)DIAG_VALUE_PART * n;
      c += 1.0;
#pragma unroll
      for (int k = 0; k < DIAG_VALUE_PART; ++k) s[k] += p[k];
    }
  }
  c = wave_sum_d(c);
#pragma unroll
  for (int k = 0; k < DIAG_VALUE_PART; ++k) s[k] = wave_sum_d(s[k]);
  if (threadIdx.x == 0) {
    double* a = acc + 6 * g;
    a[0] = c * (double)T;
#pragma unroll
    for (int k = 0; k < DIAG_VALUE_PART; ++k) a[1 + k] = s[k];
  }
}

// One row of one matrix over the legal set S (bit a of word; all of 0..A-1 without
// masks): -> false when S is empty or ANY of the A logits is non-finite; else mx, lse.
__device__ __forceinline__ bool diag_row_lse(const float* z, int A, uint32_t word, double& lse) {
  bool finite = true;
  double mx = -INFINITY;
  for (int a = 0; a < A; ++a) {
    const float x = z[a];
    finite = finite && ((__float_as_uint(x) & 0x7f800000u) != 0x7f800000u);
    if (A > 32 || ((word >> a) & 1u)) mx = fmax(mx, (double)x);
  }
  if (!finite || mx == -INFINITY) return false;  // (finite logits: the maximum is -inf only over an empty set)
  double sum = 0.0;
  for (int a = 0; a < A; ++a)
    if (A > 32 || ((word >> a) & 1u)) sum += exp((double)z[a] - mx);
  lse = mx + log(sum);
  return true;
}

__global__ void diag_policy_rows_kernel(const float* zo, int ldo, const float* zn, int ldn, const uint32_t* legal,
                                        const uint8_t* groups, int M, int T, int A, int G, double* rows,
                                        int32_t* bad_envs, int32_t* bad_rows) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= M) return;
  const uint32_t all = A >= 32 ? 0xffffffffu : ((1u << A) - 1u);
  const uint32_t word = legal != nullptr ? (legal[m] & all) : all;
  const float* po = zo + (long long)m * ldo;
  const float* pn = zn + (long long)m * ldn;
  double lo = 0.0, ln = 0.0;
  const bool ok_o = diag_row_lse(po, A, word, lo);  // (both are evaluated: no short cut in the reads)
  const bool ok_n = diag_row_lse(pn, A, word, ln);
  const bool ok = ok_o && ok_n;
  double kl = 0.0, h = 0.0;
  if (ok) {
    for (int a = 0; a < A; ++a) {
      if (A > 32 || ((word >> a) & 1u)) {
        const double lpo = (double)po[a] - lo, lpn = (double)pn[a] - ln;
        kl += __dmul_rn(exp(lpo), lpo - lpn);
        h -= __dmul_rn(exp(lpn), lpn);
      }
    }
  }
  double* r = rows + (long long)DIAG_POLICY_PART * m;
  r[0] = ok ? 1.0 : 0.0, r[1] = kl, r[2] = h;
  if (!ok && bad_rows != nullptr) atomicAdd(bad_rows, 1);
  if (m % T == 0 && bad_envs != nullptr && diag_group(groups, m / T) >= G) atomicAdd(bad_envs, 1);
}

__global__ void diag_policy_groups_kernel(const double* rows, const uint8_t* groups, int N, int T, double* acc) {
  const int g = blockIdx.x;  // one wave per group
  double c = 0.0, skl = 0.0, sh = 0.0, mkl = -INFINITY;
  for (int n = threadIdx.x; n < N; n += 64) {
    if (diag_group(groups, n) == g) {
      for (int t = 0; t < T; ++t) {
        const double* r = rows + DIAG_POLICY_PART * ((long long)n * T + t);
        if (r[0] != 0.0) {
          c += 1.0;
          skl += r[1];
          sh += r[2];
          mkl = fmax(mkl, r[1]);
        }
      }
    }
  }
  c = wave_sum_d(c), skl = wave_sum_d(skl), sh = wave_sum_d(sh), mkl = wave_max_d(mkl);
  if (threadIdx.x == 0) {
    double* a = acc + 4 * g;
    a[0] = c, a[1] = skl, a[2] = sh, a[3] = mkl;
  }
}

// Slice k of segment [lo, hi): elements lo + k*len .. lo + (k+1)*len - 1 (cut at hi) with
// len = ceil((hi - lo) / 64) rounded up to a multiple of the block: a function of the
// offsets alone.  The block's threads stride the slice, then wave butterfly + 4 waves in LDS.
__global__ void __launch_bounds__(DIAG_BLOCK)
    diag_seg_parts_kernel(const float* x, const float* y, const int64_t* offsets, double* part) {
  __shared__ double sh[DIAG_BLOCK / 64][4];
  const int k = blockIdx.x, s = blockIdx.y;
  const long long lo = offsets[s], hi = offsets[s + 1];
  long long len = (hi - lo + DIAG_SEG_SLICES - 1) / DIAG_SEG_SLICES;
  len = (len + DIAG_BLOCK - 1) / DIAG_BLOCK * DIAG_BLOCK;
  const long long b = lo + (long long)k * len;
  const long long e = b + len < hi ? b + len : hi;
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  for (long long i = b + threadIdx.x; i < e; i += DIAG_BLOCK) {
    const double xd = x[i], yd = y != nullptr ? (double)y[i] : 0.0;
    const double d = xd - yd;
    v[0] += xd * xd;  // (products of two floats: exact in double)
    v[1] += yd * yd;
    v[2] += xd * yd;
    v[3] += __dmul_rn(d, d);
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) v[c] = wave_sum_d(v[c]);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int c = 0; c < 4; ++c) sh[w][c] = v[c];
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    double t = sh[0][threadIdx.x];
#pragma unroll
    for (int ww = 1; ww < DIAG_BLOCK / 64; ++ww) t += sh[ww][threadIdx.x];
    part[((long long)s * DIAG_SEG_SLICES + k) * 4 + threadIdx.x] = t;
  }
}

__global__ void diag_seg_final_kernel(const double* part, double* out) {
  const int s = blockIdx.x;  // one wave per segment, lane k holds slice k
  const double* p = part + ((long long)s * DIAG_SEG_SLICES + threadIdx.x) * 4;
  double v[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) v[c] = wave_sum_d(p[c]);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int c = 0; c < 4; ++c) out[4LL * s + c] = v[c];
  }
}

}  // namespace acmi

using namespace acmi;

extern "C" {

int64_t acmi_diag_ws_doubles(int64_t M, int64_t S) {
  const int64_t rows = M < 1 ? 0 : DIAG_VALUE_PART * M;  // (N <= M: the value partials; 3 M: the policy rows)
  const int64_t segs = S < 1 ? 0 : (int64_t)DIAG_SEG_SLICES * 4 * S;
  return rows > segs ? rows : segs;
}

int acmi_diag_value(const float* values, const float* targets, const uint8_t* groups, int N, int T, int G, double* ws,
                    double* acc, int32_t* bad_envs, acmi_stream_t stream) {
  ACMI_REQUIRE(values != nullptr && targets != nullptr && ws != nullptr && acc != nullptr, ACMI_ERR_ARG,
               "acmi_diag_value: a required pointer is NULL");
  ACMI_REQUIRE(N >= 1 && T >= 1 && (long long)N * T <= INT_MAX && G >= 1 && G <= DIAG_MAX_GROUPS, ACMI_ERR_ARG,
               "acmi_diag_value: N=%d, T=%d must be at least 1 (N*T below 2^31) and G=%d in 1..%d", N, T, G,
               DIAG_MAX_GROUPS);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(diag_value_envs_kernel, dim3(cdiv(N, DIAG_BLOCK)), dim3(DIAG_BLOCK), 0, s, values, targets,
                     groups, N, T, G, ws, bad_envs);
  hipLaunchKernelGGL(diag_value_groups_kernel, dim3(G), dim3(64), 0, s, ws, groups, N, T, acc);
  ACMI_LAUNCH_CHECK("acmi_diag_value");
  return ACMI_OK;
}

int acmi_diag_policy(const float* logits_old, int ld_old, const float* logits_new, int ld_new, const uint32_t* legal,
                     const uint8_t* groups, int N, int T, int A, int G, double* ws, double* acc, int32_t* bad_envs,
                     int32_t* bad_rows, acmi_stream_t stream) {
  ACMI_REQUIRE(logits_old != nullptr && logits_new != nullptr && ws != nullptr && acc != nullptr, ACMI_ERR_ARG,
               "acmi_diag_policy: a required pointer is NULL");
  ACMI_REQUIRE(N >= 1 && T >= 1 && (long long)N * T <= INT_MAX && G >= 1 && G <= DIAG_MAX_GROUPS, ACMI_ERR_ARG,
               "acmi_diag_policy: N=%d, T=%d must be at least 1 (N*T below 2^31) and G=%d in 1..%d", N, T, G,
               DIAG_MAX_GROUPS);
  ACMI_REQUIRE(A >= 1 && A <= (legal != nullptr ? 32 : 64), ACMI_ERR_ARG,
               "acmi_diag_policy: num_actions=%d outside 1..%d%s", A, legal != nullptr ? 32 : 64,
               legal != nullptr ? " (a legal-action mask holds at most 32)" : "");
  ACMI_REQUIRE(ld_old >= A && ld_new >= A, ACMI_ERR_ARG, "acmi_diag_policy: ld_old=%d, ld_new=%d below num_actions=%d",
               ld_old, ld_new, A);
  hipStream_t s = (hipStream_t)stream;
  const int M = N * T;
  hipLaunchKernelGGL(diag_policy_rows_kernel, dim3(cdiv(M, DIAG_BLOCK)), dim3(DIAG_BLOCK), 0, s, logits_old, ld_old,
                     logits_new, ld_new, legal, groups, M, T, A, G, ws, bad_envs, bad_rows);
  hipLaunchKernelGGL(diag_policy_groups_kernel, dim3(G), dim3(64), 0, s, ws, groups, N, T, acc);
  ACMI_LAUNCH_CHECK("acmi_diag_policy");
  return ACMI_OK;
}

int acmi_diag_segments(const float* x, const float* y, const int64_t* offsets, int S, double* ws, double* out,
                       acmi_stream_t stream) {
  ACMI_REQUIRE(x != nullptr && offsets != nullptr && ws != nullptr && out != nullptr, ACMI_ERR_ARG,
               "acmi_diag_segments: a required pointer is NULL");
  ACMI_REQUIRE(S >= 1 && S <= DIAG_SEG_MAX, ACMI_ERR_ARG, "acmi_diag_segments: S=%d outside 1..%d", S, DIAG_SEG_MAX);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(diag_seg_parts_kernel, dim3(DIAG_SEG_SLICES, S), dim3(DIAG_BLOCK), 0, s, x, y, offsets, ws);
  hipLaunchKernelGGL(diag_seg_final_kernel, dim3(S), dim3(64), 0, s, ws, out);
  ACMI_LAUNCH_CHECK("acmi_diag_segments");
  return ACMI_OK;
}

}  // extern "C"
