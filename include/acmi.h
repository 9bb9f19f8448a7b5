/*
 * acmi.h — C-ABI of libacmi, the MI355X-native (gfx950) A2C/ACKTR hot path.
 *
 * Drop-in boundary for the reference's TF graph + kfac ops on the rollout and
 * update path of jrobine/actor-critic.  Every entry point
 *   - takes caller-owned DEVICE buffers (plain pointers, sizes, no torch types),
 *   - is stream-ordered on `stream` (a hipStream_t), asynchronous, never
 *     allocates and never synchronises (so a caller may capture it in a graph),
 *   - returns 0 (ACMI_OK) or a negative ACMI_ERR_* code; the message is in
 *     acmi_last_error() (thread-local).
 *
 * Reference interface each entry point replaces is cited as path:line into
 * /root/reference.  Layouts: NHWC u8 observations,
 * HWIO conv weights, [in,out] FC weights (reference nn.py:8-84), fp32 math.
 */
#ifndef ACMI_H_
#define ACMI_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ACMI_ABI_VERSION 4  /* 3: acmi_env_state_t.game, acmi_rollout_io_t step fusion fields;
                               4: ws_floats on acmi_backward / acmi_kfac_output_stats, per-net
                                  mode fields in acmi_net_t */

enum {
  ACMI_OK = 0,
  ACMI_ERR_ARG = -1,   /* bad shape / null pointer / unsupported size   */
  ACMI_ERR_HIP = -2,   /* a HIP launch failed                             */
  ACMI_ERR_WS = -3,    /* caller workspace too small                      */
};

typedef void* acmi_stream_t; /* hipStream_t */

const char* acmi_last_error(void);
int acmi_abi_version(void);
/* Host-only: sizeof of the ABI structs, in the order acmi_net_t, acmi_acts_t,
 * acmi_bwd_t, acmi_env_state_t, acmi_rollout_io_t (n <= 5 written), so a
 * binding can check its struct mirrors (returns the number written). */
int acmi_abi_struct_sizes(int64_t* sizes, int n);

/* Arithmetic of the fused weight-gradient + K-FAC A-factor reductions (conv2,
 * conv3, heads; the dominant K-FAC covariance work, kfac cov_update_thunks,
 * actorcritic/kfac_utils.py:39,44).  Both modes are fp32-accurate:
 *   ACMI_GEMM_X3  16-bit split operands on the 16-bit matrix cores (default):
 *                 f16x2 (two f16 parts, 3 MFMAs, power-of-two scales from
 *                 published maxima) for the conv tower, the dX chain, the band
 *                 and fc4 reductions; bf16x3 (6 MFMAs) for the small rest
 *   ACMI_GEMM_F32 v_mfma_f32_32x32x2_f32
 * Initial mode from the environment variable ACMI_GEMM ("x3" / "f32").
 * The acmi_set_*_mode functions set the PROCESS DEFAULT, which nets with a
 * zero mode field use; a net's own field overrides it (acmi_net_t).
 * Not stream-ordered: set it between launches. */
#define ACMI_GEMM_F32 0
#define ACMI_GEMM_X3 1
int acmi_set_gemm_mode(int mode);
int acmi_get_gemm_mode(void);

/* Precision of the forward's conv tower (rollout and update forward; BASELINE
 * configs[4] "bf16 forward / fp32 K-FAC factors" -- an extension, the
 * reference computes in fp32):
 *   ACMI_FWD_F32   f16x2 split operands (scaled f16 h + l, three MFMAs per
 *                  product), f32-accurate (default)
 *   ACMI_FWD_BF16  one 16-bit MFMA per product: weights and conv2/conv3 inputs
 *                  scaled by powers of two and rounded once to f16 (u8 pixels
 *                  exact), f32 accumulation.  The error bound is RELATIVE TO
 *                  EACH TENSOR'S RANGE: elements within 2^-14 of their tensor's
 *                  bound keep 11-bit significands (finer than bf16's 8), but
 *                  f16's exponent range is narrower than bf16's -- elements
 *                  below ~2^-28 of the bound become f16 subnormals and below
 *                  ~2^-38 flush to zero, where bf16 would keep them.  The
 *                  bounds are weight-derived (loose), which widens that margin;
 *                  the tests check error against each tensor's range
 * The backward, the K-FAC statistics and the optimizers stay f32-accurate; they
 * read the activations the forward produced.  Initial mode from ACMI_FORWARD
 * ("bf16" / "f32").  Not stream-ordered: set it between launches.
 * The 16-bit arithmetic lives in the fused conv tower only: setting
 * ACMI_FWD_BF16 fails (ACMI_ERR_ARG) in ACMI_GEMM_F32 mode, and a forward in
 * that mode fails without net->conv_prep or on observations / an image stride
 * that are not 16-byte aligned -- the mode is never silently ignored. */
#define ACMI_FWD_F32 0
#define ACMI_FWD_BF16 1
int acmi_set_forward_mode(int mode);
int acmi_get_forward_mode(void);

/* How conv2 / conv3 form their weight gradient + A factor in ACMI_GEMM_X3 mode
 * (both fp32-accurate, same sums reassociated):
 *   ACMI_CONV_STATS_BAND    pixel-pair band reduction (default): each pair of
 *                           input pixels sharing a patch is multiplied once over
 *                           the images' dense activation rows, the patch sums
 *                           folded afterwards (2.5x / 1.6x fewer MACs for conv3 /
 *                           conv2 than patch rows, no im2col gather)
 *   ACMI_CONV_STATS_PATCHES [P;1]^T [P | dY] over the im2col patch rows
 * Initial mode from ACMI_BAND ("0" = patches).  The band plans (sub-tile
 * groups, fold tables) are built on the first backward of each device and
 * kept for the process: that first acmi_backward allocates and synchronises
 * once (do not capture it in a graph).  Not stream-ordered. */
#define ACMI_CONV_STATS_PATCHES 0
#define ACMI_CONV_STATS_BAND 1
int acmi_set_conv_stats_mode(int mode);
int acmi_get_conv_stats_mode(void);
/* plan facts of the band reduction of conv2 (layer 1) or conv3 (layer 2) at
 * `rows` images: info[0] sub-tiles, [1] groups (blocks per chunk), [2] chunks,
 * [3] rows per chunk, [4] sum over groups of the busiest SIMD's sub-tiles */
int acmi_band_info(int layer, int C3, int64_t rows, int64_t* info);

/* ------------------------------------------------------------------------
 * Model layout.  Replaces AtariModel._build_params
 * (actorcritic/envs/atari/model.py:129-170, nn.py:8-84).
 * The flat fp32 parameter vector holds, in order:
 *   conv1.W[8][8][4][32] conv1.b[32] conv2.W[4][4][32][64] conv2.b[64]
 *   conv3.W[3][3][64][C3] conv3.b[C3] fc4.W[49*C3][512] fc4.b[512]
 *   pi.W[512][A] pi.b[A] v.W[512][1] v.b[1]
 * so each layer's homogeneous weight matrix [W; b] ((K+1) x Cout, the K-FAC
 * block of envs/atari/model.py:219-246) is one contiguous row-major slice.
 * ---------------------------------------------------------------------- */
#define ACMI_NUM_LAYERS 6   /* conv1 conv2 conv3 fc4 fc_policy fc_baseline */
#define ACMI_NUM_AFACT 5    /* fc_policy and fc_baseline share one A factor */
#define ACMI_NUM_GFACT 6

typedef struct acmi_net {
  int num_actions;     /* A  (Breakout 4, full Atari 18); 1 <= A <= 64    */
  int conv3_filters;   /* C3 (32 ACKTR, 64 A2C: a2c_acktr.py:51-53)       */
  const float* params; /* device, acmi_param_count() floats               */
  const void* conv_prep; /* nullable: device, acmi_conv_prep_bytes(C3) bytes,
                            filled by acmi_conv_prepare from THESE params (the
                            caller re-prepares after every parameter change) */
  /* This net's arithmetic, each the mode + 1 (ACMI_GEMM_*, ACMI_FWD_*,
   * ACMI_CONV_STATS_*); 0 = the process default (acmi_set_*_mode).  Every
   * entry point taking a net runs in its net's modes (held per calling thread
   * for the call), so two nets in one process, or two threads, never see each
   * other's settings; an invalid combination fails with ACMI_ERR_ARG. */
  int gemm_mode;
  int forward_mode;
  int conv_stats_mode;
} acmi_net_t;

/* The forward's fused conv tower (x3 gemm mode), fc4 at rollout batches
 * (split-K slabs with a forward workspace) and the backward's conv2 input
 * gradient (acmi_backward, acmi_kfac_output_stats) read their weights as
 * pre-split f16x2 MFMA fragments -- scaled f16 (h, l) pairs, with a header of
 * power-of-two scale bounds (max |W| per layer, weight-derived activation
 * bounds) -- when net->conv_prep is set: acmi_conv_prepare writes them
 * (stream-ordered, a few small kernels) -- once per parameter version, not per
 * rollout step or update.  With conv_prep == NULL the forward runs the
 * per-layer conv kernels and fc4 / the conv2 input gradient the generic
 * split-per-block bf16x3 GEMM: f32-class like the prepared path, not
 * bit-identical to it (the sampled-loss chain then stores its conv1-output
 * gradient and reduces its G factor separately); the 16-bit forward
 * (ACMI_FWD_BF16) needs conv_prep. */
int64_t acmi_conv_prep_bytes(int conv3_filters);
int acmi_conv_prepare(const acmi_net_t* net, void* conv_prep, acmi_stream_t stream);

int64_t acmi_param_count(int num_actions, int conv3_filters);
/* off[2*l] = W offset, off[2*l+1] = b offset of layer l (12 entries)       */
int acmi_param_offsets(int num_actions, int conv3_filters, int64_t* off12);

/* K-FAC block geometry: din[l] = K_l + 1 (homogeneous), dout[l] = Cout_l.
 * stat_off[0..4] = offsets of A factors (din^2 each, A4 shared by l=4,5),
 * stat_off[5..10] = offsets of G factors (dout^2), *total = floats overall. */
int acmi_kfac_layout(int num_actions, int conv3_filters, int64_t* din6,
                     int64_t* dout6, int64_t* stat_off11, int64_t* total);

/* ------------------------------------------------------------------------
 * Forward.  Replaces the TF graph of AtariModel.__init__/_build_layers
 * (envs/atari/model.py:77-217): u8/255 normalise (:92-95), conv1 8x8 s4,
 * conv2 4x4 s2, conv3 3x3 s1 (VALID, +bias, ReLU), NHWC flatten, fc4 512
 * ReLU, policy logits and value heads.  `obs` holds B NHWC u8 images
 * [84][84][4]; image b starts at obs + b*img_stride (bytes), which lets the
 * rollout read step t of a [N][T][84][84][4] buffer in place.
 *
 * Addressing (acmi_forward, acmi_forward_strided; every violation is
 * ACMI_ERR_ARG before anything is enqueued):
 *   - img_stride >= 28224, obs and img_stride multiples of 4 (the per-layer
 *     conv1 loads a pixel's 4 channels as one uint32);
 *   - the fused conv tower (net->conv_prep, ACMI_GEMM_X3) loads 16 bytes: it
 *     runs only when obs and img_stride are multiples of 16, the per-layer
 *     kernels otherwise (f32-class either way, not bit-identical to each
 *     other).  ACMI_FWD_BF16 exists only in the tower and is refused otherwise;
 *   - ld_logits >= num_actions (columns past num_actions are not written),
 *     value non-NULL unless want_value == 0 (then it is not written);
 *   - 32-bit offsets: (B - 1) * img_stride + 28224 < 2^31 and
 *     (B - 1) * act_img_stride * 12800 + 12800 < 2^31 (a1's floats);
 *   - B == 0 is ACMI_OK and writes nothing.
 * ---------------------------------------------------------------------- */
typedef struct acmi_acts {
  float* a1;     /* [B][20][20][32] post-ReLU                               */
  float* a2;     /* [B][9][9][64]                                           */
  float* a3;     /* [B][7][7][C3]  (= the NHWC-flattened fc4 input)         */
  float* a4;     /* [B][512]                                                */
  float* logits; /* [B][ld_logits]                                          */
  float* value;  /* [B]  (may be NULL when want_value == 0)                 */
  int ld_logits;
  float* ws;     /* optional split-K workspace (NULL: no split), floats:  */
  int64_t ws_floats; /* >= acmi_forward_ws_floats(B) enables it            */
  /* optional ReLU' bit masks of a1..a3 (all three or none; NULL: none): bit e
   * of word e / 32 = (a[e] > 0), i.e. one word per 32 channels of a pixel --
   * m1 [B][400], m2 [B][81][2], m3 [B][49][C3/32] uint32.  acmi_forward writes
   * them beside the activations (same image stride); acmi_backward and
   * acmi_kfac_output_stats then mask the input gradients from them instead of
   * re-reading the f32 activations (1/32 of the bytes; results bit-identical). */
  uint32_t* m1;
  uint32_t* m2;
  uint32_t* m3;
} acmi_acts_t;

int64_t acmi_forward_ws_floats(int B);

int acmi_forward(const acmi_net_t* net, const uint8_t* obs, int64_t img_stride,
                 int B, const acmi_acts_t* acts, int want_value,
                 acmi_stream_t stream);

/* ------------------------------------------------------------------------
 * Categorical sampling.  Replaces Categorical.sample (tf.multinomial) and
 * the squeeze of policies.py:86, model.py:135-151.  Counter-based RNG:
 * u = u01(key4(seed, stream_id, counter, row)); when `uniforms` is non-NULL
 * it supplies u[row] instead (parity tests).  Inverse-CDF over softmax in
 * f32.  A row with a NaN/inf logit yields action -1 and sets *bad_rows
 * (device int, accumulated) — the reference would instead emit index A and
 * fail later in sparse_softmax_cross_entropy (README.md:53-54).
 * mode != 0 -> argmax (Categorical.mode, model.py:153-169).
 * ---------------------------------------------------------------------- */
int acmi_sample_actions(const float* logits, int ld, int B, int A,
                        uint32_t seed, uint32_t stream_id, uint32_t counter,
                        const float* uniforms, int mode, int32_t* actions,
                        int32_t* bad_rows, acmi_stream_t stream);
/* The same for rows row_offset .. row_offset+B-1 of a larger batch (the RNG
 * key uses the global row): a batch sampled in pieces (the rollout's env
 * halves on two streams) draws exactly the actions of one launch. */
int acmi_sample_actions_at(const float* logits, int ld, int B, int A,
                           uint32_t seed, uint32_t stream_id, uint32_t counter,
                           int row_offset, const float* uniforms, int mode,
                           int32_t* actions, int32_t* bad_rows,
                           acmi_stream_t stream);
/* counter = *counter_dev + counter_add (counter_dev: device uint32, nullable):
 * a rollout captured once in a hipGraph and replayed reads its RNG counter
 * from device memory, the host refreshing it before each replay. */
int acmi_sample_actions_dev(const float* logits, int ld, int B, int A,
                            uint32_t seed, uint32_t stream_id,
                            const uint32_t* counter_dev, uint32_t counter_add,
                            int row_offset, const float* uniforms, int mode,
                            int32_t* actions, int32_t* bad_rows,
                            acmi_stream_t stream);

/* Per-row Categorical.entropy and log_prob(actions) (policies.py:87-89);
 * either output may be NULL (log_prob needs actions). */
int acmi_categorical(const float* logits, int ld, int B, int A,
                     const int32_t* actions, float* entropy, float* log_prob,
                     acmi_stream_t stream);

/* ------------------------------------------------------------------------
 * n-step targets and advantage.  Replaces objectives.py:123-130 with the
 * py_func closures _discount (:178-202) and _discount_bootstrap (:205-214).
 * Batch-major [N][T].  gamma_pow[k] = f32(gamma)**f32(k) (numpy float32
 * power, exactly the D-matrix entries of objectives.py:183-187), k < T;
 * boot_pow[k] = k-fold sequential f32 product of f32(gamma) (the float32
 * cumprod of objectives.py:211), k <= T.  Both tables are host-computed.
 * target[n,t] = sum_{i=t..stop} r[n,i]*gamma_pow[i-t] (ascending i, no FMA,
 *              stop = first terminal >= t)  +  boot_pow[T-t]*v_boot[n] (if no
 *              terminal in t..T-1);   adv = target - value.
 * ---------------------------------------------------------------------- */
int acmi_returns(const float* rewards, const uint8_t* terminals,
                 const float* values, const float* v_boot, int N, int T,
                 const float* gamma_pow, const float* boot_pow, float* targets,
                 float* adv, acmi_stream_t stream);

/* GAE(lambda) targets and advantages -- an option BEYOND the reference (whose
 * A2CObjective uses the n-step targets of acmi_returns, objectives.py:123-130;
 * BASELINE.json north_star names the GAE scan).  Batch-major [N][T], v_boot[N]
 * = V(s_T).  delta_t = r_t + gamma*V_{t+1}*(1-d_t) - V_t (V_T = v_boot),
 * A_t = delta_t + gamma*lambda*(1-d_t)*A_{t+1}, target_t = A_t + V_t; float32,
 * no contraction, in exactly that order.  lambda = 1 gives the n-step targets
 * in exact arithmetic.  0 <= lambda <= 1. */
int acmi_gae(const float* rewards, const uint8_t* terminals, const float* values,
             const float* v_boot, int N, int T, float gamma, float lambda,
             float* targets, float* adv, acmi_stream_t stream);

/* Truncation-aware targets (time limits, Pardo et al. 2018): acmi_returns and
 * acmi_gae plus truncated [N][T] u8, read only where terminals is set.  A
 * truncated terminal still cuts the return, but keeps its bootstrap from the
 * value of the next observation, which with lazy auto-reset is already in the
 * batch: V_{t+1} = values[n][t+1], or v_boot[n] at t = T-1.
 *   GAE:    live = d_t == 0, boot = live || trunc_t,
 *           delta_t = (r_t + (boot ? gamma*V_{t+1} : 0)) - V_t,
 *           A_t = delta_t + (live ? gamma*lambda*A_{t+1} : 0), target = A_t + V_t;
 *   n-step: stop as acmi_returns; the bootstrap term is
 *           boot_pow[stop+1-t]*V_{stop+1} when stop is a truncated terminal,
 *           boot_pow[T-t]*v_boot when there is no terminal, else 0.
 * float32, no contraction, in that order; truncated all zero: the bytes of
 * acmi_returns / acmi_gae (one kernel body each). */
int acmi_returns_trunc(const float* rewards, const uint8_t* terminals,
                       const uint8_t* truncated, const float* values,
                       const float* v_boot, int N, int T, const float* gamma_pow,
                       const float* boot_pow, float* targets, float* adv,
                       acmi_stream_t stream);
int acmi_gae_trunc(const float* rewards, const uint8_t* terminals,
                   const uint8_t* truncated, const float* values, const float* v_boot,
                   int N, int T, float gamma, float lambda, float* targets,
                   float* adv, acmi_stream_t stream);

/* V-trace targets and advantages (Espeholt et al. 2018, IMPALA) -- beyond the
 * reference: acmi_gae_trunc's scan with clipped importance weights, for data
 * that the policy being updated did not collect (several passes over a batch,
 * lagging actors).  One launch; batch-major [N][T] rows m = n*T + t.
 *   logits [N*T][ld], actions: the CURRENT policy and the taken actions;
 *   behaviour_logp[N*T]: log mu(a) of the policy that acted;
 *   truncated: nullable (NULL: every terminal cuts the bootstrap);
 *   legal, bad_rows: nullable, as the *_masked entry points take them (A <= 32
 *   with legal; log pi of an action outside the row's set is -INFINITY and the
 *   row counts in *bad_rows).
 * Per row, f32: logp = acmi_categorical's log_prob (the same statements, the
 * same bits), D = logp - behaviour_logp, w = expf(D),
 *   rho = min(rho_bar, w), c = min(c_bar, w);
 *   D = +inf: the bars; D = -inf: 0; D a NaN (both log-probabilities -inf):
 *   rho = c = 0 -- the row contributes nothing.
 * Per env, in reverse, with vs_T = V_T = v_boot, live = d_t == 0,
 * boot = live || truncated_t (the chain is cut at every terminal):
 *   delta_t = rho_t * ((r_t + (boot ? gamma*V_{t+1} : 0)) - V_t)
 *   acc_t   = delta_t + (live ? ((gamma*lambda) * c_t) * acc_{t+1} : 0)
 *   targets = vs_t = acc_t + V_t
 *   nextv   = live ? vs_{t+1} : (truncated_t ? V_{t+1} : 0)
 *   adv_t   = rho_t * ((r_t + gamma*nextv) - V_t)
 * float32, no contraction, in exactly that order (actorcritic/vtrace.py
 * restates it); gamma*lambda is formed as acmi_gae forms it, so rho = c = 1
 * (behaviour_logp = logp, bars >= 1) gives the bytes of acmi_gae /
 * acmi_gae_trunc's targets.  Outputs: targets, adv, rho (the clipped rho),
 * each [N*T], and log_prob (nullable) = logp.  0 <= lambda <= 1, c_bar > 0,
 * rho_bar >= c_bar, N, T >= 0 (N*T == 0: ACMI_OK, nothing enqueued). */
int acmi_vtrace(const float* logits, int ld, int A, const int32_t* actions,
                const float* behaviour_logp, const float* rewards,
                const uint8_t* terminals, const uint8_t* truncated,
                const float* values, const float* v_boot, int N, int T, float gamma,
                float lambda, float rho_bar, float c_bar, const uint32_t* legal,
                int32_t* bad_rows, float* targets, float* adv, float* rho,
                float* log_prob, acmi_stream_t stream);

/* Advantage normalisation (an option beyond the reference, which has none,
 * objectives.py:128-130): moments[0..1] = (sum, sum of squares) of adv[0..M)
 * in double, fixed order (ws: acmi_adv_moments_ws_doubles(M) doubles).  A
 * data-parallel caller sums the moments over ranks, then
 * acmi_adv_normalize: adv = (adv - mean) / (std + eps), mean/std (population)
 * from moments over `count` rows (the global batch). */
int64_t acmi_adv_moments_ws_doubles(int64_t M);
int acmi_adv_moments(const float* adv, int64_t M, double* ws, double* moments,
                     acmi_stream_t stream);
int acmi_adv_normalize(float* adv, int64_t M, const double* moments, double count,
                       double eps, acmi_stream_t stream);

/* Reward scaling by the running standard deviation of the discounted return,
 * one set of statistics per group of envs (per game); an option beyond the
 * reference (baselines' VecNormalize(ret=True)).  State across updates:
 * carry[N] f32 (each env's running return, starts 0), stats[G][3] f64 (count,
 * mean, M2 per group, starts 0), groups[N] u8; G in 1..64.  Per update, over
 * rewards[N][T] f32 and terminals[N][T] u8 (a truncation is a terminal here):
 *   scan    per env, ascending t, float32, no contraction: R = R*gamma,
 *           R = R + r[n][t]; that R is the sample u[n][t]; a terminal sets
 *           R = 0 after the sample; carry[n] = R at the end.
 *   moments[g] = (c, s, q): the number of samples of group g's envs (N_g*T),
 *           sum u and sum u^2, each u converted to double and summed in
 *           double in a fixed order (no floating-point atomics: same bytes in,
 *           same bytes out).  ws: acmi_retnorm_ws_doubles(N) doubles.
 * A data-parallel caller sums the moments over ranks between the two calls.
 *   merge   (acmi_retnorm_apply, once, one thread per group, double) for c > 0:
 *           mb = s/c, M2b = max(q - s*s/c, 0), tot = n + c, d = mb - mean,
 *           mean += d*c/tot, M2 += M2b + d*d*n*c/tot, n = tot (Chan et al.);
 *           c == 0 leaves the group's stats alone (all-zero moments: frozen).
 *   scale   inv[g] = f32(1/sqrt(M2/n + eps)) from the merged stats (n == 0:
 *           1.0f); out = clamp(r*inv[groups[n]], -clip, +clip) in float32,
 *           clip <= 0: no clamp.  out == rewards is allowed; inv_out ([G] f32)
 *           is nullable.
 * An env whose group id is >= G touches no memory outside the buffers, joins no
 * group and keeps its rewards as they are (unscaled, unclamped); its carry
 * advances all the same, and acmi_retnorm_scan counts it once per call in
 * *bad_envs (device int32, nullable, accumulated).
 * Three launches in all (scan 2, apply 1, the latter one workgroup), no host
 * synchronisation.  ACMI_ERR_ARG before anything is enqueued: a null required
 * pointer, N < 1, T < 1, G outside 1..64, gamma outside [0, 1], eps < 0. */
int64_t acmi_retnorm_ws_doubles(int64_t N);
int acmi_retnorm_scan(const float* rewards, const uint8_t* terminals,
                      const uint8_t* groups, int N, int T, int G, float gamma,
                      float* carry, double* ws, double* moments, int32_t* bad_envs,
                      acmi_stream_t stream);
int acmi_retnorm_apply(const float* rewards, const uint8_t* groups, int N, int T, int G,
                       const double* moments, double* stats, double eps, float clip,
                       float* out, float* inv_out, acmi_stream_t stream);

/* Episode statistics per group of envs (per game), accumulated on the device:
 * the return and the length of every episode that ended in a rollout; an
 * option beyond the reference, which averages one batch's episode rewards on
 * the host.  State across calls: length_carry[N] i32 (the steps of each env's
 * running episode, starts 0), acc[G][8] f64, groups[N] u8; G in 1..64.  Per
 * call, over episode_rewards[N][T] f32 (what the steppers write: an episode's
 * total reward at the step that ended it, a NaN everywhere else):
 *   scan    per env, ascending t: len += 1; if episode_rewards[n][t] is not a
 *           NaN, (ret = that float, len) is one sample of group groups[n] and
 *           len = 0; length_carry[n] = len at the end.  "Is a NaN" is decided
 *           on the bits, (bits & 0x7fffffff) > 0x7f800000: every NaN payload
 *           means "no episode", +-inf is a sample.
 *   acc[g]  column 0: episodes, 1: sum ret, 2: sum ret^2, 3: sum len,
 *           4: max ret, 5: max(-ret), 6: max len, 7: max(-len).  Columns 0-3
 *           are sums in double (ret converted to double first), in a fixed
 *           order without floating-point atomics: same bytes in, same bytes
 *           out.  A cleared accumulator holds 0 in columns 0-3 and -inf in
 *           columns 4-7; the negated minima let one MAX all-reduce serve both
 *           ends.  (+0 and -0 compare equal: which of them a zero maximum
 *           holds is not specified.)  ws: acmi_epstats_ws_doubles(N) doubles.
 * A call ADDS its samples to what acc holds; the device never resets acc, the
 * caller clears it.  A data-parallel reader sums columns 0-3 and maximises
 * columns 4-7 over ranks.
 * An env whose group id is >= G touches no memory outside the buffers and
 * joins no group; its length_carry advances all the same, and it is counted
 * once per call in *bad_envs (device int32, nullable, accumulated).
 * Two launches, no host synchronisation.  ACMI_ERR_ARG before anything is
 * enqueued: a null required pointer, N < 1, T < 1, G outside 1..64. */
int64_t acmi_epstats_ws_doubles(int64_t N);
int acmi_epstats_update(const float* episode_rewards, /* [N][T] f32, a NaN = no episode ended here */
                        const uint8_t* groups,         /* [N], as acmi_retnorm_scan's */
                        int N, int T, int G,
                        int32_t* length_carry,         /* [N] steps of the running episode, starts 0 */
                        double* ws, double* acc,       /* acc: [G][8] f64, accumulated in place */
                        int32_t* bad_envs,             /* nullable, accumulated */
                        acmi_stream_t stream);

/* Update diagnostics (an option beyond the reference): what one parameter update
 * did, as double accumulators per group of envs (per game) that a log line reads
 * with one copy.  Rows are env-major [N][T]: row m belongs to env m / T.
 * groups[N] u8 is nullable (NULL: every env in group 0); G in 1..64.  An env
 * whose group id is >= G adds nothing and is counted once per call in *bad_envs
 * (device int32, nullable, accumulated).  Every call OVERWRITES its output;
 * nothing carries over between calls.  Every sum is formed in double in an
 * order that the arguments alone fix (partials in ws, one reducing kernel; no
 * floating-point atomics): same bytes in, same bytes out.  Two launches per
 * call, no host synchronisation.  ws: acmi_diag_ws_doubles(M, S) doubles serve
 * any of the three calls over M = N*T rows / S segments (calls that share one
 * ws must be ordered on one stream).
 *
 * acmi_diag_value: acc[g] = (n, sum v, sum y, sum y^2, sum e, sum e^2) over the
 *   rows of group g, v = (double)values[m], y = (double)targets[m], e = y - v
 *   (rounded to double), e^2 rounded before it is added.  The explained variance
 *   1 - Var(e)/Var(y) is the reader's to derive.
 * acmi_diag_policy: acc[g] = (n, sum KL(old||new), sum H(new), max KL) over the
 *   GOOD rows of group g; the maximum starts at -inf.  legal: one uint32 word per
 *   row (nullable; bit a set = action a is legal, bits at or above A ignored), the
 *   meaning the *_masked entry points give it: every sum below runs over the
 *   legal set S only, an illegal logit influences nothing.  Per row and matrix,
 *   in double from the float32 logits z: mx = max_S z, lse = mx + log(sum_S
 *   exp(z - mx)), logp = z - lse, p = exp(logp), all in ascending action order;
 *   KL = sum_S round(p_old (logp_old - logp_new)), H = -sum_S round(p_new logp_new).
 *   A row is BAD when S is empty or any of its A logits, in either matrix, is
 *   not finite; a bad row adds nothing and counts in *bad_rows (device int32,
 *   nullable, accumulated), whatever its env's group.  A in 1..64 without legal,
 *   1..32 with it; ld_old, ld_new >= A.
 * acmi_diag_segments: out[s] = (sum x^2, sum y^2, sum x y, sum (x - y)^2) over the
 *   elements [offsets[s], offsets[s+1]) of x and y, products and the difference
 *   formed in double ((x - y)^2 rounded before it is added).  y is nullable and
 *   then counts as zero.  offsets: device int64 [S + 1], non-decreasing (the
 *   CALLER checks that: the entry point never reads them on the host); an empty
 *   segment gives zeros.  A segment is cut into 64 slices whose length follows
 *   from its two offsets alone, never from the grid.  S in 1..65535.
 *
 * ACMI_ERR_ARG before anything is enqueued: a null required pointer (values,
 * targets, logits_old, logits_new, x, offsets, ws, acc / out), N < 1, T < 1,
 * N*T >= 2^31, G outside 1..64, A or ld_* out of range, S outside 1..65535. */
int64_t acmi_diag_ws_doubles(int64_t M, int64_t S);
int acmi_diag_value(const float* values, const float* targets, /* [N][T] f32 each */
                    const uint8_t* groups,                      /* [N], nullable */
                    int N, int T, int G,
                    double* ws, double* acc,                    /* acc: [G][6] f64, overwritten */
                    int32_t* bad_envs,                          /* nullable, accumulated */
                    acmi_stream_t stream);
int acmi_diag_policy(const float* logits_old, int ld_old,      /* [N*T][ld_old] f32 */
                     const float* logits_new, int ld_new,      /* [N*T][ld_new] f32 */
                     const uint32_t* legal,                     /* [N*T], nullable */
                     const uint8_t* groups,                     /* [N], nullable */
                     int N, int T, int A, int G,
                     double* ws, double* acc,                   /* acc: [G][4] f64, overwritten */
                     int32_t* bad_envs, int32_t* bad_rows,      /* nullable, accumulated */
                     acmi_stream_t stream);
int acmi_diag_segments(const float* x, const float* y,         /* y nullable: zeros */
                       const int64_t* offsets,                  /* device int64 [S + 1] */
                       int S,
                       double* ws, double* out,                 /* out: [S][4] f64, overwritten */
                       acmi_stream_t stream);

/* ------------------------------------------------------------------------
 * A2C losses and their gradient w.r.t. the head outputs.  Replaces
 * objectives.py:132-154 and the head part of tf.gradients of
 * L = L_pi + vcoef*L_v (objectives.py:78).  M = N*T rows.
 *   L_pi = -(mean(adv*logpi(a)) + beta*mean(H)),  L_v = mean((target-V)^2/2)
 * dhead[m][0..A-1] = dL/dlogits, dhead[m][A] = dL/dV, row stride ldh >= A+1,
 * each scaled by grad_scale (1/world_size for data-parallel means).
 * loss_out[0..2] = grad_scale * (L_pi, L_v, mean entropy) — deterministic
 * two-pass sums; scaled like dhead so that a SUM all-reduce over the ranks
 * (the update buffer's loss slots) yields the global means.
 * ws: >= acmi_a2c_loss_ws_floats(M) floats.
 * ---------------------------------------------------------------------- */
int64_t acmi_a2c_loss_ws_floats(int M);
int acmi_a2c_loss(const float* logits, int ld, const float* values,
                  const int32_t* actions, const float* targets,
                  const float* adv, int M, int A, float beta, float vcoef,
                  float grad_scale, float* dhead, int ldh, float* ws,
                  float* loss_out, acmi_stream_t stream);

/* ------------------------------------------------------------------------
 * PPO clipped-surrogate losses (Schulman et al. 2017; beyond the reference)
 * and their gradient w.r.t. the head outputs, in acmi_a2c_loss's layout.
 * Per row: r = exp(logpi(a) - old_logp),
 *   s = min(r*adv, clamp(r, 1-clip_eps, 1+clip_eps)*adv),
 *   L_pi = -(mean(s) + beta*mean(H));
 *   vclip > 0:  Vc = old_values + clamp(V - old_values, +-vclip),
 *               L_v = mean(max((V-target)^2, (Vc-target)^2)/2)
 *   vclip <= 0: L_v = mean((target-V)^2/2)   (old_values may be null).
 * dhead as acmi_a2c_loss (row stride ldh >= A+1, column A = dL/dV, padding
 * zero, scaled by grad_scale/M): the policy term of a row is
 * -(adv*r)(onehot - p) where the unclipped product is the minimum and 0 where
 * the clipped one is; the entropy term is always there.  dL/dV is
 * vcoef*(V-target) where the unclipped square is the maximum, else 0.
 * loss_out[0..3] = grad_scale * (L_pi, L_v, mean entropy,
 * mean(old_logp - logpi(a)) -- the approximate KL);
 * clip_frac_out (nullable) [0] = grad_scale * mean(|r-1| > clip_eps).
 * Deterministic two-pass sums.  The log-sum-exp and logpi(a) are computed
 * like acmi_categorical's: with old_logp from it on the same logits r == 1.0f
 * and dhead equals acmi_a2c_loss's bit for bit.
 * ws: >= acmi_ppo_loss_ws_floats(M) floats.  clip_eps > 0.
 * ---------------------------------------------------------------------- */
int64_t acmi_ppo_loss_ws_floats(int M);
int acmi_ppo_loss(const float* logits, int ld, const float* values,
                  const int32_t* actions, const float* old_logp,
                  const float* old_values, const float* targets,
                  const float* adv, int M, int A, float clip_eps, float vclip,
                  float beta, float vcoef, float grad_scale, float* dhead,
                  int ldh, float* ws, float* loss_out, float* clip_frac_out,
                  acmi_stream_t stream);

/* ------------------------------------------------------------------------
 * Row gather (PPO's shuffled minibatches; beyond the reference).
 * For r in [0, rows): i = index[r];
 *   image:   obs_out + r*out_stride  <-  obs + i*img_stride   (28224 bytes)
 *   vectors: vec_dst[k][r] <- vec_src[k][i]  for k < nvec  (4-byte elements, bit copies)
 * index values outside [0, src_rows) never touch memory outside the buffers: that
 * output row (image and vectors) is zero-filled and *bad_rows (nullable, device int,
 * accumulated) counts it.  Duplicates in index are allowed.  obs_out must not overlap
 * obs; vec_dst[k] must not overlap vec_src[k].  obs, obs_out, img_stride, out_stride
 * 16-byte aligned, both strides >= 28224; obs == NULL gathers the vectors only (obs_out
 * and the strides are then ignored).  0 <= nvec <= 8; vec_src / vec_dst are host arrays
 * of nvec device pointers (passed to the kernel by value).  rows == 0 is ACMI_OK
 * without a launch; every argument error is ACMI_ERR_ARG before anything is enqueued.
 * One launch, no allocation, no sync.
 * ---------------------------------------------------------------------- */
int acmi_gather_rows(const uint8_t* obs, int64_t img_stride, int64_t src_rows,
                     const int32_t* index, int64_t rows,
                     uint8_t* obs_out, int64_t out_stride,
                     int nvec, const void* const* vec_src, void* const* vec_dst,
                     int32_t* bad_rows, acmi_stream_t stream);

/* ------------------------------------------------------------------------
 * Backward through the tower (the rest of tf.gradients, objectives.py:78)
 * fused with the K-FAC input-factor statistics (kfac cov_update_thunks,
 * kfac_utils.py:39,44; registration envs/atari/model.py:219-246):
 *   grads  <- dL/dparams in the param layout (overwritten)
 *   a_stats (nullable) <- for l = 0..4: A_l = mean over rows of [x;1][x;1]^T
 *           (conv: x = the (kh,kw,cin) input patch at every output location,
 *            rows = B*locations; fc: x = the input row; A_4 = fc4 output).
 * dhead: [B][ldh] from acmi_a2c_loss, ldh >= A+1 and a multiple of 4 (rows
 * are read as float4; padding columns zero), else ACMI_ERR_ARG before anything
 * is enqueued.  d1..d4 are [B]x(layer output) scratch.
 * obs: image b at obs + b*img_stride as for acmi_forward, B >= 1,
 * img_stride >= 28224, (B - 1) * img_stride + 28224 < 2^31.  Alignment, by the
 * widest load made from obs: without statistics (acmi_backward, a_stats ==
 * NULL) obs and img_stride multiples of 4, as the forward (conv1's weight
 * gradient reads uint32 pixels); with statistics (a_stats != NULL, and
 * acmi_backward_stacked always) multiples of 8 (conv1's A factor reads two
 * pixels per load).  Every violation is ACMI_ERR_ARG before anything is
 * enqueued (nothing is written).
 * ws: ws_floats >= acmi_backward_ws_floats(B, A, C3) floats; a smaller
 * ws_floats fails with ACMI_ERR_WS before anything is enqueued (nothing is
 * written).  Layout: [operand-scale scratch | conv1 A-factor integers |
 * split-K partials]; the partial region is everything past the fixed prefix, so
 * a larger workspace only lets more of the small layers' finalizes share one
 * launch (results bit-identical for every legal size).
 * net->conv_prep (when non-null) must have been prepared (acmi_conv_prepare)
 * from the same parameters as net->params: its header supplies the a1 / a2 /
 * a3 bounds that scale the f16x2 operands of the conv2 / conv3 / fc4
 * reductions, and the pre-split weights of the input-gradient chain.  Callers
 * re-prepare after every parameter update (NetEngine does, keyed by its
 * parameter version); a stale prep gives wrong scales, not an error.
 * ---------------------------------------------------------------------- */
typedef struct acmi_bwd {
  float* d1; /* [B][20][20][32] */
  float* d2; /* [B][9][9][64]   */
  float* d3; /* [B][7][7][C3]   */
  float* d4; /* [B][512]        */
  const float* dhead;
  int ldh;
} acmi_bwd_t;

int64_t acmi_backward_ws_floats(int B, int num_actions, int conv3_filters);
int acmi_backward(const acmi_net_t* net, const uint8_t* obs,
                  int64_t img_stride, int B, const acmi_acts_t* acts,
                  const acmi_bwd_t* bwd, float* grads, float* a_stats,
                  float* ws, int64_t ws_floats, acmi_stream_t stream);

/* ------------------------------------------------------------------------
 * K-FAC output-factor statistics (kfac "gradients" estimation mode over the
 * predictive distributions registered at policies.py:146-158 and
 * baselines.py:55-69): y_pi ~ Categorical(logits) and y_v ~ N(V, 1) are
 * sampled with the counter RNG keyed (seed, 0, counter, row_offset + b) --
 * row_offset = the global row of batch row 0 (rank * B for an env shard), so
 * a data-parallel shard draws exactly the full batch's samples; the per-example
 * gradients of -log p(y) w.r.t. each registered layer output are
 * back-propagated (dX only) and G_l = mean over rows of g g^T is written to
 * g_stats (layout of acmi_kfac_layout, G part).  Reuses bwd->d1..d4 and ws
 * (ws_floats >= acmi_backward_ws_floats(B, A, C3), else ACMI_ERR_WS before
 * anything is enqueued; layout [scratch | sampled head gradients | partials]).
 * ---------------------------------------------------------------------- */
int acmi_kfac_output_stats(const acmi_net_t* net, int B,
                           const acmi_acts_t* acts, const acmi_bwd_t* bwd,
                           uint32_t seed, uint32_t row_offset, uint32_t counter,
                           float* g_stats, float* ws, int64_t ws_floats,
                           acmi_stream_t stream);
/* acmi_backward + the input-gradient half of acmi_kfac_output_stats in one
 * call, with conv2's input gradient of BOTH chains as one launch (one W2^T
 * stream over the loss chain's and the sampled chain's image rows, the
 * epilogue chosen per tile: the masked d1 store, or conv1's G-factor Gram).
 * bwd / ws: the loss chain's (as acmi_backward); bwd_s / ws_s: the sampled
 * chain's own d1..d4 and workspace (ws_floats, ws_s_floats >=
 * acmi_backward_ws_floats), on which acmi_kfac_output_stats_finish then forms
 * the G factors.  The pair is bit-identical to acmi_backward followed by
 * acmi_kfac_output_stats(bwd_s, ws_s) with the same seed / row_offset /
 * counter, and records the same dX event.  Without net->conv_prep or in
 * ACMI_GEMM_F32 mode the two conv2 launches run one after the other.
 * Reference: the same graphs as acmi_backward / acmi_kfac_output_stats
 * (objectives.py:78-79, policies.py:157-158). */
int acmi_backward_stacked(const acmi_net_t* net, const uint8_t* obs, int64_t img_stride,
                          int B, const acmi_acts_t* acts, const acmi_bwd_t* bwd,
                          float* grads, float* a_stats, float* ws, int64_t ws_floats,
                          const acmi_bwd_t* bwd_s, uint32_t seed, uint32_t row_offset,
                          uint32_t counter, float* ws_s, int64_t ws_s_floats,
                          acmi_stream_t stream);
int acmi_kfac_output_stats_finish(const acmi_net_t* net, int B, const acmi_acts_t* acts,
                                  const acmi_bwd_t* bwd_s, float* g_stats, float* ws_s,
                                  int64_t ws_s_floats, acmi_stream_t stream);
/* Makes `stream` wait (stream-ordered, no host sync) for the point right after
 * the input-gradient chain of the most recent acmi_backward on this device, so
 * a sampled-loss chain (acmi_kfac_output_stats on its own buffers) enqueued on
 * `stream` afterwards runs next to that backward's weight-gradient reductions. */
int acmi_stream_wait_backward_dx(acmi_stream_t stream);

/* ------------------------------------------------------------------------
 * K-FAC running factors: zero-initialised EMA with zero-debias (kfac
 * FisherFactor cov update with cov_ema_decay, a2c_acktr.py:245):
 *   biased = decay*biased + (1-decay)*stats;  factors = biased * debias
 * (debias = 1/(1-decay^t), host-computed).  n floats.
 * ---------------------------------------------------------------------- */
int acmi_kfac_ema(float* biased, float* factors, const float* stats,
                  int64_t n, float decay, float debias, float stats_scale,
                  acmi_stream_t stream);

/* Factor statistics as upper triangles, for the data-parallel all-reduce of the
 * A / G statistics (the symmetric half only, 40 % fewer
 * bytes on the wire): which = 1 the A factors, 2 the G factors, 3 both; the
 * selected factors of the acmi_kfac_layout stats area packed back to back,
 * factor f (n x n) as n(n+1)/2 floats, row r's columns r .. n-1.  Unpack writes
 * both halves (the factors come back exactly symmetric).  Stream-ordered. */
int64_t acmi_kfac_packed_floats(int num_actions, int conv3_filters, int which);
int acmi_kfac_pack(int num_actions, int conv3_filters, int which, const float* stats, float* packed,
                   acmi_stream_t stream);
int acmi_kfac_unpack(int num_actions, int conv3_filters, int which, const float* packed, float* stats,
                     acmi_stream_t stream);

/* ------------------------------------------------------------------------
 * Damped inverses (kfac inv_update_thunks, kfac_utils.py:46-50): per layer
 *   lambda_l = damping / (conv_normalize && l<3 ? locations_l : 1)
 *   pi_l = sqrt((tr A_l / din_l) / (tr G_l / dout_l))
 *   Ainv_l = (A_l + pi_l*sqrt(lambda_l) I)^-1,  Ginv_l = (G_l + sqrt(lambda_l)/pi_l I)^-1
 * computed in fp64 (block Gauss-Jordan, SPD, no pivoting) and stored f32.
 * inv layout: 12 blocks, m = 2l (Ainv_l, n = din_l) and 2l+1 (Ginv_l,
 * n = dout_l); block m is n rows of stride ld_m = n rounded up to 4 at
 * offsets[m] (acmi_kfac_inverse_layout), padding columns zero, so the
 * preconditioning GEMMs read aligned float4 runs.
 * ws: >= acmi_kfac_inverse_ws_doubles(...) doubles.
 * ---------------------------------------------------------------------- */
int acmi_kfac_inverse_layout(int num_actions, int conv3_filters, int64_t* offsets,
                             int64_t* lds);
int64_t acmi_kfac_inverse_floats(int num_actions, int conv3_filters);
int64_t acmi_kfac_inverse_ws_doubles(int num_actions, int conv3_filters);
int acmi_kfac_inverse(int num_actions, int conv3_filters,
                      const float* factors, float damping, int conv_normalize,
                      float* inv, double* ws, acmi_stream_t stream);

/* Eigendecomposition of every damped-factor input (fp64 cyclic Jacobi):
 * eigenvalues (ascending) of A_l / G_l written to `eigvals` in the factor
 * layout order (diagnostic and parity path; north_star "KFAC eigenvalues"). */
int64_t acmi_kfac_eig_ws_doubles(int num_actions, int conv3_filters);
int acmi_kfac_eigvals(int num_actions, int conv3_filters, const float* factors,
                      double* eigvals, double* ws, acmi_stream_t stream);

/* ------------------------------------------------------------------------
 * Natural-gradient step (KfacOptimizer.apply_gradients, kfac_utils.py:53,
 * a2c_acktr.py:243-246):  Delta_l = Ainv_l [dW_l; db_l] Ginv_l;
 *   coeff = min(1, sqrt(norm_constraint / (lr^2 * sum_l <g_l, Delta_l>)));
 *   v = momentum*v + coeff*Delta;   params -= lr*v.
 * coeff is computed on the device (no host round trip); *coeff_out gets it.
 * ws: >= acmi_kfac_step_ws_floats() floats; scratch, its contents on entry do
 * not matter.  precon (nparams floats) is an output.
 * ---------------------------------------------------------------------- */
int64_t acmi_kfac_step_ws_floats(int num_actions, int conv3_filters);
int acmi_kfac_step(int num_actions, int conv3_filters, float* params,
                   float* velocity, const float* grads, const float* inv,
                   float lr, float momentum, float norm_constraint,
                   float* precon, float* ws, float* coeff_out,
                   acmi_stream_t stream);

/* ------------------------------------------------------------------------
 * First-order optimizers.  ClipGlobalNormOptimizer (nn.py:159-189) + TF1
 * MomentumOptimizer (cold start, a2c_acktr.py:240-241) / RMSPropOptimizer
 * (a2c_acktr.py:250-251, decay .9, momentum 0, eps 1e-10, ms init 1).
 * clip_norm <= 0 disables clipping.  norm_out (nullable) <- global norm.
 * ---------------------------------------------------------------------- */
int64_t acmi_opt_ws_floats(int64_t n);
int acmi_momentum_apply(float* params, float* accum, const float* grads,
                        int64_t n, float lr, float momentum, float clip_norm,
                        float* ws, float* norm_out, acmi_stream_t stream);
int acmi_rmsprop_apply(float* params, float* ms, float* mom,
                       const float* grads, int64_t n, float lr, float decay,
                       float momentum, float eps, float clip_norm, float* ws,
                       float* norm_out, acmi_stream_t stream);
/* TF1 AdamOptimizer (beyond the reference; the PPO example's optimizer):
 * m = b1*m + (1-b1)*g;  v = b2*v + (1-b2)*g^2;  var -= lr_t*m/(sqrt(v)+eps),
 * lr_t = lr*sqrt(1-b2^t)/(1-b1^t) formed by the caller (t = 1, 2, ...).
 * Clipping, ws and norm_out as above. */
int acmi_adam_apply(float* params, float* m, float* v, const float* grads,
                    int64_t n, float lr_t, float beta1, float beta2, float eps,
                    float clip_norm, float* ws, float* norm_out,
                    acmi_stream_t stream);

/* ------------------------------------------------------------------------
 * Batched synthetic Atari stepper — replaces MultiEnv.step/reset over
 * SubprocessEnv (multi_env.py:49-81, 121-137, 140-362) with the semantics
 * of FrameStackWrapper (wrappers.py:201-235) and EpisodeInfoWrapper
 * (wrappers.py:263-323).  Frames are 84x84 u8 from mix32 of
 * (seed, env, episode, step, action); rewards in {-1,0,1} w.p. .05/.9/.05;
 * episode length 50 + (hash % 451).  State arrays are per env ([N]).
 * Stacks are NHWC [84][84][4] u8; env n reads obs_in + n*in_stride and
 * writes obs_out + n*out_stride (in-place allowed).
 * Mixed games (Atari-57, BASELINE configs[4] -- an extension: the
 * reference's MultiEnv holds one game, multi_env.py:36-47): with `game`
 * set, env n plays game[n] (0..56, the order of wrappers.ATARI57), whose
 * own salt, episode-length range, reward rates and legal-action count
 * (actions past it step as NOOP) replace the defaults above; game 12
 * (Breakout) keeps them.  game == NULL: every env the default game.
 * ---------------------------------------------------------------------- */
typedef struct acmi_env_state {
  int32_t* episode;   /* episode index                                    */
  int32_t* step;      /* steps taken in the current episode               */
  int32_t* length;    /* terminal step of the current episode             */
  float* total;       /* EpisodeInfoWrapper.total_reward                   */
  uint8_t* done;      /* _AutoResetWrapper._terminated                     */
  const uint8_t* game; /* game index per env, or NULL (read only)          */
} acmi_env_state_t;

int acmi_env_reset(const acmi_env_state_t* st, int N, int env_offset,
                   uint32_t seed, uint8_t* obs_out, int64_t out_stride,
                   acmi_stream_t stream);
/* rewards/terminals/episode_rewards: element n at [n*ld]; episode_rewards
 * gets the episode total at a terminal step and NaN otherwise.           */
int acmi_env_step(const acmi_env_state_t* st, int N, int env_offset,
                  uint32_t seed, const int32_t* actions, const uint8_t* obs_in,
                  int64_t in_stride, uint8_t* obs_out, int64_t out_stride,
                  float* rewards, uint8_t* terminals, float* episode_rewards,
                  int64_t ld, acmi_stream_t stream);

/* ------------------------------------------------------------------------
 * Device games: small real games that step and render on the
 * GPU straight into the stacked observation -- game 0 Catch (3 own actions),
 * game 1 Breakout (4).  Integer dynamics; the rule book is the host
 * implementation actorcritic/envs/games/host.py (HostGame), which the kernel
 * reproduces bit for bit: frames, rewards, terminals, state.  Actions at or
 * past a game's own count act as NOOP.
 * acmi_game_step has acmi_env_step's arguments and semantics word for word
 * (lazy auto-reset at the step after a terminal, the FrameStackWrapper roll
 * with zero-fill on a terminal step and the reset frame repeated 4x,
 * episode_rewards NaN unless the episode ended; in place allowed); strides
 * are multiples of 16, at least 84*84*4.  vars holds acmi_game_state_ints()
 * int32 per env: ball x, y, vx, vy, paddle x, lives, three brick words (row r,
 * column c: bit 12*(r%2)+c of word r/2), zero padding.  The struct's size
 * is not among acmi_abi_struct_sizes' five: acmi_game_state_bytes() is it.
 * ---------------------------------------------------------------------- */
typedef struct acmi_game_state {
  int32_t* episode;   /* episode index                                    */
  int32_t* step;      /* steps taken in the current episode               */
  float* total;       /* EpisodeInfoWrapper.total_reward                   */
  uint8_t* done;      /* _AutoResetWrapper._terminated                     */
  int32_t* vars;      /* [N][acmi_game_state_ints()] game variables        */
  int32_t game;       /* 0 Catch, 1 Breakout                               */
} acmi_game_state_t;

int acmi_game_state_ints(void);
int64_t acmi_game_state_bytes(void);
int acmi_game_reset(const acmi_game_state_t* st, int N, int env_offset,
                    uint32_t seed, uint8_t* obs_out, int64_t out_stride,
                    acmi_stream_t stream);
int acmi_game_step(const acmi_game_state_t* st, int N, int env_offset,
                   uint32_t seed, const int32_t* actions, const uint8_t* obs_in,
                   int64_t in_stride, uint8_t* obs_out, int64_t out_stride,
                   float* rewards, uint8_t* terminals, float* episode_rewards,
                   int64_t ld, acmi_stream_t stream);

/* acmi_game_step under rules that separate "cut the return here" from "the
 * game restarts" (host.py, "Cuts"; the reference's AtariEpisodicLifeWrapper,
 * envs/atari/wrappers.py:89-117, and a time limit that is not a terminal).
 *   game over  = the game's own end (Catch: the ball landed; Breakout: no
 *                lives or no bricks) or step >= cap, cap = max_steps, or the
 *                game's own with 0 (Breakout 2000, Catch none);
 *   terminals  = game over, or (episodic_life and a life went in this step):
 *                the learner's terminal, which also zero-fills the old
 *                channels of the stack;
 *   truncated  = step >= cap and not the game's own end and not a life cut:
 *                the cap alone ended the episode (nullable: not written);
 *   episode_rewards = the whole game's total at a game-over step (a truncated
 *                one included), the quiet NaN otherwise (life cuts included).
 * done becomes a code: 0 running, 1 game over (the next step resets lazily, as
 * acmi_game_step), 2 life lost (the next step restarts the stack from the
 * current state's frame repeated 4x -- FrameStackWrapper.reset -- and the game,
 * episode, step and total go on).  Only this entry point writes 2.  Rules
 * {0, 0} with truncated == NULL write the bytes of acmi_game_step (one kernel).
 * rules == NULL, episodic_life outside {0, 1} or max_steps outside 0..2000:
 * ACMI_ERR_ARG, nothing enqueued. */
typedef struct acmi_game_rules {
  int32_t episodic_life; /* 1: a lost life is a terminal for the learner    */
  int32_t max_steps;     /* step cap 1..2000; 0 = the game's own             */
} acmi_game_rules_t;

int acmi_game_step_cuts(const acmi_game_state_t* st, const acmi_game_rules_t* rules,
                        int N, int env_offset, uint32_t seed, const int32_t* actions,
                        const uint8_t* obs_in, int64_t in_stride, uint8_t* obs_out,
                        int64_t out_stride, float* rewards, uint8_t* terminals,
                        uint8_t* truncated, float* episode_rewards, int64_t ld,
                        acmi_stream_t stream);

/* Mixed batches: Catch and Breakout envs side by side in one launch, under one
 * policy head (the envs' own action sets as per-env legal-action words: catch
 * 0b0111, breakout 0b1111; actorcritic.envs.games: DeviceGameEnvs('catch+breakout')).
 * acmi_game_count() is 2; acmi_game_actions(game) is a game's own action count (3, 4;
 * ACMI_ERR_ARG for another id).
 * games: one byte per env OF THE CALL (device; the pointer already at the call's first
 * env, as the state pointers are): env n plays games[n], whatever st->game says (which
 * must still be a valid id).  games == NULL: st->game for every env; then
 * acmi_game_reset_mixed is acmi_game_reset and acmi_game_step_mixed is
 * acmi_game_step_cuts, byte for byte (the same two kernels).  rules is required, as in
 * acmi_game_step_cuts, and holds for every env; {0, 0} gives acmi_game_step's behaviour.
 * An env's trace is a function of (seed, env_offset + n, its game, its actions) only.
 * An id at or past acmi_game_count() makes a BAD env: its state is left untouched, its
 * output stack zero-filled, reward 0, terminal 0, truncated 0, episode reward the quiet
 * NaN, and it is counted once per call in bad_envs (device int32, nullable,
 * accumulates; the caller zeroes it).
 * Argument errors are ACMI_ERR_ARG with nothing enqueued, as above. */
int acmi_game_count(void);
int acmi_game_actions(int game);
int acmi_game_reset_mixed(const acmi_game_state_t* st, const uint8_t* games, int N,
                          int env_offset, uint32_t seed, uint8_t* obs_out,
                          int64_t out_stride, int32_t* bad_envs, acmi_stream_t stream);
int acmi_game_step_mixed(const acmi_game_state_t* st, const uint8_t* games,
                         const acmi_game_rules_t* rules, int N, int env_offset,
                         uint32_t seed, const int32_t* actions, const uint8_t* obs_in,
                         int64_t in_stride, uint8_t* obs_out, int64_t out_stride,
                         float* rewards, uint8_t* terminals, uint8_t* truncated,
                         float* episode_rewards, int64_t ld, int32_t* bad_envs,
                         acmi_stream_t stream);

/* ------------------------------------------------------------------------
 * Atari frame preprocessing for real (raw RGB) frames, batched over envs:
 * replaces the frame half of the reference's per-env wrapper chain
 *   AtariFrameskipWrapper  (envs/atari/wrappers.py:54-67: np.amax of the last
 *                           two raw frames),
 *   AtariPreprocessFrameWrapper (wrappers.py:30-33: cv2 RGB2GRAY + INTER_AREA
 *                           resize to 84x84),
 *   FrameStackWrapper      (wrappers.py:224-235: roll, zero on terminal,
 *                           insert; reset repeats the frame 4 times).
 * Env n's frames: raw + n*env_stride is its LAST frame [H][W][3] u8, and, when
 * frame_stride != 0 and (nframes null or nframes[n] >= 2), the frame before
 * it is at + frame_stride (max-pooled with it).  H, W in [84, 504],
 * H*W <= 40960, W a multiple of 4, not both multiples of 84 (cv2's
 * integer-ratio fast path is not restated); raw/strides 4-byte aligned.
 * ---------------------------------------------------------------------- */
/* gray [84][84] u8 of env n at gray_out + n*out_stride */
int acmi_atari_preprocess(const uint8_t* raw, int64_t env_stride,
                          int64_t frame_stride, const uint8_t* nframes, int N,
                          int H, int W, uint8_t* gray_out, int64_t out_stride,
                          acmi_stream_t stream);
/* 4-frame stacks [84][84][4] u8 at stack + n*stack_stride: reset != 0 ->
 * [f,f,f,f]; else [s1,s2,s3,f], or [0,0,0,f] where terminals[n] != 0
 * (terminals nullable).  stack_in == stack_out is allowed. */
int acmi_atari_stack(const uint8_t* raw, int64_t env_stride, int64_t frame_stride,
                     const uint8_t* nframes, int N, int H, int W,
                     const uint8_t* terminals, int reset, const uint8_t* stack_in,
                     uint8_t* stack_out, int64_t stack_stride, acmi_stream_t stream);
/* The rollout form for host-stepped envs: _AutoResetWrapper.step over
 * FrameStackWrapper.reset/step (multi_env.py:121-137, wrappers.py:224-235) of N
 * envs in one launch.  `frames` holds nslots raw [H][W][3] u8 frames, slot s at
 * frames + s*frame_stride (frame_stride >= H*W*3; one frame each: the host
 * chain has already max-pooled the skipped pair).  step_slot / reset_slot:
 * device int32[N], negative = absent; terminals: device u8[N], nullable.
 * With G / R the gray + INTER_AREA of frames step_slot[n] / reset_slot[n]
 * (acmi_atari_preprocess's arithmetic), env n's stack word p becomes
 *   step  reset   out[p]
 *   >= 0  <  0    (term ? 0 : in[p] >> 8) | G << 24
 *   >= 0  >= 0    (term ? 0 : (R*0x01010101) >> 8) | G << 24   reset, then step
 *   <  0  >= 0    R*0x01010101                                 the first reset
 *   <  0  <  0    in[p]                                        env not stepped
 * stack_in + n*in_stride -> stack_out + n*out_stride; stack_in == stack_out
 * needs equal strides, otherwise the stacks read and written must not overlap.
 * stack_in may be NULL when no env reads it (rows 2, 3, and row 1 on a
 * terminal).  An env with a slot >= nslots reads nothing: its stack is zero and
 * *bad_envs (device int, nullable, accumulated) counts it once; so is an env
 * that needs stack_in when it is NULL.  Shapes and alignment as above, for
 * frames, both stacks and all three strides; N <= 65535. */
int acmi_atari_rollout_frames(const uint8_t* frames, int64_t frame_stride,
                              int64_t nslots, int H, int W, int N,
                              const int32_t* step_slot, const int32_t* reset_slot,
                              const uint8_t* terminals, const uint8_t* stack_in,
                              int64_t in_stride, uint8_t* stack_out,
                              int64_t out_stride, int32_t* bad_envs,
                              acmi_stream_t stream);
/* The launch plan the three entry points above make for H x W frames, host
 * arithmetic only (no GPU needed, nothing launched): out = {fixed3, max_run_y,
 * max_run_x, band_rows, lds_bytes_frames, lds_bytes_rollout} -- whether the
 * kernels with run lengths fixed at 3 are chosen (both longest runs <= 3;
 * otherwise the table-driven ones), the longest INTER_AREA run over the 84
 * destination rows / columns, the gray source rows a band of 21 output rows
 * may stage in LDS, and the dynamic LDS bytes of acmi_atari_preprocess / _stack
 * and of acmi_atari_rollout_frames.  ACMI_ERR_ARG for a shape they refuse. */
int acmi_atari_plan(int H, int W, int32_t out[6]);

/* Rollout variant of acmi_forward: batch row b reads image b of `obs` and
 * writes activation row b*act_img_stride (env-major [N][T] buffers, the
 * pointers in *acts pre-offset by step t), so step t of a T-step rollout
 * lands where the update expects it and the update re-uses it: a1..a4, value
 * and m1..m3 at b*act_img_stride rows of their own row size, logits at
 * b*act_img_stride*ld_logits floats; the rows in between are not touched.
 * act_img_stride >= 1; obs / img_stride / ld_logits as for acmi_forward. */
int acmi_forward_strided(const acmi_net_t* net, const uint8_t* obs,
                         int64_t img_stride, int B, const acmi_acts_t* acts,
                         int want_value, int64_t act_img_stride,
                         acmi_stream_t stream);

/* One whole rollout step (MultiEnvAgent.interact's loop body, agents.py:
 * 199-219: sample_actions + MultiEnv.step) in two launch groups: the tower
 * of acmi_forward_strided up to fc4, then ONE fused kernel per env (one
 * workgroup each) that finalises a4, computes the heads, samples the action
 * (acmi_sample_actions_dev semantics, row = io->row_offset + b) and steps the
 * env (acmi_env_step semantics, reading the same frames `obs`).  Bit-identical
 * to acmi_forward_strided + acmi_sample_actions_dev + acmi_env_step.
 * Takes net->num_actions <= 31 only (the fused kernel keeps the A + 1 heads of
 * its env in 32 floats of LDS): 32..64 actions fail with ACMI_ERR_ARG before
 * anything is enqueued; step those with the three calls above, which take the
 * whole 1..64 (MultiEnvAgent does). */
typedef struct acmi_rollout_io {
  uint32_t seed, stream_id, counter; /* sampler RNG key                      */
  const uint32_t* counter_dev;       /* nullable: counter += *counter_dev     */
  int row_offset;                    /* global row of batch row 0            */
  int32_t* actions;                  /* out, element b at [b*ld] (ld below)  */
  int32_t* bad_rows;                 /* device counter of non-finite rows    */
  acmi_env_state_t state;            /* env state of batch row 0's env       */
  int env_offset;                    /* global env id of batch row 0         */
  uint32_t env_seed;
  uint8_t* obs_out;                  /* next stacked frames, env b at b*out_stride */
  int64_t out_stride;
  float* rewards;                    /* element b at [b*ld]                  */
  uint8_t* terminals;
  float* episode_rewards;
  int64_t ld;
  /* Step fusion (zero / NULL: off).  next_acts: after its env step, each
   * env's workgroup runs the NEXT step's conv tower on the stack it just
   * wrote (obs_out, image stride out_stride), from LDS, into next_acts'
   * a1..a3 / m1..m3 rows (image stride next_act_stride) -- the tower launch
   * of the next step is then skipped by passing tower_done = 1 with it.
   * Needs the fused tower (x3 gemm mode, prepared weights, 16-byte aligned
   * obs_out / out_stride).  Bit-identical to the unfused steps.
   * At B <= 64 the fused step splits each image's tower over 7 workgroups;
   * their env step then leaves the post-step env states pending in acts->ws
   * (after the fc4 slabs; acmi_forward_ws_floats(B) reserves them) and the
   * NEXT step's fc4 launch commits them into `state`: consecutive fused steps
   * of a rollout must pass the same acts->ws, and a rollout must end with an
   * unfused step (next_acts = NULL, tower_done = 1), whose launch commits the
   * last pending states before its own env step.  Every step at B <= 64 commits
   * the entries still flagged there first, so a rollout abandoned between
   * fused steps is committed by the next rollout's step 0 on the same
   * acts->ws; the pending area must start zeroed (zero-fill the forward
   * workspace once before its first rollout step). */
  int tower_done;
  const struct acmi_acts* next_acts;
  int64_t next_act_stride;
  /* nullable: the stacks this step reads (obs) are also copied to
   * obs_copy + b*out_stride (step 0 reads the previous rollout's final
   * stacks in place and files them into the batch's step-0 rows) */
  uint8_t* obs_copy;
} acmi_rollout_io_t;
int acmi_rollout_step(const acmi_net_t* net, const uint8_t* obs,
                      int64_t img_stride, int B, const acmi_acts_t* acts,
                      int64_t act_img_stride, const acmi_rollout_io_t* io,
                      acmi_stream_t stream);

/* ------------------------------------------------------------------------
 * Legal-action masks (invalid-action masking; beyond the reference).  Opt-in:
 * each entry point below is its unmasked counterpart plus `legal`, device
 * uint32[rows], bit a of legal[row] set = action a is legal for that row (a
 * caller with a row offset passes the pointer pre-offset).  S = the legal
 * a < A; bits at or above A are ignored.  A <= 32 (a larger A, or a NULL
 * `legal`, is ACMI_ERR_ARG before anything is enqueued; the unmasked entry
 * points keep 1..64).  Per row, in f32, ascending a, the unmasked kernels'
 * expressions restricted to S:
 *   mx = max_S z, se = sum_S expf(z - mx), lse = mx + logf(se),
 *   p_a = expf(z_a - lse) on S and exactly 0 elsewhere, H = -sum_S p_a (z_a - lse),
 *   log_prob(a) = z_a - lse on S, -INFINITY elsewhere.
 * Sampling: inverse CDF over S (target = u * se, the running sum over S
 * ascending; the fallback is the LAST LEGAL action), mode = first maximal
 * legal index; the non-finite check covers all A logits; an empty S yields
 * -1 and counts in bad_rows like a non-finite row.  Gradients: columns
 * outside S of dhead / the sampled head gradient are +0.0f; an illegal
 * logit, however large (finite), influences nothing.  Loss kernels: a row
 * whose S is empty or whose taken action is outside S is a bad row -- it adds
 * nothing to the policy / entropy (/ PPO KL and clip) sums, gets zero policy
 * columns, keeps its value term and its share of the 1/M means, and
 * increments *bad_rows (device int32, nullable); it never produces NaN/inf.
 * With the low A bits of every word set each entry point produces the bytes
 * of its unmasked counterpart (the kernels are one template).
 * ---------------------------------------------------------------------- */
int acmi_sample_actions_masked(const float* logits, int ld, int B, int A,
                               uint32_t seed, uint32_t stream_id,
                               const uint32_t* counter_dev, uint32_t counter_add,
                               int row_offset, const float* uniforms, int mode,
                               const uint32_t* legal, int32_t* actions,
                               int32_t* bad_rows, acmi_stream_t stream);
int acmi_categorical_masked(const float* logits, int ld, int B, int A,
                            const int32_t* actions, const uint32_t* legal,
                            float* entropy, float* log_prob, acmi_stream_t stream);
/* Workspaces: acmi_a2c_loss_ws_floats / acmi_ppo_loss_ws_floats; the loss
 * slots and grad_scale are the unmasked calls'.  With old_logp from
 * acmi_categorical_masked on the same logits and mask the PPO ratio is exactly
 * 1 and dhead is acmi_a2c_loss_masked's, bit for bit. */
int acmi_a2c_loss_masked(const float* logits, int ld, const float* values,
                         const int32_t* actions, const float* targets,
                         const float* adv, int M, int A, float beta, float vcoef,
                         float grad_scale, float* dhead, int ldh, float* ws,
                         float* loss_out, const uint32_t* legal, int32_t* bad_rows,
                         acmi_stream_t stream);
int acmi_ppo_loss_masked(const float* logits, int ld, const float* values,
                         const int32_t* actions, const float* old_logp,
                         const float* old_values, const float* targets,
                         const float* adv, int M, int A, float clip_eps, float vclip,
                         float beta, float vcoef, float grad_scale, float* dhead,
                         int ldh, float* ws, float* loss_out, float* clip_frac_out,
                         const uint32_t* legal, int32_t* bad_rows, acmi_stream_t stream);
/* acmi_kfac_output_stats with y ~ Cat over S (the same RNG key): the sampled
 * head gradient is p - onehot(y) on S and 0 elsewhere; the value draw is
 * unchanged.  (acmi_backward_stacked has no masked form.) */
int acmi_kfac_output_stats_masked(const acmi_net_t* net, int B, const acmi_acts_t* acts,
                                  const acmi_bwd_t* bwd, uint32_t seed, uint32_t row_offset,
                                  uint32_t counter, const uint32_t* legal, float* g_stats,
                                  float* ws, int64_t ws_floats, acmi_stream_t stream);
/* acmi_rollout_step with env b's draw over legal[b] (one word per env of the
 * call): bit-identical to acmi_forward_strided + acmi_sample_actions_masked +
 * acmi_env_step. */
int acmi_rollout_step_masked(const acmi_net_t* net, const uint8_t* obs,
                             int64_t img_stride, int B, const acmi_acts_t* acts,
                             int64_t act_img_stride, const acmi_rollout_io_t* io,
                             const uint32_t* legal, acmi_stream_t stream);

/* ------------------------------------------------------------------------
 * The fused rollout step for the device games: acmi_rollout_step[_masked] with
 * acmi_game_step_mixed in place of acmi_env_step -- the same two launch groups,
 * the same kernels with the games' step in their tail.  Bit-identical to
 * acmi_forward_strided + acmi_sample_actions_dev[_masked] + acmi_game_step_mixed
 * (state arrays, truncations and bad_envs included).
 *   io         as for acmi_rollout_step (row_offset, env_offset, env_seed, ld,
 *              tower_done / next_acts / next_act_stride / obs_copy and the
 *              num_actions <= 31 limit unchanged); io.state is ignored.
 *   state      the game state, pointers at batch row 0's env.
 *   games      one byte per env of the call, nullable (state.game for all).
 *   rules      as for acmi_game_step_cuts; {0, 0} gives acmi_game_step's step.
 *   truncated  nullable; element b at [b*io.ld], like the terminals.
 *   bad_envs   nullable; a bad env (games[b] >= acmi_game_count()) keeps its
 *              state, gets a zero stack (the next tower runs on zeros), reward
 *              0, terminal 0, truncated 0, a NaN episode reward, and is counted
 *              once per step.
 *   pend       the pending area of the split form, B * acmi_game_pend_ints()
 *              int32, 16-byte aligned, zeroed before its first step.  At B <= 64
 *              a step with next_acts leaves each env's post-step state (episode,
 *              step, total, done code, vars and a flag) there, and the NEXT
 *              step's fc4 launch commits the flagged entries into `state`; so
 *              every step of such a rollout passes the same pend, the rollout
 *              ends with an unfused-tower step (next_acts = NULL, tower_done =
 *              1), and a caller that re-initialises `state` (acmi_game_reset*)
 *              zeroes pend as well, or a stale entry would be committed over the
 *              reset state.  It is NOT in acts->ws: acmi_forward_ws_floats is
 *              unchanged.  Required (ACMI_ERR_ARG) at B <= 64 with next_acts or
 *              tower_done set; unused above 64.
 * legal: nullable; as in acmi_rollout_step_masked (then num_actions <= 32 holds
 * anyway).  NULL pointers among the required ones, rules or state.game out of
 * range, num_actions > 31, a missing or misaligned pend: ACMI_ERR_ARG before
 * anything is enqueued.  B = 0: ACMI_OK, nothing launched.  The struct's size:
 * acmi_rollout_game_io_bytes() (it is not among acmi_abi_struct_sizes' five).
 * ---------------------------------------------------------------------- */
typedef struct acmi_rollout_game_io {
  acmi_rollout_io_t io;
  acmi_game_state_t state;
  const uint8_t* games;
  acmi_game_rules_t rules;
  uint8_t* truncated;
  int32_t* bad_envs;
  int32_t* pend;
} acmi_rollout_game_io_t;
int acmi_game_pend_ints(void);
int64_t acmi_rollout_game_io_bytes(void);
int acmi_rollout_step_games(const acmi_net_t* net, const uint8_t* obs,
                            int64_t img_stride, int B, const acmi_acts_t* acts,
                            int64_t act_img_stride, const acmi_rollout_game_io_t* io,
                            const uint32_t* legal, acmi_stream_t stream);

/* ------------------------------------------------------------------------
 * Building blocks exposed for parity tests and the bench (not needed by a
 * reference-shaped caller).
 * ---------------------------------------------------------------------- */
/* Host-only self-check of the GEMM launch planners (no GPU needed): the
 * slab groups of the fused wgrad/A-factor reduction cover every needed
 * sub-tile and column sum for K = 64..max_k, split-K chunks cover the rows,
 * the forward's fc4 split counts all have a compiled heads / tail kernel.
 * Returns 0, or the first failing K (-1: chunk plan, -3000: fc4 split counts). */
int acmi_selftest_plans(int max_k);
/* Host-only diagnostic: the number of times acmi_backward / acmi_kfac_output_stats
 * finalized their deferred small-layer set early because the next layer's
 * split-K partials did not fit in the rest of the workspace (a legal size near
 * the minimum), since the previous call of this function (which resets it). */
int acmi_debug_ws_flushes(void);
/* Diagnostic (same-lease A/B of conv2's input gradient in the two K-FAC chains):
 * mode 0 = the two launches of acmi_backward / acmi_kfac_output_stats (the
 * loss chain's d2a -> masked d1 with max |d1| into d1max; the sampled chain's
 * d2b -> conv1's G-factor Gram partials); mode 1 = the same products stacked in
 * one launch (one W2^T stream, the epilogue chosen per tile); mode 2 = the two
 * launches of mode 0 on the resident form (W2^T held in LDS, one 768-thread
 * block per CU), whatever the batch size.  All three give the same bits.
 * d2max_*: the published max |d2| slots; m1: the ReLU' mask words; needs
 * net->conv_prep. */
int acmi_debug_convt2(const acmi_net_t* net, int mode, const float* d2a, const float* d2b,
                      const uint32_t* m1, float* d1, int B, float* gram_part,
                      const uint32_t* d2max_a, const uint32_t* d2max_b, uint32_t* d1max,
                      acmi_stream_t stream);
/* Diagnostic (tests, A/Bs): which form of conv2's input gradient acmi_backward and
 * acmi_kfac_output_stats launch in this process: -1 = chosen by batch size (the
 * default), 0 = always the staging form, 1 = always the resident form.  Returns
 * the previous setting.  The forms are bit-identical; only speed differs. */
int acmi_debug_convt2_form(int form);

/* C[M][N] = A[M][K] @ B[K][N], row-major fp32, f32-input MFMA */
int acmi_gemm_f32(const float* A, const float* B, float* C, int M, int N,
                  int K, acmi_stream_t stream);

/* Launch-site timing for the bench: while enabled, HIP events are recorded on
 * the launch stream around every launch of `site` (up to `capacity`);
 * acmi_prof_collect synchronises them and returns the summed milliseconds
 * and the count, then rearms.  site 0 disables.  Not graph-capture safe. */
#define ACMI_PROF_CONV1_WGRAD 1 /* conv1 [P;1]^T [dY] reduction GEMM */
#define ACMI_PROF_CONV2_WGRAD 2
#define ACMI_PROF_CONV1_FWD 3
#define ACMI_PROF_CONV1_AFACTOR 4 /* exact-integer i8-MFMA conv1 A factor */
#define ACMI_PROF_CONV2_DX 5      /* conv2 input gradient (all stride phases) */
#define ACMI_PROF_FC4_DX 6        /* fc4 input gradient d4 W4^T (+ ReLU') */
#define ACMI_PROF_CONV3_DX 7      /* conv3 input gradient */
int acmi_prof_enable(int site, int capacity);
int acmi_prof_collect(double* total_ms, int* count);

#ifdef __cplusplus
}
#endif
#endif /* ACMI_H_ */
