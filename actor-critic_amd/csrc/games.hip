// Device games: the batched stepper of Catch and Breakout (DESIGN.md 7d;
// rules in actorcritic/envs/games/host.py, dynamics and renderer in games.hpp).
// acmi_game_step has acmi_env_step's calling convention and its semantics: lazy
// auto-reset at the step after a terminal, the FrameStackWrapper roll (zero-fill
// of the three old channels on a terminal step, the reset frame repeated 4x on
// reset), the episode total at a terminal step and a quiet NaN otherwise.
// acmi_game_step_cuts is the same step under acmi_game_rules_t: a lost life may be
// the learner's terminal while the game goes on in place (done = 2: the next step
// restarts the stack only), the step cap is configurable, and a terminal that the
// cap alone caused is flagged in `truncated` for the targets (acmi_*_trunc, rl.hip).
// One 256-thread workgroup per env, one launch per step, 28 KB in and 28 KB out
// per env.
#include "games.hpp"

namespace acmi {

__global__ __launch_bounds__(kGameThreads) void game_reset_kernel(acmi_game_state_t st, int env_offset,
                                                                  uint32_t seed, uint8_t* obs, long long stride) {
  const int n = blockIdx.x;
  GameVars v;
  game_start(st.game, seed, (uint32_t)(env_offset + n), 0u, v);
  const GameView w = game_view(st.game, v);
  uint4* out = reinterpret_cast<uint4*>(obs + (long long)n * stride);
  for (int g = threadIdx.x; g < kGameFrameWords; g += kGameThreads) {
    const uint4 p = game_word(w, g);
    out[g] = make_uint4(p.x * 0x01010101u, p.y * 0x01010101u, p.z * 0x01010101u, p.w * 0x01010101u);
  }
  if (threadIdx.x == 0) {
    st.episode[n] = 0;
    st.step[n] = 0;
    st.total[n] = 0.f;
    st.done[n] = 0;
    game_store(st.vars + (long long)n * kGameInts, v);
  }
}

// Both entry points launch this kernel: acmi_game_step with rules {0, 0} and no
// truncated array, under which term == over and done never holds kLifeLost.
__global__ __launch_bounds__(kGameThreads) void game_step_kernel(
    acmi_game_state_t st, acmi_game_rules_t rules, int env_offset, uint32_t seed, const int32_t* actions,
    const uint8_t* obs_in, long long in_stride, uint8_t* obs_out, long long out_stride, float* rewards,
    uint8_t* terminals, uint8_t* truncated, float* ep_rewards, long long ld) {
  const int n = blockIdx.x;
  const uint32_t e = (uint32_t)(env_offset + n);
  // the previous stack's words first, all of a thread's at once: they do not
  // depend on the action, and a load per loop iteration would wait out one
  // memory latency per iteration (stepper.hpp env_prefetch)
  const uint4* in = reinterpret_cast<const uint4*>(obs_in + (long long)n * in_stride);
  uint4 old[kGameWords];
#pragma unroll
  for (int i = 0; i < kGameWords; ++i) {
    const int g = threadIdx.x + kGameThreads * i;
    old[i] = in[g < kGameFrameWords ? g : 0];
  }
  const uint8_t was = st.done[n];
  const bool was_done = was != kRunning;
  int32_t k = st.episode[n];
  int32_t t = st.step[n];
  float total = st.total[n];
  int32_t* vars = st.vars + (long long)n * kGameInts;
  GameVars v = game_load(vars);
  const uint32_t action = (uint32_t)actions[n];
  __syncthreads();  // everyone's state reads before thread 0's state writes
  if (was == kGameOver) {  // _AutoResetWrapper: reset lazily at the next step
    k += 1;
    t = 0;
    total = 0.f;
    game_start(st.game, seed, e, (uint32_t)k, v);
  }
  // the reset frame's state, read only if was_done; after a lost life (kLifeLost) the
  // game goes on in place and the stack restarts from the respawned ball's frame
  const GameView first = game_view(st.game, v);
  t += 1;
  float rew;
  bool own, lost;
  game_advance(st.game, seed, e, (uint32_t)k, action, v, rew, own, lost);
  const GameCut cut = game_cut(st.game, rules.episodic_life, rules.max_steps, t, own, lost);
  const bool term = cut.term;
  const GameView now = game_view(st.game, v);
  uint4* out = reinterpret_cast<uint4*>(obs_out + (long long)n * out_stride);
#pragma unroll
  for (int i = 0; i < kGameWords; ++i) {
    const int g = threadIdx.x + kGameThreads * i;
    if (g >= kGameFrameWords) break;
    uint4 o = old[i];
    if (was_done) {  // FrameStackWrapper.reset: the reset frame repeated 4x
      const uint4 r = game_word(first, g);
      o = make_uint4(r.x * 0x01010101u, r.y * 0x01010101u, r.z * 0x01010101u, r.w * 0x01010101u);
    }
    const uint4 p = game_word(now, g);
    // np.roll(stack, -1, axis=-1); zero-fill on terminal; last channel = frame
    o.x = (term ? 0u : (o.x >> 8)) | (p.x << 24);
    o.y = (term ? 0u : (o.y >> 8)) | (p.y << 24);
    o.z = (term ? 0u : (o.z >> 8)) | (p.z << 24);
    o.w = (term ? 0u : (o.w >> 8)) | (p.w << 24);
    out[g] = o;
  }
  if (threadIdx.x == 0) {
    total += rew;
    rewards[n * ld] = rew;
    terminals[n * ld] = term ? 1 : 0;
    if (truncated) truncated[n * ld] = cut.trunc ? 1 : 0;
    // EpisodeInfoWrapper sits inside the life cut: whole-game totals, at a game over only
    ep_rewards[n * ld] = cut.over ? total : __int_as_float(0x7fc00000);
    st.episode[n] = k;
    st.step[n] = t;
    st.total[n] = cut.over ? 0.f : total;
    st.done[n] = cut.over ? kGameOver : (term ? kLifeLost : kRunning);
    game_store(vars, v);
  }
}

static bool game_state_ok(const acmi_game_state_t* st) {
  return st && st->episode && st->step && st->total && st->done && st->vars && st->game >= 0 &&
         st->game < kNumDeviceGames;
}

}  // namespace acmi

using namespace acmi;

extern "C" {

int acmi_game_state_ints(void) { return kGameInts; }
int64_t acmi_game_state_bytes(void) { return (int64_t)sizeof(acmi_game_state_t); }

int acmi_game_reset(const acmi_game_state_t* st, int N, int env_offset, uint32_t seed, uint8_t* obs_out,
                    int64_t out_stride, acmi_stream_t stream) {
  ACMI_REQUIRE(game_state_ok(st) && obs_out && N >= 0 && env_offset >= 0 && out_stride >= 84 * 84 * 4 &&
                   out_stride % 16 == 0,
               ACMI_ERR_ARG, "acmi_game_reset: bad arguments");
  if (N == 0) return ACMI_OK;
  hipLaunchKernelGGL(game_reset_kernel, dim3(N), dim3(kGameThreads), 0, (hipStream_t)stream, *st, env_offset,
                     seed, obs_out, (long long)out_stride);
  ACMI_LAUNCH_CHECK("acmi_game_reset");
  return ACMI_OK;
}

int acmi_game_step(const acmi_game_state_t* st, int N, int env_offset, uint32_t seed, const int32_t* actions,
                   const uint8_t* obs_in, int64_t in_stride, uint8_t* obs_out, int64_t out_stride,
                   float* rewards, uint8_t* terminals, float* episode_rewards, int64_t ld,
                   acmi_stream_t stream) {
  ACMI_REQUIRE(game_state_ok(st) && actions && obs_in && obs_out && rewards && terminals && episode_rewards &&
                   N >= 0 && env_offset >= 0 && in_stride >= 84 * 84 * 4 && out_stride >= 84 * 84 * 4 &&
                   in_stride % 16 == 0 && out_stride % 16 == 0 && ld >= 1,
               ACMI_ERR_ARG, "acmi_game_step: bad arguments");
  if (N == 0) return ACMI_OK;
  const acmi_game_rules_t rules = {0, 0};
  hipLaunchKernelGGL(game_step_kernel, dim3(N), dim3(kGameThreads), 0, (hipStream_t)stream, *st, rules,
                     env_offset, seed, actions, obs_in, (long long)in_stride, obs_out, (long long)out_stride,
                     rewards, terminals, (uint8_t*)nullptr, episode_rewards, (long long)ld);
  ACMI_LAUNCH_CHECK("acmi_game_step");
  return ACMI_OK;
}

int acmi_game_step_cuts(const acmi_game_state_t* st, const acmi_game_rules_t* rules, int N, int env_offset,
                        uint32_t seed, const int32_t* actions, const uint8_t* obs_in, int64_t in_stride,
                        uint8_t* obs_out, int64_t out_stride, float* rewards, uint8_t* terminals,
                        uint8_t* truncated, float* episode_rewards, int64_t ld, acmi_stream_t stream) {
  ACMI_REQUIRE(game_state_ok(st) && actions && obs_in && obs_out && rewards && terminals && episode_rewards &&
                   N >= 0 && env_offset >= 0 && in_stride >= 84 * 84 * 4 && out_stride >= 84 * 84 * 4 &&
                   in_stride % 16 == 0 && out_stride % 16 == 0 && ld >= 1,
               ACMI_ERR_ARG, "acmi_game_step_cuts: bad arguments");
  ACMI_REQUIRE(rules && (rules->episodic_life == 0 || rules->episodic_life == 1) && rules->max_steps >= 0 &&
                   rules->max_steps <= BREAKOUT_MAX_STEPS,
               ACMI_ERR_ARG, "acmi_game_step_cuts: rules: episodic_life 0 or 1, max_steps 0..2000");
  if (N == 0) return ACMI_OK;
  hipLaunchKernelGGL(game_step_kernel, dim3(N), dim3(kGameThreads), 0, (hipStream_t)stream, *st, *rules,
                     env_offset, seed, actions, obs_in, (long long)in_stride, obs_out, (long long)out_stride,
                     rewards, terminals, truncated, episode_rewards, (long long)ld);
  ACMI_LAUNCH_CHECK("acmi_game_step_cuts");
  return ACMI_OK;
}

}  // extern "C"
