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
// acmi_game_*_mixed are the same two kernels with the game read per env from a byte
// array (`games`; NULL: st.game for all), so one launch steps Catch and Breakout envs
// side by side.  An id at or past kNumDeviceGames is a bad env: state untouched, stack
// zero-filled, reward 0, no terminal, NaN episode reward, counted in bad_envs.
// One 256-thread workgroup per env, one launch per step, 28 KB in and 28 KB out
// per env.
#include "games.hpp"

namespace acmi {

// A bad env's reset (games.hip, top): the whole block takes this path or none does.
__device__ __forceinline__ void game_bad_env(uint8_t* obs, int32_t* bad_envs) {
  uint4* out = reinterpret_cast<uint4*>(obs);
  for (int g = threadIdx.x; g < kGameFrameWords; g += kGameThreads) out[g] = make_uint4(0u, 0u, 0u, 0u);
  if (threadIdx.x == 0 && bad_envs) atomicAdd(bad_envs, 1);
}

__global__ __launch_bounds__(kGameThreads) void game_reset_kernel(acmi_game_state_t st, const uint8_t* games,
                                                                  int32_t* bad_envs, int env_offset,
                                                                  uint32_t seed, uint8_t* obs, long long stride) {
  const int n = blockIdx.x;
  const int game = game_of(games, game_byte(games, n), st.game);
  if ((uint32_t)game >= (uint32_t)kNumDeviceGames) {
    game_bad_env(obs + (long long)n * stride, bad_envs);
    return;
  }
  GameVars v;
  game_start(game, seed, (uint32_t)(env_offset + n), 0u, v);
  const GameView w = game_view(game, v);
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

// All three entry points launch this kernel: acmi_game_step with rules {0, 0} and no
// truncated array, under which term == over and done never holds kLifeLost; the old
// two without games.  kPerEnv: the game is read per env (games != NULL); the <false>
// form is the single-game kernel as it was before `games` (a run-time test of the
// pointer cost it 0.4 us a launch at 1024 Breakout envs: DESIGN.md 7d, "Mixed batches").
template <bool kPerEnv>
__global__ __launch_bounds__(kGameThreads) void game_step_kernel(
    acmi_game_state_t st, const uint8_t* games, int32_t* bad_envs, acmi_game_rules_t rules, int env_offset,
    uint32_t seed, const int32_t* actions, const uint8_t* obs_in, long long in_stride, uint8_t* obs_out,
    long long out_stride, float* rewards, uint8_t* terminals, uint8_t* truncated, float* ep_rewards, long long ld) {
  const int n = blockIdx.x;
  const GameCall c{st, games, bad_envs, rules, seed};
  GamePre pre;
  game_prefetch<kPerEnv>(c, n, obs_in + (long long)n * in_stride, pre);
  const uint32_t action = (uint32_t)actions[n];
  game_step_block_pre<kPerEnv>(c, n, (uint32_t)(env_offset + n), action, pre, obs_out + (long long)n * out_stride,
                               GameOut{rewards, terminals, truncated, ep_rewards, ld});
}

static void launch_game_step(const acmi_game_state_t& st, const uint8_t* games, int32_t* bad_envs,
                             const acmi_game_rules_t& rules, int N, int env_offset, uint32_t seed,
                             const int32_t* actions, const uint8_t* obs_in, int64_t in_stride, uint8_t* obs_out,
                             int64_t out_stride, float* rewards, uint8_t* terminals, uint8_t* truncated,
                             float* episode_rewards, int64_t ld, acmi_stream_t stream) {
  auto kernel = games ? game_step_kernel<true> : game_step_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3(N), dim3(kGameThreads), 0, (hipStream_t)stream, st, games, bad_envs, rules,
                     env_offset, seed, actions, obs_in, (long long)in_stride, obs_out, (long long)out_stride, rewards,
                     terminals, truncated, episode_rewards, (long long)ld);
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
  hipLaunchKernelGGL(game_reset_kernel, dim3(N), dim3(kGameThreads), 0, (hipStream_t)stream, *st,
                     (const uint8_t*)nullptr, (int32_t*)nullptr, env_offset, seed, obs_out, (long long)out_stride);
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
  launch_game_step(*st, nullptr, nullptr, rules, N, env_offset, seed, actions, obs_in, in_stride, obs_out, out_stride,
                   rewards, terminals, nullptr, episode_rewards, ld, stream);
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
  launch_game_step(*st, nullptr, nullptr, *rules, N, env_offset, seed, actions, obs_in, in_stride, obs_out,
                   out_stride, rewards, terminals, truncated, episode_rewards, ld, stream);
  ACMI_LAUNCH_CHECK("acmi_game_step_cuts");
  return ACMI_OK;
}

int acmi_game_count(void) { return kNumDeviceGames; }

int acmi_game_actions(int game) {
  ACMI_REQUIRE(game >= 0 && game < kNumDeviceGames, ACMI_ERR_ARG, "acmi_game_actions: no such game");
  return game == kCatch ? 3 : 4;
}

int acmi_game_reset_mixed(const acmi_game_state_t* st, const uint8_t* games, int N, int env_offset, uint32_t seed,
                          uint8_t* obs_out, int64_t out_stride, int32_t* bad_envs, acmi_stream_t stream) {
  ACMI_REQUIRE(game_state_ok(st) && obs_out && N >= 0 && env_offset >= 0 && out_stride >= 84 * 84 * 4 &&
                   out_stride % 16 == 0,
               ACMI_ERR_ARG, "acmi_game_reset_mixed: bad arguments");
  if (N == 0) return ACMI_OK;
  hipLaunchKernelGGL(game_reset_kernel, dim3(N), dim3(kGameThreads), 0, (hipStream_t)stream, *st, games, bad_envs,
                     env_offset, seed, obs_out, (long long)out_stride);
  ACMI_LAUNCH_CHECK("acmi_game_reset_mixed");
  return ACMI_OK;
}

int acmi_game_step_mixed(const acmi_game_state_t* st, const uint8_t* games, const acmi_game_rules_t* rules, int N,
                         int env_offset, uint32_t seed, const int32_t* actions, const uint8_t* obs_in,
                         int64_t in_stride, uint8_t* obs_out, int64_t out_stride, float* rewards,
                         uint8_t* terminals, uint8_t* truncated, float* episode_rewards, int64_t ld,
                         int32_t* bad_envs, acmi_stream_t stream) {
  ACMI_REQUIRE(game_state_ok(st) && actions && obs_in && obs_out && rewards && terminals && episode_rewards &&
                   N >= 0 && env_offset >= 0 && in_stride >= 84 * 84 * 4 && out_stride >= 84 * 84 * 4 &&
                   in_stride % 16 == 0 && out_stride % 16 == 0 && ld >= 1,
               ACMI_ERR_ARG, "acmi_game_step_mixed: bad arguments");
  ACMI_REQUIRE(rules && (rules->episodic_life == 0 || rules->episodic_life == 1) && rules->max_steps >= 0 &&
                   rules->max_steps <= BREAKOUT_MAX_STEPS,
               ACMI_ERR_ARG, "acmi_game_step_mixed: rules: episodic_life 0 or 1, max_steps 0..2000");
  if (N == 0) return ACMI_OK;
  launch_game_step(*st, games, bad_envs, *rules, N, env_offset, seed, actions, obs_in, in_stride, obs_out, out_stride,
                   rewards, terminals, truncated, episode_rewards, ld, stream);
  ACMI_LAUNCH_CHECK("acmi_game_step_mixed");
  return ACMI_OK;
}

}  // extern "C"
