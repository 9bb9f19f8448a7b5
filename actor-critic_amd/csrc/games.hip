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

// The game of env n of the call, in two halves so that the load can be issued with the
// other state reads and waited for with them: game_byte is the load, game_of moves the
// wave-uniform value to a scalar register (a byte load has no scalar form), so every
// branch on the id stays a scalar branch.
__device__ __forceinline__ int game_byte(const uint8_t* games, int n) { return games ? (int)games[n] : 0; }
__device__ __forceinline__ int game_of(const uint8_t* games, int byte, int fallback) {
  return games ? __builtin_amdgcn_readfirstlane(byte) : fallback;
}

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
  const uint32_t e = (uint32_t)(env_offset + n);
  // the env's game ahead of every other load: loads return in order, so the wait for
  // this byte after the barrier then leaves the stack words in flight
  const int gbyte = kPerEnv ? game_byte(games, n) : 0;
  // the previous stack's words next, all of a thread's at once: they do not
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
  const int game = kPerEnv ? game_of(games, gbyte, st.game) : st.game;
  // A bad env is not branched around (an early exit lets the compiler sink the state
  // loads below the barrier, behind the wait for the id): it steps as some game in
  // registers, and only what is stored differs.
  const bool bad = kPerEnv && (uint32_t)game >= (uint32_t)kNumDeviceGames;
  if (was == kGameOver) {  // _AutoResetWrapper: reset lazily at the next step
    k += 1;
    t = 0;
    total = 0.f;
    game_start(game, seed, e, (uint32_t)k, v);
  }
  // the reset frame's state, read only if was_done; after a lost life (kLifeLost) the
  // game goes on in place and the stack restarts from the respawned ball's frame
  const GameView first = game_view(game, v);
  t += 1;
  float rew;
  bool own, lost;
  game_advance(game, seed, e, (uint32_t)k, action, v, rew, own, lost);
  const GameCut cut = game_cut(game, rules.episodic_life, rules.max_steps, t, own, lost);
  const bool term = cut.term;
  const GameView now = game_view(game, v);
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
    if (bad) o = make_uint4(0u, 0u, 0u, 0u);
    out[g] = o;
  }
  if (threadIdx.x == 0 && bad) {
    rewards[n * ld] = 0.f;
    terminals[n * ld] = 0;
    if (truncated) truncated[n * ld] = 0;
    ep_rewards[n * ld] = __int_as_float(0x7fc00000);
    if (bad_envs) atomicAdd(bad_envs, 1);
  } else if (threadIdx.x == 0) {
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
