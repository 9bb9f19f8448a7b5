// Device games: the integer dynamics and the renderer of Catch and
// Breakout.  The rule book is actorcritic/envs/games/host.py (HostGame); this is
// its restatement for the stepper in games.hip and must match it bit for bit
// (tests/test_gpu_games.py).  Everything here is wave-uniform: every thread of
// an env's workgroup advances the same few integers.
#pragma once

#include "common.hpp"

namespace acmi {

constexpr int kGameInts = 12;  // int32 per env in acmi_game_state_t.vars
constexpr int kNumDeviceGames = 2;
constexpr int kCatch = 0, kBreakout = 1;
constexpr uint32_t CATCH_TAG = 0xCA7C0000u;
constexpr uint32_t BREAKOUT_TAG = 0xB4EA0000u;
constexpr int32_t BREAKOUT_MAX_STEPS = 2000;
constexpr uint8_t kRunning = 0, kGameOver = 1, kLifeLost = 2;  // acmi_game_state_t.done

constexpr int kGameFrameWords = 84 * 84 / 4;  // 16-byte words of a stack: 4 pixels x 4 channels
constexpr int kGameThreads = 256;
constexpr int kGameWords = (kGameFrameWords + kGameThreads - 1) / kGameThreads;  // 7

// vars[0..8] of an env: ball (top-left, velocity), paddle x, lives, the brick
// bits (row r, column c: bit 12*(r % 2) + c of word r / 2); vars[9..11] stay 0
struct GameVars {
  int32_t bx, by, vx, vy, px, lives;
  uint32_t b0, b1, b2;
};

__device__ __forceinline__ GameVars game_load(const int32_t* p) {
  GameVars v;
  v.bx = p[0]; v.by = p[1]; v.vx = p[2]; v.vy = p[3]; v.px = p[4]; v.lives = p[5];
  v.b0 = (uint32_t)p[6]; v.b1 = (uint32_t)p[7]; v.b2 = (uint32_t)p[8];
  return v;
}
__device__ __forceinline__ void game_store(int32_t* p, const GameVars& v) {
  p[0] = v.bx; p[1] = v.by; p[2] = v.vx; p[3] = v.vy; p[4] = v.px; p[5] = v.lives;
  p[6] = (int32_t)v.b0; p[7] = (int32_t)v.b1; p[8] = (int32_t)v.b2;
  p[9] = p[10] = p[11] = 0;
}

__device__ __forceinline__ int32_t speed4(uint32_t i) {  // (-2, -1, 1, 2)[i]
  return i == 0u ? -2 : (i == 1u ? -1 : (i == 2u ? 1 : 2));
}

// the ball of episode k of global env e (Breakout: with v.lives left)
__device__ __forceinline__ void game_spawn_ball(int game, uint32_t seed, uint32_t e, uint32_t k, GameVars& v) {
  if (game == kCatch) {
    const uint32_t h = key4(seed, e, k, CATCH_TAG);
    v.bx = 4 * (int32_t)(h % 21u);
    v.by = 0;
    v.vx = 4 * ((int32_t)((h >> 8) % 3u) - 1);
    v.vy = 4;
  } else {
    const uint32_t h = key4(seed, e, k, BREAKOUT_TAG + (uint32_t)v.lives);
    v.bx = 2 * (int32_t)(h % 42u);
    v.by = 40;
    v.vx = speed4((h >> 8) & 3u);
    v.vy = 2;
  }
}

__device__ __forceinline__ void game_start(int game, uint32_t seed, uint32_t e, uint32_t k, GameVars& v) {
  v.px = 36;
  v.lives = game == kCatch ? 1 : 3;
  v.b0 = v.b1 = v.b2 = game == kCatch ? 0u : 0xFFFFFFu;
  game_spawn_ball(game, seed, e, k, v);
}

// One step of episode k under action a; -> reward, own (the game ended by its own
// rules: Catch's ball landed, Breakout ran out of lives or bricks; the step cap is
// the stepper's business, game_cut) and lost (a life went in this step).
__device__ __forceinline__ void game_advance(int game, uint32_t seed, uint32_t e, uint32_t k, uint32_t action,
                                             GameVars& v, float& rew, bool& own, bool& lost) {
  rew = 0.f;
  lost = false;
  if (game == kCatch) {
    const uint32_t a = action < 3u ? action : 0u;
    if (a == 1u) v.px = min(v.px + 4, 72);
    if (a == 2u) v.px = max(v.px - 4, 0);
    if (v.bx + v.vx < 0 || v.bx + v.vx > 80) v.vx = -v.vx;
    v.bx += v.vx;
    v.by += 4;
    own = v.by == 76;
    if (own) {
      const int32_t d = v.bx - v.px;
      rew = (d == 0 || d == 4 || d == 8) ? 1.f : -1.f;
    }
    return;
  }
  const uint32_t a = action < 4u ? action : 0u;
  if (a == 2u) v.px = min(v.px + 4, 72);
  if (a == 3u) v.px = max(v.px - 4, 0);
  if (v.bx + v.vx < 0 || v.bx + v.vx > 82) v.vx = -v.vx;
  v.bx += v.vx;
  if (v.by + v.vy < 0) v.vy = -v.vy;
  v.by += v.vy;
  const int32_t cy = v.by + (v.vy > 0 ? 1 : 0);
  if (cy >= 12 && cy < 30) {
    const int32_t r = (cy - 12) / 3, c = v.bx / 7;
    // rows 0..3 as one 48-bit word, rows 4..5 in b2: a word picked by index (or by a
    // three-way select, which the compiler turns into one) would go through scratch
    const uint64_t lo = (uint64_t)v.b0 | ((uint64_t)v.b1 << 24);
    const bool low = r < 4;
    const int32_t i = 12 * (low ? r : r - 4) + c;
    if (((low ? lo : (uint64_t)v.b2) >> i) & 1u) {
      const uint64_t left = (low ? lo : (uint64_t)v.b2) & ~(1ull << i);
      if (low) {
        v.b0 = (uint32_t)left & 0xFFFFFFu;
        v.b1 = (uint32_t)(left >> 24);
      } else {
        v.b2 = (uint32_t)left;
      }
      rew = 1.f;
      v.vy = -v.vy;
    }
  }
  const int32_t off = v.bx - v.px;
  if (v.vy > 0 && v.by == 78 && off >= -1 && off <= 11) {
    v.vy = -2;
    v.vx = speed4((uint32_t)((off + 1) * 4 / 13));
  }
  if (v.by >= 80) {
    v.lives -= 1;
    lost = true;
    if (v.lives > 0) game_spawn_ball(game, seed, e, k, v);
  }
  own = v.lives == 0 || (v.b0 | v.b1 | v.b2) == 0u;
}

// How step t (1-based) of an episode ends under the rules (host.py, "Cuts"): over = the
// game restarts at the next step, term = what the learner sees, trunc = the cap alone
// ended it.  max_steps 0: the game's own cap (Breakout 2000, Catch none).
struct GameCut {
  bool over, term, trunc;
};
__device__ __forceinline__ GameCut game_cut(int game, int32_t episodic_life, int32_t max_steps, int32_t t, bool own,
                                            bool lost) {
  const int32_t cap = max_steps > 0 ? max_steps : (game == kBreakout ? BREAKOUT_MAX_STEPS : 0x7fffffff);
  const bool capped = t >= cap;
  const bool life = episodic_life != 0 && lost;
  GameCut c;
  c.over = own || capped;
  c.term = c.over || life;
  c.trunc = capped && !own && !life;
  return c;
}

// what a thread needs to draw pixels of a state: sizes and, per pixel, a few compares
struct GameView {
  int32_t bx, by, bs, px, ph;
  uint64_t lo;  // brick rows 0..3 (48 bits)
  uint32_t b2;  // brick rows 4..5
  bool bricks;
};
__device__ __forceinline__ GameView game_view(int game, const GameVars& v) {
  GameView w;
  w.bx = v.bx; w.by = v.by; w.px = v.px;
  w.bs = game == kCatch ? 4 : 2;
  w.ph = game == kCatch ? 4 : 2;
  w.lo = (uint64_t)v.b0 | ((uint64_t)v.b1 << 24);
  w.b2 = v.b2;
  w.bricks = game == kBreakout;
  return w;
}
// The 4 pixels of 16-byte word g (84 = 4 * 21: a word never straddles a row).
// The row decides first: most words lie in no object's rows and cost three
// compares.  Drawn bricks, then paddle, then ball: the later one wins a pixel.
__device__ __forceinline__ uint4 game_word(const GameView& w, int g) {
  const int32_t row = g / 21, col = 4 * (g % 21);
  uint32_t p[4] = {0u, 0u, 0u, 0u};
  if (w.bricks && (uint32_t)(row - 12) < 18u) {
    const int32_t r = (row - 12) / 3;
    const uint32_t line = (uint32_t)((r < 4 ? w.lo : (uint64_t)w.b2) >> (12 * (r < 4 ? r : r - 4))) & 0xFFFu;
    const uint32_t shade = 100u + 20u * (uint32_t)r;
#pragma unroll
    for (int j = 0; j < 4; ++j) p[j] = ((line >> ((col + j) / 7)) & 1u) ? shade : 0u;
  }
  if ((uint32_t)(row - 80) < (uint32_t)w.ph) {
#pragma unroll
    for (int j = 0; j < 4; ++j) p[j] = (uint32_t)(col + j - w.px) < 12u ? 200u : p[j];
  }
  if ((uint32_t)(row - w.by) < (uint32_t)w.bs) {
#pragma unroll
    for (int j = 0; j < 4; ++j) p[j] = (uint32_t)(col + j - w.bx) < (uint32_t)w.bs ? 255u : p[j];
  }
  return make_uint4(p[0], p[1], p[2], p[3]);
}

// ---------------------------------------------------------------------------
// The env step, stated once for the stand-alone kernel (games.hip) and the fused
// rollout tails (forward.hpp, GameEnv), shaped like the synthetic stepper's
// env_prefetch / env_step_block_pre / env_step_part (stepper.hpp).
// ---------------------------------------------------------------------------

// The game of env n of the call, in two halves so that the load can be issued with the
// other state reads and waited for with them: game_byte is the load, game_of moves the
// wave-uniform value to a scalar register (a byte load has no scalar form), so every
// branch on the id stays a scalar branch.
__device__ __forceinline__ int game_byte(const uint8_t* games, int n) { return games ? (int)games[n] : 0; }
__device__ __forceinline__ int game_of(const uint8_t* games, int byte, int fallback) {
  return games ? __builtin_amdgcn_readfirstlane(byte) : fallback;
}

// Everything of a launch's game step that is not a per-env output pointer.  kPerEnv
// (the functions' template parameter): the game is read per env from `games`, which
// may still be NULL at run time (st.game for all); <false> never looks at it.
struct GameCall {
  acmi_game_state_t st;
  const uint8_t* games;
  int32_t* bad_envs;
  acmi_game_rules_t rules;
  uint32_t seed;
};

struct GamePre {  // an env's pre-step state and current stack words, loaded up front
  uint4 old[kGameWords];
  int gbyte;
  uint8_t was;
  int32_t k, t;
  float total;
  GameVars v;
};

// obs_in: env n's stack.  The env's game ahead of every other load: loads return in
// order, so the wait for this byte after the barrier then leaves the stack words in
// flight.  The previous stack's words next, all of a thread's at once: they do not
// depend on the action, and a load per loop iteration would wait out one memory
// latency per iteration (stepper.hpp env_prefetch).
template <bool kPerEnv>
__device__ __forceinline__ void game_prefetch(const GameCall& c, int n, const uint8_t* obs_in, GamePre& p) {
  p.gbyte = kPerEnv ? game_byte(c.games, n) : 0;
  const uint4* in = reinterpret_cast<const uint4*>(obs_in);
#pragma unroll
  for (int i = 0; i < kGameWords; ++i) {
    const int g = threadIdx.x + kGameThreads * i;
    p.old[i] = in[g < kGameFrameWords ? g : 0];
  }
  p.was = c.st.done[n];
  p.k = c.st.episode[n];
  p.t = c.st.step[n];
  p.total = c.st.total[n];
  p.v = game_load(c.st.vars + (long long)n * kGameInts);
}

// The integer half of a step from the pre-step state: the lazy reset, the advance and
// the cut.  In: k, t, total, v before the step; out: after it (total without the
// step's reward), with the two frames' views.
struct GameMove {
  float rew;
  GameCut cut;
  GameView first, now;  // the reset frame's state (read only after a done step) and the new frame's
};
__device__ __forceinline__ GameMove game_move(int game, const acmi_game_rules_t& rules, uint32_t seed, uint32_t e,
                                              uint32_t action, uint8_t was, int32_t& k, int32_t& t, float& total,
                                              GameVars& v) {
  GameMove m;
  if (was == kGameOver) {  // _AutoResetWrapper: reset lazily at the next step
    k += 1;
    t = 0;
    total = 0.f;
    game_start(game, seed, e, (uint32_t)k, v);
  }
  // the reset frame's state, read only if was_done; after a lost life (kLifeLost) the
  // game goes on in place and the stack restarts from the respawned ball's frame
  m.first = game_view(game, v);
  t += 1;
  bool own, lost;
  game_advance(game, seed, e, (uint32_t)k, action, v, m.rew, own, lost);
  m.cut = game_cut(game, rules.episodic_life, rules.max_steps, t, own, lost);
  m.now = game_view(game, v);
  return m;
}

// word g of the new stack from the old one: FrameStackWrapper.reset (the reset frame
// repeated 4x) after a done step, then np.roll(stack, -1, axis=-1) with zero-fill on a
// terminal and the new frame in the last channel; all zero for a bad env
__device__ __forceinline__ uint4 game_stack_word(const GameMove& m, bool was_done, bool bad, uint4 o, int g) {
  if (was_done) {
    const uint4 r = game_word(m.first, g);
    o = make_uint4(r.x * 0x01010101u, r.y * 0x01010101u, r.z * 0x01010101u, r.w * 0x01010101u);
  }
  const uint4 p = game_word(m.now, g);
  const bool term = m.cut.term;
  o.x = (term ? 0u : (o.x >> 8)) | (p.x << 24);
  o.y = (term ? 0u : (o.y >> 8)) | (p.y << 24);
  o.z = (term ? 0u : (o.z >> 8)) | (p.z << 24);
  o.w = (term ? 0u : (o.w >> 8)) | (p.w << 24);
  if (bad) o = make_uint4(0u, 0u, 0u, 0u);
  return o;
}

// what one thread of the env stores beside the stack; element n of an output at [n * ld]
struct GameOut {
  float* rewards;
  uint8_t* terminals;
  uint8_t* truncated;  // nullable
  float* ep_rewards;
  long long ld;
};
// -> the state after the step is to be stored (false: a bad env, whose state stays)
__device__ __forceinline__ bool game_store_step(const GameOut& out, int n, const GameMove& m, bool bad, float& total,
                                                int32_t* bad_envs) {
  if (bad) {
    out.rewards[n * out.ld] = 0.f;
    out.terminals[n * out.ld] = 0;
    if (out.truncated) out.truncated[n * out.ld] = 0;
    out.ep_rewards[n * out.ld] = __int_as_float(0x7fc00000);
    if (bad_envs) atomicAdd(bad_envs, 1);
    return false;
  }
  total += m.rew;
  out.rewards[n * out.ld] = m.rew;
  out.terminals[n * out.ld] = m.cut.term ? 1 : 0;
  if (out.truncated) out.truncated[n * out.ld] = m.cut.trunc ? 1 : 0;
  // EpisodeInfoWrapper sits inside the life cut: whole-game totals, at a game over only
  out.ep_rewards[n * out.ld] = m.cut.over ? total : __int_as_float(0x7fc00000);
  if (m.cut.over) total = 0.f;
  return true;
}
__device__ __forceinline__ uint8_t game_done_code(const GameCut& cut) {
  return cut.over ? kGameOver : (cut.term ? kLifeLost : kRunning);
}

// One env step of env n (global id e) by a whole 256-thread workgroup, from the state
// game_prefetch read; begins with the barrier that orders every thread's state reads
// before thread 0's state writes.  mirror (nullable): the new stack is also stored
// there, 16-byte word g at mirror[g] (the fused tail's next-step tower image in LDS).
// A bad env is not branched around (an early exit lets the compiler sink the state
// loads below the barrier, behind the wait for the id): it steps as some game in
// registers, and only what is stored differs.
template <bool kPerEnv>
__device__ __forceinline__ void game_step_block_pre(const GameCall& c, int n, uint32_t e, uint32_t action,
                                                    const GamePre& pre, uint8_t* obs_out, const GameOut& outs,
                                                    uint4* mirror = nullptr) {
  const bool was_done = pre.was != kRunning;
  int32_t k = pre.k;
  int32_t t = pre.t;
  float total = pre.total;
  GameVars v = pre.v;
  __syncthreads();  // everyone's state reads before thread 0's state writes
  const int game = kPerEnv ? game_of(c.games, pre.gbyte, c.st.game) : c.st.game;
  const bool bad = kPerEnv && (uint32_t)game >= (uint32_t)kNumDeviceGames;
  const GameMove m = game_move(game, c.rules, c.seed, e, action, pre.was, k, t, total, v);
  uint4* out = reinterpret_cast<uint4*>(obs_out);
#pragma unroll
  for (int i = 0; i < kGameWords; ++i) {
    const int g = threadIdx.x + kGameThreads * i;
    if (g >= kGameFrameWords) break;
    const uint4 o = game_stack_word(m, was_done, bad, pre.old[i], g);
    out[g] = o;
    if (mirror) mirror[g] = o;
  }
  if (threadIdx.x == 0 && game_store_step(outs, n, m, bad, total, c.bad_envs)) {
    c.st.episode[n] = k;
    c.st.step[n] = t;
    c.st.total[n] = total;
    c.st.done[n] = game_done_code(m.cut);
    game_store(c.st.vars + (long long)n * kGameInts, v);
  }
}

// The env step of one of several workgroups sharing env n (the split rollout step,
// towersplit.hpp), the games' env_step_part: every part reads the pre-step state (nobody
// writes it during the launch) and advances the integers redundantly, renders the new
// stack's words [g0, g1) into `mirror` (its LDS image) and files words [o0, o1) into
// obs_out (and the old ones into obs_copy, nullable); the writer also stores the reward,
// terminal, truncation and episode total, counts a bad env, and leaves the post-step
// state in pend[n] with flag = 1 (a bad env's state stays: nothing is left pending).
// game_commit_pending, run by the next step's fc4 launch, writes it into the state.
struct GamePend {  // 20 int32 = 80 bytes per env, 16-byte aligned
  int32_t k, t, total_bits, done;
  int32_t vars[kGameInts];
  int32_t flag, pad0, pad1, pad2;
};
static_assert(sizeof(GamePend) % 16 == 0, "a pending entry is whole 16-byte words");
__device__ __forceinline__ void game_step_part(const GameCall& c, int n, uint32_t e, uint32_t action,
                                               const uint8_t* obs_in, int g0, int g1, int o0, int o1, uint8_t* obs_out,
                                               uint8_t* obs_copy, uint4* mirror, bool writer, const GameOut& outs,
                                               GamePend* pend) {
  const int gbyte = game_byte(c.games, n);
  const uint8_t was = c.st.done[n];
  const bool was_done = was != kRunning;
  int32_t k = c.st.episode[n];
  int32_t t = c.st.step[n];
  float total = c.st.total[n];
  GameVars v = game_load(c.st.vars + (long long)n * kGameInts);
  const uint4* in = reinterpret_cast<const uint4*>(obs_in);
  uint4* out = reinterpret_cast<uint4*>(obs_out);
  constexpr int NW = (36 * 21 + kGameThreads - 1) / kGameThreads;  // a part's range: <= 36 rows of 21 words
  uint4 old[NW];
#pragma unroll
  for (int i = 0; i < NW; ++i) {
    const int g = g0 + (int)threadIdx.x + kGameThreads * i;
    old[i] = in[g < g1 ? g : g0];
  }
  const int game = game_of(c.games, gbyte, c.st.game);
  const bool bad = (uint32_t)game >= (uint32_t)kNumDeviceGames;
  const GameMove m = game_move(game, c.rules, c.seed, e, action, was, k, t, total, v);
#pragma unroll
  for (int i = 0; i < NW; ++i) {
    const int g = g0 + (int)threadIdx.x + kGameThreads * i;
    if (g >= g1) break;
    const bool own = g >= o0 && g < o1;
    if (obs_copy && own) reinterpret_cast<uint4*>(obs_copy)[g] = old[i];
    const uint4 o = game_stack_word(m, was_done, bad, old[i], g);
    mirror[g] = o;
    if (own) out[g] = o;
  }
  if (writer && threadIdx.x == 0 && game_store_step(outs, n, m, bad, total, c.bad_envs)) {
    GamePend ps;
    ps.k = k;
    ps.t = t;
    ps.total_bits = __float_as_int(total);
    ps.done = game_done_code(m.cut);
    game_store(ps.vars, v);
    ps.flag = 1;
    ps.pad0 = ps.pad1 = ps.pad2 = 0;
    pend[n] = ps;
  }
}
// the pending post-step states of envs 0 .. B-1 into st (one thread per env)
__device__ __forceinline__ void game_commit_pending(const acmi_game_state_t& st, GamePend* pend, int B) {
  for (int n = threadIdx.x; n < B; n += blockDim.x) {
    if (!pend[n].flag) continue;
    const GamePend ps = pend[n];
    st.episode[n] = ps.k;
    st.step[n] = ps.t;
    st.total[n] = __int_as_float(ps.total_bits);
    st.done[n] = (uint8_t)ps.done;
    int32_t* vars = st.vars + (long long)n * kGameInts;
#pragma unroll
    for (int i = 0; i < kGameInts; ++i) vars[i] = ps.vars[i];
    pend[n].flag = 0;
  }
}

}  // namespace acmi
