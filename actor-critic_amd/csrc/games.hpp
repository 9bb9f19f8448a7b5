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

}  // namespace acmi
