// mz_breakout.h -- Breakout (MZ_ENV_BREAKOUT): a brick-breaking image game on the device, on mz_catch.h's pattern: the host-stepped path's
// own kernels around an env that lives on the device.  Unlike Catch it pays rewards during the episode (1 per brick), its episodes end on a
// miss or on a move cap, and their lengths differ from env to env.
//
// The game (games.BreakoutEnv is the specification): a rows x cols grid (cols <= 32) of cell_h x cell_w pixel cells, one uint8 frame
// [1, H, W].  Bricks fill rows 1 .. K (K = brick_rows, 1..3; one 32-bit mask per row, bit c = column c), row 0 is empty, the paddle lives
// in row rows - 1.  The ball (bx, by) moves diagonally: d = 0 up-left, 1 up-right, 2 down-right, 3 down-left.  A move, in this order:
//   1. px = clip(px + a - 1, 0, cols - 1)                                   (a: 0 left, 1 stay, 2 right)
//   2. (nx, ny) = (bx, by) + delta[d], reward = 0
//   3. nx off the grid: clamp it, d = flipx[d]
//   4. exactly one of:  ny < 0                 -> ny = 0, d = flipy[d]
//                       a brick at (ny, nx)    -> remove it, reward = 1, ny = by, d = flipy[d]
//                       ny == rows - 1         -> refill rows 1 .. K if no brick is left; then bx == px: d = flipy[d], ny = by;
//                                                 else nx == px: d = flipboth[d], ny = by; else the episode ends (reward 0)
//                       otherwise nothing
//   5. trail (lx, ly) = (bx, by), (bx, by) = (nx, ny), t += 1
//   6. t == max_moves ends the episode (a brick reward and the cap may fall on the same move)
// Reset with start code k in 0 .. 2 cols - 1: bx = k >> 1, by = K + 1, d = 2 + (k & 1), px = cols / 2, trail = ball, all bricks, t = 0.
// In self-play k = min(2 cols - 1, floor(u * 2 cols)), u the first double of Philox(seed, env, episode, BREAKOUT_STREAM); no stagger
// (episode lengths already differ).  Frame: background 0, bricks 96, trail cell 64, paddle cell 160, ball cell 255; where cells coincide
// the priority is ball, paddle, trail, brick.  Mask all legal, players 1 / 1.  A finished env restarts at once.
//
//   k_breakout_reset      : episode 0 of every env -- start codes drawn (self-play) or uploaded (arena: no Philox draw) -- with the all-legal
//                           mask and the player ids of the mode's own buffers
//   k_breakout_step       : one thread per env.  Writes ext.reward / ext.done and, for a finished env, the next episode's state
//                           (k_ext_commit, after it, bumps episode[])
//   k_breakout_render     : the one kernel that moves bytes; k_catch_render's form.  The frames are one flat byte array, a lane owns one
//                           16-byte run of it, divides once for its first byte and walks the other 15 with counters, so a run may cross
//                           cells, pixel rows and envs; it stores one uint4, so a wave's store is 1 KiB contiguous.  A byte's value is the
//                           five-level rule above, recomputed when the walk enters another cell; the brick test is a bit test on the
//                           row's mask.
//   k_breakout_arena_step : mz_arena_image.h's ply record, then the step without restart: a finished game's state stays as it was, so the
//                           renderer repeats its last frame, which the root builder no longer reads
#pragma once
#include "mz_arena_image.h"

namespace mz {

constexpr int ENV_BREAKOUT = 7;
constexpr int IMGARENA_BREAKOUT = 3;  // the image arena's third front end (IMGARENA_CATCH, IMGARENA_EXTERNAL: mz_arena_image.h)
constexpr unsigned BREAKOUT_STREAM = 0x71000000u;  // the start code's Philox stream (0x4.., 0x5.., 0x60.., 0x61.., 0x70.. are taken)
constexpr int BREAKOUT_FIELDS = 10;                // ints per env in BreakoutEnv::s

struct BreakoutEnv {
    int rows, cols, K, max_moves;  // grid, brick rows, move cap
    int ch, cw;                    // cell size in pixels
    int H, W, FE;                  // frame height, width, bytes (H * W)
    int B;
    int* s;  // [BREAKOUT_FIELDS][B]: bx, by, d, px, lx, ly, t, brick row masks 0..2
};

enum { BO_BX = 0, BO_BY, BO_D, BO_PX, BO_LX, BO_LY, BO_T, BO_BRICK };

struct BreakoutLaunch {
    BreakoutEnv c;
    int B;
    unsigned long long seed;
    const int* action;        // [B] the search's sampled actions
    const unsigned* episode;  // [B] EnvState::episode (bumped by k_ext_commit, after the step)
    const int* start;         // arena reset only: [B] uploaded start codes (null: drawn)
    float* reward;            // ExtEnv::reward
    unsigned char* done;      // ExtEnv::done
    unsigned char* frames;    // ExtEnv::frames, [pad16(B * FE)]
    unsigned char* mask;      // resets only: [B][3] all legal
    int* cur;                 // resets only: [B] player ids 1 / 1
    int* opp;
};

struct BreakoutArenaLaunch {
    ImgArenaLaunch R;  // (R.c unused)
    BreakoutEnv c;
};

__device__ __forceinline__ int& breakout_field(const BreakoutEnv& c, int f, int e) { return c.s[(size_t)f * c.B + e]; }
__device__ __forceinline__ unsigned breakout_full_row(const BreakoutEnv& c) { return c.cols == 32 ? 0xffffffffu : (1u << c.cols) - 1u; }

__device__ __forceinline__ int breakout_start_code(const BreakoutLaunch& G, int e, unsigned episode) {
    Philox g(G.seed, (unsigned)e, episode, BREAKOUT_STREAM);
    const int n = 2 * G.c.cols, k = (int)floor(g.uniform() * (double)n);
    return k < n - 1 ? k : n - 1;
}

__device__ inline void breakout_start(const BreakoutEnv& c, int e, int k) {
    const int bx = k >> 1, by = c.K + 1;
    breakout_field(c, BO_BX, e) = bx;
    breakout_field(c, BO_BY, e) = by;
    breakout_field(c, BO_D, e) = 2 + (k & 1);
    breakout_field(c, BO_PX, e) = c.cols / 2;
    breakout_field(c, BO_LX, e) = bx;
    breakout_field(c, BO_LY, e) = by;
    breakout_field(c, BO_T, e) = 0;
    for (int r = 0; r < 3; r++) breakout_field(c, BO_BRICK + r, e) = r < c.K ? (int)breakout_full_row(c) : 0;
}

// One move of env e with action a.  A game that goes on has its new state stored; a finished one is left as it was (the caller restarts
// or freezes it).  Returns done.
__device__ inline bool breakout_move(const BreakoutEnv& c, int e, int a, float& reward) {
    int px = breakout_field(c, BO_PX, e) + a - 1;
    px = px < 0 ? 0 : (px > c.cols - 1 ? c.cols - 1 : px);
    const int bx = breakout_field(c, BO_BX, e), by = breakout_field(c, BO_BY, e);
    int d = breakout_field(c, BO_D, e);
    unsigned br[3];
    for (int r = 0; r < 3; r++) br[r] = (unsigned)breakout_field(c, BO_BRICK + r, e);
    int nx = bx + ((d == 1 || d == 2) ? 1 : -1), ny = by + (d >= 2 ? 1 : -1);
    reward = 0.0f;
    bool done = false;
    if (nx < 0 || nx > c.cols - 1) {
        nx = nx < 0 ? 0 : c.cols - 1;
        d ^= 1;  // flipx = (1, 0, 3, 2)
    }
    const int brow = ny - 1;  // the brick row ny would enter
    if (ny < 0) {
        ny = 0;
        d = 3 - d;  // flipy = (3, 2, 1, 0)
    } else if (brow >= 0 && brow < c.K && (((brow == 0 ? br[0] : (brow == 1 ? br[1] : br[2])) >> nx) & 1u)) {
        const unsigned bit = 1u << nx;
        if (brow == 0) br[0] &= ~bit;
        else if (brow == 1) br[1] &= ~bit;
        else br[2] &= ~bit;
        reward = 1.0f;
        ny = by;
        d = 3 - d;
    } else if (ny == c.rows - 1) {
        if ((br[0] | br[1] | br[2]) == 0u)
            for (int r = 0; r < 3; r++) br[r] = r < c.K ? breakout_full_row(c) : 0u;
        if (bx == px) { d = 3 - d; ny = by; }
        else if (nx == px) { d ^= 2; ny = by; }  // flipboth = (2, 3, 0, 1)
        else done = true;
    }
    const int t = breakout_field(c, BO_T, e) + 1;
    if (t == c.max_moves) done = true;
    if (!done) {
        breakout_field(c, BO_PX, e) = px;
        breakout_field(c, BO_LX, e) = bx;
        breakout_field(c, BO_LY, e) = by;
        breakout_field(c, BO_BX, e) = nx;
        breakout_field(c, BO_BY, e) = ny;
        breakout_field(c, BO_D, e) = d;
        breakout_field(c, BO_T, e) = t;
        for (int r = 0; r < 3; r++) breakout_field(c, BO_BRICK + r, e) = (int)br[r];
    }
    return done;
}

__global__ void k_breakout_reset(const BreakoutLaunch G) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= G.B) return;
    breakout_start(G.c, e, G.start ? G.start[e] : breakout_start_code(G, e, 0u));
    for (int a = 0; a < 3; a++) G.mask[(size_t)e * 3 + a] = 1;
    G.cur[e] = 1;
    G.opp[e] = 1;
}

__global__ void k_breakout_step(const BreakoutLaunch G) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= G.B) return;
    float reward;
    const bool done = breakout_move(G.c, e, G.action[e], reward);
    G.reward[e] = reward;
    G.done[e] = done ? 1 : 0;
    if (done) breakout_start(G.c, e, breakout_start_code(G, e, G.episode[e] + 1u));
}

// what the renderer needs of one env
struct BreakoutView {
    int bx, by, px, lx, ly;
    unsigned br[3];
};

__device__ __forceinline__ BreakoutView breakout_view(const BreakoutEnv& c, int e) {
    BreakoutView v;
    v.bx = breakout_field(c, BO_BX, e); v.by = breakout_field(c, BO_BY, e); v.px = breakout_field(c, BO_PX, e);
    v.lx = breakout_field(c, BO_LX, e); v.ly = breakout_field(c, BO_LY, e);
    for (int r = 0; r < 3; r++) v.br[r] = (unsigned)breakout_field(c, BO_BRICK + r, e);
    return v;
}

__device__ __forceinline__ uint32_t breakout_cell(const BreakoutEnv& c, const BreakoutView& v, int cy, int cx) {
    if (cy == v.by && cx == v.bx) return 255u;
    if (cy == c.rows - 1 && cx == v.px) return 160u;
    if (cy == v.ly && cx == v.lx) return 64u;
    const unsigned m = cy == 1 ? v.br[0] : (cy == 2 ? v.br[1] : (cy == 3 ? v.br[2] : 0u));  // (rows past K hold 0)
    return ((m >> cx) & 1u) ? 96u : 0u;
}

__global__ __launch_bounds__(256) void k_breakout_render(const BreakoutLaunch G) {
    const BreakoutEnv& c = G.c;
    const size_t total = (size_t)G.B * c.FE, i0 = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 16;
    if (i0 >= total) return;  // (the last run starts inside the last env; its bytes past `total` lie in the allocation's padding)
    int e = (int)(i0 / c.FE);
    const int j = (int)(i0 - (size_t)e * c.FE);
    int row = j / c.W, col = j - row * c.W;
    int cy = row / c.ch, ry = row - cy * c.ch;  // cell row, pixel row inside the cell
    int cx = col / c.cw, rx = col - cx * c.cw;  // cell column, pixel column inside the cell
    BreakoutView v = breakout_view(c, e);
    uint32_t val = breakout_cell(c, v, cy, cx);
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int q = 0; q < 16; q++) {
        w[q >> 2] |= val << (8 * (q & 3));
        bool moved = false;
        if (++rx == c.cw) { rx = 0; cx++; moved = true; }
        if (++col == c.W) {
            col = cx = rx = 0;
            moved = true;
            ++row;
            if (++ry == c.ch) { ry = 0; cy++; }
            if (row == c.H) {
                row = cy = ry = 0;
                if (++e < G.B) v = breakout_view(c, e);
            }
        }
        if (moved) val = e < G.B ? breakout_cell(c, v, cy, cx) : 0u;
    }
    *reinterpret_cast<uint4*>(G.frames + i0) = make_uint4(w[0], w[1], w[2], w[3]);
}

__global__ void k_breakout_arena_step(const BreakoutArenaLaunch Q) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= Q.R.L.B || !Q.R.a.live[e]) return;
    const int a = imgarena_record(Q.R, e);
    float reward;
    const bool done = breakout_move(Q.c, e, a, reward);
    imgarena_outcome(Q.R, e, reward, done);
}

}  // namespace mz
