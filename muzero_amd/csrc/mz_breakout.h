// mz_breakout.h -- Breakout (MZ_ENV_BREAKOUT): a brick-breaking image game on the device, on mz_grid_game.h's kernels: the host-stepped
// path's own kernels around an env that lives on the device.  Unlike Catch it pays rewards during the episode (1 per brick), its episodes
// end on a miss or on a move cap, and their lengths differ from env to env.
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
// The state is ten ints per env: bx, by, d, px, lx, ly, t and the brick row masks 0..2.  The renderer's brick test is a bit test on the row's
// mask.
#pragma once
#include "mz_grid_game.h"

namespace mz {

constexpr int ENV_BREAKOUT = 7;
constexpr int IMGARENA_BREAKOUT = 3;  // the image arena's third front end (IMGARENA_CATCH, IMGARENA_EXTERNAL: mz_arena_image.h)
constexpr unsigned BREAKOUT_STREAM = 0x71000000u;  // the start code's Philox stream (0x4.., 0x5.., 0x60.., 0x61.., 0x70.. are taken)

struct Breakout : GridGame {
    int K, max_moves;  // brick rows, move cap
    enum { BX = 0, BY, D, PX, LX, LY, T, BRICK, FIELDS = BRICK + 3 };
    static constexpr unsigned STREAM = BREAKOUT_STREAM;
    static constexpr int KIND = ENV_BREAKOUT, ARENA = IMGARENA_BREAKOUT;
    static constexpr const char *NAME = "Breakout", *STRUCT = "mz_breakout_env", *OBS_VALUES = "frame bytes / 255, action planes of 1/3, 2/3";

    __device__ __forceinline__ unsigned full_row() const { return cols == 32 ? 0xffffffffu : (1u << cols) - 1u; }

    __device__ __forceinline__ int code(double u, int, unsigned) const {
        const int n = 2 * cols, k = (int)floor(u * (double)n);
        return k < n - 1 ? k : n - 1;
    }

    __device__ inline void start(int e, int k) const {
        const int bx = k >> 1, by = K + 1;
        field(BX, e) = bx;
        field(BY, e) = by;
        field(D, e) = 2 + (k & 1);
        field(PX, e) = cols / 2;
        field(LX, e) = bx;
        field(LY, e) = by;
        field(T, e) = 0;
        for (int r = 0; r < 3; r++) field(BRICK + r, e) = r < K ? (int)full_row() : 0;
    }

    __device__ inline bool move(int e, int a, float& reward) const {
        int px = field(PX, e) + a - 1;
        px = px < 0 ? 0 : (px > cols - 1 ? cols - 1 : px);
        const int bx = field(BX, e), by = field(BY, e);
        int d = field(D, e);
        unsigned br[3];
        for (int r = 0; r < 3; r++) br[r] = (unsigned)field(BRICK + r, e);
        int nx = bx + ((d == 1 || d == 2) ? 1 : -1), ny = by + (d >= 2 ? 1 : -1);
        reward = 0.0f;
        bool done = false;
        if (nx < 0 || nx > cols - 1) {
            nx = nx < 0 ? 0 : cols - 1;
            d ^= 1;  // flipx = (1, 0, 3, 2)
        }
        const int brow = ny - 1;  // the brick row ny would enter
        if (ny < 0) {
            ny = 0;
            d = 3 - d;  // flipy = (3, 2, 1, 0)
        } else if (brow >= 0 && brow < K && (((brow == 0 ? br[0] : (brow == 1 ? br[1] : br[2])) >> nx) & 1u)) {
            const unsigned bit = 1u << nx;
            if (brow == 0) br[0] &= ~bit;
            else if (brow == 1) br[1] &= ~bit;
            else br[2] &= ~bit;
            reward = 1.0f;
            ny = by;
            d = 3 - d;
        } else if (ny == rows - 1) {
            if ((br[0] | br[1] | br[2]) == 0u)
                for (int r = 0; r < 3; r++) br[r] = r < K ? full_row() : 0u;
            if (bx == px) { d = 3 - d; ny = by; }
            else if (nx == px) { d ^= 2; ny = by; }  // flipboth = (2, 3, 0, 1)
            else done = true;
        }
        const int t = field(T, e) + 1;
        if (t == max_moves) done = true;
        if (!done) {
            field(PX, e) = px;
            field(LX, e) = bx;
            field(LY, e) = by;
            field(BX, e) = nx;
            field(BY, e) = ny;
            field(D, e) = d;
            field(T, e) = t;
            for (int r = 0; r < 3; r++) field(BRICK + r, e) = (int)br[r];
        }
        return done;
    }

    struct View {
        int bx, by, px, lx, ly;
        unsigned br[3];
    };
    __device__ __forceinline__ View view(int e) const {
        View v;
        v.bx = field(BX, e); v.by = field(BY, e); v.px = field(PX, e);
        v.lx = field(LX, e); v.ly = field(LY, e);
        for (int r = 0; r < 3; r++) v.br[r] = (unsigned)field(BRICK + r, e);
        return v;
    }
    __device__ __forceinline__ uint32_t cell(const View& v, int cy, int cx) const {
        if (cy == v.by && cx == v.bx) return 255u;
        if (cy == rows - 1 && cx == v.px) return 160u;
        if (cy == v.ly && cx == v.lx) return 64u;
        const unsigned m = cy == 1 ? v.br[0] : (cy == 2 ? v.br[1] : (cy == 3 ? v.br[2] : 0u));  // (rows past K hold 0)
        return ((m >> cx) & 1u) ? 96u : 0u;
    }
};

}  // namespace mz
