// mz_grid_game.h -- what the device image games (mz_catch.h, mz_breakout.h) share: a one-player game on a rows x cols grid of ch x cw pixel
// cells, drawn as one uint8 frame [1, H, W] per env, with 3 actions that are always legal.  A move is mz_extenv.h's act and commit with the
// PCIe copies replaced by two kernels, the step and the renderer; the arena's ply (mz_arena_image.h) takes the step without restart.
//
// A game is a type G derived from GridGame (the geometry and the state array) that adds its own parameters and
//   G::FIELDS, G::STREAM                   ints of state per env; the Philox stream of the start code's draw
//   int  code(u, e, episode)               the start code of env e's episode from the uniform draw u (self-play)
//   void start(e, code)                    the episode's first state
//   bool move(e, a, float& reward)         one move with action a; stores the new state only when the game goes on; returns done
//   G::View view(e), uint32 cell(v, cy, cx)  what the renderer loads of one env, and the byte value of its cell (cy, cx)
// All are __device__ const members; the state is reached through field(f, e).  For the host's resets a game also names itself: G::KIND
// (the MZ_ENV_ value), G::ARENA (the IMGARENA_ mode), G::NAME, G::STRUCT (its public env struct) and G::OBS_VALUES (what its observations
// hold besides 0 and 1, for the refusal of int8 replay states).
//
//   k_game_reset<G>      : episode 0 of every env -- start codes drawn (self-play) or uploaded (arena: no Philox draw) -- with the all-legal
//                          mask and the player ids of the mode's own buffers
//   k_game_step<G>       : one thread per env.  Reads the sampled action, moves, writes ext.reward / ext.done (what the host's commit
//                          uploads) and, for a finished env, the next episode's state.  k_ext_commit (after it) bumps episode[].
//   k_game_render<G>     : paints every env's next frame into ext.frames (what the host's act uploads).  The only kernel here that moves bytes
//                          (C4: 512 x 9 216 B per move): the frames are one flat byte array, a lane owns one 16-byte run of it and stores
//                          one uint4, so a wave's store is 1 KiB contiguous.  A lane divides once for its first byte (env, pixel row, pixel
//                          column, cell row, cell column) and walks the other 15 with counters, so runs that cross a cell, a pixel row or
//                          an env (cell_w or W no multiple of 16) need no path of their own.  The byte value is recomputed when the walk
//                          enters another cell.  The array is allocated rounded up to 16 bytes; the bytes past the last env are written 0.
//   k_game_arena_step<G> : mz_arena_image.h's ply record, then the move without restart: a finished game's state stays as it was, so the
//                          renderer (which paints every env) repeats its last frame, which the root builder no longer reads
#pragma once
#include "mz_arena_image.h"

namespace mz {

struct GridGame {
    int rows, cols, ch, cw;  // grid and cell size in pixels
    int H, W, FE;            // frame height, width, bytes (H * W)
    int B;
    int* s;  // [G::FIELDS][B]
    __device__ __forceinline__ int& field(int f, int e) const { return s[(size_t)f * B + e]; }
};

template <class G>
struct GameLaunch {
    G g;
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

template <class G>
__device__ __forceinline__ int game_draw(const GameLaunch<G>& L, int e, unsigned episode) {
    Philox p(L.seed, (unsigned)e, episode, G::STREAM);
    return L.g.code(p.uniform(), e, episode);
}

template <class G>
__global__ void k_game_reset(const GameLaunch<G> L) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= L.g.B) return;
    L.g.start(e, L.start ? L.start[e] : game_draw(L, e, 0u));
    for (int a = 0; a < 3; a++) L.mask[(size_t)e * 3 + a] = 1;
    L.cur[e] = 1;
    L.opp[e] = 1;
}

template <class G>
__global__ void k_game_step(const GameLaunch<G> L) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= L.g.B) return;
    float reward;
    const bool done = L.g.move(e, L.action[e], reward);
    L.reward[e] = reward;
    L.done[e] = done ? 1 : 0;
    if (done) L.g.start(e, game_draw(L, e, L.episode[e] + 1u));
}

template <class G>
__global__ __launch_bounds__(256) void k_game_render(const GameLaunch<G> L) {
    const G& g = L.g;
    const size_t total = (size_t)g.B * g.FE, i0 = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 16;
    if (i0 >= total) return;  // (the last run starts inside the last env; its bytes past `total` lie in the allocation's padding)
    int e = (int)(i0 / g.FE);
    const int j = (int)(i0 - (size_t)e * g.FE);
    int row = j / g.W, col = j - row * g.W;
    int cy = row / g.ch, ry = row - cy * g.ch;  // cell row, pixel row inside the cell
    int cx = col / g.cw, rx = col - cx * g.cw;  // cell column, pixel column inside the cell
    typename G::View v = g.view(e);
    uint32_t val = g.cell(v, cy, cx);
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int q = 0; q < 16; q++) {
        w[q >> 2] |= val << (8 * (q & 3));
        bool moved = false;
        if (++rx == g.cw) { rx = 0; cx++; moved = true; }
        if (++col == g.W) {
            col = cx = rx = 0;
            moved = true;
            ++row;
            if (++ry == g.ch) { ry = 0; cy++; }
            if (row == g.H) {
                row = cy = ry = 0;
                if (++e < g.B) v = g.view(e);
            }
        }
        if (moved) val = e < g.B ? g.cell(v, cy, cx) : 0u;
    }
    *reinterpret_cast<uint4*>(L.frames + i0) = make_uint4(w[0], w[1], w[2], w[3]);
}

template <class G>
__global__ void k_game_arena_step(const ImgArenaLaunch R, const G g) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= g.B || !R.a.live[e]) return;
    const int a = imgarena_record(R, e);
    float reward;
    const bool done = g.move(e, a, reward);
    imgarena_outcome(R, e, reward, done);
}

}  // namespace mz
