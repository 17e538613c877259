// mz_catch.h -- Catch (MZ_ENV_CATCH): a learnable image game on the device, feeding the host-stepped path's own kernels.
//
// The game (games.CatchEnv is the specification): a rows x cols grid of cell_h x cell_w pixel cells, one uint8 frame [1, H, W].  A ball
// at (br, bc) falls one row per move; the paddle at column pc of the last row moves left / stays / right (actions 0 / 1 / 2, clipped at
// the walls) BEFORE the ball falls.  When the ball reaches the last row the episode ends with reward +1 (bc == pc) or -1; every other
// reward is 0.  The frame is 0 with the ball's and the paddle's cells at 255.  A finished env is reset at once: ball in row 0, paddle at
// cols / 2, ball column min(cols - 1, floor(u * cols)) with u the first double of Philox(seed, env, episode, CATCH_STREAM).  Episode 0
// of env e starts with the ball in row e % (rows - 1), so the envs do not all finish on the same move.
//
// A move is mz_extenv.h's act and commit with the PCIe copies replaced by two kernels:
//   k_catch_step   : one thread per env.  Reads the sampled action, moves paddle and ball, writes ext.reward / ext.done (what the host's
//                    commit uploads) and, for a finished env, the next episode's state.  k_ext_commit (after it) bumps episode[].
//   k_catch_render : paints every env's next frame into ext.frames (what the host's act uploads).  The only kernel here that moves bytes
//                    (C4: 512 x 9 216 B per move): the frames are one flat byte array, a lane owns one 16-byte run of it and stores it
//                    once.  A lane divides once for its first byte (env, pixel row, pixel column, cell row, cell column) and walks the
//                    other 15 with counters, so runs that cross a cell, a pixel row or an env (cell_w or W no multiple of 16) need no
//                    path of their own.  The array is allocated rounded up to 16 bytes; the bytes past the last env are written 0.
#pragma once
#include "mz_extenv.h"

namespace mz {

constexpr int ENV_CATCH = 6;
constexpr unsigned CATCH_STREAM = 0x70000000u;  // the ball column's Philox stream (0x4.., 0x5.., 0x60.., 0x61.. are taken)

struct CatchEnv {
    int rows, cols, ch, cw;  // grid and cell size in pixels
    int H, W, FE;            // frame height, width, bytes (H * W)
    int* br;                 // [B] ball row
    int* bc;                 // [B] ball column
    int* pc;                 // [B] paddle column
};

struct CatchLaunch {
    CatchEnv c;
    int B;
    unsigned long long seed;
    const int* action;        // [B] the search's sampled actions
    const unsigned* episode;  // [B] EnvState::episode (bumped by k_ext_commit, after the step)
    float* reward;            // ExtEnv::reward
    unsigned char* done;      // ExtEnv::done
    unsigned char* frames;    // ExtEnv::frames, [pad16(B * FE)]
    unsigned char* mask;      // reset only: [B][3] all legal
    int* cur;                 // reset only: [B] player ids 1 / 1
    int* opp;
};

__device__ __forceinline__ int catch_ball_col(const CatchLaunch& G, int e, unsigned episode) {
    Philox g(G.seed, (unsigned)e, episode, CATCH_STREAM);
    const int c = (int)floor(g.uniform() * (double)G.c.cols);
    return c < G.c.cols - 1 ? c : G.c.cols - 1;
}

// reset: episode 0 of every env (staggered ball rows), the all-legal mask and the player ids the search reads every move
__global__ void k_catch_reset(const CatchLaunch G) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= G.B) return;
    G.c.br[e] = e % (G.c.rows - 1);
    G.c.bc[e] = catch_ball_col(G, e, 0u);
    G.c.pc[e] = G.c.cols / 2;
    for (int a = 0; a < 3; a++) G.mask[(size_t)e * 3 + a] = 1;
    G.cur[e] = 1;
    G.opp[e] = 1;
}

__global__ void k_catch_step(const CatchLaunch G) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= G.B) return;
    const CatchEnv& c = G.c;
    int pc = c.pc[e] + G.action[e] - 1;
    pc = pc < 0 ? 0 : (pc > c.cols - 1 ? c.cols - 1 : pc);
    const int br = c.br[e] + 1;
    const bool done = br == c.rows - 1;
    G.reward[e] = done ? (c.bc[e] == pc ? 1.0f : -1.0f) : 0.0f;
    G.done[e] = done ? 1 : 0;
    if (done) {
        c.br[e] = 0;
        c.bc[e] = catch_ball_col(G, e, G.episode[e] + 1u);
        c.pc[e] = c.cols / 2;
    } else {
        c.br[e] = br;
        c.pc[e] = pc;
    }
}

__global__ __launch_bounds__(256) void k_catch_render(const CatchLaunch G) {
    const CatchEnv& c = G.c;
    const size_t total = (size_t)G.B * c.FE, i0 = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 16;
    if (i0 >= total) return;  // (the last run starts inside the last env; its bytes past `total` lie in the allocation's padding)
    int e = (int)(i0 / c.FE);
    const int j = (int)(i0 - (size_t)e * c.FE);
    int row = j / c.W, col = j - row * c.W;
    int cy = row / c.ch, ry = row - cy * c.ch;  // cell row, pixel row inside the cell
    int cx = col / c.cw, rx = col - cx * c.cw;  // cell column, pixel column inside the cell
    int br = c.br[e], bc = c.bc[e], pc = c.pc[e];
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int q = 0; q < 16; q++) {
        if (e < G.B && ((cy == br && cx == bc) || (cy == c.rows - 1 && cx == pc))) w[q >> 2] |= 0xffu << (8 * (q & 3));
        if (++rx == c.cw) { rx = 0; cx++; }
        if (++col == c.W) {
            col = cx = rx = 0;
            ++row;
            if (++ry == c.ch) { ry = 0; cy++; }
            if (row == c.H) {
                row = cy = ry = 0;
                if (++e < G.B) { br = c.br[e]; bc = c.bc[e]; pc = c.pc[e]; }
            }
        }
    }
    *reinterpret_cast<uint4*>(G.frames + i0) = make_uint4(w[0], w[1], w[2], w[3]);
}

}  // namespace mz
