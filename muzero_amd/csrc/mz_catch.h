// mz_catch.h -- Catch (MZ_ENV_CATCH): a learnable image game on the device, feeding the host-stepped path's own kernels.
//
// The game (games.CatchEnv is the specification): a rows x cols grid of cell_h x cell_w pixel cells, one uint8 frame [1, H, W].  A ball
// at (br, bc) falls one row per move; the paddle at column pc of the last row moves left / stays / right (actions 0 / 1 / 2, clipped at
// the walls) BEFORE the ball falls.  When the ball reaches the last row the episode ends with reward +1 (bc == pc) or -1; every other
// reward is 0.  The frame is 0 with the ball's and the paddle's cells at 255.  A finished env is reset at once: ball in row 0, paddle at
// cols / 2, ball column min(cols - 1, floor(u * cols)) with u the first double of Philox(seed, env, episode, CATCH_STREAM).  Episode 0
// of env e starts with the ball in row e % (rows - 1), so the envs do not all finish on the same move.
//
// The state is three ints per env (ball row, ball column, paddle column); the start code is start_row * cols + ball_col (the arena uploads
// it; no Philox draw there).  The kernels are mz_grid_game.h's.
#pragma once
#include "mz_grid_game.h"

namespace mz {

constexpr int ENV_CATCH = 6;
constexpr unsigned CATCH_STREAM = 0x70000000u;  // the ball column's Philox stream (0x4.., 0x5.., 0x60.., 0x61.. are taken)

struct Catch : GridGame {
    enum { BR = 0, BC, PC, FIELDS };
    static constexpr unsigned STREAM = CATCH_STREAM;
    static constexpr int KIND = ENV_CATCH, ARENA = IMGARENA_CATCH;
    static constexpr const char *NAME = "Catch", *STRUCT = "mz_catch_env", *OBS_VALUES = "action planes of 1/3, 2/3";

    __device__ __forceinline__ int code(double u, int e, unsigned episode) const {
        const int c = (int)floor(u * (double)cols);
        return (episode == 0u ? e % (rows - 1) : 0) * cols + (c < cols - 1 ? c : cols - 1);
    }

    __device__ __forceinline__ void start(int e, int k) const {
        field(BR, e) = k / cols;
        field(BC, e) = k % cols;
        field(PC, e) = cols / 2;
    }

    __device__ __forceinline__ bool move(int e, int a, float& reward) const {
        int pc = field(PC, e) + a - 1;
        pc = pc < 0 ? 0 : (pc > cols - 1 ? cols - 1 : pc);
        const int br = field(BR, e) + 1;
        const bool done = br == rows - 1;
        reward = done ? (field(BC, e) == pc ? 1.0f : -1.0f) : 0.0f;
        if (!done) {
            field(BR, e) = br;
            field(PC, e) = pc;
        }
        return done;
    }

    struct View {
        int br, bc, pc;
    };
    __device__ __forceinline__ View view(int e) const { return View{field(BR, e), field(BC, e), field(PC, e)}; }
    __device__ __forceinline__ uint32_t cell(const View& v, int cy, int cx) const {
        return (cy == v.br && cx == v.bc) || (cy == rows - 1 && cx == v.pc) ? 255u : 0u;
    }
};

}  // namespace mz
