// mz_arena_image.h -- the arena (mz_arena.h) for image and frame games: a one-player arena (ARENA_NONE: the challenger plays every move)
// whose roots come from the host-stepped path's frame history (mz_extenv.h: ExtEnv) instead of a device board or CartPole state.  Two
// front ends share one ply:
//   device image games          : root builder, k_arena_pre, search, record + env step (mz_grid_game.h: k_game_arena_step), k_game_render
//   (mz_catch.h, mz_breakout.h)   -- nothing crosses PCIe and nothing waits inside mz_arena_step;
//   host-stepped (act / commit) : the same ply cut where the host steps: upload, root builder, k_arena_pre, search, k_imgarena_record |
//                                 host env.step | upload, k_imgarena_commit.
//
//   k_imgarena_reset      : the arena state of k_arena_reset (a device game's state, mask and player ids: its own k_game_reset)
//   k_imgarena_ingest     : the root builder, a frozen-aware k_ext_ingest: StackFrameAndAction over the newest frame into
//                           ArenaState::obs, the frame filed in the history ring.  Geometry and values are k_ext_ingest's own (ext_source,
//                           ext_frame_value, ext_action_value).  No record ring, no temperature, no r_done: the reset flag is "first ply",
//                           the previous action is the env's own last record.  A frozen env's workgroups return before touching anything,
//                           so its history, head and root stay as they were.  The only kernel here that moves real bytes (C4: 512 envs x
//                           8 planes x 96 x 96 float32, 151 MB written per ply): one workgroup per (env, chunk), 16-byte stores.
//   k_imgarena_record     : the "after acting" half of the ply record of every LIVE env (host-stepped arenas: the act)
//   k_imgarena_commit     : host-stepped arenas: the uploaded reward and done flag of every LIVE env into return, length, freeze, totals
// One thread per env in all but the root builder: these move a few bytes per env.
#pragma once
#include "mz_arena.h"
#include "mz_extenv.h"

namespace mz {

constexpr int IMGARENA_CATCH = 1, IMGARENA_EXTERNAL = 2;  // which front end an image arena runs (0: a device-state arena of mz_arena.h)

struct ImgArenaLaunch {
    ExtLaunch L;  // the frames' geometry and history: x, B, A, OD, first (first ply), parity (ply & 1); obs = ArenaState::obs
    ArenaState a;
    const int* action;   // the search's outputs
    const double* pi;
    const double* root;
};

__global__ void k_imgarena_reset(const ImgArenaLaunch R) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e == 0) {
        for (int i = 0; i < 4; i++) R.a.totals[i] = 0;
        *R.a.n_live = R.L.B;
    }
    if (e >= R.L.B) return;
    R.a.live[e] = 1;
    R.a.winner[e] = WIN_UNFINISHED;
    R.a.length[e] = 0;
    R.a.ret[e] = 0.0;
    R.a.r_live[e] = 0;
    R.a.r_side[e] = -1;
    R.a.r_action[e] = -1;
    R.a.r_u[e] = 0.0;
    R.a.r_root[e] = 0.0;
}

// One group of VEC consecutive root floats of env e starting at j0 (VEC as ext_ingest_group: 4 where a group lies in one plane or run).
// `first`: every frame plane is the uploaded frame and every action plane 0; else plane 0 is the uploaded frame with action `a`, the
// others come from the history ring.  The group that reads the newest frame also files it (first ply: in every slot).
template <int VEC>
__device__ __forceinline__ void imgarena_group(const ImgArenaLaunch& R, int e, int j0, bool first, int a, int h, int hnew) {
    const ExtLaunch& L = R.L;
    const ExtEnv& X = L.x;
    int k, src;
    ext_source(L, j0, k, src);
    float v[VEC];
    if (src < 0) {
        const float f = ext_action_value(first ? 0 : (k == 0 ? a : X.hist_act[(size_t)e * X.S + ((h - (k - 1)) % X.S + X.S) % X.S]), L.A);
#pragma unroll
        for (int q = 0; q < VEC; q++) v[q] = f;
    } else {
        const bool fresh = k == 0 || first;
        const size_t off = fresh ? (size_t)e * X.FE + src : ((size_t)e * X.S + ((h - (k - 1)) % X.S + X.S) % X.S) * X.FE + src;
        const void* base = fresh ? X.frames : X.hist;
        const bool file = k == 0 && X.S > 0;
        const int t0 = first ? 0 : hnew, t1 = first ? X.S : hnew + 1;
        if constexpr (VEC == 4) {  // one 4-byte (uint8 frames) or 16-byte (float frames) load; the values are ext_frame_value's of its elements
            if (X.u8) {
                const uint32_t w = *reinterpret_cast<const uint32_t*>(static_cast<const unsigned char*>(base) + off);
#pragma unroll
                for (int q = 0; q < 4; q++) v[q] = ext_frame_value(L, &w, (size_t)q);
                if (file)
                    for (int t = t0; t < t1; t++) *reinterpret_cast<uint32_t*>(static_cast<unsigned char*>(X.hist) + ((size_t)e * X.S + t) * X.FE + src) = w;
            } else {
                const float4 w = *reinterpret_cast<const float4*>(static_cast<const float*>(base) + off);
#pragma unroll
                for (int q = 0; q < 4; q++) v[q] = ext_frame_value(L, &w, (size_t)q);
                if (file)
                    for (int t = t0; t < t1; t++) *reinterpret_cast<float4*>(static_cast<float*>(X.hist) + ((size_t)e * X.S + t) * X.FE + src) = w;
            }
        } else {
            v[0] = ext_frame_value(L, base, off);
            if (file)
                for (int t = t0; t < t1; t++) {
                    const size_t dst = ((size_t)e * X.S + t) * X.FE + src;
                    if (X.u8) static_cast<unsigned char*>(X.hist)[dst] = static_cast<const unsigned char*>(base)[off];
                    else static_cast<float*>(X.hist)[dst] = v[0];
                }
        }
    }
    float* o = L.obs + (size_t)e * L.OD + j0;
    if constexpr (VEC == 4) *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
    else *o = v[0];
}

// Grid and VEC as k_ext_ingest: blockIdx.y = env, blockIdx.x = chunk of its root.  The history head is kept twice, by ply parity, as
// there: a launch reads one copy and writes the other.  A frozen env's head is never read again.
template <int VEC>
__global__ __launch_bounds__(256) void k_imgarena_ingest(const ImgArenaLaunch R) {
    const ExtLaunch& L = R.L;
    const ExtEnv& X = L.x;
    const int e = blockIdx.y;
    if (!R.a.live[e]) return;
    const bool first = L.first != 0;
    const int a = first ? 0 : R.a.r_action[e];  // a live env moved at the last ply: its record holds that move
    const int h = X.S > 0 && !first ? X.head[(size_t)L.parity * L.B + e] : 0;
    const int hnew = first || X.S == 0 ? 0 : (h + 1) % X.S;
    if (blockIdx.x == 0 && threadIdx.x == 0 && X.S > 0) {
        int* ha = X.hist_act + (size_t)e * X.S;
        if (first)
            for (int k = 0; k < X.S; k++) ha[k] = 0;
        else
            ha[hnew] = a;  // (no reader of this launch: plane 0 takes `a` itself, planes k >= 1 read the other slots)
        X.head[(size_t)(L.parity ^ 1) * L.B + e] = hnew;
    }
    constexpr int iters = VEC == 4 ? EXT_ITER : 1;
#pragma unroll
    for (int it = 0; it < iters; it++) {
        const int j0 = ((blockIdx.x * iters + it) * blockDim.x + threadIdx.x) * VEC;
        if (j0 < L.OD) imgarena_group<VEC>(R, e, j0, first, a, h, hnew);
    }
}

// the "after acting" half of a live env's ply record (the searched move; k_arena_step's fields).  Returns the move.
__device__ inline int imgarena_record(const ImgArenaLaunch& R, int e) {
    const int A = R.L.A;
    int a = R.action[e];
    a = a < 0 ? 0 : (a >= A ? A - 1 : a);
    for (int k = 0; k < A; k++) R.a.r_pi[(size_t)e * A + k] = R.pi[(size_t)e * A + k];
    R.a.r_action[e] = a;
    R.a.r_side[e] = SIDE_CHALLENGER;
    R.a.r_root[e] = R.root[e];
    R.a.r_u[e] = 0.0;
    return a;
}

// the outcome of a live env's ply: the float32 reward onto the float64 return in ply order, the length, and for a finished game the
// freeze and the tally (a finished one-player episode counts under WIN_DRAW, as CartPole's does)
__device__ inline void imgarena_outcome(const ImgArenaLaunch& R, int e, float reward, bool done) {
    R.a.ret[e] += (double)reward;
    const int len = R.a.length[e] + 1;
    R.a.length[e] = len;
    if (done) {
        R.a.live[e] = 0;
        R.a.winner[e] = WIN_DRAW;
        atomicAdd(&R.a.totals[WIN_DRAW - 1], 1ULL);
        atomicAdd(&R.a.totals[3], (unsigned long long)len);
        atomicSub(R.a.n_live, 1);
    }
}

__global__ void k_imgarena_record(const ImgArenaLaunch R) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= R.L.B || !R.a.live[e]) return;  // a frozen env's searched output is discarded
    (void)imgarena_record(R, e);
}

__global__ void k_imgarena_commit(const ImgArenaLaunch R) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= R.L.B || !R.a.live[e]) return;  // a frozen env's uploaded reward and done flag are ignored
    imgarena_outcome(R, e, R.L.x.reward[e], R.L.x.done[e] != 0);
}

}  // namespace mz
