// mz_arena.h -- evaluation matches as one lock-step batch (the evaluators' game loops, pipeline.py:289-397 and 400-488, for B games at
// once).  The env state is the self-play one (mz_env.h: EnvState, the board / CartPole device functions); what differs is the
// bookkeeping around it: two sides, no root noise, NO auto-reset -- a finished env is frozen -- and a tally instead of replay items.
//
//   k_arena_reset : env reset + arena state (winner, length, return, live flag, totals)
//   k_arena_pre   : roots of the side(s) to move, staged into the root buffers of the planner that searches them; the
//                   "before acting" half of the ply record (observation, mask, player, live flag)
//   k_arena_pick  : opening and random-opponent moves, legal[floor(u * n_legal)], one wave per env
//   k_arena_step  : env.step of every LIVE env without auto-reset, win test through the last move, freeze, the "after acting" half of
//                   the ply record, totals
//
// One wave per env in pick / step: the 362-action boards need more than the 16-lane groups of mz_env.h, and every env of a launch takes
// the same path.  These kernels move a few KiB per env per ply; a ply's time is the two searches between them.
#pragma once
#include "mz_env.h"

namespace mz {

constexpr int ARENA_NONE = 0, ARENA_RANDOM = 1, ARENA_PLANNER = 2;                                // opponent kinds
constexpr int SIDE_CHALLENGER = 0, SIDE_OPPONENT = 1, SIDE_RANDOM = 2, SIDE_OPENING = 3;          // who chose a ply's move
constexpr int WIN_UNFINISHED = 0, WIN_CHALLENGER = 1, WIN_OPPONENT = 2, WIN_DRAW = 3;
constexpr unsigned ARENA_STREAM_OPENING = 0x60000000u, ARENA_STREAM_RANDOM = 0x61000000u;         // Philox streams of their own

struct ArenaState {
    int B, half;           // half: B / 2 for two-player envs (env i and i + half are a pair), 0 for one-player envs
    int opponent, opening_plies;
    // the envs' roots (what EnvLaunch.obs / mask / cur / opp point to in arena mode)
    float* obs;            // [B][D]
    unsigned char* mask;   // [B][A]
    int *cur, *opp;        // [B]
    // per env
    unsigned char* live;   // [B] 1 until the game ends
    int* winner;           // [B] WIN_*
    int* length;           // [B] plies played (openings included)
    double* ret;           // [B] undiscounted return (one-player envs); +1 / -1 / 0 from the challenger's side (board games)
    unsigned long long* totals;  // [0] challenger wins, [1] opponent wins, [2] draws / finished one-player episodes, [3] sum of finished lengths
    int* n_live;           // live envs
    // picked moves of this ply (k_arena_pick)
    int* pick;             // [B]
    double* pick_u;        // [B]
    // record of the last ply
    float* r_obs;          // [B][D]
    unsigned char* r_mask; // [B][A]
    int *r_player, *r_side, *r_action;  // [B]
    double *r_pi, *r_root, *r_u;        // [B][A], [B], [B]
    unsigned char* r_live; // [B] the env was live when the ply began (its record is this ply's)
};

// One contiguous run of envs and who moves in it.  Searched runs are staged to `obs / mask / cur / opp / temp` (the searching planner's
// root buffers, run-relative) and read their move back from `action / pi / root`; picked runs leave all of them null.
struct ArenaSeg {
    int lo, n, side;
    float* obs;
    unsigned char* mask;
    int *cur, *opp;
    double* temp;
    const int* action;
    const double* pi;
    const double* root;
};

struct ArenaLaunch {
    EnvLaunch L;  // env state; obs / mask / cur / opp are the arena's own root buffers
    ArenaState a;
    int ply, nseg;
    ArenaSeg seg[2];
};

inline void arena_free(ArenaState& a) {
    void* bufs[] = {a.obs, a.mask, a.cur, a.opp, a.live, a.winner, a.length, a.ret, a.totals, a.n_live, a.pick, a.pick_u,
                    a.r_obs, a.r_mask, a.r_player, a.r_side, a.r_action, a.r_pi, a.r_root, a.r_u, a.r_live};
    for (void* b : bufs)
        if (b) (void)hipFree(b);
    a = ArenaState{};
}

inline hipError_t arena_alloc(ArenaState& a, int B, int A, int D) {
    arena_free(a);
    a.B = B;
    hipError_t r;
#define MZ_ALLOC(ptr, bytes)                                      \
    if ((r = hipMalloc(&(ptr), (bytes))) != hipSuccess) return r; \
    if ((r = hipMemset((ptr), 0, (bytes))) != hipSuccess) return r;
    MZ_ALLOC(a.obs, (size_t)B * D * sizeof(float) + 256);
    MZ_ALLOC(a.mask, (size_t)B * A + 16);
    MZ_ALLOC(a.cur, (size_t)B * sizeof(int));
    MZ_ALLOC(a.opp, (size_t)B * sizeof(int));
    MZ_ALLOC(a.live, (size_t)B);
    MZ_ALLOC(a.winner, (size_t)B * sizeof(int));
    MZ_ALLOC(a.length, (size_t)B * sizeof(int));
    MZ_ALLOC(a.ret, (size_t)B * sizeof(double));
    MZ_ALLOC(a.totals, 4 * sizeof(unsigned long long));
    MZ_ALLOC(a.n_live, sizeof(int));
    MZ_ALLOC(a.pick, (size_t)B * sizeof(int));
    MZ_ALLOC(a.pick_u, (size_t)B * sizeof(double));
    MZ_ALLOC(a.r_obs, (size_t)B * D * sizeof(float) + 256);
    MZ_ALLOC(a.r_mask, (size_t)B * A + 16);
    MZ_ALLOC(a.r_player, (size_t)B * sizeof(int));
    MZ_ALLOC(a.r_side, (size_t)B * sizeof(int));
    MZ_ALLOC(a.r_action, (size_t)B * sizeof(int));
    MZ_ALLOC(a.r_pi, (size_t)B * A * sizeof(double));
    MZ_ALLOC(a.r_root, (size_t)B * sizeof(double));
    MZ_ALLOC(a.r_u, (size_t)B * sizeof(double));
    MZ_ALLOC(a.r_live, (size_t)B);
#undef MZ_ALLOC
    return hipDeviceSynchronize();  // (the fills run on the NULL stream: see env_alloc)
}

// ---- reset: k_env_reset's body on the arena's root buffers, plus the arena state ----
__global__ void k_arena_reset(const ArenaLaunch R) {
    const EnvLaunch& L = R.L;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e == 0) {
        for (int i = 0; i < 4; i++) { L.env.counters[i] = 0; R.a.totals[i] = 0; }
        *R.a.n_live = L.B;
    }
    if (e >= L.B) return;
    L.env.steps[e] = 0;
    L.env.episode[e] = 0;
    if (L.env.kind == ENV_CARTPOLE) {
        double s[4];
        cartpole_fresh(L, e, s);
        for (int i = 0; i < 4; i++) L.env.cp_state[e * 4 + i] = s[i];
        cartpole_obs_reset(L, e, s);
        L.mask[(size_t)e * 2] = 1; L.mask[(size_t)e * 2 + 1] = 1;
        L.cur[e] = 1; L.opp[e] = 1;
    } else {
        board_fresh(L, e);
    }
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

// ---- staging ----
// dst[0, n) = src[0, n) by the whole grid: 16-byte loads and stores where both ends are 16-byte aligned, the tail (and unaligned runs) by element
template <typename T>
__device__ inline void arena_copy(T* __restrict__ dst, const T* __restrict__ src, size_t n, size_t tid, size_t nthreads) {
    constexpr size_t V = 16 / sizeof(T);
    const bool aligned = ((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src)) & 15) == 0;
    const size_t nv = aligned ? n / V : 0;
    const uint4* s4 = reinterpret_cast<const uint4*>(src);
    uint4* d4 = reinterpret_cast<uint4*>(dst);
    for (size_t i = tid; i < nv; i += nthreads) d4[i] = s4[i];
    for (size_t i = nv * V + tid; i < n; i += nthreads) dst[i] = src[i];
}

// the searched runs' masks: the env's own mask, all-legal for a frozen env (a finished board may be full: the search needs a legal move)
__device__ inline void arena_stage_mask(const ArenaLaunch& R, const ArenaSeg& s, int A, size_t tid, size_t nthreads) {
    const unsigned char* src = R.a.mask + (size_t)s.lo * A;
    const size_t n = (size_t)s.n * A;
    const bool aligned = ((reinterpret_cast<uintptr_t>(s.mask) | reinterpret_cast<uintptr_t>(src)) & 15) == 0;
    const size_t nv = aligned ? n / 16 : 0;
    for (size_t i = tid; i < nv; i += nthreads) {
        uint4 v = reinterpret_cast<const uint4*>(src)[i];
        unsigned int w[4] = {v.x, v.y, v.z, v.w};
        int e = (int)((16 * i) / A), r = (int)((16 * i) - (size_t)e * A);
        bool frozen = !R.a.live[s.lo + e];
#pragma unroll
        for (int k = 0; k < 16; k++) {
            if (frozen) w[k >> 2] = (w[k >> 2] & ~(0xffu << (8 * (k & 3)))) | (1u << (8 * (k & 3)));
            if (++r == A && k < 15) {
                r = 0;
                e++;
                frozen = e < s.n ? !R.a.live[s.lo + e] : false;
            }
        }
        reinterpret_cast<uint4*>(s.mask)[i] = make_uint4(w[0], w[1], w[2], w[3]);
    }
    for (size_t i = nv * 16 + tid; i < n; i += nthreads) s.mask[i] = R.a.live[s.lo + (int)(i / A)] ? src[i] : (unsigned char)1;
}

__global__ __launch_bounds__(256) void k_arena_pre(const ArenaLaunch R) {
    const size_t tid = blockIdx.x * (size_t)blockDim.x + threadIdx.x, nthreads = gridDim.x * (size_t)blockDim.x;
    const int B = R.a.B, A = R.L.env.A, D = R.L.env.D;
    for (int k = 0; k < R.nseg; k++) {
        const ArenaSeg& s = R.seg[k];
        if (!s.obs) continue;  // a picked run: nothing is searched
        arena_copy(s.obs, R.a.obs + (size_t)s.lo * D, (size_t)s.n * D, tid, nthreads);
        arena_stage_mask(R, s, A, tid, nthreads);
        for (size_t i = tid; i < (size_t)s.n; i += nthreads) {
            s.cur[i] = R.a.cur[s.lo + i];
            s.opp[i] = R.a.opp[s.lo + i];
            s.temp[i] = 1.0;  // the recorded policy is the visit distribution; the move (most-visited child) does not depend on it
        }
    }
    // the "before acting" half of the record.  A frozen env's roots no longer change, so copying them again leaves its record as it was
    arena_copy(R.a.r_obs, R.a.obs, (size_t)B * D, tid, nthreads);
    arena_copy(R.a.r_mask, R.a.mask, (size_t)B * A, tid, nthreads);
    for (size_t i = tid; i < (size_t)B; i += nthreads) {
        R.a.r_player[i] = R.a.cur[i];
        R.a.r_live[i] = R.a.live[i];
    }
}

__device__ inline const ArenaSeg& arena_seg_of(const ArenaLaunch& R, int e) { return R.seg[(R.nseg > 1 && e >= R.seg[1].lo) ? 1 : 0]; }

// ---- opening and random-opponent moves: legal[floor(u * n_legal)], one wave per env ----
// u: one Philox double per (pair, ply) for an opening -- both games of a pair draw the same -- and per (env, ply) for the random opponent
__global__ __launch_bounds__(256) void k_arena_pick(const ArenaLaunch R) {
    const int e = (int)((blockIdx.x * (size_t)blockDim.x + threadIdx.x) >> 6), lane = (int)(threadIdx.x & 63);
    if (e >= R.a.B) return;
    const ArenaSeg& s = arena_seg_of(R, e);
    if (s.obs || !R.a.live[e]) return;  // searched, or frozen
    const int A = R.L.env.A;
    const bool opening = s.side == SIDE_OPENING;
    Philox g(R.L.seed, (unsigned)(opening && R.a.half ? e % R.a.half : e), (unsigned)R.ply, opening ? ARENA_STREAM_OPENING : ARENA_STREAM_RANDOM);
    const double u = g.uniform();
    const unsigned char* m = R.a.mask + (size_t)e * A;
    int n = 0;
    for (int a0 = 0; a0 < A; a0 += 64) n += __popcll(__ballot(a0 + lane < A && m[a0 + lane] != 0));
    if (n == 0) return;  // (cannot happen for a live env: a full board is a finished game)
    int k = (int)(u * (double)n);
    if (k > n - 1) k = n - 1;
    int before = 0, chosen = -1;
    for (int a0 = 0; a0 < A && chosen < 0; a0 += 64) {
        const bool legal = a0 + lane < A && m[a0 + lane] != 0;
        const unsigned long long bal = __ballot(legal);
        const int c = __popcll(bal);
        if (k < before + c) {
            const int rank = __popcll(bal & ((1ull << lane) - 1ull));  // legal moves of this chunk below this lane
            const unsigned long long hit = __ballot(legal && rank == k - before);
            chosen = a0 + (int)__ffsll((long long)hit) - 1;
        }
        before += c;
    }
    if (lane == 0) {
        R.a.pick[e] = chosen;
        R.a.pick_u[e] = u;
    }
}

// ---- env.step without auto-reset ----
// BoardGameEnv.step (games/env.py:117-154) by the 64 lanes of an env's wave; board_step_group's logic, with the finished game frozen
// instead of reset.  `done`: winner colour (0: none) and whether the game is over.
__device__ inline void arena_board_step(const EnvLaunch& L, int e, int lane, int a, int& winner, bool& done) {
    const int n = L.env.bn, nn = L.env.nn;
    signed char* b = L.env.board + (size_t)e * nn;
    signed char* pl = L.env.planes + (size_t)e * 8 * nn;
    const int me = L.env.player[e], opp = 3 - me, st = L.env.steps[e];
    signed char* mine = pl + (me - 1) * 4 * nn;
    const signed char* theirs = pl + (opp - 1) * 4 * nn;
    winner = 0;
    if (a == nn) {  // resign (games/env.py:134-136)
        winner = opp;
    } else if (st >= (L.env.win - 1) * 2) {  // games/tictactoe.py:37-38, games/gomoku.py:76-77 with the pre-increment step count
        // lanes 0..7 walk one ray each from the new stone (which the rays do not include)
        const int r = a / n, c = a % n, d = lane & 3, sg = (lane & 4) ? -1 : 1;
        const int dr = sg * (d == 0 ? 0 : d == 3 ? -1 : 1), dc = sg * (d == 1 ? 0 : 1);  // (0,1) (1,0) (1,1) (-1,1)
        const int k = lane < 8 ? board_line(b, n, r, c, dr, dc, me) : 0;
        const int k2 = __shfl_xor(k, 4);
        if (__ballot(lane < 4 && 1 + k + k2 >= L.env.win) != 0) winner = me;
    }
    bool open = false;  // an empty point other than the one just played
    for (int i0 = 0; i0 < nn; i0 += 64) open = open || __ballot(i0 + lane < nn && b[i0 + lane] == 0 && i0 + lane != a) != 0;
    done = winner != 0 || !open;
    if (done) {
        if (lane == 0 && a < nn) b[a] = (signed char)me;  // the final position; planes, observation, mask and player stay as they were
        return;
    }
    // history shift mine[t] <- mine[t - 1], mine[0] <- the mover's stones, and the observation of the next side to move
    // (games/env.py:242-271): its own history (unchanged by this move), the mover's new history, the colour plane.  Plane t is
    // written from plane t - 1 before that one is overwritten (t walks downwards; a wave's memory operations are served in order)
    float* o = L.obs + (size_t)e * 9 * nn;
    for (int t = 3; t >= 0; t--)
        for (int i = lane; i < nn; i += 64) {
            const signed char v = t > 0 ? mine[(t - 1) * nn + i] : (signed char)((b[i] == me || i == a) ? 1 : 0);
            const signed char x = theirs[t * nn + i];
            mine[t * nn + i] = v;
            o[(2 * t) * nn + i] = (float)x;
            o[(2 * t + 1) * nn + i] = (float)v;
        }
    for (int i = lane; i < nn; i += 64) o[8 * nn + i] = opp == 1 ? 1.0f : 0.0f;
    if (lane == 0) {
        L.mask[(size_t)e * (nn + 1) + a] = 0;
        b[a] = (signed char)me;
        L.env.player[e] = opp;
        L.env.steps[e] = st + 1;
        L.cur[e] = opp;
        L.opp[e] = me;
    }
}

// CartPole step of env_step_one without the reset (lane 0 of the env's wave); returns done
__device__ inline bool arena_cartpole_step(const EnvLaunch& L, int e, int a) {
    double s[4];
    for (int i = 0; i < 4; i++) s[i] = L.env.cp_state[e * 4 + i];
    const bool term = cartpole_physics(s, a);
    const int st = L.env.steps[e] + 1;
    L.env.steps[e] = st;
    if (term || st >= 500) return true;
    for (int i = 0; i < 4; i++) L.env.cp_state[e * 4 + i] = s[i];
    float* o = L.obs + (size_t)e * 20;  // appendleft (gym_env.py:317-324)
    for (int k = 3; k > 0; k--)
        for (int i = 0; i < 5; i++) o[k * 5 + i] = o[(k - 1) * 5 + i];
    for (int i = 0; i < 4; i++) o[i] = (float)s[i];
    o[4] = (float)((a + 1) / (double)2);
    return false;
}

__global__ __launch_bounds__(256) void k_arena_step(const ArenaLaunch R) {
    const EnvLaunch& L = R.L;
    const int e = (int)((blockIdx.x * (size_t)blockDim.x + threadIdx.x) >> 6), lane = (int)(threadIdx.x & 63);
    if (e >= R.a.B || !R.a.live[e]) return;  // a frozen env's searched output is discarded
    const ArenaSeg& s = arena_seg_of(R, e);
    const int A = L.env.A, i = e - s.lo;
    const bool searched = s.obs != nullptr;
    int a = searched ? s.action[i] : R.a.pick[e];
    a = a < 0 ? 0 : (a >= A ? A - 1 : a);
    // the "after acting" half of the record
    for (int k = lane; k < A; k += 64) R.a.r_pi[(size_t)e * A + k] = searched ? s.pi[(size_t)i * A + k] : 0.0;
    if (lane == 0) {
        R.a.r_action[e] = a;
        R.a.r_side[e] = s.side;
        R.a.r_root[e] = searched ? s.root[i] : 0.0;
        R.a.r_u[e] = searched ? 0.0 : R.a.pick_u[e];
    }
    bool done;
    int result = WIN_DRAW;
    double ret;
    if (L.env.kind == ENV_CARTPOLE) {
        int d = 0;
        if (lane == 0) d = arena_cartpole_step(L, e, a) ? 1 : 0;
        done = __shfl(d, 0) != 0;
        ret = (double)L.env.steps[e];  // reward 1 per step (the last one included)
        if (lane == 0) R.a.ret[e] = ret;
    } else {
        const int st = L.env.steps[e];
        int winner;
        arena_board_step(L, e, lane, a, winner, done);
        const int challenger = e < R.a.half ? 1 : 2;  // black in the lower half, white in the upper
        result = winner == 0 ? WIN_DRAW : (winner == challenger ? WIN_CHALLENGER : WIN_OPPONENT);
        ret = winner == 0 ? 0.0 : (winner == challenger ? 1.0 : -1.0);
        if (done && lane == 0) {
            L.env.steps[e] = st + 1;
            R.a.ret[e] = ret;
        }
    }
    if (lane == 0) {
        const int len = L.env.steps[e];
        R.a.length[e] = len;
        if (done) {
            R.a.live[e] = 0;
            R.a.winner[e] = result;
            atomicAdd(&R.a.totals[result - 1], 1ULL);
            atomicAdd(&R.a.totals[3], (unsigned long long)len);
            atomicSub(R.a.n_live, 1);
        }
    }
}

}  // namespace mz
