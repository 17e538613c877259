// mz_go.h -- Go on the device (MZ_ENV_GO): the board game in which a move removes whole connected groups, legality (suicide, ko) depends
// on the liberties of every group on the board, and the end is decided by flood-filling the empty regions.  muzero_amd.games.GoEnv is the
// definition; these kernels are held to it byte for byte.  The rules:
//   board     rows x cols, each 3 .. 19, point r * cols + c, empty at the start; players 1 (black, moves first) and 2 (white); nn = rows *
//             cols, nn + 2 actions.  A group is a 4-connected set of stones of one colour, a liberty an empty 4-neighbour of one of them.
//   placement (a < nn) the stone goes on the empty point a, then every opposing group without a liberty is removed.  Legal iff the point is
//             empty, it is not the ko point, and the mover's group containing the new stone has a liberty after those removals (suicide is
//             illegal, a "suicide" that captures is legal).
//   ko        a placement that captures exactly one stone, by a stone that is a one-stone group with exactly one liberty (the captured
//             point), forbids that point to the opponent on the next ply only; any ply, a pass included, clears it.  No superko.
//   pass      (a == nn) always legal, a real ply.       resign (a == nn + 1) -1 for the mover; legal iff allow_resign.
//   end       a resignation; a pass directly after a pass; or the ply that makes steps == max_plies, whatever the action.  The last two
//             end in a Tromp-Taylor area count: a colour's area is its stones plus every empty region whose neighbouring stones are all of
//             that colour.  Black wins iff 2 * black_area > 2 * white_area + komi2, white iff less, equal is a draw; the final mover gets
//             +1, -1 or 0.
//   history   both colours' planes advance on every ply, pass included, as in Othello.  The side to move switches, and the mask is
//             rebuilt, only if the game goes on.
// The state lives in EnvState as for the other board games (bn = columns, nn = points, `board` one byte per point, `planes` the two
// colours' four history planes); the ko point (int, -1: none) and the "previous ply was a pass" flag are two per-env arrays of the
// planner's, carried in GoRules.
//
// Layout: ONE WORKGROUP PER ENV, ONE THREAD PER POINT (block = nn rounded up to 64, at most 384), cell classes and group values in LDS.
// One rule implementation, go_step<ARENA>.  Its core is one primitive, go_propagate: over the 4-connected components of equal cell class
// (black, white, empty) carry a pair of values to the fixed point, the first under min, the second under max (an `or` of flags is a max
// of 0 / 1, its negation a min).  Every round each cell takes the min / max over itself and its neighbours of its own class, so after k
// rounds a cell holds the reduction over all cells within k steps inside its component; a component of m cells has diameter < m, so fewer
// than nn rounds reach the fixed point and THE LOOP IS BOUNDED BY nn ROUNDS.  The only earlier exit is __syncthreads_or("changed") == 0,
// which is uniform over the workgroup.  No thread leaves before a barrier the others reach: frozen and out-of-range envs are decided per
// workgroup before any barrier, and every branch around a barrier depends on the action, the step count and the pass flag only, which
// all threads of the workgroup load alike.  No atomics but the existing counters', no spin, nothing between workgroups.
//   liberties  seed each stone with the smallest and the largest index of its own empty neighbours (sentinels GO_NONE_LO / GO_NONE_HI
//              without one) and propagate: then every stone knows its group's liberties -- none (hi < 0), exactly one (lo == hi, and
//              which), or at least two (lo < hi).
//   captures   after the placement: the opposing stones with hi < 0.          ko: one captured stone, the new stone has no neighbour of
//              its own colour and exactly one empty neighbour after the removal.
//   mask       a second propagation on the board without the captured stones; an empty point is legal for the next side iff it is not
//              the ko point and it has an empty neighbour, or touches an own group with lo < hi (a liberty elsewhere), or touches an
//              opposing group with lo == hi (this point is its only liberty: the placement captures).  That is the suicide test.
//   count      the same primitive over the empty cells: min of "touches no black", max of "touches white".
// A move: ONE batch of loads, the rule, ONE batch of stores -- both histories shifted, the next side's observation, mask, board, cur / opp,
// ko, pass flag, counters -- or the fresh game through the same stores (self-play), or nothing but the final board, captures included
// (arena: a finished game is frozen).  The result depends on nothing but the position.  Launch-latency-sized, as all of mz_env.h.
#pragma once
#include "mz_arena.h"

namespace mz {

constexpr int ENV_GO = 10;
constexpr int GO_MAX_POINTS = 384;  // 19 * 19 = 361 rounded up to whole waves
constexpr int GO_NONE_LO = 0x7fff, GO_NONE_HI = -1;

struct GoRules {
    int rows, cols;
    int komi2;         // twice the komi
    int max_plies;     // resolved: 1 .. 2 * nn
    int allow_resign;
    int temp_steps;    // the board schedule: 1.0 for the first temp_steps moves of an episode, then 0.1
    int* ko;           // [B] the point forbidden to the side to move (-1: none)
    int* passf;        // [B] 1: the previous ply was a pass
};

struct GoLaunch {
    EnvLaunch L;
    GoRules G;
};

struct GoShared {
    short lo[GO_MAX_POINTS], hi[GO_MAX_POINTS];
    signed char cls[GO_MAX_POINTS];  // 0 empty, 1 black, 2 white, 3 off the board (threads past nn)
    int cap, ko;
};

inline int go_block(int nn) { return (nn + 63) / 64 * 64; }

// the four neighbours of point t (-1: off the board)
__device__ __forceinline__ void go_neighbours(int t, int rows, int cols, int nn, int nb[4]) {
    const int r = t / cols, c = t - r * cols;
    const bool on = t < nn;
    nb[0] = on && r > 0 ? t - cols : -1;
    nb[1] = on && r < rows - 1 ? t + cols : -1;
    nb[2] = on && c > 0 ? t - 1 : -1;
    nb[3] = on && c < cols - 1 ? t + 1 : -1;
}

// THE primitive: (lo, hi) of every cell becomes (min, max) over its 4-connected component of equal class in S.cls.  At most nn rounds (see
// the top of the file); the early exit is workgroup-uniform.  S.cls must be visible (a barrier since its last store); on return S.lo /
// S.hi hold every cell's result and are visible.
__device__ inline void go_propagate(GoShared& S, int t, int cell, const int nb[4], int nn, int& lo, int& hi) {
    S.lo[t] = (short)lo;
    S.hi[t] = (short)hi;
    __syncthreads();
    for (int round = 0; round < nn; round++) {
        int l = lo, h = hi;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int q = nb[k];
            if (q >= 0 && S.cls[q] == cell) {
                const int ql = S.lo[q], qh = S.hi[q];
                l = ql < l ? ql : l;
                h = qh > h ? qh : h;
            }
        }
        if (!__syncthreads_or(l != lo || h != hi)) break;  // every read of this round is done; nothing changed anywhere: the fixed point
        lo = l; hi = h;
        S.lo[t] = (short)lo;
        S.hi[t] = (short)hi;
        __syncthreads();
    }
}

// a stone's own liberties: the smallest and the largest index of its empty neighbours
__device__ __forceinline__ void go_seed_liberties(const GoShared& S, int cell, const int nb[4], int& lo, int& hi) {
    lo = GO_NONE_LO; hi = GO_NONE_HI;
    if (cell == 1 || cell == 2) {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int q = nb[k];
            if (q >= 0 && S.cls[q] == 0) { lo = q < lo ? q : lo; hi = q > hi ? q : hi; }
        }
    }
}

// a fresh game (GoEnv.reset) by env e's workgroup: thread t writes point t, as the step's own fresh-game stores do
__device__ inline void go_fresh(const EnvLaunch& L, const GoRules& G, int e, int t) {
    const int nn = L.env.nn, A = L.env.A;
    signed char* pl = L.env.planes + (size_t)e * 8 * nn;
    float* o = L.obs + (size_t)e * 9 * nn;
    if (t < nn) {
        L.env.board[(size_t)e * nn + t] = 0;
        for (int k = 0; k < 8; k++) { pl[k * nn + t] = 0; o[k * nn + t] = 0.0f; }
        o[8 * nn + t] = 1.0f;
        L.mask[(size_t)e * A + t] = 1;
    }
    if (t != 0) return;
    L.env.steps[e] = 0;
    L.env.episode[e] = 0;
    L.mask[(size_t)e * A + nn] = 1;
    L.mask[(size_t)e * A + nn + 1] = (unsigned char)(G.allow_resign != 0);
    G.ko[e] = -1;
    G.passf[e] = 0;
    L.env.player[e] = 1;
    L.cur[e] = 1;
    L.opp[e] = 2;
}

// one workgroup per env (grid = B, block = go_block(nn))
__global__ void __launch_bounds__(GO_MAX_POINTS) k_go_reset(const GoLaunch P) {
    const EnvLaunch& L = P.L;
    const int e = blockIdx.x, t = threadIdx.x;
    if (e == 0 && t == 0)
        for (int i = 0; i < 4; i++) L.env.counters[i] = 0;
    if (e >= L.B) return;
    go_fresh(L, P.G, e, t);
}

// before the search of a move (k_env_pre with this game's own switch step)
__global__ void k_go_pre(const GoLaunch P) {
    const EnvLaunch& L = P.L;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= L.B) return;
    double T = L.temperature;
    if (T < 0.0) T = L.env.steps[e] < P.G.temp_steps ? 1.0 : 0.1;
    L.temp_out[e] = T;
    L.env.r_player[(size_t)L.slot * L.B + e] = L.cur[e];
}

// GoEnv.step of env e with action a, by the whole workgroup (thread t = point t; threads past nn only keep the barriers).  ARENA = false: a
// finished game resets at once (self-play); true: it is frozen -- only the final board is written.  `winner`: the winning colour (0:
// none); `reward`: the mover's.
template <bool ARENA>
__device__ inline void go_step(const EnvLaunch& L, const GoRules& G, GoShared& S, int e, int t, int a, int& winner, float& reward, bool& done) {
    const int rows = G.rows, cols = G.cols, nn = L.env.nn, A = L.env.A;
    signed char* b = L.env.board + (size_t)e * nn;
    signed char* pl = L.env.planes + (size_t)e * 8 * nn;
    const bool on = t < nn;
    // the pre-move state, one batch (plane 3 of either colour falls out of the history: not loaded)
    const int me = L.env.player[e], opp = 3 - me, st = L.env.steps[e], pass_prev = G.passf[e];
    int cell = on ? b[t] : 3;
    signed char raw[2][3];
#pragma unroll
    for (int c = 0; c < 2; c++)
#pragma unroll
        for (int k = 0; k < 3; k++) raw[c][k] = on ? pl[(4 * c + k) * nn + t] : (signed char)0;
    int nb[4];
    go_neighbours(t, rows, cols, nn, nb);
    const bool placed = a >= 0 && a < nn, passed = a == nn, resign = a > nn;
    winner = 0;
    reward = 0.0f;
    done = resign || (passed && pass_prev != 0) || st + 1 == G.max_plies;
    if (placed && t == a) cell = me;
    S.cls[t] = (signed char)cell;
    if (t == 0) { S.cap = -1; S.ko = -1; }
    __syncthreads();
    int lo, hi;
    if (placed) {  // (uniform) the captures and the ko point
        go_seed_liberties(S, cell, nb, lo, hi);
        go_propagate(S, t, cell, nb, nn, lo, hi);
        const bool captured = cell == opp && hi < 0;
        const int ncap = __syncthreads_count(captured);
        if (captured) { cell = 0; S.cap = t; S.cls[t] = 0; }
        __syncthreads();
        if (ncap == 1 && t == a) {
            int own = 0, empty = 0;
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (nb[k] >= 0) { own += S.cls[nb[k]] == me; empty += S.cls[nb[k]] == 0; }
            if (own == 0 && empty == 1) S.ko = S.cap;
        }
    }
    bool legal = false;
    int ko = -1;
    if (!done) {  // (uniform) the next side's placements, on the board without the captured stones
        go_seed_liberties(S, cell, nb, lo, hi);
        go_propagate(S, t, cell, nb, nn, lo, hi);
        ko = S.ko;  // (stored before the propagation's first barrier)
        if (cell == 0 && t != ko) {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int q = nb[k];
                if (q < 0) continue;
                const int qc = S.cls[q];
                const bool one = S.lo[q] == S.hi[q];  // a group with exactly one liberty: this point
                legal = legal || qc == 0 || (qc == opp && !one) || (qc == me && one);  // opp moves next
            }
        }
    } else if (!resign) {  // (uniform) the area count: empty regions by what they touch
        bool tb = false, tw = false;
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (nb[k] >= 0) { tb = tb || S.cls[nb[k]] == 1; tw = tw || S.cls[nb[k]] == 2; }
        lo = cell == 0 && tb ? 0 : 1;  // min: 0 iff the region touches black
        hi = cell == 0 && tw ? 1 : 0;  // max: 1 iff the region touches white
        go_propagate(S, t, cell, nb, nn, lo, hi);
        const int black = __syncthreads_count(cell == 1 || (cell == 0 && lo == 0 && hi == 0));
        const int white = __syncthreads_count(cell == 2 || (cell == 0 && lo == 1 && hi == 1));
        const int diff = 2 * black - 2 * white - G.komi2;  // > 0: black wins
        if (diff != 0) {
            winner = diff > 0 ? 1 : 2;
            reward = winner == me ? 1.0f : -1.0f;
        }
    }
    if (resign) {  // the mover loses
        reward = -1.0f;
        winner = opp;
    }
    if (ARENA && done) {  // the final position, captures included; planes, observation, mask and player stay as they were
        if (on) b[t] = (signed char)cell;
        return;
    }
    // what is stored: the position after the move and the histories shifted, or (self-play, the game is over) the fresh game
    const bool fresh = done;
    const int next = fresh ? 1 : opp;
    if (on) {
        if (fresh) { cell = 0; legal = true; }
        signed char h[2][4];  // the two colours' histories after this ply: [stones now, plane 0, plane 1, plane 2]
        h[0][0] = (signed char)(cell == 1);
        h[1][0] = (signed char)(cell == 2);
#pragma unroll
        for (int c = 0; c < 2; c++)
#pragma unroll
            for (int k = 0; k < 3; k++) h[c][k + 1] = fresh ? (signed char)0 : raw[c][k];
        float* o = L.obs + (size_t)e * 9 * nn;
        b[t] = (signed char)cell;
        const int own = next - 1;  // the next side to move sees its own history first
#pragma unroll
        for (int k = 0; k < 4; k++) {
            pl[k * nn + t] = h[0][k];
            pl[(4 + k) * nn + t] = h[1][k];
            o[(2 * k) * nn + t] = (float)(own == 0 ? h[0][k] : h[1][k]);
            o[(2 * k + 1) * nn + t] = (float)(own == 0 ? h[1][k] : h[0][k]);
        }
        o[8 * nn + t] = next == 1 ? 1.0f : 0.0f;
        L.mask[(size_t)e * A + t] = (unsigned char)legal;
    }
    if (t == 0) {
        L.mask[(size_t)e * A + nn] = 1;
        L.mask[(size_t)e * A + nn + 1] = (unsigned char)(G.allow_resign != 0);
        G.ko[e] = fresh ? -1 : ko;
        G.passf[e] = fresh ? 0 : (int)passed;
        if (fresh) {
            atomicAdd(&L.env.counters[2], 1ULL);
            atomicAdd(&L.env.counters[3], (unsigned long long)(st + 1));
            L.env.steps[e] = 0;
            L.env.episode[e] += 1;
        } else {
            L.env.steps[e] = st + 1;
        }
        L.env.player[e] = next;
        L.cur[e] = next;
        L.opp[e] = 3 - next;
    }
}

// after the search: env.step(action), record, auto-reset; one workgroup per env (grid = B)
__global__ void __launch_bounds__(GO_MAX_POINTS) k_go_step(const GoLaunch P) {
    __shared__ GoShared S;
    const int e = blockIdx.x, t = threadIdx.x;
    if (e >= P.L.B) return;  // (per workgroup)
    const int a = P.L.action[e];
    int winner;
    float reward;
    bool done;
    go_step<false>(P.L, P.G, S, e, t, a, winner, reward, done);
    if (t == 0) env_record(P.L, e, a, reward, done);
}

// ---- arena (mz_arena.h's bookkeeping around the same step) ----
struct GoArena {
    ArenaLaunch R;
    GoRules G;
};

__global__ void __launch_bounds__(GO_MAX_POINTS) k_go_arena_reset(const GoArena Q) {
    const ArenaLaunch& R = Q.R;
    const EnvLaunch& L = R.L;
    const int e = blockIdx.x, t = threadIdx.x;
    if (e == 0 && t == 0) {
        for (int i = 0; i < 4; i++) { L.env.counters[i] = 0; R.a.totals[i] = 0; }
        *R.a.n_live = L.B;
    }
    if (e >= L.B) return;
    go_fresh(L, Q.G, e, t);
    if (t != 0) return;
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

// opening and random-opponent moves: k_arena_pick's draw, legal[floor(u * n_legal)], over the placements and the pass (entries 0 .. nn
// of the mask) -- a random move never resigns.  One thread per env.
__global__ void k_go_arena_pick(const GoArena Q) {
    const ArenaLaunch& R = Q.R;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= R.a.B) return;
    const ArenaSeg& s = arena_seg_of(R, e);
    if (s.obs || !R.a.live[e]) return;  // searched, or frozen
    const int A = R.L.env.A, n_pick = A - 1;
    const bool opening = s.side == SIDE_OPENING;
    Philox g(R.L.seed, (unsigned)(opening && R.a.half ? e % R.a.half : e), (unsigned)R.ply, opening ? ARENA_STREAM_OPENING : ARENA_STREAM_RANDOM);
    const double u = g.uniform();
    const unsigned char* m = R.a.mask + (size_t)e * A;
    int n = 0;
    for (int c = 0; c < n_pick; c++) n += m[c] != 0;
    if (n == 0) return;  // (cannot happen: the pass is always legal)
    int k = (int)(u * (double)n);
    if (k > n - 1) k = n - 1;
    int chosen = -1;
    for (int c = 0; c < n_pick && chosen < 0; c++)
        if (m[c] != 0 && k-- == 0) chosen = c;
    R.a.pick[e] = chosen;
    R.a.pick_u[e] = u;
}

// k_arena_step for this game: one workgroup per env (grid = B)
__global__ void __launch_bounds__(GO_MAX_POINTS) k_go_arena_step(const GoArena Q) {
    __shared__ GoShared S;
    const ArenaLaunch& R = Q.R;
    const EnvLaunch& L = R.L;
    const int e = blockIdx.x, t = threadIdx.x;
    if (e >= R.a.B || !R.a.live[e]) return;  // (per workgroup) a frozen env's searched output is discarded
    const ArenaSeg& s = arena_seg_of(R, e);
    const int A = L.env.A, i = e - s.lo;
    const bool searched = s.obs != nullptr;
    int a = searched ? s.action[i] : R.a.pick[e];
    a = a < 0 ? 0 : (a >= A ? A - 1 : a);
    // the "after acting" half of the record
    for (int k = t; k < A; k += blockDim.x) R.a.r_pi[(size_t)e * A + k] = searched ? s.pi[(size_t)i * A + k] : 0.0;
    if (t == 0) {
        R.a.r_action[e] = a;
        R.a.r_side[e] = s.side;
        R.a.r_root[e] = searched ? s.root[i] : 0.0;
        R.a.r_u[e] = searched ? 0.0 : R.a.pick_u[e];
    }
    const int st = L.env.steps[e];
    int winner;
    float reward;
    bool done;
    go_step<true>(L, Q.G, S, e, t, a, winner, reward, done);
    if (t == 0) {
        const int challenger = e < R.a.half ? 1 : 2;  // black in the lower half, white in the upper
        const int result = winner == 0 ? WIN_DRAW : (winner == challenger ? WIN_CHALLENGER : WIN_OPPONENT);
        const int len = st + 1;
        if (done) L.env.steps[e] = len;
        R.a.length[e] = len;
        if (done) {
            R.a.ret[e] = winner == 0 ? 0.0 : (winner == challenger ? 1.0 : -1.0);
            R.a.live[e] = 0;
            R.a.winner[e] = result;
            atomicAdd(&R.a.totals[result - 1], 1ULL);
            atomicAdd(&R.a.totals[3], (unsigned long long)len);
            atomicSub(R.a.n_live, 1);
        }
    }
}

}  // namespace mz
