// mz_connect4.h -- Connect Four on the device (MZ_ENV_CONNECT4): the two-player board game whose board is not square and whose action
// count (one per column, plus resign) is not tied to its point count.  muzero_amd.games.ConnectFourEnv is the definition; these kernels
// are held to it byte for byte.  The state lives in EnvState as for the other board games -- bn = columns, nn = rows * columns, win,
// `board` one byte per point (0 empty, 1 black, 2 white; point = row * cols + column, row rows - 1 is the bottom), `planes` the two
// colours' four history planes -- so the arena's records and the compact replay states read what they always read.
//
// One rule implementation, c4_step<ARENA>, by the 16 lanes of an env's group (16 consecutive lanes of one wave, all active):
//   1. ONE batch of loads: action, player, step count, and per lane up to four points (nn <= 64) of the board and of the eight history
//      planes (both colours: whose move it is comes back with the same batch);
//   2. the two colours' 64-bit bitboards from ballots over the board bytes (bit = point); gravity and the column-full test from the
//      occupancy (stones in the column = popcount under the column mask); the win test walks the eight rays from the placed stone
//      on the mover's bitboard with explicit row and column bounds, so no line continues across a row edge;
//   3. ONE batch of stores: history shift, the next side's observation, mask, board, cur / opp, counters -- or the reset (self-play),
//      or nothing but the final stone (arena: a finished game is frozen).
// Two global round trips per move.  These kernels are launch-latency-sized (a few hundred bytes per env), as all of mz_env.h.
#pragma once
#include "mz_arena.h"

namespace mz {

constexpr int ENV_CONNECT4 = 8;

struct C4Launch {
    EnvLaunch L;
    int rows, cols;
    int temp_steps;  // the board schedule: 1.0 for the first temp_steps moves of an episode, then 0.1
};

__device__ __forceinline__ unsigned long long c4_bit(int p) { return 1ULL << p; }

// stones of `stones` in a row from (r, c) exclusive in direction (dr, dc): stops at the board's edges, so a line never wraps
__device__ inline int c4_ray(unsigned long long stones, int rows, int cols, int r, int c, int dr, int dc) {
    int k = 0;
    r += dr; c += dc;
    while (r >= 0 && r < rows && c >= 0 && c < cols && ((stones >> (r * cols + c)) & 1ULL)) { k++; r += dr; c += dc; }
    return k;
}

__device__ inline unsigned long long c4_column_mask(int rows, int cols, int c) {
    unsigned long long m = 0;
    for (int r = 0; r < rows; r++) m |= c4_bit(r * cols + c);
    return m;
}

// a fresh game (ConnectFourEnv.reset), one thread per env
__device__ inline void c4_fresh(const EnvLaunch& L, int e) {
    const int nn = L.env.nn, A = L.env.A;
    for (int i = 0; i < nn; i++) L.env.board[(size_t)e * nn + i] = 0;
    for (int i = 0; i < 8 * nn; i++) L.env.planes[(size_t)e * 8 * nn + i] = 0;
    for (int a = 0; a < A; a++) L.mask[(size_t)e * A + a] = 1;
    float* o = L.obs + (size_t)e * 9 * nn;
    for (int i = 0; i < 8 * nn; i++) o[i] = 0.0f;
    for (int i = 0; i < nn; i++) o[8 * nn + i] = 1.0f;
    L.env.player[e] = 1;
    L.cur[e] = 1;
    L.opp[e] = 2;
}

__global__ void k_c4_reset(const C4Launch P) {
    const EnvLaunch& L = P.L;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e == 0)
        for (int i = 0; i < 4; i++) L.env.counters[i] = 0;
    if (e >= L.B) return;
    L.env.steps[e] = 0;
    L.env.episode[e] = 0;
    c4_fresh(L, e);
}

// before the search of a move (k_env_pre with this game's own switch step)
__global__ void k_c4_pre(const C4Launch P) {
    const EnvLaunch& L = P.L;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= L.B) return;
    double T = L.temperature;
    if (T < 0.0) T = L.env.steps[e] < P.temp_steps ? 1.0 : 0.1;
    L.temp_out[e] = T;
    L.env.r_player[(size_t)L.slot * L.B + e] = L.cur[e];
}

// ConnectFourEnv.step of env e with action a (the same in all 16 lanes).  ARENA = false: a finished game resets at once (self-play);
// true: it is frozen -- only the final stone is placed.  `winner`: the winning colour (0: none); `reward`: the mover's.
template <bool ARENA>
__device__ inline void c4_step(const C4Launch& P, int e, int lane, int a, int& winner, float& reward, bool& done) {
    const EnvLaunch& L = P.L;
    const int rows = P.rows, cols = P.cols, nn = L.env.nn, A = L.env.A;
    signed char* b = L.env.board + (size_t)e * nn;
    signed char* pl = L.env.planes + (size_t)e * 8 * nn;
    // the pre-move state, one batch: lane owns points lane, lane + 16, lane + 32, lane + 48 of the board and of all eight history planes
    // (both colours: whose move it is comes back with the same batch)
    const int me = L.env.player[e], opp = 3 - me, st = L.env.steps[e];
    signed char bi[4], raw[8][4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int i = lane + 16 * j, q = i < nn ? i : 0;
        bi[j] = b[q];
#pragma unroll
        for (int k = 0; k < 8; k++) raw[k][j] = pl[k * nn + q];
    }
    signed char* mine = pl + (me - 1) * 4 * nn;
    const bool is_black = me == 1;  // planes 0-3: black's history, 4-7: white's
    signed char m[3][4], t[4][4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
#pragma unroll
        for (int k = 0; k < 3; k++) m[k][j] = is_black ? raw[k][j] : raw[4 + k][j];
#pragma unroll
        for (int k = 0; k < 4; k++) t[k][j] = is_black ? raw[4 + k][j] : raw[k][j];
    }
    const int base = (int)(__lane_id() & 48u);
    unsigned long long black = 0, white = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const bool cell = lane + 16 * j < nn;
        black |= ((__ballot(cell && bi[j] == 1) >> base) & 0xffffULL) << (16 * j);
        white |= ((__ballot(cell && bi[j] == 2) >> base) & 0xffffULL) << (16 * j);
    }
    const unsigned long long occ = black | white, full = nn == 64 ? ~0ULL : c4_bit(nn) - 1ULL;
    winner = 0;
    reward = 0.0f;
    int p = -1, row = -1;  // the placed stone's point and row
    const int c = a < 0 ? 0 : a;
    unsigned long long my_stones = me == 1 ? black : white;
    if (a >= cols) {  // resign: the mover loses
        reward = -1.0f;
        winner = opp;
    } else {
        const int height = __popcll(occ & c4_column_mask(rows, cols, c));  // gravity: stones already in the column
        row = height < rows ? rows - 1 - height : 0;                       // (a full column is masked out of the search: never reached)
        p = row * cols + c;
        my_stones |= c4_bit(p);
        if (st >= (L.env.win - 1) * 2) {  // the family's gate, with the pre-increment step count
            const int dirs[4][2] = {{0, 1}, {1, 0}, {1, 1}, {-1, 1}};
            for (int d = 0; d < 4; d++)
                if (1 + c4_ray(my_stones, rows, cols, row, c, dirs[d][0], dirs[d][1]) + c4_ray(my_stones, rows, cols, row, c, -dirs[d][0], -dirs[d][1]) >= L.env.win)
                    winner = me;
            if (winner) reward = 1.0f;
        }
    }
    done = winner != 0 || (p >= 0 && (occ | c4_bit(p)) == full);  // the win is tested first: a win on the last empty cell is a win
    float* o = L.obs + (size_t)e * 9 * nn;
    if (!done) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int i = lane + 16 * j;
            if (i < nn) {
                const signed char nm0 = (signed char)((my_stones >> i) & 1ULL);  // the mover's history after this move: [stones now, m0, m1, m2]
                mine[i] = nm0; mine[nn + i] = m[0][j]; mine[2 * nn + i] = m[1][j]; mine[3 * nn + i] = m[2][j];
                // observation of the next side to move: its own history, the mover's, the colour plane
                o[0 * nn + i] = (float)t[0][j]; o[1 * nn + i] = (float)nm0;
                o[2 * nn + i] = (float)t[1][j]; o[3 * nn + i] = (float)m[0][j];
                o[4 * nn + i] = (float)t[2][j]; o[5 * nn + i] = (float)m[1][j];
                o[6 * nn + i] = (float)t[3][j]; o[7 * nn + i] = (float)m[2][j];
                o[8 * nn + i] = opp == 1 ? 1.0f : 0.0f;
                if (i == p) b[i] = (signed char)me;
            }
        }
        if (lane == 0) {
            if (row == 0) L.mask[(size_t)e * A + c] = 0;  // the column's top cell is taken
            L.env.player[e] = opp;
            L.env.steps[e] = st + 1;
            L.cur[e] = opp;
            L.opp[e] = me;
        }
    } else if (ARENA) {
        if (lane == 0 && p >= 0) b[p] = (signed char)me;  // the final position; planes, observation, mask and player stay as they were
    } else {  // auto-reset: c4_fresh by the group
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int i = lane + 16 * j;
            if (i < nn) {
                b[i] = 0;
#pragma unroll
                for (int k = 0; k < 8; k++) { pl[k * nn + i] = 0; o[k * nn + i] = 0.0f; }
                o[8 * nn + i] = 1.0f;
            }
        }
        for (int k = lane; k < A; k += 16) L.mask[(size_t)e * A + k] = 1;
        if (lane == 0) {
            atomicAdd(&L.env.counters[2], 1ULL);
            atomicAdd(&L.env.counters[3], (unsigned long long)(st + 1));
            L.env.steps[e] = 0;
            L.env.episode[e] += 1;
            L.env.player[e] = 1;
            L.cur[e] = 1;
            L.opp[e] = 2;
        }
    }
}

// after the search: env.step(action), record, auto-reset; 16 threads per env, as k_env_step
__global__ void k_c4_step(const C4Launch P) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x, e = g >> 4, lane = g & 15;
    if (e >= P.L.B) return;
    const int a = P.L.action[e];
    int winner;
    float reward;
    bool done;
    c4_step<false>(P, e, lane, a, winner, reward, done);
    if (lane == 0) env_record(P.L, e, a, reward, done);
}

// ---- arena (mz_arena.h's bookkeeping around the same step) ----
struct C4Arena {
    ArenaLaunch R;
    int rows, cols;
};

__global__ void k_c4_arena_reset(const C4Arena Q) {
    const ArenaLaunch& R = Q.R;
    const EnvLaunch& L = R.L;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e == 0) {
        for (int i = 0; i < 4; i++) { L.env.counters[i] = 0; R.a.totals[i] = 0; }
        *R.a.n_live = L.B;
    }
    if (e >= L.B) return;
    L.env.steps[e] = 0;
    L.env.episode[e] = 0;
    c4_fresh(L, e);
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

// opening and random-opponent moves: k_arena_pick's draw, legal[floor(u * n_legal)], over the COLUMNS only -- a random move never
// resigns.  One thread per env (at most 64 columns).
__global__ void k_c4_arena_pick(const C4Arena Q) {
    const ArenaLaunch& R = Q.R;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= R.a.B) return;
    const ArenaSeg& s = arena_seg_of(R, e);
    if (s.obs || !R.a.live[e]) return;  // searched, or frozen
    const int A = R.L.env.A, cols = Q.cols;
    const bool opening = s.side == SIDE_OPENING;
    Philox g(R.L.seed, (unsigned)(opening && R.a.half ? e % R.a.half : e), (unsigned)R.ply, opening ? ARENA_STREAM_OPENING : ARENA_STREAM_RANDOM);
    const double u = g.uniform();
    const unsigned char* m = R.a.mask + (size_t)e * A;
    int n = 0;
    for (int c = 0; c < cols; c++) n += m[c] != 0;
    if (n == 0) return;  // (cannot happen for a live env: a full board is a finished game)
    int k = (int)(u * (double)n);
    if (k > n - 1) k = n - 1;
    int chosen = -1;
    for (int c = 0; c < cols && chosen < 0; c++)
        if (m[c] != 0 && k-- == 0) chosen = c;
    R.a.pick[e] = chosen;
    R.a.pick_u[e] = u;
}

// k_arena_step for this game: 16 threads per env
__global__ void k_c4_arena_step(const C4Arena Q) {
    const ArenaLaunch& R = Q.R;
    const EnvLaunch& L = R.L;
    const int g = blockIdx.x * blockDim.x + threadIdx.x, e = g >> 4, lane = g & 15;
    if (e >= R.a.B || !R.a.live[e]) return;  // a frozen env's searched output is discarded
    const ArenaSeg& s = arena_seg_of(R, e);
    const int A = L.env.A, i = e - s.lo;
    const bool searched = s.obs != nullptr;
    int a = searched ? s.action[i] : R.a.pick[e];
    a = a < 0 ? 0 : (a >= A ? A - 1 : a);
    // the "after acting" half of the record
    for (int k = lane; k < A; k += 16) R.a.r_pi[(size_t)e * A + k] = searched ? s.pi[(size_t)i * A + k] : 0.0;
    if (lane == 0) {
        R.a.r_action[e] = a;
        R.a.r_side[e] = s.side;
        R.a.r_root[e] = searched ? s.root[i] : 0.0;
        R.a.r_u[e] = searched ? 0.0 : R.a.pick_u[e];
    }
    const int st = L.env.steps[e];
    C4Launch P{};
    P.L = L; P.rows = Q.rows; P.cols = Q.cols;
    int winner;
    float reward;
    bool done;
    c4_step<true>(P, e, lane, a, winner, reward, done);
    if (lane == 0) {
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
