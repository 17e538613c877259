// mz_othello.h -- Othello on the device (MZ_ENV_OTHELLO): the board game in which a move changes more than one point (a placement flips
// up to about a dozen stones in eight directions), legality depends on the whole position (the mask is rebuilt every ply), a side without
// a placement must pass (a real ply: games are longer than the point count), and the game ends by counting when neither side can place --
// so a normal placement can earn its mover -1 or 0.  muzero_amd.games.OthelloEnv is the definition; these kernels are held to it byte for
// byte.  Actions: a < nn places on point a = row * cols + column, nn passes, nn + 1 resigns.  The state lives in EnvState as for the other
// board games -- bn = columns, nn = rows * columns (<= 64), `board` one byte per point (0 empty, 1 black, 2 white), `planes` the two
// colours' four history planes -- so the arena's records and the compact replay states read what they always read.  Unlike the other
// board games BOTH colours' histories advance on every ply, pass included: plane k of colour p holds p's stones as they stood k plies
// ago, so a flipped stone leaves its old owner's newest plane.
//
// One rule implementation, oth_step<ARENA>, by the 16 lanes of an env's group (16 consecutive lanes of one wave, all active), on
// mz_connect4.h's shape:
//   1. ONE batch of loads: action, player, step count, and per lane up to four points of the board and of the six history planes that survive the shift;
//   2. the two colours' 64-bit bitboards from ballots over the board bytes (bit = point).  A direction is a shift by 1, cols - 1, cols or
//      cols + 1, left or right, under a mask that clears the column the shift wraps into (derived from cols) and everything past bit nn.
//      The EIGHT DIRECTIONS ARE SPREAD OVER THE LANES: lane l works on direction l & 7.  The flips of the chosen point: the run of
//      opposing stones from the point in the lane's direction (at most max(rows, cols) - 2 propagation steps), kept iff the cell after it
//      holds a stone of the mover; an OR over the 8 lanes (three shuffles) gives the flip set.  The legal placements of BOTH colours on the
//      position after the move: lanes 0-7 flood black's stones through white's in their direction, lanes 8-15 white's through black's,
//      the step after the run lands on an empty cell; one OR over each half.  So a move costs two flood fills per lane, not sixteen;
//   3. the end test (neither colour can place), the count by __popcll after the flips, the next mask (placements, or pass; resign);
//   4. ONE batch of stores: both histories shifted, the next side's observation, mask, board, cur / opp, counters -- or the fresh game
//      (self-play), or nothing but the final board, flips included (arena: a finished game is frozen).
// Two global round trips per move.  These kernels are launch-latency-sized (a few hundred bytes per env), as all of mz_env.h.
#pragma once
#include "mz_arena.h"

namespace mz {

constexpr int ENV_OTHELLO = 9;

struct OthLaunch {
    EnvLaunch L;
    int rows, cols;
    int temp_steps;  // the board schedule: 1.0 for the first temp_steps moves of an episode, then 0.1
};

typedef unsigned long long oth_bb;

// one of the eight directions as a masked shift
struct OthDir {
    int sh;       // 1, cols - 1, cols, cols + 1
    bool left;    // towards higher points
    oth_bb keep;  // the cells a shifted stone may land on: not the column the shift wraps into, and below bit nn
};

__device__ __forceinline__ oth_bb oth_full(int nn) { return nn == 64 ? ~0ULL : (1ULL << nn) - 1ULL; }

__device__ inline oth_bb oth_column(int rows, int cols, int c) {
    oth_bb m = 0;
    for (int r = 0; r < rows; r++) m |= 1ULL << (r * cols + c);
    return m;
}

// direction d in 0..7: 0 east (+1), 1 south-west (+cols - 1), 2 south (+cols), 3 south-east (+cols + 1), 4-7 their opposites
__device__ inline OthDir oth_dir(int d, int rows, int cols) {
    const int k = d & 3;
    OthDir D;
    D.sh = k == 0 ? 1 : cols + k - 2;
    D.left = d < 4;
    const oth_bb full = oth_full(rows * cols);
    const oth_bb not_first = full & ~oth_column(rows, cols, 0), not_last = full & ~oth_column(rows, cols, cols - 1);
    // the column moves by +1 for east and south-east, by -1 for south-west (left shifts); mirrored for the right shifts; not at all for south / north
    const int dc = k == 2 ? 0 : (k == 1 ? -1 : 1) * (D.left ? 1 : -1);
    D.keep = dc == 0 ? full : (dc > 0 ? not_first : not_last);
    return D;
}

__device__ __forceinline__ oth_bb oth_shift(oth_bb x, const OthDir& D) { return (D.left ? x << D.sh : x >> D.sh) & D.keep; }

// OR over the 8 lanes that share lane >> 3
__device__ __forceinline__ oth_bb oth_or8(oth_bb v) {
    v |= __shfl_xor(v, 1); v |= __shfl_xor(v, 2); v |= __shfl_xor(v, 4);
    return v;
}

// in direction D: the cells on which `mine` may place because of a run of `theirs` in that direction
__device__ inline oth_bb oth_moves_dir(oth_bb mine, oth_bb theirs, const OthDir& D, int reach) {
    oth_bb t = oth_shift(mine, D) & theirs;
    for (int i = 1; i < reach; i++) t |= oth_shift(t, D) & theirs;
    return oth_shift(t, D) & ~(mine | theirs);
}

// in direction D: the stones of `theirs` that a stone of `mine` placed on `spot` (one bit) flips
__device__ inline oth_bb oth_flips_dir(oth_bb spot, oth_bb mine, oth_bb theirs, const OthDir& D, int reach) {
    oth_bb run = oth_shift(spot, D) & theirs;
    for (int i = 1; i < reach; i++) run |= oth_shift(run, D) & theirs;
    return (oth_shift(run, D) & ~run & mine) ? run : 0ULL;  // the cell after the run: a stone of the mover anchors it
}

// all eight directions by one thread (the resets)
__device__ inline oth_bb oth_moves_serial(oth_bb mine, oth_bb theirs, int rows, int cols) {
    const int reach = (rows > cols ? rows : cols) - 2;
    oth_bb m = 0;
    for (int d = 0; d < 8; d++) m |= oth_moves_dir(mine, theirs, oth_dir(d, rows, cols), reach);
    return m;
}

__device__ inline void oth_start(int rows, int cols, oth_bb& black, oth_bb& white) {
    const int r0 = rows / 2 - 1, c0 = cols / 2 - 1;
    white = (1ULL << (r0 * cols + c0)) | (1ULL << ((r0 + 1) * cols + c0 + 1));
    black = (1ULL << (r0 * cols + c0 + 1)) | (1ULL << ((r0 + 1) * cols + c0));
}

// a fresh game (OthelloEnv.reset), one thread per env
__device__ inline void oth_fresh(const OthLaunch& P, int e) {
    const EnvLaunch& L = P.L;
    const int nn = L.env.nn, A = L.env.A;
    oth_bb black, white;
    oth_start(P.rows, P.cols, black, white);
    const oth_bb moves = oth_moves_serial(black, white, P.rows, P.cols);
    signed char* pl = L.env.planes + (size_t)e * 8 * nn;
    float* o = L.obs + (size_t)e * 9 * nn;
    for (int i = 0; i < nn; i++) {
        const int bk = (int)((black >> i) & 1ULL), wh = (int)((white >> i) & 1ULL);
        L.env.board[(size_t)e * nn + i] = (signed char)(bk + 2 * wh);
        for (int k = 0; k < 8; k++) { pl[k * nn + i] = 0; o[k * nn + i] = 0.0f; }
        pl[i] = (signed char)bk; pl[4 * nn + i] = (signed char)wh;
        o[i] = (float)bk; o[nn + i] = (float)wh;
        o[8 * nn + i] = 1.0f;
        L.mask[(size_t)e * A + i] = (unsigned char)((moves >> i) & 1ULL);
    }
    L.mask[(size_t)e * A + nn] = moves == 0;
    L.mask[(size_t)e * A + nn + 1] = 1;
    L.env.player[e] = 1;
    L.cur[e] = 1;
    L.opp[e] = 2;
}

__global__ void k_oth_reset(const OthLaunch P) {
    const EnvLaunch& L = P.L;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e == 0)
        for (int i = 0; i < 4; i++) L.env.counters[i] = 0;
    if (e >= L.B) return;
    L.env.steps[e] = 0;
    L.env.episode[e] = 0;
    oth_fresh(P, e);
}

// before the search of a move (k_env_pre with this game's own switch step)
__global__ void k_oth_pre(const OthLaunch P) {
    const EnvLaunch& L = P.L;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= L.B) return;
    double T = L.temperature;
    if (T < 0.0) T = L.env.steps[e] < P.temp_steps ? 1.0 : 0.1;
    L.temp_out[e] = T;
    L.env.r_player[(size_t)L.slot * L.B + e] = L.cur[e];
}

// OthelloEnv.step of env e with action a (the same in all 16 lanes).  ARENA = false: a finished game resets at once (self-play); true:
// it is frozen -- only the final board is written.  `winner`: the winning colour (0: none); `reward`: the mover's.
template <bool ARENA>
__device__ inline void oth_step(const OthLaunch& P, int e, int lane, int a, int& winner, float& reward, bool& done) {
    const EnvLaunch& L = P.L;
    const int rows = P.rows, cols = P.cols, nn = L.env.nn, A = L.env.A;
    signed char* b = L.env.board + (size_t)e * nn;
    signed char* pl = L.env.planes + (size_t)e * 8 * nn;
    // the pre-move state, one batch: lane owns points lane, lane + 16, lane + 32, lane + 48 of the board and of the older history planes
    // (plane 3 of either colour falls out of the history: not loaded)
    const int me = L.env.player[e], opp = 3 - me, st = L.env.steps[e];
    signed char bi[4], raw[2][3][4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int i = lane + 16 * j, q = i < nn ? i : 0;
        bi[j] = b[q];
#pragma unroll
        for (int c = 0; c < 2; c++)
#pragma unroll
            for (int k = 0; k < 3; k++) raw[c][k][j] = pl[(4 * c + k) * nn + q];
    }
    const int base = (int)(__lane_id() & 48u);
    oth_bb black = 0, white = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const bool cell = lane + 16 * j < nn;
        black |= ((__ballot(cell && bi[j] == 1) >> base) & 0xffffULL) << (16 * j);
        white |= ((__ballot(cell && bi[j] == 2) >> base) & 0xffffULL) << (16 * j);
    }
    const int reach = (rows > cols ? rows : cols) - 2;
    const OthDir D = oth_dir(lane & 7, rows, cols);
    // (self-play) the fresh game's placements, by the same lanes: a constant of the launch, computed outside every branch
    oth_bb start_black, start_white;
    oth_start(rows, cols, start_black, start_white);
    const oth_bb start_moves = ARENA ? 0ULL : oth_or8(oth_moves_dir(start_black, start_white, D, reach));
    winner = 0;
    reward = 0.0f;
    const bool resign = a > nn, placed = a < nn;
    // the flips of the chosen point: one direction per lane (the two halves of the group do the same work), OR over 8 lanes
    if (placed) {
        const oth_bb spot = 1ULL << (a < 0 ? 0 : a);
        const oth_bb mine = me == 1 ? black : white, theirs = me == 1 ? white : black;
        const oth_bb flips = oth_or8(oth_flips_dir(spot, mine, theirs, D, reach));
        if (me == 1) { black |= spot | flips; white &= ~flips; }
        else { white |= spot | flips; black &= ~flips; }
    }
    // both colours' placements on the position after the move: lanes 0-7 black's, lanes 8-15 white's
    const bool low = lane < 8;
    const oth_bb half_moves = oth_or8(oth_moves_dir(low ? black : white, low ? white : black, D, reach));
    const oth_bb other_moves = __shfl_xor(half_moves, 8);
    const oth_bb moves_black = low ? half_moves : other_moves, moves_white = low ? other_moves : half_moves;
    done = false;
    if (resign) {  // the mover loses
        reward = -1.0f;
        winner = opp;
        done = true;
    } else if (placed && (moves_black | moves_white) == 0) {  // neither side can place (the full board included): count after the flips
        const int nb = __popcll(black), nw = __popcll(white), mine = me == 1 ? nb : nw, theirs = me == 1 ? nw : nb;
        done = true;
        if (mine > theirs) { reward = 1.0f; winner = me; }
        else if (mine < theirs) { reward = -1.0f; winner = opp; }
    }
    if (ARENA && done) {  // the final position, flips included; planes, observation, mask and player stay as they were
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int i = lane + 16 * j;
            if (i < nn) b[i] = (signed char)(((black >> i) & 1ULL) + 2 * ((white >> i) & 1ULL));
        }
        return;
    }
    // what is stored: the position after the move and the histories shifted, or (self-play, the game is over) the fresh game
    const bool fresh = done;
    oth_bb next_moves = opp == 1 ? moves_black : moves_white;
    int next = opp;
    if (fresh) {
        black = start_black; white = start_white;
        next_moves = start_moves;
        next = 1;
    }
    float* o = L.obs + (size_t)e * 9 * nn;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int i = lane + 16 * j;
        if (i < nn) {
            signed char h[2][4];  // the two colours' histories after this ply: [stones now, plane 0, plane 1, plane 2]
            h[0][0] = (signed char)((black >> i) & 1ULL);
            h[1][0] = (signed char)((white >> i) & 1ULL);
#pragma unroll
            for (int c = 0; c < 2; c++)
#pragma unroll
                for (int k = 0; k < 3; k++) h[c][k + 1] = fresh ? (signed char)0 : raw[c][k][j];
            b[i] = (signed char)(h[0][0] + 2 * h[1][0]);
            const int own = next - 1;  // the next side to move sees its own history first
#pragma unroll
            for (int k = 0; k < 4; k++) {
                pl[k * nn + i] = h[0][k];
                pl[(4 + k) * nn + i] = h[1][k];
                o[(2 * k) * nn + i] = (float)(own == 0 ? h[0][k] : h[1][k]);
                o[(2 * k + 1) * nn + i] = (float)(own == 0 ? h[1][k] : h[0][k]);
            }
            o[8 * nn + i] = next == 1 ? 1.0f : 0.0f;
        }
    }
    for (int k = lane; k < A; k += 16)
        L.mask[(size_t)e * A + k] = k < nn ? (unsigned char)((next_moves >> k) & 1ULL) : (k == nn ? (unsigned char)(next_moves == 0) : (unsigned char)1);
    if (lane == 0) {
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

// after the search: env.step(action), record, auto-reset; 16 threads per env, as k_env_step
__global__ void k_oth_step(const OthLaunch P) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x, e = g >> 4, lane = g & 15;
    if (e >= P.L.B) return;
    const int a = P.L.action[e];
    int winner;
    float reward;
    bool done;
    oth_step<false>(P, e, lane, a, winner, reward, done);
    if (lane == 0) env_record(P.L, e, a, reward, done);
}

// ---- arena (mz_arena.h's bookkeeping around the same step) ----
struct OthArena {
    ArenaLaunch R;
    int rows, cols;
};

__global__ void k_oth_arena_reset(const OthArena Q) {
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
    OthLaunch P{};
    P.L = L; P.rows = Q.rows; P.cols = Q.cols;
    oth_fresh(P, e);
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

// opening and random-opponent moves: k_arena_pick's draw, legal[floor(u * n_legal)], over the placements or the pass (entries 0 .. nn
// of the mask) -- a random move never resigns.  One thread per env (at most 65 entries).
__global__ void k_oth_arena_pick(const OthArena Q) {
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
    if (n == 0) return;  // (cannot happen for a live env: a side without a placement has the pass)
    int k = (int)(u * (double)n);
    if (k > n - 1) k = n - 1;
    int chosen = -1;
    for (int c = 0; c < n_pick && chosen < 0; c++)
        if (m[c] != 0 && k-- == 0) chosen = c;
    R.a.pick[e] = chosen;
    R.a.pick_u[e] = u;
}

// k_arena_step for this game: 16 threads per env
__global__ void k_oth_arena_step(const OthArena Q) {
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
    OthLaunch P{};
    P.L = L; P.rows = Q.rows; P.cols = Q.cols;
    int winner;
    float reward;
    bool done;
    oth_step<true>(P, e, lane, a, winner, reward, done);
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
