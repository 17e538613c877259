// mz_extenv.h -- self-play on host-stepped environments (MZ_ENV_EXTERNAL): the two device halves of the reference's actor
// loop body (pipeline.py:91-113) around a host env.step.
//
//   act    : k_ext_ingest builds every env's observation -- StackFrameAndAction (gym_env.py:271-353) over the NEWEST
//            frame the host uploaded, newest first, with ScaledFloatFrame's x / 255 (gym_env.py:214-224) for uint8
//            frames -- into the search input and the record ring in one pass, records the player and picks the
//            temperature; the search runs; k_ext_record records action, pi and root value.
//   commit : k_ext_commit records reward and done, keeps the per-env step counts and counters[0..3], and flags an open
//            trajectory that has outgrown the record ring while a replay is attached (the device epilogue of mz_env.h
//            would read overwritten records).
//
// k_ext_ingest is the only kernel here that moves real bytes (C4: 512 envs x 8 planes x 96 x 96 float32, written twice:
// 302 MB per move; 4.7 MB of uint8 frames read): a streaming copy, one workgroup per (env, chunk of the observation),
// 16-byte stores.  The frame history is a per-env ring of S frames in HBM with a per-env head, so nothing
// shifts: output plane k (0 = newest) of a frame is history slot head - (k - 1) (k >= 1) or the uploaded frame (k = 0),
// and the uploaded frame is written to slot head + 1, which no reader of this launch touches.  The head is kept twice,
// indexed by the move's parity: a launch reads one copy and writes the other, so no workgroup sees another's update.
// Compact records (ExtLaunch::rr, RecRing in mz_env.h; stacked uint8 image frames): k_ext_ingest<VEC, true> writes the search input only and
// stores the uploaded frame's bytes as the move's record (C4: 151 MB of float32 records less per move, 4.7 MB of frame bytes more);
// k_rec_decode rebuilds a recorded move's float32 observations for mz_selfplay_read.
// uint8 frames: (float)b / 255.0f is IEEE division (no fast-math in muzero_amd/build.py FLAGS; hipcc's default
// -fhip-fp32-correctly-rounded-divide-sqrt), the float32 value numpy's astype(np.float32) / 255.0 gives.
#pragma once
#include <climits>

#include "mz_env.h"

namespace mz {

constexpr int ENV_EXTERNAL = 5;

struct ExtEnv {
    int S;          // stack_history; 0: the host uploads whole observations
    int image;      // frame [C,H,W] -> obs [S*(C+1),H,W]; else frame [D] -> obs [S, D+1]
    int C, HW;      // frame channels (vector frames: D) and plane size (vector frames: 1)
    int FE;         // frame elements, C * HW
    int u8;         // frames are uint8, scaled by 1 / 255
    int temp_steps; // temperature < 0: 1.0 for the first temp_steps moves of an episode, then 0.1
    void* frames;   // [B][FE] uploaded newest frames (uint8 or float32)
    void* hist;     // [B][S][FE] frame history ring (same element type)
    int* hist_act;  // [B][S] action history ring (the action that led to the frame in the same slot)
    int* head;      // [2][B] history head, by move parity
    float* reward;  // [B] uploaded rewards
    unsigned char* done;  // [B] uploaded done flags
    int* err;       // [1] smallest env whose open trajectory outgrew the record ring (INT_MAX: none)
    int* enc_err;   // [1] int8 replay states only: smallest env with an observation element int8 cannot hold (ReplayRing.enc_err), else null
};

struct ExtLaunch {
    EnvState env;
    ExtEnv x;
    int B, A, OD;        // envs, actions, observation floats per env
    int slot, prev_slot; // record slot of this move and of the previous one
    int first;           // first move after the reset: every env starts an episode
    int parity;          // move index & 1: head[parity] is read, head[parity ^ 1] written
    int sims;
    int check;           // a replay is attached: check trajectory length against the record ring
    long long move_abs;
    double temperature;
    float* obs;          // the search input [B][OD]
    const int* cur;
    double* temp_out;
    const int* action;
    const double* pi;
    const double* root;
    RecRing rr;          // compact record ring (rr.frames set): the uploaded frame is the move's record, r_obs does not exist
};

__device__ __forceinline__ float ext_frame_value(const ExtLaunch& L, const void* base, size_t i) {
    return L.x.u8 ? (float)static_cast<const unsigned char*>(base)[i] / 255.0f : static_cast<const float*>(base)[i];
}

// the action plane's value, float32 of the reference's (action + 1) / num_actions (a Python float, gym_env.py:333-336)
__device__ __forceinline__ float ext_action_value(int a, int A) { return (float)((double)(a + 1) / (double)A); }

// per-env bookkeeping of one act: action history and head, player record, temperature (one thread per env)
__device__ inline void ext_ingest_env(const ExtLaunch& L, int e, bool reset, int a) {
    const ExtEnv& X = L.x;
    if (X.S > 0) {
        int* ha = X.hist_act + (size_t)e * X.S;
        if (reset) {
            for (int k = 0; k < X.S; k++) ha[k] = 0;
            X.head[(size_t)(L.parity ^ 1) * L.B + e] = 0;
        } else {
            const int h = (X.head[(size_t)L.parity * L.B + e] + 1) % X.S;
            ha[h] = a;
            X.head[(size_t)(L.parity ^ 1) * L.B + e] = h;
        }
    }
    double T = L.temperature;
    if (T < 0.0) T = L.env.steps[e] < X.temp_steps ? 1.0 : 0.1;  // config.py:236-249 (k_env_pre's schedule)
    L.temp_out[e] = T;
    L.env.r_player[(size_t)L.slot * L.B + e] = L.cur[e];
}

// Where output element j of env e comes from: frame k (0 = newest) element `src`, or the action plane of frame k (src < 0).
__device__ __forceinline__ void ext_source(const ExtLaunch& L, int j, int& k, int& src) {
    const ExtEnv& X = L.x;
    if (X.S == 0) { k = 0; src = j; return; }
    if (X.image) {
        const int p = j / X.HW, i = j - p * X.HW;
        if (p < X.S * X.C) { k = p / X.C; src = (p - k * X.C) * X.HW + i; }
        else { k = p - X.S * X.C; src = -1; }
    } else {
        k = j / (X.C + 1);
        const int r = j - k * (X.C + 1);
        src = r < X.C ? r : -1;
    }
}

// One group of VEC consecutive output floats of env e starting at j0 (VEC = 1: any shape; VEC = 4: image frames whose plane size is a
// multiple of 4, so the group lies in one plane and reads one run of its source frame).
// REC (compact record ring: stacked uint8 image frames): no float32 record; the group that files the newest frame in the history also
// stores its bytes to the move's record slot.
template <int VEC, bool REC>
__device__ __forceinline__ void ext_ingest_group(const ExtLaunch& L, int e, int j0, bool reset, int a, int h, int hnew) {
    const ExtEnv& X = L.x;
    int k, src;
    ext_source(L, j0, k, src);
    float* o1 = L.obs + (size_t)e * L.OD + j0;
    float* o2 = nullptr;
    if constexpr (!REC) o2 = L.env.r_obs + ((size_t)L.slot * L.B + e) * L.OD + j0;
    float v[VEC];
    if (src < 0) {  // action plane: (a + 1) / A of the action that led to frame k; 0 for every plane after a reset
        const float f = ext_action_value(reset ? 0 : (k == 0 ? a : X.hist_act[(size_t)e * X.S + ((h - (k - 1)) % X.S + X.S) % X.S]), L.A);
#pragma unroll
        for (int q = 0; q < VEC; q++) v[q] = f;
    } else {
        const bool fresh = k == 0 || reset;  // the uploaded frame (after a reset: every history slot is that frame)
        const size_t off = fresh ? (size_t)e * X.FE + src : ((size_t)e * X.S + ((h - (k - 1)) % X.S + X.S) % X.S) * X.FE + src;
        const bool file = k == 0 && X.S > 0;  // this group owns its run of the newest frame: it also files it in the history
        const int t0 = reset ? 0 : hnew, t1 = reset ? X.S : hnew + 1;
        if (X.u8) {
            const unsigned char* s = static_cast<const unsigned char*>(fresh ? X.frames : X.hist) + off;
            if constexpr (VEC == 4) {
                const uint32_t w = *reinterpret_cast<const uint32_t*>(s);
#pragma unroll
                for (int q = 0; q < 4; q++) v[q] = (float)((w >> (8 * q)) & 0xffu) / 255.0f;
                if (file)
                    for (int t = t0; t < t1; t++) *reinterpret_cast<uint32_t*>(static_cast<unsigned char*>(X.hist) + ((size_t)e * X.S + t) * X.FE + src) = w;
                if constexpr (REC)
                    if (file) *reinterpret_cast<uint32_t*>(L.rr.frames + ((size_t)L.slot * L.B + e) * L.rr.stride + src) = w;
            } else {
                v[0] = (float)s[0] / 255.0f;
                if (file)
                    for (int t = t0; t < t1; t++) static_cast<unsigned char*>(X.hist)[((size_t)e * X.S + t) * X.FE + src] = s[0];
                if constexpr (REC)
                    if (file) L.rr.frames[((size_t)L.slot * L.B + e) * L.rr.stride + src] = s[0];
            }
        } else {
            const float* s = static_cast<const float*>(fresh ? X.frames : X.hist) + off;
            if constexpr (VEC == 4) {
                const float4 w = *reinterpret_cast<const float4*>(s);
                v[0] = w.x; v[1] = w.y; v[2] = w.z; v[3] = w.w;
                if (file)
                    for (int t = t0; t < t1; t++) *reinterpret_cast<float4*>(static_cast<float*>(X.hist) + ((size_t)e * X.S + t) * X.FE + src) = w;
            } else {
                v[0] = s[0];
                if (file)
                    for (int t = t0; t < t1; t++) static_cast<float*>(X.hist)[((size_t)e * X.S + t) * X.FE + src] = s[0];
            }
        }
    }
    if constexpr (VEC == 4) {
        const float4 w = make_float4(v[0], v[1], v[2], v[3]);
        *reinterpret_cast<float4*>(o1) = w;
        if constexpr (!REC) *reinterpret_cast<float4*>(o2) = w;
    } else {
        *o1 = v[0];
        if constexpr (!REC) *o2 = v[0];
    }
}

// blockIdx.y = env, blockIdx.x = chunk of the env's observation.  VEC = 4 (image frames, plane size a multiple of 4): every thread
// moves ITER groups of four floats, the groups of one pass lane-consecutive, so each wave-wide store is 1 KiB contiguous (16 bytes per
// lane: float32 frames load 16 bytes per lane too, uint8 frames 4).  VEC = 1: one float per thread (vector frames, odd planes).
constexpr int EXT_ITER = 4;

template <int VEC, bool REC = false>
__global__ __launch_bounds__(256) void k_ext_ingest(const ExtLaunch L) {
    const ExtEnv& X = L.x;
    const int e = blockIdx.y;
    const size_t prev = (size_t)L.prev_slot * L.B + e;
    const bool reset = L.first || L.env.r_done[prev] != 0;
    const int a = reset ? 0 : L.env.r_action[prev];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if constexpr (REC) L.rr.age[(size_t)L.slot * L.B + e] = reset ? 0 : L.env.steps[e];  // (before ext_ingest_env: same thread, no race)
        ext_ingest_env(L, e, reset, a);
    }
    const int h = X.S > 0 && !reset ? X.head[(size_t)L.parity * L.B + e] : 0;
    const int hnew = reset || X.S == 0 ? 0 : (h + 1) % X.S;
    constexpr int iters = VEC == 4 ? EXT_ITER : 1;
#pragma unroll
    for (int it = 0; it < iters; it++) {
        const int j0 = ((blockIdx.x * iters + it) * blockDim.x + threadIdx.x) * VEC;
        if (j0 < L.OD) ext_ingest_group<VEC, REC>(L, e, j0, reset, a, h, hnew);
    }
}

// mz_selfplay_read on a compact record ring: the float32 observations [B][OD] of the move in slot L.slot, rebuilt by the window rule
// (RecRing, mz_env.h) into L.obs -- k_ext_ingest's geometry (ext_source) and values (ext_frame_value, ext_action_value), so what a
// reader gets is what the search saw.  Grid and VEC as k_ext_ingest: VEC = 4 stores 16 bytes per lane.
template <int VEC>
__global__ __launch_bounds__(256) void k_rec_decode(const ExtLaunch L) {
    const RecRing& Q = L.rr;
    const int e = blockIdx.y, R = L.env.ring_len;
    const int age = Q.age[(size_t)L.slot * L.B + e];
    constexpr int iters = VEC == 4 ? EXT_ITER : 1;
#pragma unroll
    for (int it = 0; it < iters; it++) {
        const int j0 = ((blockIdx.x * iters + it) * blockDim.x + threadIdx.x) * VEC;
        if (j0 >= L.OD) continue;
        int k, src;
        ext_source(L, j0, k, src);
        float v[VEC];
        if (src < 0) {
            const float f = ext_action_value(k < age ? L.env.r_action[(size_t)((L.slot + R - k - 1) % R) * L.B + e] : 0, L.A);
#pragma unroll
            for (int q = 0; q < VEC; q++) v[q] = f;
        } else {
            const unsigned char* s = Q.frames + ((size_t)((L.slot + R - (k < age ? k : age)) % R) * L.B + e) * Q.stride;
#pragma unroll
            for (int q = 0; q < VEC; q++) v[q] = ext_frame_value(L, s, (size_t)src + q);
        }
        float* o = L.obs + (size_t)e * L.OD + j0;
        if constexpr (VEC == 4) *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
        else *o = v[0];
    }
}

// after the search: the move's action, policy and root value into the record slot (one thread per (env, action))
__global__ void k_ext_record(const ExtLaunch L) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= L.B * L.A) return;
    const int e = i / L.A, a = i - e * L.A;
    const size_t rec = (size_t)L.slot * L.B + e;
    L.env.r_pi[rec * L.A + a] = L.pi[i];
    if (a == 0) {
        L.env.r_action[rec] = L.action[e];
        L.env.r_root[rec] = L.root[e];
    }
}

// commit: the outcome of the acted move (reward, done) into the record slot, step counts and counters as the device envs keep
// them (env_record, board_step_*), and the record ring's capacity check of the device epilogue
__global__ void k_ext_commit(const ExtLaunch L) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= L.B) return;
    const size_t rec = (size_t)L.slot * L.B + e;
    const bool done = L.x.done[e] != 0;
    L.env.r_reward[rec] = L.x.reward[e];
    L.env.r_done[rec] = done ? 1 : 0;
    const int st = L.env.steps[e];
    if (done) {
        atomicAdd(&L.env.counters[2], 1ULL);
        atomicAdd(&L.env.counters[3], (unsigned long long)(st + 1));
        L.env.steps[e] = 0;
        L.env.episode[e] += 1;
    } else {
        L.env.steps[e] = st + 1;
    }
    if (e == 0) {
        atomicAdd(&L.env.counters[0], (unsigned long long)L.B);
        atomicAdd(&L.env.counters[1], (unsigned long long)L.B * (unsigned long long)L.sims);
    }
    // the epilogue reads positions ep_start .. move_abs of the env's open trajectory from the record ring: all of them must still be there
    // (compact records: and the rr.extra = S moves before ep_start that the first position's window reaches back to)
    if (L.check && L.move_abs + 1 - L.env.ep_start[e] > (long long)(L.env.ring_len - L.rr.extra)) atomicMin(L.x.err, e);
}

}  // namespace mz
