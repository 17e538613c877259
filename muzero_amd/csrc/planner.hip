// planner.hip -- host side of libmzplanner_hip.so: the C ABI of include/mzplanner.h over the gfx950 kernels
// in mz_search.h / mz_mlp.h / mz_env.h (MLP nets: one fused LDS-resident kernel per move) and mz_conv.h / mz_convnet.h
// (conv nets: HBM-resident trees + MFMA conv towers, a short kernel sequence per simulation).
// One planner handle == one GPU, one HIP stream, all state in HBM.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/mzplanner.h"
#include "mz_env.h"
#include "mz_arena.h"
#include "mz_arena_image.h"
#include "mz_extenv.h"
#include "mz_catch.h"
#include "mz_breakout.h"
#include "mz_connect4.h"
#include "mz_othello.h"
#include "mz_go.h"
#include "mz_search.h"
#include "mz_search_fast.h"
#include "mz_convnet.h"

using namespace mz;

static thread_local std::string g_err;

static int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

#define HIPCHK(expr)                                                                                          \
    do {                                                                                                      \
        hipError_t _e = (expr);                                                                               \
        if (_e != hipSuccess)                                                                                 \
            return fail(MZ_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e) + " (" + __FILE__ + ":" + \
                                      std::to_string(__LINE__) + ")");                                       \
    } while (0)

struct HostTensor {
    std::vector<float> data;
    std::vector<int64_t> shape;
};

static const char* kMlpNames[L_COUNT] = {
    "represent_net.net.0",          "represent_net.net.2",          "dynamics_net.transition_net.0", "dynamics_net.transition_net.2",
    "dynamics_net.reward_net.0",    "dynamics_net.reward_net.2",    "prediction_net.policy_net.0",   "prediction_net.policy_net.2",
    "prediction_net.value_net.0",   "prediction_net.value_net.2",
};

// The compiled builds of the tuned kernel k_search_fast<planes, TR = TV = tiles, FUSE, AC, kFastHW, SPB> (mz_search_fast.h), one entry
// each.  A handle's family (planes, tiles, ac) is fixed at create; a launch adds FUSE (env step in the kernel) and SPB.
struct FastKey {
    int planes, tiles, ac;  // ac: the action count as a constant (10, 4, 2) or 0
    bool fuse, spb;
};
struct FastBuild {
    FastKey key;
    const void* fn;
};
#define MZ_FB(PL, T, F, AC, SPB) {{PL, T, AC, F, SPB}, reinterpret_cast<const void*>(&k_search_fast<PL, T, T, F, AC, kFastHW, SPB>)}
#define MZ_FB4(PL, T) MZ_FB(PL, T, false, 0, false), MZ_FB(PL, T, false, 2, false), MZ_FB(PL, T, true, 0, false), MZ_FB(PL, T, true, 2, false)
static const FastBuild kFastBuilds[] = {
    // ten actions and MSE heads (TicTacToe's MLP net, config.py:106-136); SPB: the board games' self-play settings as constants
    MZ_FB(256, 1, false, 10, false), MZ_FB(256, 1, true, 10, false), MZ_FB(256, 1, false, 10, true), MZ_FB(256, 1, true, 10, true),
    // four actions, categorical heads, the 512-plane net (LunarLander's shape)
    MZ_FB(512, 2, false, 4, false), MZ_FB(512, 2, true, 4, false),
    // categorical heads by (planes, head tiles); AC = 2: two actions, single player (classic control)
    MZ_FB4(256, 1), MZ_FB4(512, 2),
#ifndef MZ_DEV_SHAPES  // development builds: only the C2 / C3 shapes (a third of the compile time); the others run the generic kernel
    MZ_FB4(256, 2), MZ_FB4(512, 1),
#endif
};
#undef MZ_FB4
#undef MZ_FB

static const FastBuild* fast_find(const FastKey& k) {
    for (const FastBuild& b : kFastBuilds)
        if (b.key.planes == k.planes && b.key.tiles == k.tiles && b.key.ac == k.ac && b.key.fuse == k.fuse && b.key.spb == k.spb) return &b;
    return nullptr;
}

// the name mz_planner_describe reports for a k_search_fast launch
static std::string fast_name(const FastKey& k, bool own_layout) {
    char b[160];
    snprintf(b, sizeof b, "k_search_fast<planes=%d, TR=%d, TV=%d, FUSE=%s, AC=%d, HW=%s%s> (LDS trees%s, one launch per move)", k.planes, k.tiles, k.tiles,
             k.fuse ? "true" : "false", k.ac, kFastHW ? "true" : "false", k.spb ? ", SPB=true" : "", own_layout ? ", own carve-out" : "");
    return b;
}

// Device reload (mz_pack.h): the bound tensors, the source maps decoded from the host packers, and the tables the gather kernels read
struct BoundTensor {
    const float* d;
    std::vector<int64_t> shape;
    size_t numel;
};
struct PackState {
    std::map<std::string, BoundTensor> bound;
    bool maps_valid = false;   // false: the next refresh derives the maps (names or shapes changed)
    bool srcs_dirty = true;    // a bound address changed: upload the source table
    bool table_in_flight = false;  // an upload from the pinned tables was enqueued since the stream was last drained
    std::vector<PackTensor> tensors;  // tensor ids = the order of `bound` when the maps were derived
    std::vector<size_t> buf_bytes;
    std::vector<int> buf_kind;
    PackEntry* d_map = nullptr;
    PackChunk *d_chunks_f32 = nullptr, *d_chunks_w3 = nullptr;
    int n_chunks_f32 = 0, n_chunks_w3 = 0;
    PackSrc *d_srcs = nullptr, *h_srcs = nullptr;  // h_*: pinned
    void **d_dst = nullptr, **h_dst = nullptr;
    hipEvent_t ev_in = nullptr, ev_out = nullptr;
    long long bytes_read = 0, bytes_written = 0;  // per refresh: entries + sources, destinations
    void free_maps() {
        for (void* b : {(void*)d_map, (void*)d_chunks_f32, (void*)d_chunks_w3, (void*)d_srcs, (void*)d_dst})
            if (b) (void)hipFree(b);
        if (h_srcs) (void)hipHostFree(h_srcs);
        if (h_dst) (void)hipHostFree(h_dst);
        d_map = nullptr; d_chunks_f32 = d_chunks_w3 = nullptr; d_srcs = h_srcs = nullptr; d_dst = h_dst = nullptr;
        n_chunks_f32 = n_chunks_w3 = 0;
        maps_valid = false;
    }
};

struct mz_planner {
    mz_config cfg;
    int device = 0;
    hipStream_t stream = nullptr;
    std::map<std::string, HostTensor> params;
    bool committed = false;

    MlpNet net{};
    MlpLds o{};
    float* d_w[L_COUNT] = {};
    float* d_b[L_COUNT] = {};
    SearchParams sp{};   // tree_mode 0 layout
    SearchParams sp2{};  // tree_mode 2 layout (valid if tree2_ok)
    bool tree2_ok = false;
    int lds_mode0 = 0, lds_mode2 = 0;
    // tree_mode 2 behind the TUNED kernel's own, smaller network carve-out (k_search_fast keeps the num_planes-wide layers in registers: of
    // the generic H1 / V1 buffers it uses 16 KiB each, for its K-split partial tiles): lets four-action, 50-simulation searches at
    // num_planes 512 (the LunarLander-shaped configuration) fit 160 KiB.  Only used when the generic carve-out does not fit.
    SearchParams sp2f{};
    bool tree2f_ok = false;
    int lds_mode2f = 0, fast_delta = 0;
    double* d_ftab_tri = nullptr;
    InferParams ip{};
    // tuned kernel for the benchmark shapes (mz_search_fast.h): per-wave weight streams of the wide layers
    FastKey fast{};            // its build family (planner_init); planes 0: the shape-generic kernel only
    bool fast_mse = false;     // the tuned kernel's shape, but an MSE head outside the ten-action build: the shape-generic kernel
    bool fast_layout = false;  // k_search_fast runs in its own LDS carve-out (sp2f) unless a search is scripted
    bool tree_old = false;       // MZ_TREE_OLD=1: evaluate every level on every descent (A/B measurements, tests)
    bool force_generic = false;  // MZ_FORCE_GENERIC=1: run the shape-generic kernel (A/B measurements, tests)
    int hwx = -1;  // k_search_fast helper-wave work split (MZ_HWX=0..3 overrides the default: A/B measurements)
    std::string last_dispatch = "none yet";  // what the last search launch ran (mz_planner_describe)
    float* d_stream[1] = {};
    float* d_bias_all = nullptr;
    double *d_dbg_noise = nullptr, *d_dbg_utie = nullptr, *d_dbg_ufinal = nullptr;  // mz_debug_capture_rng
    FastWeights fw{};

    // per-env device buffers (capacity cfg.num_envs)
    float* d_obs = nullptr;
    unsigned char* d_mask = nullptr;
    int *d_cur = nullptr, *d_opp = nullptr;
    double* d_temp = nullptr;
    double *d_noise = nullptr, *d_utie = nullptr, *d_ufinal = nullptr;
    float* d_hidden = nullptr;
    double* d_ftab = nullptr;
    int* d_action = nullptr;
    double *d_pi = nullptr, *d_root = nullptr;
    int* d_visits = nullptr;
    int* d_err = nullptr;
    long long* d_stamps = nullptr;
    // scripted hook
    float *d_spi0 = nullptr, *d_svalues = nullptr, *d_srewards = nullptr;
    int *d_tparent = nullptr, *d_taction = nullptr;
    // inference API buffers
    float *d_inf_in = nullptr, *d_inf_hidden = nullptr, *d_inf_reward = nullptr, *d_inf_value = nullptr, *d_inf_pi = nullptr;
    int* d_inf_action = nullptr;
    int inf_cap = 0;

    // conv nets (MZ_NET_BOARD / MZ_NET_ATARI): network, HBM tree regions and the per-simulation exchange buffers
    bool conv = false;
    // MLP nets whose trees do not fit the LDS-resident kernels (many simulations, > 64 actions; MZ_HBM_TREE=1 forces it): the
    // HBM tree kernels around k_infer launches, one (select, inference, backup) triple per simulation
    bool hbm_tree = false;
    SearchParams spg{};  // tree layout inside a per-workgroup HBM region (hbm_tree)
    float* d_pi_scratch = nullptr;
    ConvNetDev cnet{};
    unsigned char* d_regions = nullptr;
    float *d_pi0 = nullptr, *d_sim_reward = nullptr, *d_sim_value = nullptr;
    const float** d_srcptrs = nullptr;
    float **d_dstptrs = nullptr, **d_rootptrs = nullptr;
    int* d_sim_action = nullptr;

    // self-play
    EnvState env{};
    int env_kind = MZ_ENV_NONE;
    unsigned int move_counter = 0;
    int ring_len = 0, ring_pos = 0, ring_count = 0;
    bool has_replay = false;
    ReplayRing replay{};
    int* d_epi_off = nullptr;        // per-env slot offsets of the move being written (k_epi_scan)
    long long* d_epi_ctr = nullptr;  // reserved write cursor of the attached replay ring (k_epilogue reserves, k_epi_publish commits)
    long long selfplay_moves = 0;  // moves since mz_selfplay_reset
    int c4_temp_steps = 6;         // MZ_ENV_CONNECT4: the board temperature schedule's switch step
    int oth_temp_steps = 6;        // MZ_ENV_OTHELLO: likewise
    GoRules go{};                  // MZ_ENV_GO: the rules of the last reset and the two per-env arrays (ko point, pass flag)
    int go_cap = 0;                // envs the two arrays hold
    // host-stepped envs (MZ_ENV_EXTERNAL): device side of the frames / history, pinned staging of every upload and download
    ExtEnv ext{};
    int ext_od = 0;
    bool ext_pending = false;  // an act is waiting for its commit
    bool ext_broken = false;   // a commit found an open trajectory longer than the record ring: reset before anything else
    void* h_ext_frames = nullptr;
    unsigned char *h_ext_mask = nullptr, *h_ext_done = nullptr;
    int *h_ext_cur = nullptr, *h_ext_opp = nullptr, *h_ext_action = nullptr, *h_ext_err = nullptr;
    float* h_ext_reward = nullptr;
    RecRing rr{};                  // compact record ring (MZ_RECORD_FRAMES_U8; rr.frames null: float32 records in env.r_obs)
    int rec_S = 0;                 // its stack_history
    float* d_rec_stage = nullptr;  // [B][obs] one move of decoded observations (mz_selfplay_read, allocated by the first read)
    std::tuple<Catch, Breakout> games{};  // the device image games (mz_grid_game.h): the state of the one being played; frames, rewards and done flags are ext's buffers

    // arena (mz_arena.h): evaluation games in lock-step on this handle's env state
    ArenaState arena{};
    bool arena_open = false;
    int arena_ply = 0;
    mz_planner* arena_q = nullptr;  // the borrowed opponent planner (MZ_ARENA_PLANNER)
    int arena_img = 0;              // IMGARENA_CATCH / _BREAKOUT / _EXTERNAL: the roots come from ext's frame history (mz_arena_image.h)
    bool arena_pending = false;     // host-stepped arena: an act is waiting for its commit
    std::vector<unsigned char> arena_live_h;  // host-stepped arena: the live flags (the host uploads every done flag, so it knows them)
    hipEvent_t ev_arena_pre = nullptr, ev_arena_q = nullptr;  // order the two planners' streams within a ply

    // weights bound in device memory (mz_planner_bind_param_device / mz_planner_refresh_params; mz_pack.h)
    struct PackState* pk = nullptr;
    bool params_touched = false;  // a commit or refresh was called: mz_planner_set_tower_precision is no longer legal

    // profiling
    bool profiling = false;
    hipEvent_t ev_begin = nullptr, ev_end = nullptr;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> kev;
    size_t kev_used = 0;
};

static int obs_dim(const mz_config& c) { return c.obs_c * c.obs_h * c.obs_w; }
static int pad16(int x) { return (x + 15) & ~15; }

extern "C" const char* mz_last_error(void) { return g_err.c_str(); }
extern "C" const char* mz_version(void) { return "mzplanner 0.1 (gfx950)"; }

// Which kernel build this handle's last search launch dispatched to, and every diagnostic switch as this handle read it (mzplanner.h)
static thread_local std::string g_describe;
extern "C" const char* mz_planner_describe(mz_planner* p) {
    if (!p) return "null planner";
    char b[512];
    const ConvSwitches& cs = conv_switches();
    snprintf(b, sizeof b,
             "; switches: MZ_FORCE_GENERIC=%d MZ_HWX=%d MZ_TREE_OLD=%d MZ_HBM_TREE=%d"
             " | per process: MZ_ACTION_SPARSE=%d MZ_ACTION_FUSE=%d MZ_CONV_SPEC=%d MZ_TOWER=%d MZ_CONV_TILE=%d MZ_CONV_G=%d MZ_CONV_NCT=%d",
             (int)p->force_generic, p->hwx, (int)p->tree_old, (int)p->hbm_tree, cs.action_sparse, cs.action_fuse, cs.conv_spec, cs.tower, cs.conv_tile, cs.conv_g, cs.conv_nct);
    g_describe = "search: " + p->last_dispatch + b;
    if (p->conv && p->cnet.split)  // the build conv_run_split dispatches this net's tower convs to (the same chooser)
        g_describe += std::string(" | conv_precision=bf16x3: ") + split_geometry(p->cnet.hh, p->cnet.hw, p->cnet.P).name + ", one launch per conv";
    else if (p->conv) g_describe += " | conv_precision=f32";
    if (p->conv && (p->cnet.split || p->cnet.tower_split)) {  // the fused split tower a num_envs-wide launch takes (tower_run's chooser)
        const TowerGeom g = split_tower_geometry(p->cfg.num_envs, p->cnet.P, p->cnet.hh, p->cnet.hw);
        g_describe += std::string(p->cnet.tower_split ? " | tower_precision=bf16x3: " : " | tower: ") +
                      (g.npt ? split_tower_name(g) + ", fused" : std::string("no fused split build (MZ_TOWER=0 or no geometry), one launch per conv"));
    } else if (p->conv) {
        g_describe += " | tower_precision=f32";
    }
    return g_describe.c_str();
}

// mzplanner.h: the fused towers of a conv net on k_res_tower_bf16x3 (mz_tower_split.h); everything else of the net stays as conv_precision says
extern "C" int mz_planner_set_tower_precision(mz_planner* p, int32_t precision) {
    if (!p) return fail(MZ_E_INVALID, "null planner");
    if (precision != MZ_TOWER_F32 && precision != MZ_TOWER_BF16X3) return fail(MZ_E_INVALID, "tower_precision must be MZ_TOWER_F32 (0) or MZ_TOWER_BF16X3 (1)");
    if (!p->conv) return fail(MZ_E_INVALID, "tower_precision needs a conv net: MZ_NET_MLP has no residual towers");
    if (p->params_touched) return fail(MZ_E_STATE, "tower_precision is set after mz_planner_create and before the first mz_planner_commit_params / mz_planner_refresh_params");
    if (precision == MZ_TOWER_BF16X3) {
        if (conv_switches().tower == 0) return fail(MZ_E_INVALID, "tower_precision MZ_TOWER_BF16X3 needs the fused towers: MZ_TOWER=0 is set");
        if (!split_tower_geometry(1, p->cnet.P, p->cnet.hh, p->cnet.hw).npt)
            return fail(MZ_E_INVALID, "tower_precision MZ_TOWER_BF16X3: this net has no fused-tower geometry (num_planes a multiple of 16 and <= 128, a hidden state of at most 96 pixels that fits the LDS)");
    }
    p->cnet.tower_split = precision == MZ_TOWER_BF16X3 ? 1 : 0;
    return MZ_OK;
}

static void compute_layout(mz_planner* p) {
    const mz_config& c = p->cfg;
    MlpNet& n = p->net;
    n.in_dim = obs_dim(c); n.A = c.num_actions; n.P = c.num_planes; n.H = c.hidden_dim;
    n.Sv = c.value_support_size; n.Sr = c.reward_support_size;
    n.in_pad = pad16(n.in_dim); n.h_pad = pad16(n.H); n.x_pad = n.h_pad + pad16(n.A); n.p_pad = pad16(n.P);
    const int dims[L_COUNT][2] = {{n.P, n.in_dim}, {n.H, n.P}, {n.P, n.H + n.A}, {n.H, n.P}, {n.P, n.H},
                                  {n.Sr, n.P},     {n.P, n.H}, {n.A, n.P},       {n.P, n.H}, {n.Sv, n.P}};
    for (int l = 0; l < L_COUNT; l++) {
        MlpLayer& L = n.L[l];
        L.n = dims[l][0]; L.k = dims[l][1];
        L.n_tiles = (L.n + 15) / 16;
        if (l == L_DYN0) {  // [hidden padded to 16 | one-hot action block(s)], summation order: mz_mlp.h header
            const int ab = (n.A + 15) / 16, a_last = n.A - 16 * (ab - 1);
            L.kg = n.h_pad / 16 + ab;
            L.last_steps = (a_last + 3) / 4;
        } else {
            L.kg = (L.k + 15) / 16;
            const int rem = L.k - 16 * (L.kg - 1);
            L.last_steps = rem < 4 ? rem : 4;
        }
        L.split = (l == L_REP1 || l == L_DYN1 || l == L_REW1 || l == L_POL1 || l == L_VAL1) ? 1 : 0;
        L.kq = (L.kg + 3) / 4;
    }
    MlpLds& o = p->o;
    int off = 0;
    const int xk = n.in_pad > n.x_pad ? n.in_pad : n.x_pad;
    o.X = off; off += xk * 16;
    o.H1 = off; off += n.p_pad * 16;
    o.V1 = off; off += n.p_pad * 16;
    o.HN = off; off += n.h_pad * 16;
    o.HS = off; off += n.h_pad * 16;
    int mx = n.A; mx = n.Sv > mx ? n.Sv : mx; mx = n.Sr > mx ? n.Sr : mx;
    o.lg_stride = pad16(mx) + 1;  // odd stride: 16 envs read their logits rows without LDS bank conflicts
    o.LG = off; off += ((2 * 16 * o.lg_stride + 3) & ~3);
    o.OUT = off; off += 64;
    o.BIAS = off;
    for (int l = 0; l < L_COUNT; l++) { n.L[l].b_lds = off; off += n.L[l].n_tiles * 16; }
    o.PM = off; off += 128;
    o.total_floats = off;

    // search kernel: tree part after the network part
    SearchParams& s = p->sp;
    s.net = n; s.o = o;
    s.S = c.num_simulations; s.A = c.num_actions; s.NN = c.num_simulations + 1;
    int b = o.total_floats * 4;
    auto take = [&](int bytes, int align) { b = (b + align - 1) / align * align; int r = b; b += bytes; return r; };
    s.t_nodes = take(16 * s.NN * (int)sizeof(TreeNode), 16);
    s.t_child = take(16 * s.NN * s.A * 2, 16);
    s.t_prior = take(16 * s.A * 8, 16);
    s.t_tmp = take(16 * s.A * 8, 16);
    s.t_pi0 = take(16 * s.A * 4, 16);
    s.t_mm = take(16 * 2 * 8, 16);
    s.t_sel = take(128 * 4, 16);
    s.t_ptr = take(32 * 8, 16);
    s.t_ftab = take((s.S + 1) * (s.S + 1) * 8, 16);
    s.lds_bytes = (b + 15) & ~15;
    // tree_mode 2 layout (mz_tree2.h) replaces t_nodes / t_child / t_ftab when it fits in LDS
    p->lds_mode0 = s.lds_bytes;
    p->tree2_ok = false;
    if (s.A <= 16 && s.NN < 255) {
        b = o.total_floats * 4;
        const int n2 = take(16 * s.NN * 16, 16), e2 = take(16 * s.NN * s.A * 16, 16), pr = take(16 * s.A * 8, 16), tm = take(16 * s.A * 8, 16),
                  p0 = take(16 * s.A * 4, 16), mmo = take(16 * 2 * 8, 16), se = take(128 * 4, 16), pt = take(32 * 8, 16),
                  ft = take(((s.S + 1) * (s.S + 2) / 2) * 8, 16), ca = take(16 * (s.NN + 1) * 16, 16), pa = take(16 * (s.NN + 3) * 2, 16),
                  ve = take(16 * 32, 16);
        const int total = (b + 15) & ~15;
        if (total <= 160 * 1024) {
            p->tree2_ok = true;
            p->lds_mode2 = total;
            p->sp2 = s;
            SearchParams& q = p->sp2;
            q.t2_nodes = n2; q.t2_entries = e2; q.t_prior = pr; q.t_tmp = tm; q.t_pi0 = p0; q.t_mm = mmo; q.t_sel = se; q.t_ptr = pt;
            q.t2_ftab = ft; q.t_cache = ca; q.t_path = pa; q.t_ver = ve;
            q.lds_bytes = total; q.tree_mode = 2;
        }
        constexpr int kFastPart = 4 * 4 * 256;  // floats of H1 / V1 the tuned kernel touches: [4 waves][<= 4 tiles] float4[64]
        if (!p->tree2_ok && n.p_pad * 16 > kFastPart) {
            const int delta = 2 * (n.p_pad * 16 - kFastPart);
            MlpLds of = o;
            of.V1 = o.H1 + kFastPart;
            of.HN -= delta; of.HS -= delta; of.LG -= delta; of.OUT -= delta; of.BIAS -= delta; of.PM -= delta; of.total_floats -= delta;
            b = of.total_floats * 4;
            const int n2 = take(16 * s.NN * 16, 16), e2 = take(16 * s.NN * s.A * 16, 16), pr = take(16 * s.A * 8, 16), tm = take(16 * s.A * 8, 16),
                      p0 = take(16 * s.A * 4, 16), mmo = take(16 * 2 * 8, 16), se = take(128 * 4, 16), pt = take(32 * 8, 16),
                      ft = take(((s.S + 1) * (s.S + 2) / 2) * 8, 16), ca = take(16 * (s.NN + 1) * 16, 16), pa = take(16 * (s.NN + 3) * 2, 16),
                      ve = take(16 * 32, 16);
            const int total = (b + 15) & ~15;
            if (total <= 160 * 1024) {
                p->tree2f_ok = true;
                p->lds_mode2f = total;
                p->fast_delta = delta;
                p->sp2f = s;
                SearchParams& q = p->sp2f;
                q.o = of;
                q.t2_nodes = n2; q.t2_entries = e2; q.t_prior = pr; q.t_tmp = tm; q.t_pi0 = p0; q.t_mm = mmo; q.t_sel = se; q.t_ptr = pt;
                q.t2_ftab = ft; q.t_cache = ca; q.t_path = pa; q.t_ver = ve;
                q.lds_bytes = total; q.tree_mode = 2;
            }
        }
    }

    InferParams& ip = p->ip;
    ip.net = n; ip.o = o;
    b = o.total_floats * 4;
    ip.t_ptr = take(32 * 8, 16);
    ip.t_pi = take(16 * n.A * 4, 16);
    ip.t_act = take(16 * 4, 16);
    ip.lds_bytes = (b + 15) & ~15;
}

// conv nets: the tree part only, laid out from offset 0 of a per-workgroup HBM region (same structure as tree_mode 0 in LDS)
static void compute_layout_conv(mz_planner* p, SearchParams* target = nullptr) {
    const mz_config& c = p->cfg;
    SearchParams& s = target ? *target : p->sp;
    s.S = c.num_simulations; s.A = c.num_actions; s.NN = c.num_simulations + 1;
    int b = 0;
    auto take = [&](int bytes, int align) { b = (b + align - 1) / align * align; int r = b; b += bytes; return r; };
    s.t_nodes = take(16 * s.NN * (int)sizeof(TreeNode), 16);
    s.t_child = take(16 * s.NN * s.A * 2, 16);
    s.t_prior = take(16 * s.A * 8, 16);
    s.t_tmp = take(16 * s.A * 8, 16);
    s.t_pi0 = take(16 * s.A * 4, 16);
    s.t_mm = take(16 * 2 * 8, 16);
    s.t_sel = take(128 * 4, 16);
    s.t_ptr = take(32 * 8, 16);
    s.t_ftab = take((s.S + 1) * (s.S + 1) * 8, 16);
    s.lds_bytes = (b + 255) & ~255;
    s.tree_mode = 0;
    if (!target) {
        p->lds_mode0 = s.lds_bytes;
        p->tree2_ok = false;
    }
}

static int planner_init(mz_planner* p, bool conv);
extern "C" int mz_planner_destroy(mz_planner* p);

extern "C" int mz_planner_create(const mz_config* cfg, int device_id, mz_planner** out) {
    if (!cfg || !out) return fail(MZ_E_INVALID, "null argument");
    const bool conv = cfg->net_kind == MZ_NET_BOARD || cfg->net_kind == MZ_NET_ATARI;
    if (cfg->net_kind != MZ_NET_MLP && !conv) return fail(MZ_E_INVALID, "unknown net_kind");
    if (cfg->net_kind == MZ_NET_BOARD && (long long)cfg->obs_h * cfg->obs_w > 361) return fail(MZ_E_INVALID, "board larger than 361 points (19 x 19)");
    // board nets reach 19 x 19 (362 actions: the HBM tree's select covers 384); MLP and Atari nets keep 256
    const int max_actions = cfg->net_kind == MZ_NET_BOARD ? 384 : 256;
    if (cfg->num_actions < 1 || cfg->num_actions > max_actions)
        return fail(MZ_E_INVALID, max_actions == 384 ? "num_actions must be in [1, 384] for board nets" : "num_actions must be in [1, 256]");
    if (cfg->num_simulations < 1 || cfg->num_simulations > 4000) return fail(MZ_E_INVALID, "num_simulations out of range");
    if (conv) {
        if (cfg->obs_c < 1 || cfg->obs_h < 1 || cfg->obs_w < 1 || cfg->num_res_blocks < 0) return fail(MZ_E_INVALID, "bad conv network dimensions");
        if (cfg->net_kind == MZ_NET_ATARI && (cfg->obs_h != 96 || cfg->obs_w != 96))
            return fail(MZ_E_INVALID, "MuZeroAtariNet takes 96x96 frames (its hidden state is fixed at 6x6, network.py:515)");
        if (cfg->num_planes > 512) return fail(MZ_E_INVALID, "conv nets: num_planes must be <= 512");
    }
    if ((!conv && cfg->hidden_dim < 1) || cfg->num_planes < 1 || cfg->num_envs < 1) return fail(MZ_E_INVALID, "bad network/env dimensions");
    if (cfg->value_support_size < 1 || cfg->reward_support_size < 1 || cfg->value_support_size > 1023 || cfg->reward_support_size > 1023)
        return fail(MZ_E_INVALID, "support sizes must be in [1, 1023]");
    if ((cfg->value_support_size > 1 && cfg->value_support_size % 2 == 0) || (cfg->reward_support_size > 1 && cfg->reward_support_size % 2 == 0))
        return fail(MZ_E_INVALID, "support sizes must be odd (or 1): the kernels take the expectation over the support with unit spacing, which linspace(-half, half, size) has at odd sizes only");
    if (cfg->is_board_game && cfg->discount != 1.0) return fail(MZ_E_INVALID, "board games require discount == 1.0 (mcts.py:349-350)");
    if (cfg->conv_precision != MZ_CONV_F32 && cfg->conv_precision != MZ_CONV_BF16X3)
        return fail(MZ_E_INVALID, "conv_precision must be MZ_CONV_F32 (0) or MZ_CONV_BF16X3 (1)");
    if (cfg->conv_precision == MZ_CONV_BF16X3 && cfg->net_kind == MZ_NET_MLP)
        return fail(MZ_E_INVALID, "conv_precision MZ_CONV_BF16X3 needs a conv net: MZ_NET_MLP has no convolutions");
    if (cfg->conv_precision == MZ_CONV_BF16X3 && cfg->net_kind == MZ_NET_ATARI)
        return fail(MZ_E_INVALID, "conv_precision MZ_CONV_BF16X3 is built for MZ_NET_BOARD only: MZ_NET_ATARI's strided stages and 6 x 6 tower have no split build");
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (ndev <= 0) return fail(MZ_E_HIP, "no HIP device visible: the planner has no CPU fallback");
    if (device_id < 0 || device_id >= ndev) return fail(MZ_E_INVALID, "device_id out of range");
    mz_planner* p = new mz_planner();
    p->cfg = *cfg;
    p->device = device_id;
    {   // the per-handle diagnostic switches (mzplanner.h), read here once
        const char* fg = getenv("MZ_FORCE_GENERIC");
        const char* hx = getenv("MZ_HWX");
        const char* to = getenv("MZ_TREE_OLD");
        const char* ht = getenv("MZ_HBM_TREE");
        p->force_generic = fg && fg[0] == '1';
        if (hx) p->hwx = atoi(hx);
        p->tree_old = to && to[0] == '1';
        p->hbm_tree = !conv && ht && ht[0] == '1';  // (MLP nets; planner_init adds the trees that do not fit LDS)
    }
    const int rc = planner_init(p, conv);  // every failure past this point releases what was allocated so far
    if (rc) {
        (void)mz_planner_destroy(p);
        return rc;
    }
    *out = p;
    return MZ_OK;
}

static int planner_init(mz_planner* p, bool conv) {
    const mz_config* cfg = &p->cfg;
    const int device_id = p->device;
    p->conv = conv;
    if (conv) {
        ConvNetDev& n = p->cnet;
        n.kind = cfg->net_kind; n.in_c = cfg->obs_c; n.in_h = cfg->obs_h; n.in_w = cfg->obs_w; n.A = cfg->num_actions;
        n.R = cfg->num_res_blocks; n.P = cfg->num_planes; n.Sv = cfg->value_support_size; n.Sr = cfg->reward_support_size;
        n.split = cfg->conv_precision == MZ_CONV_BF16X3 ? 1 : 0;
        n.hh = conv && cfg->net_kind == MZ_NET_ATARI ? 6 : cfg->obs_h;
        n.hw = conv && cfg->net_kind == MZ_NET_ATARI ? 6 : cfg->obs_w;
        p->cfg.hidden_dim = n.hidden_size();
        compute_layout_conv(p);
    } else {
        compute_layout(p);
    }
    if (!conv) {
        p->hbm_tree = p->hbm_tree || cfg->num_actions > 16 * MAX_CH || (p->sp.lds_bytes > 160 * 1024 && !p->tree2_ok);
        if (p->hbm_tree) {
            if (p->ip.lds_bytes > 160 * 1024) {
                const int need = p->ip.lds_bytes;
                return fail(MZ_E_INVALID, "network needs " + std::to_string(need) + " bytes of LDS per workgroup (> 160 KiB)");
            }
            compute_layout_conv(p, &p->spg);
        }
    }
    HIPCHK(hipSetDevice(device_id));
    HIPCHK(hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking));
    const mz_config& c = p->cfg;
    const size_t B = (size_t)c.num_envs, A = (size_t)c.num_actions, S = (size_t)c.num_simulations;
    const int mt = c.max_ties > 0 ? c.max_ties : 4 * c.num_simulations + 8;
    p->cfg.max_ties = mt;
    HIPCHK(hipMalloc(&p->d_obs, B * obs_dim(c) * sizeof(float) + 256));  // + slack: conv staging reads whole 16-byte pixel quads
    HIPCHK(hipMalloc(&p->d_mask, B * A));
    HIPCHK(hipMalloc(&p->d_cur, B * sizeof(int)));
    HIPCHK(hipMalloc(&p->d_opp, B * sizeof(int)));
    HIPCHK(hipMalloc(&p->d_temp, B * sizeof(double)));
    HIPCHK(hipMalloc(&p->d_noise, B * A * sizeof(double)));
    HIPCHK(hipMalloc(&p->d_utie, B * (size_t)mt * sizeof(double)));
    HIPCHK(hipMalloc(&p->d_ufinal, B * sizeof(double)));
    HIPCHK(hipMalloc(&p->d_hidden, B * (S + 1) * (size_t)c.hidden_dim * sizeof(float) + 256));
    HIPCHK(hipMalloc(&p->d_ftab, (S + 1) * (S + 1) * sizeof(double)));
    HIPCHK(hipMalloc(&p->d_action, B * sizeof(int)));
    HIPCHK(hipMalloc(&p->d_pi, B * A * sizeof(double)));
    HIPCHK(hipMalloc(&p->d_root, B * sizeof(double)));
    HIPCHK(hipMalloc(&p->d_visits, B * A * sizeof(int)));
    HIPCHK(hipMalloc(&p->d_err, sizeof(int)));
    HIPCHK(hipMemset(p->d_err, 0, sizeof(int)));
    HIPCHK(hipMalloc(&p->d_stamps, 16 * sizeof(long long)));
    HIPCHK(hipMemset(p->d_stamps, 0, 16 * sizeof(long long)));
    HIPCHK(hipMemset(p->d_mask, 1, B * A));
    HIPCHK(hipDeviceSynchronize());  // (the fills above run on the NULL stream, which p->stream -- non-blocking -- never waits for)
    // child_U factor table: pb(N) / (n_child + 1) in float64 with the host libm, i.e. the very values math.log /
    // math.sqrt give the reference (mcts.py:193-195)
    std::vector<double> ft((S + 1) * (S + 1));
    for (size_t N = 0; N <= S; N++) {
        const double pb = (std::log(((double)N + c.pb_c_base + 1.0) / c.pb_c_base) + c.pb_c_init) * std::sqrt((double)N);
        for (size_t cn = 0; cn <= S; cn++) ft[N * (S + 1) + cn] = pb / (double)(cn + 1);
    }
    HIPCHK(hipMemcpy(p->d_ftab, ft.data(), ft.size() * sizeof(double), hipMemcpyHostToDevice));
    {
        std::vector<double> tri;
        for (size_t N = 0; N <= S; N++)
            for (size_t cn = 0; cn <= N; cn++) tri.push_back(ft[N * (S + 1) + cn]);
        HIPCHK(hipMalloc(&p->d_ftab_tri, tri.size() * sizeof(double)));
        HIPCHK(hipMemcpy(p->d_ftab_tri, tri.data(), tri.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    HIPCHK(hipEventCreate(&p->ev_begin));
    HIPCHK(hipEventCreate(&p->ev_end));
    if (conv || p->hbm_tree) {
        const size_t blocks = (B + TILE_E - 1) / TILE_E, HS = (size_t)p->cfg.hidden_dim;
        HIPCHK(hipMalloc(&p->d_regions, blocks * (size_t)(conv ? p->sp.lds_bytes : p->spg.lds_bytes)));
        HIPCHK(hipMalloc(&p->d_pi_scratch, B * A * sizeof(float)));
        HIPCHK(hipMalloc(&p->d_pi0, B * A * sizeof(float)));
        HIPCHK(hipMalloc(&p->d_sim_reward, B * sizeof(float)));
        HIPCHK(hipMalloc(&p->d_sim_value, B * sizeof(float)));
        HIPCHK(hipMalloc(&p->d_srcptrs, B * sizeof(float*)));
        HIPCHK(hipMalloc(&p->d_dstptrs, B * sizeof(float*)));
        HIPCHK(hipMalloc(&p->d_rootptrs, B * sizeof(float*)));
        HIPCHK(hipMalloc(&p->d_sim_action, B * sizeof(int)));
        std::vector<float*> roots(B);
        for (size_t i = 0; i < B; i++) roots[i] = p->d_hidden + i * (S + 1) * HS;
        HIPCHK(hipMemcpy(p->d_rootptrs, roots.data(), B * sizeof(float*), hipMemcpyHostToDevice));
        if (conv) {
            return MZ_OK;
        }
    }
    int max_lds = p->tree2_ok ? p->lds_mode2 : (p->tree2f_ok ? p->lds_mode2f : 0);
    if (p->lds_mode0 <= 160 * 1024 && p->lds_mode0 > max_lds) max_lds = p->lds_mode0;
    if (max_lds == 0) max_lds = p->ip.lds_bytes;  // hbm_tree: the LDS-resident search kernels are never launched
    if (p->lds_mode0 > 160 * 1024) p->tree_old = false;  // only the mode-2 layout fits
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_search<false>), hipFuncAttributeMaxDynamicSharedMemorySize, max_lds));
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_search<true>), hipFuncAttributeMaxDynamicSharedMemorySize, max_lds));
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_infer<false>), hipFuncAttributeMaxDynamicSharedMemorySize, p->ip.lds_bytes));
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_infer<true>), hipFuncAttributeMaxDynamicSharedMemorySize, p->ip.lds_bytes));
    if (c.hidden_dim == 64 && (c.num_planes == 256 || c.num_planes == 512) && c.num_actions <= 16 && c.value_support_size <= 32 &&
        c.reward_support_size <= 32 && (c.value_support_size + 15) / 16 == (c.reward_support_size + 15) / 16 &&
        (size_t)c.num_envs * (c.num_simulations + 1) * 256 < ((size_t)1 << 32)) {  // (the tuned kernel addresses the node store with 32-bit byte offsets)
        // the build family (kFastBuilds).  An MSE head's one-neuron layer runs on the vector ALUs in its own summation order (mz_mlp.h,
        // scalar_head_tile): of the tuned builds only the ten-action one has that form
        const int tiles = p->net.L[L_VAL1].n_tiles;
        const bool categorical = c.value_support_size > 1 && c.reward_support_size > 1;
        if (c.num_planes == 256 && c.num_actions == 10 && c.value_support_size == 1 && c.reward_support_size == 1)
            p->fast = FastKey{256, 1, 10, false, false};
        else if (!categorical)
            p->fast_mse = true;
        else if (c.num_actions == 4 && c.num_planes == 512 && tiles == 2)
            p->fast = FastKey{512, 2, 4, false, false};
        else  // (AC = 2: compile-time specialisation for two actions, single player, mz_tree2.h)
            p->fast = FastKey{c.num_planes, tiles, c.num_actions == 2 && !c.is_board_game ? 2 : 0, false, false};
        if (p->fast.planes && !fast_find(p->fast)) p->fast = FastKey{};  // (-DMZ_DEV_SHAPES)
        // the tuned kernel's own carve-out (sp2f): only where the generic one does not fit (the ten-action build is 256 planes wide and
        // always fits the generic one)
        p->fast_layout = !p->tree2_ok && p->tree2f_ok && p->fast.planes && p->fast.ac != 10 && !p->force_generic && !p->tree_old;
        if (p->fast.planes)
            for (const FastBuild& b : kFastBuilds) HIPCHK(hipFuncSetAttribute(b.fn, hipFuncAttributeMaxDynamicSharedMemorySize, max_lds));
    }
    return MZ_OK;
}

static void ext_free(mz_planner* p);
struct ImageGame;
static const ImageGame* image_game(int env_kind);
static int image_game_moves(mz_planner* p, const ImageGame& g, double temperature, int n_moves);
static int image_game_plies(mz_planner* p, const ImageGame& g, int n_plies);

extern "C" int mz_planner_destroy(mz_planner* p) {
    if (!p) return MZ_OK;
    (void)hipSetDevice(p->device);
    if (p->stream) (void)hipStreamSynchronize(p->stream);
    void* bufs[] = {p->d_obs, p->d_mask, p->d_cur, p->d_opp, p->d_temp, p->d_noise, p->d_utie, p->d_ufinal, p->d_hidden, p->d_ftab, p->d_ftab_tri,
                    p->d_action, p->d_pi, p->d_root, p->d_visits, p->d_err, p->d_stamps, p->d_spi0, p->d_svalues, p->d_srewards, p->d_tparent,
                    p->d_taction, p->d_inf_in, p->d_inf_hidden, p->d_inf_reward, p->d_inf_value, p->d_inf_pi, p->d_inf_action};
    for (void* b : bufs)
        if (b) (void)hipFree(b);
    for (int l = 0; l < L_COUNT; l++) {
        if (p->d_w[l]) (void)hipFree(p->d_w[l]);
        if (p->d_b[l]) (void)hipFree(p->d_b[l]);
    }
    if (p->d_stream[0]) (void)hipFree(p->d_stream[0]);
    if (p->d_bias_all) (void)hipFree(p->d_bias_all);
    if (p->d_dbg_noise) { (void)hipFree(p->d_dbg_noise); (void)hipFree(p->d_dbg_utie); (void)hipFree(p->d_dbg_ufinal); }
    if (p->d_epi_ctr) (void)hipFree(p->d_epi_ctr);
    if (p->d_epi_off) (void)hipFree(p->d_epi_off);
    if (p->go.ko) (void)hipFree(p->go.ko);
    if (p->go.passf) (void)hipFree(p->go.passf);
    void* cbufs[] = {p->d_pi_scratch, p->d_regions, p->d_pi0, p->d_sim_reward, p->d_sim_value, (void*)p->d_srcptrs, p->d_dstptrs, p->d_rootptrs, p->d_sim_action};
    for (void* b : cbufs)
        if (b) (void)hipFree(b);
    if (p->pk) {
        p->pk->free_maps();
        if (p->pk->ev_in) (void)hipEventDestroy(p->pk->ev_in);
        if (p->pk->ev_out) (void)hipEventDestroy(p->pk->ev_out);
        delete p->pk;
    }
    convnet_free(p->cnet);
    env_free(p->env);
    arena_free(p->arena);
    if (p->ev_arena_pre) (void)hipEventDestroy(p->ev_arena_pre);
    if (p->ev_arena_q) (void)hipEventDestroy(p->ev_arena_q);
    ext_free(p);
    for (auto& pr : p->kev) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
    if (p->ev_begin) (void)hipEventDestroy(p->ev_begin);
    if (p->ev_end) (void)hipEventDestroy(p->ev_end);
    if (p->stream) (void)hipStreamDestroy(p->stream);
    delete p;
    return MZ_OK;
}

extern "C" int32_t mz_planner_hidden_size(const mz_planner* p) { return p ? p->cfg.hidden_dim : 0; }

extern "C" int mz_planner_set_param(mz_planner* p, const char* name, const float* h_data, const int64_t* shape, int32_t ndim) {
    if (!p || !name || !h_data || !shape || ndim < 1 || ndim > 4) return fail(MZ_E_INVALID, "bad argument to mz_planner_set_param");
    HostTensor t;
    size_t n = 1;
    for (int i = 0; i < ndim; i++) { t.shape.push_back(shape[i]); n *= (size_t)shape[i]; }
    t.data.assign(h_data, h_data + n);
    p->params[name] = std::move(t);
    p->committed = false;
    return MZ_OK;
}

// column of layer l's weight matrix that lane group q supplies for k-step s of block g (-1: padding).  Hidden-type
// blocks: 16g + 4q + s; the dynamics layer's action block(s): action 16(g - hblocks) + 4s + q (mz_mlp.h header).
static int packed_k(const MlpNet& n, int l, int g, int q, int s) {
    const MlpLayer& L = n.L[l];
    if (l == L_DYN0) {
        const int hb = n.h_pad / 16;
        if (g >= hb) {
            const int a = 16 * (g - hb) + 4 * s + q;
            return a < n.A ? n.H + a : -1;
        }
        const int k = 16 * g + 4 * q + s;
        return k < n.H ? k : -1;
    }
    const int k = 16 * g + 4 * q + s;
    return k < L.k ? k : -1;
}

extern "C" int mz_planner_commit_params(mz_planner* p) {
    if (!p) return fail(MZ_E_INVALID, "null planner");
    p->params_touched = true;
    HIPCHK(hipSetDevice(p->device));
    if (p->conv) {
        HIPCHK(hipStreamSynchronize(p->stream));
        ConvNetDev fresh = p->cnet;
        fresh.allocs.clear(); fresh.rep_res.clear(); fresh.dyn_res.clear(); fresh.pred_res.clear();
        fresh.bufA = fresh.bufB = fresh.bufC = nullptr; fresh.buf_elems = 0;
        fresh.tw_rep = fresh.tb_rep = fresh.tw_dyn = fresh.tb_dyn = fresh.tw_pred = fresh.tb_pred = nullptr;
        fresh.dyn_act_w = nullptr; fresh.dyn_inv_hw = 0; fresh.dyn_sp_w = nullptr; fresh.dyn_sp_terms = nullptr;
        convnet_free(p->cnet);
        p->cnet = fresh;
        ParamMap pm;
        for (auto& kv : p->params) pm[kv.first] = HostTensorRef{kv.second.data.data(), kv.second.shape};
        std::string err;
        const int rc = convnet_build(p->cnet, pm, &err);
        if (rc) return fail(rc == -2 ? MZ_E_HIP : (err.rfind("missing", 0) == 0 ? MZ_E_STATE : MZ_E_INVALID), err);
        hipError_t e = convnet_ensure_buffers(p->cnet, p->cfg.num_envs);
        if (e != hipSuccess) return fail(MZ_E_HIP, std::string("conv work buffers: ") + hipGetErrorString(e));
        p->committed = true;
        return MZ_OK;
    }
    for (int l = 0; l < L_COUNT; l++) {
        const MlpLayer& L = p->net.L[l];
        const std::string wn = std::string(kMlpNames[l]) + ".weight", bn = std::string(kMlpNames[l]) + ".bias";
        auto wi = p->params.find(wn), bi = p->params.find(bn);
        if (wi == p->params.end() || bi == p->params.end()) return fail(MZ_E_STATE, "missing parameter " + wn + " / " + bn);
        const HostTensor &W = wi->second, &Bv = bi->second;
        if (W.shape.size() != 2 || W.shape[0] != L.n || W.shape[1] != L.k || Bv.data.size() != (size_t)L.n)
            return fail(MZ_E_INVALID, "shape mismatch for " + wn + ": expected [" + std::to_string(L.n) + ", " + std::to_string(L.k) + "]");
        // A-operand fragment order of v_mfma_f32_16x16x4_f32 in the summation order of mz_mlp.h
        std::vector<float> pw((size_t)L.n_tiles * L.kg * 256, 0.0f), pb((size_t)L.n_tiles * 16, 0.0f);
        for (int t = 0; t < L.n_tiles; t++)
            for (int g = 0; g < L.kg; g++)
                for (int lane = 0; lane < 64; lane++)
                    for (int s = 0; s < 4; s++) {
                        const int nn = 16 * t + (lane & 15), kk = packed_k(p->net, l, g, lane >> 4, s);
                        if (nn < L.n && kk >= 0) pw[(((size_t)t * L.kg + g) * 64 + lane) * 4 + s] = W.data[(size_t)nn * L.k + kk];
                    }
        for (int i = 0; i < L.n; i++) pb[i] = Bv.data[i];
        if (!p->d_w[l]) HIPCHK(hipMalloc(&p->d_w[l], pw.size() * sizeof(float)));
        if (!p->d_b[l]) HIPCHK(hipMalloc(&p->d_b[l], pb.size() * sizeof(float)));
        HIPCHK(hipMemcpy(p->d_w[l], pw.data(), pw.size() * sizeof(float), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(p->d_b[l], pb.data(), pb.size() * sizeof(float), hipMemcpyHostToDevice));
        p->net.L[l].w = p->d_w[l];
        p->net.L[l].b = p->d_b[l];
    }
    {
        // all padded bias vectors in one buffer, laid out like their LDS copies (stage_biases)
        const int base = p->o.BIAS, count = p->o.PM - p->o.BIAS;
        std::vector<float> all((size_t)count, 0.0f);
        for (int l = 0; l < L_COUNT; l++) {
            const HostTensor& Bv = p->params.find(std::string(kMlpNames[l]) + ".bias")->second;
            for (int i = 0; i < p->net.L[l].n; i++) all[p->net.L[l].b_lds - base + i] = Bv.data[i];
        }
        if (!p->d_bias_all) HIPCHK(hipMalloc(&p->d_bias_all, all.size() * sizeof(float)));
        HIPCHK(hipMemcpy(p->d_bias_all, all.data(), all.size() * sizeof(float), hipMemcpyHostToDevice));
        p->net.b_all = p->d_bias_all; p->net.b_base = base; p->net.b_count = count;
    }
    p->sp.net = p->net;
    p->ip.net = p->net;
    if (p->fast.planes) {
        // ONE per-wave weight stream in consumption order (layout: mz_search_fast.h header), for the family's weight ring depth
        const bool sc = kFastSC && p->fast.ac == 10, ax = kFastAX && p->fast.ac == 10;  // (mz_search_fast.h: scalar heads / action column outside the stream)
        const int NT = p->fast.planes / 64, TR = sc ? 0 : p->fast.tiles, TV = TR, RD = fast_rd(p->fast.planes, p->fast.ac);
        const int XG = ax ? 4 : 5;
        const int I_D1 = 0, I_D2 = I_D1 + XG, I_R1 = I_D2 + 4, I_R2 = I_R1 + 4, I_V1 = I_R2 + TR, I_V2 = I_V1 + 4, I_END = I_V2 + TV;
        const int SL = (I_END + RD - 1) / RD * RD;
        const size_t stream_floats = (size_t)WG_WAVES * SL * NT * 256;
        std::vector<float> st(stream_floats + (ax ? (size_t)p->cfg.num_actions * p->fast.planes : 0), 0.0f);
        auto put = [&](int w, int slot, int j, int l, int row_tile, int g) {
            const MlpLayer& L = p->net.L[l];
            const HostTensor& W = p->params.find(std::string(kMlpNames[l]) + ".weight")->second;
            float* d = &st[(((size_t)w * SL + slot) * NT + j) * 256];
            for (int lane = 0; lane < 64; lane++)
                for (int i = 0; i < 4; i++) {
                    const int nn = 16 * row_tile + (lane & 15), kk = packed_k(p->net, l, g, lane >> 4, i);
                    if (nn < L.n && kk >= 0) d[lane * 4 + i] = W.data[(size_t)nn * L.k + kk];
                }
        };
        for (int w = 0; w < WG_WAVES; w++) {
            for (int g = 0; g < XG; g++)
                for (int j = 0; j < NT; j++) put(w, I_D1 + g, j, L_DYN0, NT * w + j, g);
            for (int idx = 0; idx < 4 * NT; idx++) put(w, I_D2 + idx / NT, idx % NT, L_DYN1, idx % 4, NT * w + idx / 4);
            for (int g = 0; g < 4; g++)
                for (int j = 0; j < NT; j++) put(w, I_R1 + g, j, L_REW0, NT * w + j, g);
            for (int idx = 0; idx < TR * NT; idx++) put(w, I_R2 + idx / NT, idx % NT, L_REW1, idx % TR, NT * w + idx / TR);
            for (int g = 0; g < 4; g++)
                for (int j = 0; j < NT; j++) put(w, I_V1 + g, j, L_VAL0, NT * w + j, g);
            for (int idx = 0; idx < TV * NT; idx++) put(w, I_V2 + idx / NT, idx % NT, L_VAL1, idx % TV, NT * w + idx / TV);
        }
        if (ax) {  // the action columns of the dynamics net's first layer, one row per action
            const HostTensor& W = p->params.find(std::string(kMlpNames[L_DYN0]) + ".weight")->second;
            const MlpLayer& L = p->net.L[L_DYN0];
            for (int a = 0; a < p->cfg.num_actions; a++)
                for (int r = 0; r < L.n; r++) st[stream_floats + (size_t)a * p->fast.planes + r] = W.data[(size_t)r * L.k + p->net.H + a];
        }
        if (!p->d_stream[0]) HIPCHK(hipMalloc(&p->d_stream[0], st.size() * sizeof(float)));
        HIPCHK(hipMemcpy(p->d_stream[0], st.data(), st.size() * sizeof(float), hipMemcpyHostToDevice));
        p->fw.stream = reinterpret_cast<const float4*>(p->d_stream[0]);
        p->fw.bytes = (unsigned)(stream_floats * sizeof(float));
        p->fw.wact = ax ? p->d_stream[0] + stream_floats : nullptr;
    }
    p->committed = true;
    return MZ_OK;
}

// ---------------------------------------------------------------------------------------------------------
// weights from device memory (mz_pack.h)
// ---------------------------------------------------------------------------------------------------------
// every packed weight buffer of the handle in a fixed order: what a commit writes, what a refresh rewrites, what mz_debug_read_packed reads
static void packed_buffers(const mz_planner* p, std::vector<PackBufferRef>& out) {
    out.clear();
    if (p->conv) {
        convnet_packed_buffers(p->cnet, out);
        return;
    }
    for (int l = 0; l < L_COUNT; l++) {
        const MlpLayer& L = p->net.L[l];
        if (p->d_w[l]) out.push_back(PackBufferRef{p->d_w[l], (size_t)L.n_tiles * L.kg * 256 * sizeof(float), PACK_F32, std::string(kMlpNames[l]) + ".w"});
        if (p->d_b[l]) out.push_back(PackBufferRef{p->d_b[l], (size_t)L.n_tiles * 16 * sizeof(float), PACK_F32, std::string(kMlpNames[l]) + ".b"});
    }
    if (p->d_bias_all) out.push_back(PackBufferRef{p->d_bias_all, (size_t)(p->o.PM - p->o.BIAS) * sizeof(float), PACK_F32, "bias_all"});
    if (p->d_stream[0]) {
        const bool ax = kFastAX && p->fast.ac == 10;
        out.push_back(PackBufferRef{p->d_stream[0], (size_t)p->fw.bytes + (ax ? (size_t)p->cfg.num_actions * p->fast.planes * sizeof(float) : 0), PACK_F32,
                                    "fast_stream"});
    }
}

extern "C" int mz_planner_bind_param_device(mz_planner* p, const char* name, const float* d_data, const int64_t* shape, int32_t ndim) {
    if (!p || !name || !d_data || !shape || ndim < 1 || ndim > 4) return fail(MZ_E_INVALID, "bad argument to mz_planner_bind_param_device");
    const std::string nm(name), nbt = "num_batches_tracked";
    if (nm.size() >= nbt.size() && nm.compare(nm.size() - nbt.size(), nbt.size(), nbt) == 0)
        return fail(MZ_E_INVALID, nm + ": num_batches_tracked is no float32 tensor and no weight of the planner");
    BoundTensor t;
    t.d = d_data; t.numel = 1;
    for (int i = 0; i < ndim; i++) {
        if (shape[i] < 1) return fail(MZ_E_INVALID, nm + ": empty dimension");
        t.shape.push_back(shape[i]);
        t.numel *= (size_t)shape[i];
    }
    if (t.numel > PACK_MAX_NUMEL) return fail(MZ_E_INVALID, nm + ": more than 2^24 - 2 elements (use mz_planner_set_param)");
    HIPCHK(hipSetDevice(p->device));
    hipPointerAttribute_t at{};
    if (hipPointerGetAttributes(&at, d_data) != hipSuccess) {
        (void)hipGetLastError();
        return fail(MZ_E_INVALID, nm + ": not a device pointer");
    }
    if (at.type != hipMemoryTypeDevice || at.device != p->device)
        return fail(MZ_E_INVALID, nm + ": not device memory of the planner's GPU (device " + std::to_string(p->device) + ")");
    {
        hipDeviceptr_t base = nullptr;
        size_t size = 0;
        if (hipMemGetAddressRange(&base, &size, const_cast<float*>(d_data)) == hipSuccess) {
            const char *lo = static_cast<const char*>(base), *q = reinterpret_cast<const char*>(d_data);
            if (q < lo || q + t.numel * sizeof(float) > lo + size) return fail(MZ_E_INVALID, nm + ": the tensor leaves its device allocation");
        } else {
            (void)hipGetLastError();  // (memory the runtime reports no range for, e.g. mapped virtual ranges: the attributes above stand)
        }
    }
    if ((reinterpret_cast<uintptr_t>(d_data) & 3) != 0) return fail(MZ_E_INVALID, nm + ": misaligned float32 pointer");
    if (!p->pk) p->pk = new PackState();
    PackState& k = *p->pk;
    if (k.table_in_flight) {  // the pinned source table may still be read by an enqueued upload
        HIPCHK(hipStreamSynchronize(p->stream));
        k.table_in_flight = false;
    }
    auto it = k.bound.find(nm);
    if (it == k.bound.end() || it->second.shape != t.shape) k.maps_valid = false;
    k.srcs_dirty = true;
    k.bound[nm] = std::move(t);
    return MZ_OK;
}

// Once per binding: the host commit over probe tensors (mz_pack.h), read back and decoded into the gather maps.  Leaves the packed
// buffers allocated (by that commit, sizes and all) and the handle's kernel parameters pointing at them.
static int pack_build_maps(mz_planner* p) {
    PackState& k = *p->pk;
    HIPCHK(hipStreamSynchronize(p->stream));  // searches in flight read the buffers the probe commits overwrite / reallocate
    k.table_in_flight = false;
    k.free_maps();
    std::vector<PackTensor>& T = k.tensors;
    T.clear();
    for (auto& kv : k.bound) {
        PackTensor t;
        t.name = kv.first; t.shape = kv.second.shape; t.numel = kv.second.numel;
        T.push_back(std::move(t));
    }
    pack_assign_roles(T);
    const float unit_var = pack_unit_var();
    if (unit_var == 0.0f) return fail(MZ_E_INVALID, "device reload: no running_var probes the BatchNorm fold exactly");
    std::map<std::string, HostTensor> saved = std::move(p->params);
    p->params.clear();
    for (const PackTensor& t : T) {
        HostTensor h;
        h.shape = t.shape;
        h.data.resize(t.numel);
        p->params[t.name] = std::move(h);
    }
    std::vector<PackBufferRef> bufs;
    std::vector<std::vector<unsigned char>> img[3];
    int rc = MZ_OK;
    for (int pass = 0; pass < 3 && rc == MZ_OK; pass++) {
        for (size_t i = 0; i < T.size(); i++) pack_probe_values(T[i], (int)i, pass, unit_var, p->params[T[i].name].data.data());
        rc = mz_planner_commit_params(p);  // validates names and shapes exactly as for host tensors
        if (rc) break;
        packed_buffers(p, bufs);
        if (pass == 0) {
            k.buf_bytes.clear(); k.buf_kind.clear();
            for (const PackBufferRef& b : bufs) { k.buf_bytes.push_back(b.bytes); k.buf_kind.push_back(b.kind); }
        } else if (bufs.size() != k.buf_bytes.size()) {
            rc = fail(MZ_E_INVALID, "device reload: the packed buffers changed between two commits");
            break;
        }
        img[pass].resize(bufs.size());
        for (size_t b = 0; b < bufs.size() && rc == MZ_OK; b++) {
            size_t alloc = 0;
            if (bufs[b].bytes != k.buf_bytes[b] || !bufs[b].d || hipMemPtrGetInfo(bufs[b].d, &alloc) != hipSuccess || alloc < bufs[b].bytes) {
                (void)hipGetLastError();
                rc = fail(MZ_E_INVALID, "device reload: " + bufs[b].label + " is not the size the host path allocated");
                break;
            }
            img[pass][b].resize(bufs[b].bytes);
            if (bufs[b].kind != PACK_STATIC && hipMemcpy(img[pass][b].data(), bufs[b].d, bufs[b].bytes, hipMemcpyDeviceToHost) != hipSuccess)
                rc = fail(MZ_E_HIP, "device reload: reading " + bufs[b].label + " back failed");
        }
    }
    p->params = std::move(saved);
    p->committed = false;  // the buffers hold probe values until the refresh that called this has written them
    if (rc) return rc;
    std::vector<PackChunk> cf, cw;
    std::vector<PackEntry> map, ent;
    std::vector<size_t> buf_elems(bufs.size(), 0);
    std::string err;
    for (size_t b = 0; b < bufs.size(); b++) {
        if (bufs[b].kind == PACK_STATIC) continue;
        const bool w3 = bufs[b].kind == PACK_W3;
        if (w3 ? bufs[b].bytes % (1536 * 2) != 0 : bufs[b].bytes % 4 != 0) return fail(MZ_E_INVALID, "device reload: odd size of " + bufs[b].label);
        const size_t n = w3 ? bufs[b].bytes / 2 / 3 : bufs[b].bytes / 4;
        if (n >= ((size_t)1 << 31)) return fail(MZ_E_INVALID, "device reload: " + bufs[b].label + " is too large");
        buf_elems[b] = n;
        ent.resize(n);
        const bool ok = w3 ? pack_decode_w3(reinterpret_cast<const uint16_t*>(img[0][b].data()), reinterpret_cast<const uint16_t*>(img[1][b].data()),
                                            reinterpret_cast<const uint16_t*>(img[2][b].data()), n, T, ent.data(), &err)
                           : pack_decode_f32(reinterpret_cast<const float*>(img[0][b].data()), reinterpret_cast<const float*>(img[1][b].data()),
                                             reinterpret_cast<const float*>(img[2][b].data()), n, T, ent.data(), &err);
        if (!ok) return fail(MZ_E_INVALID, "device reload: cannot derive the layout of " + bufs[b].label + ": " + err);
        pack_make_chunks((int)b, n, w3 ? PACK_CHUNK_W3 : PACK_CHUNK_F32, ent.data(), w3 ? cw : cf, map);
    }
    if (map.size() >= ((size_t)1 << 31)) return fail(MZ_E_INVALID, "device reload: the network is too large");
    if (!pack_check_bounds(cf, map, T, buf_elems, &err) || !pack_check_bounds(cw, map, T, buf_elems, &err)) return fail(MZ_E_INVALID, err);
    for (const PackChunk& c : cw)
        if (c.n % 512 || c.off % 512) return fail(MZ_E_INVALID, "device reload: a split-bf16 chunk is no whole number of term blocks");
    HIPCHK(hipMalloc(&k.d_map, (map.size() + 4) * sizeof(PackEntry)));
    HIPCHK(hipMemcpy(k.d_map, map.data(), map.size() * sizeof(PackEntry), hipMemcpyHostToDevice));
    if (!cf.empty()) {
        HIPCHK(hipMalloc(&k.d_chunks_f32, cf.size() * sizeof(PackChunk)));
        HIPCHK(hipMemcpy(k.d_chunks_f32, cf.data(), cf.size() * sizeof(PackChunk), hipMemcpyHostToDevice));
    }
    if (!cw.empty()) {
        HIPCHK(hipMalloc(&k.d_chunks_w3, cw.size() * sizeof(PackChunk)));
        HIPCHK(hipMemcpy(k.d_chunks_w3, cw.data(), cw.size() * sizeof(PackChunk), hipMemcpyHostToDevice));
    }
    k.n_chunks_f32 = (int)cf.size(); k.n_chunks_w3 = (int)cw.size();
    HIPCHK(hipMalloc(&k.d_srcs, T.size() * sizeof(PackSrc)));
    HIPCHK(hipMalloc(&k.d_dst, bufs.size() * sizeof(void*)));
    HIPCHK(hipHostMalloc(&k.h_srcs, T.size() * sizeof(PackSrc)));
    HIPCHK(hipHostMalloc(&k.h_dst, bufs.size() * sizeof(void*)));
    for (size_t b = 0; b < bufs.size(); b++) k.h_dst[b] = nullptr;
    if (!k.ev_in) HIPCHK(hipEventCreateWithFlags(&k.ev_in, hipEventDisableTiming));
    if (!k.ev_out) HIPCHK(hipEventCreateWithFlags(&k.ev_out, hipEventDisableTiming));
    k.bytes_read = (long long)(map.size() * sizeof(PackEntry));
    k.bytes_written = 0;
    for (const PackEntry& e : map)
        if (e.tid >= 0) k.bytes_read += 4;
    for (size_t b = 0; b < bufs.size(); b++)
        if (bufs[b].kind != PACK_STATIC) k.bytes_written += (long long)bufs[b].bytes;
    k.srcs_dirty = true;
    k.maps_valid = true;
    return MZ_OK;
}

extern "C" int mz_planner_refresh_params(mz_planner* p, void* producer_stream) {
    if (!p) return fail(MZ_E_INVALID, "null planner");
    p->params_touched = true;
    if (!p->pk || p->pk->bound.empty()) return fail(MZ_E_STATE, "no tensor bound: call mz_planner_bind_param_device for every tensor first");
    HIPCHK(hipSetDevice(p->device));
    PackState& k = *p->pk;
    std::vector<PackBufferRef> bufs;
    if (k.maps_valid) {  // a failed host commit may have released the buffers
        packed_buffers(p, bufs);
        if (bufs.size() != k.buf_bytes.size()) k.maps_valid = false;
    }
    if (!k.maps_valid) {
        const int rc = pack_build_maps(p);
        if (rc) return rc;
        packed_buffers(p, bufs);
    }
    for (size_t b = 0; b < bufs.size(); b++)
        if (!bufs[b].d || bufs[b].bytes != k.buf_bytes[b] || bufs[b].kind != k.buf_kind[b])
            return fail(MZ_E_STATE, "device reload: " + bufs[b].label + " changed since the tensors were bound");
    hipStream_t producer = static_cast<hipStream_t>(producer_stream);
    // a host commit of a conv net reallocates (after draining the stream): follow the buffers
    bool moved = false;
    for (size_t b = 0; b < bufs.size(); b++) moved = moved || k.h_dst[b] != bufs[b].d;
    if (moved) {
        for (size_t b = 0; b < bufs.size(); b++) k.h_dst[b] = bufs[b].d;
        HIPCHK(hipMemcpyAsync(k.d_dst, k.h_dst, bufs.size() * sizeof(void*), hipMemcpyHostToDevice, p->stream));
        k.table_in_flight = true;
    }
    if (k.srcs_dirty) {
        const std::vector<PackTensor>& T = k.tensors;
        for (size_t i = 0; i < T.size(); i++) {
            auto ptr = [&](int id) { return id >= 0 ? k.bound.find(T[id].name)->second.d : nullptr; };
            PackSrc s{};
            s.p = ptr((int)i);
            s.kind = T[i].fold_kind < 0 ? 0 : T[i].fold_kind;
            s.inner = 1;
            if (s.kind == 1) {
                const PackTensor& g = T[T[i].fold_gamma];
                s.gamma = ptr(g.gamma); s.mean = ptr(g.mean); s.var = ptr(g.var);
                s.inner = (int)(T[i].numel / (size_t)T[i].shape[0]);
            } else if (s.kind == 2) {
                s.gamma = ptr(T[i].gamma); s.mean = ptr(T[i].mean); s.var = ptr(T[i].var);
            }
            k.h_srcs[i] = s;
        }
        HIPCHK(hipMemcpyAsync(k.d_srcs, k.h_srcs, T.size() * sizeof(PackSrc), hipMemcpyHostToDevice, p->stream));
        k.table_in_flight = true;
        k.srcs_dirty = false;
    }
    // the producer's writes before this call -> the pack kernels -> the producer's next writes; searches already enqueued on the planner's
    // stream finish on the old weights by stream order.  No host synchronisation.
    HIPCHK(hipEventRecord(k.ev_in, producer));
    HIPCHK(hipStreamWaitEvent(p->stream, k.ev_in, 0));
    if (k.n_chunks_f32) hipLaunchKernelGGL(k_pack_f32, dim3(k.n_chunks_f32), dim3(256), 0, p->stream, k.d_chunks_f32, k.d_map, k.d_srcs, k.d_dst);
    if (k.n_chunks_w3) hipLaunchKernelGGL(k_pack_w3, dim3(k.n_chunks_w3), dim3(256), 0, p->stream, k.d_chunks_w3, k.d_map, k.d_srcs, k.d_dst);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(k.ev_out, p->stream));
    HIPCHK(hipStreamWaitEvent(producer, k.ev_out, 0));
    p->committed = true;
    return MZ_OK;
}

// test hooks, not part of the ABI header.  mz_debug_read_packed: packed weight buffer `index` of the handle (per-layer weights and biases,
// bias block, fast stream; conv w / b / w3, tails, heads, tower tables), copied to h_out (NULL: only its size and name); MZ_E_INVALID past
// the last buffer.  mz_debug_packed_info: [0] the buffer's device address, [1] pack kernels per refresh, [2] bytes a refresh reads
// (entries + sources), [3] bytes it writes.
extern "C" int mz_debug_read_packed(mz_planner* p, int32_t index, void* h_out, int64_t* bytes, const char** label) {
    if (!p) return fail(MZ_E_INVALID, "null planner");
    static thread_local std::string g_label;
    std::vector<PackBufferRef> bufs;
    packed_buffers(p, bufs);
    if (index < 0 || (size_t)index >= bufs.size()) return fail(MZ_E_INVALID, "no packed buffer " + std::to_string(index));
    if (bytes) *bytes = (int64_t)bufs[index].bytes;
    g_label = bufs[index].label;
    if (label) *label = g_label.c_str();
    if (h_out) {
        HIPCHK(hipSetDevice(p->device));
        HIPCHK(hipStreamSynchronize(p->stream));
        HIPCHK(hipMemcpy(h_out, bufs[index].d, bufs[index].bytes, hipMemcpyDeviceToHost));
    }
    return MZ_OK;
}

extern "C" int mz_debug_packed_info(mz_planner* p, int32_t index, int64_t out[4]) {
    if (!p || !out) return fail(MZ_E_INVALID, "null argument");
    std::vector<PackBufferRef> bufs;
    packed_buffers(p, bufs);
    if (index < 0 || (size_t)index >= bufs.size()) return fail(MZ_E_INVALID, "no packed buffer " + std::to_string(index));
    out[0] = (int64_t)reinterpret_cast<uintptr_t>(bufs[index].d);
    const PackState* k = p->pk;
    out[1] = k ? (k->n_chunks_f32 > 0) + (k->n_chunks_w3 > 0) : 0;
    out[2] = k ? k->bytes_read : 0;
    out[3] = k ? k->bytes_written : 0;
    return MZ_OK;
}

// mz_debug_conv3x3: ONE 3x3 stride-1 conv layer through the production code -- build_conv (no BatchNorm: the commit's f32 and w3 packers on
// h_weight [cout][cin][3][3]) in a temporary ConvNetDev whose `split` is the handle's conv_precision, h_bias (NULL: zeros) over the layer's
// bias buffer, conv_run on the handle's stream: the build split_geometry / conv_geometry pick for the planner.  h_in [batch][cin_real][h][w];
// h_rows: image b is row h_rows[b] of h_in, launched through per-image pointers (the search's node-store gather); h_action: channels
// cin_real .. cin - 1 are the action planes of a num_actions-action net; h_residual / h_out [batch][cout][h][w].  *build_name: the build that
// ran.  Everything lives in allocations of this call: the handle's weights and buffers are not touched.
extern "C" int mz_debug_conv3x3(mz_planner* p, int32_t batch, int32_t cin_real, int32_t cin, int32_t cout, int32_t h, int32_t w, const float* h_weight,
                                const float* h_bias, const float* h_in, const int32_t* h_rows, const int32_t* h_action, int32_t num_actions,
                                const float* h_residual, int32_t relu, float* h_out, const char** build_name) {
    if (!p || !h_weight || !h_in || !h_out) return fail(MZ_E_INVALID, "null argument to mz_debug_conv3x3");
    if (!p->conv) return fail(MZ_E_INVALID, "mz_debug_conv3x3 needs a conv net: MZ_NET_MLP has no convolutions");
    if (batch < 1 || batch > 4096) return fail(MZ_E_INVALID, "mz_debug_conv3x3: batch must be in [1, 4096]");
    if (cin_real < 1 || cin_real > cin || cin > 1024 || cout < 1 || cout > 512) return fail(MZ_E_INVALID, "mz_debug_conv3x3: 1 <= cin_real <= cin <= 1024, 1 <= cout <= 512");
    if (h < 3 || h > 19 || w < 3 || w > 19) return fail(MZ_E_INVALID, "mz_debug_conv3x3: h and w must be in [3, 19]");
    if (h_action ? num_actions < 1 : cin != cin_real) return fail(MZ_E_INVALID, "mz_debug_conv3x3: channels past cin_real need h_action and num_actions >= 1");
    for (int b = 0; b < batch; b++) {
        if (h_rows && (h_rows[b] < 0 || h_rows[b] >= batch)) return fail(MZ_E_INVALID, "mz_debug_conv3x3: h_rows out of range");
        if (h_action && (h_action[b] < 0 || h_action[b] >= num_actions)) return fail(MZ_E_INVALID, "mz_debug_conv3x3: h_action out of range");
    }
    HIPCHK(hipSetDevice(p->device));
    struct Scratch {  // every device allocation of the call, the layer's included
        ConvNetDev n;
        ~Scratch() {
            for (void* b : n.allocs) (void)hipFree(b);
        }
        hipError_t alloc(void** d, size_t bytes) {
            hipError_t e = hipMalloc(d, bytes + 256);  // + slack: the f32 kernels read the last pixel quad of a channel as 16 bytes
            if (e != hipSuccess) return e;
            n.allocs.push_back(*d);
            return hipMemset(*d, 0, bytes + 256);
        }
    } s;
    s.n.kind = MZ_NET_BOARD;
    s.n.split = p->cnet.split;
    ParamMap pm;
    pm["w"] = HostTensorRef{h_weight, {cout, cin, 3, 3}};
    ConvLayerDev layer;
    std::string err;
    const int rc = build_conv(s.n, pm, "w", "", cin, cin_real, cout, 3, 1, &layer, &err);
    if (rc) return fail(rc == -2 ? MZ_E_HIP : MZ_E_INVALID, "mz_debug_conv3x3: " + err);
    const size_t hw = (size_t)h * w, in_floats = (size_t)batch * cin_real * hw, out_floats = (size_t)batch * cout * hw;
    float *d_in = nullptr, *d_res = nullptr, *d_out = nullptr;
    const float** d_ptrs = nullptr;
    int* d_act = nullptr;
    HIPCHK(s.alloc(reinterpret_cast<void**>(&d_in), in_floats * sizeof(float)));
    HIPCHK(s.alloc(reinterpret_cast<void**>(&d_out), out_floats * sizeof(float)));
    HIPCHK(hipDeviceSynchronize());  // (the memsets above run on the null stream)
    if (h_bias) HIPCHK(hipMemcpyAsync(layer.b, h_bias, (size_t)cout * sizeof(float), hipMemcpyHostToDevice, p->stream));
    HIPCHK(hipMemcpyAsync(d_in, h_in, in_floats * sizeof(float), hipMemcpyHostToDevice, p->stream));
    std::vector<const float*> ptrs;  // (alive until the stream is drained)
    if (h_rows) {
        for (int b = 0; b < batch; b++) ptrs.push_back(d_in + (size_t)h_rows[b] * cin_real * hw);
        HIPCHK(s.alloc(reinterpret_cast<void**>(&d_ptrs), (size_t)batch * sizeof(float*)));
        HIPCHK(hipDeviceSynchronize());
        HIPCHK(hipMemcpyAsync(d_ptrs, ptrs.data(), (size_t)batch * sizeof(float*), hipMemcpyHostToDevice, p->stream));
    }
    if (h_action) {
        HIPCHK(s.alloc(reinterpret_cast<void**>(&d_act), (size_t)batch * sizeof(int)));
        HIPCHK(hipDeviceSynchronize());
        HIPCHK(hipMemcpyAsync(d_act, h_action, (size_t)batch * sizeof(int), hipMemcpyHostToDevice, p->stream));
    }
    if (h_residual) {
        HIPCHK(s.alloc(reinterpret_cast<void**>(&d_res), out_floats * sizeof(float)));
        HIPCHK(hipDeviceSynchronize());  // (alloc's memset runs on the null stream, which the planner's non-blocking stream does not wait for: unsynchronised it can
                                         // land after the copy below and zero the head of a large residual)
        HIPCHK(hipMemcpyAsync(d_res, h_residual, out_floats * sizeof(float), hipMemcpyHostToDevice, p->stream));
    }
    static thread_local std::string g_build;
    if (layer.w3) {
        g_build = split_geometry(h, w, cout).name;
    } else {
        const ConvGeom g = conv_geometry(batch, h, w, 1, cout, true);
        g_build = "k_conv3x3 f32: " + std::to_string(g.th) + " x " + std::to_string(g.tw) + " tiles, G=" + std::to_string(g.G) + ", NPT=" + std::to_string(g.npt) +
                  ", NCT=" + std::to_string(g.nct) + (g.whole ? " (whole image)" : " (tiled)");
    }
    if (build_name) *build_name = g_build.c_str();
    conv_run(p->stream, layer, batch, h_rows ? nullptr : d_in, d_ptrs, d_act, h_action ? num_actions : 0, h, w, d_res, d_out, relu != 0, d_in, in_floats);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h_out, d_out, out_floats * sizeof(float), hipMemcpyDeviceToHost, p->stream));
    HIPCHK(hipStreamSynchronize(p->stream));
    return MZ_OK;
}

// mz_debug_res_tower: ONE residual tower of n_convs = 2 * blocks convs through the production code -- build_conv per layer (no BatchNorm) in
// a temporary ConvNetDev in the handle's precision (split where conv_precision or tower_precision is bf16x3), the tower tables, tower_run on
// the handle's stream.  h_weight [n_convs][P][P][3][3], h_bias [n_convs][P], h_in / h_out [batch][P][h][w].  *build_name: the build that ran,
// with G and NPT; *tower_ms (may be NULL): the tower's launches between two HIP events on the handle's stream.  Everything lives in allocations of this call: the handle's weights and buffers are not touched.
extern "C" int mz_debug_res_tower(mz_planner* p, int32_t batch, int32_t planes, int32_t h, int32_t w, int32_t n_convs, const float* h_weight,
                                  const float* h_bias, const float* h_in, float* h_out, const char** build_name, float* tower_ms) {
    if (!p || !h_weight || !h_bias || !h_in || !h_out) return fail(MZ_E_INVALID, "null argument to mz_debug_res_tower");
    if (!p->conv) return fail(MZ_E_INVALID, "mz_debug_res_tower needs a conv net: MZ_NET_MLP has no residual towers");
    if (batch < 1 || batch > 4096) return fail(MZ_E_INVALID, "mz_debug_res_tower: batch must be in [1, 4096]");
    if (planes < 1 || planes > 512) return fail(MZ_E_INVALID, "mz_debug_res_tower: planes must be in [1, 512]");
    if (h < 3 || h > 19 || w < 3 || w > 19) return fail(MZ_E_INVALID, "mz_debug_res_tower: h and w must be in [3, 19]");
    if (n_convs < 2 || n_convs > 64 || (n_convs & 1)) return fail(MZ_E_INVALID, "mz_debug_res_tower: n_convs must be even and in [2, 64]");
    HIPCHK(hipSetDevice(p->device));
    struct Scratch {
        ConvNetDev n;
        ~Scratch() {
            for (void* b : n.allocs) (void)hipFree(b);
        }
        hipError_t alloc(void** d, size_t bytes) {
            hipError_t e = hipMalloc(d, bytes + 256);  // + slack: the f32 kernels read the last pixel quad of a channel as 16 bytes
            if (e != hipSuccess) return e;
            n.allocs.push_back(*d);
            return hipMemset(*d, 0, bytes + 256);
        }
    } s;
    const bool split = p->cnet.split || p->cnet.tower_split;
    s.n.kind = MZ_NET_BOARD;
    s.n.split = split ? 1 : 0;
    s.n.P = planes;
    std::vector<ResBlockDev> blocks(n_convs / 2);
    const size_t wn = (size_t)planes * planes * 9;
    std::string err;
    for (int i = 0; i < n_convs; i++) {
        ParamMap pm;
        pm["w"] = HostTensorRef{h_weight + (size_t)i * wn, {planes, planes, 3, 3}};
        ConvLayerDev* layer = (i & 1) ? &blocks[i / 2].c2 : &blocks[i / 2].c1;
        const int rc = build_conv(s.n, pm, "w", "", planes, planes, planes, 3, 1, layer, &err);
        if (rc) return fail(rc == -2 ? MZ_E_HIP : MZ_E_INVALID, "mz_debug_res_tower: " + err);
        HIPCHK(hipMemcpy(layer->b, h_bias + (size_t)i * planes, (size_t)planes * sizeof(float), hipMemcpyHostToDevice));
    }
    const void* const* ts = nullptr;
    float *tw = nullptr, *tb = nullptr;
    if (split) {
        if (split_tower_table(s.n, blocks, &ts)) return fail(MZ_E_HIP, "mz_debug_res_tower: hipMalloc/hipMemcpy failed");
    } else if (planes <= 128 && (planes & 15) == 0) {  // the float32 tower's back-to-back tables, as convnet_build lays them out
        const size_t pw = (size_t)(planes / 16) * (planes / 16) * 9 * 256;
        HIPCHK(s.alloc(reinterpret_cast<void**>(&tw), n_convs * pw * sizeof(float)));
        HIPCHK(s.alloc(reinterpret_cast<void**>(&tb), (size_t)n_convs * planes * sizeof(float)));
        HIPCHK(hipDeviceSynchronize());
        for (int i = 0; i < n_convs; i++) {
            const ConvLayerDev& c = (i & 1) ? blocks[i / 2].c2 : blocks[i / 2].c1;
            HIPCHK(hipMemcpy(tw + i * pw, c.w, pw * sizeof(float), hipMemcpyDeviceToDevice));
            HIPCHK(hipMemcpy(tb + (size_t)i * planes, c.b, (size_t)planes * sizeof(float), hipMemcpyDeviceToDevice));
        }
    }
    const size_t floats = (size_t)batch * planes * h * w;
    float* d[3] = {nullptr, nullptr, nullptr};
    for (int i = 0; i < 3; i++) HIPCHK(s.alloc(reinterpret_cast<void**>(&d[i]), floats * sizeof(float)));
    HIPCHK(hipDeviceSynchronize());  // (the memsets above run on the null stream)
    HIPCHK(hipMemcpyAsync(d[0], h_in, floats * sizeof(float), hipMemcpyHostToDevice, p->stream));
    static thread_local std::string g_build;
    const TowerGeom gs = ts ? split_tower_geometry(batch, planes, h, w) : TowerGeom{0, 0, 0, 0};
    const TowerGeom gf = (tw && tb) ? tower_geometry(batch, planes, h, w) : TowerGeom{0, 0, 0, 0};
    if (gs.npt) g_build = split_tower_name(gs);
    else if (split) g_build = std::string("per conv: ") + split_geometry(h, w, planes).name;
    else if (gf.npt) g_build = "k_res_tower<NPT=" + std::to_string(gf.npt) + ">, G=" + std::to_string(gf.G);
    else g_build = "per conv: k_conv3x3 f32";
    if (build_name) *build_name = g_build.c_str();
    hipEvent_t ev[2] = {nullptr, nullptr};
    if (tower_ms) {
        HIPCHK(hipEventCreate(&ev[0]));
        HIPCHK(hipEventCreate(&ev[1]));
        HIPCHK(hipEventRecord(ev[0], p->stream));
    }
    const float* out = tower_run(p->stream, blocks, 0, n_convs / 2, batch, d[0], d[1], d[2], h, w, tw, tb, ts);
    if (tower_ms) HIPCHK(hipEventRecord(ev[1], p->stream));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h_out, out, floats * sizeof(float), hipMemcpyDeviceToHost, p->stream));
    HIPCHK(hipStreamSynchronize(p->stream));
    if (tower_ms) {
        HIPCHK(hipEventElapsedTime(tower_ms, ev[0], ev[1]));
        (void)hipEventDestroy(ev[0]);
        (void)hipEventDestroy(ev[1]);
    }
    return MZ_OK;
}

// ---------------------------------------------------------------------------------------------------------
// inference API
// ---------------------------------------------------------------------------------------------------------
static int ensure_infer_buffers(mz_planner* p, int batch) {
    if (batch <= p->inf_cap) return MZ_OK;
    void* old[] = {p->d_inf_in, p->d_inf_hidden, p->d_inf_reward, p->d_inf_value, p->d_inf_pi, p->d_inf_action};
    for (void* b : old)
        if (b) (void)hipFree(b);
    const size_t B = (size_t)batch;
    const size_t in = (size_t)(obs_dim(p->cfg) > p->cfg.hidden_dim ? obs_dim(p->cfg) : p->cfg.hidden_dim);
    HIPCHK(hipMalloc(&p->d_inf_in, B * in * sizeof(float) + 256));
    HIPCHK(hipMalloc(&p->d_inf_hidden, B * p->cfg.hidden_dim * sizeof(float)));
    HIPCHK(hipMalloc(&p->d_inf_reward, B * sizeof(float)));
    HIPCHK(hipMalloc(&p->d_inf_value, B * sizeof(float)));
    HIPCHK(hipMalloc(&p->d_inf_pi, B * p->cfg.num_actions * sizeof(float)));
    HIPCHK(hipMalloc(&p->d_inf_action, B * sizeof(int)));
    p->inf_cap = batch;
    return MZ_OK;
}

static int run_infer(mz_planner* p, bool initial, int batch, const float* h_in, const int32_t* h_action, float* h_hidden, float* h_reward,
                     float* h_pi, float* h_value) {
    if (!p || batch < 1 || !h_in) return fail(MZ_E_INVALID, "bad argument to inference call");
    if (!p->committed) return fail(MZ_E_STATE, "weights not committed: call mz_planner_set_param for every tensor, then mz_planner_commit_params");
    HIPCHK(hipSetDevice(p->device));
    int rc = ensure_infer_buffers(p, batch);
    if (rc) return rc;
    const size_t in_w = initial ? obs_dim(p->cfg) : p->cfg.hidden_dim;
    HIPCHK(hipMemcpyAsync(p->d_inf_in, h_in, (size_t)batch * in_w * sizeof(float), hipMemcpyHostToDevice, p->stream));
    if (!initial) HIPCHK(hipMemcpyAsync(p->d_inf_action, h_action, (size_t)batch * sizeof(int), hipMemcpyHostToDevice, p->stream));
    if (p->conv) {
        hipError_t e = convnet_ensure_buffers(p->cnet, batch);
        if (e != hipSuccess) return fail(MZ_E_HIP, std::string("conv work buffers: ") + hipGetErrorString(e));
        if (initial) convnet_initial(p->stream, p->cnet, batch, p->d_inf_in, nullptr, p->d_inf_hidden, p->d_inf_pi, p->d_inf_value);
        else convnet_recurrent(p->stream, p->cnet, batch, nullptr, p->d_inf_in, p->d_inf_action, nullptr, p->d_inf_hidden, p->d_inf_reward,
                               p->d_inf_value, p->d_inf_pi);
        HIPCHK(hipGetLastError());
    } else {
    InferParams ip = p->ip;
    ip.B = batch; ip.in = p->d_inf_in; ip.in_ptrs = nullptr; ip.out_ptrs = nullptr; ip.action = p->d_inf_action; ip.hidden_out = p->d_inf_hidden; ip.reward = p->d_inf_reward;
    ip.value = p->d_inf_value; ip.pi = p->d_inf_pi;
    const dim3 grid((batch + TILE_E - 1) / TILE_E), block(WG_THREADS);
    if (initial) hipLaunchKernelGGL(k_infer<true>, grid, block, ip.lds_bytes, p->stream, ip);
    else hipLaunchKernelGGL(k_infer<false>, grid, block, ip.lds_bytes, p->stream, ip);
    HIPCHK(hipGetLastError());
    }
    if (h_hidden) HIPCHK(hipMemcpyAsync(h_hidden, p->d_inf_hidden, (size_t)batch * p->cfg.hidden_dim * sizeof(float), hipMemcpyDeviceToHost, p->stream));
    if (h_reward) HIPCHK(hipMemcpyAsync(h_reward, p->d_inf_reward, (size_t)batch * sizeof(float), hipMemcpyDeviceToHost, p->stream));
    if (h_value) HIPCHK(hipMemcpyAsync(h_value, p->d_inf_value, (size_t)batch * sizeof(float), hipMemcpyDeviceToHost, p->stream));
    if (h_pi) HIPCHK(hipMemcpyAsync(h_pi, p->d_inf_pi, (size_t)batch * p->cfg.num_actions * sizeof(float), hipMemcpyDeviceToHost, p->stream));
    HIPCHK(hipStreamSynchronize(p->stream));
    return MZ_OK;
}

extern "C" int mz_planner_initial_inference(mz_planner* p, int32_t batch, const float* h_obs, float* h_hidden, float* h_pi, float* h_value) {
    return run_infer(p, true, batch, h_obs, nullptr, h_hidden, nullptr, h_pi, h_value);
}

extern "C" int mz_planner_recurrent_inference(mz_planner* p, int32_t batch, const float* h_hidden, const int32_t* h_action, float* h_hidden_out,
                                              float* h_reward, float* h_pi, float* h_value) {
    if (!h_action) return fail(MZ_E_INVALID, "null action");
    return run_infer(p, false, batch, h_hidden, h_action, h_hidden_out, h_reward, h_pi, h_value);
}

// ---------------------------------------------------------------------------------------------------------
// search
// ---------------------------------------------------------------------------------------------------------
static int next_kernel_events(mz_planner* p, hipEvent_t* a, hipEvent_t* b) {
    if (p->kev_used == p->kev.size()) {
        hipEvent_t x, y;
        HIPCHK(hipEventCreate(&x));
        HIPCHK(hipEventCreate(&y));
        p->kev.emplace_back(x, y);
    }
    *a = p->kev[p->kev_used].first;
    *b = p->kev[p->kev_used].second;
    p->kev_used++;
    return MZ_OK;
}

// the SearchParams fields the LDS-tree kernels and the HBM-tree sequence share, over a tree layout: the search configuration, this
// call's modes and the planner's buffers.  The one place a search advances move_counter (the key of its Philox draws).
static SearchParams search_params(mz_planner* p, const SearchParams& layout, int batch, int deterministic, bool has_mask, bool injected_rng) {
    const mz_config& c = p->cfg;
    SearchParams s = layout;
    s.discount = c.discount; s.board = c.is_board_game; s.has_bounds = c.has_known_bounds;
    s.kb_min = c.known_bounds_min; s.kb_max = c.known_bounds_max; s.alpha = c.root_dirichlet_alpha; s.eps = c.root_exploration_eps;
    s.deterministic = deterministic; s.has_mask = has_mask ? 1 : 0;
    const bool want_noise = !deterministic && c.root_dirichlet_alpha > 0.0 && c.root_exploration_eps > 0.0;  // mcts.py:361
    s.noise_mode = want_noise ? (injected_rng ? 1 : 2) : 0; s.legacy_promo = c.legacy_scalar_promotion ? 1 : 0;
    s.rng_mode = injected_rng ? 0 : 1;
    s.max_ties = c.max_ties;
    s.B = batch;
    s.obs = p->d_obs; s.mask = p->d_mask; s.cur = p->d_cur; s.opp = p->d_opp; s.temperature = p->d_temp;
    s.noise = p->d_noise; s.u_tie = p->d_utie; s.u_final = p->d_ufinal; s.hidden = p->d_hidden; s.ftab = p->d_ftab;
    s.out_action = p->d_action; s.out_pi = p->d_pi; s.out_root = p->d_root; s.out_visits = p->d_visits; s.err = p->d_err;
    s.seed = c.seed; s.move_counter = p->move_counter++; s.env_offset = 0;
    s.dbg_noise = p->d_dbg_noise; s.dbg_utie = p->d_dbg_utie; s.dbg_ufinal = p->d_dbg_ufinal;
    return s;
}

// MLP nets whose trees fit LDS: one fused kernel per search (with fenv: per self-play move)
static int launch_lds_search(mz_planner* p, int batch, int deterministic, bool has_mask, bool injected_rng, bool scripted, const EnvLaunch* fenv) {
    const mz_config& c = p->cfg;
    const bool fastlayout = p->fast_layout && !scripted;
    const bool mode2 = (p->tree2_ok && !p->tree_old) || fastlayout;
    SearchParams s = search_params(p, fastlayout ? p->sp2f : (mode2 ? p->sp2 : p->sp), batch, deterministic, has_mask, injected_rng);
    s.tree_mode = mode2 ? 2 : 0;
    s.net = p->net;
    if (fastlayout) {  // the bias block sits `fast_delta` floats lower in this carve-out
        s.net.b_base -= p->fast_delta;
        for (int l = 0; l < L_COUNT; l++) s.net.L[l].b_lds -= p->fast_delta;
    }
    s.ftab_tri = p->d_ftab_tri;
    s.s_pi0 = p->d_spi0; s.s_values = p->d_svalues; s.s_rewards = p->d_srewards; s.trace_parent = p->d_tparent; s.trace_action = p->d_taction;
    s.stamps = p->d_stamps;
    s.fuse_env = fenv ? 1 : 0;
    // both jobs where both heads are categorical (classic control: -3.8 % on C2, same box); the normalisation alone for the MSE heads of
    // the board games, which have no softmax row (C3: -1.2 %)
    s.hwx = p->hwx >= 0 ? p->hwx : ((c.reward_support_size > 1 && c.value_support_size > 1) ? 3 : 1);
    if (fenv) s.fenv = *fenv;
    const dim3 grid((batch + TILE_E - 1) / TILE_E), block(WG_THREADS);
    if (scripted) {
        p->last_dispatch = "k_search<SCRIPTED=true> (scripted-network test hook)";
        hipLaunchKernelGGL(k_search<true>, grid, block, s.lds_bytes, p->stream, s);
    } else if (p->fast.planes && !p->force_generic && s.tree_mode == 2) {  // (k_search_fast is written for the tree_mode 2 layout)
        FastKey k = p->fast;
        k.fuse = fenv != nullptr;
        // SPB: the build with the board games' self-play settings as compile-time constants (mz_search_fast.h)
        k.spb = k.ac == 10 && s.board && s.has_bounds && s.discount == 1.0 && s.noise_mode == 2 && s.rng_mode == 1 && !s.deterministic && s.has_mask;
        const FastBuild* b = fast_find(k);
        p->last_dispatch = fast_name(k, fastlayout);
        if (!b) return fail(MZ_E_STATE, "not compiled: " + p->last_dispatch);
        void* args[] = {&s, &p->fw};
        HIPCHK(hipLaunchKernel(b->fn, grid, dim3(kFastHW ? 2 * WG_THREADS : WG_THREADS), args, s.lds_bytes, p->stream));
    } else {
        p->last_dispatch = p->force_generic ? "k_search<false> (shape-generic, forced by MZ_FORCE_GENERIC=1)"
                           : p->fast_mse && s.tree_mode == 2 ? "k_search<false> (shape-generic; MSE head outside the ten-action build)"
                                                              : "k_search<false> (shape-generic: no tuned build for this shape)";
        hipLaunchKernelGGL(k_search<false>, grid, block, s.lds_bytes, p->stream, s);
    }
    return MZ_OK;
}

// conv nets, and MLP nets whose trees do not fit LDS: HBM-resident trees, root inference -> init -> S x {select, network evaluation,
// expand + backup} -> play
static int launch_hbm_search(mz_planner* p, int batch, int deterministic, bool has_mask, bool injected_rng, bool scripted) {
    const mz_config& c = p->cfg;
    const bool mlp = !p->conv;
    p->last_dispatch = std::string(mlp ? "k_infer" : "conv towers (mz_convnet.h: k_conv3x3 / k_res_tower / k_head)") +
                       " around HBM trees: k_gtree_select_wave + k_gtree_backup per simulation";
    SearchParams s = search_params(p, mlp ? p->spg : p->sp, batch, deterministic, has_mask, injected_rng);
    s.trace_parent = scripted ? p->d_tparent : nullptr; s.trace_action = scripted ? p->d_taction : nullptr;
    const dim3 grid((batch + TILE_E - 1) / TILE_E), block(WG_THREADS);
    InferParams ip = p->ip;
    ip.net = p->net; ip.B = batch; ip.in = nullptr; ip.in_ptrs = nullptr; ip.action = p->d_sim_action; ip.hidden_out = nullptr;
    ip.out_ptrs = nullptr; ip.reward = p->d_sim_reward; ip.value = p->d_sim_value; ip.pi = p->d_pi_scratch;
    GTreeLaunch G{};
    G.P = s; G.regions = p->d_regions; G.hidden_size = c.hidden_dim; G.src_ptrs = p->d_srcptrs; G.dst_ptrs = p->d_dstptrs;
    G.actions = p->d_sim_action;
    if (scripted) {
        G.pi0 = p->d_spi0;
    } else if (mlp) {
        InferParams r = ip;
        r.in = p->d_obs; r.out_ptrs = p->d_rootptrs; r.pi = p->d_pi0;
        hipLaunchKernelGGL(k_infer<true>, grid, block, r.lds_bytes, p->stream, r);  // root value discarded (mcts.py:356-367)
        G.pi0 = p->d_pi0;
    } else {
        convnet_initial(p->stream, p->cnet, batch, p->d_obs, p->d_rootptrs, nullptr, p->d_pi0, p->d_sim_value);  // root value discarded
        G.pi0 = p->d_pi0;
    }
    const bool any_n = c.num_actions > 248;  // (np_sum_f64 / _f32 are numpy's sums up to 248 actions: mz_device.h)
    if (any_n) hipLaunchKernelGGL(k_gtree_init<true>, grid, block, 0, p->stream, G);
    else hipLaunchKernelGGL(k_gtree_init<false>, grid, block, 0, p->stream, G);
    for (int sim = 0; sim < c.num_simulations; sim++) {
        G.sim = sim;
        // one wave per env (k_gtree_select_wave); more than 256 actions: the wider build, 6 chunks of 64 lanes (the same arithmetic and tie order)
        if (c.num_actions > 64 * MAX_CH64) hipLaunchKernelGGL(k_gtree_select_wave<MAX_CH64_WIDE>, dim3((batch + 3) / 4), block, 0, p->stream, G);
        else hipLaunchKernelGGL(k_gtree_select_wave<MAX_CH64>, dim3((batch + 3) / 4), block, 0, p->stream, G);
        if (scripted) {
            G.reward = p->d_srewards + sim; G.value = p->d_svalues + sim; G.rv_stride = c.num_simulations;
        } else if (mlp) {
            InferParams r = ip;
            r.in_ptrs = p->d_srcptrs; r.out_ptrs = p->d_dstptrs;
            hipLaunchKernelGGL(k_infer<false>, grid, block, r.lds_bytes, p->stream, r);
            G.reward = p->d_sim_reward; G.value = p->d_sim_value; G.rv_stride = 1;
        } else {
            convnet_recurrent(p->stream, p->cnet, batch, p->d_srcptrs, nullptr, p->d_sim_action, p->d_dstptrs, nullptr, p->d_sim_reward,
                              p->d_sim_value, nullptr, p->d_hidden, (size_t)c.num_envs * (c.num_simulations + 1) * (size_t)c.hidden_dim);
            G.reward = p->d_sim_reward; G.value = p->d_sim_value; G.rv_stride = 1;
        }
        hipLaunchKernelGGL(k_gtree_backup, grid, block, 0, p->stream, G);
    }
    if (any_n) hipLaunchKernelGGL(k_gtree_finish<true>, grid, block, 0, p->stream, G);
    else hipLaunchKernelGGL(k_gtree_finish<false>, grid, block, 0, p->stream, G);
    return MZ_OK;
}

// launches one search over inputs that are already resident in the planner's device buffers
static int launch_search(mz_planner* p, int batch, int deterministic, bool has_mask, bool injected_rng, bool scripted, const EnvLaunch* fenv = nullptr) {
    hipEvent_t ea = nullptr, eb = nullptr;
    if (p->profiling) {
        int rc = next_kernel_events(p, &ea, &eb);
        if (rc) return rc;
        HIPCHK(hipEventRecord(ea, p->stream));
    }
    const int rc = p->conv || p->hbm_tree ? launch_hbm_search(p, batch, deterministic, has_mask, injected_rng, scripted)
                                          : launch_lds_search(p, batch, deterministic, has_mask, injected_rng, scripted, fenv);
    if (rc) return rc;
    HIPCHK(hipGetLastError());
    if (p->profiling) HIPCHK(hipEventRecord(eb, p->stream));
    return MZ_OK;
}

static int upload_roots(mz_planner* p, int batch, const float* h_obs, const uint8_t* h_mask, const int32_t* h_cur, const int32_t* h_opp,
                        const double* h_temp, const mz_rng_inputs* rng, int deterministic) {
    const mz_config& c = p->cfg;
    const size_t B = (size_t)batch, A = (size_t)c.num_actions;
    if (h_obs) HIPCHK(hipMemcpyAsync(p->d_obs, h_obs, B * obs_dim(c) * sizeof(float), hipMemcpyHostToDevice, p->stream));
    if (h_mask) HIPCHK(hipMemcpyAsync(p->d_mask, h_mask, B * A, hipMemcpyHostToDevice, p->stream));
    HIPCHK(hipMemcpyAsync(p->d_cur, h_cur, B * sizeof(int), hipMemcpyHostToDevice, p->stream));
    HIPCHK(hipMemcpyAsync(p->d_opp, h_opp, B * sizeof(int), hipMemcpyHostToDevice, p->stream));
    HIPCHK(hipMemcpyAsync(p->d_temp, h_temp, B * sizeof(double), hipMemcpyHostToDevice, p->stream));
    if (rng) {
        const bool want_noise = !deterministic && c.root_dirichlet_alpha > 0.0 && c.root_exploration_eps > 0.0;
        if (want_noise) {
            if (!rng->h_noise) return fail(MZ_E_INVALID, "rng inputs given but h_noise is NULL while the search mixes Dirichlet noise");
            HIPCHK(hipMemcpyAsync(p->d_noise, rng->h_noise, B * A * sizeof(double), hipMemcpyHostToDevice, p->stream));
        }
        if (!rng->h_u_tie || (!deterministic && !rng->h_u_final)) return fail(MZ_E_INVALID, "rng inputs need h_u_tie and h_u_final");
        HIPCHK(hipMemcpyAsync(p->d_utie, rng->h_u_tie, B * (size_t)c.max_ties * sizeof(double), hipMemcpyHostToDevice, p->stream));
        if (rng->h_u_final) HIPCHK(hipMemcpyAsync(p->d_ufinal, rng->h_u_final, B * sizeof(double), hipMemcpyHostToDevice, p->stream));
    }
    return MZ_OK;
}

static int download_results(mz_planner* p, int batch, int32_t* h_action, double* h_pi, double* h_root, int32_t* h_visits) {
    const size_t B = (size_t)batch, A = (size_t)p->cfg.num_actions;
    int err = 0;
    if (h_action) HIPCHK(hipMemcpyAsync(h_action, p->d_action, B * sizeof(int), hipMemcpyDeviceToHost, p->stream));
    if (h_pi) HIPCHK(hipMemcpyAsync(h_pi, p->d_pi, B * A * sizeof(double), hipMemcpyDeviceToHost, p->stream));
    if (h_root) HIPCHK(hipMemcpyAsync(h_root, p->d_root, B * sizeof(double), hipMemcpyDeviceToHost, p->stream));
    if (h_visits) HIPCHK(hipMemcpyAsync(h_visits, p->d_visits, B * A * sizeof(int), hipMemcpyDeviceToHost, p->stream));
    HIPCHK(hipMemcpyAsync(&err, p->d_err, sizeof(int), hipMemcpyDeviceToHost, p->stream));
    HIPCHK(hipStreamSynchronize(p->stream));
    if (err) {
        HIPCHK(hipMemsetAsync(p->d_err, 0, sizeof(int), p->stream));
        HIPCHK(hipStreamSynchronize(p->stream));
        if (err == 4) return fail(MZ_E_TIES, "injected tie-break stream exhausted (raise mz_config.max_ties)");
        return fail(MZ_E_INVALID, "search kernel reported error " + std::to_string(err));
    }
    return MZ_OK;
}

extern "C" int mz_planner_search(mz_planner* p, int32_t batch, const float* h_obs, const uint8_t* h_mask, const int32_t* h_cur,
                                 const int32_t* h_opp, const double* h_temp, int32_t deterministic, const mz_rng_inputs* rng,
                                 int32_t* h_action, double* h_pi, double* h_root, int32_t* h_visits) {
    if (!p || !h_obs || !h_cur || !h_opp || !h_temp || !h_action || !h_pi || !h_root) return fail(MZ_E_INVALID, "null argument to mz_planner_search");
    if (batch < 1 || batch > p->cfg.num_envs) return fail(MZ_E_INVALID, "batch exceeds mz_config.num_envs");
    if (!p->committed) return fail(MZ_E_STATE, "weights not committed");
    HIPCHK(hipSetDevice(p->device));
    int rc = upload_roots(p, batch, h_obs, h_mask, h_cur, h_opp, h_temp, rng, deterministic);
    if (rc) return rc;
    rc = launch_search(p, batch, deterministic, h_mask != nullptr, rng != nullptr, false);
    if (rc) return rc;
    return download_results(p, batch, h_action, h_pi, h_root, h_visits);
}

extern "C" int mz_planner_search_scripted(mz_planner* p, int32_t batch, const float* h_pi0, const float* h_values, const float* h_rewards,
                                          const uint8_t* h_mask, const int32_t* h_cur, const int32_t* h_opp, const double* h_temp,
                                          int32_t deterministic, const mz_rng_inputs* rng, int32_t* h_action, double* h_pi, double* h_root,
                                          int32_t* h_visits, int32_t* h_tparent, int32_t* h_taction) {
    if (!p || !h_pi0 || !h_values || !h_rewards || !h_cur || !h_opp || !h_temp || !h_action || !h_pi || !h_root)
        return fail(MZ_E_INVALID, "null argument to mz_planner_search_scripted");
    if (batch < 1 || batch > p->cfg.num_envs) return fail(MZ_E_INVALID, "batch exceeds mz_config.num_envs");
    HIPCHK(hipSetDevice(p->device));
    const size_t B = (size_t)p->cfg.num_envs, A = (size_t)p->cfg.num_actions, S = (size_t)p->cfg.num_simulations;
    if (!p->d_spi0) {
        HIPCHK(hipMalloc(&p->d_spi0, B * A * sizeof(float)));
        HIPCHK(hipMalloc(&p->d_svalues, B * S * sizeof(float)));
        HIPCHK(hipMalloc(&p->d_srewards, B * S * sizeof(float)));
        HIPCHK(hipMalloc(&p->d_tparent, B * S * sizeof(int)));
        HIPCHK(hipMalloc(&p->d_taction, B * S * sizeof(int)));
    }
    const size_t b = (size_t)batch;
    HIPCHK(hipMemcpyAsync(p->d_spi0, h_pi0, b * A * sizeof(float), hipMemcpyHostToDevice, p->stream));
    HIPCHK(hipMemcpyAsync(p->d_svalues, h_values, b * S * sizeof(float), hipMemcpyHostToDevice, p->stream));
    HIPCHK(hipMemcpyAsync(p->d_srewards, h_rewards, b * S * sizeof(float), hipMemcpyHostToDevice, p->stream));
    int rc = upload_roots(p, batch, nullptr, h_mask, h_cur, h_opp, h_temp, rng, deterministic);
    if (rc) return rc;
    rc = launch_search(p, batch, deterministic, h_mask != nullptr, rng != nullptr, true);
    if (rc) return rc;
    if (h_tparent) HIPCHK(hipMemcpyAsync(h_tparent, p->d_tparent, b * S * sizeof(int), hipMemcpyDeviceToHost, p->stream));
    if (h_taction) HIPCHK(hipMemcpyAsync(h_taction, p->d_taction, b * S * sizeof(int), hipMemcpyDeviceToHost, p->stream));
    return download_results(p, batch, h_action, h_pi, h_root, h_visits);
}

// ---------------------------------------------------------------------------------------------------------
// device-resident self-play
// ---------------------------------------------------------------------------------------------------------
// Starts an empty record ring.  Its length: 64 moves (16 where that would pass 4 GB of observations) or, with a replay attached, every
// env's open trajectory -- a whole board game, or the acc + unroll + td window (pipeline.py:118-121), but never longer than an episode can
// get when its step limit is known (max_steps > 0): the classic configs set acc_seq_length = 9999 ("never flush mid-episode",
// config.py:198), and 10 014 slots x 4096 envs of CartPole records would be ~5 GB.
// Compact records (mz_selfplay_reset_external, MZ_RECORD_FRAMES_U8): `obs_bytes` is one env's record of a move (its padded frame) and the
// ring keeps `extra` = S moves more, which the window of the oldest move reaches back to (RecRing, mz_env.h).  The compact ring is
// host-stepped env state: ext_free is the one place that calls rec_free, and every reset of another mode starts with ext_free.
static void rec_free(mz_planner* p) {
    if (p->rr.frames) (void)hipFree(p->rr.frames);
    if (p->rr.age) (void)hipFree(p->rr.age);
    if (p->d_rec_stage) (void)hipFree(p->d_rec_stage);
    p->rr = RecRing{};
    p->rec_S = 0;
    p->d_rec_stage = nullptr;
}

static void ring_start(mz_planner* p, int max_steps, size_t obs_bytes = 0, int extra = 0) {
    const mz_config& c = p->cfg;
    if (obs_bytes == 0) obs_bytes = (size_t)obs_dim(c) * sizeof(float);
    p->ring_len = (size_t)c.num_envs * obs_bytes * 64 > ((size_t)4 << 30) ? 16 : 64;
    if (p->has_replay) {
        const int window = p->replay.acc + p->replay.K + p->replay.td;
        int need = c.is_board_game ? c.num_actions + 1 : window;
        if (max_steps > 0) {
            const int capped = max_steps + (c.is_board_game ? 1 : p->replay.K + p->replay.td);
            need = c.is_board_game ? capped : (window < capped ? window : capped);
        }
        if (need > p->ring_len) p->ring_len = (need + 7) & ~7;
    }
    p->ring_len += extra;
    p->selfplay_moves = 0;
    p->ring_pos = 0;
    p->ring_count = 0;
}

// after a move's records are in the ring: the attached replay's items (k_epi_scan -> k_epilogue -> k_epi_publish), then the next slot
static int ring_finish_move(mz_planner* p) {
    if (p->has_replay) {
        EpiLaunch E{};
        E.env = p->env; E.ring = p->replay; E.B = p->cfg.num_envs; E.move_abs = p->selfplay_moves; E.rr = p->rr;
        hipLaunchKernelGGL(k_epi_scan, dim3(1), dim3(1024), 0, p->stream, E);
        if (E.ring.state_format != STATE_F32) {  // compact states: before k_epilogue moves ep_start
            const int per = E.ring.state_format == STATE_I8 ? 1024 : 4096, chunks = (E.ring.row_bytes + 3 + per - 1) / per;
            if (p->rr.frames)  // (compact records: the reset admitted them with frames_u8 states only)
                hipLaunchKernelGGL(k_epi_states<true>, dim3(chunks < 64 ? chunks : 64, EPS_ITEMS), dim3(256), 0, p->stream, E);
            else
                hipLaunchKernelGGL(k_epi_states<false>, dim3(chunks < 64 ? chunks : 64, EPS_ITEMS), dim3(256), 0, p->stream, E);
        }
        hipLaunchKernelGGL(k_epilogue, dim3(p->cfg.num_envs), dim3(64), (size_t)p->ring_len * sizeof(double), p->stream, E);
        hipLaunchKernelGGL(k_epi_publish, dim3(1), dim3(1), 0, p->stream, p->replay);
    }
    HIPCHK(hipGetLastError());
    p->selfplay_moves++;
    p->ring_pos = (p->ring_pos + 1) % p->ring_len;
    if (p->ring_count < p->ring_len) p->ring_count++;
    return MZ_OK;
}

extern "C" int mz_selfplay_reset(mz_planner* p, int32_t env_kind, const double* h_init_state) {
    if (!p) return fail(MZ_E_INVALID, "null planner");
    HIPCHK(hipSetDevice(p->device));
    const mz_config& c = p->cfg;
    int board_n = 3, num_to_win = 3;
    if (env_kind == MZ_ENV_CARTPOLE) {
        if (c.num_actions != 2 || obs_dim(c) != 20) return fail(MZ_E_INVALID, "CartPole env needs num_actions == 2 and a (4,5) observation");
    } else if (env_kind == MZ_ENV_TICTACTOE) {
        if (c.num_actions != 10 || obs_dim(c) != 81) return fail(MZ_E_INVALID, "TicTacToe env needs num_actions == 10 and a (9,3,3) observation");
    } else if (env_kind == MZ_ENV_GOMOKU) {
        if (c.net_kind != MZ_NET_BOARD || c.obs_c != 9 || c.obs_h != c.obs_w || c.num_actions != c.obs_h * c.obs_w + 1 || c.obs_h < 5)
            return fail(MZ_E_INVALID, "Gomoku env needs a board net with a (9,N,N) observation, N >= 5, and num_actions == N*N + 1");
        board_n = c.obs_h;
        num_to_win = 5;
    } else if (env_kind == MZ_ENV_SYNTHETIC) {
        if (h_init_state) return fail(MZ_E_INVALID, "the synthetic env takes no initial state");
    } else if (env_kind == MZ_ENV_CATCH) {
        return fail(MZ_E_INVALID, "MZ_ENV_CATCH has its own reset: mz_selfplay_reset_catch");
    } else if (env_kind == MZ_ENV_BREAKOUT) {
        return fail(MZ_E_INVALID, "MZ_ENV_BREAKOUT has its own reset: mz_selfplay_reset_breakout");
    } else if (env_kind == MZ_ENV_CONNECT4) {
        return fail(MZ_E_INVALID, "MZ_ENV_CONNECT4 has its own reset: mz_selfplay_reset_connect4");
    } else if (env_kind == MZ_ENV_OTHELLO) {
        return fail(MZ_E_INVALID, "MZ_ENV_OTHELLO has its own reset: mz_selfplay_reset_othello");
    } else if (env_kind == MZ_ENV_GO) {
        return fail(MZ_E_INVALID, "MZ_ENV_GO has its own reset: mz_selfplay_reset_go");
    } else {
        return fail(MZ_E_INVALID, "unknown env kind");
    }
    if (p->has_replay && p->replay.state_format != STATE_F32) {
        if (p->replay.state_format != STATE_I8 || (env_kind != MZ_ENV_TICTACTOE && env_kind != MZ_ENV_GOMOKU))
            return fail(MZ_E_INVALID, "mz_replay_ring.state_format: of the device envs only TicTacToe and Gomoku have exact compact states (MZ_STATE_I8); "
                                      "CartPole and the synthetic env need MZ_STATE_F32, MZ_STATE_FRAMES_U8 a host-stepped env with uint8 frames");
        p->replay.row_bytes = obs_dim(c);
        p->replay.enc_err = nullptr;
    }
    ext_free(p);  // (leaves host-stepped self-play: its buffers and a compact record ring end here)
    p->env_kind = env_kind;
    p->arena_open = false;
    // gym's TimeLimit ends CartPole after 500 steps, the synthetic frames env after 1000; a board game's ring holds the whole game
    const int limit = env_kind == MZ_ENV_CARTPOLE ? 500 : (env_kind == MZ_ENV_SYNTHETIC ? 1000 : (1 << 30) - 64);
    ring_start(p, c.is_board_game ? 0 : limit);
    hipError_t e = env_alloc(p->env, env_kind, c.num_envs, c.num_actions, obs_dim(c), p->ring_len, board_n, num_to_win);
    if (e != hipSuccess) return fail(MZ_E_HIP, std::string("env_alloc: ") + hipGetErrorString(e));
    if (h_init_state) HIPCHK(hipMemcpyAsync(p->env.init_state, h_init_state, (size_t)c.num_envs * 4 * sizeof(double), hipMemcpyHostToDevice, p->stream));
    EnvLaunch L{};
    L.env = p->env; L.B = c.num_envs; L.seed = c.seed; L.use_init = h_init_state != nullptr;
    L.obs = p->d_obs; L.mask = p->d_mask; L.cur = p->d_cur; L.opp = p->d_opp;
    hipLaunchKernelGGL(k_env_reset, dim3((c.num_envs + 255) / 256), dim3(256), 0, p->stream, L);
    if (env_kind == MZ_ENV_SYNTHETIC)
        hipLaunchKernelGGL(k_env_synth_obs, dim3(((size_t)c.num_envs * ((obs_dim(c) + 3) / 4) + 255) / 256), dim3(256), 0, p->stream, L);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(p->stream));
    return MZ_OK;
}

// ---------------------------------------------------------------------------------------------------------
// Connect Four (mz_connect4.h): its own reset, pre and step launches around the board-net search
// ---------------------------------------------------------------------------------------------------------
static C4Launch c4_launch(mz_planner* p, const EnvLaunch& L) {
    C4Launch P{};
    P.L = L; P.rows = p->cfg.obs_h; P.cols = p->cfg.obs_w; P.temp_steps = p->c4_temp_steps;
    return P;
}

// what both resets check: the net, the board and the env struct; every refusal names the offending field
static int c4_check(mz_planner* p, const mz_connect4_env* env, const std::string& fn) {
    const mz_config& c = p->cfg;
    if (c.net_kind != MZ_NET_BOARD) return fail(MZ_E_INVALID, fn + ": mz_config.net_kind must be MZ_NET_BOARD (Connect Four plays on the board conv net)");
    if (c.obs_c != 9) return fail(MZ_E_INVALID, fn + ": mz_config.obs_c must be 9 (4 history planes per colour and the colour plane), not " + std::to_string(c.obs_c));
    if (c.num_actions != c.obs_w + 1)
        return fail(MZ_E_INVALID, fn + ": mz_config.num_actions must be obs_w + 1 = " + std::to_string(c.obs_w + 1) + " (one per column, and resign), not " + std::to_string(c.num_actions));
    if (c.obs_h * c.obs_w > 64)
        return fail(MZ_E_INVALID, fn + ": mz_config.obs_h * obs_w = " + std::to_string(c.obs_h * c.obs_w) + " points, the board holds at most 64 (one 64-bit bitboard per colour)");
    const int longest = c.obs_h > c.obs_w ? c.obs_h : c.obs_w;
    if (env->num_to_win < 2 || env->num_to_win > longest)
        return fail(MZ_E_INVALID, fn + ": mz_connect4_env.num_to_win must be in 2 .. max(obs_h, obs_w) = " + std::to_string(longest) + ", not " + std::to_string(env->num_to_win));
    if (env->temp_switch_steps < 0) return fail(MZ_E_INVALID, fn + ": mz_connect4_env.temp_switch_steps must be >= 0");
    return MZ_OK;
}

extern "C" int mz_selfplay_reset_connect4(mz_planner* p, const mz_connect4_env* env) {
    if (!p || !env) return fail(MZ_E_INVALID, "null argument to mz_selfplay_reset_connect4");
    HIPCHK(hipSetDevice(p->device));
    const mz_config& c = p->cfg;
    int rc = c4_check(p, env, "mz_selfplay_reset_connect4");
    if (rc) return rc;
    if (p->has_replay && p->replay.state_format != STATE_F32) {
        if (p->replay.state_format != STATE_I8)
            return fail(MZ_E_INVALID, "mz_replay_ring.state_format: the device Connect Four env has float32 (MZ_STATE_F32) and exact int8 (MZ_STATE_I8) states; "
                                      "MZ_STATE_FRAMES_U8 needs a host-stepped env with uint8 frames");
        p->replay.row_bytes = obs_dim(c);
        p->replay.enc_err = nullptr;
    }
    ext_free(p);
    p->env_kind = MZ_ENV_CONNECT4;
    p->arena_open = false;
    p->c4_temp_steps = env->temp_switch_steps > 0 ? env->temp_switch_steps : 6;  // (the existing rule's value for num_actions <= 10)
    const int nn = c.obs_h * c.obs_w;
    ring_start(p, c.is_board_game ? nn : (1 << 30) - 64);  // a board game's ring holds the whole game: at most one ply per point
    hipError_t e = env_alloc(p->env, ENV_CONNECT4, c.num_envs, c.num_actions, obs_dim(c), p->ring_len, c.obs_w, env->num_to_win, true, nn);
    if (e != hipSuccess) return fail(MZ_E_HIP, std::string("env_alloc: ") + hipGetErrorString(e));
    EnvLaunch L{};
    L.env = p->env; L.B = c.num_envs; L.seed = c.seed;
    L.obs = p->d_obs; L.mask = p->d_mask; L.cur = p->d_cur; L.opp = p->d_opp;
    hipLaunchKernelGGL(k_c4_reset, dim3((c.num_envs + 255) / 256), dim3(256), 0, p->stream, c4_launch(p, L));
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(p->stream));
    return MZ_OK;
}

// one move: temperatures and the record's first half, the search (or, search == false, the caller's d_action / d_pi / d_root), env.step +
// record + auto-reset
static int c4_move(mz_planner* p, const EnvLaunch& L, bool search) {
    const mz_config& c = p->cfg;
    const C4Launch P = c4_launch(p, L);
    hipLaunchKernelGGL(k_c4_pre, dim3((c.num_envs + 255) / 256), dim3(256), 0, p->stream, P);
    HIPCHK(hipMemcpyAsync(p->env.r_obs + (size_t)p->ring_pos * c.num_envs * obs_dim(c), p->d_obs, (size_t)c.num_envs * obs_dim(c) * sizeof(float),
                          hipMemcpyDeviceToDevice, p->stream));
    if (search) {
        int rc = launch_search(p, c.num_envs, 0, true, false, false);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(k_c4_step, dim3((c.num_envs + 15) / 16), dim3(256), 0, p->stream, P);
    return MZ_OK;
}

// Test hook: one move of all envs with the caller's actions through the launches of a self-play move, without the search.  The recorded
// policy is the one-hot of the action, the root value 0.
extern "C" int mz_connect4_debug_step(mz_planner* p, const int32_t* h_action) {
    if (!p || !h_action) return fail(MZ_E_INVALID, "null argument to mz_connect4_debug_step");
    if (p->env_kind != MZ_ENV_CONNECT4 || p->arena_open) return fail(MZ_E_STATE, "mz_connect4_debug_step: call mz_selfplay_reset_connect4 first");
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(hipStreamSynchronize(p->stream));
    const mz_config& c = p->cfg;
    const size_t B = (size_t)c.num_envs, A = (size_t)c.num_actions;
    std::vector<unsigned char> mask(B * A);
    HIPCHK(hipMemcpy(mask.data(), p->d_mask, B * A, hipMemcpyDeviceToHost));
    std::vector<double> pi(B * A, 0.0), root(B, 0.0);
    for (size_t e = 0; e < B; e++) {
        const int a = h_action[e];
        if (a < 0 || a >= (int)A || !mask[e * A + a])
            return fail(MZ_E_INVALID, "mz_connect4_debug_step: h_action[" + std::to_string(e) + "] = " + std::to_string(a) + " is not a legal action of env " + std::to_string(e));
        pi[e * A + a] = 1.0;
    }
    HIPCHK(hipMemcpy(p->d_action, h_action, B * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(p->d_pi, pi.data(), B * A * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(p->d_root, root.data(), B * sizeof(double), hipMemcpyHostToDevice));
    EnvLaunch L{};
    L.env = p->env; L.B = c.num_envs; L.seed = c.seed; L.temperature = 1.0; L.move_counter = p->move_counter;
    L.obs = p->d_obs; L.mask = p->d_mask; L.cur = p->d_cur; L.opp = p->d_opp; L.temp_out = p->d_temp;
    L.action = p->d_action; L.pi = p->d_pi; L.root = p->d_root; L.slot = p->ring_pos; L.sims = 0;
    int rc = c4_move(p, L, false);
    if (rc) return rc;
    return ring_finish_move(p);
}

// Test hook: the envs' legal-action masks as the next search will see them, uint8 [B, A]
extern "C" int mz_connect4_debug_mask(mz_planner* p, uint8_t* h_mask) {
    if (!p || !h_mask) return fail(MZ_E_INVALID, "null argument to mz_connect4_debug_mask");
    if (p->env_kind != MZ_ENV_CONNECT4 || p->arena_open) return fail(MZ_E_STATE, "mz_connect4_debug_mask: call mz_selfplay_reset_connect4 first");
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(hipStreamSynchronize(p->stream));
    HIPCHK(hipMemcpy(h_mask, p->d_mask, (size_t)p->cfg.num_envs * p->cfg.num_actions, hipMemcpyDeviceToHost));
    return MZ_OK;
}

// ---------------------------------------------------------------------------------------------------------
// Othello (mz_othello.h): its own reset, pre and step launches around the board-net search
// ---------------------------------------------------------------------------------------------------------
static OthLaunch oth_launch(mz_planner* p, const EnvLaunch& L) {
    OthLaunch P{};
    P.L = L; P.rows = p->cfg.obs_h; P.cols = p->cfg.obs_w; P.temp_steps = p->oth_temp_steps;
    return P;
}

// what both resets check: the net, the board and the env struct; every refusal names the offending field
static int oth_check(mz_planner* p, const mz_othello_env* env, const std::string& fn) {
    const mz_config& c = p->cfg;
    if (c.net_kind != MZ_NET_BOARD) return fail(MZ_E_INVALID, fn + ": mz_config.net_kind must be MZ_NET_BOARD (Othello plays on the board conv net)");
    if (c.obs_c != 9) return fail(MZ_E_INVALID, fn + ": mz_config.obs_c must be 9 (4 history planes per colour and the colour plane), not " + std::to_string(c.obs_c));
    if (c.obs_h < 4 || c.obs_h > 8) return fail(MZ_E_INVALID, fn + ": mz_config.obs_h must be in 4 .. 8 (rows of a board of at most 64 points), not " + std::to_string(c.obs_h));
    if (c.obs_w < 4 || c.obs_w > 8) return fail(MZ_E_INVALID, fn + ": mz_config.obs_w must be in 4 .. 8 (columns of a board of at most 64 points), not " + std::to_string(c.obs_w));
    if (c.num_actions != c.obs_h * c.obs_w + 2)
        return fail(MZ_E_INVALID, fn + ": mz_config.num_actions must be obs_h * obs_w + 2 = " + std::to_string(c.obs_h * c.obs_w + 2) + " (one per point, pass, resign), not " + std::to_string(c.num_actions));
    if (env->temp_switch_steps < 0) return fail(MZ_E_INVALID, fn + ": mz_othello_env.temp_switch_steps must be >= 0");
    return MZ_OK;
}

extern "C" int mz_selfplay_reset_othello(mz_planner* p, const mz_othello_env* env) {
    if (!p || !env) return fail(MZ_E_INVALID, "null argument to mz_selfplay_reset_othello");
    HIPCHK(hipSetDevice(p->device));
    const mz_config& c = p->cfg;
    int rc = oth_check(p, env, "mz_selfplay_reset_othello");
    if (rc) return rc;
    if (p->has_replay && p->replay.state_format != STATE_F32) {
        if (p->replay.state_format != STATE_I8)
            return fail(MZ_E_INVALID, "mz_replay_ring.state_format: the device Othello env has float32 (MZ_STATE_F32) and exact int8 (MZ_STATE_I8) states; "
                                      "MZ_STATE_FRAMES_U8 needs a host-stepped env with uint8 frames");
        p->replay.row_bytes = obs_dim(c);
        p->replay.enc_err = nullptr;
    }
    ext_free(p);
    p->env_kind = MZ_ENV_OTHELLO;
    p->arena_open = false;
    p->oth_temp_steps = env->temp_switch_steps > 0 ? env->temp_switch_steps : 6;
    const int nn = c.obs_h * c.obs_w;
    // a board game's ring holds the whole game: at most nn - 4 placements, each after at most one pass (a resignation takes the place of a ply)
    ring_start(p, c.is_board_game ? 2 * (nn - 4) : (1 << 30) - 64);
    hipError_t e = env_alloc(p->env, ENV_OTHELLO, c.num_envs, c.num_actions, obs_dim(c), p->ring_len, c.obs_w, 0, true, nn);
    if (e != hipSuccess) return fail(MZ_E_HIP, std::string("env_alloc: ") + hipGetErrorString(e));
    EnvLaunch L{};
    L.env = p->env; L.B = c.num_envs; L.seed = c.seed;
    L.obs = p->d_obs; L.mask = p->d_mask; L.cur = p->d_cur; L.opp = p->d_opp;
    hipLaunchKernelGGL(k_oth_reset, dim3((c.num_envs + 255) / 256), dim3(256), 0, p->stream, oth_launch(p, L));
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(p->stream));
    return MZ_OK;
}

// one move: temperatures and the record's first half, the search (or, search == false, the caller's d_action / d_pi / d_root), env.step +
// record + auto-reset
static int oth_move(mz_planner* p, const EnvLaunch& L, bool search) {
    const mz_config& c = p->cfg;
    const OthLaunch P = oth_launch(p, L);
    hipLaunchKernelGGL(k_oth_pre, dim3((c.num_envs + 255) / 256), dim3(256), 0, p->stream, P);
    HIPCHK(hipMemcpyAsync(p->env.r_obs + (size_t)p->ring_pos * c.num_envs * obs_dim(c), p->d_obs, (size_t)c.num_envs * obs_dim(c) * sizeof(float),
                          hipMemcpyDeviceToDevice, p->stream));
    if (search) {
        int rc = launch_search(p, c.num_envs, 0, true, false, false);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(k_oth_step, dim3((c.num_envs + 15) / 16), dim3(256), 0, p->stream, P);
    return MZ_OK;
}

// Test hook: one move of all envs with the caller's actions through the launches of a self-play move, without the search.  The recorded
// policy is the one-hot of the action, the root value 0.
extern "C" int mz_othello_debug_step(mz_planner* p, const int32_t* h_action) {
    if (!p || !h_action) return fail(MZ_E_INVALID, "null argument to mz_othello_debug_step");
    if (p->env_kind != MZ_ENV_OTHELLO || p->arena_open) return fail(MZ_E_STATE, "mz_othello_debug_step: call mz_selfplay_reset_othello first");
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(hipStreamSynchronize(p->stream));
    const mz_config& c = p->cfg;
    const size_t B = (size_t)c.num_envs, A = (size_t)c.num_actions;
    std::vector<unsigned char> mask(B * A);
    HIPCHK(hipMemcpy(mask.data(), p->d_mask, B * A, hipMemcpyDeviceToHost));
    std::vector<double> pi(B * A, 0.0), root(B, 0.0);
    for (size_t e = 0; e < B; e++) {
        const int a = h_action[e];
        if (a < 0 || a >= (int)A || !mask[e * A + a])
            return fail(MZ_E_INVALID, "mz_othello_debug_step: h_action[" + std::to_string(e) + "] = " + std::to_string(a) + " is not a legal action of env " + std::to_string(e));
        pi[e * A + a] = 1.0;
    }
    HIPCHK(hipMemcpy(p->d_action, h_action, B * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(p->d_pi, pi.data(), B * A * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(p->d_root, root.data(), B * sizeof(double), hipMemcpyHostToDevice));
    EnvLaunch L{};
    L.env = p->env; L.B = c.num_envs; L.seed = c.seed; L.temperature = 1.0; L.move_counter = p->move_counter;
    L.obs = p->d_obs; L.mask = p->d_mask; L.cur = p->d_cur; L.opp = p->d_opp; L.temp_out = p->d_temp;
    L.action = p->d_action; L.pi = p->d_pi; L.root = p->d_root; L.slot = p->ring_pos; L.sims = 0;
    int rc = oth_move(p, L, false);
    if (rc) return rc;
    return ring_finish_move(p);
}

// Test hook: the envs' legal-action masks as the next search will see them, uint8 [B, A]
extern "C" int mz_othello_debug_mask(mz_planner* p, uint8_t* h_mask) {
    if (!p || !h_mask) return fail(MZ_E_INVALID, "null argument to mz_othello_debug_mask");
    if (p->env_kind != MZ_ENV_OTHELLO || p->arena_open) return fail(MZ_E_STATE, "mz_othello_debug_mask: call mz_selfplay_reset_othello first");
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(hipStreamSynchronize(p->stream));
    HIPCHK(hipMemcpy(h_mask, p->d_mask, (size_t)p->cfg.num_envs * p->cfg.num_actions, hipMemcpyDeviceToHost));
    return MZ_OK;
}

// Test hook: the envs' boards, int8 [B, nn] (0 empty, 1 black, 2 white) -- in self-play the positions the next move starts from, in an
// arena the live games' positions and the finished games' frozen final boards
extern "C" int mz_othello_debug_board(mz_planner* p, int8_t* h_board) {
    if (!p || !h_board) return fail(MZ_E_INVALID, "null argument to mz_othello_debug_board");
    if (p->env_kind != MZ_ENV_OTHELLO) return fail(MZ_E_STATE, "mz_othello_debug_board: call mz_selfplay_reset_othello or mz_arena_reset_othello first");
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(hipStreamSynchronize(p->stream));
    HIPCHK(hipMemcpy(h_board, p->env.board, (size_t)p->cfg.num_envs * p->env.nn, hipMemcpyDeviceToHost));
    return MZ_OK;
}

// ---------------------------------------------------------------------------------------------------------
// Go (mz_go.h): its own reset, pre and step launches around the board-net search; one workgroup per env
// ---------------------------------------------------------------------------------------------------------
// what both resets check: the net, the board and the env struct; every refusal names the offending field.  Changes nothing: a refused
// reset leaves a running game's rules as they were (go_apply stores them once every check has passed).
static int go_check(mz_planner* p, const mz_go_env* env, const std::string& fn) {
    const mz_config& c = p->cfg;
    if (c.net_kind != MZ_NET_BOARD) return fail(MZ_E_INVALID, fn + ": mz_config.net_kind must be MZ_NET_BOARD (Go plays on the board conv net)");
    if (c.obs_c != 9) return fail(MZ_E_INVALID, fn + ": mz_config.obs_c must be 9 (4 history planes per colour and the colour plane), not " + std::to_string(c.obs_c));
    if (c.obs_h < 3 || c.obs_h > 19) return fail(MZ_E_INVALID, fn + ": mz_config.obs_h must be in 3 .. 19 (rows of the board), not " + std::to_string(c.obs_h));
    if (c.obs_w < 3 || c.obs_w > 19) return fail(MZ_E_INVALID, fn + ": mz_config.obs_w must be in 3 .. 19 (columns of the board), not " + std::to_string(c.obs_w));
    const int nn = c.obs_h * c.obs_w;
    if (c.obs_h != c.obs_w && nn > 64)
        return fail(MZ_E_INVALID, fn + ": mz_config.obs_h x obs_w = " + std::to_string(c.obs_h) + " x " + std::to_string(c.obs_w) +
                                      ": a board of more than 64 points must be square (non-square boards above 64 points are not held to the oracle search and are refused)");
    if (c.num_actions != nn + 2)
        return fail(MZ_E_INVALID, fn + ": mz_config.num_actions must be obs_h * obs_w + 2 = " + std::to_string(nn + 2) + " (one per point, pass, resign), not " + std::to_string(c.num_actions));
    if (env->temp_switch_steps < 0) return fail(MZ_E_INVALID, fn + ": mz_go_env.temp_switch_steps must be >= 0");
    if (env->komi2 < 0 || env->komi2 > 2 * nn) return fail(MZ_E_INVALID, fn + ": mz_go_env.komi2 must be in 0 .. 2 * obs_h * obs_w = " + std::to_string(2 * nn) + ", not " + std::to_string(env->komi2));
    if (env->max_plies < 0 || env->max_plies > 2 * nn)
        return fail(MZ_E_INVALID, fn + ": mz_go_env.max_plies must be 0 (2 * obs_h * obs_w) or in 1 .. " + std::to_string(2 * nn) + ", not " + std::to_string(env->max_plies));
    if (env->allow_resign != 0 && env->allow_resign != 1) return fail(MZ_E_INVALID, fn + ": mz_go_env.allow_resign must be 0 or 1");
    return MZ_OK;
}

// the rules of an accepted reset and the two per-env arrays (ko point, pass flag) into p->go
static int go_apply(mz_planner* p, const mz_go_env* env) {
    const mz_config& c = p->cfg;
    const int nn = c.obs_h * c.obs_w;
    if (p->go_cap < c.num_envs) {
        if (p->go.ko) (void)hipFree(p->go.ko);
        if (p->go.passf) (void)hipFree(p->go.passf);
        p->go.ko = nullptr; p->go.passf = nullptr; p->go_cap = 0;
        HIPCHK(hipMalloc(&p->go.ko, (size_t)c.num_envs * sizeof(int)));
        HIPCHK(hipMalloc(&p->go.passf, (size_t)c.num_envs * sizeof(int)));
        p->go_cap = c.num_envs;
    }
    p->go.rows = c.obs_h; p->go.cols = c.obs_w;
    p->go.komi2 = env->komi2;
    p->go.max_plies = env->max_plies > 0 ? env->max_plies : 2 * nn;
    p->go.allow_resign = env->allow_resign;
    p->go.temp_steps = env->temp_switch_steps > 0 ? env->temp_switch_steps : 6;
    return MZ_OK;
}

extern "C" int mz_selfplay_reset_go(mz_planner* p, const mz_go_env* env) {
    if (!p || !env) return fail(MZ_E_INVALID, "null argument to mz_selfplay_reset_go");
    HIPCHK(hipSetDevice(p->device));
    const mz_config& c = p->cfg;
    if (p->has_replay && p->replay.state_format != STATE_F32 && p->replay.state_format != STATE_I8)
        return fail(MZ_E_INVALID, "mz_replay_ring.state_format: the device Go env has float32 (MZ_STATE_F32) and exact int8 (MZ_STATE_I8) states; "
                                  "MZ_STATE_FRAMES_U8 needs a host-stepped env with uint8 frames");
    int rc = go_check(p, env, "mz_selfplay_reset_go");
    if (rc) return rc;
    rc = go_apply(p, env);
    if (rc) return rc;
    if (p->has_replay && p->replay.state_format == STATE_I8) {
        p->replay.row_bytes = obs_dim(c);
        p->replay.enc_err = nullptr;
    }
    ext_free(p);
    p->env_kind = MZ_ENV_GO;
    p->arena_open = false;
    const int nn = c.obs_h * c.obs_w;
    // a board game's ring holds the whole game: max_plies plies
    ring_start(p, c.is_board_game ? p->go.max_plies : (1 << 30) - 64);
    hipError_t e = env_alloc(p->env, ENV_GO, c.num_envs, c.num_actions, obs_dim(c), p->ring_len, c.obs_w, 0, true, nn);
    if (e != hipSuccess) return fail(MZ_E_HIP, std::string("env_alloc: ") + hipGetErrorString(e));
    GoLaunch P{};
    P.L.env = p->env; P.L.B = c.num_envs; P.L.seed = c.seed;
    P.L.obs = p->d_obs; P.L.mask = p->d_mask; P.L.cur = p->d_cur; P.L.opp = p->d_opp;
    P.G = p->go;
    hipLaunchKernelGGL(k_go_reset, dim3(c.num_envs), dim3(go_block(nn)), 0, p->stream, P);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(p->stream));
    return MZ_OK;
}

// one move: temperatures and the record's first half, the search (or, search == false, the caller's d_action / d_pi / d_root), env.step +
// record + auto-reset
static int go_move(mz_planner* p, const EnvLaunch& L, bool search) {
    const mz_config& c = p->cfg;
    GoLaunch P{};
    P.L = L; P.G = p->go;
    hipLaunchKernelGGL(k_go_pre, dim3((c.num_envs + 255) / 256), dim3(256), 0, p->stream, P);
    HIPCHK(hipMemcpyAsync(p->env.r_obs + (size_t)p->ring_pos * c.num_envs * obs_dim(c), p->d_obs, (size_t)c.num_envs * obs_dim(c) * sizeof(float),
                          hipMemcpyDeviceToDevice, p->stream));
    if (search) {
        int rc = launch_search(p, c.num_envs, 0, true, false, false);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(k_go_step, dim3(c.num_envs), dim3(go_block(c.obs_h * c.obs_w)), 0, p->stream, P);
    return MZ_OK;
}

// Test hook: one move of all envs with the caller's actions through the launches of a self-play move, without the search.  The recorded
// policy is the one-hot of the action, the root value 0.
extern "C" int mz_go_debug_step(mz_planner* p, const int32_t* h_action) {
    if (!p || !h_action) return fail(MZ_E_INVALID, "null argument to mz_go_debug_step");
    if (p->env_kind != MZ_ENV_GO || p->arena_open) return fail(MZ_E_STATE, "mz_go_debug_step: call mz_selfplay_reset_go first");
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(hipStreamSynchronize(p->stream));
    const mz_config& c = p->cfg;
    const size_t B = (size_t)c.num_envs, A = (size_t)c.num_actions;
    std::vector<unsigned char> mask(B * A);
    HIPCHK(hipMemcpy(mask.data(), p->d_mask, B * A, hipMemcpyDeviceToHost));
    std::vector<double> pi(B * A, 0.0), root(B, 0.0);
    for (size_t e = 0; e < B; e++) {
        const int a = h_action[e];
        if (a < 0 || a >= (int)A || !mask[e * A + a])
            return fail(MZ_E_INVALID, "mz_go_debug_step: h_action[" + std::to_string(e) + "] = " + std::to_string(a) + " is not a legal action of env " + std::to_string(e));
        pi[e * A + a] = 1.0;
    }
    HIPCHK(hipMemcpy(p->d_action, h_action, B * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(p->d_pi, pi.data(), B * A * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(p->d_root, root.data(), B * sizeof(double), hipMemcpyHostToDevice));
    EnvLaunch L{};
    L.env = p->env; L.B = c.num_envs; L.seed = c.seed; L.temperature = 1.0; L.move_counter = p->move_counter;
    L.obs = p->d_obs; L.mask = p->d_mask; L.cur = p->d_cur; L.opp = p->d_opp; L.temp_out = p->d_temp;
    L.action = p->d_action; L.pi = p->d_pi; L.root = p->d_root; L.slot = p->ring_pos; L.sims = 0;
    int rc = go_move(p, L, false);
    if (rc) return rc;
    return ring_finish_move(p);
}

// Test hook: the envs' legal-action masks as the next search will see them, uint8 [B, A]
extern "C" int mz_go_debug_mask(mz_planner* p, uint8_t* h_mask) {
    if (!p || !h_mask) return fail(MZ_E_INVALID, "null argument to mz_go_debug_mask");
    if (p->env_kind != MZ_ENV_GO || p->arena_open) return fail(MZ_E_STATE, "mz_go_debug_mask: call mz_selfplay_reset_go first");
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(hipStreamSynchronize(p->stream));
    HIPCHK(hipMemcpy(h_mask, p->d_mask, (size_t)p->cfg.num_envs * p->cfg.num_actions, hipMemcpyDeviceToHost));
    return MZ_OK;
}

// Test hook: the envs' boards, int8 [B, nn] (0 empty, 1 black, 2 white) -- in self-play the positions the next move starts from, in an
// arena the live games' positions and the finished games' frozen final boards
extern "C" int mz_go_debug_board(mz_planner* p, int8_t* h_board) {
    if (!p || !h_board) return fail(MZ_E_INVALID, "null argument to mz_go_debug_board");
    if (p->env_kind != MZ_ENV_GO) return fail(MZ_E_STATE, "mz_go_debug_board: call mz_selfplay_reset_go or mz_arena_reset_go first");
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(hipStreamSynchronize(p->stream));
    HIPCHK(hipMemcpy(h_board, p->env.board, (size_t)p->cfg.num_envs * p->env.nn, hipMemcpyDeviceToHost));
    return MZ_OK;
}

extern "C" int mz_selfplay_step(mz_planner* p, double temperature, int32_t n_moves) {
    if (!p || n_moves < 1) return fail(MZ_E_INVALID, "bad argument to mz_selfplay_step");
    if (p->arena_open) return fail(MZ_E_STATE, "mz_selfplay_step during an arena: call mz_selfplay_reset first");
    if (p->env_kind == MZ_ENV_NONE) return fail(MZ_E_STATE, "call mz_selfplay_reset first");
    if (p->env_kind == MZ_ENV_EXTERNAL) return fail(MZ_E_STATE, "mz_selfplay_step on host-stepped envs: use mz_selfplay_external_act / _commit");
    if (!p->committed) return fail(MZ_E_STATE, "weights not committed");
    HIPCHK(hipSetDevice(p->device));
    if (const ImageGame* g = image_game(p->env_kind)) return image_game_moves(p, *g, temperature, n_moves);
    const mz_config& c = p->cfg;
    for (int m = 0; m < n_moves; m++) {
        EnvLaunch L{};
        L.env = p->env; L.B = c.num_envs; L.seed = c.seed; L.temperature = temperature; L.move_counter = p->move_counter;
        L.obs = p->d_obs; L.mask = p->d_mask; L.cur = p->d_cur; L.opp = p->d_opp; L.temp_out = p->d_temp;
        L.action = p->d_action; L.pi = p->d_pi; L.root = p->d_root; L.slot = p->ring_pos; L.sims = c.num_simulations;
        if (p->env_kind == MZ_ENV_CONNECT4) {
            int rc = c4_move(p, L, true);
            if (rc) return rc;
        } else if (p->env_kind == MZ_ENV_OTHELLO) {
            int rc = oth_move(p, L, true);
            if (rc) return rc;
        } else if (p->env_kind == MZ_ENV_GO) {
            int rc = go_move(p, L, true);
            if (rc) return rc;
        } else if (!p->conv && !p->hbm_tree && p->env_kind != MZ_ENV_SYNTHETIC) {  // (synthetic frames are redrawn by k_env_synth_obs below)
            // MLP nets with LDS trees: the whole move -- temperature / record, search, env.step, auto-reset -- is ONE kernel launch
            // (C2: 727.7 us per move against 734.6 us for the four launches below, same box, same build)
            int rc = launch_search(p, c.num_envs, 0, true, false, false, &L);
            if (rc) return rc;
        } else {
            // temperatures for this move, then the search, then env.step + record + auto-reset
            hipLaunchKernelGGL(k_env_pre, dim3((c.num_envs + 255) / 256), dim3(256), 0, p->stream, L);
            HIPCHK(hipMemcpyAsync(p->env.r_obs + (size_t)p->ring_pos * c.num_envs * obs_dim(c), p->d_obs, (size_t)c.num_envs * obs_dim(c) * sizeof(float),
                                  hipMemcpyDeviceToDevice, p->stream));
            int rc = launch_search(p, c.num_envs, 0, true, false, false);
            if (rc) return rc;
            hipLaunchKernelGGL(k_env_step, dim3((c.num_envs + 15) / 16), dim3(256), 0, p->stream, L);
            if (p->env_kind == MZ_ENV_SYNTHETIC)
                hipLaunchKernelGGL(k_env_synth_obs, dim3(((size_t)c.num_envs * ((obs_dim(c) + 3) / 4) + 255) / 256), dim3(256), 0, p->stream, L);
        }
        int rc = ring_finish_move(p);
        if (rc) return rc;
    }
    return MZ_OK;
}

// ---------------------------------------------------------------------------------------------------------
// self-play on host-stepped environments (mz_extenv.h)
// ---------------------------------------------------------------------------------------------------------
static void ext_free(mz_planner* p) {
    void* dbufs[] = {p->ext.frames, p->ext.hist, p->ext.hist_act, p->ext.head, p->ext.reward, p->ext.done, p->ext.err, p->ext.enc_err};
    if (p->ext.enc_err) p->replay.enc_err = nullptr;
    for (void* b : dbufs)
        if (b) (void)hipFree(b);
    void* hbufs[] = {p->h_ext_frames, p->h_ext_mask, p->h_ext_done, p->h_ext_cur, p->h_ext_opp, p->h_ext_action, p->h_ext_err, p->h_ext_reward};
    for (void* b : hbufs)
        if (b) (void)hipHostFree(b);
    p->ext = ExtEnv{};
    rec_free(p);
    std::apply([](auto&... g) { (((void)hipFree(g.s), g = {}), ...); }, p->games);  // (hipFree(nullptr) is a no-op)
    p->h_ext_frames = nullptr; p->h_ext_mask = p->h_ext_done = nullptr;
    p->h_ext_cur = p->h_ext_opp = p->h_ext_action = p->h_ext_err = nullptr;
    p->h_ext_reward = nullptr;
}

static ExtLaunch ext_launch(mz_planner* p, double temperature) {
    const mz_config& c = p->cfg;
    ExtLaunch L{};
    L.env = p->env; L.x = p->ext; L.B = c.num_envs; L.A = c.num_actions; L.OD = p->ext_od;
    L.slot = p->ring_pos; L.prev_slot = (p->ring_pos + p->ring_len - 1) % p->ring_len; L.first = p->selfplay_moves == 0;
    L.parity = (int)(p->selfplay_moves & 1); L.sims = c.num_simulations; L.check = p->has_replay ? 1 : 0; L.move_abs = p->selfplay_moves;
    L.temperature = temperature; L.obs = p->d_obs; L.cur = p->d_cur; L.temp_out = p->d_temp;
    L.action = p->d_action; L.pi = p->d_pi; L.root = p->d_root; L.rr = p->rr;
    return L;
}

// the frames an mz_external_env describes must stack to the network's observation
static int ext_check_frames(mz_planner* p, const mz_external_env* x) {
    const mz_config& c = p->cfg;
    const int S = x->stack_history;
    if (S < 0 || x->frame_c < 1 || x->frame_h < 1 || x->frame_w < 1 || x->max_episode_steps < 0 || x->temp_switch_steps < 0)
        return fail(MZ_E_INVALID, "mz_external_env: stack_history >= 0, frame dimensions >= 1, max_episode_steps >= 0, temp_switch_steps >= 0");
    if (!x->is_obs_image && (x->frame_h != 1 || x->frame_w != 1))
        return fail(MZ_E_INVALID, "mz_external_env: vector frames are frame_c = D, frame_h = frame_w = 1");
    const long long FE = (long long)x->frame_c * x->frame_h * x->frame_w;
    const long long stacked = S == 0 ? FE : (x->is_obs_image ? (long long)S * (x->frame_c + 1) * x->frame_h * x->frame_w : (long long)S * (x->frame_c + 1));
    if (stacked != obs_dim(c))
        return fail(MZ_E_INVALID, "mz_external_env: the stacked observation has " + std::to_string(stacked) + " values, the network's (obs_c*obs_h*obs_w) " +
                                      std::to_string(obs_dim(c)));
    if (S == 0 && x->frame_u8) return fail(MZ_E_INVALID, "mz_external_env: frame_u8 needs stack_history > 0 (whole observations are float32)");
    return MZ_OK;
}

// ExtEnv's geometry and device buffers, and the pinned staging of every upload and download (after ext_free)
static int ext_alloc(mz_planner* p, const mz_external_env* x) {
    const mz_config& c = p->cfg;
    const int S = x->stack_history;
    const long long FE = (long long)x->frame_c * x->frame_h * x->frame_w;
    ExtEnv& X = p->ext;
    X.S = S; X.image = x->is_obs_image ? 1 : 0; X.C = x->frame_c; X.HW = x->frame_h * x->frame_w; X.FE = (int)FE; X.u8 = x->frame_u8 ? 1 : 0;
    X.temp_steps = x->temp_switch_steps > 0 ? x->temp_switch_steps : (c.num_actions <= 10 ? 6 : 30);
    p->ext_od = obs_dim(c);
    const size_t B = (size_t)c.num_envs, fbytes = (size_t)FE * (X.u8 ? 1 : 4);
    HIPCHK(hipMalloc(&X.frames, (B * fbytes + 15) / 16 * 16));  // (whole 16-byte runs: the device games' renderers store nothing narrower)
    if (S > 0) {
        HIPCHK(hipMalloc(&X.hist, B * S * fbytes));
        HIPCHK(hipMalloc(&X.hist_act, B * S * sizeof(int)));
        HIPCHK(hipMalloc(&X.head, 2 * B * sizeof(int)));
        HIPCHK(hipMemsetAsync(X.head, 0, 2 * B * sizeof(int), p->stream));
    }
    HIPCHK(hipMalloc(&X.reward, B * sizeof(float)));
    HIPCHK(hipMalloc(&X.done, B));
    HIPCHK(hipMalloc(&X.err, sizeof(int)));
    HIPCHK(hipHostMalloc(&p->h_ext_frames, B * fbytes, hipHostMallocDefault));
    HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&p->h_ext_mask), B * c.num_actions, hipHostMallocDefault));
    HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&p->h_ext_cur), B * sizeof(int), hipHostMallocDefault));
    HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&p->h_ext_opp), B * sizeof(int), hipHostMallocDefault));
    HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&p->h_ext_action), B * sizeof(int), hipHostMallocDefault));
    HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&p->h_ext_reward), B * sizeof(float), hipHostMallocDefault));
    HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&p->h_ext_done), B, hipHostMallocDefault));
    HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&p->h_ext_err), sizeof(int), hipHostMallocDefault));
    const int none = INT_MAX;
    HIPCHK(hipMemcpyAsync(X.err, &none, sizeof(int), hipMemcpyHostToDevice, p->stream));
    HIPCHK(hipStreamSynchronize(p->stream));
    return MZ_OK;
}

// The reset of both kinds that run on ExtEnv: host-stepped envs (`sname` "mz_external_env") and the device Catch env, which describes its
// frames with the same struct ("mz_catch_env": its refusals name that struct's record_format).
static int ext_reset(mz_planner* p, const mz_external_env* x, int env_kind, const std::string& sname) {
    HIPCHK(hipSetDevice(p->device));
    const mz_config& c = p->cfg;
    const int S = x->stack_history;
    int rc = ext_check_frames(p, x);
    if (rc) return rc;
    const long long FE = (long long)x->frame_c * x->frame_h * x->frame_w;
    const int fmt = p->has_replay ? p->replay.state_format : STATE_F32;
    if (fmt == STATE_FRAMES_U8) {
        if (S == 0 || !x->is_obs_image || !x->frame_u8)
            return fail(MZ_E_INVALID, "mz_replay_ring.state_format MZ_STATE_FRAMES_U8 needs stack_history > 0, is_obs_image and frame_u8 (float frames are not bytes)");
        if (c.num_actions > 256) return fail(MZ_E_INVALID, "mz_replay_ring.state_format MZ_STATE_FRAMES_U8 holds an action in one byte: num_actions > 256");
    }
    if (x->record_format != MZ_RECORD_F32 && x->record_format != MZ_RECORD_FRAMES_U8)
        return fail(MZ_E_INVALID, sname + ".record_format must be MZ_RECORD_F32 or MZ_RECORD_FRAMES_U8");
    const bool rec = x->record_format == MZ_RECORD_FRAMES_U8;
    if (rec) {
        if (S == 0 || !x->is_obs_image || !x->frame_u8)
            return fail(MZ_E_INVALID, sname + ".record_format MZ_RECORD_FRAMES_U8 needs stack_history > 0, is_obs_image and frame_u8 (a record is one uint8 frame)");
        if (c.num_actions > 256) return fail(MZ_E_INVALID, sname + ".record_format MZ_RECORD_FRAMES_U8 rebuilds one-byte actions: num_actions > 256");
        if (p->has_replay && fmt != STATE_FRAMES_U8)
            return fail(MZ_E_INVALID, sname + ".record_format MZ_RECORD_FRAMES_U8 feeds a replay of mz_replay_ring.state_format MZ_STATE_FRAMES_U8 only");
    }
    ext_free(p);
    p->arena_open = false;
    p->env_kind = env_kind;
    p->ext_pending = p->ext_broken = false;
    const size_t rec_stride = ((size_t)FE + 15) / 16 * 16;
    if (rec) ring_start(p, x->max_episode_steps, rec_stride, S);
    else ring_start(p, x->max_episode_steps);
    hipError_t e = env_alloc(p->env, ENV_EXTERNAL, c.num_envs, c.num_actions, obs_dim(c), p->ring_len, 3, 3, !rec);
    if (e != hipSuccess) return fail(MZ_E_HIP, std::string("env_alloc: ") + hipGetErrorString(e));
    if (rec) {
        RecRing& Q = p->rr;
        const size_t slots = (size_t)p->ring_len * c.num_envs;
        Q.stride = (int)rec_stride; Q.FE = (int)FE; Q.extra = S;
        p->rec_S = S;
        hipError_t r = hipMalloc(reinterpret_cast<void**>(&Q.frames), slots * rec_stride);
        if (r == hipSuccess) r = hipMalloc(reinterpret_cast<void**>(&Q.age), slots * sizeof(int));
        if (r == hipSuccess) r = hipMemsetAsync(Q.frames, 0, slots * rec_stride, p->stream);
        if (r == hipSuccess) r = hipMemsetAsync(Q.age, 0, slots * sizeof(int), p->stream);
        if (r != hipSuccess) {  // no half-built ring: the handle is left without an env, as before its first reset
            (void)hipGetLastError();
            ext_free(p);
            p->env_kind = MZ_ENV_NONE;
            return fail(MZ_E_HIP, std::string("compact record ring: ") + hipGetErrorString(r));
        }
    }
    rc = ext_alloc(p, x);
    if (rc) return rc;
    ExtEnv& X = p->ext;
    if (fmt != STATE_F32) {
        ReplayRing& R = p->replay;
        R.fS = S; R.fC = X.C; R.fHW = X.HW; R.fP = S * X.FE;
        R.row_bytes = fmt == STATE_I8 ? obs_dim(c) : (R.fP + S + 15) / 16 * 16;
        R.enc_err = nullptr;
        if (fmt == STATE_I8) {  // whole observations of any env: every emitted state is checked
            const int none = INT_MAX;
            HIPCHK(hipMalloc(&X.enc_err, sizeof(int)));
            R.enc_err = X.enc_err;
            HIPCHK(hipMemcpyAsync(X.enc_err, &none, sizeof(int), hipMemcpyHostToDevice, p->stream));
            HIPCHK(hipStreamSynchronize(p->stream));
        }
    }
    return MZ_OK;
}

extern "C" int mz_selfplay_reset_external(mz_planner* p, const mz_external_env* x) {
    if (!p || !x) return fail(MZ_E_INVALID, "null argument to mz_selfplay_reset_external");
    return ext_reset(p, x, MZ_ENV_EXTERNAL, "mz_external_env");
}

// The device work of an act, shared by the host-stepped path and Catch: observations from ext.frames into the search input and the record
// ring, the search (move_counter keys the Philox draws as in mz_selfplay_step), the move's action / pi / root value into the record slot.
static int ext_enqueue_act(mz_planner* p, const ExtLaunch& L) {
    const mz_config& c = p->cfg;
    const int OD = p->ext_od;
    const bool vec4 = (p->ext.S > 0 && p->ext.image && p->ext.HW % 4 == 0) || (p->ext.S == 0 && OD % 4 == 0);  // (four floats of one plane / run per group)
    const dim3 grid4((OD / 4 + 256 * EXT_ITER - 1) / (256 * EXT_ITER), c.num_envs), grid1((OD + 63) / 64, c.num_envs);
    if (p->rr.frames) {  // compact records: the same pass without the float32 record
        if (vec4) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ext_ingest<4, true>), grid4, dim3(256), 0, p->stream, L);
        else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ext_ingest<1, true>), grid1, dim3(64), 0, p->stream, L);
    } else if (vec4)
        hipLaunchKernelGGL(k_ext_ingest<4>, grid4, dim3(256), 0, p->stream, L);
    else
        hipLaunchKernelGGL(k_ext_ingest<1>, grid1, dim3(64), 0, p->stream, L);
    HIPCHK(hipGetLastError());
    int rc = launch_search(p, c.num_envs, 0, true, false, false);
    if (rc) return rc;
    hipLaunchKernelGGL(k_ext_record, dim3((c.num_envs * c.num_actions + 255) / 256), dim3(256), 0, p->stream, L);
    HIPCHK(hipGetLastError());
    return MZ_OK;
}

// The device work of a commit: ext.reward / ext.done into the record slot, step counts, counters, the record ring's capacity check.
static int ext_enqueue_commit(mz_planner* p, const ExtLaunch& L) {
    hipLaunchKernelGGL(k_ext_commit, dim3((p->cfg.num_envs + 255) / 256), dim3(256), 0, p->stream, L);
    HIPCHK(hipGetLastError());
    return MZ_OK;
}

extern "C" int mz_selfplay_external_act(mz_planner* p, const void* h_frames, const uint8_t* h_mask, const int32_t* h_cur, const int32_t* h_opp,
                                        double temperature, int32_t* h_action) {
    if (!p || !h_frames || !h_mask || !h_cur || !h_opp || !h_action) return fail(MZ_E_INVALID, "null argument to mz_selfplay_external_act");
    if (p->arena_open) return fail(MZ_E_STATE, "mz_selfplay_external_act during an arena: call mz_selfplay_reset_external first");
    if (p->env_kind != MZ_ENV_EXTERNAL) return fail(MZ_E_STATE, "call mz_selfplay_reset_external first");
    if (p->ext_broken) return fail(MZ_E_STATE, "a commit found an over-long trajectory or a state its replay format cannot hold: call mz_selfplay_reset_external");
    if (p->ext_pending) return fail(MZ_E_STATE, "mz_selfplay_external_act twice: commit the last act's outcome first");
    if (!p->committed) return fail(MZ_E_STATE, "weights not committed");
    HIPCHK(hipSetDevice(p->device));
    const mz_config& c = p->cfg;
    const size_t B = (size_t)c.num_envs, fbytes = B * p->ext.FE * (p->ext.u8 ? 1 : 4);
    // pinned staging: the copies below are true asynchronous DMA on the planner's stream
    std::memcpy(p->h_ext_frames, h_frames, fbytes);
    std::memcpy(p->h_ext_mask, h_mask, B * c.num_actions);
    std::memcpy(p->h_ext_cur, h_cur, B * sizeof(int));
    std::memcpy(p->h_ext_opp, h_opp, B * sizeof(int));
    HIPCHK(hipMemcpyAsync(p->ext.frames, p->h_ext_frames, fbytes, hipMemcpyHostToDevice, p->stream));
    HIPCHK(hipMemcpyAsync(p->d_mask, p->h_ext_mask, B * c.num_actions, hipMemcpyHostToDevice, p->stream));
    HIPCHK(hipMemcpyAsync(p->d_cur, p->h_ext_cur, B * sizeof(int), hipMemcpyHostToDevice, p->stream));
    HIPCHK(hipMemcpyAsync(p->d_opp, p->h_ext_opp, B * sizeof(int), hipMemcpyHostToDevice, p->stream));
    int rc = ext_enqueue_act(p, ext_launch(p, temperature));
    if (rc) return rc;
    int err = 0;
    HIPCHK(hipMemcpyAsync(p->h_ext_action, p->d_action, B * sizeof(int), hipMemcpyDeviceToHost, p->stream));
    HIPCHK(hipMemcpyAsync(&err, p->d_err, sizeof(int), hipMemcpyDeviceToHost, p->stream));
    HIPCHK(hipStreamSynchronize(p->stream));
    if (err) {
        HIPCHK(hipMemsetAsync(p->d_err, 0, sizeof(int), p->stream));
        HIPCHK(hipStreamSynchronize(p->stream));
        return fail(MZ_E_INVALID, "search kernel reported error " + std::to_string(err));
    }
    std::memcpy(h_action, p->h_ext_action, B * sizeof(int));
    p->ext_pending = true;
    return MZ_OK;
}

extern "C" int mz_selfplay_external_commit(mz_planner* p, const float* h_reward, const uint8_t* h_done) {
    if (!p || !h_reward || !h_done) return fail(MZ_E_INVALID, "null argument to mz_selfplay_external_commit");
    if (p->arena_open) return fail(MZ_E_STATE, "mz_selfplay_external_commit during an arena: call mz_selfplay_reset_external first");
    if (p->env_kind != MZ_ENV_EXTERNAL) return fail(MZ_E_STATE, "call mz_selfplay_reset_external first");
    if (p->ext_broken) return fail(MZ_E_STATE, "a commit found an over-long trajectory or a state its replay format cannot hold: call mz_selfplay_reset_external");
    if (!p->ext_pending) return fail(MZ_E_STATE, "mz_selfplay_external_commit without an mz_selfplay_external_act");
    HIPCHK(hipSetDevice(p->device));
    const mz_config& c = p->cfg;
    const size_t B = (size_t)c.num_envs;
    std::memcpy(p->h_ext_reward, h_reward, B * sizeof(float));
    std::memcpy(p->h_ext_done, h_done, B);
    HIPCHK(hipMemcpyAsync(p->ext.reward, p->h_ext_reward, B * sizeof(float), hipMemcpyHostToDevice, p->stream));
    HIPCHK(hipMemcpyAsync(p->ext.done, p->h_ext_done, B, hipMemcpyHostToDevice, p->stream));
    int crc = ext_enqueue_commit(p, ext_launch(p, 0.0));
    if (crc) return crc;
    p->ext_pending = false;
    if (p->has_replay) {  // the length check must pass before the epilogue may read the trajectories
        HIPCHK(hipMemcpyAsync(p->h_ext_err, p->ext.err, sizeof(int), hipMemcpyDeviceToHost, p->stream));
        HIPCHK(hipStreamSynchronize(p->stream));
        if (*p->h_ext_err != INT_MAX) {
            p->ext_broken = true;
            return fail(MZ_E_INVALID, "env " + std::to_string(*p->h_ext_err) + ": open trajectory of more than " + std::to_string(p->ring_len - p->rr.extra) +
                                          " moves outgrew the record ring (raise mz_external_env.max_episode_steps); no items written, reset next");
        }
    }
    const int rc = ring_finish_move(p);
    if (rc == MZ_OK && p->has_replay && p->replay.enc_err) {  // (the encoder has just seen the states this move emitted)
        HIPCHK(hipMemcpyAsync(p->h_ext_err, p->replay.enc_err, sizeof(int), hipMemcpyDeviceToHost, p->stream));
        HIPCHK(hipStreamSynchronize(p->stream));
        if (*p->h_ext_err != INT_MAX) {
            p->ext_broken = true;
            return fail(MZ_E_INVALID, "env " + std::to_string(*p->h_ext_err) + ": an observation holds a value that mz_replay_ring.state_format MZ_STATE_I8 "
                                          "cannot hold exactly; the replay count did not advance, reset next");
        }
    }
    return rc;
}

// ---------------------------------------------------------------------------------------------------------
// Device image games (mz_grid_game.h): the host-stepped path's device work around an env that lives on the device.  The host side is one
// set of templates over the game type G; a game adds its geometry check (its defaults and its refusals), its reset entry points (a null
// check, the arena's range checks of its start codes, one call) and its row in IMAGE_GAMES.
// ---------------------------------------------------------------------------------------------------------
template <class G>
static GameLaunch<G> game_launch(mz_planner* p) {
    GameLaunch<G> L{};
    L.g = std::get<G>(p->games); L.seed = p->cfg.seed;
    L.action = p->d_action; L.episode = p->env.episode; L.reward = p->ext.reward; L.done = p->ext.done;
    L.frames = static_cast<unsigned char*>(p->ext.frames); L.mask = p->d_mask; L.cur = p->d_cur; L.opp = p->d_opp;
    return L;
}

static dim3 per_env(mz_planner* p) { return dim3((p->cfg.num_envs + 255) / 256); }

template <class G>
static void game_render(mz_planner* p) {
    const GameLaunch<G> L = game_launch<G>(p);
    const size_t runs = ((size_t)L.g.B * L.g.FE + 15) / 16;
    hipLaunchKernelGGL(k_game_render<G>, dim3((unsigned)((runs + 255) / 256)), dim3(256), 0, p->stream, L);
}

// What every grid game asks of the planner's mz_config, for the reset `fn` of the game `name`
static int game_config_check(mz_planner* p, const std::string& fn, const char* name) {
    const mz_config& c = p->cfg;
    if (c.is_board_game) return fail(MZ_E_INVALID, fn + ": is_board_game must be 0 (" + name + " is a one-player game)");
    if (c.num_actions != 3) return fail(MZ_E_INVALID, fn + ": num_actions must be 3 (left, stay, right), not " + std::to_string(c.num_actions));
    if (c.obs_c < 2 || (c.obs_c & 1))
        return fail(MZ_E_INVALID, fn + ": obs_c must be 2 * stack_history (S one-channel frames and S action planes), not " + std::to_string(c.obs_c));
    return MZ_OK;
}

// A checked rows x cols grid on the planner's frame: the game's geometry (its state array comes from game_alloc), and the frames as an
// mz_external_env whose record ring holds an open trajectory of `longest` moves
static void game_frames(mz_planner* p, int rows, int cols, int longest, int record_format, GridGame& g, mz_external_env& x) {
    const mz_config& c = p->cfg;
    g.rows = rows; g.cols = cols; g.ch = c.obs_h / rows; g.cw = c.obs_w / cols; g.H = c.obs_h; g.W = c.obs_w; g.FE = c.obs_h * c.obs_w; g.B = c.num_envs;
    x = mz_external_env{};
    x.stack_history = c.obs_c / 2; x.is_obs_image = 1; x.frame_c = 1; x.frame_h = c.obs_h; x.frame_w = c.obs_w; x.frame_u8 = 1;
    x.max_episode_steps = longest;
    x.record_format = record_format;
}

// Catch's geometry off the planner's mz_config, for the reset `fn` (self-play or arena)
static int game_geometry(mz_planner* p, const mz_catch_env* env, const std::string& fn, Catch& g, mz_external_env& x) {
    const mz_config& c = p->cfg;
    const int rows = env->rows == 0 && env->cols == 0 ? 12 : env->rows, cols = env->rows == 0 && env->cols == 0 ? 12 : env->cols;
    int rc = game_config_check(p, fn, Catch::NAME);
    if (rc) return rc;
    if (rows < 2 || c.obs_h % rows != 0)
        return fail(MZ_E_INVALID, "mz_catch_env.rows must be >= 2 and divide obs_h = " + std::to_string(c.obs_h) + ", not " + std::to_string(rows));
    if (cols < 1 || c.obs_w % cols != 0)
        return fail(MZ_E_INVALID, "mz_catch_env.cols must be >= 1 and divide obs_w = " + std::to_string(c.obs_w) + ", not " + std::to_string(cols));
    game_frames(p, rows, cols, rows - 1, env->record_format, g, x);  // (rows - 1: an episode's length)
    return MZ_OK;
}

// Breakout's, with the defaults filled in
static int game_geometry(mz_planner* p, const mz_breakout_env* env, const std::string& fn, Breakout& g, mz_external_env& x) {
    const mz_config& c = p->cfg;
    mz_breakout_env v = *env;
    if (v.rows == 0 && v.cols == 0) v.rows = v.cols = 12;
    if (v.brick_rows == 0) v.brick_rows = 3;
    if (v.max_moves == 0) v.max_moves = 200;
    int rc = game_config_check(p, fn, Breakout::NAME);
    if (rc) return rc;
    if (v.brick_rows < 1 || v.brick_rows > 3) return fail(MZ_E_INVALID, "mz_breakout_env.brick_rows must be 1, 2 or 3, not " + std::to_string(v.brick_rows));
    if (v.max_moves < 1) return fail(MZ_E_INVALID, "mz_breakout_env.max_moves must be >= 1, not " + std::to_string(v.max_moves));
    if (v.cols > 32) return fail(MZ_E_INVALID, "mz_breakout_env.cols must be <= 32 (a brick row is one 32-bit mask), not " + std::to_string(v.cols));
    if (v.rows < v.brick_rows + 3 || c.obs_h % v.rows != 0)
        return fail(MZ_E_INVALID, "mz_breakout_env.rows must be >= brick_rows + 3 = " + std::to_string(v.brick_rows + 3) + " and divide obs_h = " +
                                      std::to_string(c.obs_h) + ", not " + std::to_string(v.rows));
    if (v.cols < 3 || c.obs_w % v.cols != 0)
        return fail(MZ_E_INVALID, "mz_breakout_env.cols must be >= 3 and divide obs_w = " + std::to_string(c.obs_w) + ", not " + std::to_string(v.cols));
    g.K = v.brick_rows; g.max_moves = v.max_moves;
    game_frames(p, v.rows, v.cols, v.max_moves, v.record_format, g, x);  // (max_moves: an episode's longest)
    return MZ_OK;
}

// the game's state array (after ext_free)
template <class G>
static int game_alloc(mz_planner* p, G g) {
    HIPCHK(hipMalloc(reinterpret_cast<void**>(&g.s), (size_t)G::FIELDS * g.B * sizeof(int)));
    std::get<G>(p->games) = g;
    return MZ_OK;
}

template <class G, class Env>
static int game_selfplay_reset(mz_planner* p, const Env* env, const std::string& fn) {
    G g{};
    mz_external_env x;
    int rc = game_geometry(p, env, fn, g, x);
    if (rc) return rc;
    if (p->has_replay && p->replay.state_format == STATE_I8)
        return fail(MZ_E_INVALID, std::string("mz_replay_ring.state_format: ") + G::NAME + " observations (" + G::OBS_VALUES +
                                      ") are not int8 values; MZ_STATE_F32 or MZ_STATE_FRAMES_U8");
    rc = ext_reset(p, &x, G::KIND, G::STRUCT);
    if (rc) return rc;
    rc = game_alloc(p, g);
    if (rc) return rc;
    hipLaunchKernelGGL(k_game_reset<G>, per_env(p), dim3(256), 0, p->stream, game_launch<G>(p));
    game_render<G>(p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(p->stream));
    return MZ_OK;
}

extern "C" int mz_selfplay_reset_catch(mz_planner* p, const mz_catch_env* env) {
    if (!p || !env) return fail(MZ_E_INVALID, "null argument to mz_selfplay_reset_catch");
    return game_selfplay_reset<Catch>(p, env, "mz_selfplay_reset_catch");
}

extern "C" int mz_selfplay_reset_breakout(mz_planner* p, const mz_breakout_env* env) {
    if (!p || !env) return fail(MZ_E_INVALID, "null argument to mz_selfplay_reset_breakout");
    return game_selfplay_reset<Breakout>(p, env, "mz_selfplay_reset_breakout");
}

// ---------------------------------------------------------------------------------------------------------
// Device image games behind one table: what differs between them is the env's step (self-play: with restart; arena: with the ply record
// and the freeze) and its renderer, all instances of mz_grid_game.h's kernels.  A game is one header and one row here.
// ---------------------------------------------------------------------------------------------------------
struct ImageGame {
    int env_kind;
    const char* reset_name;                                   // the self-play reset, named in refusals
    void (*step)(mz_planner*);                                // self-play: ext.reward / ext.done, restart on done
    void (*render)(mz_planner*);                              // every env's next frame into ext.frames
    void (*arena_step)(mz_planner*, const ImgArenaLaunch&);   // arena: ply record, step, outcome, freeze
};

template <class G>
static constexpr ImageGame image_game_row(const char* reset_name) {
    return {G::KIND, reset_name,
            [](mz_planner* p) { hipLaunchKernelGGL(k_game_step<G>, per_env(p), dim3(256), 0, p->stream, game_launch<G>(p)); },
            game_render<G>,
            [](mz_planner* p, const ImgArenaLaunch& R) {
                hipLaunchKernelGGL(k_game_arena_step<G>, per_env(p), dim3(256), 0, p->stream, R, std::get<G>(p->games));
            }};
}

static const ImageGame IMAGE_GAMES[] = {
    image_game_row<Catch>("mz_selfplay_reset_catch"),
    image_game_row<Breakout>("mz_selfplay_reset_breakout"),
};

static const ImageGame* image_game(int env_kind) {
    for (const ImageGame& g : IMAGE_GAMES)
        if (g.env_kind == env_kind) return &g;
    return nullptr;
}

// mz_selfplay_step on a device image game: per move the act's device work, the env's step and next frame, the commit's device work, the
// epilogue.  Nothing is copied and nothing waits inside the loop.  What the host-stepped path reads back per commit is read back once per
// call, and only with a replay attached (one synchronisation at the end of the call): the record ring's capacity check -- a guard here, the
// reset sized the ring for the game's longest episode, so the moves of this call already ran their epilogues when it is read -- and the
// search kernels' error word.
static int image_game_moves(mz_planner* p, const ImageGame& g, double temperature, int n_moves) {
    if (p->ext_broken)
        return fail(MZ_E_STATE, std::string("an earlier mz_selfplay_step found an over-long trajectory or a search error: call ") + g.reset_name);
    for (int m = 0; m < n_moves; m++) {
        const ExtLaunch L = ext_launch(p, temperature);
        int rc = ext_enqueue_act(p, L);
        if (rc) return rc;
        g.step(p);
        g.render(p);
        rc = ext_enqueue_commit(p, L);
        if (rc) return rc;
        rc = ring_finish_move(p);
        if (rc) return rc;
    }
    if (p->has_replay) {
        int err = 0;
        HIPCHK(hipMemcpyAsync(p->h_ext_err, p->ext.err, sizeof(int), hipMemcpyDeviceToHost, p->stream));
        HIPCHK(hipMemcpyAsync(&err, p->d_err, sizeof(int), hipMemcpyDeviceToHost, p->stream));
        HIPCHK(hipStreamSynchronize(p->stream));
        if (*p->h_ext_err != INT_MAX) {
            p->ext_broken = true;
            return fail(MZ_E_INVALID, "env " + std::to_string(*p->h_ext_err) + ": open trajectory of more than " + std::to_string(p->ring_len - p->rr.extra) +
                                          " moves outgrew the record ring; reset next");
        }
        if (err) {
            HIPCHK(hipMemsetAsync(p->d_err, 0, sizeof(int), p->stream));
            HIPCHK(hipStreamSynchronize(p->stream));
            p->ext_broken = true;
            return fail(MZ_E_INVALID, "search kernel reported error " + std::to_string(err));
        }
    }
    return MZ_OK;
}

extern "C" int mz_selfplay_attach_replay(mz_planner* p, const mz_replay_ring* ring) {
    if (!p) return fail(MZ_E_INVALID, "null planner");
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(hipStreamSynchronize(p->stream));  // attach / detach drain the planner: after a detach the caller owns counter and priorities again
    if (!ring) {
        p->has_replay = false;
        return MZ_OK;
    }
    const mz_config& c = p->cfg;
    if (ring->capacity < 1 || !ring->state || !ring->action || !ring->pi_prob || !ring->value || !ring->reward || !ring->priority || !ring->num_added)
        return fail(MZ_E_INVALID, "mz_replay_ring: capacity and every array but `origin` are required");
    if (ring->unroll_steps < 1 || ring->td_steps < 0 || ring->td_steps > 32 || ring->acc_seq_length < 1)
        return fail(MZ_E_INVALID, "mz_replay_ring: unroll_steps >= 1, 0 <= td_steps <= 32, acc_seq_length >= 1");
    {   // the epilogue kernels write through these pointers: every one must be memory of the planner's GPU (a host-resident replay would fault)
        const void* ptrs[8] = {ring->state, ring->action, ring->pi_prob, ring->value, ring->reward, ring->priority, ring->num_added, ring->origin};
        static const char* names[8] = {"state", "action", "pi_prob", "value", "reward", "priority", "num_added", "origin"};
        for (int i = 0; i < 8; i++) {
            if (!ptrs[i]) continue;  // (origin is optional)
            hipPointerAttribute_t at{};
            const hipError_t e = hipPointerGetAttributes(&at, ptrs[i]);
            if (e != hipSuccess || at.type != hipMemoryTypeDevice || at.device != p->device) {
                (void)hipGetLastError();
                return fail(MZ_E_INVALID, std::string("mz_replay_ring.") + names[i] + " is not memory of the planner's GPU");
            }
        }
    }
    if (ring->state_format != MZ_STATE_F32 && ring->state_format != MZ_STATE_I8 && ring->state_format != MZ_STATE_FRAMES_U8)
        return fail(MZ_E_INVALID, "mz_replay_ring.state_format must be MZ_STATE_F32, MZ_STATE_I8 or MZ_STATE_FRAMES_U8");
    ReplayRing& R = p->replay;
    R.state_format = ring->state_format; R.row_bytes = 0; R.fS = R.fC = R.fHW = R.fP = 0; R.enc_err = nullptr;
    R.capacity = ring->capacity; R.state = ring->state; R.action = reinterpret_cast<signed char*>(ring->action); R.action16 = c.num_actions > 128 ? 1 : 0; R.pi_prob = ring->pi_prob;
    R.value = ring->value; R.reward = ring->reward; R.priority = ring->priority; R.num_added = reinterpret_cast<long long*>(ring->num_added);
    R.origin = ring->origin; R.acc = ring->acc_seq_length; R.K = ring->unroll_steps; R.td = ring->td_steps; R.board = c.is_board_game;
    for (int i = 0; i <= R.td; i++) R.pw[i] = std::pow(c.discount, (double)i);  // Python's discount ** i (pipeline.py:663-666)
    // the device-owned write cursor starts at the caller's count; the caller's counter is from now on only PUBLISHED to
    if (!p->d_epi_ctr) HIPCHK(hipMalloc(&p->d_epi_ctr, 2 * sizeof(long long)));
    HIPCHK(hipMemsetAsync(p->d_epi_ctr, 0, 2 * sizeof(long long), p->stream));
    HIPCHK(hipMemcpyAsync(p->d_epi_ctr, R.num_added, sizeof(long long), hipMemcpyDeviceToDevice, p->stream));
    HIPCHK(hipStreamSynchronize(p->stream));
    R.ctr = p->d_epi_ctr;
    if (!p->d_epi_off) HIPCHK(hipMalloc(&p->d_epi_off, (size_t)c.num_envs * sizeof(int)));
    R.off = p->d_epi_off;
    p->has_replay = true;
    p->arena_open = false;
    p->env_kind = MZ_ENV_NONE;  // the record ring must be re-sized: mz_selfplay_reset next
    return MZ_OK;
}

extern "C" int mz_selfplay_read(mz_planner* p, int32_t n_moves, float* h_obs, int32_t* h_action, float* h_reward, double* h_pi,
                                double* h_root, int32_t* h_player, uint8_t* h_done) {
    if (!p || n_moves < 1 || n_moves > p->ring_count) return fail(MZ_E_INVALID, "n_moves exceeds the recorded history");
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(hipStreamSynchronize(p->stream));
    const size_t B = (size_t)p->cfg.num_envs, A = (size_t)p->cfg.num_actions, D = (size_t)obs_dim(p->cfg);
    // the ring is slot-major, so the last n_moves records are at most two contiguous slot ranges per field: 7 (or 14)
    // copies per call, not 7 per move
    const int first = ((p->ring_pos - n_moves) % p->ring_len + p->ring_len) % p->ring_len;
    const int n1 = n_moves < p->ring_len - first ? n_moves : p->ring_len - first;  // moves before the ring wraps
    if (h_obs && p->rr.frames) {
        // compact records: the oldest requested move's window reaches back S more moves (fewer at the start of the run), and an act
        // that waits for its commit has already written its frame over the oldest slot of a full ring
        const long long before = p->selfplay_moves - n_moves;
        const int back = before < p->rec_S ? (int)before : p->rec_S;
        const int held = p->ring_count - (p->ext_pending && p->ring_count == p->ring_len ? 1 : 0);
        if (n_moves + back > held)
            return fail(MZ_E_INVALID, "mz_external_env.record_format MZ_RECORD_FRAMES_U8: the record ring no longer holds the " + std::to_string(back) +
                                          " moves before the oldest requested one that its observation is rebuilt from (read fewer moves, or without h_obs)");
        if (!p->d_rec_stage) HIPCHK(hipMalloc(reinterpret_cast<void**>(&p->d_rec_stage), B * D * sizeof(float)));
        ExtLaunch L = ext_launch(p, 0.0);
        L.obs = p->d_rec_stage;
        const int OD = p->ext_od;
        for (int i = 0; i < n_moves; i++) {  // move by move through the staging buffer, in stream order
            L.slot = (first + i) % p->ring_len;
            if (p->ext.HW % 4 == 0) hipLaunchKernelGGL(k_rec_decode<4>, dim3((OD / 4 + 256 * EXT_ITER - 1) / (256 * EXT_ITER), (unsigned)B), dim3(256), 0, p->stream, L);
            else hipLaunchKernelGGL(k_rec_decode<1>, dim3((OD + 63) / 64, (unsigned)B), dim3(64), 0, p->stream, L);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(h_obs + (size_t)i * B * D, p->d_rec_stage, B * D * sizeof(float), hipMemcpyDeviceToHost, p->stream));
        }
        h_obs = nullptr;  // (done; the other fields as ever)
    }
    for (int part = 0; part < 2; part++) {
        const size_t slot = part == 0 ? (size_t)first : 0, cnt = part == 0 ? (size_t)n1 : (size_t)(n_moves - n1), done_moves = part == 0 ? 0 : (size_t)n1;
        if (cnt == 0) continue;
        if (h_obs) HIPCHK(hipMemcpyAsync(h_obs + done_moves * B * D, p->env.r_obs + slot * B * D, cnt * B * D * sizeof(float), hipMemcpyDeviceToHost, p->stream));
        if (h_action) HIPCHK(hipMemcpyAsync(h_action + done_moves * B, p->env.r_action + slot * B, cnt * B * sizeof(int), hipMemcpyDeviceToHost, p->stream));
        if (h_reward) HIPCHK(hipMemcpyAsync(h_reward + done_moves * B, p->env.r_reward + slot * B, cnt * B * sizeof(float), hipMemcpyDeviceToHost, p->stream));
        if (h_pi) HIPCHK(hipMemcpyAsync(h_pi + done_moves * B * A, p->env.r_pi + slot * B * A, cnt * B * A * sizeof(double), hipMemcpyDeviceToHost, p->stream));
        if (h_root) HIPCHK(hipMemcpyAsync(h_root + done_moves * B, p->env.r_root + slot * B, cnt * B * sizeof(double), hipMemcpyDeviceToHost, p->stream));
        if (h_player) HIPCHK(hipMemcpyAsync(h_player + done_moves * B, p->env.r_player + slot * B, cnt * B * sizeof(int), hipMemcpyDeviceToHost, p->stream));
        if (h_done) HIPCHK(hipMemcpyAsync(h_done + done_moves * B, p->env.r_done + slot * B, cnt * B, hipMemcpyDeviceToHost, p->stream));
    }
    HIPCHK(hipStreamSynchronize(p->stream));
    return MZ_OK;
}

extern "C" int mz_selfplay_record_info(mz_planner* p, int64_t out[4]) {
    if (!p || !out) return fail(MZ_E_INVALID, "null argument");
    if (p->env_kind == MZ_ENV_NONE || p->arena_open) return fail(MZ_E_STATE, "call mz_selfplay_reset first");
    const int64_t B = p->cfg.num_envs, A = p->cfg.num_actions, D = obs_dim(p->cfg);
    const bool rec = p->rr.frames != nullptr;
    out[0] = rec ? MZ_RECORD_FRAMES_U8 : MZ_RECORD_F32;
    out[1] = p->ring_len;
    out[2] = rec ? B * p->rr.stride : B * D * (int64_t)sizeof(float);
    // r_action, r_reward, r_pi, r_root, r_player, r_done (EnvState) and the compact ring's step counts
    out[3] = out[1] * (out[2] + B * (int64_t)(sizeof(int) + sizeof(float) + A * sizeof(double) + sizeof(double) + sizeof(int) + 1 + (rec ? sizeof(int) : 0)));
    return MZ_OK;
}

extern "C" int mz_selfplay_counters(mz_planner* p, int64_t out[4]) {
    if (!p || !out) return fail(MZ_E_INVALID, "null argument");
    if (p->env_kind == MZ_ENV_NONE || p->arena_open) return fail(MZ_E_STATE, "call mz_selfplay_reset first");
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(hipStreamSynchronize(p->stream));
    unsigned long long c[4];
    HIPCHK(hipMemcpy(c, p->env.counters, sizeof(c), hipMemcpyDeviceToHost));
    for (int i = 0; i < 4; i++) out[i] = (int64_t)c[i];
    return MZ_OK;
}

// ---------------------------------------------------------------------------------------------------------
// arena: evaluation matches in lock-step (mz_arena.h)
// ---------------------------------------------------------------------------------------------------------
static bool arena_same_config(const mz_config& a, const mz_config& b) {
    mz_config x = a, y = b;
    x.seed = y.seed = 0;
    return x.net_kind == y.net_kind && x.obs_c == y.obs_c && x.obs_h == y.obs_h && x.obs_w == y.obs_w && x.num_actions == y.num_actions &&
           x.num_planes == y.num_planes && x.hidden_dim == y.hidden_dim && x.num_res_blocks == y.num_res_blocks &&
           x.value_support_size == y.value_support_size && x.reward_support_size == y.reward_support_size &&
           x.num_simulations == y.num_simulations && x.discount == y.discount && x.pb_c_base == y.pb_c_base && x.pb_c_init == y.pb_c_init &&
           x.is_board_game == y.is_board_game && x.has_known_bounds == y.has_known_bounds && x.known_bounds_min == y.known_bounds_min &&
           x.known_bounds_max == y.known_bounds_max && x.root_dirichlet_alpha == y.root_dirichlet_alpha &&
           x.root_exploration_eps == y.root_exploration_eps && x.num_envs == y.num_envs && x.max_ties == y.max_ties &&
           x.legacy_scalar_promotion == y.legacy_scalar_promotion && x.conv_precision == y.conv_precision;
}

static ArenaLaunch arena_launch(mz_planner* p) {
    const mz_config& c = p->cfg;
    ArenaLaunch R{};
    R.L.env = p->env; R.L.B = c.num_envs; R.L.seed = c.seed; R.L.sims = c.num_simulations;
    R.L.obs = p->arena.obs; R.L.mask = p->arena.mask; R.L.cur = p->arena.cur; R.L.opp = p->arena.opp;
    R.a = p->arena;
    R.ply = p->arena_ply;
    return R;
}

// a searched run: staged into, and read back from, the root buffers of the planner `s` that searches it
static void arena_seg_searched(ArenaSeg& g, mz_planner* s) {
    g.obs = s->d_obs; g.mask = s->d_mask; g.cur = s->d_cur; g.opp = s->d_opp; g.temp = s->d_temp;
    g.action = s->d_action; g.pi = s->d_pi; g.root = s->d_root;
}

// what every arena reset on the lock-step board / CartPole arena checks after its env's own geometry: the sides, the borrowed opponent,
// committed weights; then it drains the stream and makes the events that order the two planners' streams
static int arena_check_sides(mz_planner* p, bool two, int opponent_kind, mz_planner* q, int opening_plies, bool init_refused) {
    const mz_config& c = p->cfg;
    if (opponent_kind != MZ_ARENA_NONE && opponent_kind != MZ_ARENA_RANDOM && opponent_kind != MZ_ARENA_PLANNER) return fail(MZ_E_INVALID, "unknown opponent kind");
    if (two != (opponent_kind != MZ_ARENA_NONE)) return fail(MZ_E_INVALID, "two-player envs need an opponent (MZ_ARENA_RANDOM / MZ_ARENA_PLANNER), one-player envs MZ_ARENA_NONE");
    if (two && (c.num_envs & 1)) return fail(MZ_E_INVALID, "two-player arenas need an even num_envs (env i and i + num_envs / 2 are a pair)");
    if (opening_plies < 0) return fail(MZ_E_INVALID, "opening_plies must be >= 0");
    if (init_refused) return fail(MZ_E_INVALID, "only the CartPole env takes an initial state");
    if (opponent_kind == MZ_ARENA_PLANNER) {
        if (!q || q == p) return fail(MZ_E_INVALID, "MZ_ARENA_PLANNER needs a second planner");
        if (q->device != p->device) return fail(MZ_E_INVALID, "the opponent planner must be on the challenger's device");
        if (!arena_same_config(p->cfg, q->cfg)) return fail(MZ_E_INVALID, "the opponent planner's mz_config must equal the challenger's (apart from the seed)");
        if (p->conv && p->cnet.tower_split != q->cnet.tower_split) return fail(MZ_E_INVALID, "the opponent planner's tower_precision must equal the challenger's");
        if (!q->committed) return fail(MZ_E_STATE, "the opponent planner's weights are not committed");
    } else if (q) {
        return fail(MZ_E_INVALID, "an opponent planner is given but the opponent kind is not MZ_ARENA_PLANNER");
    }
    if (!p->committed) return fail(MZ_E_STATE, "weights not committed");
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(hipStreamSynchronize(p->stream));
    if (!p->ev_arena_pre) {
        HIPCHK(hipEventCreateWithFlags(&p->ev_arena_pre, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&p->ev_arena_q, hipEventDisableTiming));
    }
    return MZ_OK;
}

extern "C" int mz_arena_reset(mz_planner* p, int32_t env_kind, int32_t opponent_kind, mz_planner* q, int32_t opening_plies, const double* h_init_state) {
    if (!p) return fail(MZ_E_INVALID, "null planner");
    const mz_config& c = p->cfg;
    int board_n = 3, num_to_win = 3;
    if (env_kind == MZ_ENV_CARTPOLE) {
        if (c.num_actions != 2 || obs_dim(c) != 20) return fail(MZ_E_INVALID, "CartPole env needs num_actions == 2 and a (4,5) observation");
    } else if (env_kind == MZ_ENV_TICTACTOE) {
        if (c.num_actions != 10 || obs_dim(c) != 81) return fail(MZ_E_INVALID, "TicTacToe env needs num_actions == 10 and a (9,3,3) observation");
    } else if (env_kind == MZ_ENV_GOMOKU) {
        if (c.net_kind != MZ_NET_BOARD || c.obs_c != 9 || c.obs_h != c.obs_w || c.num_actions != c.obs_h * c.obs_w + 1 || c.obs_h < 5)
            return fail(MZ_E_INVALID, "Gomoku env needs a board net with a (9,N,N) observation, N >= 5, and num_actions == N*N + 1");
        board_n = c.obs_h;
        num_to_win = 5;
    } else if (env_kind == MZ_ENV_CATCH) {
        return fail(MZ_E_INVALID, "mz_arena_reset: MZ_ENV_CATCH has its own arena reset: mz_arena_reset_catch");
    } else if (env_kind == MZ_ENV_BREAKOUT) {
        return fail(MZ_E_INVALID, "mz_arena_reset: MZ_ENV_BREAKOUT has its own arena reset: mz_arena_reset_breakout");
    } else if (env_kind == MZ_ENV_EXTERNAL) {
        return fail(MZ_E_INVALID, "mz_arena_reset: MZ_ENV_EXTERNAL has its own arena reset: mz_arena_reset_external");
    } else if (env_kind == MZ_ENV_CONNECT4) {
        return fail(MZ_E_INVALID, "mz_arena_reset: MZ_ENV_CONNECT4 has its own arena reset: mz_arena_reset_connect4");
    } else if (env_kind == MZ_ENV_OTHELLO) {
        return fail(MZ_E_INVALID, "mz_arena_reset: MZ_ENV_OTHELLO has its own arena reset: mz_arena_reset_othello");
    } else if (env_kind == MZ_ENV_GO) {
        return fail(MZ_E_INVALID, "mz_arena_reset: MZ_ENV_GO has its own arena reset: mz_arena_reset_go");
    } else {
        return fail(MZ_E_INVALID, "the arena plays the device envs CartPole, TicTacToe and Gomoku (not the synthetic kind)");
    }
    const bool two = env_kind != MZ_ENV_CARTPOLE;
    int rc = arena_check_sides(p, two, opponent_kind, q, opening_plies, h_init_state && env_kind != MZ_ENV_CARTPOLE);
    if (rc) return rc;
    p->env_kind = env_kind;
    ext_free(p);  // (the arena keeps its own one-ply float32 record, ArenaState::r_obs: a compact self-play ring ends here)
    p->ring_len = 1; p->ring_pos = 0; p->ring_count = 0;  // no self-play records in this mode (mz_selfplay_read: MZ_E_INVALID)
    p->selfplay_moves = 0;
    hipError_t e = env_alloc(p->env, env_kind, c.num_envs, c.num_actions, obs_dim(c), 1, board_n, num_to_win);
    if (e != hipSuccess) return fail(MZ_E_HIP, std::string("env_alloc: ") + hipGetErrorString(e));
    e = arena_alloc(p->arena, c.num_envs, c.num_actions, obs_dim(c));
    if (e != hipSuccess) return fail(MZ_E_HIP, std::string("arena_alloc: ") + hipGetErrorString(e));
    p->arena.half = two ? c.num_envs / 2 : 0;
    p->arena.opponent = opponent_kind;
    p->arena.opening_plies = opening_plies;
    p->arena_q = opponent_kind == MZ_ARENA_PLANNER ? q : nullptr;
    p->arena_ply = 0;
    p->arena_img = 0;
    if (h_init_state) HIPCHK(hipMemcpyAsync(p->env.init_state, h_init_state, (size_t)c.num_envs * 4 * sizeof(double), hipMemcpyHostToDevice, p->stream));
    ArenaLaunch R = arena_launch(p);
    R.L.use_init = h_init_state != nullptr;
    hipLaunchKernelGGL(k_arena_reset, dim3((c.num_envs + 255) / 256), dim3(256), 0, p->stream, R);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(p->stream));
    p->arena_open = true;
    return MZ_OK;
}

// Connect Four in the two-player arena: mz_arena_reset's states and tally around mz_connect4.h's reset, pick and step
extern "C" int mz_arena_reset_connect4(mz_planner* p, const mz_connect4_env* env, int32_t opponent_kind, mz_planner* q, int32_t opening_plies) {
    if (!p || !env) return fail(MZ_E_INVALID, "null argument to mz_arena_reset_connect4");
    const mz_config& c = p->cfg;
    int rc = c4_check(p, env, "mz_arena_reset_connect4");
    if (rc) return rc;
    rc = arena_check_sides(p, true, opponent_kind, q, opening_plies, false);
    if (rc) return rc;
    p->env_kind = MZ_ENV_CONNECT4;
    ext_free(p);
    p->ring_len = 1; p->ring_pos = 0; p->ring_count = 0;  // no self-play records in this mode (mz_selfplay_read: MZ_E_INVALID)
    p->selfplay_moves = 0;
    hipError_t e = env_alloc(p->env, ENV_CONNECT4, c.num_envs, c.num_actions, obs_dim(c), 1, c.obs_w, env->num_to_win, true, c.obs_h * c.obs_w);
    if (e != hipSuccess) return fail(MZ_E_HIP, std::string("env_alloc: ") + hipGetErrorString(e));
    e = arena_alloc(p->arena, c.num_envs, c.num_actions, obs_dim(c));
    if (e != hipSuccess) return fail(MZ_E_HIP, std::string("arena_alloc: ") + hipGetErrorString(e));
    p->arena.half = c.num_envs / 2;
    p->arena.opponent = opponent_kind;
    p->arena.opening_plies = opening_plies;
    p->arena_q = opponent_kind == MZ_ARENA_PLANNER ? q : nullptr;
    p->arena_ply = 0;
    p->arena_img = 0;
    C4Arena Q{};
    Q.R = arena_launch(p); Q.rows = c.obs_h; Q.cols = c.obs_w;
    hipLaunchKernelGGL(k_c4_arena_reset, dim3((c.num_envs + 255) / 256), dim3(256), 0, p->stream, Q);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(p->stream));
    p->arena_open = true;
    return MZ_OK;
}

// Othello in the two-player arena: mz_arena_reset's states and tally around mz_othello.h's reset, pick and step
extern "C" int mz_arena_reset_othello(mz_planner* p, const mz_othello_env* env, int32_t opponent_kind, mz_planner* q, int32_t opening_plies) {
    if (!p || !env) return fail(MZ_E_INVALID, "null argument to mz_arena_reset_othello");
    const mz_config& c = p->cfg;
    int rc = oth_check(p, env, "mz_arena_reset_othello");
    if (rc) return rc;
    rc = arena_check_sides(p, true, opponent_kind, q, opening_plies, false);
    if (rc) return rc;
    p->env_kind = MZ_ENV_OTHELLO;
    ext_free(p);
    p->ring_len = 1; p->ring_pos = 0; p->ring_count = 0;  // no self-play records in this mode (mz_selfplay_read: MZ_E_INVALID)
    p->selfplay_moves = 0;
    hipError_t e = env_alloc(p->env, ENV_OTHELLO, c.num_envs, c.num_actions, obs_dim(c), 1, c.obs_w, 0, true, c.obs_h * c.obs_w);
    if (e != hipSuccess) return fail(MZ_E_HIP, std::string("env_alloc: ") + hipGetErrorString(e));
    e = arena_alloc(p->arena, c.num_envs, c.num_actions, obs_dim(c));
    if (e != hipSuccess) return fail(MZ_E_HIP, std::string("arena_alloc: ") + hipGetErrorString(e));
    p->arena.half = c.num_envs / 2;
    p->arena.opponent = opponent_kind;
    p->arena.opening_plies = opening_plies;
    p->arena_q = opponent_kind == MZ_ARENA_PLANNER ? q : nullptr;
    p->arena_ply = 0;
    p->arena_img = 0;
    OthArena Q{};
    Q.R = arena_launch(p); Q.rows = c.obs_h; Q.cols = c.obs_w;
    hipLaunchKernelGGL(k_oth_arena_reset, dim3((c.num_envs + 255) / 256), dim3(256), 0, p->stream, Q);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(p->stream));
    p->arena_open = true;
    return MZ_OK;
}

// Go in the two-player arena: mz_arena_reset's states and tally around mz_go.h's reset, pick and step
extern "C" int mz_arena_reset_go(mz_planner* p, const mz_go_env* env, int32_t opponent_kind, mz_planner* q, int32_t opening_plies) {
    if (!p || !env) return fail(MZ_E_INVALID, "null argument to mz_arena_reset_go");
    const mz_config& c = p->cfg;
    HIPCHK(hipSetDevice(p->device));
    int rc = go_check(p, env, "mz_arena_reset_go");
    if (rc) return rc;
    rc = arena_check_sides(p, true, opponent_kind, q, opening_plies, false);
    if (rc) return rc;
    rc = go_apply(p, env);
    if (rc) return rc;
    p->env_kind = MZ_ENV_GO;
    ext_free(p);
    p->ring_len = 1; p->ring_pos = 0; p->ring_count = 0;  // no self-play records in this mode (mz_selfplay_read: MZ_E_INVALID)
    p->selfplay_moves = 0;
    hipError_t e = env_alloc(p->env, ENV_GO, c.num_envs, c.num_actions, obs_dim(c), 1, c.obs_w, 0, true, c.obs_h * c.obs_w);
    if (e != hipSuccess) return fail(MZ_E_HIP, std::string("env_alloc: ") + hipGetErrorString(e));
    e = arena_alloc(p->arena, c.num_envs, c.num_actions, obs_dim(c));
    if (e != hipSuccess) return fail(MZ_E_HIP, std::string("arena_alloc: ") + hipGetErrorString(e));
    p->arena.half = c.num_envs / 2;
    p->arena.opponent = opponent_kind;
    p->arena.opening_plies = opening_plies;
    p->arena_q = opponent_kind == MZ_ARENA_PLANNER ? q : nullptr;
    p->arena_ply = 0;
    p->arena_img = 0;
    GoArena Q{};
    Q.R = arena_launch(p); Q.G = p->go;
    hipLaunchKernelGGL(k_go_arena_reset, dim3(c.num_envs), dim3(go_block(c.obs_h * c.obs_w)), 0, p->stream, Q);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(p->stream));
    p->arena_open = true;
    return MZ_OK;
}

extern "C" int mz_arena_step(mz_planner* p, int32_t n_plies) {
    if (!p || n_plies < 1) return fail(MZ_E_INVALID, "bad argument to mz_arena_step");
    if (!p->arena_open) return fail(MZ_E_STATE, "call mz_arena_reset first");
    if (p->arena_img == IMGARENA_EXTERNAL) return fail(MZ_E_STATE, "mz_arena_step on a host-stepped arena: use mz_arena_external_act / _commit");
    mz_planner* q = p->arena_q;
    if (!p->committed || (q && !q->committed)) return fail(MZ_E_STATE, "weights not committed");
    HIPCHK(hipSetDevice(p->device));
    if (p->arena_img) return image_game_plies(p, *image_game(p->env_kind), n_plies);  // (a device image game: the host-stepped arena left above)
    const mz_config& c = p->cfg;
    const int B = c.num_envs, half = p->arena.half;
    const dim3 waves((B + 3) / 4), block(256);
    const bool c4 = p->env_kind == MZ_ENV_CONNECT4, oth = p->env_kind == MZ_ENV_OTHELLO, go = p->env_kind == MZ_ENV_GO;
    for (int m = 0; m < n_plies; m++) {
        ArenaLaunch R = arena_launch(p);
        const int t = p->arena_ply;
        const bool opening = t < p->arena.opening_plies;
        // black moves at even plies; the challenger is black in the lower half of the envs and white in the upper half
        const int other = p->arena.opponent == MZ_ARENA_RANDOM ? SIDE_RANDOM : SIDE_OPPONENT;
        if (half) {
            R.nseg = 2;
            R.seg[0].lo = 0; R.seg[0].n = half; R.seg[0].side = opening ? SIDE_OPENING : ((t & 1) ? other : SIDE_CHALLENGER);
            R.seg[1].lo = half; R.seg[1].n = half; R.seg[1].side = opening ? SIDE_OPENING : ((t & 1) ? SIDE_CHALLENGER : other);
        } else {
            R.nseg = 1;
            R.seg[0].lo = 0; R.seg[0].n = B; R.seg[0].side = opening ? SIDE_OPENING : SIDE_CHALLENGER;
        }
        bool picks = false;
        int n_p = 0, n_q = 0;
        for (int k = 0; k < R.nseg; k++) {
            if (R.seg[k].side == SIDE_CHALLENGER) { arena_seg_searched(R.seg[k], p); n_p = R.seg[k].n; }
            else if (R.seg[k].side == SIDE_OPPONENT) { arena_seg_searched(R.seg[k], q); n_q = R.seg[k].n; }
            else picks = true;
        }
        const size_t work = (size_t)B * obs_dim(c) / 4 + 1;
        const int pre_blocks = (int)((work + 255) / 256 < 1024 ? (work + 255) / 256 : 1024);
        hipLaunchKernelGGL(k_arena_pre, dim3(pre_blocks), block, 0, p->stream, R);
        C4Arena Q{};  // (Connect Four: its own pick -- columns only -- and step, 16 lanes per env)
        Q.R = R; Q.rows = c.obs_h; Q.cols = c.obs_w;
        OthArena O{};  // (Othello likewise: placements or the pass, never resign)
        O.R = R; O.rows = c.obs_h; O.cols = c.obs_w;
        GoArena G{};  // (Go: placements and the pass, never resign; one workgroup per env)
        G.R = R; G.G = p->go;
        if (picks && c4) hipLaunchKernelGGL(k_c4_arena_pick, dim3((B + 255) / 256), block, 0, p->stream, Q);
        else if (picks && oth) hipLaunchKernelGGL(k_oth_arena_pick, dim3((B + 255) / 256), block, 0, p->stream, O);
        else if (picks && go) hipLaunchKernelGGL(k_go_arena_pick, dim3((B + 255) / 256), block, 0, p->stream, G);
        else if (picks) hipLaunchKernelGGL(k_arena_pick, waves, block, 0, p->stream, R);
        HIPCHK(hipGetLastError());
        if (n_q) {  // the opponent's half on its own stream, beside the challenger's
            HIPCHK(hipEventRecord(p->ev_arena_pre, p->stream));
            HIPCHK(hipStreamWaitEvent(q->stream, p->ev_arena_pre, 0));
            int rc = launch_search(q, n_q, 1, true, false, false);
            if (rc) return rc;
            HIPCHK(hipEventRecord(p->ev_arena_q, q->stream));
        }
        if (n_p) {
            int rc = launch_search(p, n_p, 1, true, false, false);
            if (rc) return rc;
        }
        if (n_q) HIPCHK(hipStreamWaitEvent(p->stream, p->ev_arena_q, 0));
        if (c4) hipLaunchKernelGGL(k_c4_arena_step, dim3((B + 15) / 16), block, 0, p->stream, Q);
        else if (oth) hipLaunchKernelGGL(k_oth_arena_step, dim3((B + 15) / 16), block, 0, p->stream, O);
        else if (go) hipLaunchKernelGGL(k_go_arena_step, dim3(B), dim3(go_block(c.obs_h * c.obs_w)), 0, p->stream, G);
        else hipLaunchKernelGGL(k_arena_step, waves, block, 0, p->stream, R);
        HIPCHK(hipGetLastError());
        p->arena_ply++;
    }
    return MZ_OK;
}

// drains the arena's work (the opponent's stream is ordered before the challenger's k_arena_step) and reports a search error of either side
static int arena_drain(mz_planner* p) {
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(hipStreamSynchronize(p->stream));
    mz_planner* both[2] = {p, p->arena_q};
    for (mz_planner* s : both) {
        if (!s) continue;
        int err = 0;
        HIPCHK(hipMemcpy(&err, s->d_err, sizeof(int), hipMemcpyDeviceToHost));
        if (err) {
            HIPCHK(hipMemset(s->d_err, 0, sizeof(int)));
            return fail(MZ_E_INVALID, "search kernel reported error " + std::to_string(err));
        }
    }
    return MZ_OK;
}

extern "C" int mz_arena_read_ply(mz_planner* p, float* h_obs, uint8_t* h_mask, int32_t* h_player, int32_t* h_side, double* h_pi, double* h_root,
                                 int32_t* h_action, double* h_u, uint8_t* h_live) {
    if (!p) return fail(MZ_E_INVALID, "null planner");
    if (!p->arena_open || p->arena_ply < 1) return fail(MZ_E_STATE, "no arena ply played yet");
    int rc = arena_drain(p);
    if (rc) return rc;
    const size_t B = (size_t)p->cfg.num_envs, A = (size_t)p->cfg.num_actions, D = (size_t)obs_dim(p->cfg);
    const ArenaState& a = p->arena;
    if (h_obs) HIPCHK(hipMemcpy(h_obs, a.r_obs, B * D * sizeof(float), hipMemcpyDeviceToHost));
    if (h_mask) HIPCHK(hipMemcpy(h_mask, a.r_mask, B * A, hipMemcpyDeviceToHost));
    if (h_player) HIPCHK(hipMemcpy(h_player, a.r_player, B * sizeof(int), hipMemcpyDeviceToHost));
    if (h_side) HIPCHK(hipMemcpy(h_side, a.r_side, B * sizeof(int), hipMemcpyDeviceToHost));
    if (h_pi) HIPCHK(hipMemcpy(h_pi, a.r_pi, B * A * sizeof(double), hipMemcpyDeviceToHost));
    if (h_root) HIPCHK(hipMemcpy(h_root, a.r_root, B * sizeof(double), hipMemcpyDeviceToHost));
    if (h_action) HIPCHK(hipMemcpy(h_action, a.r_action, B * sizeof(int), hipMemcpyDeviceToHost));
    if (h_u) HIPCHK(hipMemcpy(h_u, a.r_u, B * sizeof(double), hipMemcpyDeviceToHost));
    if (h_live) HIPCHK(hipMemcpy(h_live, a.r_live, B, hipMemcpyDeviceToHost));
    return MZ_OK;
}

extern "C" int mz_arena_result(mz_planner* p, int32_t* h_winner, int32_t* h_length, double* h_ret, int64_t totals[4], int32_t* n_live) {
    if (!p) return fail(MZ_E_INVALID, "null planner");
    if (!p->arena_open) return fail(MZ_E_STATE, "call mz_arena_reset first");
    int rc = arena_drain(p);
    if (rc) return rc;
    const size_t B = (size_t)p->cfg.num_envs;
    const ArenaState& a = p->arena;
    if (h_winner) HIPCHK(hipMemcpy(h_winner, a.winner, B * sizeof(int), hipMemcpyDeviceToHost));
    if (h_length) HIPCHK(hipMemcpy(h_length, a.length, B * sizeof(int), hipMemcpyDeviceToHost));
    if (h_ret) HIPCHK(hipMemcpy(h_ret, a.ret, B * sizeof(double), hipMemcpyDeviceToHost));
    if (totals) {
        unsigned long long t[4];
        HIPCHK(hipMemcpy(t, a.totals, sizeof(t), hipMemcpyDeviceToHost));
        for (int i = 0; i < 4; i++) totals[i] = (int64_t)t[i];
    }
    if (n_live) HIPCHK(hipMemcpy(n_live, a.n_live, sizeof(int), hipMemcpyDeviceToHost));
    return MZ_OK;
}

// ---------------------------------------------------------------------------------------------------------
// arena on image and frame games (mz_arena_image.h): the device image games, and envs the host steps
// ---------------------------------------------------------------------------------------------------------
static ImgArenaLaunch imgarena_launch(mz_planner* p) {
    const mz_config& c = p->cfg;
    ImgArenaLaunch R{};
    R.L.env = p->env; R.L.x = p->ext; R.L.B = c.num_envs; R.L.A = c.num_actions; R.L.OD = p->ext_od;
    R.L.first = p->arena_ply == 0; R.L.parity = p->arena_ply & 1; R.L.obs = p->arena.obs;
    R.a = p->arena;
    R.action = p->d_action; R.pi = p->d_pi; R.root = p->d_root;
    return R;
}

// What both resets share: `x` describes the frames (checked as the self-play reset checks it; `sname` names the struct in refusals).
// Leaves the handle in an image arena of `mode` at ply 0 with every buffer allocated; the caller fills the env's state and launches
// k_imgarena_reset.
static int imgarena_reset(mz_planner* p, const mz_external_env* x, int env_kind, int mode, const std::string& sname) {
    const mz_config& c = p->cfg;
    int rc = ext_check_frames(p, x);
    if (rc) return rc;
    if (x->record_format != MZ_RECORD_F32) return fail(MZ_E_INVALID, sname + ".record_format must be MZ_RECORD_F32 (0): the arena has no record ring");
    if (!p->committed) return fail(MZ_E_STATE, "weights not committed");
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(hipStreamSynchronize(p->stream));
    ext_free(p);
    p->env_kind = env_kind;
    p->arena_open = false;  // (until every buffer is there)
    p->ring_len = 1; p->ring_pos = 0; p->ring_count = 0;  // no self-play records in this mode (mz_selfplay_read: MZ_E_INVALID)
    p->selfplay_moves = 0;
    hipError_t e = env_alloc(p->env, ENV_EXTERNAL, c.num_envs, c.num_actions, obs_dim(c), 1, 3, 3, false);
    if (e != hipSuccess) return fail(MZ_E_HIP, std::string("env_alloc: ") + hipGetErrorString(e));
    e = arena_alloc(p->arena, c.num_envs, c.num_actions, obs_dim(c));
    if (e != hipSuccess) return fail(MZ_E_HIP, std::string("arena_alloc: ") + hipGetErrorString(e));
    rc = ext_alloc(p, x);
    if (rc) return rc;
    p->arena.half = 0;
    p->arena.opponent = MZ_ARENA_NONE;
    p->arena.opening_plies = 0;
    p->arena_q = nullptr;
    p->arena_ply = 0;
    p->arena_img = mode;
    p->arena_pending = false;
    p->arena_live_h.assign((size_t)c.num_envs, 1);
    return MZ_OK;
}

// What the device games' arena resets share: `g` and `x` are the checked geometry, `code` the validated start codes
template <class G>
static int game_arena_reset(mz_planner* p, const G& g, const mz_external_env& x, const std::vector<int>& code) {
    int rc = imgarena_reset(p, &x, G::KIND, G::ARENA, G::STRUCT);
    if (rc) return rc;
    rc = game_alloc(p, g);
    if (rc) return rc;
    const size_t bytes = code.size() * sizeof(int);
    int* d_code = nullptr;
    HIPCHK(hipMalloc(reinterpret_cast<void**>(&d_code), bytes));
    hipError_t he = hipMemcpy(d_code, code.data(), bytes, hipMemcpyHostToDevice);
    if (he == hipSuccess) {
        hipLaunchKernelGGL(k_imgarena_reset, per_env(p), dim3(256), 0, p->stream, imgarena_launch(p));
        GameLaunch<G> L = game_launch<G>(p);
        L.start = d_code; L.mask = p->arena.mask; L.cur = p->arena.cur; L.opp = p->arena.opp;
        hipLaunchKernelGGL(k_game_reset<G>, per_env(p), dim3(256), 0, p->stream, L);
        game_render<G>(p);
        he = hipGetLastError();
        if (he == hipSuccess) he = hipStreamSynchronize(p->stream);
    }
    (void)hipFree(d_code);
    HIPCHK(he);
    p->arena_open = true;
    return MZ_OK;
}

extern "C" int mz_arena_reset_catch(mz_planner* p, const mz_catch_env* env, const int32_t* h_ball_col, const int32_t* h_start_row) {
    if (!p || !env) return fail(MZ_E_INVALID, "null argument to mz_arena_reset_catch");
    Catch g{};
    mz_external_env x;
    int rc = game_geometry(p, env, "mz_arena_reset_catch", g, x);
    if (rc) return rc;
    std::vector<int> code((size_t)g.B);
    for (int e = 0; e < g.B; e++) {
        const int bc = h_ball_col ? h_ball_col[e] : e % g.cols, br = h_start_row ? h_start_row[e] : 0;
        if (bc < 0 || bc >= g.cols)
            return fail(MZ_E_INVALID, "mz_arena_reset_catch: h_ball_col[" + std::to_string(e) + "] = " + std::to_string(bc) + " is outside the " + std::to_string(g.cols) + " columns");
        if (br < 0 || br > g.rows - 2)
            return fail(MZ_E_INVALID, "mz_arena_reset_catch: h_start_row[" + std::to_string(e) + "] = " + std::to_string(br) + " is outside 0 .. rows - 2 = " + std::to_string(g.rows - 2));
        code[e] = br * g.cols + bc;
    }
    return game_arena_reset(p, g, x, code);
}

extern "C" int mz_arena_reset_external(mz_planner* p, const mz_external_env* env) {
    if (!p || !env) return fail(MZ_E_INVALID, "null argument to mz_arena_reset_external");
    int rc = imgarena_reset(p, env, MZ_ENV_EXTERNAL, IMGARENA_EXTERNAL, "mz_external_env");
    if (rc) return rc;
    hipLaunchKernelGGL(k_imgarena_reset, dim3((p->cfg.num_envs + 255) / 256), dim3(256), 0, p->stream, imgarena_launch(p));
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(p->stream));
    p->arena_open = true;
    return MZ_OK;
}

// The front half of a ply, shared by both front ends: the roots of the live envs from ext.frames (k_imgarena_ingest), k_arena_pre's
// staging and "before acting" record, one deterministic search of all B roots.
static int imgarena_enqueue_search(mz_planner* p, const ImgArenaLaunch& R) {
    const mz_config& c = p->cfg;
    const int B = c.num_envs, OD = p->ext_od;
    const bool vec4 = (p->ext.S > 0 && p->ext.image && p->ext.HW % 4 == 0) || (p->ext.S == 0 && OD % 4 == 0);  // (as ext_enqueue_act)
    if (vec4) hipLaunchKernelGGL(k_imgarena_ingest<4>, dim3((OD / 4 + 256 * EXT_ITER - 1) / (256 * EXT_ITER), B), dim3(256), 0, p->stream, R);
    else hipLaunchKernelGGL(k_imgarena_ingest<1>, dim3((OD + 63) / 64, B), dim3(64), 0, p->stream, R);
    ArenaLaunch Q = arena_launch(p);
    Q.nseg = 1;
    Q.seg[0].lo = 0; Q.seg[0].n = B; Q.seg[0].side = SIDE_CHALLENGER;
    arena_seg_searched(Q.seg[0], p);
    const size_t work = (size_t)B * obs_dim(c) / 4 + 1;
    const int pre_blocks = (int)((work + 255) / 256 < 1024 ? (work + 255) / 256 : 1024);
    hipLaunchKernelGGL(k_arena_pre, dim3(pre_blocks), dim3(256), 0, p->stream, Q);
    HIPCHK(hipGetLastError());
    return launch_search(p, B, 1, true, false, false);
}

// mz_arena_step on a device image game's arena: nothing is copied and nothing waits
static int image_game_plies(mz_planner* p, const ImageGame& g, int n_plies) {
    for (int m = 0; m < n_plies; m++) {
        const ImgArenaLaunch R = imgarena_launch(p);
        int rc = imgarena_enqueue_search(p, R);
        if (rc) return rc;
        g.arena_step(p, R);
        g.render(p);
        HIPCHK(hipGetLastError());
        p->arena_ply++;
    }
    return MZ_OK;
}

extern "C" int mz_arena_reset_breakout(mz_planner* p, const mz_breakout_env* env, const int32_t* h_start_code) {
    if (!p || !env) return fail(MZ_E_INVALID, "null argument to mz_arena_reset_breakout");
    Breakout g{};
    mz_external_env x;
    int rc = game_geometry(p, env, "mz_arena_reset_breakout", g, x);
    if (rc) return rc;
    std::vector<int> code((size_t)g.B);
    for (int e = 0; e < g.B; e++) {
        code[e] = h_start_code ? h_start_code[e] : e % (2 * g.cols);
        if (code[e] < 0 || code[e] >= 2 * g.cols)
            return fail(MZ_E_INVALID, "mz_arena_reset_breakout: h_start_code[" + std::to_string(e) + "] = " + std::to_string(code[e]) + " is outside 0 .. 2 * cols - 1 = " +
                                          std::to_string(2 * g.cols - 1));
    }
    return game_arena_reset(p, g, x, code);
}

extern "C" int mz_arena_external_act(mz_planner* p, const void* h_frames, const uint8_t* h_mask, const int32_t* h_cur, const int32_t* h_opp,
                                     int32_t* h_action, uint8_t* h_live) {
    if (!p || !h_frames || !h_mask || !h_cur || !h_opp || !h_action || !h_live) return fail(MZ_E_INVALID, "null argument to mz_arena_external_act");
    if (!p->arena_open || p->arena_img != IMGARENA_EXTERNAL) return fail(MZ_E_STATE, "mz_arena_external_act: call mz_arena_reset_external first");
    if (p->arena_pending) return fail(MZ_E_STATE, "mz_arena_external_act twice: report the last act's outcome with mz_arena_external_commit first");
    if (!p->committed) return fail(MZ_E_STATE, "weights not committed");
    HIPCHK(hipSetDevice(p->device));
    const mz_config& c = p->cfg;
    const size_t B = (size_t)c.num_envs, A = (size_t)c.num_actions, fb = (size_t)p->ext.FE * (p->ext.u8 ? 1 : 4);
    // pinned staging, live envs only: a frozen env's entries are not read, so its staged frame, mask and player ids stay its last ones
    for (size_t e = 0; e < B; e++) {
        if (!p->arena_live_h[e]) continue;
        std::memcpy(static_cast<unsigned char*>(p->h_ext_frames) + e * fb, static_cast<const unsigned char*>(h_frames) + e * fb, fb);
        std::memcpy(p->h_ext_mask + e * A, h_mask + e * A, A);
        p->h_ext_cur[e] = h_cur[e];
        p->h_ext_opp[e] = h_opp[e];
    }
    HIPCHK(hipMemcpyAsync(p->ext.frames, p->h_ext_frames, B * fb, hipMemcpyHostToDevice, p->stream));
    HIPCHK(hipMemcpyAsync(p->arena.mask, p->h_ext_mask, B * A, hipMemcpyHostToDevice, p->stream));
    HIPCHK(hipMemcpyAsync(p->arena.cur, p->h_ext_cur, B * sizeof(int), hipMemcpyHostToDevice, p->stream));
    HIPCHK(hipMemcpyAsync(p->arena.opp, p->h_ext_opp, B * sizeof(int), hipMemcpyHostToDevice, p->stream));
    const ImgArenaLaunch R = imgarena_launch(p);
    int rc = imgarena_enqueue_search(p, R);
    if (rc) return rc;
    hipLaunchKernelGGL(k_imgarena_record, dim3((c.num_envs + 255) / 256), dim3(256), 0, p->stream, R);
    HIPCHK(hipGetLastError());
    int err = 0;
    HIPCHK(hipMemcpyAsync(p->h_ext_action, p->arena.r_action, B * sizeof(int), hipMemcpyDeviceToHost, p->stream));  // (a frozen env: its last move)
    HIPCHK(hipMemcpyAsync(&err, p->d_err, sizeof(int), hipMemcpyDeviceToHost, p->stream));
    HIPCHK(hipStreamSynchronize(p->stream));
    if (err) {
        HIPCHK(hipMemsetAsync(p->d_err, 0, sizeof(int), p->stream));
        HIPCHK(hipStreamSynchronize(p->stream));
        return fail(MZ_E_INVALID, "search kernel reported error " + std::to_string(err));
    }
    std::memcpy(h_action, p->h_ext_action, B * sizeof(int));
    std::memcpy(h_live, p->arena_live_h.data(), B);
    p->arena_pending = true;
    return MZ_OK;
}

extern "C" int mz_arena_external_commit(mz_planner* p, const float* h_reward, const uint8_t* h_done) {
    if (!p || !h_reward || !h_done) return fail(MZ_E_INVALID, "null argument to mz_arena_external_commit");
    if (!p->arena_open || p->arena_img != IMGARENA_EXTERNAL) return fail(MZ_E_STATE, "mz_arena_external_commit: call mz_arena_reset_external first");
    if (!p->arena_pending) return fail(MZ_E_STATE, "mz_arena_external_commit without an mz_arena_external_act");
    HIPCHK(hipSetDevice(p->device));
    const size_t B = (size_t)p->cfg.num_envs;
    for (size_t e = 0; e < B; e++) {
        const bool live = p->arena_live_h[e] != 0;
        p->h_ext_reward[e] = live ? h_reward[e] : 0.0f;
        p->h_ext_done[e] = live && h_done[e] ? 1 : 0;
    }
    HIPCHK(hipMemcpyAsync(p->ext.reward, p->h_ext_reward, B * sizeof(float), hipMemcpyHostToDevice, p->stream));
    HIPCHK(hipMemcpyAsync(p->ext.done, p->h_ext_done, B, hipMemcpyHostToDevice, p->stream));
    hipLaunchKernelGGL(k_imgarena_commit, dim3((p->cfg.num_envs + 255) / 256), dim3(256), 0, p->stream, imgarena_launch(p));
    HIPCHK(hipGetLastError());
    for (size_t e = 0; e < B; e++)
        if (p->h_ext_done[e]) p->arena_live_h[e] = 0;
    p->arena_ply++;
    p->arena_pending = false;
    return MZ_OK;
}

// ---------------------------------------------------------------------------------------------------------
// measurement hooks
// ---------------------------------------------------------------------------------------------------------
// diagnostic builds only (-DMZ_STAMPS): per-phase cycle sums of the last search launch, block 0.  Not part of the ABI header.
extern "C" int mz_debug_read_stamps(mz_planner* p, long long out[16]) {
    if (!p || !out) return fail(MZ_E_INVALID, "null argument");
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(hipStreamSynchronize(p->stream));
    HIPCHK(hipMemcpy(out, p->d_stamps, 16 * sizeof(long long), hipMemcpyDeviceToHost));
#ifdef MZ_STAMPS
    unsigned long long dbg[8];
    HIPCHK(hipMemcpyFromSymbol(dbg, HIP_SYMBOL(mz::g_dbg), sizeof(dbg)));
    long long sub[8];
    HIPCHK(hipMemcpyFromSymbol(sub, HIP_SYMBOL(mz::g_sub), sizeof(sub)));
    for (int i = 0; i < 4; i++) out[11 + i] = sub[i];
    (void)dbg;
#endif
    return MZ_OK;
}

// diagnostic builds only (-DMZ_STAMPS): register-accumulated segment stamps of tree2_select [0..11] and tree2_backup [12..23]
// diagnostic (stamps build): every workgroup's duration [0..1023] and start stamp [1024..2047] of the last search launch
extern "C" int mz_debug_read_wg_cycles(mz_planner* p, long long out[2048]) {
    if (!p || !out) return fail(MZ_E_INVALID, "null argument");
    for (int i = 0; i < 2048; i++) out[i] = 0;
#ifdef MZ_STAMPS
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(hipStreamSynchronize(p->stream));
    HIPCHK(hipMemcpyFromSymbol(out, HIP_SYMBOL(mz::g_wg_cyc), 2048 * sizeof(long long)));
#endif
    return MZ_OK;
}

extern "C" int mz_debug_read_tree_stamps(mz_planner* p, long long out[32]) {
    if (!p || !out) return fail(MZ_E_INVALID, "null argument");
    for (int i = 0; i < 32; i++) out[i] = 0;
#ifdef MZ_STAMPS
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(hipStreamSynchronize(p->stream));
    HIPCHK(hipMemcpyFromSymbol(out, HIP_SYMBOL(mz::g_ts), 24 * sizeof(long long)));
    HIPCHK(hipMemcpyFromSymbol(out + 24, HIP_SYMBOL(mz::g_root_ts), 8 * sizeof(long long)));  // root inference segments (mz_mlp.h)
#endif
    return MZ_OK;
}

// test hooks, not part of the ABI header: capture the randomness a production-mode (on-device Philox) search consumes --
// normalised root Dirichlet noise, tie-break uniforms in the order they were drawn, the final action-sampling uniform -- in
// the layout of mz_rng_inputs, so a test can check their distributions and replay the same search in parity mode.
extern "C" int mz_debug_capture_rng(mz_planner* p, int32_t enable) {
    if (!p) return fail(MZ_E_INVALID, "null planner");
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(hipStreamSynchronize(p->stream));
    const size_t B = (size_t)p->cfg.num_envs, A = (size_t)p->cfg.num_actions, T = (size_t)p->cfg.max_ties;
    if (enable && !p->d_dbg_noise) {
        HIPCHK(hipMalloc(&p->d_dbg_noise, B * A * sizeof(double)));
        HIPCHK(hipMalloc(&p->d_dbg_utie, B * T * sizeof(double)));
        HIPCHK(hipMalloc(&p->d_dbg_ufinal, B * sizeof(double)));
    }
    if (!enable) {
        if (p->d_dbg_noise) { (void)hipFree(p->d_dbg_noise); (void)hipFree(p->d_dbg_utie); (void)hipFree(p->d_dbg_ufinal); }
        p->d_dbg_noise = p->d_dbg_utie = p->d_dbg_ufinal = nullptr;
    } else {  // 0.5 where a search draws nothing: what the parity-mode tests inject for unused slots
        std::vector<double> half(B * (T > A ? T : A), 0.5);
        HIPCHK(hipMemcpy(p->d_dbg_utie, half.data(), B * T * sizeof(double), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(p->d_dbg_ufinal, half.data(), B * sizeof(double), hipMemcpyHostToDevice));
        HIPCHK(hipMemset(p->d_dbg_noise, 0, B * A * sizeof(double)));
        HIPCHK(hipDeviceSynchronize());
    }
    return MZ_OK;
}

extern "C" int mz_debug_read_rng(mz_planner* p, double* h_noise, double* h_utie, double* h_ufinal) {
    if (!p || !p->d_dbg_noise) return fail(MZ_E_STATE, "mz_debug_capture_rng(p, 1) first");
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(hipStreamSynchronize(p->stream));
    const size_t B = (size_t)p->cfg.num_envs, A = (size_t)p->cfg.num_actions, T = (size_t)p->cfg.max_ties;
    if (h_noise) HIPCHK(hipMemcpy(h_noise, p->d_dbg_noise, B * A * sizeof(double), hipMemcpyDeviceToHost));
    if (h_utie) HIPCHK(hipMemcpy(h_utie, p->d_dbg_utie, B * T * sizeof(double), hipMemcpyDeviceToHost));
    if (h_ufinal) HIPCHK(hipMemcpy(h_ufinal, p->d_dbg_ufinal, B * sizeof(double), hipMemcpyDeviceToHost));
    return MZ_OK;
}

// test hook, not part of the ABI header: overwrite the per-env step counters of the running episodes (lets a test reach the
// TimeLimit-500 truncation of CartPole without a policy that balances the pole for 500 steps)
extern "C" int mz_debug_set_env_steps(mz_planner* p, const int32_t* h_steps) {
    if (!p || !h_steps) return fail(MZ_E_INVALID, "null argument");
    if (p->env_kind == MZ_ENV_NONE) return fail(MZ_E_STATE, "call mz_selfplay_reset first");
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(hipStreamSynchronize(p->stream));
    HIPCHK(hipMemcpy(p->env.steps, h_steps, (size_t)p->cfg.num_envs * sizeof(int), hipMemcpyHostToDevice));
    return MZ_OK;
}

// diagnostic builds only (-DMZ_STAMPS -DMZ_COUNTERS): tree counters [levels, cache hits, descents, min-max changes]
extern "C" int mz_debug_read_counters(mz_planner* p, long long out[8]) {
    if (!p || !out) return fail(MZ_E_INVALID, "null argument");
    for (int i = 0; i < 8; i++) out[i] = 0;
#ifdef MZ_STAMPS
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(hipStreamSynchronize(p->stream));
    unsigned long long dbg[8];
    HIPCHK(hipMemcpyFromSymbol(dbg, HIP_SYMBOL(mz::g_dbg), sizeof(dbg)));
    for (int i = 0; i < 8; i++) out[i] = (long long)dbg[i];
    long long sub[8];
    HIPCHK(hipMemcpyFromSymbol(sub, HIP_SYMBOL(mz::g_sub), sizeof(sub)));
    (void)sub;
#endif
    return MZ_OK;
}

extern "C" int mz_planner_synchronize(mz_planner* p) {
    if (!p) return fail(MZ_E_INVALID, "null planner");
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(hipStreamSynchronize(p->stream));
    return MZ_OK;
}

extern "C" int mz_profile_begin(mz_planner* p) {
    if (!p) return fail(MZ_E_INVALID, "null planner");
    HIPCHK(hipSetDevice(p->device));
    p->profiling = true;
    p->kev_used = 0;
    HIPCHK(hipEventRecord(p->ev_begin, p->stream));
    return MZ_OK;
}

extern "C" int mz_profile_end(mz_planner* p, double* elapsed_ms, double* search_kernel_ms, int64_t* search_kernel_launches) {
    if (!p || !p->profiling) return fail(MZ_E_STATE, "mz_profile_end without mz_profile_begin");
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(hipEventRecord(p->ev_end, p->stream));
    HIPCHK(hipEventSynchronize(p->ev_end));
    float ms = 0.0f;
    HIPCHK(hipEventElapsedTime(&ms, p->ev_begin, p->ev_end));
    if (elapsed_ms) *elapsed_ms = ms;
    double ksum = 0.0;
    for (size_t i = 0; i < p->kev_used; i++) {
        float k = 0.0f;
        HIPCHK(hipEventElapsedTime(&k, p->kev[i].first, p->kev[i].second));
        ksum += k;
    }
    if (search_kernel_ms) *search_kernel_ms = ksum;
    if (search_kernel_launches) *search_kernel_launches = (int64_t)p->kev_used;
    p->profiling = false;
    return MZ_OK;
}
