// mz_learn_conv_host.h -- what learner.hip (the C ABI of include/mzlearner.h) calls for net_kind == MZL_NET_BOARD: the conv-net learner of
// learner_conv.hip over the kernels of mz_learn_conv.h, and the call structs of its diagnostic hooks (mzlc_debug_*, defined in mz_learn_conv_debug.h, which
// learner_conv.hip includes).  Internal to libmzlearner_hip.so.
#pragma once
#include <stdint.h>

#include <string>

#include "../../include/mzlearner.h"

struct mzlc_learner;

int mzlc_create(const mzl_config* cfg, int device_id, int num_cus, mzlc_learner** out, std::string& err);
void mzlc_destroy(mzlc_learner* h);
int64_t mzlc_num_params(const mzlc_learner* h);
int mzlc_num_tensors(const mzlc_learner* h);
int mzlc_tensor_info(const mzlc_learner* h, int i, const char** name, int64_t* offset, int32_t* rows, int32_t* cols);
int mzlc_num_buffers(const mzlc_learner* h);
int mzlc_buffer_info(const mzlc_learner* h, int i, const char** name, int64_t* offset, int32_t* count);
int64_t mzlc_num_running(const mzlc_learner* h);
int mzlc_set_wgrad_precision(mzlc_learner* h, int precision, std::string& err);
int mzlc_wgrad_precision(const mzlc_learner* h);
int mzlc_set_atari_precision(mzlc_learner* h, int tower_precision, int stage_precision, std::string& err);
int mzlc_tower_precision(const mzlc_learner* h);
int mzlc_stage_precision(const mzlc_learner* h);
int mzlc_bind(mzlc_learner* h, float* params, float* grads, float* m, float* v);
int mzlc_bind_buffers(mzlc_learner* h, float* running, int64_t* num_batches);
int mzlc_commit(mzlc_learner* h, void* stream, std::string& err);
int mzlc_grad(mzlc_learner* h, const mzl_batch* b, void* stream, std::string& err);
int mzlc_apply(mzlc_learner* h, double lr, double beta1, double beta2, double eps, double weight_decay, double max_grad_norm, int64_t step, void* stream,
               std::string& err);
int mzlc_debug_tensor(const mzlc_learner* h, const char* what, int a, int b, void** ptr, int64_t* count);
int mzlc_debug_conv(mzlc_learner* h, int direction, int batch, int cin_real, int cin, int cout, int bh, int bw, const float* h_weight, const float* h_in,
                    const int32_t* h_action, int num_actions, float* h_out, const char** build_name, std::string& err);

// diagnostic (tests): ONE stride-1 conv of the Atari net's tile path (mzl_debug_conv_tile; exported, not part of include/mzlearner.h).  Host pointers
// throughout; null = absent.  direction 0: the forward conv, c_in = cin input and c_out = cout output channels; 1: the data gradient (c_in = cout,
// c_out = cin).  The plane is cut into 12 x 12 tiles, or 12 x 16 where the handle cuts wide tiles (W a multiple of 16, at least 48).
struct mzl_tile_call {
    int32_t direction;
    int32_t precision;     // MZL_CONV_F32 | MZL_CONV_BF16X3, whatever the handle's switches
    int32_t route;         // 0: halo_in + out_plane (the update); 1: halo_in, inner-only tiles + k_lc_tile_scatter; 2: whole haloed tiles + k_lc_tile_scatter
    int32_t batch, cin, cout, H, W;
    int32_t groups;        // out: the tiles of the call (workgroup rows of the conv; rows of `part`)
    int32_t pad_;
    const float* weight;   // [cout][cin][3][3], the LAYER's weight in both directions
    const float* in;       // [B][c_in][H][W]
    const float* skip;     // [B][c_out][H][W] or null
    const float* mask;     // route 0: [B][c_out][H][W] or null; the result is zeroed where mask (mcoef: a mask + b) <= 0 and the ST_BWD sums are taken
    const float* mcoef;    // [2][c_out] or null
    const float* partner;  // [B][c_out][H][W]: comes with mask
    float* out;            // [B][c_out][H][W]; preset to NaN bits, so an unwritten element shows
    float* part;           // route 0, or null: [groups][pad16(c_out)][4] ST_FWD partials (no mask, no skip) | [groups][pad16(c_out)][2] ST_BWD partials (mask)
};
int mzlc_debug_conv_tile(mzlc_learner* h, mzl_tile_call* c, const char** build_name, std::string& err);

// diagnostic (tests): ONE launch group of the Atari representation outside its stride-1 convs (mzl_debug_atari_stage; exported, not part of
// include/mzlearner.h), through the AtariRun members the update calls.  Host pointers throughout; null = absent; outputs are preset to NaN bits.
//   S2_FWD    weight [cout][cin][3][3], in0 = x [B][cin][2H][2W]  -> out = y [B][cout][H][W]     (gather, k_lc_pack_par, tap-set convs, accumulate, scatter)
//   S2_DGRAD  weight, in0 = dy [B][cout][H][W]                    -> out = dx [B][cin][2H][2W]   (transposed pack, par_row_d taps, the parity scatter)
//   POOL_FWD  in0 [B][cin][H][W] (H, W even)                      -> out [B][cin][H/2][W/2]
//   POOL_BWD  in0 = gout [B][cin][H/2][W/2]                       -> out = gin [B][cin][H][W]
//   RELU_BWD  in0 = g, in1 = x, both B cin H W elements           -> out = dz
//   ENTRY     in0 = x, in1 = gs | null, in2 = extra | null, in3 = partner, all [B][cin][H W]; scale; launcher
//                                                                 -> out = dz, stats [groups][pad16(cin)][2], groups
//   NORMALIZE in0 = x [B][cin][H W]                               -> out = s
//   GATHER    in0 = src0 (in1 = src1: IN_BNBWD) [B][cin][stride H][stride W], coef [3][cin] | null, mode (IN_* of mz_learn_conv.h: 0 ident, 1 bnrelu,
//             2 bnbwd), stride 1 | 2, origin (py, px), inner_only  -> out = tiles [B nty ntx][cin][14][tw + 2]
//   SCATTER   in0 = tiles [B nty ntx][cin][14][tw + 2] (src_inner: [..][cin][12][tw]), in1 = skip [B][cin][stride H][stride W] | null, stride, origin,
//             want_stats                                          -> out = plane [B][cin][stride H][stride W] (NaN bits where this parity does not
//             write), stats [groups][pad16(cin)][4] (pivot, sum, sum of squares, count), groups
// S2_*, GATHER and SCATTER need an Atari handle (its tile geometries and switches: wide tiles, par_compact); the others run on any conv handle.
enum { MZL_STAGE_S2_FWD = 0, MZL_STAGE_S2_DGRAD = 1, MZL_STAGE_POOL_FWD = 2, MZL_STAGE_POOL_BWD = 3, MZL_STAGE_RELU_BWD = 4, MZL_STAGE_ENTRY = 5,
       MZL_STAGE_NORMALIZE = 6, MZL_STAGE_GATHER = 7, MZL_STAGE_SCATTER = 8 };
enum { MZL_ENTRY_ATARI = 0, MZL_ENTRY_TOWER = 1, MZL_ENTRY_REP12 = 2 };  // AtariRun::entry | launch_entry (H W = the handle's hw) | AtariRun::entry12
struct mzl_stage_call {
    int32_t op;            // MZL_STAGE_*
    int32_t batch, cin, cout, H, W;
    int32_t mode, stride, py, px, inner_only, src_inner, want_stats, launcher;
    int32_t groups;        // out: rows of `stats`
    float scale;           // ENTRY: on gs
    const float* weight;
    const float* in0;
    const float* in1;
    const float* in2;
    const float* in3;
    const float* coef;
    float* out;
    float* stats;          // sized by the caller for the most groups the op can write: B * ceil(H W / 32)
};
int mzlc_debug_atari_stage(mzlc_learner* h, mzl_stage_call* c, const char** build_name, std::string& err);

// diagnostic (tests): ONE layer's weight gradient (mzl_debug_wgrad; exported, not part of include/mzlearner.h).  Host pointers throughout.
struct mzl_wgrad_layer {
    const float* dz;        // [nsrc][B][cout][h][w]   (nsrc = 1 outside mode `steps`)
    const float* x;         // [nsrc][B][cin_real][h][w]
    const float* y;         // or null: with dcoef, dy = c1 dz + c2 y + c3 per output channel
    const float* dcoef;     // [nsrc][3][cout] or null (identity)
    const float* xcoef;     // [nsrc][2][cin_real] or null; given: x' = relu(a x + b) while staging (IN_BNRELU)
    const int32_t* action;  // [B] or null: cin - cin_real action planes behind the real channels
    const float* preload;   // [cout][cin][3][3] or null (zeros): what the output holds before the launch (accumulate = 1 adds to it)
    float* out;             // [cout][cin][3][3]: the gradient as k_lc_wreduce (and k_lc_wgrad_act_reduce) write it
    int32_t cin_real, cin, cout, pad_;
};
enum { MZL_WGRAD_PLAIN = 0, MZL_WGRAD_PAIR = 1, MZL_WGRAD_STEPS = 2, MZL_WGRAD_RING = 3 };
struct mzl_wgrad_call {
    int32_t mode;          // MZL_WGRAD_*
    int32_t batch, h, w;   // images (ring: tiles with their halo) per source and their size
    int32_t num_actions, nsrc, accumulate;
    // overrides, 0: what the update would choose
    int32_t sg;            // images per staging round
    int32_t layout;        // 1 side by side, 2 stacked
    int32_t ipw;           // images per chunk
    int32_t remap;         // 1 XCD remap on, 2 off
    int32_t act_route;     // 1 inside the MFMA kernel, 2 the sparse gather
    // mode ring
    int32_t ring_rows;     // -1: the handle's switches; 0 .. 3: this build, refused where the update's conditions do not give it
    int32_t tapmask;       // 0 / 0x1ff: nine taps; 0x010, 0x018, 0x012, 0x01b: a parity plane's tap set
    mzl_wgrad_layer layer[2];  // [1]: the second layer of mode `pair`
};
int mzlc_debug_wgrad(mzlc_learner* h, const mzl_wgrad_call* c, const char** build_name, std::string& err);

// diagnostic (tests): ONE conv of a BatchNorm tower as the update runs it (mzl_debug_conv_fused; exported, not part of include/mzlearner.h): staging
// transform, write-through, epilogue (skip, mask, statistics) and the finalize kernel behind it.  Host pointers throughout; null = absent.
// direction 0: the forward conv, c_in = cin input and c_out = cout output channels; 1: the data gradient (c_in = cout, c_out = cin).
struct mzl_fused_conv {
    const float* weight;       // [cout][cin][3][3], the LAYER's weight in both directions
    const float* in0;          // [B][c_in][h][w]      (mode apply: y, [B][cin][h][w])
    const float* in1;          // the same shape: y (IN_BNBWD) | the residual (IN_BNRES; mode apply: the residual or null)
    const float* coef;         // [3][c_in]: (a, b, -) | (c1, c2, c3); null with in_mode 0   (mode apply: [2][cin])
    const float* mat_preload;  // [B][c_in][h][w]: what mat_out holds before the launch; null: no write-through
    const float* skip;         // [B][c_out][h][w] or null
    const float* mask;         // [B][c_out][h][w] or null
    const float* mcoef;        // [2][c_out] or null
    const float* partner;      // [B][c_out][h][w] or null (partner_is_mask: the mask buffer itself is passed as the partner)
    const float* gamma;        // [c_out]  finalize 1, 2
    const float* beta;         // [c_out]  finalize 1
    const float* save_in;      // [2][c_out] (mean, invstd)  finalize 2
    const float* part_in;      // mode finalize: [groups][pad16(c_out)][4 | 2]
    float* out;                // [B][c_out][h][w]; preset to NaN bits, so an unwritten element shows
    float* mat_out;            // [B][c_in][h][w]
    float* part;               // [groups][pad16(c_out)][4 | 2] as the conv wrote them (NaN bits where it wrote nothing), or null
    float* coef_out;           // [3][pad16(c_out)]  finalize 1, 2 (NaN bits before the launch: the padding channels show)
    float* save_out;           // [2][pad16(c_out)]  finalize 1
    float* running_mean;       // [c_out] in / out, or null  finalize 1
    float* running_var;
    float* dgamma;             // [c_out] in / out  finalize 2
    float* dbeta;
    int64_t* num_batches;      // in / out, or null  finalize 1
    int32_t direction, in_mode, stat_mode;  // IN_* and ST_* of mz_learn_conv.h
    int32_t finalize;          // 0 none, 1 OP_BNFWD (needs ST_FWD), 2 OP_BNBWD (needs ST_BWD)
    int32_t accumulate, partner_is_mask, cin, cout;
};
enum { MZL_FUSED_CONV = 0, MZL_FUSED_PAIR = 1, MZL_FUSED_FINALIZE = 2, MZL_FUSED_APPLY = 3 };
struct mzl_fused_call {
    int32_t mode;        // MZL_FUSED_*
    int32_t batch, h, w;
    int32_t groups;      // mode finalize: in, the groups of part_in; otherwise out: the image groups (workgroup rows) of the conv
    int32_t no_side;     // 1: the generic build on a 15 x 15 board too (0: the handle's choice)
    float count;         // mode finalize: the statistics' element count (the update: batch * h * w)
    int32_t pad_;
    mzl_fused_conv conv[2];  // [1]: the second job of mode pair
};
int mzlc_debug_conv_fused(mzlc_learner* h, mzl_fused_call* c, const char** build_name, std::string& err);

// diagnostic (tests): the head block alone (mzl_debug_heads; exported, not part of include/mzlearner.h): the update's own launch code (launch_heads) on
// temporary buffers.  Host pointers throughout; a null OUTPUT is skipped.  P, hw, A, K, the support sizes: the handle's.  With ng = 3 K groups in the
// update's order (step t: reward, policy, value), oc = 1, 2, 1 planes and n_out = reward support, A, value support outputs per head:
//   params / grads: per head (reward, policy, value) w1 [oc][P], gamma [oc], beta [oc], lw [n_out][oc * hw], lb [n_out];
//   running: per head mean [oc], variance [oc]; nbt: [3].
// Outputs are preset to NaN bits: a plane the head does not have, a logit beyond its n_out stay so.
struct mzl_heads_call {
    int32_t batch, rows;      // images; rows of the target tables (idx addresses them)
    const float* F_pred;      // [K][B][P][hw] the prediction tower's outputs (policy, value)
    const float* F_rew;       // [K][B][P][hw] the dynamics tower's raw outputs (reward)
    const float* params;
    const float* running;
    const int64_t* nbt;
    const float* pi;          // [rows][K][A]
    const float* value;       // [rows][K]
    const float* reward;      // [rows][K]
    const int64_t* idx;       // [B], each in [0, rows)
    const float* w;           // [B]
    float* u;                 // [ng][B][2][hw]
    float* spart_fwd;         // [ng][B][2][2] pivoted forward partials (k_lch_conv)
    float* spiv;              // [ng][B][2]
    float* coef;              // [ng][2][5]: a, b, c1, c2, c3
    float* save;              // [ng][2][2]: mean, invstd
    float* feat;              // [ng][B][2 hw]
    float* dlogit;            // [ng][B][n_max]
    float* dzb;               // [ng][B][2][hw]
    float* spart_bwd;         // [ng][B][2][2] (sum dz, sum dz u) (k_lch_loss)
    float* lpart;             // [ng][B]
    float* loss;              // [1]
    float* prio;              // [B]
    float* running_out;
    int64_t* nbt_out;
    float* dF_pred;           // [K][B][P][hw]
    float* dF_rew;
    float* wpart;             // [K][hp_total], per head: w1, lw, lb
    float* grads;
};
int mzlc_debug_heads(mzlc_learner* h, const mzl_heads_call* c, std::string& err);
