// mz_learn_conv_host.h -- what learner.hip (the C ABI of include/mzlearner.h) calls for net_kind == MZL_NET_BOARD: the conv-net learner of
// learner_conv.hip over the kernels of mz_learn_conv.h.  Internal to libmzlearner_hip.so.
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
int mzlc_bind(mzlc_learner* h, float* params, float* grads, float* m, float* v);
int mzlc_bind_buffers(mzlc_learner* h, float* running, int64_t* num_batches);
int mzlc_commit(mzlc_learner* h, void* stream, std::string& err);
int mzlc_grad(mzlc_learner* h, const mzl_batch* b, void* stream, std::string& err);
int mzlc_apply(mzlc_learner* h, double lr, double beta1, double beta2, double eps, double weight_decay, double max_grad_norm, int64_t step, void* stream,
               std::string& err);
int mzlc_debug_tensor(const mzlc_learner* h, const char* what, int a, int b, void** ptr, int64_t* count);
int mzlc_debug_conv(mzlc_learner* h, int direction, int batch, int cin_real, int cin, int cout, int bh, int bw, const float* h_weight, const float* h_in,
                    const int32_t* h_action, int num_actions, float* h_out, const char** build_name, std::string& err);

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
