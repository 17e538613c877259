// mz_learn_conv_debug.h -- the conv learner's diagnostic hooks (mzlc_debug_*: what learner.hip's mzl_debug_* exports call; tests and tools/*_bench.py only,
// the update runs none of this).  NOT a header of its own: learner_conv.hip includes it ONCE, at its end, so that the hooks stay in that translation unit
// and call the update's own builders -- Sched, AtariRun, make_geom, launch_ops, launch_heads, pack_lin -- of its anonymous namespace, never copies of them.
//
// Every hook that touches the device works inside one DebugCall: the temporary buffers of the call, the handle's switches as they were, the event pair
// of the timed launch.  Its destructor synchronises, frees, puts the switches back and (after fail()) clears the sticky HIP error, so a hook leaves by
// plain `return` on every path and can neither leak nor leave a switch flipped for the next real update.
#pragma once

#include <cstdarg>

namespace {

struct DebugCall {
    mzlc_learner* const h;
    std::string& err;
    // EVERY switch of the handle any hook writes, saved here and restored by the destructor whatever the hook did
    const bool halo_in, out_plane, xcd_remap, act_sparse, ring_rows, row_steps, quad_steps, bad_dispatch;
    std::vector<void*> tmp;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    float ms = 0.0f;
    bool failed = false;

    DebugCall(mzlc_learner* h_, std::string& err_)
        : h(h_), err(err_), halo_in(h_->halo_in), out_plane(h_->out_plane), xcd_remap(h_->xcd_remap), act_sparse(h_->act_sparse), ring_rows(h_->ring_rows),
          row_steps(h_->row_steps), quad_steps(h_->quad_steps), bad_dispatch(h_->bad_dispatch) {}
    DebugCall(const DebugCall&) = delete;
    DebugCall& operator=(const DebugCall&) = delete;
    ~DebugCall() {
        (void)hipDeviceSynchronize();
        for (void* p : tmp) (void)hipFree(p);
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        h->halo_in = halo_in; h->out_plane = out_plane; h->xcd_remap = xcd_remap; h->act_sparse = act_sparse; h->ring_rows = ring_rows; h->row_steps = row_steps;
        h->quad_steps = quad_steps; h->bad_dispatch = bad_dispatch;
        if (failed) (void)hipGetLastError();
    }

    // a temporary buffer of `bytes` (+ 256 spare ones), every byte set to `fill`
    bool alloc(void** p, size_t bytes, int fill = 0) {
        if (hipMalloc(p, bytes + 256) != hipSuccess) return false;
        tmp.push_back(*p);
        return hipMemset(*p, fill, bytes + 256) == hipSuccess;
    }
    template <typename T> bool zeros(T** d, size_t n) { return alloc((void**)d, n * sizeof(T)); }
    template <typename T> bool nanbuf(T** d, size_t n) { return alloc((void**)d, n * sizeof(T), 0xff); }  // NaN bits: an element no kernel wrote shows
    template <typename T> bool put(T* d, const T* src, size_t n) { return hipMemcpy(d, src, n * sizeof(T), hipMemcpyHostToDevice) == hipSuccess; }
    template <typename T> bool up(T** d, const T* src, size_t n) { return zeros(d, n) && (!src || put(*d, src, n)); }  // (no source: zeros)
    template <typename T> bool down(T* dst, const T* d, size_t n) { return !dst || !d || hipMemcpy(dst, d, n * sizeof(T), hipMemcpyDeviceToHost) == hipSuccess; }  // (an absent output is skipped)
    // host [groups][rows][C] -> device [groups][dst_rows][cpad], rows beyond `rows` and the padding channels zero: how the finalize kernels leave their coefficient tables
    bool put_rows(float* d, const float* src, int C, int cpad, int rows, int dst_rows, int groups = 1) {
        std::vector<float> t((size_t)groups * dst_rows * cpad, 0.0f);
        for (int s = 0; s < groups; s++)
            for (int k = 0; k < rows; k++)
                for (int ch = 0; ch < C; ch++) t[((size_t)s * dst_rows + k) * cpad + ch] = src[((size_t)s * rows + k) * C + ch];
        return put(d, t.data(), t.size());
    }
    bool up_rows(float** d, const float* src, int C, int cpad, int rows, int dst_rows, int groups = 1) {
        return zeros(d, (size_t)groups * dst_rows * cpad) && put_rows(*d, src, C, cpad, rows, dst_rows, groups);
    }
    // `launch` between two events on `st`: us() after ran() is its time (the us= of the build names, which tools/*_bench.py read).  false: no events
    template <typename F> bool timed(hipStream_t st, F&& launch) {
        if (hipEventCreate(&ev0) != hipSuccess || hipEventCreate(&ev1) != hipSuccess) return false;
        (void)hipEventRecord(ev0, st);
        launch();
        (void)hipEventRecord(ev1, st);
        return true;
    }
    // did the launches so far go out and run?
    bool ran() {
        const bool ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess;
        if (ok && ev1) (void)hipEventElapsedTime(&ms, ev0, ev1);
        return ok;
    }
    double us() const { return (double)ms * 1e3; }
    // what ran: kept in the handle, so *build_name stays valid until the next call
    __attribute__((format(printf, 3, 4))) void name(const char** build_name, const char* fmt, ...) {
        char buf[320];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof(buf), fmt, ap);
        va_end(ap);
        h->debug_name = buf;
        if (build_name) *build_name = h->debug_name.c_str();
    }
    int fail(int rc, const char* m) {
        err = m;
        failed = true;
        return rc;
    }
};

constexpr size_t PACK_JOB_BYTES = sizeof(LcPackSplitJob) > sizeof(LcPackJob) ? sizeof(LcPackSplitJob) : sizeof(LcPackJob);

// ONE layer's weight d_w [cout][cin][3][3] through the production packer (k_lc_pack | k_lc_pack_bf16x3) on a one-layer table: only the copy of the asked
// direction exists (the other has no tiles).  d_job: PACK_JOB_BYTES of the call.  false: the job did not reach the device
bool pack_one_layer(void* d_job, bool split, bool dgrad, int cout, int cin, int n_cb, int co_tiles, const float* d_w, float* d_packed, hipStream_t st) {
    auto put_job = [&](auto j) {
        j.w_off = 0; j.cout = cout; j.cin = cin; j.cin_d = dgrad ? cin : 0;
        if (!dgrad) { j.n_cb = n_cb; j.co_tiles = co_tiles; } else { j.n_cb_d = n_cb; j.co_tiles_d = co_tiles; }
        return hipMemcpy(d_job, &j, sizeof(j), hipMemcpyHostToDevice) == hipSuccess;
    };
    if (split) {
        if (!put_job(LcPackSplitJob{})) return false;
        hipLaunchKernelGGL(k_lc_pack_bf16x3, dim3(64, 1), dim3(256), 0, st, reinterpret_cast<const LcPackSplitJob*>(d_job), d_w, reinterpret_cast<u32x4*>(d_packed));
    } else {
        if (!put_job(LcPackJob{})) return false;
        hipLaunchKernelGGL(k_lc_pack, dim3(64, 1), dim3(256), 0, st, reinterpret_cast<const LcPackJob*>(d_job), d_w, d_packed);
    }
    return true;
}

}  // namespace

// diagnostic (tests): device pointers of saved tensors, MZL_E_INVALID for anything else.  what: "y" (a = application: 0 representation, 1 + t dynamics_t,
// 1 + K + t prediction_t, 1 + 2 K the Atari net's res_blocks_3; b = layer of the tower), "x" (materialised post-ReLU outputs), "fcoef" (the layer's
// BatchNorm as applied: [3][pad16(C)], rows a, b), "s" (a = t), "gs" (a = 0: the hidden-state gradient buffer GsA, else GsB).  Round 6
// (tests/forced_masks.py: the decisions of THIS forward pass -- ReLU masks, normalisation arg-min / arg-max -- for a float64 reference that takes the
// same branches): "feat" the heads' post-ReLU features [3 K groups][B][2 hw]; the Atari representation's plane tensors "a1" / "a2" (post-ReLU conv_1 /
// conv_2), "s48_h1" / "s48_x" / "s24_h1" / "s24_x" (b = block: the block's inner post-ReLU tensor -- only with MZLC_KEEP_H1=1; else "s48_y1" /
// "s48_fcoef1" / .., its raw conv output and BatchNorm coefficients as for "y" / "fcoef" -- and the block's output), "hraw" (the pooled 6 x 6 state
// before normalisation); "obs": the gathered, decoded observations [B][C0][H][W] of the last batch (tests/test_gpu_replay_codec.py).  *count: floats of
// the tensor at the last batch where the shape is known here, else the allocation's.  "packed3": the split operand copies (32-bit words), where the
// handle has any.  (The heads' gradients towards the towers are not answered here: mzlc_debug_heads returns them, dF_pred / dF_rew.)
int mzlc_debug_tensor(const mzlc_learner* h, const char* what, int a, int b, void** ptr, int64_t* count) {
    const std::string w = what;
    const AppBufs* ap = nullptr;
    if (a == 0) ap = &h->app_rep;
    else if (a >= 1 && a <= h->K) ap = &h->app_dyn[a - 1];
    else if (a > h->K && a <= 2 * h->K) ap = &h->app_pred[a - 1 - h->K];
    else if (a == 2 * h->K + 1 && h->atari) ap = &h->a12;
    *count = (int64_t)h->T;
    if (ap == &h->a12) *count = (int64_t)h->maxB * h->P * (h->obsH / 8) * (h->obsW / 8);  // (the 12 x 12 stage of the Atari representation)
    if (w == "obs") { *ptr = h->obs; *count = (int64_t)h->lastB * h->C0 * h->obsH * h->obsW; return MZL_OK; }  // k_lc_gather's output [B][C0][H][W]
    if (w == "y" && ap && b >= 0 && b < (int)ap->y.size()) { *ptr = ap->y[b]; return MZL_OK; }
    if (w == "x" && ap && b >= 0 && b < (int)ap->x.size()) { *ptr = ap->x[b]; return MZL_OK; }
    if (w == "fcoef" && ap && b >= 0 && b < (int)ap->fcoef.size()) { *ptr = ap->fcoef[b]; *count = 3 * (int64_t)pad16(h->P); return MZL_OK; }
    if (w == "s" && a >= 0 && a < h->K) { *ptr = h->s[a]; return MZL_OK; }
    if (w == "feat") { *ptr = h->hfeat; *count = (int64_t)3 * h->K * h->lastB * LCH_MAXOC * h->hw; return MZL_OK; }
    if (h->atari) {
        const int64_t n48 = (int64_t)h->lastB * 128 * (h->obsH / 2) * (h->obsW / 2), n24 = (int64_t)h->lastB * h->P * (h->obsH / 4) * (h->obsW / 4);
        if (w == "a1") { *ptr = h->a1; *count = n48; return MZL_OK; }
        if (w == "a2") { *ptr = h->a2; *count = n24; return MZL_OK; }
        if (w == "hraw") { *ptr = h->hraw; *count = (int64_t)h->lastB * h->P * h->hw; return MZL_OK; }
        if (b >= 0 && b < 2) {
            if (w == "s48_y1") { *ptr = h->sb48.y[2 * b]; *count = n48; return MZL_OK; }
            if (w == "s24_y1") { *ptr = h->sb24.y[2 * b]; *count = n24; return MZL_OK; }
            if (w == "s48_fcoef1") { *ptr = h->sb48.fcoef[2 * b]; *count = 3 * 128; return MZL_OK; }
            if (w == "s24_fcoef1") { *ptr = h->sb24.fcoef[2 * b]; *count = 3 * (int64_t)pad16(h->P); return MZL_OK; }
            if (w == "s48_h1") { *ptr = h->sb48.h1[b]; *count = n48; return MZL_OK; }
            if (w == "s48_x") { *ptr = h->sb48.x[b]; *count = n48; return MZL_OK; }
            if (w == "s24_h1") { *ptr = h->sb24.h1[b]; *count = n24; return MZL_OK; }
            if (w == "s24_x") { *ptr = h->sb24.x[b]; *count = n24; return MZL_OK; }
        }
    }
    if (w == "gs") { *ptr = a ? h->GsB : h->GsA; return MZL_OK; }
    if (w == "packed3" && h->packed3 && h->n_pack3) { *ptr = h->packed3; *count = (int64_t)h->packed3_words * 4; return MZL_OK; }  // the split operand copies, as 32-bit words
    return MZL_E_INVALID;
}

// diagnostic (tests): ONE 3x3 conv through the production packers (k_lc_pack | k_lc_pack_bf16x3), make_geom and the production dispatcher
// (launch_ops) at the handle's conv_precision: identity staging, no statistics, skip or mask.  direction 0: the forward conv of h_in
// [batch][cin_real][bh][bw] (+ action planes up to cin channels) -> h_out [batch][cout][bh][bw]; direction 1: the data gradient of
// dy = h_in [batch][cout][bh][bw] -> h_out [batch][cin][bh][bw] (the transposed, tap-flipped copy).  Host pointers; temporary device buffers of its
// own on the NULL stream (the handle's weights, saved tensors and operand copies are not touched); *build_name ("<precision> <kernel> NPT= SIDE= G=
// <direction> us=<HIP-event time of the launch>") stays valid until the next call.
int mzlc_debug_conv(mzlc_learner* h, int direction, int batch, int cin_real, int cin, int cout, int bh, int bw, const float* h_weight, const float* h_in,
                    const int32_t* h_action, int num_actions, float* h_out, const char** build_name, std::string& err) {
    if (h->atari) { err = "board nets only (MZL_NET_BOARD)"; return MZL_E_INVALID; }
    if (!h_weight || !h_in || !h_out || !build_name) { err = "null argument"; return MZL_E_INVALID; }
    if (direction != 0 && direction != 1) { err = "direction must be 0 (forward) or 1 (data gradient)"; return MZL_E_INVALID; }
    if (batch < 1 || batch > 4096 || cin_real < 1 || cin < cin_real || cin > 4096 || cout < 1 || cout > 1024 || bh < 1 || bw < 1 || bh * bw > 240) {
        err = "bad shape: batch in [1, 4096], 1 <= cin_real <= cin <= 4096, cout in [1, 1024], bh * bw in [1, 240]";
        return MZL_E_INVALID;
    }
    if (direction == 1 && cin != cin_real) { err = "the data gradient needs cin == cin_real (action planes receive no gradient)"; return MZL_E_INVALID; }
    if (cin > cin_real && (!h_action || num_actions < 1)) { err = "cin > cin_real needs h_action and num_actions >= 1 (the action planes)"; return MZL_E_INVALID; }
    if (cin > cin_real)
        for (int b = 0; b < batch; b++)
            if (h_action[b] < 0 || h_action[b] >= num_actions) { err = "h_action out of [0, num_actions)"; return MZL_E_INVALID; }
    if (hipSetDevice(h->device) != hipSuccess) { err = "hipSetDevice"; return MZL_E_HIP; }
    const int k_in = direction == 0 ? cin : cout, c_in_mem = direction == 0 ? cin_real : cout, c_out = direction == 0 ? cout : cin;
    Geom g;
    if (!make_geom(g, bh, bw, h->allow_side, h->sw.pick, batch, cdiv(cdiv(c_out, 16), 4), h->num_cus)) { err = "image does not fit the conv kernels' tiling"; return MZL_E_INVALID; }
    const size_t lds = h->split ? conv_split_lds(g.G, bh, bw, pad16(c_in_mem)) : conv_lds(g.qstride, pad16(c_in_mem));
    if (lds > 160 * 1024) { err = "image too large for the conv kernel's LDS layout"; return MZL_E_INVALID; }
    const int hw = bh * bw, co_tiles = cdiv(c_out, 16), n_cb = cdiv(k_in, h->split ? 32 : 16);
    const size_t n_w = (size_t)cout * cin * 9, n_in = (size_t)batch * c_in_mem * hw, n_out = (size_t)batch * c_out * hw;
    const size_t n_packed = (size_t)co_tiles * n_cb * 9 * (h->split ? 192 * 4 : 256);  // floats
    float *d_w = nullptr, *d_in = nullptr, *d_out = nullptr, *d_packed = nullptr;
    int* d_act = nullptr;
    void* d_job = nullptr;
    DebugCall dc(h, err);
    if (!dc.zeros(&d_w, n_w) || !dc.zeros(&d_in, n_in) || !dc.zeros(&d_out, n_out) || !dc.zeros(&d_packed, n_packed) || !dc.zeros(&d_act, (size_t)batch) ||
        !dc.alloc(&d_job, PACK_JOB_BYTES))
        return dc.fail(MZL_E_HIP, "hipMalloc failed");
    if (!dc.put(d_w, h_weight, n_w) || !dc.put(d_in, h_in, n_in) || (cin > cin_real && !dc.put(d_act, h_action, (size_t)batch))) return dc.fail(MZL_E_HIP, "hipMemcpy failed");
    hipStream_t st = nullptr;
    if (!pack_one_layer(d_job, h->split, direction == 1, cout, cin, n_cb, co_tiles, d_w, d_packed, st)) return dc.fail(MZL_E_HIP, "hipMemcpy failed");
    Op o{};
    o.kind = OP_CONV; o.npt = g.npt; o.side15 = g.side15 ? 1 : 0; o.split = h->split;
    LcConv& c = o.conv;
    c.B = batch; c.G = g.G; c.h = bh; c.w_img = bw; c.qstride = g.qstride;
    c.cin_real = c_in_mem; c.cin = k_in; c.n_cb = n_cb; c.cout = c_out; c.co_tiles = co_tiles;
    c.cpad_in = pad16(c_in_mem); c.cpad_out = pad16(c_out);
    c.w = d_packed; c.in0 = d_in; c.out = d_out; c.in_mode = IN_IDENT; c.stat_mode = ST_NONE;
    c.action = cin > cin_real ? d_act : nullptr; c.num_actions = num_actions;
    h->bad_dispatch = false;
    int rc = 0;
    if (!dc.timed(st, [&] { rc = launch_ops(h, &o, nullptr, st); })) return dc.fail(MZL_E_HIP, "hipEventCreate failed");
    const bool bad = h->bad_dispatch, ran = dc.ran();
    if (rc != 0 || bad) return dc.fail(MZL_E_INVALID, "no kernel build for this conv");
    if (!ran) return dc.fail(MZL_E_HIP, "the conv failed to launch or run");
    if (!dc.down(h_out, d_out, n_out)) return dc.fail(MZL_E_HIP, "hipMemcpy failed");
    dc.name(build_name, "%s %s NPT=%d SIDE=%d G=%d %s us=%.1f", h->split ? "bf16x3" : "f32", h->split ? "k_lc_conv_bf16x3" : "k_lc_conv", g.npt, g.side15 ? 15 : 0, g.G,
            direction == 0 ? "forward" : "dgrad", dc.us());
    return MZL_OK;
}

// diagnostic (tests): ONE stride-1 conv of the Atari representation's tile path as the update builds it -- k_lc_tile_gather cuts the host-supplied plane
// into haloed tiles (AtariRun::gather, the geometry gt / gt16 by the plane's width), AtariRun::conv_tiles_plane_op (route 0: the update's default, the
// out_plane epilogue) or conv_tiles_op + k_lc_tile_scatter (route 1: inner-only tiles, MZLC_NO_OUT_PLANE's form; route 2: whole haloed tiles,
// MZLC_NO_HALO_IN's form) build the op from a one-layer table, launch_ops dispatches it -- at the precision of the CALL (the production packers
// k_lc_pack | k_lc_pack_bf16x3 on the call's weight).  Every pointer of the op is redirected to a temporary buffer of this call (NULL stream); the
// handle's weights, operand copies, saved tensors and switches are as before when it returns.  *build_name stays valid until the next call:
//   "<precision> <kernel> NPT= HALO= PLANE= tile=12x<tw> tiles=<per image> groups= dir=forward|dgrad stat=ST_.. us=<HIP-event time of the conv launch>"
int mzlc_debug_conv_tile(mzlc_learner* h, mzl_tile_call* c, const char** build_name, std::string& err) {
    if (!h->atari) { err = "Atari nets only (MZL_NET_ATARI): the board nets' convs go through mzl_debug_conv"; return MZL_E_INVALID; }
    if (!c->weight || !c->in || !c->out) { err = "null argument (weight, in, out)"; return MZL_E_INVALID; }
    if (c->direction != 0 && c->direction != 1) { err = "direction must be 0 (forward) or 1 (data gradient)"; return MZL_E_INVALID; }
    if (c->precision != MZL_CONV_F32 && c->precision != MZL_CONV_BF16X3) { err = "precision must be MZL_CONV_F32 (0) or MZL_CONV_BF16X3 (1)"; return MZL_E_INVALID; }
    if (c->route < 0 || c->route > 2) { err = "route must be 0 (out_plane), 1 (inner tiles + scatter) or 2 (whole haloed tiles + scatter)"; return MZL_E_INVALID; }
    const int B = c->batch, H = c->H, W = c->W;
    if (B < 1 || B > 256 || c->cin < 1 || c->cin > 1024 || c->cout < 1 || c->cout > 1024 || H < TILE || W < TILE || H > 96 || W > 96 || H % TILE) {
        err = "bad shape: batch in [1, 256], cin and cout in [1, 1024], H a multiple of 12, H and W in [12, 96]";
        return MZL_E_INVALID;
    }
    if (hipSetDevice(h->device) != hipSuccess) { err = "hipSetDevice"; return MZL_E_HIP; }
    DebugCall dc(h, err);
    h->halo_in = c->route != 2; h->out_plane = c->route == 0; h->bad_dispatch = false;
    hipStream_t st = nullptr;
    const AtariRun R{h, B, st};
    const int tw = R.tile_w(W);
    if (W % tw) return dc.fail(MZL_E_INVALID, "bad shape: W must divide into tiles of 12 columns (or 16: widths that are a multiple of 16 and at least 48)");
    const bool dg = c->direction == 1, split = c->precision == MZL_CONV_BF16X3;
    const int c_in = dg ? c->cout : c->cin, c_out = dg ? c->cin : c->cout, cpo = pad16(c_out), nt = R.ntiles(H, W), groups = B * nt;
    if ((size_t)B * (c_in > c_out ? c_in : c_out) * H * W * sizeof(float) >= ((size_t)1 << 32)) return dc.fail(MZL_E_INVALID, "the plane tensor must stay below 4 GiB");
    if (c->route != 0 && (c->mask || c->partner || c->mcoef || c->part)) return dc.fail(MZL_E_INVALID, "mask, mcoef, partner and part belong to route 0: the scatter routes mask and sum in kernels of their own");
    if (c->mcoef && !c->mask) return dc.fail(MZL_E_INVALID, "inconsistent arguments: mcoef without mask");
    if ((c->mask != nullptr) != (c->partner != nullptr)) return dc.fail(MZL_E_INVALID, "inconsistent arguments: mask and partner come together (the update masks where it takes the BatchNorm-backward sums)");
    if (c->mask && !c->part) return dc.fail(MZL_E_INVALID, "inconsistent arguments: a masked conv leaves its ST_BWD partial sums: part");
    if (c->part && !c->mask && c->skip) return dc.fail(MZL_E_INVALID, "inconsistent arguments: the forward statistics (part without mask) are taken from a conv without skip");
    LayerInfo L;  // a one-layer table: the packed copy of the asked direction at offset 0 of this call's buffer
    L.cin_real = c->cin; L.cin = c->cin; L.cout = c->cout; L.cin_d = dg ? c->cin : 0;
    L.n_cb = cdiv(L.cin, 16); L.co_tiles = cdiv(L.cout, 16); L.n_cb_d = cdiv(L.cout, 16); L.co_tiles_d = L.cin_d ? cdiv(L.cin_d, 16) : 0;
    L.n_cb3 = cdiv(L.cin, 32); L.n_cb3_d = cdiv(L.cout, 32);
    L.split3 = split;
    const int co_tiles = dg ? L.co_tiles_d : L.co_tiles, n_cb = split ? (dg ? L.n_cb3_d : L.n_cb3) : (dg ? L.n_cb_d : L.n_cb);
    const size_t n_w = (size_t)c->cout * c->cin * 9, n_packed = (size_t)co_tiles * n_cb * 9 * (split ? 192 * 4 : 256);
    const size_t ts2 = (size_t)(TILE + 2) * (tw + 2), n_in = (size_t)B * c_in * H * W, n_out = (size_t)B * c_out * H * W;
    float *d_w = nullptr, *d_packed = nullptr, *d_in = nullptr, *d_tiles = nullptr, *d_tb = nullptr, *d_out = nullptr, *d_skip = nullptr, *d_mask = nullptr, *d_partner = nullptr,
          *d_mcoef = nullptr, *d_part = nullptr;
    void* d_job = nullptr;
    bool ok = dc.up(&d_w, c->weight, n_w) && dc.zeros(&d_packed, n_packed) && dc.up(&d_in, c->in, n_in) && dc.zeros(&d_tiles, (size_t)groups * c_in * ts2) &&
              dc.nanbuf(&d_out, n_out) && dc.alloc(&d_job, PACK_JOB_BYTES);
    if (c->route != 0) ok = ok && dc.nanbuf(&d_tb, (size_t)groups * c_out * ts2);
    if (c->skip) ok = ok && dc.up(&d_skip, c->skip, n_out);
    if (c->mask) ok = ok && dc.up(&d_mask, c->mask, n_out) && dc.up(&d_partner, c->partner, n_out);
    if (c->mcoef) ok = ok && dc.up_rows(&d_mcoef, c->mcoef, c_out, cpo, 2, 2);
    if (c->part) ok = ok && dc.nanbuf(&d_part, (size_t)groups * cpo * 4);
    if (!ok) return dc.fail(MZL_E_HIP, "hipMalloc / hipMemcpy failed");
    if (!pack_one_layer(d_job, split, dg, c->cout, c->cin, n_cb, co_tiles, d_w, d_packed, st)) return dc.fail(MZL_E_HIP, "hipMemcpy failed");
    R.gather(d_in, nullptr, nullptr, IN_IDENT, c_in, H, W, H, W, 1, 1, 0, 0, 0, d_tiles);
    Op o = c->route == 0 ? R.conv_tiles_plane_op(L, dg, H, W, d_tiles, d_out, d_skip, d_part, d_mask, d_partner, d_mcoef) : R.conv_tiles_op(L, dg, H, W, d_tiles, d_tb);
    o.conv.w = d_packed;
    if (o.conv.cin_real != c_in || o.conv.cout != c_out || o.conv.cpad_out != cpo || o.conv.n_cb != n_cb) return dc.fail(MZL_E_STATE, "internal: conv_base disagrees with the call's channels");
    int rc = 0;
    if (!dc.timed(st, [&] { rc = launch_ops(h, &o, nullptr, st); })) return dc.fail(MZL_E_HIP, "hipEventCreate failed");
    const bool bad = h->bad_dispatch;
    if (rc == 0 && !bad && c->route != 0) R.scatter(d_tb, c_out, H, W, d_out, H, W, 1, 1, 0, 0, d_skip, nullptr, R.halo_in());
    const bool ran = dc.ran();
    if (rc != 0 || bad) return dc.fail(MZL_E_INVALID, "no kernel build for this tile conv");
    if (!ran) return dc.fail(MZL_E_HIP, "the tile conv failed to launch or run");
    if (!dc.down(c->out, d_out, n_out)) return dc.fail(MZL_E_HIP, "hipMemcpy failed");
    if (!dc.down(c->part, d_part, (size_t)groups * cpo * (c->mask ? 2 : 4))) return dc.fail(MZL_E_HIP, "hipMemcpy failed");
    c->groups = groups;
    dc.name(build_name, "%s %s NPT=%d HALO=%d PLANE=%d tile=12x%d tiles=%d groups=%d dir=%s stat=%s us=%.1f", split ? "bf16x3" : "f32", split ? "k_lc_conv_bf16x3" : "k_lc_conv", o.npt,
            o.conv.halo_in, o.conv.out_plane, tw, nt, groups, dg ? "dgrad" : "forward", o.conv.stat_mode == ST_FWD ? "ST_FWD" : o.conv.stat_mode == ST_BWD ? "ST_BWD" : "ST_NONE", dc.us());
    return MZL_OK;
}

// diagnostic (tests): ONE launch group of the Atari representation outside its stride-1 convs (mz_learn_conv_host.h, mzl_stage_call), through the
// AtariRun members the update itself calls -- s2_fwd / s2_dgrad (gather, tap-set convs on copies packed by k_lc_pack_par at the handle's par_compact,
// accumulation, scatter), pool_fwd / pool_bwd / relu_bwd, entry / entry12 / launch_entry, launch_normalize, gather, scatter.  Every device pointer is
// a temporary buffer of this call (NULL stream), outputs and intermediate tiles are preset to NaN bits; the handle's weights, saved tensors and
// switches are as before when it returns.  A bad shape is refused before any launch; a tap set the dispatcher has no build for ends the call with
// nothing launched after it.  *build_name stays valid until the next call and says what ran.
int mzlc_debug_atari_stage(mzlc_learner* h, mzl_stage_call* c, const char** build_name, std::string& err) {
    const int op = c->op, B = c->batch, C = c->cin, H = c->H, W = c->W;
    auto bad = [&](const char* m) { err = m; return (int)MZL_E_INVALID; };
    if (op < MZL_STAGE_S2_FWD || op > MZL_STAGE_SCATTER) return bad("op: not one of MZL_STAGE_*");
    const bool s2 = op == MZL_STAGE_S2_FWD || op == MZL_STAGE_S2_DGRAD, gs = op == MZL_STAGE_GATHER || op == MZL_STAGE_SCATTER, pool = op == MZL_STAGE_POOL_FWD || op == MZL_STAGE_POOL_BWD;
    if ((s2 || gs) && !h->atari) return bad("op: s2_fwd, s2_dgrad, gather and scatter need an Atari handle (MZL_NET_ATARI): the tile geometries are its own");
    if (B < 1 || B > 256) return bad("batch: must be in [1, 256]");
    if (C < 1 || C > 1024) return bad("C (cin): must be in [1, 1024]");
    if (s2 && (c->cout < 1 || c->cout > 1024)) return bad("cout: must be in [1, 1024]");
    if (H < 1 || W < 1 || H > 96 || W > 96) return bad("H, W: must be in [1, 96]");
    if (!c->in0) return bad("in0: null argument");
    if (!c->out) return bad("out: null argument");
    if (s2 && !c->weight) return bad("weight: null argument");
    const int stride = s2 ? 2 : (gs ? c->stride : 1);
    if (gs && stride != 1 && stride != 2) return bad("stride: must be 1 or 2");
    if (gs && (c->py < 0 || c->py >= stride || c->px < 0 || c->px >= stride)) return bad("origin (py, px): must lie in [0, stride)");
    if ((s2 || gs) && H % TILE) return bad("H: the tiled plane's height must be a multiple of 12");
    if ((s2 || gs) && (stride * H > 96 || stride * W > 96)) return bad("H, W: the strided plane must stay within 96 x 96");
    if (pool && ((H | W) & 1)) return bad("H, W: odd source sizes (the pools halve an even plane)");
    const int hw = H * W, cpad = pad16(C);
    if (op == MZL_STAGE_RELU_BWD && !c->in1) return bad("in1 (x): null argument");
    if (op == MZL_STAGE_ENTRY) {
        if (!c->in3) return bad("in3 (partner): null argument");
        if (!c->stats) return bad("stats: null argument");
        if (c->launcher < MZL_ENTRY_ATARI || c->launcher > MZL_ENTRY_REP12) return bad("launcher: must be 0 (atari), 1 (tower) or 2 (rep12)");
        if (c->launcher == MZL_ENTRY_TOWER && hw != h->hw) return bad("hw (H, W): launcher tower runs launch_entry, whose grid is cut for the handle's own hw");
        if (c->launcher == MZL_ENTRY_REP12 && (c->in1 || !c->in2)) return bad("in1 (gs), in2 (extra): launcher rep12 takes extra and no gs");
    }
    if (op == MZL_STAGE_GATHER) {
        if (c->mode != IN_IDENT && c->mode != IN_BNRELU && c->mode != IN_BNBWD) return bad("mode: must be 0 (ident), 1 (bnrelu) or 2 (bnbwd)");
        if (c->mode != IN_IDENT && !c->coef) return bad("coef: null argument (modes bnrelu and bnbwd)");
        if (c->mode == IN_BNBWD && !c->in1) return bad("in1 (src1): null argument (mode bnbwd)");
    }
    if (op == MZL_STAGE_SCATTER && c->want_stats && !c->stats) return bad("stats: null argument (want_stats)");
    const int cmax = s2 && c->cout > C ? c->cout : C;
    if ((size_t)B * cmax * stride * H * stride * W * sizeof(float) > ((size_t)1 << 30)) return bad("batch: the planes of the call must stay within 1 GiB");
    if (hipSetDevice(h->device) != hipSuccess) { err = "hipSetDevice"; return MZL_E_HIP; }
    hipStream_t st = nullptr;
    const AtariRun R{h, B, st};
    int tw = TILE, nt = 0;
    if (s2 || gs) {
        tw = R.tile_w(W);
        if (W % tw) return bad("W: the tiled plane's width must divide into tiles of 12 columns (or 16: widths that are a multiple of 16 and at least 48)");
        nt = R.ntiles(H, W);
        if (s2 && conv_lds(R.tgeom(W).qstride, pad16(op == MZL_STAGE_S2_FWD ? C : c->cout)) > 160 * 1024) return bad("cin / cout: the conv's input channels do not fit its LDS slab");
    }
    DebugCall dc(h, err);
    const size_t ts2 = (size_t)(TILE + 2) * (tw + 2), n_plane = (size_t)B * C * hw;
    const auto cpt_build = [](int C_) { const int cpt = cdiv(C_, 8); return cpt <= 2 ? 2 : cpt <= 8 ? 8 : cpt <= 16 ? 16 : 32; };  // the CPT= of the channel-strided kernels' build
    c->groups = 0;
    h->bad_dispatch = false;
    float *d_in0 = nullptr, *d_in1 = nullptr, *d_in2 = nullptr, *d_in3 = nullptr, *d_out = nullptr, *d_stats = nullptr;
    if (s2) {
        const bool dg = op == MZL_STAGE_S2_DGRAD;
        const int cin = C, cout = c->cout, k_in = dg ? cout : cin, k_out = dg ? cin : cout;  // the conv's own input / output channels
        const size_t n_w = (size_t)cout * cin * 9, per = (size_t)cdiv(k_out, 16) * cdiv(k_in, 16) * 9 * 256;
        const size_t n_x = dg ? (size_t)B * cout * hw : (size_t)B * cin * 4 * hw, n_y = dg ? (size_t)B * cin * 4 * hw : (size_t)B * cout * hw;
        float *d_w = nullptr, *d_packed = nullptr, *d_ta = nullptr, *d_tb = nullptr;
        LcPackPar* d_jobs = nullptr;
        std::vector<LcPackPar> pj(4);
        int w_off[4];
        for (int pq = 0; pq < 4; pq++) {
            LcPackPar j{};
            w_off[pq] = (int)(pq * per);
            j.w_off = 0; j.cout = cout; j.cin = cin; j.dst_off = w_off[pq]; j.n_cb = cdiv(k_in, 16); j.co_tiles = cdiv(k_out, 16); j.transpose = dg ? 1 : 0; j.compact = h->par_compact ? 1 : 0;
            par_tapmap(pq >> 1, pq & 1, dg, j.tapmap);
            pj[pq] = j;
        }
        if (!(dc.up(&d_w, c->weight, n_w) && dc.zeros(&d_packed, 4 * per) && dc.up(&d_in0, c->in0, n_x) && dc.nanbuf(&d_ta, (size_t)B * nt * pad16(k_in) * ts2) &&
              dc.nanbuf(&d_tb, (size_t)B * nt * pad16(k_out) * ts2) && dc.nanbuf(&d_out, n_y) && dc.up(&d_jobs, pj.data(), 4)))
            return dc.fail(MZL_E_HIP, "hipMalloc / hipMemcpy failed");
        hipLaunchKernelGGL(k_lc_pack_par, dim3(64, 4), dim3(256), 0, st, static_cast<const LcPackPar*>(d_jobs), d_w, d_packed);
        bool built;
        if (!dg) built = R.s2_fwd(d_packed, w_off, d_in0, cin, cout, H, W, d_ta, d_tb, d_out);
        else {
            R.gather(d_in0, nullptr, nullptr, IN_IDENT, cout, H, W, H, W, 1, 1, 0, 0, 0, d_ta);  // dy tiles with halo, as atari_rep_bwd cuts them
            built = R.s2_dgrad(d_packed, w_off, d_ta, cin, cout, H, W, d_tb, d_out);
        }
        const int npt = R.tgeom(W).npt;
        if (!built || h->bad_dispatch) {
            dc.name(nullptr, "no kernel build: kConvBuilds has none for NPT=%d (tile 12x%d) and the %s tap sets in the compact form", npt, tw, dg ? "data-gradient" : "forward");
            return dc.fail(MZL_E_INVALID, h->debug_name.c_str());
        }
        if (!dc.ran()) return dc.fail(MZL_E_HIP, "the stride-2 conv failed to launch or run");
        if (!dc.down(c->out, d_out, n_y)) return dc.fail(MZL_E_HIP, "hipMemcpy failed");
        int m[4];
        for (int pq = 0; pq < 4; pq++) m[pq] = h->par_compact ? par_tapmask(pq >> 1, pq & 1, dg) : 0x1ff;
        dc.name(build_name, "f32 k_lc_conv %s NPT=%d tile=12x%d tiles=%d compact=%d masks=0x%03x,0x%03x,0x%03x,0x%03x", dg ? "s2_dgrad" : "s2_fwd", npt, tw, nt, h->par_compact ? 1 : 0,
                m[0], m[1], m[2], m[3]);
    } else if (pool) {
        const bool fwd = op == MZL_STAGE_POOL_FWD;
        const size_t n_small = n_plane / 4;
        if (!(dc.up(&d_in0, c->in0, fwd ? n_plane : n_small) && dc.nanbuf(&d_out, fwd ? n_small : n_plane))) return dc.fail(MZL_E_HIP, "hipMalloc / hipMemcpy failed");
        if (fwd) R.pool_fwd(d_in0, d_out, C, H, W);
        else R.pool_bwd(d_in0, d_out, C, H, W);
        if (!dc.ran()) return dc.fail(MZL_E_HIP, "the pool failed to launch or run");
        if (!dc.down(c->out, d_out, fwd ? n_small : n_plane)) return dc.fail(MZL_E_HIP, "hipMemcpy failed");
        dc.name(build_name, "%s %dx%d -> %dx%d", fwd ? "k_lc_pool_fwd" : "k_lc_pool_bwd", fwd ? H : H / 2, fwd ? W : W / 2, fwd ? H / 2 : H, fwd ? W / 2 : W);
    } else if (op == MZL_STAGE_RELU_BWD) {
        if (!(dc.up(&d_in0, c->in0, n_plane) && dc.up(&d_in1, c->in1, n_plane) && dc.nanbuf(&d_out, n_plane))) return dc.fail(MZL_E_HIP, "hipMalloc / hipMemcpy failed");
        R.relu_bwd(d_in0, d_in1, d_out, (long long)n_plane);
        if (!dc.ran()) return dc.fail(MZL_E_HIP, "k_lc_relu_bwd failed to launch or run");
        if (!dc.down(c->out, d_out, n_plane)) return dc.fail(MZL_E_HIP, "hipMemcpy failed");
        dc.name(build_name, "k_lc_relu_bwd n=%lld", (long long)n_plane);
    } else if (op == MZL_STAGE_ENTRY) {
        const size_t n_stat = (size_t)B * cdiv(hw, 32) * cpad * 2;
        bool ok = dc.up(&d_in0, c->in0, n_plane) && dc.up(&d_in3, c->in3, n_plane) && dc.nanbuf(&d_out, n_plane) && dc.nanbuf(&d_stats, n_stat);
        if (c->in1) ok = ok && dc.up(&d_in1, c->in1, n_plane);
        if (c->in2) ok = ok && dc.up(&d_in2, c->in2, n_plane);
        if (!ok) return dc.fail(MZL_E_HIP, "hipMalloc / hipMemcpy failed");
        int groups;
        const char* what;
        if (c->launcher == MZL_ENTRY_ATARI) {
            groups = R.entry(d_in0, d_in1, c->scale, d_in2, d_in3, d_out, C, hw, d_stats);
            what = (!c->in1 && c->in2 && hw % 4 == 0) ? "AtariRun::entry k_lc_entry_plain" : "AtariRun::entry k_lc_entry";
        } else if (c->launcher == MZL_ENTRY_REP12) {
            groups = R.entry12(d_in0, d_in2, d_in3, d_out, C, hw, d_stats);
            what = "AtariRun::entry12 k_lc_entry";
        } else {
            LcEntry e{};
            e.x = d_in0; e.gs = d_in1; e.extra = d_in2; e.partner = d_in3; e.dz = d_out; e.stat_part = d_stats; e.scale = c->scale; e.B = B; e.C = C; e.hw = hw; e.cpad = cpad;
            launch_entry(h, e, st);
            groups = entry_groups(h, B);
            what = "launch_entry k_lc_entry";
        }
        if (groups < 1 || (size_t)groups * cpad * 2 > n_stat) return dc.fail(MZL_E_STATE, "internal: more statistic groups than chunks");
        if (!dc.ran()) return dc.fail(MZL_E_HIP, "the entry kernel failed to launch or run");
        if (!dc.down(c->out, d_out, n_plane) || !dc.down(c->stats, d_stats, (size_t)groups * cpad * 2)) return dc.fail(MZL_E_HIP, "hipMemcpy failed");
        c->groups = groups;
        dc.name(build_name, "%s CPT=%d groups=%d", what, cpt_build(C), groups);
    } else if (op == MZL_STAGE_NORMALIZE) {
        if (!(dc.up(&d_in0, c->in0, n_plane) && dc.nanbuf(&d_out, n_plane))) return dc.fail(MZL_E_HIP, "hipMalloc / hipMemcpy failed");
        launch_normalize(d_in0, d_out, B, C, hw, st);
        if (!dc.ran()) return dc.fail(MZL_E_HIP, "k_lc_normalize failed to launch or run");
        if (!dc.down(c->out, d_out, n_plane)) return dc.fail(MZL_E_HIP, "hipMemcpy failed");
        dc.name(build_name, "k_lc_normalize CPT=%d", cpt_build(C));
    } else if (op == MZL_STAGE_GATHER) {
        const size_t n_src = n_plane * stride * stride, n_t = (size_t)B * nt * C * ts2;
        float* d_coef = nullptr;
        bool ok = dc.up(&d_in0, c->in0, n_src) && dc.nanbuf(&d_out, n_t);
        if (c->in1) ok = ok && dc.up(&d_in1, c->in1, n_src);
        if (c->coef) ok = ok && dc.up_rows(&d_coef, c->coef, C, cpad, 3, 3);
        if (!ok) return dc.fail(MZL_E_HIP, "hipMalloc / hipMemcpy failed");
        R.gather(d_in0, d_in1, d_coef, c->mode, C, H, W, stride * H, stride * W, stride, stride, c->py, c->px, c->inner_only ? 1 : 0, d_out);
        if (!dc.ran()) return dc.fail(MZL_E_HIP, "k_lc_tile_gather failed to launch or run");
        if (!dc.down(c->out, d_out, n_t)) return dc.fail(MZL_E_HIP, "hipMemcpy failed");
        c->groups = B * nt;
        dc.name(build_name, "k_lc_tile_gather tile=12x%d tiles=%d mode=%d stride=%d origin=(%d,%d) inner_only=%d remap=%d chunks=%d", tw, B * nt, c->mode, stride, c->py, c->px,
                c->inner_only ? 1 : 0, (h->sw.gather_xcd && (B * nt) % 8 == 0) ? 1 : 0, cdiv(C * (int)ts2, 1024));
    } else {  // MZL_STAGE_SCATTER
        const size_t n_dst = n_plane * stride * stride, n_t = (size_t)B * nt * C * (c->src_inner ? (size_t)TILE * tw : ts2), n_stat = (size_t)B * cdiv(hw, 32) * cpad * 4;
        bool ok = dc.up(&d_in0, c->in0, n_t) && dc.nanbuf(&d_out, n_dst);
        if (c->in1) ok = ok && dc.up(&d_in1, c->in1, n_dst);
        if (c->want_stats) ok = ok && dc.nanbuf(&d_stats, n_stat);
        if (!ok) return dc.fail(MZL_E_HIP, "hipMalloc / hipMemcpy failed");
        const int groups = R.scatter(d_in0, C, H, W, d_out, stride * H, stride * W, stride, stride, c->py, c->px, d_in1, d_stats, c->src_inner != 0);
        if ((size_t)groups * cpad * 4 > n_stat) return dc.fail(MZL_E_STATE, "internal: more statistic groups than chunks");
        if (!dc.ran()) return dc.fail(MZL_E_HIP, "k_lc_tile_scatter failed to launch or run");
        if (!dc.down(c->out, d_out, n_dst) || (c->want_stats && !dc.down(c->stats, d_stats, (size_t)groups * cpad * 4))) return dc.fail(MZL_E_HIP, "hipMemcpy failed");
        c->groups = c->want_stats ? groups : 0;
        dc.name(build_name, "k_lc_tile_scatter CPT=%d tile=12x%d stride=%d origin=(%d,%d) src_inner=%d skip=%d stats=%d", cpt_build(C), tw, stride, c->py, c->px, c->src_inner ? 1 : 0,
                c->in1 ? 1 : 0, c->want_stats ? 1 : 0);
    }
    return MZL_OK;
}

// diagnostic (tests): ONE layer's weight gradient, the ops built by the update's own builders -- Sched::wgrad_ops on a board handle (mode plain, and two
// different layers in one paired launch: pair), Sched::wgrad_ops_steps (steps: nsrc sources of `batch` images in one launch), AtariRun::wgrad_tile_ops
// on an Atari handle (ring: haloed tiles, the dy ring zeroed) -- with make_geom called as mzlc_create calls it for that batch, launched by launch_ops.
// The builders point the partials and the result at the handle's buffers, sized for its own net: both (and the sparse action route's partials) are
// redirected to temporary buffers sized for the chunks of THIS call; the handle's weights, gradients, saved tensors and operand copies are not
// touched.  NULL stream; *build_name stays valid until the next call and says what ran:
//   "<precision> <kernel build> mode= SG= cols|rows|single P4= nsteps= ipw= chunks= cps= nsrc= remap= act=none|kernel|sparse ring_rows= taps=0x.. us=<launch time>"
int mzlc_debug_wgrad(mzlc_learner* h, const mzl_wgrad_call* c, const char** build_name, std::string& err) {
    const int mode = c->mode, B = c->batch, bh = c->h, bw = c->w;
    if (mode < MZL_WGRAD_PLAIN || mode > MZL_WGRAD_RING) { err = "mode must be 0 (plain), 1 (pair), 2 (steps) or 3 (ring)"; return MZL_E_INVALID; }
    if (mode == MZL_WGRAD_RING && !h->atari) { err = "mode ring needs an Atari handle (MZL_NET_ATARI): board nets have no tile path"; return MZL_E_INVALID; }
    if (mode != MZL_WGRAD_RING && h->atari) { err = "modes plain, pair and steps need a board handle (MZL_NET_BOARD); an Atari handle takes mode ring"; return MZL_E_INVALID; }
    const int nl = mode == MZL_WGRAD_PAIR ? 2 : 1, nsrc = mode == MZL_WGRAD_STEPS ? c->nsrc : 1;
    if (B < 1 || B > 4096 || bh < 1 || bw < 1) { err = "bad shape: batch in [1, 4096], h and w at least 1"; return MZL_E_INVALID; }
    if (bh * bw > (mode == MZL_WGRAD_RING ? 256 : 240)) { err = "h * w outside what the weight-gradient kernel's geometry takes (240 positions; 256 for the Atari net's wide tiles)"; return MZL_E_INVALID; }
    if (mode == MZL_WGRAD_STEPS && (nsrc < 1 || nsrc > 64)) { err = "mode steps: nsrc in [1, 64]"; return MZL_E_INVALID; }
    if (c->sg < 0 || c->ipw < 0 || c->layout < 0 || c->layout > 2 || c->remap < 0 || c->remap > 2 || c->act_route < 0 || c->act_route > 2) { err = "bad override (sg, ipw >= 0; layout, remap, act_route in [0, 2])"; return MZL_E_INVALID; }
    if (c->ipw > B) { err = "ipw override above the batch"; return MZL_E_INVALID; }
    for (int l = 0; l < nl; l++) {
        const mzl_wgrad_layer& J = c->layer[l];
        if (!J.dz || !J.x || !J.out) { err = "null argument (dz, x, out)"; return MZL_E_INVALID; }
        if (J.cin_real < 1 || J.cin < J.cin_real || J.cin > 4096 || J.cout < 1 || J.cout > 1024) { err = "bad channels: 1 <= cin_real <= cin <= 4096, cout in [1, 1024] (cin < cin_real is no layer)"; return MZL_E_INVALID; }
        if ((J.y != nullptr) != (J.dcoef != nullptr)) { err = "y and dcoef come together"; return MZL_E_INVALID; }
        if (J.cin > J.cin_real) {
            if (mode != MZL_WGRAD_PLAIN) { err = "action planes (cin > cin_real) in mode plain only: the update never pairs or defers that layer"; return MZL_E_INVALID; }
            if (!J.action || c->num_actions < 1) { err = "cin > cin_real needs action and num_actions >= 1 (the action planes)"; return MZL_E_INVALID; }
            for (int b = 0; b < B; b++)
                if (J.action[b] < 0 || J.action[b] >= c->num_actions) { err = "action out of [0, num_actions)"; return MZL_E_INVALID; }
            if (c->act_route == 2 && (J.cin - J.cin_real != c->num_actions || c->num_actions > 256)) { err = "the sparse action route needs cin - cin_real == num_actions <= 256 (one thread per plane)"; return MZL_E_INVALID; }
        } else if (J.action || c->act_route) { err = "action / act_route without action planes (cin == cin_real)"; return MZL_E_INVALID; }
        if (mode == MZL_WGRAD_RING && (J.y || J.xcoef || c->accumulate)) { err = "mode ring: the tile path stages dy and x as they are and never accumulates"; return MZL_E_INVALID; }
        if (mode == MZL_WGRAD_STEPS && c->accumulate) { err = "mode steps never accumulates"; return MZL_E_INVALID; }
    }
    if (mode == MZL_WGRAD_RING) {
        if (c->tapmask != 0 && c->tapmask != 0x1ff && c->tapmask != 0x010 && c->tapmask != 0x018 && c->tapmask != 0x012 && c->tapmask != 0x01b) { err = "tap mask: 0 / 0x1ff, 0x010, 0x018, 0x012 or 0x01b"; return MZL_E_INVALID; }
        if (c->ring_rows < -1 || c->ring_rows > 3) { err = "ring_rows in [-1, 3]"; return MZL_E_INVALID; }
        if (c->ring_rows > 0 && c->sg > 1) { err = "ring_rows > 0 needs one image per staging round (SG = 1)"; return MZL_E_INVALID; }
        if (bh < 3 || bw < 3) { err = "mode ring: a tile with its halo is at least 3 x 3"; return MZL_E_INVALID; }
        if (c->layer[0].cout > pad16(h->P > 128 ? h->P : 128)) { err = "mode ring: cout above the handle's identity-coefficient rows"; return MZL_E_INVALID; }
    } else if (c->ring_rows > 0 || (c->tapmask && c->tapmask != 0x1ff)) { err = "ring_rows / tap masks belong to mode ring"; return MZL_E_INVALID; }
    if (hipSetDevice(h->device) != hipSuccess) { err = "hipSetDevice"; return MZL_E_HIP; }

    // ---- geometry: as mzlc_create builds it (board: hidden_geom for this batch and this layer's block grid; ring: the tile geometries, no batch) ----
    const mzl_wgrad_layer& J0 = c->layer[0];
    WgradPick pick = h->sw.pick;
    if (c->sg > 0) pick.sg_force = c->sg;
    if (c->layout) pick.stack_rows = c->layout == 2;
    Geom g;
    int fit;
    if (mode == MZL_WGRAD_RING) fit = make_geom(g, bh, bw, false, pick, 0, 1, 256, true, bh * bw > 240) ? 0 : 1;  // (an Atari handle: never wsplit)
    else fit = hidden_geom(h, g, bh, bw, B, h->allow_side, pick, J0.cout, J0.cin_real, h->wsplit);
    if (fit == 1) { err = c->sg > 0 ? "SG override: the staging lanes (SG quads-per-image <= 64) or the LDS of two workgroups per CU do not hold that many images per round" : "image does not fit the kernels' geometry"; return MZL_E_INVALID; }
    if (fit == 2) { err = c->sg > 0 ? "SG override: the staging lanes (SG quads-per-image <= 64) or the LDS of one workgroup (160 KB of split planes) do not hold that many images per round" : "image does not fit the split weight gradient's planes"; return MZL_E_INVALID; }
    if ((h->wsplit ? wgrad_split_lds(g.SPY, g.SPX) : wgrad_lds(g)) > 160 * 1024) { err = "the weight-gradient planes of this geometry exceed the LDS"; return MZL_E_INVALID; }

    // ---- device buffers ----
    DebugCall dc(h, err);
    const size_t hw = (size_t)bh * bw;
    struct Dev { float *dz = nullptr, *x = nullptr, *y = nullptr, *dcoef = nullptr, *xcoef = nullptr, *out = nullptr, *part = nullptr, *part_act = nullptr; int* act = nullptr; LcWgradSrc* srcs = nullptr; };
    Dev d[2];
    for (int l = 0; l < nl; l++) {
        const mzl_wgrad_layer& J = c->layer[l];
        const size_t n_dz = (size_t)nsrc * B * J.cout * hw, n_x = (size_t)nsrc * B * J.cin_real * hw, n_out = (size_t)J.cout * J.cin * 9;
        const int cpo = pad16(J.cout), cpi = pad16(J.cin_real);
        if (!dc.zeros(&d[l].dz, n_dz) || !dc.zeros(&d[l].x, n_x) || !dc.zeros(&d[l].out, n_out) || !dc.zeros(&d[l].dcoef, (size_t)nsrc * 3 * cpo) || !dc.zeros(&d[l].xcoef, (size_t)nsrc * 3 * cpi) ||
            !dc.zeros(&d[l].act, (size_t)B) || !dc.zeros(&d[l].srcs, (size_t)nsrc) || (J.y && !dc.zeros(&d[l].y, n_dz)))
            return dc.fail(MZL_E_HIP, "hipMalloc failed");
        std::vector<float> ident;  // no dcoef: dy = dz, (c1, c2, c3) = (1, 0, 0) per source
        if (!J.dcoef) {
            ident.assign((size_t)nsrc * 3 * J.cout, 0.0f);
            for (int s = 0; s < nsrc; s++)
                for (int ch = 0; ch < J.cout; ch++) ident[(size_t)s * 3 * J.cout + ch] = 1.0f;
        }
        bool ok = dc.put(d[l].dz, J.dz, n_dz) && dc.put(d[l].x, J.x, n_x) && dc.put_rows(d[l].dcoef, J.dcoef ? J.dcoef : ident.data(), J.cout, cpo, 3, 3, nsrc);
        if (J.xcoef) ok = ok && dc.put_rows(d[l].xcoef, J.xcoef, J.cin_real, cpi, 2, 3, nsrc);
        if (J.y) ok = ok && dc.put(d[l].y, J.y, n_dz);
        if (J.action) ok = ok && dc.put(d[l].act, J.action, (size_t)B);
        if (J.preload) ok = ok && dc.put(d[l].out, J.preload, n_out);
        if (!d[l].y) d[l].y = d[l].dz;  // (identity coefficients: c2 = 0, as the tile path passes its dy tiles twice)
        std::vector<LcWgradSrc> tab(nsrc);
        for (int s = 0; s < nsrc; s++) {
            tab[s].dz = d[l].dz + (size_t)s * B * J.cout * hw; tab[s].y = d[l].y + (size_t)s * B * J.cout * hw; tab[s].dcoef = d[l].dcoef + (size_t)s * 3 * cpo;
            tab[s].x0 = d[l].x + (size_t)s * B * J.cin_real * hw; tab[s].xcoef = J.xcoef ? d[l].xcoef + (size_t)s * 3 * cpi : nullptr;
        }
        ok = ok && dc.put(d[l].srcs, tab.data(), tab.size());
        if (!ok) return dc.fail(MZL_E_HIP, "hipMemcpy failed");
    }

    // ---- the ops, by the update's builders ----
    if (c->remap) h->xcd_remap = c->remap == 1;
    if (mode == MZL_WGRAD_RING && c->ring_rows >= 0) { h->ring_rows = c->ring_rows > 0; h->row_steps = c->ring_rows == 2; h->quad_steps = c->ring_rows == 3; }
    std::vector<Op> ops[2];
    for (int l = 0; l < nl; l++) {
        const mzl_wgrad_layer& J = c->layer[l];
        LayerInfo L;
        L.cin_real = J.cin_real; L.cin = J.cin; L.cout = J.cout; L.co_tiles = cdiv(J.cout, 16); L.w_off = 0;
        Sched s{h, B, l, mode == MZL_WGRAD_PAIR, g, J.cout};
        s.ipw_force = c->ipw; s.act_route = c->act_route; s.A_force = c->num_actions;
        const int x_mode = J.xcoef ? IN_BNRELU : IN_IDENT;
        if (mode == MZL_WGRAD_RING) {
            signed char m[9];
            int pq = -1;
            for (int k = 0; k < 4; k++)
                if (par_tapmask(k >> 1, k & 1, false) == c->tapmask) pq = k;
            if (pq >= 0) par_tapmap(pq >> 1, pq & 1, false, m);
            const AtariRun R{h, B, nullptr};
            R.wgrad_tile_ops(ops[l], s, L, J.cin_real, d[l].dz, d[l].x, pq >= 0 ? m : nullptr);
        } else if (mode == MZL_WGRAD_STEPS) {
            s.wgrad_ops_steps(ops[l], L, d[l].srcs, nsrc, x_mode);
        } else {
            s.wgrad_ops(ops[l], L, d[l].dz, d[l].y, d[l].dcoef, d[l].x, x_mode, J.xcoef ? d[l].xcoef : nullptr, J.cin > J.cin_real ? d[l].act : nullptr, c->accumulate ? 1 : 0);
        }
        if (ops[l].size() < 2 || ops[l][0].kind != OP_WGRAD || ops[l][1].kind != OP_WREDUCE) return dc.fail(MZL_E_STATE, "internal: unexpected op list");
        // partials and result: buffers of this call, sized from the ops the builder made
        LcWreduce& wr = ops[l][1].wr;
        if (!dc.zeros(&d[l].part, (size_t)wr.chunks * 9 * wr.co_pad * wr.ci_pad)) return dc.fail(MZL_E_HIP, "hipMalloc failed");
        ops[l][0].wg.part = d[l].part; wr.part = d[l].part; wr.grad = d[l].out;
        if (ops[l].size() > 2) {
            if (ops[l].size() != 3 || ops[l][2].kind != OP_WGRAD_ACT) return dc.fail(MZL_E_STATE, "internal: unexpected op list");
            LcWgradAct& wa = ops[l][2].wa;
            if (!dc.zeros(&d[l].part_act, (size_t)wa.nchunk * wa.cout * wa.A * 9)) return dc.fail(MZL_E_HIP, "hipMalloc failed");
            wa.part = d[l].part_act; wa.grad = d[l].out;
        }
    }
    const LcWgrad& W0 = ops[0][0].wg;
    if (mode == MZL_WGRAD_RING && c->ring_rows >= 0 && W0.ring_rows != c->ring_rows) return dc.fail(MZL_E_INVALID, "the update's conditions do not give this ring_rows build for this tile (1: any; 2: pitch above 16 and at most 16 inner columns; 3: 12 inner columns)");
    if (mode == MZL_WGRAD_PAIR && ops[0].size() != ops[1].size()) return dc.fail(MZL_E_STATE, "internal: op lists of the pair do not line up");

    // ---- launch: the timed interval is the first op alone (the weight-gradient kernel, not its reduction) ----
    hipStream_t st = nullptr;
    h->bad_dispatch = false;
    auto launch = [&](size_t i) { return launch_ops(h, &ops[0][i], nl == 2 ? &ops[1][i] : nullptr, st); };
    int rc = 0;
    if (!dc.timed(st, [&] { rc = launch(0); })) return dc.fail(MZL_E_HIP, "hipEventCreate failed");
    for (size_t i = 1; i < ops[0].size() && rc == 0; i++) rc = launch(i);
    const bool bad = h->bad_dispatch, ran = dc.ran();
    if (rc != 0 || bad) return dc.fail(MZL_E_INVALID, "no kernel build for this weight gradient");
    if (!ran) return dc.fail(MZL_E_HIP, "the weight gradient failed to launch or run");
    for (int l = 0; l < nl; l++)
        if (!dc.down(c->layer[l].out, d[l].out, (size_t)c->layer[l].cout * c->layer[l].cin * 9)) return dc.fail(MZL_E_HIP, "hipMemcpy failed");
    static const char* modes[4] = {"plain", "pair", "steps", "ring"};
    const bool has_act = J0.cin > J0.cin_real;
    dc.name(build_name, "%s %s mode=%s SG=%d %s P4=%d nsteps=%d ipw=%d chunks=%d cps=%d nsrc=%d remap=%d act=%s ring_rows=%d taps=0x%03x us=%.1f", h->split ? "bf16x3" : "f32",
            h->dbg_wgrad_build, modes[mode], W0.sg, W0.sg == 1 ? "single" : (W0.sg_cols ? "cols" : "rows"), W0.P4, W0.nsteps, W0.ipw, ops[0][1].wr.chunks, W0.srcs ? W0.cps : 0,
            W0.srcs ? W0.nsrc : 0, h->dbg_wgrad_remap, !has_act ? "none" : (ops[0].size() > 2 ? "sparse" : "kernel"), W0.ring_rows, W0.tapmask ? W0.tapmask : 0x1ff, dc.us());
    return MZL_OK;
}

// diagnostic (tests): ONE conv of a BatchNorm tower as the update runs it -- staging transform (all four IN_ modes), write-through, epilogue (skip, mask,
// ST_FWD / ST_BWD partials) and the finalize kernel that follows -- or two such convs of different layers in one paired launch (pair), a finalize
// kernel alone on host-supplied partials of any group count (finalize), or k_lc_apply alone (apply).  Production code throughout: the packers, make_geom
// as mzlc_create calls it for that batch, the Sched builders conv_base / op_conv / op_bnfwd / op_bnbwd / op_apply with the LcConv fields set as tower_fwd and
// tower_bwd set them, launch_ops.  The builders point at the handle's weights, statistics, parameters, gradients and running statistics: every one of
// those pointers is redirected to a temporary buffer of this call (NULL stream), the handle is not touched.  *build_name stays valid until the next call:
//   "<precision> <kernel> NPT= SIDE= G= groups= z= mode=IN_.. stat=ST_.. dir=forward|dgrad pair=0|1 fin=none|fwd|bwd"   (conv, pair)
//   "<precision> k_lc_bn_fwd|k_lc_bn_bwd groups= C= cpad= accumulate="   (finalize)        "<precision> k_lc_apply n= C= hw= res=0|1"   (apply)
int mzlc_debug_conv_fused(mzlc_learner* h, mzl_fused_call* c, const char** build_name, std::string& err) {
    if (h->atari) { err = "board nets only (MZL_NET_BOARD)"; return MZL_E_INVALID; }
    const int mode = c->mode, B = c->batch, bh = c->h, bw = c->w;
    if (mode < MZL_FUSED_CONV || mode > MZL_FUSED_APPLY) { err = "mode must be 0 (conv), 1 (pair), 2 (finalize) or 3 (apply)"; return MZL_E_INVALID; }
    if (B < 1 || B > 4096 || bh < 1 || bw < 1 || bh * bw > 240) { err = "bad shape: batch in [1, 4096], h * w in [1, 240]"; return MZL_E_INVALID; }
    const int nj = mode == MZL_FUSED_PAIR ? 2 : 1, hw = bh * bw;
    for (int l = 0; l < nj; l++) {
        const mzl_fused_conv& J = c->conv[l];
        if (J.cin < 1 || J.cin > 4096 || J.cout < 1 || J.cout > 1024) { err = "bad channels: cin in [1, 4096], cout in [1, 1024]"; return MZL_E_INVALID; }
        if (mode == MZL_FUSED_APPLY) {
            if (!J.in0 || !J.coef || !J.out) { err = "null argument (mode apply: in0 = y, coef, out)"; return MZL_E_INVALID; }
            continue;
        }
        if (J.finalize < 0 || J.finalize > 2) { err = "finalize must be 0 (none), 1 (OP_BNFWD) or 2 (OP_BNBWD)"; return MZL_E_INVALID; }
        if (J.finalize == 1 && (!J.gamma || !J.beta || !J.coef_out || !J.save_out)) { err = "null argument (finalize 1: gamma, beta, coef_out, save_out)"; return MZL_E_INVALID; }
        if (J.finalize == 1 && ((J.running_mean != nullptr) != (J.running_var != nullptr))) { err = "inconsistent arguments: running_mean and running_var come together"; return MZL_E_INVALID; }
        if (J.finalize == 2 && (!J.gamma || !J.save_in || !J.coef_out || !J.dgamma || !J.dbeta)) { err = "null argument (finalize 2: gamma, save_in, coef_out, dgamma, dbeta)"; return MZL_E_INVALID; }
        if (mode == MZL_FUSED_FINALIZE) {
            if (J.finalize == 0 || !J.part_in) { err = "null argument (mode finalize: finalize 1 or 2 and part_in)"; return MZL_E_INVALID; }
            if (c->groups < 1 || c->groups > (1 << 20) || !(c->count >= 1.0f)) { err = "mode finalize: groups in [1, 2^20], count at least 1"; return MZL_E_INVALID; }
            continue;
        }
        if (!J.weight || !J.in0 || !J.out) { err = "null argument (weight, in0, out)"; return MZL_E_INVALID; }
        if (J.direction != 0 && J.direction != 1) { err = "direction must be 0 (forward) or 1 (data gradient)"; return MZL_E_INVALID; }
        if (J.in_mode < IN_IDENT || J.in_mode > IN_BNRES) { err = "in_mode must be 0 (IN_IDENT), 1 (IN_BNRELU), 2 (IN_BNBWD) or 3 (IN_BNRES)"; return MZL_E_INVALID; }
        if (J.stat_mode < ST_NONE || J.stat_mode > ST_BWD) { err = "stat_mode must be 0 (ST_NONE), 1 (ST_FWD) or 2 (ST_BWD)"; return MZL_E_INVALID; }
        if ((J.in_mode != IN_IDENT) != (J.coef != nullptr)) { err = "inconsistent arguments: coef comes with a staging transform (in_mode 1, 2, 3) and only with one"; return MZL_E_INVALID; }
        if ((J.in_mode == IN_BNBWD || J.in_mode == IN_BNRES) != (J.in1 != nullptr)) { err = "inconsistent arguments: in1 comes with IN_BNBWD and IN_BNRES and only with them"; return MZL_E_INVALID; }
        if ((J.mat_preload != nullptr) != (J.mat_out != nullptr)) { err = "inconsistent arguments: mat_preload and mat_out come together"; return MZL_E_INVALID; }
        if (J.mat_out && J.in_mode != IN_BNRELU && J.in_mode != IN_BNRES) { err = "inconsistent arguments: the write-through (mat_out) exists for IN_BNRELU and IN_BNRES staging only"; return MZL_E_INVALID; }
        if (J.mcoef && !J.mask) { err = "inconsistent arguments: mcoef without mask"; return MZL_E_INVALID; }
        if (J.partner_is_mask && (!J.mask || J.partner)) { err = "inconsistent arguments: partner_is_mask needs mask and no partner array of its own"; return MZL_E_INVALID; }
        if ((J.stat_mode == ST_BWD) != (J.partner != nullptr || J.partner_is_mask != 0)) { err = "inconsistent arguments: ST_BWD needs a partner (or partner_is_mask), and a partner needs ST_BWD"; return MZL_E_INVALID; }
        if ((J.stat_mode != ST_NONE) != (J.part != nullptr)) { err = "inconsistent arguments: part comes with a stat_mode and only with one"; return MZL_E_INVALID; }
        if (J.finalize && J.finalize != J.stat_mode) { err = "inconsistent arguments: finalize 1 follows ST_FWD, finalize 2 follows ST_BWD"; return MZL_E_INVALID; }
    }
    if (nj == 2 && (c->conv[0].in_mode != c->conv[1].in_mode || c->conv[0].finalize != c->conv[1].finalize)) { err = "mode pair: the two jobs share in_mode and finalize (one kernel build per launch)"; return MZL_E_INVALID; }
    if (hipSetDevice(h->device) != hipSuccess) { err = "hipSetDevice"; return MZL_E_HIP; }

    // ---- geometry: as mzlc_create builds it (hidden_geom), for this batch and the first job's layer ----
    Geom g;
    if (hidden_geom(h, g, bh, bw, h->sw.images(B), h->allow_side && !c->no_side, h->sw.pick, c->conv[0].cout, c->conv[0].cout, false)) {
        err = "image does not fit the conv kernels' tiling";
        return MZL_E_INVALID;
    }

    DebugCall dc(h, err);
    hipStream_t st = nullptr;
    const char* prec = h->split ? "bf16x3" : "f32";

    if (mode == MZL_FUSED_APPLY) {
        const mzl_fused_conv& J = c->conv[0];
        const int C = J.cin, cpad = pad16(C);
        const size_t n = (size_t)B * C * hw;
        float *d_y = nullptr, *d_res = nullptr, *d_coef = nullptr, *d_out = nullptr;
        if (!dc.up(&d_y, J.in0, n) || (J.in1 && !dc.up(&d_res, J.in1, n)) || !dc.up_rows(&d_coef, J.coef, C, cpad, 2, 3) || !dc.nanbuf(&d_out, n)) return dc.fail(MZL_E_HIP, "hipMalloc / hipMemcpy failed");
        const Sched s{h, B, 0, false, g, C};
        const Op o = s.op_apply(d_y, d_res, d_coef, d_out);
        h->bad_dispatch = false;
        const int rc = launch_ops(h, &o, nullptr, st);
        if (rc != 0 || h->bad_dispatch) return dc.fail(MZL_E_INVALID, "no kernel for this op");
        if (!dc.ran()) return dc.fail(MZL_E_HIP, "k_lc_apply failed to launch or run");
        if (!dc.down(J.out, d_out, n)) return dc.fail(MZL_E_HIP, "hipMemcpy failed");
        dc.name(build_name, "%s k_lc_apply n=%lld C=%d hw=%d res=%d", prec, o.ap.n, C, hw, J.in1 ? 1 : 0);
        return MZL_OK;
    }

    struct Dev {
        float *w = nullptr, *packed = nullptr, *in0 = nullptr, *in1 = nullptr, *coef = nullptr, *mat = nullptr, *skip = nullptr, *mask = nullptr, *mcoef = nullptr, *partner = nullptr,
              *out = nullptr, *part = nullptr, *gamma = nullptr, *beta = nullptr, *save_in = nullptr, *coef_out = nullptr, *save_out = nullptr, *rm = nullptr, *rv = nullptr,
              *dgamma = nullptr, *dbeta = nullptr;
        int64_t* nbt = nullptr;
        void* job = nullptr;
        int c_in = 0, c_out = 0, cpo = 0, groups = 0;
    };
    Dev d[2];
    std::vector<Op> ops[2];
    for (int l = 0; l < nj; l++) {
        const mzl_fused_conv& J = c->conv[l];
        Dev& D = d[l];
        const bool conv = mode != MZL_FUSED_FINALIZE;
        D.c_in = conv && J.direction == 1 ? J.cout : J.cin;
        D.c_out = conv && J.direction == 1 ? J.cin : J.cout;
        D.cpo = pad16(D.c_out);
        D.groups = conv ? cdiv(B, g.G) : c->groups;
        const int cpi = pad16(D.c_in), C = D.c_out;
        const size_t n_in = (size_t)B * D.c_in * hw, n_out = (size_t)B * D.c_out * hw, n_part = (size_t)D.groups * D.cpo * 4;
        LayerInfo L;  // the layer of the conv (its packed copies at offset 0 of this call's buffer) and the BatchNorm behind the conv's OUTPUT
        L.cin_real = J.cin; L.cin = J.cin; L.cout = J.cout; L.cin_d = conv && J.direction == 1 ? J.cin : 0;
        L.n_cb = cdiv(L.cin, 16); L.co_tiles = cdiv(L.cout, 16); L.n_cb_d = cdiv(L.cout, 16); L.co_tiles_d = L.cin_d ? cdiv(L.cin_d, 16) : 0;
        L.n_cb3 = cdiv(L.cin, 32); L.n_cb3_d = cdiv(L.cout, 32);
        L.split3 = h->split;
        L.bn.C = C; L.bn.cpad = D.cpo;
        Sched s{h, B, l, nj == 2, g, C};
        bool ok = dc.nanbuf(&D.part, n_part);
        if (conv) {
            const bool dg = J.direction == 1;
            const int co_tiles = dg ? L.co_tiles_d : L.co_tiles, n_cb = h->split ? (dg ? L.n_cb3_d : L.n_cb3) : (dg ? L.n_cb_d : L.n_cb);
            const size_t n_w = (size_t)J.cout * J.cin * 9, n_packed = (size_t)co_tiles * n_cb * 9 * (h->split ? 192 * 4 : 256);
            const size_t lds = h->split ? conv_split_lds(g.G, bh, bw, cpi) : conv_lds(g.qstride, cpi);
            if (lds > 160 * 1024) return dc.fail(MZL_E_INVALID, "image too large for the conv kernel's LDS layout");
            ok = ok && dc.up(&D.w, J.weight, n_w) && dc.zeros(&D.packed, n_packed) && dc.up(&D.in0, J.in0, n_in) && dc.nanbuf(&D.out, n_out) && dc.alloc(&D.job, PACK_JOB_BYTES);
            if (J.in1) ok = ok && dc.up(&D.in1, J.in1, n_in);
            if (J.coef) ok = ok && dc.up_rows(&D.coef, J.coef, D.c_in, cpi, 3, 3);
            if (J.mat_out) ok = ok && dc.up(&D.mat, J.mat_preload, n_in);
            if (J.skip) ok = ok && dc.up(&D.skip, J.skip, n_out);
            if (J.mask) ok = ok && dc.up(&D.mask, J.mask, n_out);
            if (J.mcoef) ok = ok && dc.up_rows(&D.mcoef, J.mcoef, C, D.cpo, 2, 3);
            if (J.partner) ok = ok && dc.up(&D.partner, J.partner, n_out);
            if (!ok) return dc.fail(MZL_E_HIP, "hipMalloc / hipMemcpy failed");
            if (!pack_one_layer(D.job, h->split, dg, J.cout, J.cin, n_cb, co_tiles, D.w, D.packed, st)) return dc.fail(MZL_E_HIP, "hipMemcpy failed");
            LcConv k = s.conv_base(L, dg);  // (the fields below: as tower_fwd / tower_bwd fill them)
            k.w = D.packed;
            k.in0 = D.in0; k.in1 = D.in1; k.coef = D.coef; k.in_mode = J.in_mode; k.mat_out = D.mat; k.out = D.out;
            k.skip = D.skip; k.mask = D.mask; k.mcoef = D.mcoef; k.partner = J.partner_is_mask ? D.mask : D.partner;
            k.stat_mode = J.stat_mode; k.stat_part = J.stat_mode != ST_NONE ? D.part : nullptr;
            if (k.cin_real != D.c_in || k.cout != D.c_out || k.cpad_out != D.cpo || k.cpad_in != cpi) return dc.fail(MZL_E_STATE, "internal: conv_base disagrees with the call's channels");
            ops[l].push_back(s.op_conv(k, L.split3));
        } else {
            ok = ok && dc.put(D.part, J.part_in, (size_t)D.groups * D.cpo * (J.finalize == 1 ? 4 : 2));
        }
        if (J.finalize == 1) {
            ok = ok && dc.up(&D.gamma, J.gamma, C) && dc.up(&D.beta, J.beta, C) && dc.nanbuf(&D.coef_out, (size_t)3 * D.cpo) && dc.nanbuf(&D.save_out, (size_t)2 * D.cpo);
            if (J.running_mean) ok = ok && dc.up(&D.rm, J.running_mean, C) && dc.up(&D.rv, J.running_var, C);
            if (J.num_batches) ok = ok && dc.up(&D.nbt, J.num_batches, 1);
            if (!ok) return dc.fail(MZL_E_HIP, "hipMalloc / hipMemcpy failed");
            Op o = s.op_bnfwd(L, D.coef_out, D.save_out);
            o.bf.part = D.part; o.bf.gamma = D.gamma; o.bf.beta = D.beta; o.bf.running_mean = D.rm; o.bf.running_var = D.rv; o.bf.num_batches = D.nbt;
            if (!conv) { o.bf.groups = D.groups; o.bf.count = c->count; }
            ops[l].push_back(o);
        } else if (J.finalize == 2) {
            ok = ok && dc.up(&D.gamma, J.gamma, C) && dc.up_rows(&D.save_in, J.save_in, C, D.cpo, 2, 3) && dc.nanbuf(&D.coef_out, (size_t)3 * D.cpo) && dc.up(&D.dgamma, J.dgamma, C) &&
                 dc.up(&D.dbeta, J.dbeta, C);
            if (!ok) return dc.fail(MZL_E_HIP, "hipMalloc / hipMemcpy failed");
            Op o = s.op_bnbwd(L, D.save_in, D.coef_out, D.groups, J.accumulate ? 1 : 0);
            o.bb.part = D.part; o.bb.gamma = D.gamma; o.bb.dgamma = D.dgamma; o.bb.dbeta = D.dbeta;
            if (!conv) o.bb.count = c->count;
            ops[l].push_back(o);
        }
        if (!ok) return dc.fail(MZL_E_HIP, "hipMalloc / hipMemcpy failed");
    }
    if (nj == 2 && ops[0].size() != ops[1].size()) return dc.fail(MZL_E_STATE, "internal: op lists of the pair do not line up");

    // ---- launch ----
    h->bad_dispatch = false;
    int rc = 0;
    for (size_t i = 0; i < ops[0].size() && rc == 0; i++) rc = launch_ops(h, &ops[0][i], nj == 2 ? &ops[1][i] : nullptr, st);
    const bool bad = h->bad_dispatch, ran = dc.ran();
    if (rc != 0 || bad) return dc.fail(MZL_E_INVALID, "launch_ops refused the job: no kernel build for it (a conv that leaves ST_FWD statistics carries no skip and no mask)");
    if (!ran) return dc.fail(MZL_E_HIP, "the kernels failed to launch or run");
    for (int l = 0; l < nj; l++) {
        const mzl_fused_conv& J = c->conv[l];
        const Dev& D = d[l];
        const size_t C = D.c_out, n_in = (size_t)B * D.c_in * hw, n_out = (size_t)B * D.c_out * hw;
        bool ok = true;
        if (mode != MZL_FUSED_FINALIZE) {
            ok = dc.down(J.out, D.out, n_out) && dc.down(J.mat_out, D.mat, n_in);
            if (J.stat_mode != ST_NONE) ok = ok && dc.down(J.part, D.part, (size_t)D.groups * D.cpo * (J.stat_mode == ST_FWD ? 4 : 2));
        }
        if (J.finalize) ok = ok && dc.down(J.coef_out, D.coef_out, (size_t)3 * D.cpo);
        if (J.finalize == 1) ok = ok && dc.down(J.save_out, D.save_out, (size_t)2 * D.cpo) && dc.down(J.running_mean, D.rm, C) && dc.down(J.running_var, D.rv, C) && dc.down(J.num_batches, D.nbt, 1);
        if (J.finalize == 2) ok = ok && dc.down(J.dgamma, D.dgamma, C) && dc.down(J.dbeta, D.dbeta, C);
        if (!ok) return dc.fail(MZL_E_HIP, "hipMemcpy failed");
    }
    const mzl_fused_conv& J0 = c->conv[0];
    if (mode == MZL_FUSED_FINALIZE) {
        dc.name(build_name, "%s %s groups=%d C=%d cpad=%d accumulate=%d", prec, J0.finalize == 1 ? "k_lc_bn_fwd" : "k_lc_bn_bwd", d[0].groups, d[0].c_out, d[0].cpo, J0.accumulate ? 1 : 0);
    } else {
        static const char* in_names[4] = {"IN_IDENT", "IN_BNRELU", "IN_BNBWD", "IN_BNRES"};
        static const char* st_names[3] = {"ST_NONE", "ST_FWD", "ST_BWD"};
        static const char* fin_names[3] = {"none", "fwd", "bwd"};
        const Op& o = ops[0][0];
        int z = cdiv(o.conv.co_tiles, 4);
        if (nj == 2 && cdiv(ops[1][0].conv.co_tiles, 4) > z) z = cdiv(ops[1][0].conv.co_tiles, 4);
        c->groups = d[0].groups;
        dc.name(build_name, "%s %s NPT=%d SIDE=%d G=%d groups=%d z=%d mode=%s stat=%s dir=%s pair=%d fin=%s", prec, h->split ? "k_lc_conv_bf16x3" : "k_lc_conv", o.npt, o.side15 ? 15 : 0,
                o.conv.G, d[0].groups, z, in_names[J0.in_mode], st_names[J0.stat_mode], J0.direction == 0 ? "forward" : "dgrad", nj == 2 ? 1 : 0, fin_names[J0.finalize]);
    }
    return MZL_OK;
}

// diagnostic (tests): the head block ALONE -- k_lc_pack_lin through pack_lin, then launch_heads, the function mzlc_grad calls -- on host-supplied tower
// outputs, head parameters, running statistics, targets, rows and weights.  P, hw, A, K and the support sizes are the handle's.  Every buffer is a
// temporary one of this call (NULL stream; outputs preset to NaN bits, so an element no kernel wrote shows): the handle's weights, saved tensors,
// gradients and running statistics are not touched.  Layouts: mz_learn_conv_host.h.
int mzlc_debug_heads(mzlc_learner* h, const mzl_heads_call* c, std::string& err) {
    const int B = c->batch, K = h->K, ng = 3 * K, hw = h->hw, P = h->P;
    if (B < 1 || B > h->maxB) { err = "batch must be in [1, max_batch]"; return MZL_E_INVALID; }
    if (c->rows < 1 || c->rows > (1 << 24)) { err = "rows (of the target tables) must be in [1, 2^24]"; return MZL_E_INVALID; }
    if (!c->F_pred || !c->F_rew || !c->params || !c->running || !c->nbt || !c->pi || !c->value || !c->reward || !c->idx || !c->w) {
        err = "null argument (F_pred, F_rew, params, running, nbt, pi, value, reward, idx, w)";
        return MZL_E_INVALID;
    }
    for (int b = 0; b < B; b++)
        if (c->idx[b] < 0 || c->idx[b] >= c->rows) { err = "idx out of [0, rows)"; return MZL_E_INVALID; }
    if (hipSetDevice(h->device) != hipSuccess) { err = "hipSetDevice"; return MZL_E_HIP; }
    // the heads with offsets into this call's compact vectors: per head (reward, policy, value) w1, gamma, beta, lw, lb; running mean, variance
    LchHead head[3];
    int lwT_off[3], np = 0, nr = 0, nl = 0;
    for (int i = 0; i < 3; i++) {
        LchHead H = h->head[i];
        const int nf = H.oc * hw;
        H.w1_off = np; np += H.oc * P;
        H.gamma_off = np; np += H.oc;
        H.beta_off = np; np += H.oc;
        H.lw_off = np; np += H.n_out * nf;
        H.lb_off = np; np += H.n_out;
        H.rm_off = nr; nr += H.oc;
        H.rv_off = nr; nr += H.oc;
        H.nbt_idx = i;
        lwT_off[i] = nl; nl += H.n_out * nf;
        head[i] = H;
    }
    DebugCall dc(h, err);
    const size_t nF = (size_t)K * B * P * hw, gb = (size_t)ng * B;
    float *dFp = nullptr, *dFr = nullptr, *d_params = nullptr, *d_running = nullptr, *d_pi = nullptr, *d_value = nullptr, *d_reward = nullptr, *d_w = nullptr, *d_lwT = nullptr;
    int64_t *d_nbt = nullptr, *d_idx = nullptr;
    LchGroup* d_groups = nullptr;
    HeadBufs hb{};
    float *spart_fwd = nullptr, *d_prio = nullptr;
    bool ok = dc.up(&dFp, c->F_pred, nF) && dc.up(&dFr, c->F_rew, nF) && dc.up(&d_params, c->params, (size_t)np) && dc.up(&d_running, c->running, (size_t)nr) && dc.up(&d_nbt, c->nbt, 3) &&
              dc.up(&d_pi, c->pi, (size_t)c->rows * K * h->A) && dc.up(&d_value, c->value, (size_t)c->rows * K) && dc.up(&d_reward, c->reward, (size_t)c->rows * K) &&
              dc.up(&d_idx, c->idx, (size_t)B) && dc.up(&d_w, c->w, (size_t)B) && dc.zeros(&d_lwT, (size_t)nl) && dc.zeros(&d_groups, (size_t)ng);
    ok = ok && dc.nanbuf(&hb.grads, np) && dc.nanbuf(&hb.u, gb * LCH_MAXOC * hw) && dc.nanbuf(&hb.dzb, gb * LCH_MAXOC * hw) && dc.nanbuf(&hb.feat, gb * LCH_MAXOC * hw) &&
         dc.nanbuf(&hb.dlogit, gb * h->n_max) && dc.nanbuf(&hb.spart, gb * LCH_MAXOC * 2) && dc.nanbuf(&spart_fwd, gb * LCH_MAXOC * 2) && dc.nanbuf(&hb.spiv, gb * LCH_MAXOC) &&
         dc.nanbuf(&hb.coef, (size_t)ng * LCH_MAXOC * 5) && dc.nanbuf(&hb.save, (size_t)ng * LCH_MAXOC * 2) && dc.nanbuf(&hb.lpart, gb) && dc.nanbuf(&hb.wpart, (size_t)K * h->hp_total) &&
         dc.nanbuf(&hb.dF_pred, nF) && dc.nanbuf(&hb.dF_rew, nF) && dc.nanbuf(&hb.loss, 1) && dc.nanbuf(&d_prio, B);
    if (!ok) return dc.fail(MZL_E_HIP, "hipMalloc / hipMemcpy failed");
    std::vector<LchGroup> groups(ng);
    for (int t = 0; t < K; t++) {  // (as mzlc_grad orders them)
        groups[3 * t + 0] = LchGroup{dFr + (size_t)t * B * P * hw, 0, t};
        groups[3 * t + 1] = LchGroup{dFp + (size_t)t * B * P * hw, 1, t};
        groups[3 * t + 2] = LchGroup{dFp + (size_t)t * B * P * hw, 2, t};
    }
    if (!dc.put(d_groups, groups.data(), (size_t)ng)) return dc.fail(MZL_E_HIP, "hipMemcpy failed");
    hipStream_t st = nullptr;
    pack_lin(head, lwT_off, hw, d_params, d_lwT, st);
    hb.head = head; hb.lwT_off = lwT_off; hb.groups = d_groups; hb.params = d_params; hb.running = d_running; hb.nbt = d_nbt; hb.lwT = d_lwT; hb.spart_fwd = spart_fwd;
    LcBatch bt{};
    bt.pi = d_pi; bt.value = d_value; bt.reward = d_reward; bt.idx = d_idx; bt.w = d_w; bt.prio = d_prio; bt.B = B; bt.K = K; bt.A = h->A;
    launch_heads(h, hb, bt, st);
    if (!dc.ran()) return dc.fail(MZL_E_HIP, "the head kernels failed to launch or run");
    ok = dc.down(c->u, hb.u, gb * LCH_MAXOC * hw) && dc.down(c->spart_fwd, spart_fwd, gb * LCH_MAXOC * 2) && dc.down(c->spiv, hb.spiv, gb * LCH_MAXOC) &&
         dc.down(c->coef, hb.coef, (size_t)ng * LCH_MAXOC * 5) && dc.down(c->save, hb.save, (size_t)ng * LCH_MAXOC * 2) && dc.down(c->feat, hb.feat, gb * LCH_MAXOC * hw) &&
         dc.down(c->dlogit, hb.dlogit, gb * h->n_max) && dc.down(c->dzb, hb.dzb, gb * LCH_MAXOC * hw) && dc.down(c->spart_bwd, hb.spart, gb * LCH_MAXOC * 2) &&
         dc.down(c->lpart, hb.lpart, gb) && dc.down(c->loss, hb.loss, 1) && dc.down(c->prio, d_prio, (size_t)B) && dc.down(c->running_out, d_running, (size_t)nr) &&
         dc.down(c->nbt_out, d_nbt, 3) && dc.down(c->dF_pred, hb.dF_pred, nF) && dc.down(c->dF_rew, hb.dF_rew, nF) && dc.down(c->wpart, hb.wpart, (size_t)K * h->hp_total) &&
         dc.down(c->grads, hb.grads, (size_t)np);
    return ok ? MZL_OK : dc.fail(MZL_E_HIP, "hipMemcpy failed");
}
