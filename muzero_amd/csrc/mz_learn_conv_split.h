// mz_learn_conv_split.h -- the opt-in split-bf16 3x3 conv of the conv-net learners (board nets: mzl_config.conv_precision == MZL_CONV_BF16X3, every
// tower; the Atari net: mzl_set_atari_precision, per group of layers) for gfx950: k_lc_conv's job -- forward convs and data gradients -- on
// v_mfma_f32_16x16x32_bf16 instead of v_mfma_f32_16x16x4_f32.
//
// A float32 is exactly the sum of three bf16 values (mz_split3.h), so a float32-grade product is six bf16 products accumulated in float32: hh, hm,
// mh, hl, lh, mm (the three dropped cross terms are below 2^-24 of the product).  What k_lc_conv_bf16x3 keeps of k_lc_conv, bit for bit:
//   * the staging transform (BatchNorm + ReLU | block output relu(a y2 + b + x) | BatchNorm backward from two tensors | action planes) is the same
//     float32 code, and the mat_out write-through stores ITS result: the masks, the saved tensors and k_lc_wgrad's inputs are what they are in the
//     f32 path given the same conv outputs;
//   * the epilogue (statistics around the pivot, skip, mask, ST_BWD sums, 16-byte stores) is k_lc_conv's, in float32 on the float32 accumulators;
//   * the job description (Pair<LcConv>), the grid and the pixel tilings (NPT, G images per workgroup, the 15 x 15 SIDE build).
// What differs: the transformed value is split AFTER the transform, while it is written to LDS, in the planner kernel's layout
//     slab[term h, m, l][channel octet q][position][8 bf16]                        (32-channel blocks; a position is one of the G haloed image planes)
// -- lane (q = lane >> 4, j = lane & 15) of the MFMA reads pixel j's 16 bytes of octet q.  192 bytes per position: 55.5 KB at 15 x 15, so two
// workgroups per CU still fit; the slab is single-buffered, the next block's values wait in registers while this block's MFMAs run (wave w stages
// octet w: channels 32 cb + 8 w + c; lane = pixel quad, as in k_lc_conv).  Weights: three bf16 fragment streams per (output-channel tile, 32-channel
// block, tap), zero-padded to 32 input channels, packed on the GPU by k_lc_pack_bf16x3 (one copy per orientation) and read from L2 one or two steps ahead.
// LcConv::w points at that copy and LcConv::n_cb counts 32-channel blocks in this path.
// ONE summation order in every build -- (32-channel block, tap, term hh, hm, mh, hl, lh, mm), channel 32 cb + k in k slot k of a step: the generic
// and the SIDE build give the same bits, and so do the tile-path builds (HALO, PLANE: the Atari net's 48 x 48 and 24 x 24 stages, mzl_set_atari_precision).
// No TAPMASK builds: the stride-2 parity planes stay float32.
#pragma once
#include "mz_learn_conv.h"
#include "mz_split3.h"

namespace mzlc {

typedef __bf16 lc_bf16x8 __attribute__((ext_vector_type(8)));

// dynamic LDS of k_lc_conv_bf16x3: the slab of G haloed planes + the staging coefficients
inline size_t conv_split_lds(int G, int h, int w, int cpad_in) { return (size_t)192 * G * (h + 2) * (w + 2) + (size_t)3 * cpad_in * sizeof(float); }

// HALO / PLANE: the tile path of the Atari net's representation (LcConv::halo_in / out_plane, k_lc_conv's PLANE build), identity staging only.
// HALO: in0 holds the (h + 2) x (w + 2) positions of a tile WITH its halo in the slab's own row pitch, so the staging is a linear copy of the
// tile -- a lane's quad is four consecutive slab positions and may run over a row end, ring positions included -- and only the h x w inner
// positions are computed.  PLANE: the epilogue writes them (and reads skip / mask / partner) at their place in planes [B][cout][pl_h][pl_w].
// Neither touches the k loop: a tile-path conv sums in the order of every other build.
template <int NPT, int MODE, int SIDE, bool HALO = false, bool PLANE = false>
__global__ __launch_bounds__(256, 2) void k_lc_conv_bf16x3(const Pair<LcConv> PJ) {
    static_assert(!HALO || (MODE == IN_IDENT && SIDE == 0), "the tile path stages gathered tiles: identity, one tile per workgroup");
    static_assert(!PLANE || HALO, "the plane epilogue belongs to the halo_in builds");
    const bool second = (int)blockIdx.y >= PJ.na;
    LcConv L = second ? PJ.b : PJ.a;
    if constexpr (SIDE > 0) { L.h = SIDE; L.w_img = SIDE; L.G = 1; }
    if constexpr (HALO) L.G = 1;
    L.in_mode = MODE;
    const int by = second ? (int)blockIdx.y - PJ.na : (int)blockIdx.y;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    u32x4* slab = reinterpret_cast<u32x4*>(smem);  // [3 terms][4 octets][npos]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), q = lane >> 4, j = lane & 15;
    const int hw = L.h * L.w_img, siw = L.w_img + 2, plane = (L.h + 2) * siw;
    const int npos = L.G * plane, tstr = 4 * npos;
    float* s_coef = reinterpret_cast<float*>(slab + 3 * tstr);  // [3][cpad_in]
    const int img0 = by * L.G;
    const int QP = (hw + 3) >> 2;
    const float r_qp = 1.0f / (float)QP, r_iw = 1.0f / (float)L.w_img, r_hw = 1.0f / (float)hw;
    const __amdgpu_buffer_rsrc_t rs_in0 = mkrs(L.in0), rs_in1 = mkrs(L.in1 ? L.in1 : L.in0), rs_mat = mkrs(L.mat_out ? L.mat_out : L.in0);
    // ---- staging plan: lane t of every wave owns pixel quad t of the group (k_lc_conv's); wave w the channel octet w of each 32-channel block ----
    const int in_hw = HALO ? plane : hw;  // positions per image and channel of in0
    const int QPs = HALO ? (plane + 3) >> 2 : QP;
    const float r_qps = HALO ? 1.0f / (float)QPs : r_qp;
    const int sg = lc_idiv(lane, r_qps), qd = lane - sg * QPs, p0 = qd * 4, bimg = img0 + sg;
    const bool w_ok = lane < L.G * QPs && bimg < L.B;
    const int cimg = bimg < L.B ? bimg : L.B - 1;
    const unsigned w_voff = (unsigned)(((size_t)cimg * L.cin_real * in_hw + (size_t)(w_ok ? p0 : 0)) * sizeof(float));
    const int w_act = (w_ok && L.action) ? L.action[cimg] : -1;
    int w_spos[4], w_pm[4];  // slab position (16-byte words, octet plane included) of the quad's pixels, or -1
#pragma unroll
    for (int e = 0; e < 4; e++) {
        const int pp = p0 + e, py = lc_idiv(pp, r_iw), px = pp - py * L.w_img;
        w_spos[e] = (w_ok && pp < in_hw) ? (sg < L.G ? sg : 0) * plane + (HALO ? pp : (py + 1) * siw + px + 1) + wave * npos : -1;
        w_pm[e] = L.cin > L.cin_real ? pp % L.num_actions : 0;
    }
    constexpr bool TWO = MODE == IN_BNBWD || MODE == IN_BNRES;
    float4 sv0[8], sv1[TWO ? 8 : 1];  // [c]: channel 32 cb + 8 wave + c of the block in flight, pixels p0 .. p0 + 3
    auto fetch = [&](int cb) {
#pragma unroll
        for (int c = 0; c < 8; c++) {
            const int ch = cb * 32 + 8 * wave + c, chc = ch < L.cin_real ? ch : 0;
            sv0[c] = ld4(rs_in0, w_voff, chc * in_hw * (int)sizeof(float));
            if constexpr (TWO) sv1[c] = ld4(rs_in1, w_voff, chc * in_hw * (int)sizeof(float));
        }
    };
    auto transform_store = [&](int cb) {
        float v[8][4];
#pragma unroll
        for (int c = 0; c < 8; c++) {
            const int ch = cb * 32 + 8 * wave + c;  // wave-uniform
            const float x[4] = {sv0[c].x, sv0[c].y, sv0[c].z, sv0[c].w};
            if (ch < L.cin_real) {  // k_lc_conv's transforms, operation for operation (same bits)
                if constexpr (MODE == IN_BNRELU) {
                    const float a = s_coef[ch], b = s_coef[L.cpad_in + ch];
#pragma unroll
                    for (int e = 0; e < 4; e++) {
                        const float t = fmaf(a, x[e], b);
                        v[c][e] = t > 0.0f ? t : 0.0f;
                    }
                } else if constexpr (MODE == IN_BNBWD) {
                    const float c1 = s_coef[ch], c2 = s_coef[L.cpad_in + ch], c3 = s_coef[2 * L.cpad_in + ch];
                    const float y[4] = {sv1[c].x, sv1[c].y, sv1[c].z, sv1[c].w};
#pragma unroll
                    for (int e = 0; e < 4; e++) v[c][e] = fmaf(c1, x[e], fmaf(c2, y[e], c3));
                } else if constexpr (MODE == IN_BNRES) {
                    const float a = s_coef[ch], b = s_coef[L.cpad_in + ch];
                    const float r[4] = {sv1[c].x, sv1[c].y, sv1[c].z, sv1[c].w};
#pragma unroll
                    for (int e = 0; e < 4; e++) {
                        const float t = fmaf(a, x[e], b) + r[e];
                        v[c][e] = t > 0.0f ? t : 0.0f;
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < 4; e++) v[c][e] = x[e];
                }
            } else {  // action planes (flat element f = c * hw + pixel of the [A, h, w] block is 1 iff f % A == action), or the padding to 32 channels
                const int t = ch < L.cin ? (int)(((long long)(ch - L.cin_real) * hw) % L.num_actions) : 0;
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    int m = w_pm[e] + t;
                    m = m >= L.num_actions ? m - L.num_actions : m;
                    v[c][e] = (ch < L.cin && m == w_act) ? 1.0f : 0.0f;
                }
            }
        }
        // the split: after the transform, on the way into LDS -- pixel e's 8 channels are one 16-byte word of each term plane
#pragma unroll
        for (int e = 0; e < 4; e++) {
            unsigned hb[8], mb[8], lb[8];
#pragma unroll
            for (int c = 0; c < 8; c++) mz::conv_split3(v[c][e], hb[c], mb[c], lb[c]);
            if (w_spos[e] >= 0) {
                u32x4* d = slab + w_spos[e];
                d[0] = u32x4{hb[0] | (hb[1] << 16), hb[2] | (hb[3] << 16), hb[4] | (hb[5] << 16), hb[6] | (hb[7] << 16)};
                d[tstr] = u32x4{mb[0] | (mb[1] << 16), mb[2] | (mb[3] << 16), mb[4] | (mb[5] << 16), mb[6] | (mb[7] << 16)};
                d[2 * tstr] = u32x4{lb[0] | (lb[1] << 16), lb[2] | (lb[3] << 16), lb[4] | (lb[5] << 16), lb[6] | (lb[7] << 16)};
            }
        }
        if ((MODE == IN_BNRES || MODE == IN_BNRELU) && L.mat_out && blockIdx.z == 0 && w_ok) {  // write-through of the FLOAT32 value, as k_lc_conv's
#pragma unroll
            for (int c = 0; c < 8; c++) {
                const int ch = cb * 32 + 8 * wave + c;
                if (ch < L.cin_real) {
                    float* o = L.mat_out + ((size_t)cimg * L.cin_real + ch) * hw + p0;
                    if (p0 + 3 < hw) {
                        __builtin_amdgcn_raw_buffer_store_b128(u32x4{__float_as_uint(v[c][0]), __float_as_uint(v[c][1]), __float_as_uint(v[c][2]), __float_as_uint(v[c][3])},
                                                               rs_mat, w_voff, ch * hw * (int)sizeof(float), 0);
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; e++)
                            if (p0 + e < hw) o[e] = v[c][e];
                    }
                }
            }
        }
    };
    // ---- A-operand rows of this lane: pixel slot p = pt * 16 + j -> image g of the group, pixel (py, px); octet q ----
    int off[NPT];
#pragma unroll
    for (int pt = 0; pt < NPT; pt++) {
        const int p = pt * 16 + j, g = lc_idiv(p, r_hw), pp = p - g * hw, py = lc_idiv(pp, r_iw), px = pp - py * L.w_img;
        off[pt] = (g < L.G ? g * plane + py * siw + px : 0) + q * npos;
    }
    f32x4 acc[NPT];
#pragma unroll
    for (int pt = 0; pt < NPT; pt++) acc[pt] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int cot = blockIdx.z * 4 + wave, ctc = cot < L.co_tiles ? cot : L.co_tiles - 1;
    const __amdgpu_buffer_rsrc_t rs_w = mkrs(L.w);
    const int wbase = ctc * L.n_cb * 9 * 3072, n_steps = L.n_cb * 9;  // 3072 bytes per step: [term][64 lanes] x 8 bf16
    struct W3 { u32x4 t[3]; };
    auto wload = [&](int step) {
        const int sc = step < n_steps ? step : n_steps - 1;
        W3 r;
#pragma unroll
        for (int t = 0; t < 3; t++) r.t[t] = __builtin_amdgcn_raw_buffer_load_b128(rs_w, lane * 16, wbase + sc * 3072 + t * 1024, 0);
        return r;
    };
    // the first weights and the first block are requested BEFORE the LDS fill below: their latency runs under it
    constexpr int WAHEAD = NPT >= 13 ? 1 : 2;  // weight steps in flight: a step of the large tilings is >= 78 MFMAs, and their builds have no registers to spare
    W3 w1 = wload(0), w2 = wload(WAHEAD == 2 ? 1 : 0);
    fetch(0);
    for (int i = tid; i < 3 * tstr; i += 256) slab[i] = u32x4{0u, 0u, 0u, 0u};  // halo, unused positions and images past the batch stay zero
    if (MODE != IN_IDENT)
        for (int i = tid; i < 3 * L.cpad_in; i += 256) s_coef[i] = L.coef[i];
    __syncthreads();
    transform_store(0);
    __syncthreads();
    auto tap_step = [&](int step, int toff) {
        const lc_bf16x8 wh = __builtin_bit_cast(lc_bf16x8, w1.t[0]), wm = __builtin_bit_cast(lc_bf16x8, w1.t[1]), wl = __builtin_bit_cast(lc_bf16x8, w1.t[2]);
        if constexpr (WAHEAD == 2) {
            w1 = w2;
            w2 = wload(step + 2);
        } else {
            w1 = wload(step + 1);
        }
#pragma unroll
        for (int pt = 0; pt < NPT; pt++) {
            const u32x4* a = slab + off[pt] + toff;
            const lc_bf16x8 xh = __builtin_bit_cast(lc_bf16x8, a[0]), xm = __builtin_bit_cast(lc_bf16x8, a[tstr]), xl = __builtin_bit_cast(lc_bf16x8, a[2 * tstr]);
            // the term order of every build: hh, hm, mh, hl, lh, mm
            acc[pt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xh, wh, acc[pt], 0, 0, 0);
            acc[pt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xh, wm, acc[pt], 0, 0, 0);
            acc[pt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xm, wh, acc[pt], 0, 0, 0);
            acc[pt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xh, wl, acc[pt], 0, 0, 0);
            acc[pt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xl, wh, acc[pt], 0, 0, 0);
            acc[pt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xm, wm, acc[pt], 0, 0, 0);
        }
    };
    for (int cb = 0; cb < L.n_cb; cb++) {
        if (cb + 1 < L.n_cb) fetch(cb + 1);  // (workgroup-uniform)
#pragma unroll 1
        for (int tap = 0; tap < 9; tap++) {  // (not unrolled: nine unrolled taps let the scheduler hoist LDS reads until the two-tensor builds spill)
            const int ky = tap / 3;
            tap_step(cb * 9 + tap, ky * siw + (tap - 3 * ky));
        }
        __syncthreads();  // every wave has read this block's slab
        if (cb + 1 < L.n_cb) transform_store(cb + 1);
        __syncthreads();
    }
    // ---- epilogue: k_lc_conv's (PLANE: its out_plane build's), on the float32 accumulators: lane (q, j) holds pixel slots pt * 16 + 4 q + r
    // (r = 0..3) of output channel 16 cot + j ----
    if (cot >= L.co_tiles) return;  // wave-uniform (no barrier below)
    const int co = cot * 16 + j;
    const bool co_ok = co < L.cout;
    const __amdgpu_buffer_rsrc_t rs_out = mkrs(L.out), rs_skip = mkrs(L.skip ? L.skip : L.out), rs_mask = mkrs(L.mask ? L.mask : L.out),
                                 rs_part = mkrs(L.partner ? L.partner : L.out);
    // (PLANE: the workgroup's image is tile (tyi, txi) of plane image pimg; offsets stay below 4 GiB: the launcher checks the plane tensor's size)
    const int pl_nt = PLANE ? L.pl_nty * L.pl_ntx : 1;
    const int pimg = PLANE ? img0 / pl_nt : 0, ptl = PLANE ? img0 - pimg * pl_nt : 0, tyi = PLANE ? ptl / L.pl_ntx : 0, txi = PLANE ? ptl - tyi * L.pl_ntx : 0;
    const int pl_hw = L.pl_h * L.pl_w;
    const unsigned soff = PLANE ? (unsigned)(((size_t)pimg * L.cout * pl_hw + (size_t)(tyi * L.h) * L.pl_w + (size_t)txi * L.w_img) * sizeof(float))
                                : (unsigned)((size_t)img0 * L.cout * hw * sizeof(float));
    float ma = 1.0f, mb = 0.0f;
    if (L.mask && L.mcoef && co_ok) { ma = L.mcoef[co]; mb = L.mcoef[L.cpad_out + co]; }
    const bool part_is_mask = L.partner == L.mask;
    float s1 = 0.0f, s2 = 0.0f;
    // ST_FWD: the batch statistics are summed around a PIVOT, the workgroup's first output of the channel (see k_lc_conv)
    const bool st_fwd = L.stat_mode == ST_FWD;
    const float pvt = st_fwd ? __shfl(acc[0][0], j) : 0.0f;
    const int nimg = (img0 + L.G <= L.B) ? L.G : (L.B - img0 > 0 ? L.B - img0 : 0);
    if (st_fwd) {
        const int nvalid = nimg * hw;
#pragma unroll
        for (int pt = 0; pt < NPT; pt++) {
            if ((pt + 1) * 16 <= nvalid) {
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const float u = acc[pt][r] - pvt;
                    s1 += u;
                    s2 = fmaf(u, u, s2);
                }
            } else {
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const float u = (pt * 16 + 4 * q + r) < nvalid ? acc[pt][r] - pvt : 0.0f;
                    s1 += u;
                    s2 = fmaf(u, u, s2);
                }
            }
        }
    }
    constexpr int EC = NPT < 3 ? NPT : 3;
    constexpr int NB = (NPT + EC - 1) / EC;
    // regular batches of EC tiles (every lane's four slots one whole quad of one image): unconditional 16-byte operand loads, issued one batch ahead
    const bool quads_whole = (hw & 3) == 0;
    int nfast = 0;
#pragma unroll
    for (int it = 0; it < NB; it++)
        if (nfast == it && (quads_whole || (L.G == 1 && (it * EC + EC) * 16 <= hw))) nfast = it + 1;
    if (MZLC_EPI_PIPE == 0) nfast = 0;
    struct Bt { f32x4 kv[EC], mv[EC], yv[EC]; unsigned vo[EC]; bool valid[EC]; };
    auto issue = [&](int pb, Bt& b) {
#pragma unroll
        for (int e = 0; e < EC; e++) {
            const int p = (pb + e) * 16 + 4 * q;
            const int g = lc_idiv(p, r_hw), pp = p - g * hw;
            b.valid[e] = co_ok && (pb + e < NPT) && (g < L.G) && (img0 + g < L.B);
            const int gs = b.valid[e] ? g : 0, cs = co_ok ? co : 0, ps = b.valid[e] ? pp : 0;  // (a real address for every lane)
            if constexpr (PLANE) {
                const int py = lc_idiv(ps, r_iw), px = ps - py * L.w_img;
                b.vo[e] = (unsigned)(cs * pl_hw + py * L.pl_w + px) * (unsigned)sizeof(float);
            } else
            b.vo[e] = (unsigned)((gs * L.cout + cs) * hw + ps) * (unsigned)sizeof(float);
            b.kv[e] = b.mv[e] = b.yv[e] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (pb + e < NPT) {
                if (L.skip) { const float4 t = ld4(rs_skip, b.vo[e], soff); b.kv[e] = f32x4{t.x, t.y, t.z, t.w}; }
                if (L.mask) { const float4 t = ld4(rs_mask, b.vo[e], soff); b.mv[e] = f32x4{t.x, t.y, t.z, t.w}; }
                if (L.partner && !part_is_mask) { const float4 t = ld4(rs_part, b.vo[e], soff); b.yv[e] = f32x4{t.x, t.y, t.z, t.w}; }
            }
        }
    };
    auto finish = [&](int pb, const Bt& b) {
#pragma unroll
        for (int e = 0; e < EC; e++) {
            if (pb + e >= NPT) continue;
            f32x4 v = acc[pb + e];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                float t = v[r] + (b.valid[e] ? b.kv[e][r] : 0.0f);
                const float mvr = b.valid[e] ? b.mv[e][r] : 0.0f;
                if (L.mask && !(fmaf(ma, mvr, mb) > 0.0f)) t = 0.0f;
                if (!b.valid[e]) t = 0.0f;
                const float pv = b.valid[e] ? (part_is_mask ? b.mv[e][r] : b.yv[e][r]) : 0.0f;
                if (L.stat_mode == ST_BWD) {
                    s1 += t;
                    s2 = fmaf(t, pv, s2);
                }
                v[r] = t;
            }
            if (b.valid[e])
                __builtin_amdgcn_raw_buffer_store_b128(u32x4{__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3])}, rs_out,
                                                       b.vo[e], soff, 0);
        }
    };
    Bt bt[2];
    if (nfast > 0) issue(0, bt[0]);
#pragma unroll
    for (int it = 0; it < NB; it++) {
        const int pb = it * EC;
        if (it < nfast) {
            if (it + 1 < nfast) issue(pb + EC, bt[(it + 1) & 1]);
            __builtin_amdgcn_sched_barrier(0);
            finish(pb, bt[it & 1]);
            __builtin_amdgcn_sched_barrier(0);
            continue;
        }
        unsigned vo[EC][4];
        bool ok[EC][4], vec[EC];
        f32x4 kv[EC], mv[EC], yv[EC];
#pragma unroll
        for (int e = 0; e < EC; e++) {
            const int pt = pb + e < NPT ? pb + e : NPT - 1;
            const int p = pt * 16 + 4 * q;
            int g = lc_idiv(p, r_hw), pp = p - g * hw;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                ok[e][r] = co_ok && (pb + e < NPT) && (g < L.G) && (img0 + g < L.B);
                if constexpr (PLANE) {
                    const int py = lc_idiv(pp, r_iw), px = pp - py * L.w_img;
                    vo[e][r] = (unsigned)(co * pl_hw + py * L.pl_w + px) * (unsigned)sizeof(float);
                } else
                vo[e][r] = (unsigned)((g * L.cout + co) * hw + pp) * (unsigned)sizeof(float);
                pp++;
                if (pp == hw) { pp = 0; g++; }
            }
            vec[e] = ok[e][0] && ok[e][1] && ok[e][2] && ok[e][3] && vo[e][3] == vo[e][0] + 12;
            kv[e] = mv[e] = yv[e] = f32x4{0.f, 0.f, 0.f, 0.f};
            auto ldv = [&](const __amdgpu_buffer_rsrc_t rs, f32x4& d) {
                if (vec[e]) {
                    const float4 t = ld4(rs, vo[e][0], soff);
                    d = f32x4{t.x, t.y, t.z, t.w};
                } else {
#pragma unroll
                    for (int r = 0; r < 4; r++)
                        if (ok[e][r]) d[r] = ld1(rs, vo[e][r], soff);
                }
            };
            if (L.skip) ldv(rs_skip, kv[e]);
            if (L.mask) ldv(rs_mask, mv[e]);
            if (L.partner && !part_is_mask) ldv(rs_part, yv[e]);
        }
#pragma unroll
        for (int e = 0; e < EC; e++) {
            if (pb + e >= NPT) continue;
            f32x4 v = acc[pb + e];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                float t = v[r] + kv[e][r];
                if (L.mask && !(fmaf(ma, mv[e][r], mb) > 0.0f)) t = 0.0f;
                if (!ok[e][r]) t = 0.0f;
                const float pv = part_is_mask ? mv[e][r] : yv[e][r];
                if (L.stat_mode == ST_BWD) {
                    s1 += t;
                    s2 = fmaf(t, pv, s2);
                }
                v[r] = t;
            }
            if (vec[e]) {
                __builtin_amdgcn_raw_buffer_store_b128(u32x4{__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3])}, rs_out,
                                                       vo[e][0], soff, 0);
            } else {
#pragma unroll
                for (int r = 0; r < 4; r++)
                    if (ok[e][r]) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[r]), rs_out, vo[e][r], soff, 0);
            }
        }
    }
    if (L.stat_mode != ST_NONE) {  // the four lane groups q hold disjoint pixels of channel j: (q0 + q1) + (q2 + q3)
        s1 += __shfl_xor(s1, 16); s2 += __shfl_xor(s2, 16);
        s1 += __shfl_xor(s1, 32); s2 += __shfl_xor(s2, 32);
        if (q == 0 && co < L.cpad_out) {
            if (st_fwd) {
                *reinterpret_cast<float4*>(L.stat_part + ((size_t)by * L.cpad_out + co) * 4) = make_float4(co_ok ? pvt : 0.0f, s1, s2, co_ok ? (float)(nimg * hw) : 0.0f);
            } else {
                float* d = L.stat_part + ((size_t)by * L.cpad_out + co) * 2;
                d[0] = s1; d[1] = s2;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Operand copies of the split path: three bf16 fragment streams per (output-channel tile, 32-channel block, tap), in consumption order --
// word [ct][cb][tap][term][lane = (q, j)] holds W_term[co = 16 ct + j][ci = 32 cb + 8 q + k][tap], k = 0..7 (k = 0 in the low half of the first
// dword, as the slab's words), zero beyond the layer's channels.  The data gradient's copy: "output" channel = the layer's input channel,
// "input" = its output channel, taps flipped.  Offsets in 16-byte words.
// ---------------------------------------------------------------------------------------------------------------------------------
struct LcPackSplitJob {
    int w_off;             // master weight [cout][cin][3][3] in params
    int cout, cin, cin_d;  // cin_d: input channels that receive a gradient, 0: no data-gradient copy
    long long f_off, d_off;  // word offsets of the forward / data-gradient copies
    int n_cb, co_tiles;      // forward: 32-blocks of cin, 16-tiles of cout
    int n_cb_d, co_tiles_d;  // data gradient: 32-blocks of cout, 16-tiles of cin_d
};
__global__ __launch_bounds__(256) void k_lc_pack_bf16x3(const LcPackSplitJob* jobs, const float* params, u32x4* packed) {
    const LcPackSplitJob J = jobs[blockIdx.y];
    const int nf = J.co_tiles * J.n_cb * 9 * 64, nd = J.co_tiles_d * J.n_cb_d * 9 * 64;  // (lane, step) pairs
    for (int e = blockIdx.x * 256 + threadIdx.x; e < nf + nd; e += gridDim.x * 256) {
        const bool fwd = e < nf;
        const int x = fwd ? e : e - nf;
        const int lane = x & 63, step = x >> 6;
        const int ncb = fwd ? J.n_cb : J.n_cb_d;
        const int tap = step % 9, cb = (step / 9) % ncb, ct = step / (9 * ncb);
        const int q = lane >> 4, jj = lane & 15;
        unsigned hb[8], mb[8], lb[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            float v = 0.0f;
            if (fwd) {
                const int co = 16 * ct + jj, ci = 32 * cb + 8 * q + k;
                if (co < J.cout && ci < J.cin) v = params[J.w_off + ((size_t)co * J.cin + ci) * 9 + tap];
            } else {
                const int ci = 16 * ct + jj, co = 32 * cb + 8 * q + k;
                if (co < J.cout && ci < J.cin_d) v = params[J.w_off + ((size_t)co * J.cin + ci) * 9 + (8 - tap)];
            }
            mz::conv_split3(v, hb[k], mb[k], lb[k]);
        }
        u32x4* d = packed + (fwd ? J.f_off : J.d_off) + (size_t)step * 192 + lane;
        d[0] = u32x4{hb[0] | (hb[1] << 16), hb[2] | (hb[3] << 16), hb[4] | (hb[5] << 16), hb[6] | (hb[7] << 16)};
        d[64] = u32x4{mb[0] | (mb[1] << 16), mb[2] | (mb[3] << 16), mb[4] | (mb[5] << 16), mb[6] | (mb[7] << 16)};
        d[128] = u32x4{lb[0] | (lb[1] << 16), lb[2] | (lb[3] << 16), lb[4] | (lb[5] << 16), lb[6] | (lb[7] << 16)};
    }
}

}  // namespace mzlc
