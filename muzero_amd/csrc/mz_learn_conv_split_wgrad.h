// mz_learn_conv_split_wgrad.h -- the opt-in split-bf16 weight gradient of the board-net learner (mzl_set_wgrad_precision(MZL_WGRAD_BF16X3)) for gfx950:
// k_lc_wgrad<ACT, RING = false>'s job on v_mfma_f32_16x16x32_bf16 instead of v_mfma_f32_16x16x4_f32.
//
//     dW[co][ci][tap] = sum_{b,p} dy[b][co][p] x'[b][ci][p + tap],   dy = c1 dz + c2 y + c3,   x' = x | relu(a x + b) | generated action planes
//
// What it keeps of k_lc_wgrad: the job description (Pair<LcWgrad>), the grid, the XCD remap, the chunking and the partials' layout
// [chunk][9][co_pad][ci_pad] (k_lc_wreduce adds them as before), the K-steps launch (srcs / cps), the staging plan (lane = (image of the round, pixel
// quad), wave w the channels w, 4 + w, ..), the float32 staging transform, short last chunks and rounds (idle slots staged as zeros), side-by-side
// and stacked rounds.  What differs: dy and x' are split into three bf16 terms (mz::conv_split3) AFTER the transform, on their way into LDS
//     plane[term h, m, l][32 channels][flat position]  (bf16),
// the pitch P is a multiple of 8 and a reduction step is 32 flat positions: lane (i16, kq) holds positions 32 g + 8 kq .. + 7 of channel i16, one
// aligned 16-byte read per term (dy) or per term and tap row (x).  The taps dx = -1 / +1 are the centre row shifted by one bf16: a funnel shift
// (v_alignbit_b32) of the centre's four dwords with one neighbour dword on either side -- no second LDS copy.  Six MFMAs per tap and step in the
// project's term order hh, hm, mh, hl, lh, mm (first letter: dy), float32 accumulators: one summation order per (SG, layout, ipw) -- (staging round,
// step, term) for every tap -- whatever the placement of the workgroups.
#pragma once
#include "mz_learn_conv.h"
#include "mz_learn_conv_split.h"
#include "mz_split3.h"

namespace mzlc {

// plane strides (bf16 elements) of a split geometry of `nsteps` 32-position steps at pitch P8 (a multiple of 8): the dy plane holds position f at f,
// the x plane at f + P8 + 8 (a zero row above, 8 elements of margin: the left neighbour dword of position 0 row -1 exists); both strides are
// 8 (mod 16) elements, an odd number of 16-byte slots, so that the 16 channels of a 16-byte read spread over the bank row.
inline int wgrad_split_spy(int nsteps) { return 32 * nsteps + 8; }
inline int wgrad_split_spx(int nsteps, int P8) { return 32 * nsteps + 2 * P8 + 24; }
// dynamic LDS: coefficients (160 floats) + 3 terms x 32 channels x (SPY + SPX) bf16
inline size_t wgrad_split_lds(int SPY, int SPX) { return 640 + (size_t)192 * (SPY + SPX); }

template <bool ACT>
__global__ __launch_bounds__(256, 1) void k_lc_wgrad_bf16x3(const Pair<LcWgrad> PJ) {
    int bx = blockIdx.x, byy = blockIdx.y;
    if (PJ.remap) {  // a chunk's blocks on one XCD (k_lc_wgrad)
        const int X = gridDim.x, Yc = PJ.a.co_blocks, nblocks = X * Yc;
        const int Lid = (int)blockIdx.x + X * (int)blockIdx.y, s = Lid >> 3;
        const int g = (Lid & 7) + 8 * (s / nblocks), blk = s % nblocks;
        bx = blk % X;
        byy = g * Yc + blk / X;
    }
    const bool second = byy >= PJ.na;
    LcWgrad L = second ? PJ.b : PJ.a;
    const int by = second ? byy - PJ.na : byy;
    int lchunk = by / L.co_blocks;  // the chunk within its unroll step
    if (L.srcs) {
        const int s = lchunk / L.cps;
        lchunk -= s * L.cps;
        const LcWgradSrc S = L.srcs[s];
        L.dz = S.dz; L.y = S.y; L.dcoef = S.dcoef; L.x0 = S.x0; L.xcoef = S.xcoef;
    }
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* s_dc = reinterpret_cast<float*>(smem);  // [3][32] dy coefficients of this block's channels
    float* s_xc = s_dc + 96;                       // [2][32]
    unsigned short* s_y = reinterpret_cast<unsigned short*>(smem + 640);  // [3][32][SPY]
    const int SPY = L.SPY, SPX = L.SPX, P8 = L.P4;
    const int yterm = 32 * SPY, xterm = 32 * SPX;
    unsigned short* s_x = s_y + 3 * yterm;                                // [3][32][SPX]: position f at f + P8 + 8
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), kq = lane >> 4, i16 = lane & 15;
    const int wm = wave >> 1, wn = wave & 1;
    const int cib = bx, cob = by % L.co_blocks, chunk = by / L.co_blocks;
    if (cib * 2 >= L.ci_tiles) return;  // (a paired job with fewer input-channel blocks; workgroup-uniform, before any barrier)
    const int hw = L.h * L.w_img, QP = (hw + 3) >> 2;
    const float r_iw = 1.0f / (float)L.w_img;
    const int co0 = cob * 32, ci0 = cib * 32;
    {
        const int n16 = (3 * (yterm + xterm)) >> 3;  // (both strides are multiples of 8 elements)
        float4* z = reinterpret_cast<float4*>(smem + 640);
        for (int i = tid; i < n16; i += 256) z[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (tid < 96) {
        const int c = co0 + (tid & 31);
        s_dc[tid] = c < L.cout ? L.dcoef[(tid >> 5) * L.cpad_out + c] : 0.0f;  // (channels past cout: dy = 0 * dz + 0 * y + 0)
    }
    if (tid >= 128 && tid < 192) {
        const int t = tid - 128, c = ci0 + (t & 31);
        s_xc[t] = (L.x_mode == IN_BNRELU && c < L.cin_real) ? L.xcoef[(t >> 5) * L.cpad_in + c] : 0.0f;
    }
    const __amdgpu_buffer_rsrc_t rs_dz = mkrs(L.dz), rs_y = mkrs(L.y), rs_x = mkrs(L.x0);
    // staging plan (k_lc_wgrad's): lane = (image of the round, pixel quad) (lanes >= sg QP idle), wave w the channels w, 4 + w, .., 28 + w
    const int gi = lc_idiv(lane, 1.0f / (float)QP), ql = lane - gi * QP;
    const bool s_ok = gi < L.sg;
    const int p0 = (s_ok ? ql : 0) * 4;
    // Elements past the image (the last quad) and idle lanes store too, unconditionally (k_lc_wgrad: a per-store predicate costs more than the store):
    // into a spare slot no MFMA reads -- dy plane index 32 nsteps (reads end at 32 nsteps - 1), x plane index SPX - 2 (reads end at SPX - 15)
    int sposy[4], sposx[4], pm[4];
#pragma unroll
    for (int e = 0; e < 4; e++) {
        const int pp = p0 + e, py = lc_idiv(pp, r_iw), px = pp - py * L.w_img;
        const int sp = (s_ok && pp < hw) ? (L.sg_cols ? py * P8 + gi * (L.w_img + 1) + px : (gi * (L.h + 1) + py) * P8 + px) : -1;
        sposy[e] = sp >= 0 ? sp : 32 * L.nsteps;
        sposx[e] = sp >= 0 ? sp + P8 + 8 : SPX - 2;
        pm[e] = ACT ? pp % L.num_actions : 0;
    }
    float4 rdz[8], ry[8], rx[8];
    int r_act = -1;
    bool r_ok = false;  // this lane's image of the round in flight belongs to the chunk (the last round may be short: its idle slots are staged as zeros)
    const int b_lo = lchunk * L.ipw, b_hi = (b_lo + L.ipw < L.B) ? b_lo + L.ipw : L.B;
    auto fetch = [&](int b) {  // round of images b .. b + sg - 1
        const int bi = b + (s_ok ? gi : 0);
        r_ok = s_ok && bi < b_hi;
        const int rel = r_ok ? bi - b : 0;
        const unsigned vo_o = (unsigned)((rel * L.cout * hw + p0) * sizeof(float)), vo_i = (unsigned)((rel * L.cin_real * hw + p0) * sizeof(float));
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int c = co0 + 4 * k + wave, cc = c < L.cout ? c : 0;
            const int so = (int)(((size_t)b * L.cout + cc) * hw * sizeof(float));
            rdz[k] = ld4(rs_dz, vo_o, so);
            ry[k] = ld4(rs_y, vo_o, so);
        }
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int c = ci0 + 4 * k + wave, cc = c < L.cin_real ? c : 0;
            rx[k] = ld4(rs_x, vo_i, (int)(((size_t)b * L.cin_real + cc) * hw * sizeof(float)));
        }
        if (ACT) r_act = L.action[b + rel];
    };
    auto stage = [&]() {
        const bool bnrelu = L.x_mode == IN_BNRELU;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int cl = 4 * k + wave, c = ci0 + cl;
            const float c1 = s_dc[cl], c2 = s_dc[32 + cl], c3 = s_dc[64 + cl];
            const float a[4] = {rdz[k].x, rdz[k].y, rdz[k].z, rdz[k].w}, yy[4] = {ry[k].x, ry[k].y, ry[k].z, ry[k].w};
            const float x[4] = {rx[k].x, rx[k].y, rx[k].z, rx[k].w};
            float vy[4], vx[4];
#pragma unroll
            for (int e = 0; e < 4; e++) vy[e] = r_ok ? fmaf(c1, a[e], fmaf(c2, yy[e], c3)) : 0.0f;
            if (!ACT || c < L.cin_real) {
                if (c >= L.cin_real) {  // (padding channels of a layer without action planes; wave-uniform)
#pragma unroll
                    for (int e = 0; e < 4; e++) vx[e] = 0.0f;
                } else if (bnrelu) {
                    const float xa = s_xc[cl], xb = s_xc[32 + cl];
#pragma unroll
                    for (int e = 0; e < 4; e++) {
                        const float t = fmaf(xa, x[e], xb);
                        vx[e] = t > 0.0f ? t : 0.0f;
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < 4; e++) vx[e] = x[e];
                }
            } else {  // action planes (network.py:440-444)
                const int t = c < L.cin ? (int)(((long long)(c - L.cin_real) * hw) % L.num_actions) : 0;
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    int m = pm[e] + t;
                    m = m >= L.num_actions ? m - L.num_actions : m;
                    vx[e] = (c < L.cin && m == r_act) ? 1.0f : 0.0f;
                }
            }
            unsigned short* py = s_y + cl * SPY;
            unsigned short* px = s_x + cl * SPX;
#pragma unroll
            for (int e = 0; e < 4; e++) {
                unsigned th, tm, tl;
                mz::conv_split3(vy[e], th, tm, tl);
                py[sposy[e]] = (unsigned short)th; py[yterm + sposy[e]] = (unsigned short)tm; py[2 * yterm + sposy[e]] = (unsigned short)tl;
                mz::conv_split3(vx[e], th, tm, tl);
                px[sposx[e]] = (unsigned short)th; px[xterm + sposx[e]] = (unsigned short)tm; px[2 * xterm + sposx[e]] = (unsigned short)tl;
            }
        }
    };
    f32x4 acc[9];
#pragma unroll
    for (int t = 0; t < 9; t++) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (b_lo < b_hi) fetch(b_lo);
    const int SGn = L.sg;
    const unsigned short* py_ = s_y + (wm * 16 + i16) * SPY + 8 * kq;            // + 32 g: the lane's eight dy positions
    const unsigned short* px_ = s_x + (wn * 16 + i16) * SPX + P8 + 8 + 8 * kq;   // + 32 g + dy P8: the centre eight of row dy
    for (int b = b_lo; b < b_hi; b += SGn) {
        __syncthreads();  // the previous round's MFMAs have read the planes (first pass: the zero fill is complete)
        stage();
        __syncthreads();
        if (b + SGn < b_hi) fetch(b + SGn);  // in flight during this round's MFMAs
        for (int g = 0; g < L.nsteps; g++) {
            u32x4 a[3];
#pragma unroll
            for (int t = 0; t < 3; t++) a[t] = *reinterpret_cast<const u32x4*>(py_ + t * yterm + 32 * g);
#pragma unroll
            for (int dy = 0; dy < 3; dy++) {
                u32x4 xs[3][3];  // [dx][term]
#pragma unroll
                for (int t = 0; t < 3; t++) {
                    const unsigned short* r = px_ + t * xterm + 32 * g + (dy - 1) * P8;
                    const u32x4 c = *reinterpret_cast<const u32x4*>(r);
                    const unsigned lf = *reinterpret_cast<const unsigned*>(r - 2), rg = *reinterpret_cast<const unsigned*>(r + 8);
                    xs[1][t] = c;
                    xs[0][t] = u32x4{__builtin_amdgcn_alignbit(c[0], lf, 16), __builtin_amdgcn_alignbit(c[1], c[0], 16), __builtin_amdgcn_alignbit(c[2], c[1], 16),
                                     __builtin_amdgcn_alignbit(c[3], c[2], 16)};
                    xs[2][t] = u32x4{__builtin_amdgcn_alignbit(c[1], c[0], 16), __builtin_amdgcn_alignbit(c[2], c[1], 16), __builtin_amdgcn_alignbit(c[3], c[2], 16),
                                     __builtin_amdgcn_alignbit(rg, c[3], 16)};
                }
#pragma unroll
                for (int dx = 0; dx < 3; dx++) {
                    const lc_bf16x8 ah = __builtin_bit_cast(lc_bf16x8, a[0]), am = __builtin_bit_cast(lc_bf16x8, a[1]), al = __builtin_bit_cast(lc_bf16x8, a[2]);
                    const lc_bf16x8 xh = __builtin_bit_cast(lc_bf16x8, xs[dx][0]), xm = __builtin_bit_cast(lc_bf16x8, xs[dx][1]), xl = __builtin_bit_cast(lc_bf16x8, xs[dx][2]);
                    f32x4 c = acc[dy * 3 + dx];
                    // the term order of every split build: hh, hm, mh, hl, lh, mm
                    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, xh, c, 0, 0, 0);
                    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, xm, c, 0, 0, 0);
                    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(am, xh, c, 0, 0, 0);
                    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, xl, c, 0, 0, 0);
                    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, xh, c, 0, 0, 0);
                    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(am, xm, c, 0, 0, 0);
                    acc[dy * 3 + dx] = c;
                }
            }
        }
    }
    // D[m = co][n = ci]: lane (kq, i16) holds rows 4 kq + r of column i16
    const int cot = cob * 2 + wm, cit = cib * 2 + wn;
    if (cot >= L.co_tiles || cit >= L.ci_tiles) return;
    const int co_pad = L.co_tiles * 16, ci_pad = L.ci_tiles * 16;
#pragma unroll
    for (int t = 0; t < 9; t++) {
        float* d = L.part + (((size_t)chunk * 9 + t) * co_pad + cot * 16 + 4 * kq) * ci_pad + cit * 16 + i16;
#pragma unroll
        for (int r = 0; r < 4; r++) d[(size_t)r * ci_pad] = acc[t][r];
    }
}

}  // namespace mzlc
