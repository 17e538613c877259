// mz_conv_split.h -- the opt-in split-bf16 3x3 conv of the board nets (mz_config.conv_precision == MZ_CONV_BF16X3) for gfx950.
//
// On gfx950 the f32-input MFMA runs at 1/16 of the bf16 rate.  A float32 is exactly the sum of three bf16 values,
//     x = h + m + l,   h = bf16(x), m = bf16(x - h), l = bf16(x - h - m)      (round to nearest even; both subtractions are exact),
// so a float32-grade product is six bf16 products accumulated in float32: hh, hm, mh, hl, lh, mm.  The three dropped cross terms
// (ml, lm, ll) are below 2^-24 of the product.  k_conv3x3_bf16x3 is the implicit GEMM of mz_conv.h on v_mfma_f32_16x16x32_bf16:
//     D[pixel][co] = bias[co] + sum over (32-channel block cb, tap, term) of A_term[pixel][32 ch] * B_term[32 ch][co]
// ONE summation order -- (32-channel block, tap, term), the 32 channels of a step in the MFMA's own order, channel cb*32 + k in
// k slot k -- in every build: an output does not depend on the batch, on the image's position in it or on the build the launcher
// picked.  It is NOT the oracle's fmaf chain: this path is held to the reference within the reference's own tolerance, not bit
// for bit to the oracle.
//   Activations stay float32 in HBM.  They are split while the slab (tile + halo) of a 32-channel block is staged into LDS: wave w
//   stages channel octet w of the block, lane l the slab positions l, l + 64, ...; each element is split once and then read by nine
//   taps and every output channel of the workgroup.  LDS layout: slab[term][octet q][position][8 bf16] -- lane (q = lane >> 4,
//   j = lane & 15) of the MFMA reads pixel j's 16 bytes of octet q: 16 consecutive 16-byte words per lane group, octet planes a
//   multiple of 256 bytes apart.  6 bytes per staged element: 57 KB (15 x 15 + halo), 84 KB (19 x 19 + halo), so the slab is
//   single-buffered (two 19 x 19 slabs exceed the 160 KB of a CU); the next block's values wait in registers while this block's MFMAs run.
//   Weights: three bf16 fragment streams per (channel tile, cb, tap), packed at commit in consumption order (3 KB per step),
//   read from L2 one step ahead.  Channel counts are zero-padded to 32 in the packed copy and in the slab.
//   workgroup = 256 threads = one image (blockIdx.y) x one spatial tile (blockIdx.x) x 64 * NCT output channels (blockIdx.z).
//   Builds: <4, 1, 0> shape-generic (8 x 8 output tiles, any board, any channel count); <15, NCT, 15> and <23, NCT, 19>: the whole
//   image per workgroup.  The epilogue computes k_conv3x3's function (bias in the accumulator, + residual, ReLU) in float32.
#pragma once
#include "mz_conv.h"
#include "mz_split3.h"

namespace mz {

typedef __bf16 conv_bf16x8 __attribute__((ext_vector_type(8)));

struct SplitConvLaunch {
    const float* const* in_ptrs;  // [B] per-image base pointers (node store rows) or null
    const float* in;              // dense [B][cin_real][h][w] if in_ptrs == null
    const int* action;            // [B] or null: channels cin_real .. cin - 1 are the dynamics net's action planes (network.py:440-444)
    int num_actions;
    int cin_real, cin;            // channels in memory / logical input channels; k runs over pad32(cin)
    int h, w;                     // image (stride 1, pad 1: input and output geometry)
    int cout;
    const conv_u32x4* w3;              // packed [co_tile][cb][tap][term h, m, l][64 lanes] x 8 bf16
    const float* bias;            // [pad16(cout)]
    const float* residual;        // dense [B][cout][h][w] or null
    float* out;                   // dense [B][cout][h][w]
    int relu;
    int th, tw, tiles_x;          // output tile (th * tw <= NPT * 16)
    int B;
};

// conv_bf16_rne / conv_split3 (x = h + m + l exactly): mz_split3.h, shared with the learner's split conv

constexpr int split_npos_pad(int npos) { return (npos + 15) & ~15; }

template <int NPT, int NCT, int SIDE>
__global__ __launch_bounds__(256, 1) void k_conv3x3_bf16x3(const SplitConvLaunch L_) {
    SplitConvLaunch L = L_;
    if constexpr (SIDE > 0) { L.h = SIDE; L.w = SIDE; L.th = SIDE; L.tw = SIDE; L.tiles_x = 1; }
    constexpr int NPOS_MAX = SIDE > 0 ? (SIDE + 2) * (SIDE + 2) : 100;  // generic: 8 x 8 tiles
    constexpr int IT = (NPOS_MAX + 63) / 64;                            // slab positions per lane
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    conv_u32x4* slab = reinterpret_cast<conv_u32x4*>(smem);  // [3 terms][4 octets][npos_pad]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), q = lane >> 4, j = lane & 15;
    const int tile = blockIdx.x, ty0 = (tile / L.tiles_x) * L.th, tx0 = (tile % L.tiles_x) * L.tw;
    const int sih = L.th + 2, siw = L.tw + 2, npos = sih * siw, npos_pad = split_npos_pad(npos), tstr = 4 * npos_pad;
    const int hw = L.h * L.w, TP = L.th * L.tw, img = blockIdx.y;
    const int n_cb = (L.cin + 31) >> 5, co_tiles = (L.cout + 15) >> 4;
    const float* src = L.in_ptrs ? L.in_ptrs[img] : L.in + (size_t)img * L.cin_real * hw;  // workgroup-uniform
    const int act = L.action ? L.action[img] : -1;

    // ---- staging plan: wave = channel octet of the block, lane = slab positions lane + 64 * it ----
    int s_goff[IT];    // pixel index in the image, or -1: zero padding / beyond the slab
    bool s_write[IT];
#pragma unroll
    for (int it = 0; it < IT; it++) {
        const int pos = lane + 64 * it;
        s_write[it] = pos < npos;
        const int pc = s_write[it] ? pos : 0, sy = pc / siw, sx = pc - sy * siw, gy = ty0 + sy - 1, gx = tx0 + sx - 1;
        s_goff[it] = (s_write[it] && gy >= 0 && gy < L.h && gx >= 0 && gx < L.w) ? gy * L.w + gx : -1;
    }
    float pf[IT][8];
    auto fetch = [&](int cb) {  // global -> registers: channels cb * 32 + 8 * wave + c
#pragma unroll
        for (int c = 0; c < 8; c++) {
            const int ch = cb * 32 + 8 * wave + c;  // wave-uniform
            if (ch < L.cin_real) {
                const float* s = src + (size_t)ch * hw;
#pragma unroll
                for (int it = 0; it < IT; it++) {
                    const float v = s[s_goff[it] >= 0 ? s_goff[it] : 0];  // (a valid address for every lane)
                    pf[it][c] = s_goff[it] >= 0 ? v : 0.0f;
                }
            } else if (ch < L.cin) {  // action plane: flat element f = (ch - cin_real) * hw + pixel of the [A, h, w] block is 1 iff f % A == action
                const int t = ((ch - L.cin_real) * hw) % L.num_actions;
#pragma unroll
                for (int it = 0; it < IT; it++)
                    pf[it][c] = (s_goff[it] >= 0 && (t + s_goff[it]) % L.num_actions == act) ? 1.0f : 0.0f;
            } else {
#pragma unroll
                for (int it = 0; it < IT; it++) pf[it][c] = 0.0f;
            }
        }
    };
    auto store = [&]() {  // split the fetched values and write the three term planes
#pragma unroll
        for (int it = 0; it < IT; it++) {
            unsigned hb[8], mb[8], lb[8];
#pragma unroll
            for (int c = 0; c < 8; c++) conv_split3(pf[it][c], hb[c], mb[c], lb[c]);
            if (s_write[it]) {
                conv_u32x4* d = slab + wave * npos_pad + lane + 64 * it;
                d[0] = conv_u32x4{hb[0] | (hb[1] << 16), hb[2] | (hb[3] << 16), hb[4] | (hb[5] << 16), hb[6] | (hb[7] << 16)};
                d[tstr] = conv_u32x4{mb[0] | (mb[1] << 16), mb[2] | (mb[3] << 16), mb[4] | (mb[5] << 16), mb[6] | (mb[7] << 16)};
                d[2 * tstr] = conv_u32x4{lb[0] | (lb[1] << 16), lb[2] | (lb[3] << 16), lb[4] | (lb[5] << 16), lb[6] | (lb[7] << 16)};
            }
        }
    };

    // ---- A-operand rows of this lane: pixel slot pt * 16 + j of the tile (slots past the tile read position 0 and are never stored) ----
    int aoff[NPT];
#pragma unroll
    for (int pt = 0; pt < NPT; pt++) {
        const int p = pt * 16 + j, pc = p < TP ? p : 0, py = pc / L.tw, px = pc - py * L.tw;
        aoff[pt] = q * npos_pad + py * siw + px;
    }
    // ---- accumulators D[pixel slot 4q + r][channel j] start at the bias ----
    f32x4 acc[NCT][NPT];
    int cot[NCT];
    const conv_u32x4* wp[NCT];
#pragma unroll
    for (int c = 0; c < NCT; c++) {
        cot[c] = blockIdx.z * 4 * NCT + wave + 4 * c;
        const int ct = cot[c] < co_tiles ? cot[c] : co_tiles - 1;  // out-of-range tiles compute a duplicate that is never stored
        const float bv = L.bias[ct * 16 + j];
#pragma unroll
        for (int pt = 0; pt < NPT; pt++) acc[c][pt] = f32x4{bv, bv, bv, bv};
        wp[c] = L.w3 + (size_t)ct * n_cb * 9 * 192 + lane;  // 192 x 16 bytes per step: [term][64 lanes]
    }
    const int n_steps = n_cb * 9;
    conv_u32x4 wn[NCT][3];  // the next step's weights
#pragma unroll
    for (int c = 0; c < NCT; c++) {
#pragma unroll
        for (int t = 0; t < 3; t++) wn[c][t] = wp[c][t * 64];
    }
    fetch(0);
    store();
    __syncthreads();
    for (int cb = 0; cb < n_cb; cb++) {
        if (cb + 1 < n_cb) fetch(cb + 1);
#pragma unroll 1
        for (int tap = 0; tap < 9; tap++) {
            conv_bf16x8 wh[NCT], wm[NCT], wl[NCT];
            const int step = cb * 9 + tap, nxt = step + 1 < n_steps ? step + 1 : step;
#pragma unroll
            for (int c = 0; c < NCT; c++) {
                wh[c] = __builtin_bit_cast(conv_bf16x8, wn[c][0]);
                wm[c] = __builtin_bit_cast(conv_bf16x8, wn[c][1]);
                wl[c] = __builtin_bit_cast(conv_bf16x8, wn[c][2]);
#pragma unroll
                for (int t = 0; t < 3; t++) wn[c][t] = wp[c][nxt * 192 + t * 64];
            }
            const int ky = tap / 3, toff = ky * siw + (tap - 3 * ky);
#pragma unroll
            for (int pt = 0; pt < NPT; pt++) {
                const conv_u32x4* a = slab + aoff[pt] + toff;
                const conv_bf16x8 xh = __builtin_bit_cast(conv_bf16x8, a[0]), xm = __builtin_bit_cast(conv_bf16x8, a[tstr]),
                                  xl = __builtin_bit_cast(conv_bf16x8, a[2 * tstr]);
                // the term order of every build: hh, hm, mh, hl, lh, mm
#pragma unroll
                for (int c = 0; c < NCT; c++) acc[c][pt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xh, wh[c], acc[c][pt], 0, 0, 0);
#pragma unroll
                for (int c = 0; c < NCT; c++) acc[c][pt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xh, wm[c], acc[c][pt], 0, 0, 0);
#pragma unroll
                for (int c = 0; c < NCT; c++) acc[c][pt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xm, wh[c], acc[c][pt], 0, 0, 0);
#pragma unroll
                for (int c = 0; c < NCT; c++) acc[c][pt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xh, wl[c], acc[c][pt], 0, 0, 0);
#pragma unroll
                for (int c = 0; c < NCT; c++) acc[c][pt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xl, wh[c], acc[c][pt], 0, 0, 0);
#pragma unroll
                for (int c = 0; c < NCT; c++) acc[c][pt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xm, wm[c], acc[c][pt], 0, 0, 0);
            }
        }
        __syncthreads();  // every wave has read this block's slab
        if (cb + 1 < n_cb) store();
        __syncthreads();
    }
    // ---- epilogue: lane (q, j) holds pixel slots pt * 16 + 4q + r (r = 0..3) of output channel 16 * tile + j: + residual, ReLU, store.
    // Whole-image builds: a lane's four slots are four consecutive pixels of the image -> one 16-byte access ----
#pragma unroll
    for (int c = 0; c < NCT; c++) {
        if (cot[c] >= co_tiles) continue;  // wave-uniform
        const int co = cot[c] * 16 + j;
        if (co >= L.cout) continue;
        const size_t obase = ((size_t)img * L.cout + co) * hw;
#pragma unroll
        for (int pt = 0; pt < NPT; pt++) {
            const int p0 = pt * 16 + 4 * q;
            f32x4 v = acc[c][pt];
            if (SIDE > 0 && p0 + 3 < hw) {
                if (L.residual) {
                    const float* rp = L.residual + obase + p0;
#pragma unroll
                    for (int r = 0; r < 4; r++) v[r] = v[r] + rp[r];
                }
#pragma unroll
                for (int r = 0; r < 4; r++)
                    if (L.relu && !(v[r] > 0.0f)) v[r] = 0.0f;
                float* op = L.out + obase + p0;
#pragma unroll
                for (int r = 0; r < 4; r++) op[r] = v[r];
            } else {
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int p = p0 + r, pc = p < TP ? p : 0, py = pc / L.tw, px = pc - py * L.tw, gy = ty0 + py, gx = tx0 + px;
                    if (p < TP && gy < L.h && gx < L.w) {
                        const size_t o = obase + (size_t)gy * L.w + gx;
                        float t = v[r] + (L.residual ? L.residual[o] : 0.0f);
                        if (L.relu && !(t > 0.0f)) t = 0.0f;
                        L.out[o] = t;
                    }
                }
            }
        }
    }
}

}  // namespace mz
