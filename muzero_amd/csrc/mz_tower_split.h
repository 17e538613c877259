// mz_tower_split.h -- a whole residual tower on split-bf16 MFMAs as ONE persistent kernel, activations resident in LDS: the job of
// k_res_tower (mz_tower.h) in the arithmetic of k_conv3x3_bf16x3 (mz_conv_split.h).
//
// k_conv3x3_bf16x3 has ONE summation order in every build: (32-channel block, tap, term hh hm mh hl lh mm), accumulator started at the
// bias, then float32 `+ residual`, then ReLU.  This kernel keeps that order, so a tower equals the chain of per-conv split launches bit
// for bit -- the contract k_res_tower has with k_conv3x3 in float32.
//   workgroup = 512 threads = 8 waves, wave w = output-channel tile w (16 channels; P % 16 == 0, P <= 128; waves past the channel tiles
//   only take part in barriers), NPT pixel tiles of 16 over the G * h * w pixels of the group's G whole images.
//   Activations: TWO buffers of three bf16 term planes in the A-operand layout of k_conv3x3_bf16x3's slab, without a halo:
//       act[term h, m, l][32-channel block][octet q][position][8 bf16]            (P32 * nposp * 6 bytes, P32 = P padded to 32)
//   Lane (q = lane >> 4, j = lane & 15) of an MFMA reads pixel j's 16 bytes of octet q.  A tap that falls outside its image reads the
//   padding position `npix` of the plane, which stays zero (nposp > G * h * w; tail slots of the last pixel tile are forced to zero, as
//   mz_tower.h's tail_keep does).  Channels P .. P32 - 1 are zeroed once and never written.
//   An activation is split ONCE, by the epilogue that produces it (conv_split3 on the float32 value after + residual and ReLU), and then
//   only read: conv 2k reads buffer 0 and writes buffer 1, conv 2k + 1 the other way round.  One barrier per convolution.
//   The residual is the exact float32 block input, never a bf16 term.  It stays in registers: the lane that computed output (pixel slot,
//   channel) of one block is the lane that needs it as the residual of the next, which is why two buffers suffice -- at the Atari
//   geometry (P = 128, two 6 x 6 images, 80 positions) one buffer is 61 440 bytes; three would not fit the CU's 160 KB.
//   Weights: every conv's own w3 stream (3 KB per (channel tile, block, tap), mz_conv_split.h), found through a small pointer table, read
//   from L2 WD - 1 steps ahead into a register ring that runs straight across layer boundaries.  No second copy of the weights exists.
//   All 9 * NPT tap offsets of a lane live in VGPRs (mz_tower.h: VALU work between MFMAs is MFMA time).
#pragma once
#include "mz_conv_split.h"

namespace mz {

struct SplitTowerLaunch {
    const float* in;                  // dense [B][P][hw]
    float* out;                       // dense [B][P][hw]
    const conv_u32x4* const* w3;      // [n_convs] each conv's packed stream [co_tile][cb][tap][term h, m, l][64 lanes] x 8 bf16
    const float* const* bias;         // [n_convs] each conv's folded bias [P]
    int n_convs;                      // 2 * blocks: even index = conv1 (ReLU), odd = conv2 (+ block input, ReLU)
    int P, h, w_img, G, B;
    int nposp;                        // positions per plane, multiple of 16, > G * h * w (at least one zero padding position)
};

constexpr size_t split_tower_lds_bytes(int P, int nposp) { return (size_t)2 * 3 * ((P + 31) / 32) * 4 * nposp * 16; }

template <int NPT>
__global__ __launch_bounds__(512, 1) void k_res_tower_bf16x3(const SplitTowerLaunch L) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    conv_u32x4* lds = reinterpret_cast<conv_u32x4*>(smem);
    unsigned short* lds16 = reinterpret_cast<unsigned short*>(smem);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), q = lane >> 4, j = lane & 15;
    const int hw = L.h * L.w_img, npix = L.G * hw, img0 = blockIdx.x * L.G;
    const int n_cb = (L.P + 31) >> 5, co_tiles = L.P >> 4;
    const int plane = L.nposp;             // 16-byte words per (term, block, octet) plane
    const int tstr = n_cb * 4 * plane;     // words per term
    const int bufsz = 3 * tstr;            // words per activation buffer
    const bool active = wave < co_tiles;   // (wave-uniform)
    const int cot = active ? wave : 0, co = cot * 16 + j;
    const float r_hw = 1.0f / (float)hw, r_w = 1.0f / (float)L.w_img;

    for (int i = tid; i < 2 * bufsz; i += 512) lds[i] = conv_u32x4{0u, 0u, 0u, 0u};
    __syncthreads();

    // ---- per-lane bookkeeping.  A-operand rows are pixel slots pt * 16 + j; accumulator rows are slots pt * 16 + 4q + r.
    // aoff[tap][pt]: word offset, inside (term 0, block 0), of the lane's A operand for that tap: the tap-shifted pixel or the zero position
    int aoff[9][NPT];
#pragma unroll
    for (int pt = 0; pt < NPT; pt++) {
        const int p = pt * 16 + j, g = conv_idiv(p, r_hw), pp = p - g * hw, y = conv_idiv(pp, r_w), x = pp - y * L.w_img;
#pragma unroll
        for (int t = 0; t < 9; t++) {
            const int yy = y + t / 3 - 1, xx = x + t % 3 - 1;
            const bool ok = p < npix && yy >= 0 && yy < L.h && xx >= 0 && xx < L.w_img;
            aoff[t][pt] = q * plane + (ok ? p + (t / 3 - 1) * L.w_img + (t % 3 - 1) : npix);
        }
    }
    // only the last pixel tile can hold slots beyond the group's pixels; their activations are forced to zero, which keeps the padding
    // positions of both buffers zero
    bool tail_keep[4];
#pragma unroll
    for (int r = 0; r < 4; r++) tail_keep[r] = (NPT - 1) * 16 + 4 * q + r < npix;
    // this lane's outputs in HBM: pixel slot p of channel co -> image, pixel; -1: nothing to load or store (tail slot, image past the
    // batch).  Computed where it is used, at the tower's two ends, instead of held in registers across the convolutions.
    auto goff = [&](int pt, int r) {
        const int p = pt * 16 + 4 * q + r, g = conv_idiv(p, r_hw), pp = p - g * hw;
        return (p < npix && img0 + g < L.B) ? g * L.P * hw + pp : -1;
    };
    const size_t gbase = ((size_t)img0 * L.P + co) * hw;
    // channel co inside a term plane, in bf16 units: block co >> 5, octet (co & 31) >> 3, element co & 7
    const int cbase16 = (((co >> 5) * 4 + ((co & 31) >> 3)) * plane) * 8 + (co & 7);
    auto put = [&](int buf, const f32x4 (&v)[NPT]) {  // split this lane's float32 activations into the three term planes of buffer `buf`
        unsigned short* d = lds16 + buf * bufsz * 8 + cbase16;
#pragma unroll
        for (int pt = 0; pt < NPT; pt++) {
#pragma unroll
            for (int r = 0; r < 4; r++) {
                unsigned hb, mb, lb;
                conv_split3(v[pt][r], hb, mb, lb);
                unsigned short* e = d + (pt * 16 + 4 * q + r) * 8;
                e[0] = (unsigned short)hb;
                e[tstr * 8] = (unsigned short)mb;
                e[2 * tstr * 8] = (unsigned short)lb;
            }
        }
    };

    // ---- the tower's input: float32 into the residual registers, split into buffer 0 ----
    f32x4 res[NPT];
    if (active) {
#pragma unroll
        for (int pt = 0; pt < NPT; pt++) {
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int o = goff(pt, r);
                res[pt][r] = o >= 0 ? L.in[gbase + (o >= 0 ? o : 0)] : 0.0f;
            }
        }
        put(0, res);
    }

    // ---- weight ring: step s of the current conv in wr[s % WD], WD - 1 steps ahead (WD | 9: static ring index, also across convs) ----
    constexpr int WD = NPT <= 2 ? 9 : 3;
    const int n_steps = n_cb * 9;
    const int wave_off = cot * n_steps * 192 + lane;  // this wave's channel tile inside a conv's stream, 16-byte words
    conv_u32x4 wr[WD][3];
    const conv_u32x4* wcur = L.w3[0] + wave_off;
    if (active) {
#pragma unroll
        for (int s0 = 0; s0 < WD - 1; s0++) {
#pragma unroll
            for (int t = 0; t < 3; t++) wr[s0][t] = wcur[s0 * 192 + t * 64];
        }
    }
    __syncthreads();

    for (int cv = 0; cv < L.n_convs; cv++) {
        const bool second = cv & 1, last = cv + 1 == L.n_convs;
        if (active) {
            const conv_u32x4* wnext = L.w3[last ? cv : cv + 1] + wave_off;  // (the last conv re-reads its own first steps: never consumed)
            const conv_u32x4* src = lds + (second ? bufsz : 0);
            f32x4 acc[NPT];
            {
                const float bv = L.bias[cv][co];
#pragma unroll
                for (int pt = 0; pt < NPT; pt++) acc[pt] = f32x4{bv, bv, bv, bv};
            }
            for (int cb = 0; cb < n_cb; cb++) {
                // (opaque to the optimiser: left visible, loop strength reduction keeps one induction pointer per (tap, tile, term) -- 27 * NPT
                // registers -- and spills; this way an operand address is aoff + one add per read)
                int cbw = cb * 4 * plane;
                asm volatile("" : "+s"(cbw));
                const conv_u32x4* sb = src + cbw;
#pragma unroll
                for (int tap = 0; tap < 9; tap++) {
                    {   // weights WD - 1 steps ahead, across the layer boundary
                        const int s2 = cb * 9 + tap + WD - 1;
                        const conv_u32x4* wp = s2 < n_steps ? wcur + s2 * 192 : wnext + (s2 - n_steps) * 192;
#pragma unroll
                        for (int t = 0; t < 3; t++) wr[(tap + WD - 1) % WD][t] = wp[t * 64];
                    }
                    const conv_bf16x8 wh = __builtin_bit_cast(conv_bf16x8, wr[tap % WD][0]), wm = __builtin_bit_cast(conv_bf16x8, wr[tap % WD][1]),
                                      wl = __builtin_bit_cast(conv_bf16x8, wr[tap % WD][2]);
#pragma unroll
                    for (int pt = 0; pt < NPT; pt++) {
                        const conv_u32x4* a = sb + aoff[tap][pt];
                        const conv_bf16x8 xh = __builtin_bit_cast(conv_bf16x8, a[0]), xm = __builtin_bit_cast(conv_bf16x8, a[tstr]),
                                          xl = __builtin_bit_cast(conv_bf16x8, a[2 * tstr]);
                        // the term order of every split build: hh, hm, mh, hl, lh, mm
                        acc[pt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xh, wh, acc[pt], 0, 0, 0);
                        acc[pt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xh, wm, acc[pt], 0, 0, 0);
                        acc[pt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xm, wh, acc[pt], 0, 0, 0);
                        acc[pt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xh, wl, acc[pt], 0, 0, 0);
                        acc[pt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xl, wh, acc[pt], 0, 0, 0);
                        acc[pt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xm, wm, acc[pt], 0, 0, 0);
                    }
                    __builtin_amdgcn_sched_barrier(0);  // a tap's operand reads stay inside the tap: hoisted across taps they spill
                }
            }
            wcur = wnext;
            // ---- epilogue in float32: lane (q, j) holds pixel slots pt * 16 + 4q + r of channel co: (+ block input), ReLU ----
#pragma unroll
            for (int pt = 0; pt < NPT; pt++) {
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    float v = acc[pt][r];
                    if (second) v = v + res[pt][r];
                    if (!(v > 0.0f)) v = 0.0f;
                    if (pt == NPT - 1 && !tail_keep[r]) v = 0.0f;
                    acc[pt][r] = v;
                }
            }
            if (second) {  // the block's output is the next block's input: its residual, exact
#pragma unroll
                for (int pt = 0; pt < NPT; pt++) res[pt] = acc[pt];
            }
            if (last) {
#pragma unroll
                for (int pt = 0; pt < NPT; pt++) {
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const int o = goff(pt, r);
                        if (o >= 0) L.out[gbase + o] = acc[pt][r];
                    }
                }
            } else {
                put(second ? 0 : 1, acc);
            }
        }
        __syncthreads();
    }
}

}  // namespace mz
