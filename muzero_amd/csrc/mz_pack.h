// mz_pack.h -- reloading a planner's weights from device memory (mz_planner_bind_param_device / mz_planner_refresh_params).
//
// The packed operand copies of a planner (MFMA fragment order, folded BatchNorm, split-bf16 streams, tower tables, the tuned kernel's
// weight stream) are defined in ONE place: the host packers of mz_planner_commit_params (planner.hip, mz_convnet.h).  The device path
// does not repeat those layouts.  Once per binding it runs the host commit three times over PROBE tensors whose values name their own
// element -- small integers, exact in float32 and, summed over the three terms, in the split-bf16 streams -- reads every packed buffer
// back and decodes, per destination element, where the host path takes it from:
//     pass 0   every tensor holds (element index + 1); BatchNorm gamma = 1, mean = 0, var + eps = 1, beta = (element index + 1)
//     pass 1   every tensor holds (tensor id + 1), BatchNorm as in pass 0 with beta = (tensor id + 1)
//     pass 2   every tensor holds 1; BatchNorm gamma = (gamma's tensor id + 2), mean = 1, beta = 0
// so a destination element reads (0, 0, 0): a zero slot; (i + 1, t + 1, 1): a copy of tensor t's element i; (i + 1, t + 1, g + 2): that
// element times the alpha of the BatchNorm with gamma g, channel = the element's index along dimension 0; (i + 1, t + 1, -(g + 2)): the
// folded bias beta[i] - mean[i] * alpha[i].  A refresh is then two gather kernels (float32 buffers, split-bf16 buffers) over those maps,
// with the fold's float32 operations in the host's order.
//
// The first part of this file is plain C++ (probe values and decoding: no HIP call), the kernels follow under __HIPCC__.
#pragma once
#include <cstdint>
#include <cstring>
#include <cmath>
#include <map>
#include <string>
#include <vector>

namespace mz {

// one packed device buffer of a planner handle, as mz_debug_read_packed enumerates them
enum { PACK_F32 = 0, PACK_W3 = 1, PACK_STATIC = 2 };  // float32 / split-bf16 stream [group][term h, m, l][512] / geometry only (never refreshed)
struct PackBufferRef {
    void* d;
    size_t bytes;
    int kind;
    std::string label;
};

enum { PACK_ROLE_PLAIN = 0, PACK_ROLE_GAMMA = 1, PACK_ROLE_BETA = 2, PACK_ROLE_MEAN = 3, PACK_ROLE_VAR = 4 };
struct PackTensor {
    std::string name;
    std::vector<int64_t> shape;
    size_t numel = 0;
    int role = PACK_ROLE_PLAIN;
    int gamma = -1, beta = -1, mean = -1, var = -1;  // the tensors of its BatchNorm (role != plain)
    // how the host path uses it as a source, found by decoding: -1 unused, 0 copy, 1 scaled by fold_gamma's alpha, 2 folded bias
    int fold_kind = -1, fold_gamma = -1;
};
struct PackEntry {  // one destination element: tensor id (-1: zero) and element index
    int tid, idx;
};

// A BatchNorm is the four tensors X.weight, X.bias, X.running_mean, X.running_var (torch's names).
inline void pack_assign_roles(std::vector<PackTensor>& T) {
    std::map<std::string, int> id;
    for (size_t i = 0; i < T.size(); i++) id[T[i].name] = (int)i;
    const std::string sfx = ".running_mean";
    for (size_t i = 0; i < T.size(); i++) {
        const std::string& n = T[i].name;
        if (n.size() <= sfx.size() || n.compare(n.size() - sfx.size(), sfx.size(), sfx) != 0) continue;
        const std::string base = n.substr(0, n.size() - sfx.size());
        auto g = id.find(base + ".weight"), b = id.find(base + ".bias"), v = id.find(base + ".running_var");
        if (g == id.end() || b == id.end() || v == id.end()) continue;
        const int ids[4] = {g->second, b->second, (int)i, v->second};
        const int roles[4] = {PACK_ROLE_GAMMA, PACK_ROLE_BETA, PACK_ROLE_MEAN, PACK_ROLE_VAR};
        for (int k = 0; k < 4; k++) {
            PackTensor& t = T[ids[k]];
            t.role = roles[k]; t.gamma = ids[0]; t.beta = ids[1]; t.mean = ids[2]; t.var = ids[3];
        }
    }
}

// the running_var whose float32 sum with the fold's eps is exactly 1 (so that the probes' alpha is exactly gamma); 0 if there is none
inline float pack_unit_var() {
    float v = 1.0f - 1e-5f;
    for (int i = 0; i < 8; i++, v = nextafterf(v, 0.0f))
        if (v + 1e-5f == 1.0f && 1.0f / sqrtf(v + 1e-5f) == 1.0f) return v;
    v = 1.0f - 1e-5f;
    for (int i = 0; i < 8; i++, v = nextafterf(v, 2.0f))
        if (v + 1e-5f == 1.0f && 1.0f / sqrtf(v + 1e-5f) == 1.0f) return v;
    return 0.0f;
}

constexpr size_t PACK_MAX_NUMEL = ((size_t)1 << 24) - 2;  // element index + 1 stays an exact float32 integer

inline void pack_probe_values(const PackTensor& t, int tid, int pass, float unit_var, float* out) {
    const size_t n = t.numel;
    switch (t.role) {
        case PACK_ROLE_GAMMA: for (size_t i = 0; i < n; i++) out[i] = pass == 2 ? (float)(tid + 2) : 1.0f; break;
        case PACK_ROLE_MEAN: for (size_t i = 0; i < n; i++) out[i] = pass == 2 ? 1.0f : 0.0f; break;
        case PACK_ROLE_VAR: for (size_t i = 0; i < n; i++) out[i] = unit_var; break;
        case PACK_ROLE_BETA: for (size_t i = 0; i < n; i++) out[i] = pass == 0 ? (float)(i + 1) : pass == 1 ? (float)(tid + 1) : 0.0f; break;
        default: for (size_t i = 0; i < n; i++) out[i] = pass == 0 ? (float)(i + 1) : pass == 1 ? (float)(tid + 1) : 1.0f; break;
    }
}

// one destination element from its three probe readings; records in T how its source tensor is used.  false: the readings are not of
// the forms above (err says which) -- the host packer does something this path does not know, and the caller refuses to refresh.
inline bool pack_classify(float a, float b, float c, std::vector<PackTensor>& T, PackEntry* e, std::string* err) {
    if (a == 0.0f && b == 0.0f && c == 0.0f) { e->tid = -1; e->idx = 0; return true; }
    const float nt = (float)T.size();
    if (!(b >= 1.0f && b <= nt) || b != floorf(b)) { *err = "probe reading names no tensor"; return false; }
    const int tid = (int)b - 1;
    PackTensor& t = T[tid];
    if (!(a >= 1.0f && a <= (float)t.numel) || a != floorf(a)) { *err = "probe reading names no element of " + t.name; return false; }
    int kind, g = -1;
    const float m = fabsf(c);
    if (c == 1.0f) kind = 0;
    else if (m >= 2.0f && m <= nt + 1.0f && m == floorf(m)) { kind = c > 0.0f ? 1 : 2; g = (int)m - 2; }
    else { *err = "probe reading names no BatchNorm for " + t.name; return false; }
    if (kind == 0 && t.role != PACK_ROLE_PLAIN) { *err = t.name + " is copied although it belongs to a BatchNorm"; return false; }
    if (kind == 1 && (t.role != PACK_ROLE_PLAIN || T[g].role != PACK_ROLE_GAMMA || t.shape.empty() || T[g].numel != (size_t)t.shape[0])) {
        *err = t.name + " is scaled by something that is no BatchNorm over its dimension 0";
        return false;
    }
    if (kind == 2 && (t.role != PACK_ROLE_BETA || t.gamma != g)) { *err = t.name + " is folded with another layer's BatchNorm"; return false; }
    if (t.fold_kind >= 0 && (t.fold_kind != kind || t.fold_gamma != g)) { *err = t.name + " is packed in two different ways"; return false; }
    t.fold_kind = kind; t.fold_gamma = g;
    e->tid = tid; e->idx = (int)a - 1;
    return true;
}

inline bool pack_decode_f32(const float* a, const float* b, const float* c, size_t n, std::vector<PackTensor>& T, PackEntry* out, std::string* err) {
    for (size_t i = 0; i < n; i++)
        if (!pack_classify(a[i], b[i], c[i], T, &out[i], err)) return false;
    return true;
}

inline float pack_bf16(uint16_t h) {
    const uint32_t u = (uint32_t)h << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}
// split-bf16 streams (mz_conv_split.h): groups of three 512-value term blocks h, m, l with h + m + l the float32 value, exactly.
// n_pairs = groups * 512 (value, position) pairs; out[q] for pair q = group * 512 + position.
inline bool pack_decode_w3(const uint16_t* a, const uint16_t* b, const uint16_t* c, size_t n_pairs, std::vector<PackTensor>& T, PackEntry* out,
                           std::string* err) {
    for (size_t q = 0; q < n_pairs; q++) {
        const size_t o = (q / 512) * 1536 + q % 512;
        const float va = pack_bf16(a[o]) + pack_bf16(a[o + 512]) + pack_bf16(a[o + 1024]);
        const float vb = pack_bf16(b[o]) + pack_bf16(b[o + 512]) + pack_bf16(b[o + 1024]);
        const float vc = pack_bf16(c[o]) + pack_bf16(c[o + 512]) + pack_bf16(c[o + 1024]);
        if (!pack_classify(va, vb, vc, T, &out[q], err)) return false;
        if (out[q].tid >= 0 && T[out[q].tid].fold_kind == 2) { *err = "a folded bias inside a split-bf16 stream"; return false; }
    }
    return true;
}

// Work list of the gather kernels: one workgroup per chunk.  A chunk never crosses a buffer; its entries start at a multiple of four in
// the entry array (16-byte loads) and its destination at a multiple of the chunk size (16-byte stores: every buffer is its own hipMalloc).
constexpr int PACK_CHUNK_F32 = 1024;  // float32 elements per workgroup: 256 lanes x 4
constexpr int PACK_CHUNK_W3 = 2048;   // split-bf16 values per workgroup: 256 lanes x 8 (one 16-byte store per term)
struct PackChunk {
    int buf, off, n, map;  // destination buffer, first element (W3: first pair), count, first entry
};

inline void pack_make_chunks(int buf, size_t n, int per, const PackEntry* entries, std::vector<PackChunk>& chunks, std::vector<PackEntry>& map) {
    for (size_t off = 0; off < n; off += per) {
        const size_t cnt = n - off < (size_t)per ? n - off : (size_t)per;
        chunks.push_back(PackChunk{buf, (int)off, (int)cnt, (int)map.size()});
        map.insert(map.end(), entries + off, entries + off + cnt);
        while (map.size() % 4) map.push_back(PackEntry{-1, 0});
    }
}

// every entry within its tensor, every chunk within its buffer and the entry array (checked before anything is launched)
inline bool pack_check_bounds(const std::vector<PackChunk>& chunks, const std::vector<PackEntry>& map, const std::vector<PackTensor>& T,
                              const std::vector<size_t>& buf_elems, std::string* err) {
    for (const PackChunk& c : chunks) {
        if (c.buf < 0 || (size_t)c.buf >= buf_elems.size() || c.off < 0 || c.n < 1 || (size_t)c.off + c.n > buf_elems[c.buf] || c.map < 0 ||
            (size_t)c.map + c.n > map.size() || c.map % 4) {
            *err = "device reload: a chunk leaves its buffer";
            return false;
        }
        for (int i = 0; i < c.n; i++) {
            const PackEntry& e = map[c.map + i];
            if (e.tid < 0) continue;
            if ((size_t)e.tid >= T.size() || e.idx < 0 || (size_t)e.idx >= T[e.tid].numel) { *err = "device reload: an entry leaves its tensor"; return false; }
            const PackTensor& t = T[e.tid];
            if (t.fold_kind == 1) {
                const PackTensor& g = T[t.fold_gamma];
                const size_t ch = (size_t)e.idx / (t.numel / (size_t)t.shape[0]);
                if (ch >= g.numel || ch >= T[g.mean].numel || ch >= T[g.var].numel) { *err = "device reload: a channel leaves its BatchNorm"; return false; }
            }
            if (t.fold_kind == 2 && ((size_t)e.idx >= T[t.gamma].numel || (size_t)e.idx >= T[t.mean].numel || (size_t)e.idx >= T[t.var].numel)) {
                *err = "device reload: a channel leaves its BatchNorm";
                return false;
            }
        }
    }
    return true;
}

// a bound tensor as the kernels see it
struct PackSrc {
    const float* p;
    const float *gamma, *mean, *var;  // kind != 0
    int kind;                         // 0 copy; 1 p[i] * alpha[i / inner]; 2 p = beta: p[i] - mean[i] * alpha[i]
    int inner;
};

}  // namespace mz

#ifdef __HIPCC__
#include "mz_conv_split.h"

namespace mz {

// The fold of build_conv / build_head (mz_convnet.h), float32 operation by operation: invstd = 1 / sqrt(var + eps), alpha = invstd * gamma,
// m = mean * alpha, bias = beta - m, w' = w * alpha.  No contraction (the library is built with -ffp-contract=off; the pragma says so
// here as well), correctly rounded division and square root (hipcc's default; never rsqrt).
__host__ __device__ __forceinline__ float pack_value(const PackSrc* __restrict__ srcs, int tid, int idx) {
#pragma clang fp contract(off)
    if (tid < 0) return 0.0f;
    const PackSrc S = srcs[tid];
    const float x = S.p[idx];
    if (S.kind == 0) return x;
    const int ch = S.kind == 1 ? idx / S.inner : idx;
    const float invstd = 1.0f / sqrtf(S.var[ch] + 1e-5f);
    const float alpha = invstd * S.gamma[ch];
    if (S.kind == 1) return x * alpha;
    const float m = S.mean[ch] * alpha;
    return x - m;
}

__global__ __launch_bounds__(256) void k_pack_f32(const PackChunk* __restrict__ chunks, const PackEntry* __restrict__ map,
                                                   const PackSrc* __restrict__ srcs, void* const* __restrict__ dst) {
    const PackChunk c = chunks[blockIdx.x];
    const int i = 4 * threadIdx.x;
    if (i >= c.n) return;
    const PackEntry* e = map + c.map + i;
    float* d = static_cast<float*>(dst[c.buf]) + c.off + i;
    if (i + 4 <= c.n) {
        const int4 e01 = *reinterpret_cast<const int4*>(e), e23 = *reinterpret_cast<const int4*>(e + 2);
        float4 v;
        v.x = pack_value(srcs, e01.x, e01.y);
        v.y = pack_value(srcs, e01.z, e01.w);
        v.z = pack_value(srcs, e23.x, e23.y);
        v.w = pack_value(srcs, e23.z, e23.w);
        *reinterpret_cast<float4*>(d) = v;
    } else {
        for (int j = 0; i + j < c.n; j++) d[j] = pack_value(srcs, e[j].tid, e[j].idx);
    }
}

// eight consecutive positions of one group per lane: h, m, l of each value (conv_split3: the host's rounding), one 16-byte store per term
__global__ __launch_bounds__(256) void k_pack_w3(const PackChunk* __restrict__ chunks, const PackEntry* __restrict__ map,
                                                  const PackSrc* __restrict__ srcs, void* const* __restrict__ dst) {
    const PackChunk c = chunks[blockIdx.x];
    const int i = 8 * threadIdx.x;
    if (i + 8 > c.n) return;  // (counts are multiples of 512)
    const PackEntry* e = map + c.map + i;
    const size_t q = (size_t)c.off + i;
    unsigned short* d = static_cast<unsigned short*>(dst[c.buf]) + (q / 512) * 1536 + q % 512;
    unsigned t[3][4];
#pragma unroll
    for (int j = 0; j < 8; j += 2) {
        const int4 ee = *reinterpret_cast<const int4*>(e + j);
        unsigned h0, m0, l0, h1, m1, l1;
        conv_split3(pack_value(srcs, ee.x, ee.y), h0, m0, l0);
        conv_split3(pack_value(srcs, ee.z, ee.w), h1, m1, l1);
        t[0][j / 2] = (h0 & 0xffffu) | (h1 << 16);
        t[1][j / 2] = (m0 & 0xffffu) | (m1 << 16);
        t[2][j / 2] = (l0 & 0xffffu) | (l1 << 16);
    }
#pragma unroll
    for (int k = 0; k < 3; k++) *reinterpret_cast<uint4*>(d + 512 * k) = make_uint4(t[k][0], t[k][1], t[k][2], t[k][3]);
}

}  // namespace mz
#endif  // __HIPCC__
