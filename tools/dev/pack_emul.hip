// Host-only check of the device reload (muzero_amd/csrc/mz_pack.h) for conv nets, no GPU needed: the REAL host packers (mz_convnet.h) with
// hipMalloc / hipMemcpy mapped to the host heap, probes -> decode -> chunks -> bounds -> the gather kernels' arithmetic on the host, compared
// byte for byte with the host build of the real values.  Meant for the host sanitizers, which then also watch the packers and the decoder:
//     python tools/dev/pack_emul_dump.py board3 /tmp/pe
//     hipcc --offload-arch=gfx950 -O1 -g -ffp-contract=off -std=c++17 -Xarch_host -fsanitize=address,undefined -Imuzero_amd/csrc
//           tools/dev/pack_emul.hip   (one command line) -o /tmp/pe/pack_emul
//     ASAN_OPTIONS=detect_leaks=0 /tmp/pe/pack_emul /tmp/pe/board3 0      # 1: conv_precision bf16x3   (the nets are not freed: no leak check)
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
static hipError_t h_malloc_v(void** p, size_t n) { *p = calloc(1, n ? n : 1); return hipSuccess; }
template <class T> static hipError_t h_malloc(T** p, size_t n) { return h_malloc_v(reinterpret_cast<void**>(p), n); }
static hipError_t h_memcpy(void* d, const void* s, size_t n, hipMemcpyKind) { memcpy(d, s, n); return hipSuccess; }
static hipError_t h_free(void* p) { free(p); return hipSuccess; }
#define hipMalloc h_malloc
#define hipMemcpy h_memcpy
#define hipFree h_free
#include "mz_convnet.h"
using namespace mz;
struct Ten { std::string name; std::vector<int64_t> shape; std::vector<float> data; };
static unsigned rne(unsigned u) { return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16; }
int main(int argc, char** argv) {
    const std::string base = argv[1];
    const int split = argc > 2 ? atoi(argv[2]) : 0;
    std::ifstream f(base + ".txt"), b(base + ".bin", std::ios::binary);
    ConvNetDev cfg;
    std::string line; std::getline(f, line);
    { std::istringstream s(line); s >> cfg.kind >> cfg.in_c >> cfg.in_h >> cfg.in_w >> cfg.A >> cfg.R >> cfg.P >> cfg.Sv >> cfg.Sr; }
    cfg.split = split; cfg.hh = cfg.kind == 2 ? 6 : cfg.in_h; cfg.hw = cfg.kind == 2 ? 6 : cfg.in_w;
    std::map<std::string, Ten> real;
    while (std::getline(f, line)) {
        std::istringstream s(line); Ten t; int nd; s >> t.name >> nd; size_t n = 1;
        for (int i = 0; i < nd; i++) { int64_t d; s >> d; t.shape.push_back(d); n *= d; }
        t.data.resize(n); b.read(reinterpret_cast<char*>(t.data.data()), n * 4); real[t.name] = t;
    }
    auto build = [&](std::map<std::string, Ten>& tens, ConvNetDev& n, std::vector<PackBufferRef>& bufs) {
        n = cfg; ParamMap pm; for (auto& kv : tens) pm[kv.first] = HostTensorRef{kv.second.data.data(), kv.second.shape};
        std::string err; int rc = convnet_build(n, pm, &err); if (rc) { printf("build failed: %s\n", err.c_str()); exit(1); }
        bufs.clear(); convnet_packed_buffers(n, bufs);
    };
    ConvNetDev nr; std::vector<PackBufferRef> br; build(real, nr, br);
    std::vector<PackTensor> T;
    for (auto& kv : real) { PackTensor t; t.name = kv.first; t.shape = kv.second.shape; t.numel = kv.second.data.size(); T.push_back(t); }
    pack_assign_roles(T);
    const float uv = pack_unit_var();
    std::map<std::string, Ten> fake = real;
    ConvNetDev np[3]; std::vector<PackBufferRef> bp[3];
    for (int pass = 0; pass < 3; pass++) {
        for (size_t i = 0; i < T.size(); i++) pack_probe_values(T[i], (int)i, pass, uv, fake[T[i].name].data.data());
        build(fake, np[pass], bp[pass]);
        if (bp[pass].size() != br.size()) { printf("buffer count differs\n"); return 1; }
    }
    std::vector<PackChunk> cf, cw; std::vector<PackEntry> map, ent; std::vector<size_t> elems(br.size(), 0); std::string err;
    for (size_t i = 0; i < br.size(); i++) {
        if (br[i].kind == PACK_STATIC) { if (memcmp(br[i].d, bp[2][i].d, br[i].bytes)) { printf("static buffer %s differs\n", br[i].label.c_str()); return 1; } continue; }
        const bool w3 = br[i].kind == PACK_W3;
        const size_t n = w3 ? br[i].bytes / 6 : br[i].bytes / 4; elems[i] = n; ent.resize(n);
        bool ok = w3 ? pack_decode_w3((const uint16_t*)bp[0][i].d, (const uint16_t*)bp[1][i].d, (const uint16_t*)bp[2][i].d, n, T, ent.data(), &err)
                     : pack_decode_f32((const float*)bp[0][i].d, (const float*)bp[1][i].d, (const float*)bp[2][i].d, n, T, ent.data(), &err);
        if (!ok) { printf("decode of %s failed: %s\n", br[i].label.c_str(), err.c_str()); return 1; }
        pack_make_chunks((int)i, n, w3 ? PACK_CHUNK_W3 : PACK_CHUNK_F32, ent.data(), w3 ? cw : cf, map);
    }
    if (!pack_check_bounds(cf, map, T, elems, &err) || !pack_check_bounds(cw, map, T, elems, &err)) { printf("bounds: %s\n", err.c_str()); return 1; }
    std::vector<PackSrc> srcs(T.size());
    for (size_t i = 0; i < T.size(); i++) {
        auto ptr = [&](int id) { return id >= 0 ? real[T[id].name].data.data() : nullptr; };
        PackSrc s{}; s.p = ptr((int)i); s.kind = T[i].fold_kind < 0 ? 0 : T[i].fold_kind; s.inner = 1;
        if (s.kind == 1) { const PackTensor& g = T[T[i].fold_gamma]; s.gamma = ptr(g.gamma); s.mean = ptr(g.mean); s.var = ptr(g.var); s.inner = (int)(T[i].numel / T[i].shape[0]); }
        else if (s.kind == 2) { s.gamma = ptr(T[i].gamma); s.mean = ptr(T[i].mean); s.var = ptr(T[i].var); }
        srcs[i] = s;
    }
    std::vector<std::vector<unsigned char>> out(br.size());
    for (size_t i = 0; i < br.size(); i++) out[i].assign(br[i].bytes, 0xAB);
    for (const PackChunk& c : cf) for (int t = 0; t < 256; t++) {  // k_pack_f32
        const int i = 4 * t; if (i >= c.n) continue;
        float* d = reinterpret_cast<float*>(out[c.buf].data()) + c.off + i; const PackEntry* e = map.data() + c.map + i;
        for (int j = 0; j < 4 && i + j < c.n; j++) d[j] = pack_value(srcs.data(), e[j].tid, e[j].idx);
    }
    for (const PackChunk& c : cw) for (int t = 0; t < 256; t++) {  // k_pack_w3
        const int i = 8 * t; if (i + 8 > c.n) continue;
        const size_t q = (size_t)c.off + i; uint16_t* d = reinterpret_cast<uint16_t*>(out[c.buf].data()) + (q / 512) * 1536 + q % 512;
        for (int j = 0; j < 8; j++) { float r = pack_value(srcs.data(), map[c.map + i + j].tid, map[c.map + i + j].idx);
            for (int k = 0; k < 3; k++) { unsigned u; memcpy(&u, &r, 4); unsigned bb = rne(u), bk = bb << 16; float ff; memcpy(&ff, &bk, 4); r = r - ff; d[512 * k + j] = (uint16_t)bb; } }
    }
    size_t total = 0; int bad = 0;
    for (size_t i = 0; i < br.size(); i++) {
        if (br[i].kind == PACK_STATIC) continue;
        total += br[i].bytes;
        if (memcmp(out[i].data(), br[i].d, br[i].bytes)) { printf("MISMATCH in %s\n", br[i].label.c_str()); bad++; }
    }
    printf("%s split=%d: %zu buffers, %zu bytes, %zu chunks, %zu entries, mismatching buffers: %d\n", base.c_str(), split, br.size(), total, cf.size() + cw.size(), map.size(), bad);
    return bad != 0;
}
