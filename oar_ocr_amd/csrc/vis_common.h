// vis_common.h -- what is specific to the hosts of the vision towers (vis_host.cc: PaddleOCR-VL; qvis_host.cc: Qwen2-VL / Qwen2.5-VL)
// on top of host_entry.h: a Linear as a 1x1 implicit GEMM with its weights packed once in the kernel's fragment order, the device, stream and allocations one
// tower owns, and the (segment, tile) tables of k::vis_attention -- built from segment lengths on the host, kept in the model's buffers on the device.
#pragma once
#include <mutex>

#include "engine.h"
#include "host_entry.h"
#include "kernels.h"

namespace oar {
namespace vishost {

struct Lin {   // y [M][N] = act(x [M][K] W^T + b) (+ residual)
    const float *w = nullptr, *b = nullptr;
    int K = 0, N = 0, fmt = 0;
};

inline void run_linear(hipStream_t s, const Lin& l, const float* x, float* y, int M, int act, const float* residual, const char* prof_class = "vis_linear") {
    k::ConvP p{};
    p.w_fmt = l.fmt;
    p.N = 1; p.H = 1; p.W = M; p.Cin = l.K; p.Ho = 1; p.Wo = M; p.Cout = l.N;
    p.kh = p.kw = p.sh = p.sw = p.dh = p.dw = 1; p.groups = 1;
    p.act.kind = act;
    p.x = x; p.w = l.w; p.bias = l.b; p.residual = residual; p.y = y; p.y_ld = l.N;
    k::conv_igemm(s, p, prof_class);
}

struct VisDevice {   // the device, the stream and the allocations of one model
    int device = 0;
    hipStream_t stream = nullptr;
    std::mutex mu;
    std::vector<std::unique_ptr<DevMem>> mem;
    double weight_bytes = 0;
    ~VisDevice() {
        if (stream) {
            Profiler::get().drop_events();
            (void)hipStreamDestroy(stream);
        }
    }
    const float* up(const std::vector<float>& v) {
        mem.emplace_back(new DevMem());
        mem.back()->upload(v.data(), v.size() * 4);
        weight_bytes += 4.0 * v.size();
        return static_cast<const float*>(mem.back()->p);
    }
    template <class T>
    T* raw(size_t count) {
        mem.emplace_back(new DevMem());
        mem.back()->alloc(count * sizeof(T));
        return static_cast<T*>(mem.back()->p);
    }
    // The format is chosen once, from the largest row count the Linear can see, and must then serve EVERY smaller call: bf16x6 weights stay only where
    // k::igemm_x6_serves_any_rows says so (igemm_weight_format also answers bf16x6 for the output-stationary kernel, which refuses small row counts).
    Lin linear(const std::vector<float>& w, const std::vector<float>& b, int N, int K, long rows) {
        Lin l;
        l.K = K; l.N = N;
        l.fmt = k::igemm_weight_format(rows, K, N, true);
        if (l.fmt != k::IGEMM_W_K16 && !(l.fmt == k::IGEMM_W_X6 && k::igemm_x6_serves_any_rows(K, N))) l.fmt = k::IGEMM_W_K16;
        l.w = up(igemm_to_fragments(l.fmt, w, N, K));
        l.b = up(b);
        return l;
    }
};

// lens -> the segments and query tiles of one k::vis_attention launch over them, and what that launch costs
struct HostTables {
    std::vector<k::VisSeg> segs;
    std::vector<k::VisTile> tiles;
    double bytes = 0.0, flops = 0.0;
    void build(const int32_t* lens, int n, int heads, int dh) {
        segs.resize((size_t)n);
        tiles.resize((size_t)k::vis_attention_tile_count(lens, n, heads));
        k::vis_attention_tables(lens, n, heads, segs.data(), tiles.data());
        k::vis_attention_cost(lens, n, heads, dh, &bytes, &flops);
    }
    void build(const std::vector<int32_t>& lens, int heads, int dh) { build(lens.data(), (int)lens.size(), heads, dh); }
};

// the device half: a model's buffers for one table pair and the pair a call put there
struct AttnTables {
    k::VisSeg* segs = nullptr;
    k::VisTile* tiles = nullptr;
    int n_tiles = 0;
    double bytes = 0.0, flops = 0.0;
    void alloc(VisDevice& dev, int max_segs, int max_tiles) {
        segs = dev.raw<k::VisSeg>((size_t)max_segs);
        tiles = dev.raw<k::VisTile>((size_t)max_tiles);
    }
    void put(const HostTables& src, hipStream_t s) {   // (pageable sources: the caller synchronises before src goes)
        OAR_HIP(hipMemcpyAsync(segs, src.segs.data(), src.segs.size() * sizeof(k::VisSeg), hipMemcpyHostToDevice, s));
        OAR_HIP(hipMemcpyAsync(tiles, src.tiles.data(), src.tiles.size() * sizeof(k::VisTile), hipMemcpyHostToDevice, s));
        n_tiles = (int)src.tiles.size(); bytes = src.bytes; flops = src.flops;
    }
};

}  // namespace vishost
}  // namespace oar
