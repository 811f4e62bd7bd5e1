// vis_common.h -- what the hosts of the vision towers share (vis_host.cc: PaddleOCR-VL; qvis_host.cc: Qwen2-VL / Qwen2.5-VL):
// the error guard of a C entry, the device allocations a model owns, the checkpoint's tensor table, bf16 widening, and a Linear as a 1x1 implicit GEMM with
// its weights packed once in the kernel's fragment order.
#pragma once
#include <algorithm>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "common.h"
#include "engine.h"
#include "kernels.h"

namespace oar {
namespace vishost {

template <typename F>
oar_status guard(F&& f) {
    try {
        f();
        return OAR_OK;
    } catch (const Error& e) {
        set_last_error(e.what());
        return e.code;
    } catch (const std::bad_alloc&) {
        set_last_error("host allocation failed");
        return OAR_OOM;
    } catch (const std::exception& e) {
        set_last_error(e.what());
        return OAR_INTERNAL;
    } catch (...) {
        set_last_error("unknown error");
        return OAR_INTERNAL;
    }
}

struct DevMem {   // one allocation, freed with the model
    void* p = nullptr;
    ~DevMem() { if (p) { (void)hipFree(p); (void)hipGetLastError(); } }
    void alloc(size_t bytes) { OAR_HIP(hipMalloc(&p, std::max<size_t>(bytes, 16))); }
    void upload(const void* src, size_t bytes) { alloc(bytes); OAR_HIP(hipMemcpy(p, src, bytes, hipMemcpyHostToDevice)); }
};

struct Table {
    std::string who;   // the entry the messages name
    std::map<std::string, const oar_lm_tensor*> by_name;
    const oar_lm_tensor& need(const std::string& name, int64_t d0, int64_t d1) const {   // [d0] (d1 < 0) or [d0, d1]
        auto it = by_name.find(name);
        OAR_CHECK(it != by_name.end(), OAR_INVALID_INPUT, who + ": tensor '" + name + "' is missing");
        const oar_lm_tensor& t = *it->second;
        OAR_CHECK(t.data != nullptr, OAR_INVALID_INPUT, who + ": tensor '" + name + "' has no data");
        OAR_CHECK(t.dtype == OAR_LM_F32 || t.dtype == OAR_LM_BF16, OAR_INVALID_INPUT, who + ": tensor '" + name + "' is neither f32 nor bf16");
        const bool ok = d1 < 0 ? (t.rank == 1 && t.dims[0] == d0) : (t.rank == 2 && t.dims[0] == d0 && t.dims[1] == d1);
        OAR_CHECK(ok, OAR_INVALID_INPUT, who + ": tensor '" + name + "' has the wrong shape");
        return t;
    }
};

inline std::vector<float> widen(const oar_lm_tensor& t, size_t n) {
    std::vector<float> v(n);
    if (t.dtype == OAR_LM_F32) std::memcpy(v.data(), t.data, n * 4);
    else
        for (size_t i = 0; i < n; ++i) {
            const uint32_t u = (uint32_t) static_cast<const uint16_t*>(t.data)[i] << 16;
            std::memcpy(&v[i], &u, 4);
        }
    return v;
}

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

struct VisDevice {   // the allocations of one model
    std::vector<std::unique_ptr<DevMem>> mem;
    double weight_bytes = 0;
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

}  // namespace vishost
}  // namespace oar
