// host_entry.h -- what the C entries of every host file share: the error guard of an entry, one device allocation, a checkpoint's tensor
// table with bf16 widening, the two "does this view lie inside its buffer" tests, and the device copies of a direct kernel entry on host arrays.
// The device check itself (require_device / open_device) is declared in common.h: engine.cc and pipeline.cc use it without this header.
#pragma once
#include <algorithm>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "common.h"

namespace oar {

// No exception crosses a C entry: the status, and the text for oar_last_error.
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

struct DevMem {   // one allocation, freed with its owner
    void* p = nullptr;
    ~DevMem() { if (p) { (void)hipFree(p); (void)hipGetLastError(); } }
    void alloc(size_t bytes) { OAR_HIP(hipMalloc(&p, std::max<size_t>(bytes, 16))); }
    void upload(const void* src, size_t bytes) { alloc(bytes); OAR_HIP(hipMemcpy(p, src, bytes, hipMemcpyHostToDevice)); }
};

struct Table {   // a checkpoint's tensors by name
    std::string who;   // the entry the messages name
    std::map<std::string, const oar_lm_tensor*> by_name;
    Table(const char* who_, const oar_lm_tensor* tensors, int32_t n) : who(who_) {
        for (int32_t i = 0; i < n; ++i)
            if (tensors[i].name) by_name[tensors[i].name] = &tensors[i];
    }
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

inline std::vector<float> widen(const oar_lm_tensor& t, size_t n) {   // the first n values as f32
    std::vector<float> v(n);
    if (t.dtype == OAR_LM_F32) std::memcpy(v.data(), t.data, n * 4);
    else
        for (size_t i = 0; i < n; ++i) {
            const uint32_t u = (uint32_t) static_cast<const uint16_t*>(t.data)[i] << 16;
            std::memcpy(&v[i], &u, 4);
        }
    return v;
}

// rows of `width` at stride ld from off: off + (rows - 1) ld + width <= total, with rows, ld, width below 2^31 (the *_supported limits): no product or sum can wrap
inline bool view_fits(size_t off, int64_t rows, int64_t ld, int64_t width, size_t total) {
    const uint64_t need = (uint64_t)(rows - 1) * (uint64_t)ld + (uint64_t)width;
    return off <= total && need <= total - off;
}
// `count` contiguous elements from off
inline bool view_fits(size_t off, uint64_t count, size_t total) { return off <= total && count <= total - off; }

// The device copies of one direct kernel entry (oar_k_* on host arrays).  The entry checks its arguments, asks for the device, and only then calls in / io /
// out / scratch -- nothing is allocated and no device function is touched before the first of them, so a bad call answers the same without a GPU.  The copies
// are synchronous and the launch goes to the null stream, as the entries always did; everything is freed on every way out, a throw included.
class DirectCall {
    struct Back { void* host; const void* dev; size_t bytes; };
    std::vector<std::unique_ptr<DevMem>> mem_;
    std::vector<Back> back_;
    DevMem& fresh() { mem_.emplace_back(new DevMem()); return *mem_.back(); }

public:
    template <class T>
    const T* in(const T* host, size_t bytes, size_t lead = 0) {   // uploaded now; null in, null out.  lead: the copy begins that many bytes into its allocation (a base off its alignment)
        if (!host) return nullptr;
        fresh().alloc(bytes + lead);
        char* at = static_cast<char*>(mem_.back()->p) + lead;
        OAR_HIP(hipMemcpy(at, host, bytes, hipMemcpyHostToDevice));
        return reinterpret_cast<const T*>(at);
    }
    template <class T>
    T* io(T* host, size_t count) {   // uploaded now, downloaded by finish()
        fresh().upload(host, count * sizeof(T));
        back_.push_back({host, mem_.back()->p, count * sizeof(T)});
        return static_cast<T*>(mem_.back()->p);
    }
    template <class T>
    T* out(T* host, size_t bytes, size_t alloc_bytes = 0, size_t lead = 0) {   // not uploaded; `bytes` from `lead` on are downloaded by finish()
        fresh().alloc(std::max(bytes, alloc_bytes) + lead);
        char* at = static_cast<char*>(mem_.back()->p) + lead;
        back_.push_back({host, at, bytes});
        return reinterpret_cast<T*>(at);
    }
    template <class T = void>
    T* scratch(size_t bytes, int fill = -1) {   // neither way; fill: a byte value (0xFF shows a word read before it was written as NaN); no bytes, no buffer
        if (!bytes) return nullptr;
        fresh().alloc(bytes);
        if (fill >= 0) OAR_HIP(hipMemset(mem_.back()->p, fill, bytes));
        return static_cast<T*>(mem_.back()->p);
    }
    void finish() {   // after the launch
        OAR_HIP(hipGetLastError());
        for (const Back& b : back_) OAR_HIP(hipMemcpy(b.host, b.dev, b.bytes, hipMemcpyDeviceToHost));
    }
};

}  // namespace oar
