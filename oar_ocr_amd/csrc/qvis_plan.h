// qvis_plan.h -- the host routines of the Qwen vision towers that need no device: the argument checks, the window plan of the Qwen2.5-VL
// tower, and the rotary tables.  Plain C++ (no HIP header), so a host-only test compiles them into a program of its own, sanitizers on.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/oar_mi355x.h"

namespace oar {
namespace qvis {

constexpr int kMaxImages = 16;

struct Status {
    oar_status code = OAR_OK;
    std::string msg;
    bool ok() const { return code == OAR_OK; }
};
inline Status bad(oar_status c, const std::string& m) { return Status{c, m}; }

// every check of a configuration; head_ok: the attention kernel's own rule (k::vis_attention_supported)
inline Status check_cfg(const oar_qvis_cfg& c, bool (*head_ok)(int64_t, int64_t)) {
    const char* who = "oar_qvis: ";
    if (c.kind != OAR_QVIS_QWEN2 && c.kind != OAR_QVIS_QWEN2_5) return bad(OAR_INVALID_INPUT, std::string(who) + "kind is neither OAR_QVIS_QWEN2 nor OAR_QVIS_QWEN2_5");
    if (!(c.embed > 0 && c.layers > 0 && c.heads > 0 && c.intermediate > 0 && c.patch > 0 && c.temporal_patch > 0 && c.channels > 0 && c.merge > 0 && c.out_hidden > 0))
        return bad(OAR_INVALID_INPUT, std::string(who) + "embed, layers, heads, intermediate, patch, temporal_patch, channels, merge and out_hidden must be positive");
    if (!(c.embed < (1 << 20) && c.intermediate < (1 << 20) && c.out_hidden < (1 << 20) && c.patch <= 64 && c.temporal_patch <= 8 && c.channels <= 16 && c.merge <= 8 && c.layers <= 1024))
        return bad(OAR_INVALID_INPUT, std::string(who) + "a dimension out of range");
    if (c.embed % c.heads != 0) return bad(OAR_INVALID_INPUT, std::string(who) + "embed is no multiple of heads");
    const int64_t kp = (int64_t)c.channels * c.temporal_patch * c.patch * c.patch;
    if (kp % 4 != 0 || c.embed % 4 != 0 || c.intermediate % 4 != 0 || c.out_hidden % 4 != 0)
        return bad(OAR_INVALID_INPUT, std::string(who) + "channels temporal_patch patch^2, embed, intermediate and out_hidden must be multiples of 4 (rows are read 16 bytes at a time)");
    if (!(c.rope_theta > 0.0f)) return bad(OAR_INVALID_INPUT, std::string(who) + "rope_theta must be positive");
    if (!(c.max_images >= 1 && c.max_images <= kMaxImages)) return bad(OAR_INVALID_INPUT, std::string(who) + "max_images must be in 1..16");
    if (!(c.max_tokens >= c.merge * c.merge && c.max_tokens <= (1 << 22))) return bad(OAR_INVALID_INPUT, std::string(who) + "max_tokens must be in merge^2..2^22");
    if (c.kind == OAR_QVIS_QWEN2_5) {
        const int unit = c.merge * c.patch;
        if (c.window_size <= 0 || c.window_size % unit != 0) return bad(OAR_INVALID_INPUT, std::string(who) + "window_size must be a positive multiple of merge * patch");
        if (c.n_fullatt < 0 || c.n_fullatt > c.layers || (c.n_fullatt > 0 && !c.fullatt_block_indexes)) return bad(OAR_INVALID_INPUT, std::string(who) + "n_fullatt outside 0..layers or null indexes");
        for (int i = 0; i < c.n_fullatt; ++i)
            if (c.fullatt_block_indexes[i] < 0 || c.fullatt_block_indexes[i] >= c.layers) return bad(OAR_INVALID_INPUT, std::string(who) + "a full-attention block index is not below layers");
    }
    if (c.act != OAR_QVIS_QUICK_GELU && c.act != OAR_QVIS_SILU && c.act != OAR_QVIS_GELU_ERF) return bad(OAR_UNSUPPORTED_OP, std::string(who) + "unknown hidden_act");
    if (!head_ok(c.heads, c.embed / c.heads)) return bad(OAR_UNSUPPORTED_OP, std::string(who) + "the head size must be a multiple of 8 in 8..80");
    return Status{};
}

// grids [n][2] = (h, w): every check of a request's composition; *total: the number of patches
inline Status check_grids(int merge, int max_images, int64_t max_tokens, int32_t n, const int32_t* grids, int64_t* total) {
    if (!(n >= 1 && n <= max_images)) return bad(OAR_INVALID_INPUT, "oar_qvis: n_images outside 1..max_images");
    if (!grids) return bad(OAR_INVALID_INPUT, "oar_qvis: null grids");
    int64_t t = 0;
    for (int i = 0; i < n; ++i) {
        const int64_t h = grids[2 * i], w = grids[2 * i + 1];
        if (!(h >= 1 && w >= 1 && h <= (1 << 15) && w <= (1 << 15))) return bad(OAR_INVALID_INPUT, "oar_qvis: a grid side outside 1..32768");
        if (h % merge != 0 || w % merge != 0) return bad(OAR_INVALID_INPUT, "oar_qvis: a grid side is no multiple of merge");
        t += h * w;
        if (t > max_tokens) return bad(OAR_INVALID_INPUT, "oar_qvis: the images hold more patches than max_tokens");
    }
    *total = t;
    return Status{};
}

struct Plan {
    std::vector<int32_t> window_index, reverse_index;   // [units]: slot -> source unit, and its inverse
    std::vector<int32_t> seg_start, seg_len;            // the windows, in patches
};

// Merge units (merge x merge patches) in window order.  window_side = window_size / (merge patch) units; every image is cut into windows of that side, the
// last row and column of windows partial; a window without units yields no segment; an image's units are offset by the units of the images in front of it.
inline Status window_plan(int merge, int patch, int window_size, int32_t n, const int32_t* grids, Plan* out) {
    if (merge <= 0 || patch <= 0 || merge > 64 || patch > 1024) return bad(OAR_INVALID_INPUT, "oar_qvis_window_plan: merge or patch out of range");
    const int unit = merge * patch;
    if (window_size <= 0 || window_size % unit != 0) return bad(OAR_INVALID_INPUT, "oar_qvis_window_plan: window_size must be a positive multiple of merge * patch");
    if (n < 0 || (n > 0 && !grids)) return bad(OAR_INVALID_INPUT, "oar_qvis_window_plan: bad grids");
    const int64_t side = window_size / unit, m2 = (int64_t)merge * merge;
    out->window_index.clear(); out->seg_start.clear(); out->seg_len.clear();
    int64_t base = 0, at = 0;
    for (int i = 0; i < n; ++i) {
        const int64_t h = grids[2 * i], w = grids[2 * i + 1];
        if (!(h >= 1 && w >= 1 && h <= (1 << 15) && w <= (1 << 15)) || h % merge || w % merge) return bad(OAR_INVALID_INPUT, "oar_qvis_window_plan: a grid side outside 1..32768 or no multiple of merge");
        const int64_t uh = h / merge, uw = w / merge;
        if ((base + uh * uw) * m2 >= ((int64_t)1 << 31)) return bad(OAR_INVALID_INPUT, "oar_qvis_window_plan: too many patches");
        const int64_t nwh = (uh + side - 1) / side, nww = (uw + side - 1) / side;
        for (int64_t wh = 0; wh < nwh; ++wh)
            for (int64_t ww = 0; ww < nww; ++ww) {
                int64_t count = 0;
                for (int64_t ih = 0; ih < side; ++ih)
                    for (int64_t iw = 0; iw < side; ++iw) {
                        const int64_t row = wh * side + ih, col = ww * side + iw;
                        if (row < uh && col < uw) { out->window_index.push_back((int32_t)(base + row * uw + col)); ++count; }
                    }
                if (count > 0) { out->seg_start.push_back((int32_t)at); out->seg_len.push_back((int32_t)(count * m2)); at += count * m2; }
            }
        base += uh * uw;
    }
    out->reverse_index.assign(out->window_index.size(), 0);
    for (size_t slot = 0; slot < out->window_index.size(); ++slot) out->reverse_index[(size_t)out->window_index[slot]] = (int32_t)slot;
    return Status{};
}

// cos / sin [T][dh / 2] for the packed patches in merge-grouped order (hb, wb, mi, mj): [row part (dh / 4) | column part (dh / 4)], angle = position x
// frequency in f32.  window_index (null: none): the rows are then laid out in window order, unit by unit.
inline void rotary_tables(int32_t n, const int32_t* grids, int merge, int dh, const std::vector<float>& inv_freq, const int32_t* window_index, std::vector<float>* cs, std::vector<float>* sn) {
    const int q4 = dh / 4, h2 = dh / 2, m2 = merge * merge;
    std::vector<int32_t> hp, wp;
    for (int i = 0; i < n; ++i) {
        const int h = grids[2 * i], w = grids[2 * i + 1];
        for (int hb = 0; hb < h / merge; ++hb)
            for (int wb = 0; wb < w / merge; ++wb)
                for (int mi = 0; mi < merge; ++mi)
                    for (int mj = 0; mj < merge; ++mj) { hp.push_back(hb * merge + mi); wp.push_back(wb * merge + mj); }
    }
    const size_t T = hp.size();
    cs->assign(T * (size_t)h2, 0.0f); sn->assign(T * (size_t)h2, 0.0f);
    for (size_t t = 0; t < T; ++t) {
        const size_t src = window_index ? (size_t)window_index[t / (size_t)m2] * (size_t)m2 + t % (size_t)m2 : t;
        const float row = (float)hp[src], col = (float)wp[src];
        float* cr = cs->data() + t * (size_t)h2;
        float* sr = sn->data() + t * (size_t)h2;
        for (int j = 0; j < q4; ++j) {
            const float ar = row * inv_freq[(size_t)j], ac = col * inv_freq[(size_t)j];
            cr[j] = std::cos(ar); sr[j] = std::sin(ar); cr[q4 + j] = std::cos(ac); sr[q4 + j] = std::sin(ac);
        }
    }
}

inline std::vector<float> inv_freq_of(int dh, float theta) {
    std::vector<float> f((size_t)dh / 4);
    for (int j = 0; j < dh / 4; ++j) f[(size_t)j] = (float)(1.0 / std::pow((double)theta, 2.0 * j / (dh / 2)));
    return f;
}

}  // namespace qvis
}  // namespace oar
