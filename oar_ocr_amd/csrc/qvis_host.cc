// qvis_host.cc -- host side of the Qwen2-VL and Qwen2.5-VL vision towers, a sibling of vis_host.cc: checks a checkpoint's tensor table, stacks
// gate / up, packs the matrices in the implicit-GEMM kernel's fragment order, uploads them, and drives one call as a fixed chain of launches over the packed
// patches of all its images.  C ABI: oar_qvis_create / encode / cost / check / destroy, oar_qvis_window_plan, and the direct entries of qvis_misc.hip.
// The Linears are k::conv_igemm as 1x1 layers, the LayerNorms k::layernorm, the attention k::vis_attention with one of two (segment, tile) table pairs --
// windows or images -- and the rest qvis_misc.hip.  The entry guard, the device check, the tensor table, the allocations and the direct entries' device
// copies come from host_entry.h; the stream a tower owns and the table pairs (HostTables / AttnTables) from vis_common.h.
#include <cmath>

#include "qvis.h"
#include "qvis_plan.h"
#include "vis_common.h"

using namespace oar;
using namespace oar::vishost;

namespace {

bool head_ok(int64_t heads, int64_t dh) { return k::vis_attention_supported(heads, dh); }

void raise(const qvis::Status& st) {
    if (!st.ok()) fail(st.code, st.msg);
}

struct BlockW {
    const float *n1g = nullptr, *n1b = nullptr, *n2g = nullptr, *n2b = nullptr;
    Lin qkv, proj, up, down;   // up: fc1, or the stacked [gate; up]
    bool full = true;          // attends over whole images
};
struct BlockT { const oar_lm_tensor *n1g, *n1b, *n2g, *n2b, *qw, *qb, *pw, *pb, *aw, *ab, *bw, *bb, *dw, *db; };

int per_block(const oar_qvis_cfg& c) { return c.kind == OAR_QVIS_QWEN2 && c.act != OAR_QVIS_QUICK_GELU ? 7 : 8; }

bool is_full(const oar_qvis_cfg& c, const std::vector<int32_t>& fullatt, int layer) {
    if (c.kind == OAR_QVIS_QWEN2) return true;
    return std::find(fullatt.begin(), fullatt.end(), layer) != fullatt.end();
}

}  // namespace

struct oar_qvis : VisDevice {
    oar_qvis_cfg cfg{};
    std::vector<int32_t> fullatt;
    std::vector<BlockW> blocks;
    Lin patch, m0, m2;
    const float *lng = nullptr, *lnb = nullptr;
    float *pix = nullptr, *x = nullptr, *x2 = nullptr, *xn = nullptr, *qkv = nullptr, *att = nullptr, *h = nullptr, *hg = nullptr, *ph = nullptr, *emb = nullptr, *emb2 = nullptr;
    float *cos = nullptr, *sin = nullptr;
    int32_t *widx = nullptr, *ridx = nullptr;
    AttnTables win, img;
    int max_segs = 0, max_tiles = 0;
    std::vector<float> inv_freq;
};

namespace {

struct CallPlan {   // img, win: the two table pairs of a call, on the host
    int T = 0;
    std::vector<int32_t> img_lens;
    qvis::Plan plan;   // QWEN2_5 only
    HostTables img, win;
};

CallPlan plan_call(const oar_qvis_cfg& c, int32_t n, const int32_t* grids) {
    CallPlan p;
    int64_t total = 0;
    raise(qvis::check_grids(c.merge, c.max_images, c.max_tokens, n, grids, &total));
    p.T = (int)total;
    for (int i = 0; i < n; ++i) p.img_lens.push_back(grids[2 * i] * grids[2 * i + 1]);
    const int dh = c.embed / c.heads;
    p.img.build(p.img_lens, c.heads, dh);
    if (c.kind == OAR_QVIS_QWEN2_5) {
        raise(qvis::window_plan(c.merge, c.patch, c.window_size, n, grids, &p.plan));
        OAR_CHECK((int64_t)p.plan.window_index.size() * c.merge * c.merge == total, OAR_INTERNAL, "oar_qvis: the window plan does not cover the patches");
        p.win.build(p.plan.seg_len, c.heads, dh);
    }
    return p;
}

}  // namespace

oar_status oar_qvis_check(const oar_qvis_cfg* cfg, int32_t n_images, const int32_t* grids_hw) {
    return guard([&] {
        OAR_CHECK(cfg, OAR_INVALID_INPUT, "oar_qvis_check: null cfg");
        raise(qvis::check_cfg(*cfg, head_ok));
        if (n_images != 0 || grids_hw) {
            int64_t total = 0;
            raise(qvis::check_grids(cfg->merge, cfg->max_images, cfg->max_tokens, n_images, grids_hw, &total));
        }
    });
}

oar_status oar_qvis_window_plan(int32_t merge, int32_t patch, int32_t window_size, int32_t n_images, const int32_t* grids_hw, int32_t* window_index, int32_t* reverse_index,
                                int32_t* seg_start, int32_t* seg_len, int32_t* n_seg) {
    return guard([&] {
        OAR_CHECK(window_index && reverse_index && seg_start && seg_len && n_seg, OAR_INVALID_INPUT, "oar_qvis_window_plan: null output");
        qvis::Plan p;
        raise(qvis::window_plan(merge, patch, window_size, n_images, grids_hw, &p));
        std::copy(p.window_index.begin(), p.window_index.end(), window_index);
        std::copy(p.reverse_index.begin(), p.reverse_index.end(), reverse_index);
        std::copy(p.seg_start.begin(), p.seg_start.end(), seg_start);
        std::copy(p.seg_len.begin(), p.seg_len.end(), seg_len);
        *n_seg = (int32_t)p.seg_len.size();
    });
}

oar_status oar_qvis_create(const oar_qvis_cfg* cfg, const oar_lm_tensor* tensors, int32_t n_tensors, int32_t device_id, oar_qvis** out) {
    return guard([&] {
        OAR_CHECK(cfg && out && (tensors || n_tensors == 0) && n_tensors >= 0, OAR_INVALID_INPUT, "oar_qvis_create: null argument");
        *out = nullptr;
        oar_qvis_cfg c = *cfg;
        raise(qvis::check_cfg(c, head_ok));
        const bool q25 = c.kind == OAR_QVIS_QWEN2_5;
        std::vector<int32_t> fullatt;
        if (q25) fullatt.assign(c.fullatt_block_indexes, c.fullatt_block_indexes + c.n_fullatt);
        const Table T("oar_qvis_create", tensors, n_tensors);
        const int D = c.embed, L = c.layers, F = c.intermediate, Kp = c.channels * c.temporal_patch * c.patch * c.patch, m2 = c.merge * c.merge, OH = c.out_hidden, dh = D / c.heads;
        // every tensor is looked up and checked before the device is touched
        const oar_lm_tensor& pw = T.need("patch_embed.proj.weight", D, Kp);
        std::vector<BlockT> bt((size_t)L);
        for (int l = 0; l < L; ++l) {
            const std::string pre = "blocks." + std::to_string(l) + ".";
            BlockT& t = bt[(size_t)l];
            t = BlockT{};
            t.n1g = &T.need(pre + "norm1.weight", D, -1); t.n2g = &T.need(pre + "norm2.weight", D, -1);
            if (!q25) { t.n1b = &T.need(pre + "norm1.bias", D, -1); t.n2b = &T.need(pre + "norm2.bias", D, -1); }
            t.qw = &T.need(pre + "attn.qkv.weight", 3 * (int64_t)D, D); t.qb = &T.need(pre + "attn.qkv.bias", 3 * (int64_t)D, -1);
            t.pw = &T.need(pre + "attn.proj.weight", D, D); t.pb = &T.need(pre + "attn.proj.bias", D, -1);
            if (q25) {
                t.aw = &T.need(pre + "mlp.gate_proj.weight", F, D); t.ab = &T.need(pre + "mlp.gate_proj.bias", F, -1);
                t.bw = &T.need(pre + "mlp.up_proj.weight", F, D); t.bb = &T.need(pre + "mlp.up_proj.bias", F, -1);
                t.dw = &T.need(pre + "mlp.down_proj.weight", D, F); t.db = &T.need(pre + "mlp.down_proj.bias", D, -1);
            } else {
                t.aw = &T.need(pre + "mlp.fc1.weight", F, D); t.ab = &T.need(pre + "mlp.fc1.bias", F, -1);
                t.dw = &T.need(pre + "mlp.fc2.weight", D, F); t.db = &T.need(pre + "mlp.fc2.bias", D, -1);
            }
        }
        const oar_lm_tensor& lng = T.need("merger.ln_q.weight", D, -1);
        const oar_lm_tensor* lnb = q25 ? nullptr : &T.need("merger.ln_q.bias", D, -1);
        const oar_lm_tensor& m0w = T.need("merger.mlp.0.weight", (int64_t)m2 * D, (int64_t)m2 * D);
        const oar_lm_tensor& m0b = T.need("merger.mlp.0.bias", (int64_t)m2 * D, -1);
        const oar_lm_tensor& m2w = T.need("merger.mlp.2.weight", OH, (int64_t)m2 * D);
        const oar_lm_tensor& m2b = T.need("merger.mlp.2.bias", OH, -1);

        open_device(device_id, "oar_qvis_create: no such device");
        std::unique_ptr<oar_qvis> M(new oar_qvis());
        M->fullatt = fullatt;
        c.fullatt_block_indexes = nullptr;   // (the caller's array ends with the call: the copy above is what the model reads)
        M->cfg = c; M->device = device_id;
        OAR_HIP(hipStreamCreateWithFlags(&M->stream, hipStreamNonBlocking));
        const long MTl = c.max_tokens, MPl = c.max_tokens / m2;
        // (a zero bias: the checkpoint's patch Linear has none, and every weight format's kernel reads one)
        M->patch = M->linear(widen(pw, (size_t)D * Kp), std::vector<float>((size_t)D, 0.0f), D, Kp, MTl);
        M->blocks.resize((size_t)L);
        for (int l = 0; l < L; ++l) {
            const BlockT& t = bt[(size_t)l];
            BlockW& W = M->blocks[(size_t)l];
            W.full = is_full(c, fullatt, l);
            W.n1g = M->up(widen(*t.n1g, (size_t)D)); W.n2g = M->up(widen(*t.n2g, (size_t)D));
            if (!q25) { W.n1b = M->up(widen(*t.n1b, (size_t)D)); W.n2b = M->up(widen(*t.n2b, (size_t)D)); }
            W.qkv = M->linear(widen(*t.qw, (size_t)3 * D * D), widen(*t.qb, (size_t)3 * D), 3 * D, D, MTl);
            W.proj = M->linear(widen(*t.pw, (size_t)D * D), widen(*t.pb, (size_t)D), D, D, MTl);
            std::vector<float> w = widen(*t.aw, (size_t)F * D), b = widen(*t.ab, (size_t)F);
            if (q25) {   // [W_gate; W_up]: one Linear gives the stacked result the gated activation reads
                const std::vector<float> w2 = widen(*t.bw, (size_t)F * D), b2 = widen(*t.bb, (size_t)F);
                w.insert(w.end(), w2.begin(), w2.end());
                b.insert(b.end(), b2.begin(), b2.end());
            }
            W.up = M->linear(w, b, q25 ? 2 * F : F, D, MTl);
            W.down = M->linear(widen(*t.dw, (size_t)D * F), widen(*t.db, (size_t)D), D, F, MTl);
        }
        M->lng = M->up(widen(lng, (size_t)D));
        if (lnb) M->lnb = M->up(widen(*lnb, (size_t)D));
        M->m0 = M->linear(widen(m0w, (size_t)m2 * D * m2 * D), widen(m0b, (size_t)m2 * D), m2 * D, m2 * D, MPl);
        M->m2 = M->linear(widen(m2w, (size_t)OH * m2 * D), widen(m2b, (size_t)OH), OH, m2 * D, MPl);
        const size_t MT = (size_t)c.max_tokens, MU = MT / (size_t)m2 + 1;
        M->pix = M->raw<float>(MT * Kp); M->x = M->raw<float>(MT * D); M->x2 = M->raw<float>(MT * D); M->xn = M->raw<float>(MT * D);
        M->qkv = M->raw<float>(MT * 3 * D); M->att = M->raw<float>(MT * D); M->h = M->raw<float>(MT * (size_t)(q25 ? 2 * F : F));
        if (q25) M->hg = M->raw<float>(MT * F);
        M->ph = M->raw<float>(MT * D); M->emb = M->raw<float>(MU * OH);
        if (q25) { M->emb2 = M->raw<float>(MU * OH); M->widx = M->raw<int32_t>(MU); M->ridx = M->raw<int32_t>(MU); }
        M->cos = M->raw<float>(MT * (dh / 2)); M->sin = M->raw<float>(MT * (dh / 2));
        // a window holds at least one merge unit, so a call has at most max_tokens / merge^2 window segments; each segment ends with at most one partial tile
        M->max_segs = (int)MU + c.max_images;
        M->max_tiles = c.heads * (int)((MT + k::kFlashQueries - 1) / k::kFlashQueries + (size_t)M->max_segs);
        M->img.alloc(*M, M->max_segs, M->max_tiles);
        if (q25) M->win.alloc(*M, M->max_segs, M->max_tiles);
        M->inv_freq = qvis::inv_freq_of(dh, c.rope_theta);
        *out = M.release();
    });
}

void oar_qvis_destroy(oar_qvis* vis) {
    if (!vis) return;
    (void)hipSetDevice(vis->device);
    delete vis;
}

oar_status oar_qvis_cost(const oar_qvis* vis, int32_t n_images, const int32_t* grids_hw, double* flops, double* bytes, int32_t* n_kernels) {
    return guard([&] {
        OAR_CHECK(vis, OAR_INVALID_INPUT, "oar_qvis_cost: null model");
        oar_qvis_cfg c = vis->cfg;
        const CallPlan p = plan_call(c, n_images, grids_hw);
        const bool q25 = c.kind == OAR_QVIS_QWEN2_5;
        const double T = p.T, D = c.embed, F = c.intermediate, Kp = (double)c.channels * c.temporal_patch * c.patch * c.patch, m2 = (double)c.merge * c.merge, OH = c.out_hidden, L = c.layers;
        double ab = 0.0, af = 0.0;
        for (const BlockW& W : vis->blocks) { ab += W.full ? p.img.bytes : p.win.bytes; af += W.full ? p.img.flops : p.win.flops; }
        const double macs = T * (Kp * D + L * (4.0 * D * D + (q25 ? 3.0 : 2.0) * D * F)) + (T / m2) * (m2 * D * m2 * D + m2 * D * OH);
        // rows read and written per launch: patch Linear (pix, x); per block norm 2, qkv 4, proj 3, norm 2 (in D), the MLP (QWEN2: fc1 D + F, act 2 F unless in the
        // epilogue, fc2 F + 2 D; QWEN2_5: gate / up D + 2 F, act 3 F, down F + 2 D); merger norm 2, mlp.0 2, mlp.2 1 + OH / (m2 D); the gathers 2 D and 2 OH / m2
        const double mlp = q25 ? 3.0 * D + 6.0 * F : 3.0 * D + (per_block(c) == 8 ? 4.0 : 2.0) * F;
        const double acts = 4.0 * T * (Kp + D + L * (11.0 * D + mlp) + 5.0 * D + OH / m2 + (q25 ? 2.0 * D + 2.0 * OH / m2 : 0.0));
        if (flops) *flops = 2.0 * macs + af;
        if (bytes) *bytes = vis->weight_bytes + acts + ab;
        if (n_kernels) *n_kernels = 1 + per_block(c) * c.layers + 3 + (q25 ? 2 : 0);
    });
}

oar_status oar_qvis_encode(oar_qvis* vis, const oar_qvis_request* req) {
    return guard([&] {
        OAR_CHECK(vis && req, OAR_INVALID_INPUT, "oar_qvis_encode: null argument");
        const oar_qvis_cfg& c = vis->cfg;
        const CallPlan p = plan_call(c, req->n_images, req->grids);
        OAR_CHECK(req->pixel_values && req->embeds, OAR_INVALID_INPUT, "oar_qvis_encode: null pixel_values or embeds");
        const bool q25 = c.kind == OAR_QVIS_QWEN2_5;
        const int T = p.T, D = c.embed, F = c.intermediate, Kp = c.channels * c.temporal_patch * c.patch * c.patch, m2 = c.merge * c.merge, OH = c.out_hidden, dh = D / c.heads, U = T / m2;
        std::vector<float> cs, sn;
        qvis::rotary_tables(req->n_images, req->grids, c.merge, dh, vis->inv_freq, q25 ? p.plan.window_index.data() : nullptr, &cs, &sn);
        OAR_CHECK((int)p.img.segs.size() <= vis->max_segs && (int)p.win.segs.size() <= vis->max_segs && (int)p.img.tiles.size() <= vis->max_tiles &&
                      (int)p.win.tiles.size() <= vis->max_tiles && cs.size() == (size_t)T * (dh / 2), OAR_INTERNAL, "oar_qvis_encode: a table is larger than its buffer");

        std::lock_guard<std::mutex> lk(vis->mu);
        OAR_HIP(hipSetDevice(vis->device));
        hipStream_t s = vis->stream;
        OAR_HIP(hipMemcpyAsync(vis->pix, req->pixel_values, (size_t)T * Kp * 4, hipMemcpyHostToDevice, s));
        OAR_HIP(hipMemcpyAsync(vis->cos, cs.data(), cs.size() * 4, hipMemcpyHostToDevice, s));
        OAR_HIP(hipMemcpyAsync(vis->sin, sn.data(), sn.size() * 4, hipMemcpyHostToDevice, s));
        vis->img.put(p.img, s);
        if (q25) {
            vis->win.put(p.win, s);
            OAR_HIP(hipMemcpyAsync(vis->widx, p.plan.window_index.data(), (size_t)U * 4, hipMemcpyHostToDevice, s));
            OAR_HIP(hipMemcpyAsync(vis->ridx, p.plan.reverse_index.data(), (size_t)U * 4, hipMemcpyHostToDevice, s));
        }
        OAR_HIP(hipStreamSynchronize(s));   // (pageable sources that end with this call)
        const int act = c.act == OAR_QVIS_QUICK_GELU ? k::QVIS_QUICK_GELU : c.act == OAR_QVIS_SILU ? k::QVIS_SILU : k::QVIS_GELU_ERF;
        const int fc1_act = per_block(c) == 8 ? k::ACT_NONE : (c.act == OAR_QVIS_SILU ? k::ACT_SWISH : k::ACT_GELU_ERF);
        auto norm = [&](const float* in, const float* g, const float* b, float* out) {
            if (q25) k::qvis_rmsnorm(s, in, g, out, T, D, 1e-6f, "qvis_norm");
            else k::layernorm(s, in, g, b, out, T, D, 1e-6f, "qvis_norm");
        };
        float *x = vis->x, *x2 = vis->x2;
        if (q25) {   // the patch Linear in the caller's order, then the merge units into window order
            run_linear(s, vis->patch, vis->pix, x2, T, k::ACT_NONE, nullptr, "qvis_linear");
            k::qvis_row_gather(s, x2, vis->widx, x, U, U, m2 * D, "qvis_gather");
        } else {
            run_linear(s, vis->patch, vis->pix, x, T, k::ACT_NONE, nullptr, "qvis_linear");
        }
        k::VisAttnP ap{};
        ap.qkv = vis->qkv; ap.cos = vis->cos; ap.sin = vis->sin; ap.o = vis->att;
        ap.nh = c.heads; ap.dh = dh; ap.ld = 3 * D; ap.scale = (float)std::pow((double)dh, -0.5);
        for (const BlockW& W : vis->blocks) {
            const AttnTables& at = W.full ? vis->img : vis->win;
            ap.segs = at.segs; ap.tiles = at.tiles; ap.n_tiles = at.n_tiles;
            norm(x, W.n1g, W.n1b, vis->xn);
            run_linear(s, W.qkv, vis->xn, vis->qkv, T, k::ACT_NONE, nullptr, "qvis_linear");
            k::vis_attention(s, ap, at.bytes, at.flops);
            run_linear(s, W.proj, vis->att, x2, T, k::ACT_NONE, x, "qvis_linear");
            norm(x2, W.n2g, W.n2b, vis->xn);
            if (q25) {
                run_linear(s, W.up, vis->xn, vis->h, T, k::ACT_NONE, nullptr, "qvis_linear");
                k::qvis_act(s, vis->h, vis->hg, T, F, act, 1, "qvis_act");
                run_linear(s, W.down, vis->hg, x, T, k::ACT_NONE, x2, "qvis_linear");
            } else {
                run_linear(s, W.up, vis->xn, vis->h, T, fc1_act, nullptr, "qvis_linear");
                if (fc1_act == k::ACT_NONE) k::qvis_act(s, vis->h, vis->h, T, F, act, 0, "qvis_act");
                run_linear(s, W.down, vis->h, x, T, k::ACT_NONE, x2, "qvis_linear");
            }
        }
        // the merger: the units are contiguous in either order, so merge^2 rows of D are one row of merge^2 D as they lie
        norm(x, vis->lng, vis->lnb, vis->xn);
        run_linear(s, vis->m0, vis->xn, vis->ph, U, k::ACT_GELU_ERF, nullptr, "qvis_linear");
        run_linear(s, vis->m2, vis->ph, vis->emb, U, k::ACT_NONE, nullptr, "qvis_linear");
        const float* emb = vis->emb;
        if (q25) { k::qvis_row_gather(s, vis->emb, vis->ridx, vis->emb2, U, U, OH, "qvis_gather"); emb = vis->emb2; }
        OAR_HIP(hipGetLastError());
        OAR_HIP(hipMemcpyAsync(req->embeds, emb, (size_t)U * OH * 4, hipMemcpyDeviceToHost, s));
        std::vector<float> fw;
        if (req->features) {
            if (q25) { fw.resize((size_t)T * D); OAR_HIP(hipMemcpyAsync(fw.data(), x, (size_t)T * D * 4, hipMemcpyDeviceToHost, s)); }
            else OAR_HIP(hipMemcpyAsync(req->features, x, (size_t)T * D * 4, hipMemcpyDeviceToHost, s));
        }
        OAR_HIP(hipStreamSynchronize(s));
        if (req->features && q25)   // a debugging output: the units go back to the caller's order on the host, no launch
            for (int slot = 0; slot < U; ++slot)
                std::memcpy(req->features + (size_t)p.plan.window_index[(size_t)slot] * m2 * D, fw.data() + (size_t)slot * m2 * D, (size_t)m2 * D * 4);
        if (Profiler::get().enabled) Profiler::get().flush();
    });
}

// ------------------------------------------------------------------------------------------------ qvis_misc.hip on host arrays
oar_status oar_k_qvis_rmsnorm(const float* x, const float* g, int64_t rows, int32_t d, float eps, float* o_io, size_t o_floats, size_t o_off) {
    return guard([&] {
        OAR_CHECK(x && g && o_io, OAR_INVALID_INPUT, "oar_k_qvis_rmsnorm: null buffer");
        OAR_CHECK(rows >= 1 && rows < (1 << 24) && d >= 4 && d % 4 == 0 && d < (1 << 20) && eps >= 0.0f, OAR_INVALID_INPUT, "oar_k_qvis_rmsnorm: rows outside 1..2^24, d no multiple of 4 or negative eps");
        OAR_CHECK((o_off & 3) == 0 && view_fits(o_off, (uint64_t)rows * d, o_floats), OAR_INVALID_INPUT, "oar_k_qvis_rmsnorm: o_off is no multiple of 4 floats or the output does not fit o_floats");
        require_device();
        DirectCall dc;
        const float *dx = dc.in(x, (size_t)rows * d * 4), *dg = dc.in(g, (size_t)d * 4);
        k::qvis_rmsnorm(nullptr, dx, dg, dc.io(o_io, o_floats) + o_off, rows, d, eps);
        dc.finish();
    });
}

oar_status oar_k_qvis_act(const float* in, size_t in_floats, int64_t rows, int32_t f, int32_t act, int32_t gated, float* o_io, size_t o_floats, size_t o_off) {
    return guard([&] {
        OAR_CHECK(in && o_io, OAR_INVALID_INPUT, "oar_k_qvis_act: null buffer");
        OAR_CHECK(rows >= 1 && rows < (1 << 24) && f >= 4 && f % 4 == 0 && f < (1 << 20), OAR_INVALID_INPUT, "oar_k_qvis_act: rows outside 1..2^24 or f no multiple of 4");
        OAR_CHECK(k::qvis_act_known(act), OAR_UNSUPPORTED_OP, "oar_k_qvis_act: unknown activation");
        const uint64_t width = (uint64_t)f * (gated ? 2 : 1);
        OAR_CHECK(view_fits(0, (uint64_t)rows * width, in_floats), OAR_INVALID_INPUT, "oar_k_qvis_act: in_floats is below rows x f (x 2 when gated)");
        OAR_CHECK((o_off & 3) == 0 && view_fits(o_off, (uint64_t)rows * f, o_floats), OAR_INVALID_INPUT, "oar_k_qvis_act: o_off is no multiple of 4 floats or the output does not fit o_floats");
        require_device();
        DevMem din, dout;
        din.upload(in, in_floats * 4); dout.upload(o_io, o_floats * 4);
        float* o = static_cast<float*>(dout.p) + o_off;
        if (gated) k::qvis_act(nullptr, static_cast<const float*>(din.p), o, rows, f, act, 1);
        else {   // in place, as the chain runs it
            OAR_HIP(hipMemcpy(o, din.p, (size_t)rows * f * 4, hipMemcpyDeviceToDevice));
            k::qvis_act(nullptr, o, o, rows, f, act, 0);
        }
        OAR_HIP(hipGetLastError());
        OAR_HIP(hipMemcpy(o_io, dout.p, o_floats * 4, hipMemcpyDeviceToHost));
    });
}

oar_status oar_k_qvis_row_gather(const float* in, int64_t n_in_rows, int32_t row_floats, const int32_t* idx, int64_t n_rows, float* o_io, size_t o_floats, size_t o_off) {
    return guard([&] {
        OAR_CHECK(in && idx && o_io, OAR_INVALID_INPUT, "oar_k_qvis_row_gather: null buffer");
        OAR_CHECK(n_rows >= 1 && n_rows < (1 << 24) && n_in_rows >= 1 && n_in_rows < (1 << 24) && row_floats >= 4 && row_floats % 4 == 0 && row_floats < (1 << 20), OAR_INVALID_INPUT,
                  "oar_k_qvis_row_gather: row counts outside 1..2^24 or row_floats no multiple of 4");
        for (int64_t r = 0; r < n_rows; ++r) OAR_CHECK(idx[r] >= 0 && idx[r] < n_in_rows, OAR_INVALID_INPUT, "oar_k_qvis_row_gather: an index outside the input rows");
        OAR_CHECK((o_off & 3) == 0 && view_fits(o_off, (uint64_t)n_rows * row_floats, o_floats), OAR_INVALID_INPUT, "oar_k_qvis_row_gather: o_off is no multiple of 4 floats or the output does not fit o_floats");
        require_device();
        DirectCall dc;
        const float* din = dc.in(in, (size_t)n_in_rows * row_floats * 4);
        const int32_t* didx = dc.in(idx, (size_t)n_rows * 4);
        k::qvis_row_gather(nullptr, din, didx, dc.io(o_io, o_floats) + o_off, n_rows, n_in_rows, row_floats);
        dc.finish();
    });
}
