// vis_host.cc -- host side of the PaddleOCR-VL vision encoder and projector: checks a checkpoint's tensor table, stacks q / k / v, packs the
// matrices in the implicit-GEMM kernel's fragment order, uploads them, and drives one call as a fixed chain of launches over the packed patches of all its
// images.  C ABI: oar_vis_create / oar_vis_encode / oar_vis_cost / oar_vis_destroy.  The Linears are k::conv_igemm as 1x1 layers (bias, GELU and residual in
// the epilogue), the LayerNorms k::layernorm, the attention k::vis_attention (vis_attention.hip), the rest vis_misc.hip.  The entry guard, the device check,
// the tensor table and the allocations come from host_entry.h; the stream a tower owns and its attention tables from vis_common.h.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "vis_common.h"

using namespace oar;
using namespace oar::vishost;

namespace {

void check_cfg(const oar_vis_cfg& c) {
    OAR_CHECK(c.hidden > 0 && c.layers > 0 && c.heads > 0 && c.intermediate > 0 && c.patch > 0 && c.channels > 0 && c.pos_grid > 0 && c.merge > 0 && c.text_hidden > 0,
              OAR_INVALID_INPUT, "oar_vis_create: hidden, layers, heads, intermediate, patch, channels, pos_grid, merge and text_hidden must be positive");
    OAR_CHECK(c.hidden < (1 << 20) && c.intermediate < (1 << 20) && c.text_hidden < (1 << 20) && c.patch <= 64 && c.channels <= 16 && c.pos_grid <= 1024 && c.merge <= 8 &&
                  c.layers <= 1024, OAR_INVALID_INPUT, "oar_vis_create: a dimension out of range");
    OAR_CHECK(c.hidden % c.heads == 0, OAR_INVALID_INPUT, "oar_vis_create: hidden is no multiple of heads");
    OAR_CHECK((c.channels * c.patch * c.patch) % 4 == 0 && c.hidden % 4 == 0 && c.intermediate % 4 == 0, OAR_INVALID_INPUT,
              "oar_vis_create: channels patch^2, hidden and intermediate must be multiples of 4 (rows are read 16 bytes at a time)");
    OAR_CHECK(c.ln_eps > 0.0f && c.rope_theta > 0.0f, OAR_INVALID_INPUT, "oar_vis_create: ln_eps and rope_theta must be positive");
    OAR_CHECK(c.act == OAR_VIS_GELU_TANH || c.act == OAR_VIS_GELU_ERF, OAR_INVALID_INPUT, "oar_vis_create: act is neither the tanh nor the erf GELU");
    OAR_CHECK(c.max_images >= 1 && c.max_images <= k::kVisMaxImages, OAR_INVALID_INPUT, "oar_vis_create: max_images must be in 1..16");
    OAR_CHECK(c.max_tokens >= c.merge * c.merge && c.max_tokens <= (1 << 22), OAR_INVALID_INPUT, "oar_vis_create: max_tokens must be in merge^2..2^22");
    OAR_CHECK(k::vis_attention_supported(c.heads, c.hidden / c.heads), OAR_UNSUPPORTED_OP, "oar_vis_create: the head size must be a multiple of 8 in 8..80");
}

struct LayerW { const float *ln1g, *ln1b, *ln2g, *ln2b; Lin qkv, out, fc1, fc2; };
struct LayerT { const oar_lm_tensor *ln1g, *ln1b, *ln2g, *ln2b, *qw, *qb, *kw, *kb, *vw, *vb, *ow, *ob, *f1w, *f1b, *f2w, *f2b; };

// grids [n][2] -> the image table; every check of a request's composition
k::VisGrids check_grids(const oar_vis_cfg& c, int32_t n, const int32_t* grids, const char* who) {
    OAR_CHECK(n >= 1 && n <= c.max_images, OAR_INVALID_INPUT, std::string(who) + ": n_images outside 1..max_images");
    OAR_CHECK(grids != nullptr, OAR_INVALID_INPUT, std::string(who) + ": null grids");
    k::VisGrids g{};
    g.n = n;
    int64_t total = 0;
    for (int i = 0; i < n; ++i) {
        const int64_t h = grids[2 * i], w = grids[2 * i + 1];
        OAR_CHECK(h >= 1 && w >= 1 && h <= (1 << 15) && w <= (1 << 15), OAR_INVALID_INPUT, std::string(who) + ": a grid side outside 1..32768");
        OAR_CHECK(h % c.merge == 0 && w % c.merge == 0, OAR_INVALID_INPUT, std::string(who) + ": a grid side is no multiple of merge");
        g.start[i] = (int)total; g.h[i] = (int)h; g.w[i] = (int)w;
        total += h * w;
        OAR_CHECK(total <= c.max_tokens, OAR_INVALID_INPUT, std::string(who) + ": the images hold more patches than max_tokens");
    }
    g.start[n] = (int)total;
    return g;
}

// the attention tables of a call: one segment per image
HostTables grid_tables(const k::VisGrids& g, int heads, int dh) {
    std::vector<int32_t> lens((size_t)g.n);
    for (int i = 0; i < g.n; ++i) lens[(size_t)i] = g.h[i] * g.w[i];
    HostTables t;
    t.build(lens, heads, dh);
    return t;
}

}  // namespace

struct oar_vis : VisDevice {
    oar_vis_cfg cfg{};
    std::vector<LayerW> layers;
    Lin patch, p1, p2;
    const float *pos_table = nullptr, *postg = nullptr, *postb = nullptr, *preg = nullptr, *preb = nullptr;
    // per-call buffers, sized for max_tokens at create
    float *pix = nullptr, *pos = nullptr, *x = nullptr, *x2 = nullptr, *xn = nullptr, *qkv = nullptr, *att = nullptr, *h = nullptr, *merged = nullptr, *ph = nullptr, *emb = nullptr;
    float *cos = nullptr, *sin = nullptr;
    AttnTables att_tab;
    int max_tiles = 0;
    std::vector<float> inv_freq;   // [dh / 4], f32
};

oar_status oar_vis_create(const oar_vis_cfg* cfg, const oar_lm_tensor* tensors, int32_t n_tensors, int32_t device_id, oar_vis** out) {
    return guard([&] {
        OAR_CHECK(cfg && out && (tensors || n_tensors == 0) && n_tensors >= 0, OAR_INVALID_INPUT, "oar_vis_create: null argument");
        *out = nullptr;
        const oar_vis_cfg c = *cfg;
        check_cfg(c);
        const Table T("oar_vis_create", tensors, n_tensors);
        const int D = c.hidden, L = c.layers, F = c.intermediate, Kp = c.channels * c.patch * c.patch, G = c.pos_grid, m2 = c.merge * c.merge, TH = c.text_hidden, dh = D / c.heads;
        // every tensor is looked up and checked before the device is touched
        const std::string vm = "visual.vision_model.";
        auto it = T.by_name.find(vm + "embeddings.patch_embedding.weight");
        OAR_CHECK(it != T.by_name.end(), OAR_INVALID_INPUT, "oar_vis_create: tensor '" + vm + "embeddings.patch_embedding.weight' is missing");
        const oar_lm_tensor& pw = *it->second;
        OAR_CHECK(pw.data && (pw.dtype == OAR_LM_F32 || pw.dtype == OAR_LM_BF16), OAR_INVALID_INPUT, "oar_vis_create: the patch embedding has no data or is neither f32 nor bf16");
        OAR_CHECK((pw.rank == 4 && pw.dims[0] == D && pw.dims[1] == c.channels && pw.dims[2] == c.patch && pw.dims[3] == c.patch) || (pw.rank == 2 && pw.dims[0] == D && pw.dims[1] == Kp),
                  OAR_INVALID_INPUT, "oar_vis_create: tensor '" + vm + "embeddings.patch_embedding.weight' has the wrong shape");
        const oar_lm_tensor& pb = T.need(vm + "embeddings.patch_embedding.bias", D, -1);
        const oar_lm_tensor& pe = T.need(vm + "embeddings.position_embedding.weight", (int64_t)G * G, D);
        std::vector<LayerT> lt((size_t)L);
        for (int l = 0; l < L; ++l) {
            const std::string pre = vm + "encoder.layers." + std::to_string(l) + ".";
            LayerT& t = lt[(size_t)l];
            t.ln1g = &T.need(pre + "layer_norm1.weight", D, -1); t.ln1b = &T.need(pre + "layer_norm1.bias", D, -1);
            t.ln2g = &T.need(pre + "layer_norm2.weight", D, -1); t.ln2b = &T.need(pre + "layer_norm2.bias", D, -1);
            t.qw = &T.need(pre + "self_attn.q_proj.weight", D, D); t.qb = &T.need(pre + "self_attn.q_proj.bias", D, -1);
            t.kw = &T.need(pre + "self_attn.k_proj.weight", D, D); t.kb = &T.need(pre + "self_attn.k_proj.bias", D, -1);
            t.vw = &T.need(pre + "self_attn.v_proj.weight", D, D); t.vb = &T.need(pre + "self_attn.v_proj.bias", D, -1);
            t.ow = &T.need(pre + "self_attn.out_proj.weight", D, D); t.ob = &T.need(pre + "self_attn.out_proj.bias", D, -1);
            t.f1w = &T.need(pre + "mlp.fc1.weight", F, D); t.f1b = &T.need(pre + "mlp.fc1.bias", F, -1);
            t.f2w = &T.need(pre + "mlp.fc2.weight", D, F); t.f2b = &T.need(pre + "mlp.fc2.bias", D, -1);
        }
        const oar_lm_tensor& postg = T.need(vm + "post_layernorm.weight", D, -1);
        const oar_lm_tensor& postb = T.need(vm + "post_layernorm.bias", D, -1);
        const oar_lm_tensor& preg = T.need("mlp_AR.pre_norm.weight", D, -1);
        const oar_lm_tensor& preb = T.need("mlp_AR.pre_norm.bias", D, -1);
        const oar_lm_tensor& l1w = T.need("mlp_AR.linear_1.weight", (int64_t)m2 * D, (int64_t)m2 * D);
        const oar_lm_tensor& l1b = T.need("mlp_AR.linear_1.bias", (int64_t)m2 * D, -1);
        const oar_lm_tensor& l2w = T.need("mlp_AR.linear_2.weight", TH, (int64_t)m2 * D);
        const oar_lm_tensor& l2b = T.need("mlp_AR.linear_2.bias", TH, -1);

        open_device(device_id, "oar_vis_create: no such device");
        std::unique_ptr<oar_vis> M(new oar_vis());
        M->cfg = c; M->device = device_id;
        OAR_HIP(hipStreamCreateWithFlags(&M->stream, hipStreamNonBlocking));
        const long MTl = c.max_tokens, MPl = c.max_tokens / m2;
        M->patch = M->linear(widen(pw, (size_t)D * Kp), widen(pb, (size_t)D), D, Kp, MTl);
        M->pos_table = M->up(widen(pe, (size_t)G * G * D));
        M->layers.resize((size_t)L);
        for (int l = 0; l < L; ++l) {
            const LayerT& t = lt[(size_t)l];
            LayerW& W = M->layers[(size_t)l];
            W.ln1g = M->up(widen(*t.ln1g, (size_t)D)); W.ln1b = M->up(widen(*t.ln1b, (size_t)D));
            W.ln2g = M->up(widen(*t.ln2g, (size_t)D)); W.ln2b = M->up(widen(*t.ln2b, (size_t)D));
            std::vector<float> w = widen(*t.qw, (size_t)D * D), b = widen(*t.qb, (size_t)D);   // [Wq; Wk; Wv]: one Linear gives the fused projection
            for (const oar_lm_tensor* mtx : {t.kw, t.vw}) { const std::vector<float> a = widen(*mtx, (size_t)D * D); w.insert(w.end(), a.begin(), a.end()); }
            for (const oar_lm_tensor* vec : {t.kb, t.vb}) { const std::vector<float> a = widen(*vec, (size_t)D); b.insert(b.end(), a.begin(), a.end()); }
            W.qkv = M->linear(w, b, 3 * D, D, MTl);
            W.out = M->linear(widen(*t.ow, (size_t)D * D), widen(*t.ob, (size_t)D), D, D, MTl);
            W.fc1 = M->linear(widen(*t.f1w, (size_t)F * D), widen(*t.f1b, (size_t)F), F, D, MTl);
            W.fc2 = M->linear(widen(*t.f2w, (size_t)D * F), widen(*t.f2b, (size_t)D), D, F, MTl);
        }
        M->postg = M->up(widen(postg, (size_t)D)); M->postb = M->up(widen(postb, (size_t)D));
        M->preg = M->up(widen(preg, (size_t)D)); M->preb = M->up(widen(preb, (size_t)D));
        M->p1 = M->linear(widen(l1w, (size_t)m2 * D * m2 * D), widen(l1b, (size_t)m2 * D), m2 * D, m2 * D, MPl);
        M->p2 = M->linear(widen(l2w, (size_t)TH * m2 * D), widen(l2b, (size_t)TH), TH, m2 * D, MPl);
        const size_t MT = (size_t)c.max_tokens;
        M->pix = M->raw<float>(MT * Kp); M->pos = M->raw<float>(MT * D); M->x = M->raw<float>(MT * D); M->x2 = M->raw<float>(MT * D); M->xn = M->raw<float>(MT * D);
        M->qkv = M->raw<float>(MT * 3 * D); M->att = M->raw<float>(MT * D); M->h = M->raw<float>(MT * F);
        M->merged = M->raw<float>(MT * D); M->ph = M->raw<float>(MT * D); M->emb = M->raw<float>((MT / m2 + 1) * TH);
        M->cos = M->raw<float>(MT * (dh / 2)); M->sin = M->raw<float>(MT * (dh / 2));
        M->max_tiles = c.heads * (int)((MT + k::kFlashQueries - 1) / k::kFlashQueries + c.max_images);
        M->att_tab.alloc(*M, k::kVisMaxImages, M->max_tiles);
        M->inv_freq.resize((size_t)dh / 4);
        for (int j = 0; j < dh / 4; ++j) M->inv_freq[(size_t)j] = (float)(1.0 / std::pow((double)c.rope_theta, 2.0 * j / (dh / 2)));
        *out = M.release();
    });
}

void oar_vis_destroy(oar_vis* vis) {
    if (!vis) return;
    (void)hipSetDevice(vis->device);
    delete vis;
}

oar_status oar_vis_cost(const oar_vis* vis, int32_t n_images, const int32_t* grids_hw, double* flops, double* bytes, int32_t* n_kernels) {
    return guard([&] {
        OAR_CHECK(vis, OAR_INVALID_INPUT, "oar_vis_cost: null model");
        const oar_vis_cfg& c = vis->cfg;
        const k::VisGrids g = check_grids(c, n_images, grids_hw, "oar_vis_cost");
        const double T = g.start[g.n], D = c.hidden, F = c.intermediate, Kp = (double)c.channels * c.patch * c.patch, m2 = (double)c.merge * c.merge, TH = c.text_hidden, L = c.layers;
        const HostTables ht = grid_tables(g, c.heads, c.hidden / c.heads);
        const double ab = ht.bytes, af = ht.flops;
        const double macs = T * (Kp * D + L * (4.0 * D * D + 2.0 * D * F)) + (T / m2) * (m2 * D * m2 * D + m2 * D * TH);
        // rows read and written per launch: embedding (pix, pos twice, x), per layer (LN 2, qkv 4, out 3, LN 2, fc1 1 + F/D, the tanh GELU 2 F/D, fc2 F/D + 2), post LN 2, projector (LN 2, gather 2, l1 2, l2 1 + TH/(m2 D))
        const double acts = 4.0 * T * (Kp + 3.0 * D + L * (14.0 * D + (c.act == OAR_VIS_GELU_ERF ? 2.0 : 4.0) * F) + 2.0 * D + 6.0 * D + D + TH / m2);
        if (flops) *flops = 2.0 * macs + L * af;
        if (bytes) *bytes = vis->weight_bytes + acts + L * ab;
        if (n_kernels) *n_kernels = (c.act == OAR_VIS_GELU_ERF ? 7 : 8) * c.layers + 7;
    });
}

oar_status oar_vis_encode(oar_vis* vis, const oar_vis_request* req) {
    return guard([&] {
        OAR_CHECK(vis && req, OAR_INVALID_INPUT, "oar_vis_encode: null argument");
        const oar_vis_cfg& c = vis->cfg;
        const k::VisGrids g = check_grids(c, req->n_images, req->grids, "oar_vis_encode");
        OAR_CHECK(req->pixel_values && req->embeds, OAR_INVALID_INPUT, "oar_vis_encode: null pixel_values or embeds");
        const int T = g.start[g.n], D = c.hidden, F = c.intermediate, Kp = c.channels * c.patch * c.patch, m2 = c.merge * c.merge, TH = c.text_hidden, dh = D / c.heads, h2 = dh / 2, q4 = dh / 4;
        // rotary tables on the host, in f32 like the reference: position x frequency, then cosf / sinf
        std::vector<float> cs((size_t)T * h2), sn((size_t)T * h2);
        for (int i = 0; i < g.n; ++i) {
            for (int idx = 0; idx < g.h[i] * g.w[i]; ++idx) {
                const float row = (float)(idx / g.w[i]), col = (float)(idx % g.w[i]);
                float* cr = cs.data() + (size_t)(g.start[i] + idx) * h2;
                float* sr = sn.data() + (size_t)(g.start[i] + idx) * h2;
                for (int j = 0; j < q4; ++j) {
                    const float ar = row * vis->inv_freq[(size_t)j], ac = col * vis->inv_freq[(size_t)j];
                    cr[j] = std::cos(ar); sr[j] = std::sin(ar); cr[q4 + j] = std::cos(ac); sr[q4 + j] = std::sin(ac);
                }
            }
        }
        const HostTables ht = grid_tables(g, c.heads, dh);
        OAR_CHECK((int)ht.tiles.size() <= vis->max_tiles, OAR_INTERNAL, "oar_vis_encode: more query tiles than the table holds");

        std::lock_guard<std::mutex> lk(vis->mu);
        OAR_HIP(hipSetDevice(vis->device));
        hipStream_t s = vis->stream;
        OAR_HIP(hipMemcpyAsync(vis->pix, req->pixel_values, (size_t)T * Kp * 4, hipMemcpyHostToDevice, s));
        OAR_HIP(hipMemcpyAsync(vis->cos, cs.data(), cs.size() * 4, hipMemcpyHostToDevice, s));
        OAR_HIP(hipMemcpyAsync(vis->sin, sn.data(), sn.size() * 4, hipMemcpyHostToDevice, s));
        AttnTables& at = vis->att_tab;
        at.put(ht, s);
        OAR_HIP(hipStreamSynchronize(s));   // (pageable sources that end with this call)
        const int act = c.act == OAR_VIS_GELU_ERF ? k::ACT_GELU_ERF : k::ACT_GELU_TANH;
        // embedding: the resampled position table is the residual of the patch Linear
        k::vis_pos_embed(s, vis->pos_table, vis->pos, g, c.pos_grid, D);
        run_linear(s, vis->patch, vis->pix, vis->x, T, k::ACT_NONE, vis->pos);
        k::VisAttnP ap{};
        ap.qkv = vis->qkv; ap.cos = vis->cos; ap.sin = vis->sin; ap.o = vis->att; ap.segs = at.segs; ap.tiles = at.tiles;
        ap.n_tiles = at.n_tiles; ap.nh = c.heads; ap.dh = dh; ap.ld = 3 * D; ap.scale = (float)std::pow((double)dh, -0.5);
        for (const LayerW& W : vis->layers) {
            k::layernorm(s, vis->x, W.ln1g, W.ln1b, vis->xn, T, D, c.ln_eps, "vis_layernorm");
            run_linear(s, W.qkv, vis->xn, vis->qkv, T, k::ACT_NONE, nullptr);
            k::vis_attention(s, ap, at.bytes, at.flops);
            run_linear(s, W.out, vis->att, vis->x2, T, k::ACT_NONE, vis->x);
            k::layernorm(s, vis->x2, W.ln2g, W.ln2b, vis->xn, T, D, c.ln_eps, "vis_layernorm");
            // (the implicit-GEMM epilogue has the erf GELU but not the tanh form, which only the element-wise kernel knows: one more launch per layer)
            run_linear(s, W.fc1, vis->xn, vis->h, T, act == k::ACT_GELU_ERF ? act : k::ACT_NONE, nullptr);
            if (act != k::ACT_GELU_ERF) { k::Act a; a.kind = act; k::unary(s, vis->h, vis->h, (int64_t)T * F, a, "vis_linear"); }
            run_linear(s, W.fc2, vis->h, vis->x, T, k::ACT_NONE, vis->x2);
        }
        k::layernorm(s, vis->x, vis->postg, vis->postb, vis->x2, T, D, c.ln_eps, "vis_layernorm");                 // x2: the features
        // projector: LayerNorm as its own launch (the kernel every other LayerNorm here uses), then one gather -- the merge is pure data movement
        k::layernorm(s, vis->x2, vis->preg, vis->preb, vis->xn, T, D, 1e-5f, "vis_layernorm");
        k::vis_merge_gather(s, vis->xn, vis->merged, g, c.merge, D);
        run_linear(s, vis->p1, vis->merged, vis->ph, T / m2, k::ACT_GELU_ERF, nullptr);
        run_linear(s, vis->p2, vis->ph, vis->emb, T / m2, k::ACT_NONE, nullptr);
        OAR_HIP(hipGetLastError());
        OAR_HIP(hipMemcpyAsync(req->embeds, vis->emb, (size_t)(T / m2) * TH * 4, hipMemcpyDeviceToHost, s));
        if (req->features) OAR_HIP(hipMemcpyAsync(req->features, vis->x2, (size_t)T * D * 4, hipMemcpyDeviceToHost, s));
        OAR_HIP(hipStreamSynchronize(s));
        if (Profiler::get().enabled) Profiler::get().flush();
    });
}
