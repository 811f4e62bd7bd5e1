// lm_host.cc -- host side of the decoder-only language model (lm_decode.hip): checks a checkpoint's tensor table, stacks / permutes / pads the matrices,
// uploads them, and drives prefill and decode as one schedule of <= 16-row steps.  C ABI: oar_lm_create / oar_lm_generate / oar_lm_cost / oar_lm_destroy.
// Opt-in (oar_lm_set_prefill): the prompt positions before each prompt's last run as token-major GEMMs and one causal flash-attention launch per layer
// (lm_prefill_gemm.hip, lm_prefill_attn.hip) into the same cache, then the chain above takes over with the last positions.
// Opt-in (oar_lm_set_decode): the steps' attention cut over the keys (lm_decode_split.hip), and a call that stops enqueuing steps once a copy of
// the device's `alive` word, looked at a fixed number of steps behind the enqueue, says that every sequence has ended.
// The entry guard, the device check, the tensor table, the allocations and the direct entries' device copies come from host_entry.h.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "host_entry.h"
#include "lm_decode.h"
#include "lm_logits.h"
#include "lm_prefill.h"
#include "lm_queue.h"

using namespace oar;

namespace {

void check_cfg(const oar_lm_cfg& c) {
    OAR_CHECK(c.hidden > 0 && c.layers > 0 && c.heads > 0 && c.kv_heads > 0 && c.head_dim > 0 && c.intermediate > 0 && c.vocab >= 2, OAR_INVALID_INPUT,
              "oar_lm_create: hidden, layers, heads, kv_heads, head_dim, intermediate must be positive and vocab >= 2");
    OAR_CHECK(c.heads % c.kv_heads == 0, OAR_INVALID_INPUT, "oar_lm_create: heads is no multiple of kv_heads");
    OAR_CHECK(k::lm_head_dim_supported(c.head_dim), OAR_UNSUPPORTED_OP, "oar_lm_create: head_dim must be a multiple of 4 in 8..128");
    OAR_CHECK(c.hidden % 4 == 0 && c.intermediate % 4 == 0, OAR_UNSUPPORTED_OP, "oar_lm_create: hidden and intermediate must be multiples of 4 (rows are read 16 bytes at a time)");
    OAR_CHECK(c.mrope_section[0] >= 0 && c.mrope_section[1] >= 0 && c.mrope_section[2] >= 0 &&
                  (int64_t)c.mrope_section[0] + c.mrope_section[1] + c.mrope_section[2] == c.head_dim / 2,
              OAR_INVALID_INPUT, "oar_lm_create: mrope_section must sum to head_dim / 2");
    OAR_CHECK(c.rms_eps > 0.0f && c.rope_theta > 0.0f, OAR_INVALID_INPUT, "oar_lm_create: rms_eps and rope_theta must be positive");
    OAR_CHECK(c.max_sequences >= 1 && c.max_sequences <= k::kLmRows, OAR_INVALID_INPUT, "oar_lm_create: max_sequences must be in 1..16");
    OAR_CHECK(c.max_positions >= 2 && c.max_positions <= (1 << 20), OAR_INVALID_INPUT, "oar_lm_create: max_positions must be in 2..2^20");
    OAR_CHECK((int64_t)c.heads * c.head_dim < (1 << 24) && c.hidden < (1 << 24) && c.intermediate < (1 << 24) && c.vocab < (1 << 24), OAR_INVALID_INPUT,
              "oar_lm_create: a dimension of 2^24 or more");
}

// Copies row `src_row` of t ([rows][K]) to row `dst_row` of a [.][Kp] matrix of t's own element size (the padding stays zero).
void put_row(std::vector<uint8_t>& dst, size_t dst_row, const oar_lm_tensor& t, size_t src_row, int K, int Kp) {
    const size_t es = t.dtype == OAR_LM_BF16 ? 2 : 4;
    std::memcpy(dst.data() + dst_row * Kp * es, static_cast<const uint8_t*>(t.data) + src_row * K * es, (size_t)K * es);
}

// Row order that puts the rotary pair (d, d + dh / 2) of every head side by side: new row head dh + 2 i + s holds old row head dh + i + s dh / 2.
size_t rope_src(size_t n, int dh) {
    const size_t head = n / dh, r = n % dh, i = r >> 1, s = r & 1;
    return head * dh + i + s * (dh / 2);
}


// What every generate entry asks of a request, the number of sequences aside (the caller has checked it): returns the prompt rows of the call.
int64_t check_request(const oar_lm_cfg& c, const oar_lm_request& r, const std::string& fn) {
    const int S = r.n_seq, MN = r.max_new_tokens, V = c.vocab;
    OAR_CHECK(MN >= 1, OAR_INVALID_INPUT, fn + ": max_new_tokens must be positive");
    OAR_CHECK(r.lengths && r.tokens && r.counts && (r.inputs_embeds || r.input_ids), OAR_INVALID_INPUT, fn + ": null lengths, outputs or inputs");
    OAR_CHECK(r.eos_token_id >= -1 && r.eos_token_id < V, OAR_INVALID_INPUT, fn + ": eos_token_id outside the vocabulary");
    int64_t total = 0;
    for (int s = 0; s < S; ++s) {
        const int T = r.lengths[s];
        OAR_CHECK(T >= 1 && (int64_t)T + MN <= c.max_positions, OAR_INVALID_INPUT, fn + ": prompt length + max_new_tokens exceeds max_positions (sequence " + std::to_string(s) + ")");
        if (r.inputs_embeds) OAR_CHECK(r.inputs_embeds[s] != nullptr, OAR_INVALID_INPUT, fn + ": null inputs_embeds entry");
        else {
            OAR_CHECK(r.input_ids[s] != nullptr, OAR_INVALID_INPUT, fn + ": null input_ids entry");
            for (int t = 0; t < T; ++t) OAR_CHECK(r.input_ids[s][t] >= 0 && r.input_ids[s][t] < V, OAR_INVALID_INPUT, fn + ": token id outside the vocabulary");
        }
        total += T;
    }
    OAR_CHECK(total < (1 << 24), OAR_INVALID_INPUT, fn + ": prompts too long");
    return total;
}

}  // namespace

struct oar_lm {
    oar_lm_cfg cfg{};
    int device = 0;
    int bf16 = 0;
    hipStream_t stream = nullptr;
    mutable std::mutex mu;
    std::vector<std::unique_ptr<DevMem>> mem;
    std::vector<k::LmLayerW> layers;
    k::LmDecodeP P{};
    DevMem work;     // arena | tokens | forced | logits | steps | ids, sized per call
    size_t work_cap = 0;
    double weight_bytes = 0;
    int prefill_mode = OAR_LM_PREFILL_ROWS;
    int chunk_rows = k::kLmPrefillDefaultChunk;
    int attention = OAR_LM_ATTN_SERIAL;
    int split_keys = k::kLmSplitDefault;
    int stop_at_eos = 0;
    DevMem split_ws;   // the split mode's partials, allocated at its first use
    size_t split_ws_cap = 0;
    DevMem logits_ws;   // the logits processors' step buffer, candidates, histories and presence bitmaps, allocated at their first use
    size_t logits_ws_cap = 0;
    int32_t* stop_ring = nullptr;   // pinned [kLmStopRing]: copies of state.alive
    hipEvent_t stop_ev[k::kLmStopRing] = {};
    int64_t steps_limit = 0, steps_enqueued = 0;   // of the last call
    uint8_t* queue_pin = nullptr;   // pinned rings of queued generation: LmState copies | LmQueueStage tables | GEMM-phase tables
    size_t queue_pin_cap = 0;
    hipEvent_t queue_ev[k::kLmQueueRing] = {};
    k::LmQueueStats queue_stats{};   // of the last queued call
    ~oar_lm() {
        for (hipEvent_t e : queue_ev)
            if (e) (void)hipEventDestroy(e);
        if (queue_pin) (void)hipHostFree(queue_pin);
        for (hipEvent_t e : stop_ev)
            if (e) (void)hipEventDestroy(e);
        if (stop_ring) (void)hipHostFree(stop_ring);
        if (stream) {
            Profiler::get().drop_events();
            (void)hipStreamDestroy(stream);
        }
    }
    void* up(const void* src, size_t bytes) {
        mem.emplace_back(new DevMem());
        mem.back()->upload(src, bytes);
        return mem.back()->p;
    }
    void* raw(size_t bytes) {
        mem.emplace_back(new DevMem());
        mem.back()->alloc(bytes);
        return mem.back()->p;
    }
};

namespace {

// Carves the per-call device memory: take() gives the next 256-byte aligned offset.
struct Carver {
    size_t off = 0;
    size_t take(size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; }
};

// The per-call device memory of a model, grown when a call needs more.
uint8_t* work_bytes(oar_lm* lm, size_t need) {
    if (need > lm->work_cap) {
        if (lm->work.p) { OAR_HIP(hipFree(lm->work.p)); lm->work.p = nullptr; lm->work_cap = 0; }
        lm->work.alloc(need);
        lm->work_cap = need;
    }
    return static_cast<uint8_t*>(lm->work.p);
}

// The chain's parameters for one call: the model's, with the split mode's workspace (allocated at its first use) when the call's attention is split.
k::LmDecodeP call_params(oar_lm* lm, int attention) {
    const oar_lm_cfg& c = lm->cfg;
    k::LmDecodeP P = lm->P;
    P.layers = lm->layers.data();
    P.split_ws = nullptr; P.split_keys = lm->split_keys;
    if (attention == OAR_LM_ATTN_SPLIT) {
        const size_t ws_b = k::lm_split_ws_floats(c.heads, c.head_dim, c.max_positions, lm->split_keys) * 4;
        if (ws_b > lm->split_ws_cap) {
            if (lm->split_ws.p) { OAR_HIP(hipFree(lm->split_ws.p)); lm->split_ws.p = nullptr; lm->split_ws_cap = 0; }
            lm->split_ws.alloc(ws_b);
            lm->split_ws_cap = ws_b;
        }
        P.split_ws = static_cast<float*>(lm->split_ws.p);
    }
    return P;
}

// The prompts of a request into the arena, sequence after sequence from row 0: the embeddings as they are, or the ids through lm_embed.
void upload_prompts(const oar_lm_request& r, const k::LmDecodeP& P, int32_t* d_ids, int32_t* d_xrows, hipStream_t s) {
    const int S = r.n_seq, D = P.D;
    if (r.inputs_embeds) {
        size_t row = 0;
        for (int q = 0; q < S; ++q) {
            OAR_HIP(hipMemcpyAsync(P.arena + row * D, r.inputs_embeds[q], (size_t)r.lengths[q] * D * 4, hipMemcpyHostToDevice, s));
            row += (size_t)r.lengths[q];
        }
    } else {
        std::vector<int32_t> ids, xr;
        for (int q = 0; q < S; ++q)
            for (int t = 0; t < r.lengths[q]; ++t) { xr.push_back((int32_t)ids.size()); ids.push_back(r.input_ids[q][t]); }
        OAR_HIP(hipMemcpyAsync(d_ids, ids.data(), ids.size() * 4, hipMemcpyHostToDevice, s));
        OAR_HIP(hipMemcpyAsync(d_xrows, xr.data(), xr.size() * 4, hipMemcpyHostToDevice, s));
        OAR_HIP(hipStreamSynchronize(s));   // (the two host vectors are pageable and end with this block)
        k::lm_embed(s, P, d_ids, d_xrows, (int)ids.size());
    }
}

// GEMM prefill of packed rows already on the device, chunk after chunk (chunk[ci] rows, tiles tile0[ci] .. tile0[ci + 1]; host_tiles: the same tiles,
// for the cost): per chunk and layer q/k/v GEMM (RMSNorm in front, bias, M-RoPE, k / v into the cache), causal attention, o GEMM + residual, gate / up GEMM
// (RMSNorm in front, silu(g) u), down GEMM + residual; the last layer stops after its q/k/v launch
void gemm_phase(const oar_lm* lm, const k::LmDecodeP& P, hipStream_t s, const k::LmPfRow* d_pfrows, const k::LmPfTile* d_pftiles, const k::LmPfTile* host_tiles,
                const std::vector<int>& pf_chunk, const std::vector<size_t>& pf_tile0, float* pf_q, float* pf_o, float* pf_h) {
    const oar_lm_cfg& c = lm->cfg;
    const int D = c.hidden, Hd = c.heads * c.head_dim, Kd = c.kv_heads * c.head_dim, F = c.intermediate;
    size_t row0 = 0;
    for (size_t ci = 0; ci < pf_chunk.size(); ++ci) {
        const int M = pf_chunk[ci];
        const k::LmPfRow* rows = d_pfrows + row0;
        const k::LmPfTile* tiles = d_pftiles + pf_tile0[ci];
        const int n_tiles = (int)(pf_tile0[ci + 1] - pf_tile0[ci]);
        double abytes = 0.0, aflops = 0.0;
        k::lm_pf_attn_cost(host_tiles + pf_tile0[ci], n_tiles, c.head_dim, &abytes, &aflops);
        for (int l = 0; l < c.layers; ++l) {
            const k::LmLayerW& Lw = lm->layers[(size_t)l];
            float* kc = P.kcache + (size_t)l * P.cache_layer;
            float* vc = P.vcache + (size_t)l * P.cache_layer;
            k::LmGemmP g{};
            g.mode = k::LM_GEMM_QKV; g.bf16 = P.bf16; g.M = M; g.N = Hd + 2 * Kd; g.K = D; g.Kp = k::lm_pad4(D); g.x = P.arena; g.x_ld = D; g.x_gather = 1; g.rows = rows;
            g.w = Lw.w_qkv; g.bias = Lw.b_qkv; g.rms_g = Lw.ln1; g.eps = P.eps; g.q = pf_q; g.q_ld = Hd; g.kc = kc; g.vc = vc; g.nq = Hd; g.nk = Kd; g.dh = c.head_dim;
            g.kvh = c.kv_heads; g.maxpos = P.maxpos; g.sec0 = P.sec0; g.sec1 = P.sec1; g.inv_freq = P.inv_freq;
            k::lm_gemm(s, g);
            if (l == c.layers - 1) break;   // nothing reads these rows' hidden state after the last layer's keys and values
            k::LmPfAttnP a{};
            a.q = pf_q; a.q_ld = Hd; a.kc = kc; a.vc = vc; a.H = c.heads; a.KVH = c.kv_heads; a.dh = c.head_dim; a.maxpos = P.maxpos;
            a.scale = 1.0f / sqrtf((float)c.head_dim); a.o = pf_o; a.o_ld = Hd; a.tiles = tiles; a.n_tiles = n_tiles;
            k::lm_prefill_attention(s, a, abytes, aflops);
            g = k::LmGemmP{};
            g.mode = k::LM_GEMM_RESID; g.bf16 = P.bf16; g.M = M; g.N = D; g.K = Hd; g.Kp = k::lm_pad4(Hd); g.x = pf_o; g.x_ld = Hd; g.rows = rows; g.w = Lw.w_o;
            g.y = P.arena; g.y_ld = D; g.y_scatter = 1;
            k::lm_gemm(s, g);
            g = k::LmGemmP{};
            g.mode = k::LM_GEMM_GATE; g.bf16 = P.bf16; g.M = M; g.N = 2 * F; g.K = D; g.Kp = k::lm_pad4(D); g.x = P.arena; g.x_ld = D; g.x_gather = 1; g.rows = rows;
            g.w = Lw.w_gu; g.rms_g = Lw.ln2; g.eps = P.eps; g.y = pf_h; g.y_ld = F;
            k::lm_gemm(s, g);
            g = k::LmGemmP{};
            g.mode = k::LM_GEMM_RESID; g.bf16 = P.bf16; g.M = M; g.N = D; g.K = F; g.Kp = k::lm_pad4(F); g.x = pf_h; g.x_ld = F; g.rows = rows; g.w = Lw.w_down;
            g.y = P.arena; g.y_ld = D; g.y_scatter = 1;
            k::lm_gemm(s, g);
        }
        row0 += (size_t)M;
    }
}

// Rotary positions of prompt position t of a sequence of length T (pid: its [3][T] position ids, or null); mx gathers the largest.
void prompt_positions(const int32_t* pid, int T, int t, int32_t rp[3], int64_t& mx, const std::string& fn) {
    for (int a = 0; a < 3; ++a) {
        rp[a] = pid ? pid[(size_t)a * T + t] : t;
        OAR_CHECK(rp[a] >= 0 && rp[a] < (1 << 24), OAR_INVALID_INPUT, fn + ": position id outside 0..2^24");
        if (pid) mx = std::max<int64_t>(mx, rp[a]);
    }
}

}  // namespace

oar_status oar_lm_create(const oar_lm_cfg* cfg, const oar_lm_tensor* tensors, int32_t n_tensors, int32_t device_id, oar_lm** out) {
    return guard([&] {
        OAR_CHECK(cfg && out && (tensors || n_tensors == 0) && n_tensors >= 0, OAR_INVALID_INPUT, "oar_lm_create: null argument");
        *out = nullptr;
        const oar_lm_cfg c = *cfg;
        check_cfg(c);
        const Table T("oar_lm_create", tensors, n_tensors);
        const int D = c.hidden, L = c.layers, H = c.heads, KVH = c.kv_heads, dh = c.head_dim, F = c.intermediate, V = c.vocab;
        const int Hd = H * dh, Kd = KVH * dh, Dp = k::lm_pad4(D), Hdp = k::lm_pad4(Hd), Fp = k::lm_pad4(F);
        // every tensor is looked up and checked before the device is touched
        const oar_lm_tensor& emb = T.need("model.embed_tokens.weight", V, D);
        const oar_lm_tensor& lmw = c.tie_embeddings ? emb : T.need("lm_head.weight", V, D);
        const oar_lm_tensor& nf = T.need("model.norm.weight", D, -1);
        const int wdt = emb.dtype;
        struct LayerT { const oar_lm_tensor *ln1, *ln2, *q, *k, *v, *o, *g, *u, *d, *bq, *bk, *bv; };
        std::vector<LayerT> lt((size_t)L);
        for (int l = 0; l < L; ++l) {
            const std::string pre = "model.layers." + std::to_string(l) + ".";
            LayerT& t = lt[(size_t)l];
            t.ln1 = &T.need(pre + "input_layernorm.weight", D, -1);
            t.ln2 = &T.need(pre + "post_attention_layernorm.weight", D, -1);
            t.q = &T.need(pre + "self_attn.q_proj.weight", Hd, D);
            t.k = &T.need(pre + "self_attn.k_proj.weight", Kd, D);
            t.v = &T.need(pre + "self_attn.v_proj.weight", Kd, D);
            t.o = &T.need(pre + "self_attn.o_proj.weight", D, Hd);
            t.g = &T.need(pre + "mlp.gate_proj.weight", F, D);
            t.u = &T.need(pre + "mlp.up_proj.weight", F, D);
            t.d = &T.need(pre + "mlp.down_proj.weight", D, F);
            t.bq = t.bk = t.bv = nullptr;
            if (c.qkv_bias) {
                t.bq = &T.need(pre + "self_attn.q_proj.bias", Hd, -1);
                t.bk = &T.need(pre + "self_attn.k_proj.bias", Kd, -1);
                t.bv = &T.need(pre + "self_attn.v_proj.bias", Kd, -1);
            }
            for (const oar_lm_tensor* m : {t.q, t.k, t.v, t.o, t.g, t.u, t.d})
                OAR_CHECK(m->dtype == wdt, OAR_INVALID_INPUT, "oar_lm_create: the weight matrices do not share one dtype (layer " + std::to_string(l) + ")");
        }
        OAR_CHECK(lmw.dtype == wdt, OAR_INVALID_INPUT, "oar_lm_create: lm_head.weight and embed_tokens do not share one dtype");

        open_device(device_id, "oar_lm_create: no such device");
        std::unique_ptr<oar_lm> M(new oar_lm());
        M->cfg = c; M->device = device_id; M->bf16 = wdt == OAR_LM_BF16;
        OAR_HIP(hipStreamCreateWithFlags(&M->stream, hipStreamNonBlocking));
        const size_t es = M->bf16 ? 2 : 4;
        M->layers.resize((size_t)L);
        for (int l = 0; l < L; ++l) {
            const LayerT& t = lt[(size_t)l];
            k::LmLayerW& W = M->layers[(size_t)l];
            const int Nqkv = Hd + 2 * Kd;
            std::vector<uint8_t> m((size_t)Nqkv * Dp * es, 0);
            for (int n = 0; n < Hd; ++n) put_row(m, (size_t)n, *t.q, rope_src((size_t)n, dh), D, Dp);
            for (int n = 0; n < Kd; ++n) put_row(m, (size_t)Hd + n, *t.k, rope_src((size_t)n, dh), D, Dp);
            for (int n = 0; n < Kd; ++n) put_row(m, (size_t)Hd + Kd + n, *t.v, (size_t)n, D, Dp);
            W.w_qkv = M->up(m.data(), m.size());
            W.b_qkv = nullptr;
            if (c.qkv_bias) {
                const std::vector<float> bq = widen(*t.bq, (size_t)Hd), bk = widen(*t.bk, (size_t)Kd), bv = widen(*t.bv, (size_t)Kd);
                std::vector<float> b((size_t)Nqkv);
                for (int n = 0; n < Hd; ++n) b[(size_t)n] = bq[rope_src((size_t)n, dh)];
                for (int n = 0; n < Kd; ++n) b[(size_t)Hd + n] = bk[rope_src((size_t)n, dh)];
                for (int n = 0; n < Kd; ++n) b[(size_t)Hd + Kd + n] = bv[(size_t)n];
                W.b_qkv = static_cast<const float*>(M->up(b.data(), b.size() * 4));
            }
            m.assign((size_t)D * Hdp * es, 0);
            for (int n = 0; n < D; ++n) put_row(m, (size_t)n, *t.o, (size_t)n, Hd, Hdp);
            W.w_o = M->up(m.data(), m.size());
            m.assign((size_t)2 * F * Dp * es, 0);
            for (int n = 0; n < F; ++n) { put_row(m, (size_t)2 * n, *t.g, (size_t)n, D, Dp); put_row(m, (size_t)2 * n + 1, *t.u, (size_t)n, D, Dp); }
            W.w_gu = M->up(m.data(), m.size());
            m.assign((size_t)D * Fp * es, 0);
            for (int n = 0; n < D; ++n) put_row(m, (size_t)n, *t.d, (size_t)n, F, Fp);
            W.w_down = M->up(m.data(), m.size());
            const std::vector<float> g1 = widen(*t.ln1, (size_t)D), g2 = widen(*t.ln2, (size_t)D);
            W.ln1 = static_cast<const float*>(M->up(g1.data(), g1.size() * 4));
            W.ln2 = static_cast<const float*>(M->up(g2.data(), g2.size() * 4));
            M->weight_bytes += (double)es * ((double)Nqkv * Dp + (double)D * Hdp + 2.0 * F * Dp + (double)D * Fp) + 4.0 * (2.0 * D + (c.qkv_bias ? Nqkv : 0));
        }
        k::LmDecodeP& P = M->P;
        {
            std::vector<uint8_t> m((size_t)V * Dp * es, 0);
            for (int n = 0; n < V; ++n) put_row(m, (size_t)n, emb, (size_t)n, D, Dp);
            P.embed = M->up(m.data(), m.size());
            P.w_lm = P.embed;
            if (!c.tie_embeddings) {
                m.assign((size_t)V * Dp * es, 0);
                for (int n = 0; n < V; ++n) put_row(m, (size_t)n, lmw, (size_t)n, D, Dp);
                P.w_lm = M->up(m.data(), m.size());
            }
            M->weight_bytes += (double)es * V * Dp + 4.0 * D;
            const std::vector<float> g = widen(nf, (size_t)D);
            P.lnf = static_cast<const float*>(M->up(g.data(), g.size() * 4));
            std::vector<float> inv((size_t)dh / 2);
            for (int i = 0; i < dh / 2; ++i) inv[(size_t)i] = (float)std::pow((double)c.rope_theta, -2.0 * i / dh);
            P.inv_freq = static_cast<const float*>(M->up(inv.data(), inv.size() * 4));
        }
        P.D = D; P.L = L; P.H = H; P.KVH = KVH; P.dh = dh; P.F = F; P.V = V; P.maxpos = c.max_positions; P.sec0 = c.mrope_section[0]; P.sec1 = c.mrope_section[1];
        P.bf16 = M->bf16; P.eps = c.rms_eps; P.layers = M->layers.data();
        P.cache_layer = (size_t)c.max_sequences * KVH * c.max_positions * dh;
        P.kcache = static_cast<float*>(M->raw(P.cache_layer * L * 4));
        P.vcache = static_cast<float*>(M->raw(P.cache_layer * L * 4));
        P.q = static_cast<float*>(M->raw((size_t)k::kLmRows * Hd * 4));
        P.o = static_cast<float*>(M->raw((size_t)k::kLmRows * Hd * 4));
        P.h = static_cast<float*>(M->raw((size_t)k::kLmRows * F * 4));
        P.part = M->raw((size_t)k::kLmRows * k::lm_head_workgroups(V) * 8);
        P.state = static_cast<k::LmState*>(M->raw(sizeof(k::LmState)));
        *out = M.release();
    });
}

void oar_lm_destroy(oar_lm* lm) {
    if (!lm) return;
    (void)hipSetDevice(lm->device);
    delete lm;
}

oar_status oar_lm_cost(const oar_lm* lm, int32_t n_rows, int32_t cache_len, double* flops, double* bytes, int32_t* n_kernels) {
    return guard([&] {
        OAR_CHECK(lm && n_rows >= 1 && n_rows <= k::kLmRows && cache_len >= 0 && cache_len <= lm->cfg.max_positions, OAR_INVALID_INPUT,
                  "oar_lm_cost: null model, n_rows outside 1..16 or cache_len outside the cache");
        const oar_lm_cfg& c = lm->cfg;
        const double D = c.hidden, Hd = (double)c.heads * c.head_dim, Kd = (double)c.kv_heads * c.head_dim, F = c.intermediate, V = c.vocab, L = c.layers, B = n_rows, n = cache_len;
        const double macs = L * (D * (Hd + 2 * Kd) + Hd * D + 3.0 * F * D + 2.0 * n * Hd) + V * D;
        const double acts = 4.0 * B * (L * (2 * D + 2 * (Hd + 2 * Kd) + 2 * Hd + 3 * D + 2 * F + 2 * D) + D + 2.0 * k::lm_head_workgroups(c.vocab) + D);
        int attention, split_keys;
        { std::lock_guard<std::mutex> lk(lm->mu); attention = lm->attention; split_keys = lm->split_keys; }
        const bool split = attention == OAR_LM_ATTN_SPLIT;
        // split mode: every span's partial (m, l, acc[dh]) per row and head is written by lm_attn_split and read by lm_attn_merge
        const double parts = split ? 2.0 * 4.0 * B * L * c.heads * (double)std::max(1, k::lm_split_spans(cache_len, split_keys)) * (c.head_dim + 2) : 0.0;
        if (flops) *flops = 2.0 * macs * B;
        if (bytes) *bytes = lm->weight_bytes + 4.0 * B * L * 2.0 * n * Kd + acts + parts;
        if (n_kernels) *n_kernels = split ? k::lm_launches_per_step_split(c.layers) : k::lm_launches_per_step(c.layers);
    });
}

namespace {

// The logits processors of a call: what oar_lm_logits_cfg asks for, checked; hist[i] / hlen[i] the prompt part of sequence i's history.
struct LogitsPlan {
    bool on = false;
    float r = 1.0f;
    int n = 0;
    std::vector<const int32_t*> hist;
    std::vector<int32_t> hlen;
};

void check_processors(float r, int n, int V, const std::string& fn) {
    OAR_CHECK(std::isfinite(r) && r >= 1.0f, OAR_INVALID_INPUT, fn + ": repetition_penalty must be finite and >= 1");
    OAR_CHECK(n >= 0, OAR_INVALID_INPUT, fn + ": no_repeat_ngram_size must be >= 0");
    OAR_CHECK(n <= 1 || V <= k::kLmSelectMaxVocab, OAR_UNSUPPORTED_OP, fn + ": no_repeat_ngram_size with a vocabulary above 2^19");
}

void check_history(const int32_t* ids, int64_t len, const std::string& fn) {
    OAR_CHECK(len >= 0 && len <= k::kLmHistoryMax, OAR_INVALID_INPUT, fn + ": history length outside 0..65536");
    OAR_CHECK(ids != nullptr || len == 0, OAR_INVALID_INPUT, fn + ": null history_ids entry");
    for (int64_t t = 0; t < len; ++t) OAR_CHECK(ids[t] >= 0, OAR_INVALID_INPUT, fn + ": negative history id");
}

LogitsPlan logits_plan(const oar_lm_cfg& c, const oar_lm_request& r, const oar_lm_logits_cfg* lp, const std::string& fn) {
    LogitsPlan g;
    if (!lp) return g;
    check_processors(lp->repetition_penalty, lp->no_repeat_ngram_size, c.vocab, fn);
    g.r = lp->repetition_penalty; g.n = lp->no_repeat_ngram_size;
    g.on = g.r != 1.0f || g.n > 1;
    if (!g.on) return g;
    OAR_CHECK((lp->history_ids == nullptr) == (lp->history_lengths == nullptr), OAR_INVALID_INPUT, fn + ": history_ids and history_lengths go together");
    OAR_CHECK(lp->history_ids || !r.inputs_embeds, OAR_INVALID_INPUT, fn + ": inputs_embeds with a logits processor need history_ids");
    for (int s = 0; s < r.n_seq; ++s) {
        const int32_t* ids = lp->history_ids ? lp->history_ids[s] : r.input_ids[s];
        const int64_t len = lp->history_ids ? lp->history_lengths[s] : r.lengths[s];
        check_history(ids, len, fn);
        g.hist.push_back(ids); g.hlen.push_back((int32_t)len);
    }
    return g;
}

// Host tables of histories: hist [rows][cap] and seen [rows][words] from the first hlen[i] ids of ids[i].
void history_tables(const std::vector<const int32_t*>& ids, const std::vector<int32_t>& hlen, int V, int cap, std::vector<int32_t>& hist, std::vector<uint32_t>& seen) {
    const size_t rows = ids.size(), words = (size_t)k::lm_select_words(V);
    hist.assign(rows * (size_t)cap, 0);
    seen.assign(rows * words, 0u);
    for (size_t q = 0; q < rows; ++q)
        for (int32_t t = 0; t < hlen[q]; ++t) {
            const int32_t id = ids[q][t];
            hist[q * (size_t)cap + (size_t)t] = id;
            if (id < V) seen[q * words + (size_t)(id >> 5)] |= 1u << (id & 31);
        }
}

// The processors' workspace (grown when a call needs more) and the call's prompt histories into it, enqueued on s from the two host vectors (the caller
// synchronises before they go): P gets the select branch's pointers.
void logits_tables(oar_lm* lm, const LogitsPlan& g, int S, int MN, k::LmDecodeP& P, std::vector<int32_t>& hist, std::vector<uint32_t>& seen, hipStream_t s) {
    const int V = lm->cfg.vocab, words = k::lm_select_words(V);
    const int cap = *std::max_element(g.hlen.begin(), g.hlen.end()) + MN;
    Carver cv;
    const size_t step_o = cv.take((size_t)k::kLmRows * k::lm_select_ld(V) * 4), part_o = cv.take((size_t)k::kLmRows * 8), hlen_o = cv.take((size_t)k::kLmRows * 4);
    const size_t seen_o = cv.take((size_t)k::kLmRows * words * 4), hist_o = cv.take((size_t)k::kLmRows * cap * 4);
    if (cv.off > lm->logits_ws_cap) {
        if (lm->logits_ws.p) { OAR_HIP(hipFree(lm->logits_ws.p)); lm->logits_ws.p = nullptr; lm->logits_ws_cap = 0; }
        lm->logits_ws.alloc(cv.off);
        lm->logits_ws_cap = cv.off;
    }
    uint8_t* w = static_cast<uint8_t*>(lm->logits_ws.p);
    history_tables(g.hist, g.hlen, V, cap, hist, seen);
    OAR_HIP(hipMemcpyAsync(w + hlen_o, g.hlen.data(), (size_t)S * 4, hipMemcpyHostToDevice, s));
    OAR_HIP(hipMemcpyAsync(w + seen_o, seen.data(), seen.size() * 4, hipMemcpyHostToDevice, s));
    OAR_HIP(hipMemcpyAsync(w + hist_o, hist.data(), hist.size() * 4, hipMemcpyHostToDevice, s));
    P.select = 1; P.step_logits = reinterpret_cast<float*>(w + step_o); P.part1 = w + part_o; P.hlen = reinterpret_cast<const int32_t*>(w + hlen_o);
    P.seen = reinterpret_cast<uint32_t*>(w + seen_o); P.hist = reinterpret_cast<int32_t*>(w + hist_o); P.hist_cap = cap; P.penalty = g.r; P.ngram = g.n;
}

// oar_lm_generate (lp null) and oar_lm_generate_ex: one schedule; a processor that is on adds its tables and lm_step's select branch, nothing else
void generate_impl(oar_lm* lm, const oar_lm_request* req, const oar_lm_logits_cfg* lp, const std::string& fn) {
    {
        OAR_CHECK(lm && req, OAR_INVALID_INPUT, fn + ": null argument");
        const oar_lm_cfg& c = lm->cfg;
        const int S = req->n_seq, MN = req->max_new_tokens, D = c.hidden, V = c.vocab;
        OAR_CHECK(S >= 1 && S <= c.max_sequences, OAR_INVALID_INPUT, fn + ": n_seq outside 1..max_sequences");
        const int64_t total = check_request(c, *req, fn);
        const LogitsPlan lg = logits_plan(c, *req, lp, fn);
        std::lock_guard<std::mutex> lk(lm->mu);
        const bool gemm = lm->prefill_mode == OAR_LM_PREFILL_GEMM;
        const int attention = lm->attention;
        const bool stop = lm->stop_at_eos && req->eos_token_id >= 0;
        // the schedule: prompt rows of all sequences in order, 16 to a step; then one step per generated token.  GEMM prefill: the prompt rows before each
        // prompt's last go to the GEMM phase's row table instead, and the first step holds the last rows alone.
        std::vector<k::LmStep> steps;
        std::vector<int> step_maxpos;
        std::vector<int32_t> next_pos((size_t)S);
        std::vector<k::LmPfRow> pf_rows;
        {
            k::LmStep cur{};
            int mp = 0, xrow = 0;
            for (int s = 0; s < S; ++s) {
                const int T = req->lengths[s];
                const int32_t* pid = req->position_ids ? req->position_ids[s] : nullptr;
                int64_t mx = pid ? INT64_MIN : T - 1;
                for (int t = 0; t < T; ++t) {
                    k::LmRow& R = cur.rows[cur.nrows];
                    R.seq = s; R.pos = t; R.xrow = xrow++; R.gen = t == T - 1 ? 0 : -1; R.pad = 0;
                    prompt_positions(pid, T, t, R.rp, mx, fn);
                    if (gemm && R.gen < 0) {   // (the slot is filled again by the next row)
                        pf_rows.push_back(k::LmPfRow{R.seq, R.pos, {R.rp[0], R.rp[1], R.rp[2]}, R.xrow, {0, 0}});
                        continue;
                    }
                    if (R.gen >= 0) cur.head[cur.nhead++] = cur.nrows;
                    mp = std::max(mp, t);
                    if (++cur.nrows == k::kLmRows) { steps.push_back(cur); step_maxpos.push_back(mp); cur = k::LmStep{}; mp = 0; }
                }
                OAR_CHECK(mx + MN < (1 << 24), OAR_INVALID_INPUT, fn + ": position id outside 0..2^24");
                next_pos[(size_t)s] = (int32_t)(mx + 1);
            }
            if (cur.nrows) { steps.push_back(cur); step_maxpos.push_back(mp); }
        }
        const int xdec0 = (int)total;
        for (int g = 1; g < MN; ++g) {   // the step that consumes token g - 1 and produces token g
            k::LmStep st{};
            int mp = 0;
            for (int s = 0; s < S; ++s) {
                k::LmRow& R = st.rows[st.nrows];
                R.seq = s; R.pos = req->lengths[s] + g - 1; R.xrow = xdec0 + s; R.gen = g; R.pad = 0;
                R.rp[0] = R.rp[1] = R.rp[2] = next_pos[(size_t)s] + g - 1;
                st.head[st.nhead++] = st.nrows++;
                mp = std::max(mp, R.pos);
            }
            steps.push_back(st); step_maxpos.push_back(mp);
        }

        // the GEMM phase: chunks of the packed rows, and every chunk's attention tiles (row_lo counts from the chunk's first row)
        std::vector<k::LmPfSpan> pf_spans;
        std::vector<int> pf_first, pf_chunk;
        std::vector<k::LmPfTile> pf_tiles;
        std::vector<size_t> pf_tile0;
        int pf_cap = 0;
        if (!pf_rows.empty()) {
            k::lm_pf_chunks(req->lengths, S, lm->chunk_rows, pf_spans, pf_first, pf_chunk);
            for (size_t ci = 0; ci < pf_chunk.size(); ++ci) {
                pf_tile0.push_back(pf_tiles.size());
                k::lm_pf_tiles(pf_spans.data() + pf_first[ci], pf_first[ci + 1] - pf_first[ci], c.heads, pf_tiles);
                pf_cap = std::max(pf_cap, pf_chunk[ci]);
            }
            pf_tile0.push_back(pf_tiles.size());
            OAR_CHECK(pf_tiles.size() < ((size_t)1 << 31), OAR_INVALID_INPUT, fn + ": prompts too long");
        }
        const size_t Hd_ = (size_t)c.heads * c.head_dim;

        OAR_HIP(hipSetDevice(lm->device));
        hipStream_t s = lm->stream;
        // per-call device memory: arena | tokens | forced | steps | ids + xrows | logits | GEMM prefill: rows | tiles | q | o | h
        Carver cv;
        const size_t arena_o = cv.take(((size_t)total + S) * D * 4), tok_o = cv.take((size_t)S * MN * 4), forced_o = cv.take((size_t)S * MN * 4);
        const size_t steps_o = cv.take(steps.size() * sizeof(k::LmStep)), ids_o = cv.take((size_t)total * 4), xrows_o = cv.take((size_t)total * 4);
        const size_t logits_o = cv.take(req->logits ? (size_t)S * MN * V * 4 : 0);
        const size_t pfr_o = cv.take(pf_rows.size() * sizeof(k::LmPfRow)), pft_o = cv.take(pf_tiles.size() * sizeof(k::LmPfTile));
        const size_t pfq_o = cv.take((size_t)pf_cap * Hd_ * 4), pfo_o = cv.take((size_t)pf_cap * Hd_ * 4), pfh_o = cv.take((size_t)pf_cap * c.intermediate * 4);
        uint8_t* w = work_bytes(lm, cv.off);
        k::LmDecodeP P = call_params(lm, attention);
        std::vector<int32_t> lg_hist;
        std::vector<uint32_t> lg_seen;
        if (lg.on) logits_tables(lm, lg, S, MN, P, lg_hist, lg_seen, s);
        if (stop && !lm->stop_ring) {
            OAR_HIP(hipHostMalloc(reinterpret_cast<void**>(&lm->stop_ring), sizeof(int32_t) * k::kLmStopRing, hipHostMallocDefault));
            for (hipEvent_t& e : lm->stop_ev) OAR_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        }
        P.arena = reinterpret_cast<float*>(w + arena_o); P.xdec0 = xdec0;
        P.tokens = reinterpret_cast<int32_t*>(w + tok_o);
        int32_t* d_forced = reinterpret_cast<int32_t*>(w + forced_o);
        k::LmStep* d_steps = reinterpret_cast<k::LmStep*>(w + steps_o);
        int32_t* d_ids = reinterpret_cast<int32_t*>(w + ids_o);
        int32_t* d_xrows = reinterpret_cast<int32_t*>(w + xrows_o);
        P.logits = req->logits ? reinterpret_cast<float*>(w + logits_o) : nullptr;
        P.forced = req->forced_tokens ? d_forced : nullptr;
        P.max_new = MN; P.eos = req->eos_token_id;
        OAR_HIP(hipMemsetAsync(P.tokens, 0, (size_t)S * MN * 4, s));
        if (P.logits) OAR_HIP(hipMemsetAsync(P.logits, 0, (size_t)S * MN * V * 4, s));
        if (req->forced_tokens) OAR_HIP(hipMemcpyAsync(d_forced, req->forced_tokens, (size_t)S * MN * 4, hipMemcpyHostToDevice, s));
        OAR_HIP(hipMemcpyAsync(d_steps, steps.data(), steps.size() * sizeof(k::LmStep), hipMemcpyHostToDevice, s));
        k::LmState st0{};
        st0.alive = S;
        OAR_HIP(hipMemcpyAsync(P.state, &st0, sizeof st0, hipMemcpyHostToDevice, s));
        upload_prompts(*req, P, d_ids, d_xrows, s);
        k::LmPfRow* d_pfrows = reinterpret_cast<k::LmPfRow*>(w + pfr_o);
        k::LmPfTile* d_pftiles = reinterpret_cast<k::LmPfTile*>(w + pft_o);
        float* pf_q = reinterpret_cast<float*>(w + pfq_o);
        float* pf_o = reinterpret_cast<float*>(w + pfo_o);
        float* pf_h = reinterpret_cast<float*>(w + pfh_o);
        if (!pf_rows.empty()) {
            OAR_HIP(hipMemcpyAsync(d_pfrows, pf_rows.data(), pf_rows.size() * sizeof(k::LmPfRow), hipMemcpyHostToDevice, s));
            OAR_HIP(hipMemcpyAsync(d_pftiles, pf_tiles.data(), pf_tiles.size() * sizeof(k::LmPfTile), hipMemcpyHostToDevice, s));
        }
        OAR_HIP(hipStreamSynchronize(s));       // (pageable sources: steps, st0, the GEMM phase's tables)
        gemm_phase(lm, P, s, d_pfrows, d_pftiles, pf_tiles.data(), pf_chunk, pf_tile0, pf_q, pf_o, pf_h);
        // stop at eos: copy c is taken behind step (c + 1) kLmStopStride - 1; before step i the host waits for the newest copy taken at a step
        // <= i - kLmStopLookahead -- the device still holds the steps after it -- and enqueues nothing more once that copy of `alive` is 0
        size_t enqueued = 0;
        int64_t seen = -1;   // the newest copy the host has looked at
        for (size_t i = 0; i < steps.size(); ++i) {
            if (stop) {
                const int64_t c = ((int64_t)i - k::kLmStopLookahead + 1) / k::kLmStopStride - 1;   // the newest copy whose step (c + 1) stride - 1 <= i - lookahead
                if ((int64_t)i >= k::kLmStopLookahead && c >= 0 && c > seen) {
                    OAR_HIP(hipEventSynchronize(lm->stop_ev[c % k::kLmStopRing]));
                    seen = c;
                }
                if (seen >= 0 && *static_cast<volatile int32_t*>(lm->stop_ring + seen % k::kLmStopRing) == 0) break;
            }
            k::lm_step(s, P, d_steps + i, steps[i].nrows, steps[i].nhead, step_maxpos[i], attention);
            enqueued = i + 1;
            if (stop && (i + 1) % k::kLmStopStride == 0) {
                const size_t slot = ((i + 1) / k::kLmStopStride - 1) % k::kLmStopRing;
                OAR_HIP(hipMemcpyAsync(lm->stop_ring + slot, &P.state->alive, 4, hipMemcpyDeviceToHost, s));
                OAR_HIP(hipEventRecord(lm->stop_ev[slot], s));
            }
        }
        lm->steps_limit = (int64_t)steps.size();
        lm->steps_enqueued = (int64_t)enqueued;
        OAR_HIP(hipGetLastError());
        OAR_HIP(hipMemcpyAsync(req->tokens, P.tokens, (size_t)S * MN * 4, hipMemcpyDeviceToHost, s));
        if (P.logits) OAR_HIP(hipMemcpyAsync(req->logits, P.logits, (size_t)S * MN * V * 4, hipMemcpyDeviceToHost, s));
        OAR_HIP(hipStreamSynchronize(s));
        if (Profiler::get().enabled) Profiler::get().flush();
        if (enqueued < steps.size()) {   // the steps never enqueued would have written eos: every sequence had ended
            const size_t first_decode = steps.size() - (size_t)(MN - 1);   // step first_decode + g - 1 gives token g >= 1
            for (int g = 1; g < MN; ++g)
                if (first_decode + (size_t)g - 1 >= enqueued)
                    for (int q = 0; q < S; ++q) req->tokens[(size_t)q * MN + g] = req->eos_token_id;
        }
        for (int q = 0; q < S; ++q) {
            int n = MN;
            if (req->eos_token_id >= 0)
                for (int g = 0; g < MN; ++g)
                    if (req->tokens[(size_t)q * MN + g] == req->eos_token_id) { n = g + 1; break; }
            req->counts[q] = n;
        }
    }
}

}  // namespace

oar_status oar_lm_generate(oar_lm* lm, const oar_lm_request* req) {
    return guard([&] { generate_impl(lm, req, nullptr, "oar_lm_generate"); });
}

oar_status oar_lm_generate_ex(oar_lm* lm, const oar_lm_request* req, const oar_lm_logits_cfg* lp) {
    return guard([&] { generate_impl(lm, req, lp, "oar_lm_generate_ex"); });
}

namespace {

void queue_check(const oar_lm_cfg* cfg, const oar_lm_request* req, int32_t slots) {
    OAR_CHECK(cfg && req, OAR_INVALID_INPUT, "oar_lm_generate_queue: null argument");
    OAR_CHECK(cfg->max_sequences >= 1 && cfg->max_sequences <= k::kLmRows && cfg->vocab >= 2 && cfg->max_positions >= 2, OAR_INVALID_INPUT,
              "oar_lm_generate_queue: max_sequences outside 1..16, vocab or max_positions below 2");
    OAR_CHECK(req->n_seq >= 1 && req->n_seq <= k::kLmQueueMaxSeq, OAR_INVALID_INPUT, "oar_lm_generate_queue: n_seq outside 1..65535");
    OAR_CHECK(slots >= 0 && slots <= cfg->max_sequences, OAR_INVALID_INPUT, "oar_lm_generate_queue: slots outside 0..max_sequences");
    check_request(*cfg, *req, "oar_lm_generate_queue");
}

}  // namespace

// What oar_lm_generate_queue asks of its arguments; needs no model and no device.
oar_status oar_lm_queue_check(const oar_lm_cfg* cfg, const oar_lm_request* req, int32_t slots) {
    return guard([&] { queue_check(cfg, req, slots); });
}

oar_status oar_lm_generate_queue(oar_lm* lm, const oar_lm_request* req, int32_t slots_arg) {
    return guard([&] {
        static const std::string fn = "oar_lm_generate_queue";
        OAR_CHECK(lm && req, OAR_INVALID_INPUT, fn + ": null argument");
        const oar_lm_cfg& c = lm->cfg;
        queue_check(&c, req, slots_arg);
        const int S = req->n_seq, MN = req->max_new_tokens, D = c.hidden, V = c.vocab, slots = slots_arg == 0 ? c.max_sequences : slots_arg;
        // every sequence's arena rows and positions
        std::vector<k::LmQueueSeq> seqs((size_t)S);
        int64_t total = 0;
        for (int q = 0; q < S; ++q) {
            const int T = req->lengths[q];
            const int32_t* pid = req->position_ids ? req->position_ids[q] : nullptr;
            int64_t mx = pid ? INT64_MIN : T - 1;
            int32_t rp[3];
            for (int t = 0; t < T; ++t) prompt_positions(pid, T, t, rp, mx, fn);
            OAR_CHECK(mx + MN < (1 << 24), OAR_INVALID_INPUT, fn + ": position id outside 0..2^24");
            seqs[(size_t)q] = k::LmQueueSeq{T, (int32_t)total, (int32_t)(mx + 1), pid};
            total += T;
        }
        std::lock_guard<std::mutex> lk(lm->mu);
        const bool gemm = lm->prefill_mode == OAR_LM_PREFILL_GEMM;
        const int attention = lm->attention;
        const int xdec0 = (int)total;
        size_t pf_rows_cap = 0, pf_tiles_cap = 0;
        if (gemm) k::lm_queue_phase_caps(req->lengths, S, slots, lm->chunk_rows, c.heads, &pf_rows_cap, &pf_tiles_cap);
        const size_t pf_cap = std::min<size_t>(pf_rows_cap, (size_t)lm->chunk_rows), Hd = (size_t)c.heads * c.head_dim;

        OAR_HIP(hipSetDevice(lm->device));
        hipStream_t s = lm->stream;
        // per-call device memory: arena | the slots' tokens, forced tokens, logits | every sequence's tokens, forced tokens, logits | stage | ids + xrows |
        // GEMM phase: rows | tiles | q | o | h
        const bool forced = req->forced_tokens != nullptr, logits = req->logits != nullptr;
        Carver cv;
        const size_t arena_o = cv.take(((size_t)total + slots) * D * 4), stok_o = cv.take((size_t)slots * MN * 4), sforced_o = cv.take(forced ? (size_t)slots * MN * 4 : 0);
        const size_t slogits_o = cv.take(logits ? (size_t)slots * MN * V * 4 : 0), otok_o = cv.take((size_t)S * MN * 4), oforced_o = cv.take(forced ? (size_t)S * MN * 4 : 0);
        const size_t ologits_o = cv.take(logits ? (size_t)S * MN * V * 4 : 0), stage_o = cv.take(sizeof(k::LmQueueStage));
        const size_t ids_o = cv.take((size_t)total * 4), xrows_o = cv.take((size_t)total * 4);
        const size_t pfr_o = cv.take(pf_rows_cap * sizeof(k::LmPfRow)), pft_o = cv.take(pf_tiles_cap * sizeof(k::LmPfTile));
        const size_t pfq_o = cv.take(pf_cap * Hd * 4), pfo_o = cv.take(pf_cap * Hd * 4), pfh_o = cv.take(pf_cap * c.intermediate * 4);
        uint8_t* w = work_bytes(lm, cv.off);
        k::LmDecodeP P = call_params(lm, attention);
        // pinned rings, entry i mod kLmQueueRing for step i: LmState copies | stages | GEMM-phase rows | tiles
        Carver pin;
        const size_t pstate_o = pin.take(sizeof(k::LmState) * k::kLmQueueRing), pstage_o = pin.take(sizeof(k::LmQueueStage) * k::kLmQueueRing);
        const size_t prow_b = (pf_rows_cap * sizeof(k::LmPfRow) + 255) & ~(size_t)255, ptile_b = (pf_tiles_cap * sizeof(k::LmPfTile) + 255) & ~(size_t)255;
        const size_t prow_o = pin.take(prow_b * k::kLmQueueRing), ptile_o = pin.take(ptile_b * k::kLmQueueRing);
        if (pin.off > lm->queue_pin_cap) {
            if (lm->queue_pin) { OAR_HIP(hipHostFree(lm->queue_pin)); lm->queue_pin = nullptr; lm->queue_pin_cap = 0; }
            OAR_HIP(hipHostMalloc(reinterpret_cast<void**>(&lm->queue_pin), pin.off, hipHostMallocDefault));
            lm->queue_pin_cap = pin.off;
        }
        for (hipEvent_t& e : lm->queue_ev)
            if (!e) OAR_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        k::LmState* pin_state = reinterpret_cast<k::LmState*>(lm->queue_pin + pstate_o);
        k::LmQueueStage* pin_stage = reinterpret_cast<k::LmQueueStage*>(lm->queue_pin + pstage_o);

        P.arena = reinterpret_cast<float*>(w + arena_o); P.xdec0 = xdec0;
        P.tokens = reinterpret_cast<int32_t*>(w + stok_o);
        P.forced = forced ? reinterpret_cast<int32_t*>(w + sforced_o) : nullptr;
        P.logits = logits ? reinterpret_cast<float*>(w + slogits_o) : nullptr;
        P.max_new = MN; P.eos = req->eos_token_id;
        k::LmQueueStage* d_stage = reinterpret_cast<k::LmQueueStage*>(w + stage_o);
        k::LmPfRow* d_pfrows = reinterpret_cast<k::LmPfRow*>(w + pfr_o);
        k::LmPfTile* d_pftiles = reinterpret_cast<k::LmPfTile*>(w + pft_o);
        k::LmQueueTurnP tp{};
        tp.turn = d_stage->turn; tp.slot_tokens = P.tokens; tp.out_tokens = reinterpret_cast<int32_t*>(w + otok_o);
        tp.slot_forced = forced ? reinterpret_cast<int32_t*>(w + sforced_o) : nullptr; tp.all_forced = forced ? reinterpret_cast<const int32_t*>(w + oforced_o) : nullptr;
        tp.slot_logits = P.logits; tp.out_logits = logits ? reinterpret_cast<float*>(w + ologits_o) : nullptr;
        tp.state = P.state; tp.max_new = MN; tp.V = V; tp.eos = req->eos_token_id;
        // everything the steps read is on the device before the first step: prompts, forced tokens, zeroed slot rows.  `alive` starts at n_seq: the chain's
        // alive == 0 guard cannot fire while sequences wait
        OAR_HIP(hipMemsetAsync(P.tokens, 0, (size_t)slots * MN * 4, s));
        OAR_HIP(hipMemsetAsync(tp.out_tokens, 0, (size_t)S * MN * 4, s));
        if (logits) OAR_HIP(hipMemsetAsync(P.logits, 0, (size_t)slots * MN * V * 4, s));
        if (forced) {
            OAR_HIP(hipMemsetAsync(tp.slot_forced, 0xFF, (size_t)slots * MN * 4, s));
            OAR_HIP(hipMemcpyAsync(w + oforced_o, req->forced_tokens, (size_t)S * MN * 4, hipMemcpyHostToDevice, s));
        }
        k::LmState st0{};
        st0.alive = S;
        OAR_HIP(hipMemcpyAsync(P.state, &st0, sizeof st0, hipMemcpyHostToDevice, s));
        upload_prompts(*req, P, reinterpret_cast<int32_t*>(w + ids_o), reinterpret_cast<int32_t*>(w + xrows_o), s);
        OAR_HIP(hipStreamSynchronize(s));       // (pageable sources: forced tokens, st0, the prompts)

        // the step loop: nothing blocks the host but the lagged event (lm_queue.h)
        k::LmQueue Q(seqs.data(), S, slots, MN, gemm, xdec0);
        std::vector<k::LmQueueAdmit> admits;
        k::LmQueuePhase ph;
        k::LmState seen_state{};
        int64_t seen = -1, gemm_phases = 0;
        for (;;) {
            const int64_t i = Q.step();
            const size_t e = (size_t)(i % k::kLmQueueRing);
            const int64_t cpy = k::lm_queue_copy_for(i);
            if (cpy > seen) {
                OAR_HIP(hipEventSynchronize(lm->queue_ev[cpy % k::kLmQueueRing]));
                seen_state = pin_state[cpy % k::kLmQueueRing];
                seen = cpy;
            }
            k::LmQueueStage& st = pin_stage[e];
            int n_turn = 0, max_pos = 0;
            const bool more = Q.next(seen >= 0 ? seen_state.done : nullptr, seen >= 0 ? k::lm_queue_copy_step(seen) : -1, st, n_turn, max_pos, admits);
            if (!more && n_turn == 0) break;
            OAR_HIP(hipMemcpyAsync(d_stage, &st, sizeof st, hipMemcpyHostToDevice, s));
            if (n_turn) { tp.n_turn = n_turn; k::lm_queue_turnover(s, tp); }
            if (!more) break;
            if (!admits.empty()) {   // one packed GEMM phase for everything admitted at this point
                k::LmPfRow* prow = reinterpret_cast<k::LmPfRow*>(lm->queue_pin + prow_o + e * prow_b);
                k::LmPfTile* ptile = reinterpret_cast<k::LmPfTile*>(lm->queue_pin + ptile_o + e * ptile_b);
                OAR_CHECK(k::lm_queue_pack(seqs.data(), admits.data(), (int)admits.size(), lm->chunk_rows, c.heads, prow, pf_rows_cap, ptile, pf_tiles_cap, ph), OAR_INTERNAL,
                          fn + ": a GEMM phase outgrew its tables");
                OAR_HIP(hipMemcpyAsync(d_pfrows, prow, ph.n_rows * sizeof(k::LmPfRow), hipMemcpyHostToDevice, s));
                OAR_HIP(hipMemcpyAsync(d_pftiles, ptile, ph.n_tiles * sizeof(k::LmPfTile), hipMemcpyHostToDevice, s));
                gemm_phase(lm, P, s, d_pfrows, d_pftiles, ptile, ph.chunk, ph.tile0, reinterpret_cast<float*>(w + pfq_o), reinterpret_cast<float*>(w + pfo_o),
                           reinterpret_cast<float*>(w + pfh_o));
                ++gemm_phases;
            }
            k::lm_step(s, P, &d_stage->step, st.step.nrows, st.step.nhead, max_pos, attention);
            if ((i + 1) % k::kLmQueueStride == 0) {
                const size_t ce = (size_t)(((i + 1) / k::kLmQueueStride - 1) % k::kLmQueueRing);
                OAR_HIP(hipMemcpyAsync(pin_state + ce, P.state, sizeof(k::LmState), hipMemcpyDeviceToHost, s));
                OAR_HIP(hipEventRecord(lm->queue_ev[ce], s));
            }
        }
        OAR_HIP(hipGetLastError());
        OAR_HIP(hipMemcpyAsync(req->tokens, tp.out_tokens, (size_t)S * MN * 4, hipMemcpyDeviceToHost, s));
        if (logits) OAR_HIP(hipMemcpyAsync(req->logits, tp.out_logits, (size_t)S * MN * V * 4, hipMemcpyDeviceToHost, s));
        OAR_HIP(hipStreamSynchronize(s));
        if (Profiler::get().enabled) Profiler::get().flush();
        k::LmQueueStats qs{};
        qs.steps = Q.step(); qs.rows = Q.rows(); qs.admissions = Q.admissions(); qs.gemm_phases = gemm_phases; qs.min_slot_admissions = Q.min_slot_admissions(); qs.min_slot_turnovers = Q.min_slot_turnovers();
        for (int q = 0; q < S; ++q) {
            int n = MN;
            if (req->eos_token_id >= 0)
                for (int g = 0; g < MN; ++g)
                    if (req->tokens[(size_t)q * MN + g] == req->eos_token_id) { n = g + 1; break; }
            req->counts[q] = n;
            // rows the sequence got after its eos step: their logits were written by the chain and are zeroed here, as the rows behind them are
            const int dead = Q.produced()[(size_t)q] - n;
            if (dead > 0) {
                qs.dead_rows += dead;
                qs.max_dead_rows = std::max<int64_t>(qs.max_dead_rows, dead);
                if (logits) std::memset(req->logits + ((size_t)q * MN + n) * V, 0, (size_t)dead * V * 4);
            }
        }
        lm->queue_stats = qs;
    });
}

oar_status oar_lm_queue_stats(const oar_lm* lm, int64_t* stats, int32_t n_stats) {
    return guard([&] {
        OAR_CHECK(lm && stats && n_stats >= 0, OAR_INVALID_INPUT, "oar_lm_queue_stats: null argument");
        std::lock_guard<std::mutex> lk(lm->mu);
        const k::LmQueueStats& q = lm->queue_stats;
        const int64_t v[8] = {q.steps, q.rows, q.dead_rows, q.admissions, q.gemm_phases, q.max_dead_rows, q.min_slot_admissions, q.min_slot_turnovers};
        for (int32_t i = 0; i < n_stats && i < 8; ++i) stats[i] = v[i];
    });
}

oar_status oar_lm_set_prefill(oar_lm* lm, int32_t mode, int32_t chunk_rows) {
    return guard([&] {
        OAR_CHECK(lm, OAR_INVALID_INPUT, "oar_lm_set_prefill: null model");
        OAR_CHECK(mode == OAR_LM_PREFILL_ROWS || mode == OAR_LM_PREFILL_GEMM, OAR_INVALID_INPUT, "oar_lm_set_prefill: mode is neither OAR_LM_PREFILL_ROWS nor OAR_LM_PREFILL_GEMM");
        OAR_CHECK(chunk_rows >= 0 && chunk_rows <= k::kLmPrefillMaxChunk, OAR_INVALID_INPUT, "oar_lm_set_prefill: chunk_rows outside 0..65536");
        std::lock_guard<std::mutex> lk(lm->mu);
        lm->prefill_mode = mode;
        lm->chunk_rows = chunk_rows == 0 ? k::kLmPrefillDefaultChunk : chunk_rows;
    });
}

oar_status oar_lm_set_decode(oar_lm* lm, int32_t attention, int32_t split_keys, int32_t stop_at_eos) {
    return guard([&] {
        OAR_CHECK(lm, OAR_INVALID_INPUT, "oar_lm_set_decode: null model");
        OAR_CHECK(attention == OAR_LM_ATTN_SERIAL || attention == OAR_LM_ATTN_SPLIT, OAR_INVALID_INPUT, "oar_lm_set_decode: attention is neither OAR_LM_ATTN_SERIAL nor OAR_LM_ATTN_SPLIT");
        OAR_CHECK(split_keys == 0 || k::lm_split_keys_supported(split_keys), OAR_INVALID_INPUT, "oar_lm_set_decode: split_keys is neither 0 nor a multiple of 64 in 64..4096");
        OAR_CHECK(stop_at_eos == 0 || stop_at_eos == 1, OAR_INVALID_INPUT, "oar_lm_set_decode: stop_at_eos outside {0, 1}");
        std::lock_guard<std::mutex> lk(lm->mu);
        lm->attention = attention;
        lm->split_keys = split_keys == 0 ? k::kLmSplitDefault : split_keys;
        lm->stop_at_eos = stop_at_eos;
    });
}

oar_status oar_lm_decode_stats(const oar_lm* lm, int64_t* steps_limit, int64_t* steps_enqueued) {
    return guard([&] {
        OAR_CHECK(lm, OAR_INVALID_INPUT, "oar_lm_decode_stats: null model");
        std::lock_guard<std::mutex> lk(lm->mu);
        if (steps_limit) *steps_limit = lm->steps_limit;
        if (steps_enqueued) *steps_enqueued = lm->steps_enqueued;
    });
}

oar_status oar_lm_prefill_cost(oar_lm* lm, int32_t n_seq, const int32_t* lengths, double* flops, double* bytes, int32_t* n_kernels) {
    return guard([&] {
        OAR_CHECK(lm && lengths && n_seq >= 1 && n_seq <= lm->cfg.max_sequences, OAR_INVALID_INPUT, "oar_lm_prefill_cost: null argument or n_seq outside 1..max_sequences");
        int64_t total = 0;
        for (int s = 0; s < n_seq; ++s) {
            OAR_CHECK(lengths[s] >= 1 && lengths[s] <= lm->cfg.max_positions, OAR_INVALID_INPUT, "oar_lm_prefill_cost: a length outside 1..max_positions");
            total += lengths[s];
        }
        OAR_CHECK(total < (1 << 24), OAR_INVALID_INPUT, "oar_lm_prefill_cost: prompts too long");
        int chunk_rows;
        { std::lock_guard<std::mutex> lk(lm->mu); chunk_rows = lm->chunk_rows; }
        const oar_lm_cfg& c = lm->cfg;
        std::vector<k::LmPfSpan> spans;
        std::vector<int> first, chunk;
        k::lm_pf_chunks(lengths, n_seq, chunk_rows, spans, first, chunk);
        const double es = lm->bf16 ? 2.0 : 4.0, D = c.hidden, Hd = (double)c.heads * c.head_dim, Kd = (double)c.kv_heads * c.head_dim, F = c.intermediate, L = c.layers;
        const double Nqkv = Hd + 2 * Kd;
        double f = 0.0, b = 0.0;
        for (size_t ci = 0; ci < chunk.size(); ++ci) {
            const double M = chunk[ci];
            std::vector<k::LmPfTile> tiles;
            k::lm_pf_tiles(spans.data() + first[ci], first[ci + 1] - first[ci], c.heads, tiles);
            double ab = 0.0, af = 0.0;
            k::lm_pf_attn_cost(tiles.data(), (int64_t)tiles.size(), c.head_dim, &ab, &af);
            // every launch: its weights once, its input and output rows
            f += L * 2.0 * M * Nqkv * D + (L - 1) * (af + 2.0 * M * (D * Hd + 2.0 * F * D + D * F));
            b += L * (es * Nqkv * D + 4.0 * M * (D + Nqkv)) + (L - 1) * (ab + es * (D * Hd + 2.0 * F * D + D * F) + 4.0 * M * ((Hd + 2 * D) + (D + F) + (F + 2 * D)));
        }
        if (flops) *flops = f;
        if (bytes) *bytes = b;
        if (n_kernels) *n_kernels = k::lm_pf_launches((int)chunk.size(), c.layers);
    });
}

// The two kernels of the GEMM prefill on caller-chosen shapes.  Every argument is checked before the device is asked for, so a bad call launches nothing (and
// answers the same with or without a GPU).
oar_status oar_k_lm_gemm(const float* x, int32_t m, int32_t k_, const void* w, int32_t w_dtype, int32_t n, float* o_io, size_t o_floats, size_t o_off) {
    return guard([&] {
        OAR_CHECK(x && w && o_io, OAR_INVALID_INPUT, "oar_k_lm_gemm: null buffer");
        OAR_CHECK(w_dtype == OAR_LM_F32 || w_dtype == OAR_LM_BF16, OAR_INVALID_INPUT, "oar_k_lm_gemm: w_dtype is neither OAR_LM_F32 nor OAR_LM_BF16");
        OAR_CHECK(m >= 1 && m <= (1 << 21) && n >= 1 && n < (1 << 24) && k_ >= 4 && k_ < (1 << 24), OAR_INVALID_INPUT, "oar_k_lm_gemm: m outside 1..2^21, or n or k outside the limits");
        OAR_CHECK(k_ % 4 == 0, OAR_UNSUPPORTED_OP, "oar_k_lm_gemm: k must be a multiple of 4 (rows are read 16 bytes at a time)");
        const uint64_t out = (uint64_t)m * (uint64_t)n;
        OAR_CHECK(view_fits(o_off, out, o_floats), OAR_INVALID_INPUT, "oar_k_lm_gemm: the output does not fit o_floats");
        require_device();
        const size_t es = w_dtype == OAR_LM_BF16 ? 2 : 4;
        DirectCall dc;
        k::LmGemmP p{};
        p.mode = k::LM_GEMM_PLAIN; p.bf16 = w_dtype == OAR_LM_BF16; p.M = m; p.N = n; p.K = k_; p.Kp = k_; p.x = dc.in(x, (size_t)m * k_ * 4); p.x_ld = k_;
        p.w = dc.in(w, (size_t)n * k_ * es);
        p.y = dc.io(o_io, o_floats) + o_off; p.y_ld = n;
        k::lm_gemm(nullptr, p);
        dc.finish();
    });
}

oar_status oar_k_lm_prefill_attention(const float* q, const float* kcache, const float* vcache, int32_t n_seq, int32_t max_positions, const int32_t* starts,
                                      const int32_t* lens, int32_t heads, int32_t kv_heads, int32_t head_dim, float* o_io, size_t o_floats, size_t o_off) {
    return guard([&] {
        OAR_CHECK(q && kcache && vcache && starts && lens && o_io, OAR_INVALID_INPUT, "oar_k_lm_prefill_attention: null buffer");
        OAR_CHECK(heads >= 1 && heads < (1 << 16) && kv_heads >= 1 && heads % kv_heads == 0, OAR_INVALID_INPUT, "oar_k_lm_prefill_attention: heads outside 1..65535 or no multiple of kv_heads");
        OAR_CHECK(k::lm_pf_head_dim_supported(head_dim), OAR_UNSUPPORTED_OP, "oar_k_lm_prefill_attention: head_dim must be a multiple of 4 in 8..128");
        OAR_CHECK(n_seq >= 1 && n_seq <= (1 << 16) && max_positions >= 1 && max_positions <= (1 << 20), OAR_INVALID_INPUT, "oar_k_lm_prefill_attention: n_seq outside 1..65536 or max_positions outside 1..2^20");
        std::vector<k::LmPfSpan> spans((size_t)n_seq);
        int64_t rows = 0;
        for (int32_t i = 0; i < n_seq; ++i) {
            OAR_CHECK(lens[i] >= 1 && starts[i] >= 0 && (int64_t)starts[i] + lens[i] <= max_positions, OAR_INVALID_INPUT, "oar_k_lm_prefill_attention: an empty sequence or positions outside the cache");
            spans[(size_t)i] = k::LmPfSpan{i, starts[i], lens[i], (int32_t)rows};
            rows += lens[i];
            OAR_CHECK(rows < (1 << 24), OAR_INVALID_INPUT, "oar_k_lm_prefill_attention: more than 2^24 query rows");
        }
        const int64_t Hd = (int64_t)heads * head_dim, n_tiles = k::lm_pf_tile_count(spans.data(), n_seq, heads);
        OAR_CHECK(n_tiles < ((int64_t)1 << 31), OAR_INVALID_INPUT, "oar_k_lm_prefill_attention: workgroup count above 2^31");
        OAR_CHECK((o_off & 3) == 0, OAR_INVALID_INPUT, "oar_k_lm_prefill_attention: o_off is no multiple of 4 floats");
        OAR_CHECK(view_fits(o_off, (uint64_t)rows * (uint64_t)Hd, o_floats), OAR_INVALID_INPUT, "oar_k_lm_prefill_attention: the output does not fit o_floats");
        std::vector<k::LmPfTile> tiles;
        k::lm_pf_tiles(spans.data(), n_seq, heads, tiles);
        require_device();
        const size_t qb = (size_t)rows * Hd * 4, cb = (size_t)n_seq * kv_heads * max_positions * head_dim * 4;
        DirectCall dc;
        k::LmPfAttnP p{};
        p.q = dc.in(q, qb); p.q_ld = (int)Hd; p.kc = dc.in(kcache, cb); p.vc = dc.in(vcache, cb); p.H = heads; p.KVH = kv_heads; p.dh = head_dim; p.maxpos = max_positions;
        p.scale = 1.0f / sqrtf((float)head_dim); p.o = dc.io(o_io, o_floats) + o_off; p.o_ld = (int)Hd;
        p.tiles = dc.in(tiles.data(), tiles.size() * sizeof(k::LmPfTile)); p.n_tiles = (int)tiles.size();
        double bytes = 0.0, flops = 0.0;
        k::lm_pf_attn_cost(tiles.data(), (int64_t)tiles.size(), head_dim, &bytes, &flops);
        k::lm_prefill_attention(nullptr, p, bytes, flops);
        dc.finish();
    });
}

// The attention of a decode step alone: split_keys 0 runs lm_attn_kernel, else lm_attn_split + lm_attn_merge over a workspace filled with 0xFF bytes (a partial
// read without having been written shows as NaN).
oar_status oar_k_lm_decode_attention(const float* q, const float* kcache, const float* vcache, int32_t n_seq, int32_t max_positions, int32_t n_rows, const int32_t* row_seq,
                                     const int32_t* row_pos, int32_t heads, int32_t kv_heads, int32_t head_dim, int32_t split_keys, float* o_io, size_t o_floats, size_t o_off) {
    return guard([&] {
        OAR_CHECK(q && kcache && vcache && row_seq && row_pos && o_io, OAR_INVALID_INPUT, "oar_k_lm_decode_attention: null buffer");
        OAR_CHECK(heads >= 1 && heads < (1 << 16) && kv_heads >= 1 && heads % kv_heads == 0, OAR_INVALID_INPUT, "oar_k_lm_decode_attention: heads outside 1..65535 or no multiple of kv_heads");
        OAR_CHECK(k::lm_head_dim_supported(head_dim), OAR_UNSUPPORTED_OP, "oar_k_lm_decode_attention: head_dim must be a multiple of 4 in 8..128");
        OAR_CHECK(n_seq >= 1 && n_seq <= (1 << 16) && max_positions >= 1 && max_positions <= (1 << 20), OAR_INVALID_INPUT, "oar_k_lm_decode_attention: n_seq outside 1..65536 or max_positions outside 1..2^20");
        OAR_CHECK(n_rows >= 1 && n_rows <= k::kLmRows, OAR_INVALID_INPUT, "oar_k_lm_decode_attention: n_rows outside 1..16");
        OAR_CHECK(split_keys == 0 || k::lm_split_keys_supported(split_keys), OAR_INVALID_INPUT, "oar_k_lm_decode_attention: split_keys is neither 0 nor a multiple of 64 in 64..4096");
        k::LmStep st{};
        int mp = 0;
        for (int32_t i = 0; i < n_rows; ++i) {
            OAR_CHECK(row_seq[i] >= 0 && row_seq[i] < n_seq && row_pos[i] >= 0 && row_pos[i] < max_positions, OAR_INVALID_INPUT, "oar_k_lm_decode_attention: a row outside the sequences or the cache");
            st.rows[i].seq = row_seq[i]; st.rows[i].pos = row_pos[i];
            mp = std::max(mp, (int)row_pos[i]);
        }
        st.nrows = n_rows;
        const int64_t Hd = (int64_t)heads * head_dim;
        OAR_CHECK((o_off & 3) == 0, OAR_INVALID_INPUT, "oar_k_lm_decode_attention: o_off is no multiple of 4 floats");
        OAR_CHECK(view_fits(o_off, (uint64_t)n_rows * (uint64_t)Hd, o_floats), OAR_INVALID_INPUT, "oar_k_lm_decode_attention: the output does not fit o_floats");
        require_device();
        const size_t qb = (size_t)n_rows * Hd * 4, cb = (size_t)n_seq * kv_heads * max_positions * head_dim * 4;
        const size_t wsb = split_keys ? k::lm_split_ws_floats(heads, head_dim, max_positions, split_keys) * 4 : 0;
        DirectCall dc;
        const int one = 1;
        k::LmAttnArgs a{};
        a.q = dc.in(q, qb); a.q_ld = (int)Hd; a.kc = dc.in(kcache, cb); a.vc = dc.in(vcache, cb); a.H = heads; a.KVH = kv_heads; a.dh = head_dim;
        a.maxpos = max_positions; a.o = dc.io(o_io, o_floats) + o_off; a.o_ld = (int)Hd; a.st = dc.in(&st, sizeof st); a.alive = dc.in(&one, 4);
        a.ws = dc.scratch<float>(wsb, 0xFF); a.split_keys = split_keys;
        OAR_HIP(hipDeviceSynchronize());
        k::lm_attention(nullptr, a, split_keys ? k::LM_ATTN_SPLIT : k::LM_ATTN_SERIAL, n_rows, false, mp);
        dc.finish();
    });
}

// What oar_lm_generate_ex asks of its arguments; needs no model and no device.
oar_status oar_lm_logits_check(const oar_lm_cfg* cfg, const oar_lm_request* req, const oar_lm_logits_cfg* lp) {
    return guard([&] {
        static const std::string fn = "oar_lm_generate_ex";
        OAR_CHECK(cfg && req, OAR_INVALID_INPUT, fn + ": null argument");
        OAR_CHECK(cfg->max_sequences >= 1 && cfg->max_sequences <= k::kLmRows && cfg->vocab >= 2 && cfg->max_positions >= 2, OAR_INVALID_INPUT,
                  fn + ": max_sequences outside 1..16, vocab or max_positions below 2");
        OAR_CHECK(req->n_seq >= 1 && req->n_seq <= cfg->max_sequences, OAR_INVALID_INPUT, fn + ": n_seq outside 1..max_sequences");
        check_request(*cfg, *req, fn);
        (void)logits_plan(*cfg, *req, lp, fn);
    });
}

// lm_select_kernel alone.  Row i is sequence i of a one-step call: with a history of H >= 1 ids the row is generated token 1 of a sequence whose prompt part is the
// first H - 1 ids and whose token 0 -- the token "fed back by the step before" -- is the last id, so the kernel's append runs too; H = 0 is token 0 of an empty prompt.
oar_status oar_k_lm_select(const float* logits, int32_t n_rows, int32_t vocab, const int32_t* hist_lengths, const int32_t* const* hist_ids, float repetition_penalty,
                           int32_t no_repeat_ngram_size, int32_t* tokens_io, size_t n_tokens, size_t off) {
    return guard([&] {
        static const std::string fn = "oar_k_lm_select";
        OAR_CHECK(logits && hist_lengths && hist_ids && tokens_io, OAR_INVALID_INPUT, fn + ": null buffer");
        OAR_CHECK(n_rows >= 1 && n_rows <= k::kLmRows, OAR_INVALID_INPUT, fn + ": n_rows outside 1..16");
        OAR_CHECK(vocab >= 2 && vocab < (1 << 24), OAR_INVALID_INPUT, fn + ": vocab outside 2..2^24 - 1");
        check_processors(repetition_penalty, no_repeat_ngram_size, vocab, fn);
        OAR_CHECK(view_fits(off, (uint64_t)n_rows, n_tokens), OAR_INVALID_INPUT, fn + ": the tokens do not fit n_tokens");
        std::vector<const int32_t*> ids;
        std::vector<int32_t> hlen;
        k::LmStep st{};
        std::vector<int32_t> toks((size_t)k::kLmRows * 2, 0);
        int cap = 1;
        for (int32_t i = 0; i < n_rows; ++i) {
            const int64_t H = hist_lengths[i];
            check_history(hist_ids[i], H, fn);
            ids.push_back(hist_ids[i]); hlen.push_back(H > 0 ? (int32_t)H - 1 : 0);
            st.rows[i].seq = i; st.rows[i].gen = H > 0 ? 1 : 0;
            if (H > 0) toks[(size_t)i * 2] = hist_ids[i][H - 1];
            st.head[i] = i;
            cap = std::max(cap, (int)H);
        }
        st.nrows = st.nhead = n_rows;
        require_device();
        const int ld = k::lm_select_ld(vocab), words = k::lm_select_words(vocab);
        std::vector<int32_t> hist;
        std::vector<uint32_t> seen;
        history_tables(ids, hlen, vocab, cap, hist, seen);
        DevBuf dl, dst, dh, dn, dsn, dt, dp, dout;
        dl.reserve((size_t)n_rows * ld * 4); dst.reserve(sizeof st); dh.reserve(hist.size() * 4); dn.reserve((size_t)k::kLmRows * 4); dsn.reserve(seen.size() * 4);
        dt.reserve(toks.size() * 4); dp.reserve((size_t)k::kLmRows * 8); dout.reserve((size_t)k::kLmRows * 4);
        OAR_HIP(hipMemcpy2D(dl.p, (size_t)ld * 4, logits, (size_t)vocab * 4, (size_t)vocab * 4, (size_t)n_rows, hipMemcpyHostToDevice));
        OAR_HIP(hipMemcpy(dst.p, &st, sizeof st, hipMemcpyHostToDevice));
        OAR_HIP(hipMemcpy(dh.p, hist.data(), hist.size() * 4, hipMemcpyHostToDevice));
        OAR_HIP(hipMemcpy(dn.p, hlen.data(), hlen.size() * 4, hipMemcpyHostToDevice));
        OAR_HIP(hipMemcpy(dsn.p, seen.data(), seen.size() * 4, hipMemcpyHostToDevice));
        OAR_HIP(hipMemcpy(dt.p, toks.data(), toks.size() * 4, hipMemcpyHostToDevice));
        OAR_HIP(hipMemset(dout.p, 0xFF, (size_t)k::kLmRows * 4));
        OAR_HIP(hipDeviceSynchronize());
        k::LmSelectP p{};
        p.st = dst.as<k::LmStep>(); p.logits = dl.as<float>(); p.ld = ld; p.V = vocab; p.words = words; p.hist = dh.as<int32_t>(); p.cap = cap; p.hlen = dn.as<int32_t>();
        p.seen = dsn.as<uint32_t>(); p.tokens = dt.as<int32_t>(); p.max_new = 2; p.penalty = repetition_penalty; p.ngram = no_repeat_ngram_size; p.part = dp.p;
        p.tok_out = dout.as<int32_t>();
        k::lm_select(nullptr, p, n_rows, false);
        OAR_HIP(hipGetLastError());
        std::vector<int32_t> out((size_t)k::kLmRows);
        OAR_HIP(hipMemcpy(out.data(), dout.p, out.size() * 4, hipMemcpyDeviceToHost));
        for (int32_t i = 0; i < n_rows; ++i) tokens_io[off + (size_t)i] = out[(size_t)i];
    });
}
