// engine_rewrite.cc -- the load-time graph rewriter: what happens to a model between the parser and the first plan.  Host-only (no HIP call): the passes read
// the nodes, the initializers and the host predicates k::*_supported.  Rewriter::run() is the table of contents: the ingestion loop, the 17 passes in the order
// that matters (3b - 3e in front of 4, 10 behind everything), the id assignment.  Pass 0's Loop matchers are in engine_loops.cc.
#include "graph_rewrite.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "common.h"

namespace oar {

using k::Act;
bool is_fusable_act(const std::string& op) {
    return op == "Relu" || op == "HardSwish" || op == "HardSigmoid" || op == "Sigmoid" || op == "LeakyRelu" || op == "Tanh" || op == "Gelu";
}
Act act_of(const GNode& n) {
    Act a;
    if (n.op == "Relu") a.kind = k::ACT_RELU;
    else if (n.op == "HardSwish") a.kind = k::ACT_HSWISH;
    else if (n.op == "HardSigmoid") { a.kind = k::ACT_HSIGMOID; a.alpha = n.af("alpha", 0.2f); a.beta = n.af("beta", 0.5f); }
    else if (n.op == "Sigmoid") a.kind = k::ACT_SIGMOID;
    else if (n.op == "LeakyRelu") { a.kind = k::ACT_LEAKY; a.alpha = n.af("alpha", 0.01f); }
    else if (n.op == "Tanh") a.kind = k::ACT_TANH;
    else if (n.op == "Erf") a.kind = k::ACT_ERF;
    else if (n.op == "Sqrt") a.kind = k::ACT_SQRT;
    else if (n.op == "Exp") a.kind = k::ACT_EXP;
    else if (n.op == "Abs") a.kind = k::ACT_ABS;
    else if (n.op == "Neg") a.kind = k::ACT_NEG;
    else if (n.op == "Reciprocal") a.kind = k::ACT_RECIP;
    else if (n.op == "Log") a.kind = k::ACT_LOG;
    else if (n.op == "Gelu") a.kind = n.as("approximate", "none") == "tanh" ? k::ACT_GELU_TANH : k::ACT_GELU_ERF;
    else if (n.op == "Softplus") a.kind = k::ACT_SOFTPLUS;
    else if (n.op == "Floor") a.kind = k::ACT_FLOOR;
    else if (n.op == "Ceil") a.kind = k::ACT_CEIL;
    else if (n.op == "Round") a.kind = k::ACT_ROUND;
    else if (n.op == "Not") a.kind = k::ACT_NOT;
    return a;
}

namespace {

struct Rewriter {
    std::vector<GNode> nodes;
    std::map<std::string, HostTensor> inits;
    std::set<std::string> graph_outs;
    int64_t opset = 17;
    std::map<std::string, std::vector<GNode>> ln_spelled;   // pass 2c: the nodes each rewritten LayerNormalization replaced, by its output name
    bool fuse_add_ln = true;                                // pass 10

    // ---- the matcher toolkit, by node index throughout.  scan() reads the current `nodes` at the head of a pass (readers, producers, nobody dead) and sweep()
    // drops what the pass killed.  Every node a helper returns is live and PLAIN: no fused activation (in front of pass 4, pass 3 alone attaches one, to Conv /
    // ConvTranspose / Linear / Gemm / Add) and no fused residual (pass 4, behind passes 3b - 3e, is the first to attach one).
    using V = std::vector<int64_t>;
    std::map<std::string, std::vector<int>> cons;
    std::map<std::string, int> producer;
    std::vector<bool> dead;
    static std::map<std::string, std::vector<int>> consumers(const std::vector<GNode>& ns) {
        std::map<std::string, std::vector<int>> c;
        for (int i = 0; i < (int)ns.size(); ++i)
            for (auto& s : ns[i].in)
                if (!s.empty()) c[s].push_back(i);
        return c;
    }
    bool is_init(const std::string& s) const { return inits.count(s) != 0; }
    // an OAR_FUSE_* switch that is on unless set to 0.  Read at every load, never cached: tests load both arms in one process
    static bool switch_on(const char* name) { const char* e = getenv(name); return !e || atoi(e) != 0; }
    void scan() {
        cons = consumers(nodes);
        producer.clear();
        for (int i = 0; i < (int)nodes.size(); ++i) for (auto& o : nodes[i].out) producer[o] = i;
        dead.assign(nodes.size(), false);
    }
    void sweep() {
        std::vector<GNode> keep;
        for (int i = 0; i < (int)nodes.size(); ++i) if (!dead[i]) keep.push_back(std::move(nodes[i]));
        nodes.swap(keep);
    }
    bool plain(int i, const char* op) const { return !dead[i] && nodes[i].op == op && nodes[i].act.kind == k::ACT_NONE && nodes[i].residual.empty(); }
    bool single_use(const std::string& v) { return cons[v].size() == 1 && !graph_outs.count(v); }
    int prodn(const std::string& v, const char* op) const {    // the producer `op` of v (v may have several readers)
        auto it = producer.find(v);
        return it != producer.end() && plain(it->second, op) ? it->second : -1;
    }
    int prod1(const std::string& v, const char* op) { return single_use(v) ? prodn(v, op) : -1; }   // ... and v read by nobody else
    int reader1(const std::string& v, const char* op) {  // the single consumer of v, an `op` reading it first
        if (!single_use(v)) return -1;
        const int c = cons[v][0];
        return plain(c, op) && nodes[c].in[0] == v ? c : -1;
    }
    V ints(const std::string& v) const {
        auto it = inits.find(v);
        return it == inits.end() || it->second.dtype == DType::F32 ? V{} : it->second.i;
    }
    V target(int r) const { return nodes[r].in.size() < 2 || nodes[r].ai("allowzero", 0) != 0 ? V{} : ints(nodes[r].in[1]); }   // of a Reshape
    bool perm_is(int t, std::initializer_list<int64_t> want) const { return nodes[t].ais("perm") == V(want); }
    bool axes_are(int n, int64_t a, int64_t rank) const {              // opset 13 input or the older attribute; a or a - rank
        const V ax = nodes[n].in.size() > 1 && !nodes[n].in[1].empty() ? ints(nodes[n].in[1]) : nodes[n].ais("axes");
        return ax.size() == 1 && (ax[0] == a || ax[0] == a - rank);
    }
    const HostTensor* f32_scalar(const std::string& v) const {
        auto it = inits.find(v);
        return it != inits.end() && it->second.dtype == DType::F32 && it->second.f.size() == 1 ? &it->second : nullptr;
    }
    static void iattr(GNode& n, const char* k, int64_t v) { Attr a; a.kind = Attr::I; a.i = v; n.attrs[k] = a; }
    static void fattr(GNode& n, const char* k, float v) { Attr a; a.kind = Attr::F; a.f = v; n.attrs[k] = a; }

    // ---- pass 0: Loop.  There is no generic sub-graph executor: two bodies are recognised, by their interface, and replaced by fused operators.
    //   4 inputs / 5 outputs: the SLANet structure head's step (PaddleOCR SLAHead._decode: AttentionGRUCell + GRUCell + both output heads, greedy feedback
    //     of the arg max)  ->  Linear (the loop-invariant projection of the features) + ONE SLADecode node (match_sla_loop)
    //   3 + 2 Ld inputs: the greedy step of a transformer decoder with a key / value cache (PP-FormulaNet)  ->  ONE FormulaDecode node; the empty initial
    //     caches and their producers leave the graph (match_formula_loop)
    // Anything else, or a body that is not one of these in a spelling its matcher tolerates, is refused with the name of the first body node that did not fit.
    void pass_0_loops() {
        std::vector<GNode> out;
        std::vector<std::string> dropped;
        for (size_t ni = 0; ni < nodes.size(); ++ni) {
            GNode& n = nodes[ni];
            if (n.op != "Loop") { out.push_back(n); continue; }
            auto bit = n.attrs.find("body");
            const OnnxModel* body = bit != n.attrs.end() && bit->second.kind == Attr::G && bit->second.g ? bit->second.g.get() : nullptr;
            if (!body || (body->inputs.size() == 4 && body->outputs.size() == 5)) {
                GNode lin, dec;
                match_sla_loop(n, inits, opset, lin, dec);
                out.push_back(std::move(lin));
                out.push_back(std::move(dec));
            } else if (body->inputs.size() >= 5 && body->inputs.size() % 2 == 1) {
                GNode dec;
                match_formula_loop(n, nodes, inits, opset, graph_outs, dec, dropped);
                out.push_back(std::move(dec));
            } else {
                fail(OAR_UNSUPPORTED_OP, "Loop (" + (n.out.empty() ? std::string("?") : n.out[0]) + "): a body with " + std::to_string(body->inputs.size()) + " inputs and " +
                                             std::to_string(body->outputs.size()) + " outputs is not supported: only the SLA decode step (i, cond, h, pre -> cond, h, pre, logits, loc) and the formula decode " +
                                             "step (i, cond, tok, K_1, V_1, ... -> cond, tok, K_1', V_1', ..., tok [, logits]) are executed as Loop bodies");
            }
        }
        nodes.swap(out);
        // the empty initial caches: their ConstantOfShape goes, and its shape Concat when nothing else reads it (the planner never sees a zero-extent tensor)
        for (int round = 0; round < 2 && !dropped.empty(); ++round) {
            std::vector<std::string> next;
            for (const std::string& nm : dropped) {
                bool read = graph_outs.count(nm) != 0;
                for (const GNode& n : nodes) for (auto& s : n.in) if (s == nm) read = true;
                if (read) continue;
                for (size_t i = 0; i < nodes.size(); ++i) {
                    if (std::find(nodes[i].out.begin(), nodes[i].out.end(), nm) == nodes[i].out.end()) continue;
                    if (nodes[i].op == "ConstantOfShape" || (round == 1 && nodes[i].op == "Concat")) {
                        if (round == 0) next.insert(next.end(), nodes[i].in.begin(), nodes[i].in.end());
                        nodes.erase(nodes.begin() + (long)i);
                    }
                    break;
                }
            }
            dropped.swap(next);
        }
    }

    // ---- pass 1: fold BatchNormalization into the producing Conv / ConvTranspose
    void pass_1_fold_batchnorm() {
        scan();
        for (int i = 0; i < (int)nodes.size(); ++i) {
            GNode& bn = nodes[i];
            if (bn.op != "BatchNormalization" || bn.in.size() < 5) continue;
            auto pit = producer.find(bn.in[0]);
            if (pit == producer.end()) continue;
            GNode& cv = nodes[pit->second];
            if (cv.op != "Conv" && cv.op != "ConvTranspose") continue;
            if (cons[bn.in[0]].size() != 1 || graph_outs.count(bn.in[0])) continue;
            if (!is_init(cv.in[1]) || !is_init(bn.in[1]) || !is_init(bn.in[2]) || !is_init(bn.in[3]) || !is_init(bn.in[4])) continue;
            if (cv.in.size() > 2 && !cv.in[2].empty() && !is_init(cv.in[2])) continue;
            const HostTensor& W = inits[cv.in[1]];
            const auto &ga = inits[bn.in[1]].f, &be = inits[bn.in[2]].f, &mu = inits[bn.in[3]].f, &va = inits[bn.in[4]].f;
            float eps = bn.af("epsilon", 1e-5f);
            int64_t C = (int64_t)ga.size();
            OAR_CHECK(W.dtype == DType::F32 && W.dims.size() == 4, OAR_MODEL_LOAD, "BN fold: conv weight must be a rank-4 f32 initializer (" + cv.in[1] + ")");
            OAR_CHECK(C > 0 && (int64_t)be.size() == C && (int64_t)mu.size() == C && (int64_t)va.size() == C, OAR_MODEL_LOAD,
                      "BatchNormalization: scale / bias / mean / var must all have C elements (" + bn.out[0] + ")");
            if (cv.in.size() > 2 && !cv.in[2].empty())
                OAR_CHECK((int64_t)inits[cv.in[2]].f.size() == C, OAR_MODEL_LOAD, "BN fold: conv bias must have C elements (" + cv.in[2] + ")");
            HostTensor W2 = W;
            std::vector<float> b2(C, 0.f);
            if (cv.in.size() > 2 && !cv.in[2].empty()) b2 = inits[cv.in[2]].f;
            std::vector<float> sc(C);
            for (int64_t c = 0; c < C; ++c) sc[c] = ga[c] / std::sqrt(va[c] + eps);
            if (cv.op == "Conv") {
                OAR_CHECK(W.dims[0] == C, OAR_SHAPE_MISMATCH, "BN fold: channel mismatch");
                int64_t per = numel(W.dims) / C;
                for (int64_t c = 0; c < C; ++c)
                    for (int64_t j = 0; j < per; ++j) W2.f[c * per + j] = W.f[c * per + j] * sc[c];
            } else {
                int64_t g = cv.ai("group", 1);
                if (g != 1) continue;
                OAR_CHECK(W.dims[1] == C, OAR_SHAPE_MISMATCH, "BN fold (convT): channel mismatch");
                int64_t khw = W.dims[2] * W.dims[3];
                for (int64_t ci = 0; ci < W.dims[0]; ++ci)
                    for (int64_t c = 0; c < C; ++c)
                        for (int64_t j = 0; j < khw; ++j) W2.f[(ci * C + c) * khw + j] = W.f[(ci * C + c) * khw + j] * sc[c];
            }
            for (int64_t c = 0; c < C; ++c) b2[c] = (b2[c] - mu[c]) * sc[c] + be[c];
            std::string wn = cv.in[1] + "::bnfold" + std::to_string(i), bnm = wn + "::b";
            W2.name = wn;
            inits[wn] = std::move(W2);
            HostTensor B; B.name = bnm; B.dtype = DType::F32; B.dims = {C}; B.f = b2;
            inits[bnm] = std::move(B);
            cv.in.resize(3);
            cv.in[1] = wn; cv.in[2] = bnm;
            cv.out[0] = bn.out[0];
            producer[bn.out[0]] = pit->second;
            dead[i] = true;
        }
        sweep();
    }

    // ---- pass 2: MatMul(x, Wconst) + Add(const bias)  ->  Linear
    void pass_2_linear() {
        scan();
        for (int i = 0; i < (int)nodes.size(); ++i) {
            GNode& mm = nodes[i];
            if (mm.op != "MatMul" || !is_init(mm.in[1]) || inits[mm.in[1]].dims.size() != 2) continue;
            mm.op = "Linear";
            auto& cs = cons[mm.out[0]];
            if (cs.size() != 1 || graph_outs.count(mm.out[0])) continue;
            GNode& ad = nodes[cs[0]];
            if (ad.op != "Add" || dead[cs[0]]) continue;
            int other = ad.in[0] == mm.out[0] ? 1 : 0;
            if (!is_init(ad.in[other])) continue;
            const HostTensor& b = inits[ad.in[other]];
            if (numel(b.dims) != inits[mm.in[1]].dims[1] || b.dims.empty() || b.dims.back() != numel(b.dims)) continue;
            mm.bias = ad.in[other];
            mm.out[0] = ad.out[0];
            dead[cs[0]] = true;
        }
        sweep();
    }

    // ---- pass 2b: GELU as exporters below opset 20 spell it (SVTRv2's MLPs and conv stem): x * 0.5 * (1 + erf(x / sqrt(2))), in either association
    //   Mul(Mul(x, Add(Erf(Div(x, 1.41421)), 1)), 0.5)   or   Mul(Mul(x, 0.5), Add(Erf(..), 1));  x / sqrt(2) may also be Mul(x, 0.70711)
    // becomes ONE Gelu node (5 element-wise launches over the widest tensor of the block -> an epilogue of the producing Linear / Conv, pass 3).
    // OAR_FUSE_GELU=0 keeps the op-by-op path.
    void pass_2b_gelu() {
        const bool fuse = switch_on("OAR_FUSE_GELU");
        scan();
        auto scalar_of = [&](const std::string& v, float& out) {
            auto it = inits.find(v);
            if (it == inits.end() || it->second.dtype != DType::F32 || it->second.f.size() != 1) return false;
            out = it->second.f[0];
            return true;
        };
        auto single_use = [&](const std::string& v) { return cons[v].size() == 1 && !graph_outs.count(v); };
        // node `i` is op(x, c) or op(c, x) with a scalar constant close to `want`: returns x's name
        auto scaled = [&](int i, const char* op, float want, bool commutes, std::string& x) {
            const GNode& q = nodes[i];
            if (q.op != op || q.in.size() != 2) return false;
            float c;
            if (scalar_of(q.in[1], c) && std::fabs(c - want) <= 1e-4f * std::fabs(want)) { x = q.in[0]; return true; }
            if (commutes && scalar_of(q.in[0], c) && std::fabs(c - want) <= 1e-4f * std::fabs(want)) { x = q.in[1]; return true; }
            return false;
        };
        for (int i = 0; fuse && i < (int)nodes.size(); ++i) {
            if (nodes[i].op != "Erf" || dead[i] || !single_use(nodes[i].out[0])) continue;
            auto pit = producer.find(nodes[i].in[0]);
            if (pit == producer.end() || dead[pit->second] || !single_use(nodes[i].in[0])) continue;
            const int pre = pit->second;
            std::string x;
            if (!scaled(pre, "Div", 1.41421356f, false, x) && !scaled(pre, "Mul", 0.70710678f, true, x)) continue;
            const int add = cons[nodes[i].out[0]][0];
            std::string e1;
            if (dead[add] || !scaled(add, "Add", 1.0f, true, e1) || e1 != nodes[i].out[0] || !single_use(nodes[add].out[0])) continue;
            const int m1 = cons[nodes[add].out[0]][0];
            if (dead[m1] || nodes[m1].op != "Mul" || nodes[m1].in.size() != 2) continue;
            const std::string other = nodes[m1].in[0] == nodes[add].out[0] ? nodes[m1].in[1] : nodes[m1].in[0];
            int last = -1, half = -1;
            if (other == x) {   // (x * (1 + erf)) * 0.5
                if (!single_use(nodes[m1].out[0])) continue;
                const int m2 = cons[nodes[m1].out[0]][0];
                std::string t;
                if (dead[m2] || !scaled(m2, "Mul", 0.5f, true, t) || t != nodes[m1].out[0]) continue;
                last = m2;
            } else {            // (x * 0.5) * (1 + erf)
                auto hit = producer.find(other);
                std::string t;
                if (hit == producer.end() || dead[hit->second] || !single_use(other) || !scaled(hit->second, "Mul", 0.5f, true, t) || t != x) continue;
                half = hit->second;
                last = m1;
            }
            GNode ge;
            ge.op = "Gelu"; ge.in = {x}; ge.out = {nodes[last].out[0]};
            for (int d : {pre, i, add, m1}) dead[d] = true;
            if (half >= 0) dead[half] = true;
            dead[last] = false;
            nodes[last] = std::move(ge);   // the last node of the pattern: every reader comes after it
        }
        sweep();
    }

    // ---- pass 2c: LayerNorm over the last axis as exporters below opset 17 spell it:
    //   m = ReduceMean(x, [a], keepdims 1);  d = Sub(x, m);  v = ReduceMean(Pow(d, 2) | Mul(d, d), [a], keepdims 1);  r = Sqrt(Add(v, eps))
    //   y = Div(d, r)  |  Mul(d, Reciprocal(r))  |  Mul(d, Div(1, r))        [-> Mul(y, gamma [C]) [-> Add(., beta [C])]]
    // becomes ONE LayerNormalization node (nine launches that pass the tensor through HBM about seven times -> one), so that an opset-13 and an opset-17 export
    // of the same block meet the same later passes.  Axes as an attribute or a constant input; Add and the Muls in either order; eps a positive f32 constant of
    // one element; gamma / beta f32 initializers of [C] or [1, .., 1, C], each folded only when the value in front of it has that single reader.  m, v, the
    // squares, the Add and the Sqrt must have one reader each, d exactly the square and the quotient, none a graph output.  a = -1 or a >= 0: the rank of x
    // is unknown here, so the replaced nodes are kept (ln_spelled) and op_layernorm plans them instead when a turns out not to be the last axis (or x has
    // rank 1, or gamma / beta do not have x's last extent).  Anything else stays as it is.  OAR_FUSE_LAYERNORM=0 keeps the op-by-op route.
    void pass_2c_layernorm() {
        const bool fuse = switch_on("OAR_FUSE_LAYERNORM");
        scan();
        auto single_use = [&](const std::string& v) { return cons[v].size() == 1 && !graph_outs.count(v); };
        auto reader = [&](const std::string& v, const char* op) -> int {   // the only reader of v, a live two-input `op` (or -1)
            if (!single_use(v)) return -1;
            const int c = cons[v][0];
            return !dead[c] && nodes[c].op == op ? c : -1;
        };
        auto scalar_is = [&](const std::string& v, float want) {
            auto it = inits.find(v);
            if (it == inits.end()) return false;
            const HostTensor& t = it->second;
            return t.dtype == DType::F32 ? (t.f.size() == 1 && t.f[0] == want) : (t.i.size() == 1 && (float)t.i[0] == want);
        };
        auto mean_axis = [&](const GNode& q, int64_t& ax) {   // ReduceMean over ONE axis, keepdims 1
            if (q.op != "ReduceMean" || q.in.empty() || q.ai("keepdims", 1) != 1) return false;
            std::vector<int64_t> a;
            if (q.in.size() > 1 && !q.in[1].empty()) {
                auto it = inits.find(q.in[1]);
                if (it == inits.end() || it->second.dtype == DType::F32) return false;
                a = it->second.i;
            } else {
                a = q.ais("axes");
            }
            if (a.size() != 1 || a[0] < -1) return false;
            ax = a[0];
            return true;
        };
        auto affine_vec = [&](const std::string& v) -> int64_t {   // elements of an f32 initializer shaped [C] or [1, .., 1, C]; 0: not one
            auto it = inits.find(v);
            if (it == inits.end() || it->second.dtype != DType::F32 || it->second.dims.empty()) return 0;
            const int64_t c = it->second.dims.back();
            return c > 0 && numel(it->second.dims) == c && (int64_t)it->second.f.size() == c ? c : 0;
        };
        for (int i = 0; fuse && i < (int)nodes.size(); ++i) {
            const GNode& sub = nodes[i];
            if (sub.op != "Sub" || dead[i] || sub.in.size() != 2) continue;
            const std::string x = sub.in[0], m = sub.in[1], d = sub.out[0];
            auto mp = producer.find(m);
            if (mp == producer.end() || dead[mp->second] || !single_use(m)) continue;
            const int rm1 = mp->second;
            int64_t ax1 = 0, ax2 = 0;
            if (!mean_axis(nodes[rm1], ax1) || nodes[rm1].in[0] != x) continue;
            // d: read by the square and by the quotient, by nothing else
            if (graph_outs.count(d)) continue;
            std::set<int> dr(cons[d].begin(), cons[d].end());
            if (dr.size() != 2) continue;
            int sq = -1, fin = -1;
            for (int c : dr) {
                const GNode& q = nodes[c];
                if (dead[c] || q.in.size() != 2) continue;
                if ((q.op == "Pow" && q.in[0] == d && scalar_is(q.in[1], 2.0f)) || (q.op == "Mul" && q.in[0] == d && q.in[1] == d)) sq = c;
            }
            if (sq < 0) continue;
            for (int c : dr) if (c != sq) fin = c;
            if ((int)cons[d].size() != (nodes[sq].op == "Mul" ? 3 : 2) || dead[fin]) continue;
            const int rm2 = reader(nodes[sq].out[0], "ReduceMean");
            if (rm2 < 0 || !mean_axis(nodes[rm2], ax2)) continue;
            // the same axis: written the same way, or -1 on one ReduceMean and a number k >= 0 on the other -- then k is kept, and op_layernorm, which knows the
            // rank, takes the node only where k is the last axis (which is what -1 says)
            if (ax2 != ax1) {
                if (std::min(ax1, ax2) != -1 || std::max(ax1, ax2) < 0) continue;
                ax1 = std::max(ax1, ax2);
            }
            const std::string& v = nodes[rm2].out[0];
            const int add = reader(v, "Add");
            if (add < 0 || nodes[add].in.size() != 2) continue;
            const std::string& epsn = nodes[add].in[0] == v ? nodes[add].in[1] : nodes[add].in[0];
            auto ei = inits.find(epsn);
            if (ei == inits.end() || ei->second.dtype != DType::F32 || ei->second.f.size() != 1 || ei->second.dims.size() > 1 || !(ei->second.f[0] > 0.0f)) continue;
            const float eps = ei->second.f[0];
            const int sqr = reader(nodes[add].out[0], "Sqrt");
            if (sqr < 0) continue;
            const std::string& r = nodes[sqr].out[0];
            if (!single_use(r) || dead[cons[r][0]]) continue;
            int inv = -1;   // Reciprocal(r) or Div(1, r) between the root and the product
            const GNode& f = nodes[fin];
            if (f.in.size() != 2) continue;
            if (cons[r][0] == fin) {
                if (!(f.op == "Div" && f.in[0] == d && f.in[1] == r)) continue;
            } else {
                inv = cons[r][0];
                const GNode& q = nodes[inv];
                const bool recip = (q.op == "Reciprocal" && q.in.size() == 1) || (q.op == "Div" && q.in.size() == 2 && q.in[1] == r && scalar_is(q.in[0], 1.0f));
                if (!recip || !single_use(q.out[0]) || cons[q.out[0]][0] != fin || f.op != "Mul") continue;
                if (!((f.in[0] == d && f.in[1] == q.out[0]) || (f.in[1] == d && f.in[0] == q.out[0]))) continue;
            }
            std::vector<int> parts = {rm1, i, sq, rm2, add, sqr, fin};
            if (inv >= 0) parts.push_back(inv);
            int last = fin;
            std::string gamma, beta;
            int64_t cg = 0;
            if (const int mu = reader(nodes[last].out[0], "Mul"); mu >= 0 && nodes[mu].in.size() == 2) {
                const std::string& o = nodes[mu].in[0] == nodes[last].out[0] ? nodes[mu].in[1] : nodes[mu].in[0];
                if ((cg = affine_vec(o)) > 0) { gamma = o; parts.push_back(mu); last = mu; }
            }
            if (const int ad = reader(nodes[last].out[0], "Add"); ad >= 0 && nodes[ad].in.size() == 2) {
                const std::string& o = nodes[ad].in[0] == nodes[last].out[0] ? nodes[ad].in[1] : nodes[ad].in[0];
                const int64_t cb = affine_vec(o);
                if (cb > 0 && (gamma.empty() || cb == cg)) { beta = o; parts.push_back(ad); last = ad; }
            }
            std::sort(parts.begin(), parts.end());
            GNode ln;
            ln.op = "LayerNormalization";
            ln.in = {x};
            if (!gamma.empty() || !beta.empty()) ln.in.push_back(gamma);
            if (!beta.empty()) ln.in.push_back(beta);
            ln.out = {nodes[last].out[0]};
            { Attr a; a.kind = Attr::I; a.i = ax1; ln.attrs["axis"] = a; }
            { Attr a; a.kind = Attr::F; a.f = eps; ln.attrs["epsilon"] = a; }
            std::vector<GNode>& spelled = ln_spelled[ln.out[0]];
            for (int p : parts) { spelled.push_back(nodes[p]); dead[p] = true; }
            dead[last] = false;
            nodes[last] = std::move(ln);   // the last node of the pattern: x is computed in front of it and every reader comes after it
        }
        sweep();
    }

    // ---- pass 3: fuse activations into Conv / ConvTranspose / Linear / Gemm / Add
    void pass_3_activations() {
        bool changed = true;
        while (changed) {
            changed = false;
            scan();
            for (int i = 0; i < (int)nodes.size(); ++i) {
                GNode& p = nodes[i];
                if (!(p.op == "Conv" || p.op == "ConvTranspose" || p.op == "Linear" || p.op == "Gemm" || p.op == "Add")) continue;
                if (p.act.kind != k::ACT_NONE) continue;
                const std::string& y = p.out[0];
                if (graph_outs.count(y)) continue;
                auto& cs = cons[y];
                if (cs.size() == 1 && is_fusable_act(nodes[cs[0]].op) && !dead[cs[0]] &&
                    !(nodes[cs[0]].op == "Gelu" && nodes[cs[0]].as("approximate", "none") == "tanh")) {   // (the tanh form only exists in the stand-alone kernel)
                    GNode& a = nodes[cs[0]];
                    p.act = act_of(a);
                    p.out[0] = a.out[0];
                    dead[cs[0]] = true;
                    changed = true;
                    continue;
                }
                if (cs.size() == 2) {
                    // x * HardSigmoid(x) (alpha 1/6, beta .5) = HardSwish ; x * Sigmoid(x) = Swish
                    for (int t = 0; t < 2; ++t) {
                        GNode& g = nodes[cs[t]];
                        GNode& mul = nodes[cs[1 - t]];
                        if (dead[cs[0]] || dead[cs[1]]) break;
                        if (!(g.op == "HardSigmoid" || g.op == "Sigmoid") || mul.op != "Mul") continue;
                        if (graph_outs.count(g.out[0]) || cons[g.out[0]].size() != 1 || cons[g.out[0]][0] != cs[1 - t]) continue;
                        bool ok = (mul.in[0] == y && mul.in[1] == g.out[0]) || (mul.in[1] == y && mul.in[0] == g.out[0]);
                        if (!ok) continue;
                        if (g.op == "HardSigmoid") {
                            float al = g.af("alpha", 0.2f), be = g.af("beta", 0.5f);
                            if (std::fabs(al - 1.0f / 6.0f) > 1e-6f || std::fabs(be - 0.5f) > 1e-6f) continue;
                            p.act.kind = k::ACT_HSWISH;
                        } else {
                            p.act.kind = k::ACT_SWISH;
                        }
                        p.out[0] = mul.out[0];
                        dead[cs[0]] = dead[cs[1]] = true;
                        changed = true;
                        break;
                    }
                }
            }
            sweep();
        }
    }

    // ---- pass 3b: the attention of a Swin block (UniMERNet's encoder), y [B, H W, C] with static H, W, ws, N = ws^2:
    //   p = Reshape(y, [0, H/ws, ws, W/ws, ws, C]) -> Transpose[0,1,3,2,4,5] -> Reshape[-1, N, C]                     (window partition)
    //   q, k, v = Linear(p);  qh, kh, vh = Transpose[0,2,1,3](Reshape(., [0, N, nh, dh]))
    //   a = Softmax(Add(Div(MatMul(qh, Transpose[0,1,3,2](kh)), c) | Mul(.., c), bias [1, nh, N, N]), -1)
    //   o = Linear(Reshape(Transpose[0,2,1,3](MatMul(a, vh)), [0, N, C]))
    //   r = Reshape(o, [-1, H/ws, W/ws, ws, ws, C]) -> Transpose[0,1,3,2,4,5] -> Reshape[-1, H W, C]                    (window reverse)
    // A Linear is per token, so the partition commutes with it: q, k, v read y in image order, ONE WindowAttention node (csrc/window_attention.hip) gathers and
    // scatters a window's tokens by address, the projection runs on its output, and both the partition and the reverse triple leave the graph (18
    // launches per block, four of them rank-6 copies of the whole token tensor, become 6).  Every intermediate must be single-use and no graph output.  It runs before
    // pass 4 so that the block's residual Add folds into the projection.  OAR_FUSE_WINDOW_ATTENTION=0, a shape k::window_attention_supported rejects (every
    // size is static here, so that is known at load time) keep the op-by-op route.
    // The padded, shifted and masked spellings are matched too, each independently of the others; with Hp = hb ws, Wp = wb ws:
    //   front:  g = Reshape(y, [0, H, W, C]) -> Pad(g, [0,0,0,0, 0,Hp-H,Wp-W,0], constant 0) -> roll by -s on axis 1, then on axis 2, each
    //           Concat(Slice(g, s:end), Slice(g, 0:s)) -> the partition's Reshape
    //   mask:   Add(.., bias) -> Reshape[-1, nW, nh, N, N] -> Add(mask [1, nW, 1, N, N]) -> Reshape[-1, nh, N, N] -> Softmax, nW = hb wb
    //   tail:   the reverse's last Reshape gives [-1, Hp, Wp, C] -> roll by +s (Concat(Slice(r, Hp-s:end), Slice(r, 0:Hp-s)); axis 2 with Wp) ->
    //           Slice(0:H, axis 1), Slice(0:W, axis 2) where that axis is padded -> Reshape[0, H W, C]
    // All of it is address arithmetic in the kernel (k::window_token_row): the node gets shift / Hp / Wp, the mask as a fifth input and, where the block pads,
    // the k and v Linears' biases (a padded token reaches them as zeros).  A Pad with another value, mode or side, a reverse roll that is not the inverse of
    // the forward one, a mask with another window count and a dynamic H / W are not matched and keep the op-by-op route.
    void pass_3b_window_attention() {
        const bool fuse = switch_on("OAR_FUSE_WINDOW_ATTENTION");
        scan();
        struct Sl { std::string src; int64_t ax, st, en; };
        auto slice1 = [&](int idx, Sl& o) {   // a single-axis unit-step Slice with constant non-negative operands
            const GNode& sl = nodes[idx];
            if (sl.op != "Slice" || sl.in.size() < 4 || sl.in.size() > 5) return false;
            const V st = ints(sl.in[1]), en = ints(sl.in[2]), ax = ints(sl.in[3]);
            if (st.size() != 1 || en.size() != 1 || ax.size() != 1 || st[0] < 0 || en[0] < 0 || ax[0] < 0) return false;
            if (sl.in.size() == 5 && !sl.in[4].empty() && ints(sl.in[4]) != V{1}) return false;
            o = Sl{sl.in[0], ax[0], st[0], en[0]};
            return true;
        };
        // Concat(Slice(src, k:end), Slice(src, 0:k)) on `axis` of extent n, 0 < k < n: roll(src, -k).  src is read by the two Slices alone, each of them by the Concat alone.
        auto roll = [&](int c, int64_t axis, int64_t n, std::string& src, int64_t& by, int* sl) {
            const GNode& cc = nodes[c];
            if (cc.op != "Concat" || cc.in.size() != 2 || cc.ai("axis", 0) != axis || cc.act.kind != k::ACT_NONE) return false;
            Sl a[2];
            for (int t = 0; t < 2; ++t) {
                sl[t] = prod1(cc.in[t], "Slice");
                if (sl[t] < 0 || !slice1(sl[t], a[t]) || a[t].ax != axis) return false;
            }
            if (a[0].src != a[1].src || a[1].st != 0 || a[0].st != a[1].en || a[0].st <= 0 || a[0].st >= n || a[0].en < n) return false;
            if (cons[a[0].src].size() != 2 || graph_outs.count(a[0].src)) return false;
            src = a[0].src; by = a[0].st;
            return true;
        };
        auto roll_of = [&](const std::string& v, int64_t axis, int64_t n, int64_t want, int* sl) -> int {   // the Concat of roll(v, -want), or -1
            if (cons[v].size() != 2 || graph_outs.count(v)) return -1;
            const int a = cons[v][0];
            if (dead[a] || nodes[a].op != "Slice" || !single_use(nodes[a].out[0])) return -1;
            const int c = cons[nodes[a].out[0]][0];
            std::string src; int64_t by = 0;
            return !dead[c] && roll(c, axis, n, src, by, sl) && src == v && by == want ? c : -1;
        };
        auto plain_linear = [&](const GNode& l, int64_t C) {
            if (l.op != "Linear" || l.act.kind != k::ACT_NONE || !l.residual.empty() || l.in.size() < 2 || !is_init(l.in[1])) return false;
            const HostTensor& w = inits[l.in[1]];
            return w.dims.size() == 2 && w.dims[0] == C && w.dims[1] == C;
        };
        for (int i = 0; fuse && i < (int)nodes.size(); ++i) {
            if (nodes[i].op != "Softmax" || dead[i]) continue;
            const GNode& sm = nodes[i];
            const int64_t sax = sm.ai("axis", -1);
            if (sax != -1 && sax != 3) continue;
            // the per-window mask, where there is one: Reshape[-1, nW, nh, N, N] -> Add(mask [1, nW, 1, N, N]) -> Reshape[-1, nh, N, N]
            std::string sv = sm.in[0], maskn;
            int m1 = -1, m2 = -1;
            const int m3 = prodn(sv, "Reshape");
            if (m3 >= 0) {
                if (!single_use(sv)) continue;
                m2 = prod1(nodes[m3].in[0], "Add");
                if (m2 < 0) continue;
                const int mi = is_init(nodes[m2].in[1]) ? 1 : is_init(nodes[m2].in[0]) ? 0 : -1;
                if (mi < 0) continue;
                maskn = nodes[m2].in[mi];
                const HostTensor& mk = inits[maskn];
                if (mk.dtype != DType::F32 || mk.dims.size() != 5 || mk.dims[0] != 1 || mk.dims[2] != 1 || mk.dims[3] != mk.dims[4] || (int64_t)mk.f.size() != numel(mk.dims)) continue;
                m1 = prod1(nodes[m2].in[1 - mi], "Reshape");
                if (m1 < 0) continue;
                sv = nodes[m1].in[0];
            }
            // scores: Add(scaled, bias) in either order, scaled = Div(MatMul, c) or Mul(MatMul, c) / Mul(c, MatMul)
            const int ad = prod1(sv, "Add");
            if (ad < 0 || !single_use(sm.out[0])) continue;
            const int bi = is_init(nodes[ad].in[1]) ? 1 : is_init(nodes[ad].in[0]) ? 0 : -1;
            if (bi < 0) continue;
            const HostTensor& bias = inits[nodes[ad].in[bi]];
            if (bias.dtype != DType::F32 || bias.dims.size() != 4 || bias.dims[0] != 1 || bias.dims[2] != bias.dims[3] || (int64_t)bias.f.size() != numel(bias.dims)) continue;
            const int64_t nh = bias.dims[1], N = bias.dims[2];
            int64_t nWm = 0;
            if (m3 >= 0) {
                const HostTensor& mk = inits[maskn];
                nWm = mk.dims[1];
                if (mk.dims[3] != N || target(m3) != V{-1, nh, N, N} || target(m1) != V{-1, nWm, nh, N, N}) continue;
            }
            const std::string& scaled = nodes[ad].in[1 - bi];
            int sc = prod1(scaled, "Div"), scale_div = 1, ci = 1;
            if (sc < 0) { sc = prod1(scaled, "Mul"); scale_div = 0; if (sc >= 0) ci = is_init(nodes[sc].in[1]) ? 1 : 0; }
            if (sc < 0) continue;
            const HostTensor* sct = f32_scalar(nodes[sc].in[ci]);
            if (!sct) continue;
            const int mm1 = prod1(nodes[sc].in[1 - ci], "MatMul");
            if (mm1 < 0) continue;
            const int mm2 = reader1(sm.out[0], "MatMul");
            if (mm2 < 0) continue;
            // heads: Transpose[0,2,1,3](Reshape(Linear, [0, N, nh, dh])), the keys once more through Transpose[0,1,3,2]
            const int tk = prod1(nodes[mm1].in[1], "Transpose");
            if (tk < 0 || !perm_is(tk, {0, 1, 3, 2})) continue;
            int64_t dh = 0;
            int tr[3], rs[3], ln[3];
            const std::string* hv[3] = {&nodes[mm1].in[0], &nodes[tk].in[0], &nodes[mm2].in[1]};
            bool ok = true;
            for (int t = 0; t < 3 && ok; ++t) {
                tr[t] = prod1(*hv[t], "Transpose");
                ok = tr[t] >= 0 && perm_is(tr[t], {0, 2, 1, 3});
                if (!ok) break;
                rs[t] = prod1(nodes[tr[t]].in[0], "Reshape");
                ok = rs[t] >= 0;
                if (!ok) break;
                const V tg = target(rs[t]);
                ok = tg.size() == 4 && tg[0] == 0 && tg[1] == N && tg[2] == nh && tg[3] > 0 && (dh == 0 || tg[3] == dh);
                if (!ok) break;
                dh = tg[3];
                ln[t] = prod1(nodes[rs[t]].in[0], "Linear");
                ok = ln[t] >= 0 && plain_linear(nodes[ln[t]], nh * dh);
            }
            if (!ok || ln[0] == ln[1] || ln[0] == ln[2] || ln[1] == ln[2]) continue;
            const int64_t C = nh * dh;
            // window partition: the three projections are the only readers of p
            const std::string pv = nodes[ln[0]].in[0];
            if (nodes[ln[1]].in[0] != pv || nodes[ln[2]].in[0] != pv || cons[pv].size() != 3 || graph_outs.count(pv)) continue;
            const int p3 = prodn(pv, "Reshape");
            if (p3 < 0 || target(p3) != V{-1, N, C}) continue;
            const int p2 = prod1(nodes[p3].in[0], "Transpose");
            if (p2 < 0 || !perm_is(p2, {0, 1, 3, 2, 4, 5})) continue;
            const int p1 = prod1(nodes[p2].in[0], "Reshape");
            if (p1 < 0) continue;
            const V pt = target(p1);
            if (pt.size() != 6 || pt[0] != 0 || pt[1] <= 0 || pt[2] <= 0 || pt[3] <= 0 || pt[4] != pt[2] || pt[5] != C || pt[2] * pt[2] != N) continue;
            const int64_t hb = pt[1], ws = pt[2], wb = pt[3], Hp = hb * ws, Wp = wb * ws;
            if (!k::window_attention_supported((int)std::min<int64_t>(ws, 1 << 20), (int)std::min<int64_t>(nh, 1 << 20), (int)std::min<int64_t>(dh, 1 << 20))) continue;
            if (Hp >= (int64_t)1 << 30 || Wp >= (int64_t)1 << 30 || (m3 >= 0 && nWm != hb * wb)) continue;
            // output side: Transpose[0,2,1,3] -> Reshape[0, N, C] -> Linear -> window reverse
            const int t2 = reader1(nodes[mm2].out[0], "Transpose");
            if (t2 < 0 || !perm_is(t2, {0, 2, 1, 3})) continue;
            const int r2 = reader1(nodes[t2].out[0], "Reshape");
            if (r2 < 0 || target(r2) != V{0, N, C}) continue;
            const int pj = reader1(nodes[r2].out[0], "Linear");
            if (pj < 0 || !plain_linear(nodes[pj], C)) continue;
            const int v1 = reader1(nodes[pj].out[0], "Reshape");
            if (v1 < 0 || target(v1) != V{-1, hb, wb, ws, ws, C}) continue;
            const int v2 = reader1(nodes[v1].out[0], "Transpose");
            if (v2 < 0 || !perm_is(v2, {0, 1, 3, 2, 4, 5})) continue;
            const int v3 = reader1(nodes[v2].out[0], "Reshape");
            if (v3 < 0) continue;
            // the reverse ends in [-1, Hp Wp, C]: the plain block, y feeds the partition.  It ends in [-1, Hp, Wp, C]: the tokens are handled as a grid, with
            // Reshape[0, H, W, C] -> Pad (bottom / right, constant 0) -> roll by -s on axis 1, then on axis 2 in front of the partition, Pad and roll each optional
            const bool grid = target(v3) == V{-1, Hp, Wp, C};
            if (!grid && target(v3) != V{-1, Hp * Wp, C}) continue;
            std::vector<int> extra;
            std::string cur = nodes[p1].in[0];
            int64_t shift = 0, H = Hp, W = Wp;
            if (grid) {
                bool counted = false;                // cur's readers are already known to be the two Slices of a roll
                if (const int c2 = prodn(cur, "Concat"); c2 >= 0) {
                    std::string s2, s1;
                    int64_t k2 = 0, k1 = 0;
                    int sa[2], sb[2];
                    if (!single_use(cur) || !roll(c2, 2, Wp, s2, k2, sa)) continue;
                    const int c1 = prodn(s2, "Concat");
                    if (c1 < 0 || !roll(c1, 1, Hp, s1, k1, sb) || k1 != k2) continue;
                    shift = k1; cur = s1; counted = true;
                    extra.insert(extra.end(), {c2, c1, sa[0], sa[1], sb[0], sb[1]});
                }
                if (const int pd = prodn(cur, "Pad"); pd >= 0) {
                    const GNode& pn = nodes[pd];
                    if (!(counted || single_use(cur)) || pn.as("mode", "constant") != "constant" || pn.in.size() < 2 || pn.in.size() > 3) continue;
                    const V pads = ints(pn.in[1]);
                    if (pads.size() != 8 || pads[0] || pads[1] || pads[2] || pads[3] || pads[4] || pads[7] || pads[5] < 0 || pads[6] < 0 || pads[5] >= ws || pads[6] >= ws) continue;
                    if (pn.in.size() == 3 && !pn.in[2].empty()) {
                        const HostTensor* pv0 = f32_scalar(pn.in[2]);
                        if (!pv0 || pv0->f[0] != 0.0f) continue;
                    }
                    H = Hp - pads[5]; W = Wp - pads[6];
                    cur = pn.in[0]; counted = false;
                    extra.push_back(pd);
                }
                const int fr = prodn(cur, "Reshape");
                if (fr < 0 || !(counted || single_use(cur)) || target(fr) != V{0, H, W, C}) continue;   // (constants: a dynamic H / W is not matched)
                cur = nodes[fr].in[0];
                extra.push_back(fr);
            }
            const std::string y = cur;
            std::string out = nodes[v3].out[0];
            if (grid) {   // behind the reverse: roll by +s (the exact inverse of the forward one) -> crop -> Reshape[0, H W, C]
                bool ok2 = true;
                if (shift > 0) {
                    int sa[2], sb[2];
                    const int c1 = roll_of(out, 1, Hp, Hp - shift, sa);
                    const int c2 = c1 < 0 ? -1 : roll_of(nodes[c1].out[0], 2, Wp, Wp - shift, sb);
                    ok2 = c2 >= 0;
                    if (ok2) { out = nodes[c2].out[0]; extra.insert(extra.end(), {c1, c2, sa[0], sa[1], sb[0], sb[1]}); }
                }
                for (int ax = 1; ax <= 2 && ok2; ++ax) {
                    if ((ax == 1 ? Hp - H : Wp - W) == 0) continue;
                    const int cr = reader1(out, "Slice");
                    Sl c;
                    ok2 = cr >= 0 && slice1(cr, c) && c.ax == ax && c.st == 0 && c.en == (ax == 1 ? H : W);
                    if (ok2) { out = nodes[cr].out[0]; extra.push_back(cr); }
                }
                if (!ok2) continue;
                const int fin = reader1(out, "Reshape");
                if (fin < 0) continue;
                const V ft = target(fin);
                if (ft != V{0, H * W, C} && ft != V{-1, H * W, C}) continue;
                out = nodes[fin].out[0];
                extra.push_back(fin);
            }
            GNode wa;
            wa.op = "WindowAttention";
            wa.in = {nodes[ln[0]].out[0], nodes[ln[1]].out[0], nodes[ln[2]].out[0], nodes[ad].in[bi]};
            if (m3 >= 0 || Hp != H || Wp != W) {   // the mask, and what a padded token becomes behind the k and v Linears: their biases
                const bool pads = Hp != H || Wp != W;
                wa.in.insert(wa.in.end(), {maskn, pads ? nodes[ln[1]].bias : std::string(), pads ? nodes[ln[2]].bias : std::string()});
            }
            wa.out = {nodes[r2].out[0]};
            iattr(wa, "ws", ws); iattr(wa, "H", H); iattr(wa, "W", W); iattr(wa, "Hp", Hp); iattr(wa, "Wp", Wp); iattr(wa, "shift", shift); iattr(wa, "heads", nh); iattr(wa, "head_dim", dh); iattr(wa, "scale_div", scale_div);
            fattr(wa, "scale", sct->f[0]);
            for (int t = 0; t < 3; ++t) nodes[ln[t]].in[0] = y;
            nodes[pj].out[0] = out;
            for (int d : {p1, p2, p3, rs[0], rs[1], rs[2], tr[0], tr[1], tr[2], tk, mm1, sc, ad, i, mm2, t2, v1, v2, v3}) dead[d] = true;
            for (int d : extra) dead[d] = true;
            for (int d : {m1, m2, m3}) if (d >= 0) dead[d] = true;
            nodes[r2] = std::move(wa);   // behind q, k and v, in front of the projection
        }
        sweep();
    }

    // ---- pass 3d: the attention of a SAM / Vary ViT block with the decomposed relative-position bias (the encoder of the larger PP-FormulaNet files; DESIGN
    //   4.35), y [B, H W, C] with static H, W; (h, w) = (H, W) for global attention, (ws, ws) for windows; N = h w, G = B (windows) nh:
    //   g = Reshape(y, [0, H, W, C]);   windows: [Pad(g, bottom / right, constant 0) ->] Reshape[0, Hp/ws, ws, Wp/ws, ws, C] -> Transpose[0,1,3,2,4,5] -> Reshape[-1, ws, ws, C]
    //   qkv = Linear(Reshape(g, [0, N, C]), [C, 3 C]) -> Reshape[0, -1, 3, nh, dh] -> Transpose[2,0,3,1,4] -> Reshape[3, -1, N, dh] -> Split(axis 0) -> 3 x Squeeze[0]
    //   s = MatMul(Mul(q, c), Transpose[0,2,1](k))   or   Mul(MatMul(q, Transpose[0,2,1](k)), c)
    //   rq = Reshape(q, [0, h, w, dh])                                                          (the UNSCALED q: the Squeeze's output itself)
    //   rh = Transpose[1,0,2,3](Reshape(MatMul(Reshape(Transpose[1,0,2,3](rq), [h, -1, dh]), RhT [h, dh, h]), [h, -1, w, h]))
    //   rw = Transpose[1,2,0,3](Reshape(MatMul(Reshape(Transpose[2,0,1,3](rq), [w, -1, dh]), RwT [w, dh, w]), [w, -1, h, w]))
    //   a = Softmax(Reshape(Add(Add(Reshape(s, [0, h, w, h, w]), Unsqueeze(rh, -1)), Unsqueeze(rw, -2)), [0, N, N]), -1)
    //   o = Linear(Reshape(Transpose[0,2,3,1,4](Reshape(MatMul(a, v), [-1, nh, h, w, dh])), [0, N, C]))
    //   windows: Reshape[-1, Hp/ws, Wp/ws, ws, ws, C] -> Transpose[0,1,3,2,4,5] -> Reshape[-1, Hp, Wp, C] -> Slice(0:H, axis 1), Slice(0:W, axis 2) where padded;
    //   Reshape(o, [0, H W, C])
    // becomes the fused Linear on y in image order, ONE RelPosAttention node (csrc/relpos_attention.hip) and the projection: the pad, partition, reverse, crop
    // and the whole score / bias subgraph leave the graph.  The match is exact, operand order included: RhT or RwT that is no initializer, a rel term taken
    // from the scaled q, an intermediate with a second reader (or that is a graph output), another permutation or target, a Pad with another value, mode or
    // side and a shape k::relpos_attention_supported rejects keep the op-by-op route.  The pass is opt-in: OAR_FUSE_RELPOS_ATTENTION=1, read at load time, turns
    // it on; unset or 0 keeps the op-by-op route.  It runs before pass 4 so that the
    // block's residual Add folds into the projection.
    void pass_3d_relpos_attention() {
        const char* fe = getenv("OAR_FUSE_RELPOS_ATTENTION");
        const bool fuse = fe && atoi(fe) != 0;           // opt-in until the three-arm speed measurement of DESIGN 4.35 exists: unset or 0 keeps the op-by-op route
        scan();
        auto table = [&](const std::string& v, int64_t n, int64_t dh) {  // a constant f32 [n, dh, n]
            auto it = inits.find(v);
            return it != inits.end() && it->second.dtype == DType::F32 && it->second.dims == V{n, dh, n} && (int64_t)it->second.f.size() == n * dh * n;
        };
        auto slice01 = [&](int idx, int64_t ax, int64_t en) {            // Slice(0 : en) on `ax`, unit step, constant operands
            const GNode& sl = nodes[idx];
            if (sl.in.size() < 4 || sl.in.size() > 5 || ints(sl.in[1]) != V{0} || ints(sl.in[2]) != V{en} || ints(sl.in[3]) != V{ax}) return false;
            return sl.in.size() == 4 || sl.in[4].empty() || ints(sl.in[4]) == V{1};
        };
        for (int i = 0; fuse && i < (int)nodes.size(); ++i) {
            if (nodes[i].op != "Softmax" || dead[i]) continue;
            const int64_t sax = nodes[i].ai("axis", -1);
            if (sax != -1 && sax != 2) continue;
            // scores: Reshape[0, N, N](Add(Add(Reshape(s, [0, h, w, h, w]), Unsqueeze(rh, -1)), Unsqueeze(rw, -2)))
            const int ra = prod1(nodes[i].in[0], "Reshape");
            if (ra < 0) continue;
            const V ta = target(ra);
            if (ta.size() != 3 || ta[0] != 0 || ta[1] < 1 || ta[1] != ta[2]) continue;
            const int64_t N = ta[1];
            const int a2 = prod1(nodes[ra].in[0], "Add");
            if (a2 < 0 || nodes[a2].in.size() != 2) continue;
            const int a1 = prod1(nodes[a2].in[0], "Add"), uw = prod1(nodes[a2].in[1], "Unsqueeze");
            if (a1 < 0 || uw < 0 || nodes[a1].in.size() != 2 || !axes_are(uw, 3, 5)) continue;
            const int s5 = prod1(nodes[a1].in[0], "Reshape"), uh = prod1(nodes[a1].in[1], "Unsqueeze");
            if (s5 < 0 || uh < 0 || !axes_are(uh, 4, 5)) continue;
            const V t5 = target(s5);
            if (t5.size() != 5 || t5[0] != 0 || t5[1] < 1 || t5[2] < 1 || t5[3] != t5[1] || t5[4] != t5[2] || t5[1] > (1 << 20) || t5[2] > (1 << 20) || t5[1] * t5[2] != N) continue;
            const int64_t h = t5[1], w = t5[2];
            // the scale, where the graph has it: on q in front of the product, or on the product
            const std::string& sv = nodes[s5].in[0];
            int mul = prod1(sv, "Mul"), mm1 = -1, scale_pre = 0;
            if (mul >= 0) {
                mm1 = prod1(nodes[mul].in[0], "MatMul");
            } else {
                mm1 = prod1(sv, "MatMul");
                mul = mm1 < 0 ? -1 : prod1(nodes[mm1].in[0], "Mul");
                scale_pre = 1;
            }
            if (mm1 < 0 || mul < 0 || nodes[mul].in.size() != 2 || nodes[mm1].in.size() != 2) continue;
            const HostTensor* sct = f32_scalar(nodes[mul].in[1]);
            if (!sct) continue;
            const std::string qn = scale_pre ? nodes[mul].in[0] : nodes[mm1].in[0];   // the unscaled q
            const int tk = prod1(nodes[mm1].in[1], "Transpose");
            if (tk < 0 || !perm_is(tk, {0, 2, 1})) continue;
            const int mm2 = reader1(nodes[i].out[0], "MatMul");
            if (mm2 < 0 || nodes[mm2].in.size() != 2) continue;
            // q, k, v: Squeeze[0] of the three outputs of Split(axis 0) of Reshape[3, -1, N, dh](Transpose[2,0,3,1,4](Reshape[0, -1, 3, nh, dh](Linear)))
            const std::string* hv[3] = {&qn, &nodes[tk].in[0], &nodes[mm2].in[1]};
            int sq[3], sp = -1;
            bool ok = true;
            for (int t = 0; t < 3 && ok; ++t) {
                sq[t] = t == 0 ? prodn(*hv[t], "Squeeze") : prod1(*hv[t], "Squeeze");
                ok = sq[t] >= 0 && axes_are(sq[t], 0, 4);
                if (!ok) break;
                const int s = prod1(nodes[sq[t]].in[0], "Split");
                ok = s >= 0 && (sp < 0 || s == sp) && nodes[s].out.size() == 3 && nodes[s].out[(size_t)t] == nodes[sq[t]].in[0];
                sp = s;
            }
            if (!ok || cons[qn].size() != 2 || graph_outs.count(qn)) continue;
            {
                const GNode& spn = nodes[sp];
                const V parts = spn.in.size() > 1 && !spn.in[1].empty() ? ints(spn.in[1]) : spn.ais("split");
                if (spn.ai("axis", 0) != 0 || !(parts.empty() || parts == V{1, 1, 1})) continue;
            }
            const int h3 = prod1(nodes[sp].in[0], "Reshape");
            if (h3 < 0) continue;
            const V t3 = target(h3);
            if (t3.size() != 4 || t3[0] != 3 || t3[1] != -1 || t3[2] != N || t3[3] < 1) continue;
            const int64_t dh = t3[3];
            const int h2 = prod1(nodes[h3].in[0], "Transpose");
            if (h2 < 0 || !perm_is(h2, {2, 0, 3, 1, 4})) continue;
            const int h1 = prod1(nodes[h2].in[0], "Reshape");
            if (h1 < 0) continue;
            const V t1 = target(h1);
            if (t1.size() != 5 || t1[0] != 0 || t1[1] != -1 || t1[2] != 3 || t1[3] < 1 || t1[3] > (1 << 20) || t1[4] != dh) continue;
            const int64_t nh = t1[3], C = nh * dh;
            const int lq = prod1(nodes[h1].in[0], "Linear");
            if (lq < 0 || nodes[lq].in.size() < 2 || !is_init(nodes[lq].in[1])) continue;
            {
                const HostTensor& wq = inits[nodes[lq].in[1]];
                if (wq.dims != V{C, 3 * C}) continue;
                if (!nodes[lq].bias.empty() && (!is_init(nodes[lq].bias) || inits[nodes[lq].bias].dtype != DType::F32 || (int64_t)inits[nodes[lq].bias].f.size() != 3 * C)) continue;
            }
            // the rel terms, both from rq = Reshape(q, [0, h, w, dh]), q's other reader
            const int qreader = scale_pre ? mul : mm1;
            const int rq = cons[qn][0] == qreader ? cons[qn][1] : cons[qn][0];
            if (rq == qreader || dead[rq] || nodes[rq].op != "Reshape" || nodes[rq].in[0] != qn || target(rq) != V{0, h, w, dh}) continue;
            const std::string& rqv = nodes[rq].out[0];
            if (cons[rqv].size() != 2 || graph_outs.count(rqv)) continue;
            const int th2 = prod1(nodes[uh].in[0], "Transpose"), tw2 = prod1(nodes[uw].in[0], "Transpose");
            if (th2 < 0 || tw2 < 0 || !perm_is(th2, {1, 0, 2, 3}) || !perm_is(tw2, {1, 2, 0, 3})) continue;
            const int rh2 = prod1(nodes[th2].in[0], "Reshape"), rw2 = prod1(nodes[tw2].in[0], "Reshape");
            if (rh2 < 0 || rw2 < 0 || target(rh2) != V{h, -1, w, h} || target(rw2) != V{w, -1, h, w}) continue;
            const int mh = prod1(nodes[rh2].in[0], "MatMul"), mw = prod1(nodes[rw2].in[0], "MatMul");
            if (mh < 0 || mw < 0 || nodes[mh].in.size() != 2 || nodes[mw].in.size() != 2 || !table(nodes[mh].in[1], h, dh) || !table(nodes[mw].in[1], w, dh)) continue;
            const int rh1 = prod1(nodes[mh].in[0], "Reshape"), rw1 = prod1(nodes[mw].in[0], "Reshape");
            if (rh1 < 0 || rw1 < 0 || target(rh1) != V{h, -1, dh} || target(rw1) != V{w, -1, dh}) continue;
            const int th1 = prod1(nodes[rh1].in[0], "Transpose"), tw1 = prod1(nodes[rw1].in[0], "Transpose");
            if (th1 < 0 || tw1 < 0 || th1 == tw1 || !perm_is(th1, {1, 0, 2, 3}) || !perm_is(tw1, {2, 0, 1, 3}) || nodes[th1].in[0] != rqv || nodes[tw1].in[0] != rqv) continue;
            // output side: Reshape[-1, nh, h, w, dh] -> Transpose[0,2,3,1,4] -> Reshape[0, N, C] -> Linear
            const int o1 = reader1(nodes[mm2].out[0], "Reshape");
            if (o1 < 0 || target(o1) != V{-1, nh, h, w, dh}) continue;
            const int o2 = reader1(nodes[o1].out[0], "Transpose");
            if (o2 < 0 || !perm_is(o2, {0, 2, 3, 1, 4})) continue;
            const int o3 = reader1(nodes[o2].out[0], "Reshape");
            if (o3 < 0 || target(o3) != V{0, N, C}) continue;
            const int pj = reader1(nodes[o3].out[0], "Linear");
            if (pj < 0 || nodes[pj].in.size() < 2 || !is_init(nodes[pj].in[1]) || inits[nodes[pj].in[1]].dims != V{C, C}) continue;
            // front side
            const int r0 = prod1(nodes[lq].in[0], "Reshape");
            if (r0 < 0 || target(r0) != V{0, N, C}) continue;
            const int f0 = prod1(nodes[r0].in[0], "Reshape");
            if (f0 < 0) continue;
            std::vector<int> extra;
            int64_t ws = 0, H = h, W = w;
            std::string y, out;
            bool padded = false;
            if (target(f0) == V{0, h, w, C}) {           // global: the key grid is the token grid
                y = nodes[f0].in[0];
                const int fin = reader1(nodes[pj].out[0], "Reshape");
                if (fin < 0 || target(fin) != V{0, H * W, C}) continue;
                out = nodes[fin].out[0];
                extra.push_back(fin);
            } else if (h == w && target(f0) == V{-1, h, h, C}) {   // windows
                ws = h;
                const int p2 = prod1(nodes[f0].in[0], "Transpose");
                if (p2 < 0 || !perm_is(p2, {0, 1, 3, 2, 4, 5})) continue;
                const int p1 = prod1(nodes[p2].in[0], "Reshape");
                if (p1 < 0) continue;
                const V pt = target(p1);
                if (pt.size() != 6 || pt[0] != 0 || pt[1] < 1 || pt[1] > (1 << 20) || pt[2] != ws || pt[3] < 1 || pt[3] > (1 << 20) || pt[4] != ws || pt[5] != C) continue;
                const int64_t hb = pt[1], wb = pt[3], Hp = hb * ws, Wp = wb * ws;
                H = Hp; W = Wp;
                std::string cur = nodes[p1].in[0];
                if (const int pd = prod1(cur, "Pad"); pd >= 0) {
                    const GNode& pn = nodes[pd];
                    if (pn.as("mode", "constant") != "constant" || pn.in.size() < 2 || pn.in.size() > 3) continue;
                    const V pads = ints(pn.in[1]);
                    if (pads.size() != 8 || pads[0] || pads[1] || pads[2] || pads[3] || pads[4] || pads[7] || pads[5] < 0 || pads[6] < 0 || pads[5] >= ws || pads[6] >= ws) continue;
                    if (pn.in.size() == 3 && !pn.in[2].empty()) {
                        const HostTensor* pv = f32_scalar(pn.in[2]);
                        if (!pv || pv->f[0] != 0.0f) continue;
                    }
                    H = Hp - pads[5]; W = Wp - pads[6];
                    padded = pads[5] || pads[6];
                    cur = pn.in[0];
                    extra.push_back(pd);
                }
                const int fr = prod1(cur, "Reshape");
                if (fr < 0 || target(fr) != V{0, H, W, C}) continue;   // (constants: a dynamic H / W is not matched)
                y = nodes[fr].in[0];
                const int v1 = reader1(nodes[pj].out[0], "Reshape");
                if (v1 < 0 || target(v1) != V{-1, hb, wb, ws, ws, C}) continue;
                const int v2 = reader1(nodes[v1].out[0], "Transpose");
                if (v2 < 0 || !perm_is(v2, {0, 1, 3, 2, 4, 5})) continue;
                const int v3 = reader1(nodes[v2].out[0], "Reshape");
                if (v3 < 0 || target(v3) != V{-1, Hp, Wp, C}) continue;
                out = nodes[v3].out[0];
                bool ok2 = true;
                for (int ax = 1; ax <= 2 && ok2; ++ax) {
                    if ((ax == 1 ? Hp - H : Wp - W) == 0) continue;
                    const int cr = reader1(out, "Slice");
                    ok2 = cr >= 0 && slice01(cr, ax, ax == 1 ? H : W);
                    if (ok2) { out = nodes[cr].out[0]; extra.push_back(cr); }
                }
                if (!ok2) continue;
                const int fin = reader1(out, "Reshape");
                if (fin < 0 || (target(fin) != V{0, H * W, C} && target(fin) != V{-1, H * W, C})) continue;
                out = nodes[fin].out[0];
                extra.insert(extra.end(), {p2, p1, fr, v1, v2, v3, fin});
            } else {
                continue;
            }
            if (!k::relpos_attention_supported(1, H, W, ws, nh, dh)) continue;
            GNode ra_node;
            ra_node.op = "RelPosAttention";
            ra_node.in = {nodes[lq].out[0], nodes[mh].in[1], nodes[mw].in[1]};
            if (padded) ra_node.in.push_back(nodes[lq].bias);   // what a padding token is behind the Linear (empty: zeros)
            ra_node.out = {nodes[o3].out[0]};
            iattr(ra_node, "H", H); iattr(ra_node, "W", W); iattr(ra_node, "ws", ws); iattr(ra_node, "heads", nh); iattr(ra_node, "head_dim", dh); iattr(ra_node, "scale_pos", scale_pre ? 0 : 1);
            fattr(ra_node, "scale", sct->f[0]);
            nodes[lq].in[0] = y;
            nodes[pj].out[0] = out;
            for (int d : {i, ra, a2, a1, uw, uh, s5, mul, mm1, tk, mm2, sq[0], sq[1], sq[2], sp, h3, h2, h1, rq, th2, tw2, rh2, rw2, mh, mw, rh1, rw1, th1, tw1, o1, o2, r0, f0}) dead[d] = true;
            for (int d : extra) dead[d] = true;
            nodes[o3] = std::move(ra_node);              // behind the fused Linear, in front of the projection
        }
        sweep();
    }

    // ---- pass 3c: multi-scale deformable attention (the cross-attention core of an RT-DETR decoder layer), in the exported spelling, with static
    //   nh, c, Q, P and levels (h_l, w_l), Lv = sum h_l w_l:
    //   weights:  Reshape(logit, [0, Q, nh, L P]) -> Softmax(-1) -> Reshape[0, Q, nh, L, P]           (the Softmax may be missing: the input holds the weights)
    //             -> Transpose[0,2,1,3,4] -> Reshape[-1, 1, Q, L P]
    //   value:    Reshape(value, [0, Lv, nh, c]) -> Split(axis 1, [h_l w_l]);   grid = Sub(Mul(loc, 2), 1),  loc [N, Q, nh, L, P, 2]
    //   level l:  Reshape(v_l, [0, h w, nh c]) -> Transpose[0,2,1] -> Reshape[-1, c, h, w]
    //             Slice(grid, l : l + 1, axis 3) -> Squeeze[3] -> Transpose[0,2,1,3,4] -> Reshape[-1, Q, P, 2]
    //             GridSample(bilinear, zeros, align_corners = 0) -> Unsqueeze[3]
    //   combine:  Concat(axis 3) -> Reshape[0, c, Q, L P] -> Mul(., weights) -> ReduceSum(-1, keepdims 0) -> Reshape[-1, nh c, Q] -> Transpose[0,2,1]
    // becomes ONE DeformableAttention node (csrc/deformable_attention.hip) on value, loc and the logits (or weights): the value already holds the c channels of
    // a (location, head) contiguously, so the taps are read from it by address.  The match is exact: another GridSample mode / padding / alignment, another
    // permutation, levels that do not sum to Lv, an intermediate with a second reader (or that is a graph output), or a shape
    // k::deformable_attention_supported rejects keep the op-by-op route, and so does OAR_FUSE_DEFORMABLE_ATTENTION=0.
    void pass_3c_deformable_attention() {
        const bool fuse = switch_on("OAR_FUSE_DEFORMABLE_ATTENTION");
        scan();
        auto scalar_is = [&](const std::string& v, float want) {
            const HostTensor* t = f32_scalar(v);
            return t && t->f[0] == want;
        };
        for (int i = 0; fuse && i < (int)nodes.size(); ++i) {
            const GNode& cc = nodes[i];
            if (cc.op != "Concat" || dead[i] || cc.ai("axis", 0) != 3 || cc.act.kind != k::ACT_NONE || cc.in.empty() || (int)cc.in.size() > k::kDefMaxLevels) continue;
            const int64_t L = (int64_t)cc.in.size();
            int64_t c = 0, nh = 0, Q = 0, P = 0, Lv = 0;
            std::vector<int64_t> lv;                 // h, w per level
            std::vector<int> kill;
            std::string gridn;
            int sp = -1;
            bool ok = true;
            for (int64_t l = 0; l < L && ok; ++l) {
                ok = false;
                const int us = prod1(cc.in[l], "Unsqueeze");
                if (us < 0 || !axes_are(us, 3, 5)) break;
                const int gs = prod1(nodes[us].in[0], "GridSample");
                if (gs < 0 || nodes[gs].in.size() != 2) break;
                const std::string mode = nodes[gs].as("mode", "linear");
                if ((mode != "linear" && mode != "bilinear") || nodes[gs].as("padding_mode", "zeros") != "zeros" || nodes[gs].ai("align_corners", 0) != 0) break;
                // value side
                const int r2 = prod1(nodes[gs].in[0], "Reshape");
                if (r2 < 0) break;
                const V t2 = target(r2);
                if (t2.size() != 4 || t2[0] != -1 || t2[1] < 1 || t2[2] < 1 || t2[3] < 1 || (c && t2[1] != c)) break;
                c = t2[1];
                const int64_t h = t2[2], w = t2[3];
                if (h >= (int64_t)1 << 30 || w >= (int64_t)1 << 30) break;
                const int t1 = prod1(nodes[r2].in[0], "Transpose");
                if (t1 < 0 || !perm_is(t1, {0, 2, 1})) break;
                const int r1 = prod1(nodes[t1].in[0], "Reshape");
                if (r1 < 0) break;
                const V tg1 = target(r1);
                if (tg1.size() != 3 || tg1[0] != 0 || tg1[1] != h * w || tg1[2] < c || tg1[2] % c || (nh && tg1[2] != nh * c)) break;
                nh = tg1[2] / c;
                const int s = prod1(nodes[r1].in[0], "Split");
                if (s < 0 || (sp >= 0 && s != sp) || (int64_t)nodes[s].out.size() != L || nodes[s].out[(size_t)l] != nodes[r1].in[0]) break;
                sp = s;
                // grid side
                const int r3 = prod1(nodes[gs].in[1], "Reshape");
                if (r3 < 0) break;
                const V t3 = target(r3);
                if (t3.size() != 4 || t3[0] != -1 || t3[1] < 1 || t3[2] < 1 || t3[3] != 2 || (Q && (t3[1] != Q || t3[2] != P))) break;
                Q = t3[1]; P = t3[2];
                const int tg = prod1(nodes[r3].in[0], "Transpose");
                if (tg < 0 || !perm_is(tg, {0, 2, 1, 3, 4})) break;
                const int sq = prod1(nodes[tg].in[0], "Squeeze");
                if (sq < 0 || !axes_are(sq, 3, 6)) break;
                const int sl = prod1(nodes[sq].in[0], "Slice");
                if (sl < 0 || nodes[sl].in.size() < 4 || nodes[sl].in.size() > 5) break;
                if (ints(nodes[sl].in[1]) != V{l} || ints(nodes[sl].in[2]) != V{l + 1} || ints(nodes[sl].in[3]) != V{3}) break;
                if (nodes[sl].in.size() == 5 && !nodes[sl].in[4].empty() && ints(nodes[sl].in[4]) != V{1}) break;
                if (!gridn.empty() && nodes[sl].in[0] != gridn) break;
                gridn = nodes[sl].in[0];
                lv.push_back(h); lv.push_back(w);
                Lv += h * w;
                kill.insert(kill.end(), {us, gs, r2, t1, r1, r3, tg, sq, sl});
                ok = true;
            }
            if (!ok || sp < 0) continue;
            // the Split: axis 1, the levels' sizes in order; in front of it Reshape(value, [0, Lv, nh, c])
            const GNode& spn = nodes[sp];
            V parts = spn.in.size() > 1 && !spn.in[1].empty() ? ints(spn.in[1]) : spn.ais("split");
            if (spn.ai("axis", 0) != 1 || (int64_t)parts.size() != L) continue;
            bool parts_ok = true;
            for (int64_t l = 0; l < L; ++l) parts_ok = parts_ok && parts[(size_t)l] == lv[(size_t)(2 * l)] * lv[(size_t)(2 * l + 1)];
            if (!parts_ok) continue;
            const int rv = prod1(spn.in[0], "Reshape");
            if (rv < 0 || target(rv) != V{0, Lv, nh, c}) continue;
            // the grid: Sub(Mul(loc, 2), 1), read by the L Slices alone
            if ((int64_t)cons[gridn].size() != L || graph_outs.count(gridn)) continue;
            const int sb = prodn(gridn, "Sub");
            if (sb < 0 || nodes[sb].in.size() != 2 || !scalar_is(nodes[sb].in[1], 1.0f)) continue;
            const int ml = prod1(nodes[sb].in[0], "Mul");
            if (ml < 0 || nodes[ml].in.size() != 2) continue;
            const int ci = scalar_is(nodes[ml].in[1], 2.0f) ? 1 : scalar_is(nodes[ml].in[0], 2.0f) ? 0 : -1;
            if (ci < 0) continue;
            const std::string locn = nodes[ml].in[1 - ci];
            // combine
            const int rc = reader1(cc.out[0], "Reshape");
            if (rc < 0 || target(rc) != V{0, c, Q, L * P}) continue;
            const int mu = reader1(nodes[rc].out[0], "Mul");
            if (mu < 0 || nodes[mu].in.size() != 2) continue;
            const int rw = prod1(nodes[mu].in[1], "Reshape");
            if (rw < 0 || target(rw) != V{-1, 1, Q, L * P}) continue;
            const int tw = prod1(nodes[rw].in[0], "Transpose");
            if (tw < 0 || !perm_is(tw, {0, 2, 1, 3, 4})) continue;
            const int r5 = prod1(nodes[tw].in[0], "Reshape");
            if (r5 < 0 || target(r5) != V{0, Q, nh, L, P}) continue;
            int sm = prod1(nodes[r5].in[0], "Softmax"), r4 = -1;
            std::string wn = nodes[r5].in[0];
            if (sm >= 0) {
                const int64_t ax = nodes[sm].ai("axis", -1);
                if (ax != -1 && ax != 3) continue;
                r4 = prod1(nodes[sm].in[0], "Reshape");
                if (r4 < 0 || target(r4) != V{0, Q, nh, L * P}) continue;
                wn = nodes[r4].in[0];
            } else if (producer.count(wn) && nodes[producer[wn]].op == "Softmax") {
                continue;                            // a Softmax that did not fit (a second reader, another axis): not ours
            } else if (const int r = prod1(wn, "Reshape"); r >= 0 && target(r) == V{0, Q, nh, L * P}) {
                r4 = r;                              // the weights as an input: the same two Reshapes without the Softmax between them
                wn = nodes[r4].in[0];
            }
            const int rd = reader1(nodes[mu].out[0], "ReduceSum");
            if (rd < 0 || !axes_are(rd, 3, 4) || nodes[rd].ai("keepdims", 1) != 0) continue;
            const int ro = reader1(nodes[rd].out[0], "Reshape");
            if (ro < 0 || target(ro) != V{-1, nh * c, Q}) continue;
            const int tf = reader1(nodes[ro].out[0], "Transpose");
            if (tf < 0 || !perm_is(tf, {0, 2, 1})) continue;
            if (!k::deformable_attention_supported(1, Q, nh, c, L, P, Lv)) continue;
            GNode da;
            da.op = "DeformableAttention";
            da.in = {nodes[rv].in[0], locn, wn};
            da.out = {nodes[tf].out[0]};
            iattr(da, "heads", nh); iattr(da, "points", P); iattr(da, "softmax", sm >= 0 ? 1 : 0);
            Attr la; la.kind = Attr::IS; la.is = lv; da.attrs["levels"] = la;
            for (int d : kill) dead[d] = true;
            for (int d : {i, sp, rv, sb, ml, rc, mu, rw, tw, r5, rd, ro}) dead[d] = true;
            if (sm >= 0) dead[sm] = true;
            if (r4 >= 0) dead[r4] = true;
            nodes[tf] = std::move(da);               // the pattern's last node: every input is computed in front of it
        }
        sweep();
    }

    // ---- pass 3e: ordinary multi-head attention with separate q / k / v sources (PaddleDetection's MultiHeadAttention as exported: the self-attention of an
    //   RT-DETR decoder layer and the AIFI layer of its hybrid encoder), with static Tq, Tk, nh, dh:
    //   heads(t, T) = Transpose[0,2,1,3](Reshape(t, [0, T, nh, dh]))                                  (t: any tensor, usually a Linear's [N, T, nh dh] output)
    //   s = Mul(MatMul(heads(q, Tq), Transpose[0,1,3,2](heads(k, Tk))), c)   or   MatMul(Mul(heads(q, Tq), c), Transpose[0,1,3,2](heads(k, Tk)))
    //   o = Reshape(Transpose[0,2,1,3](MatMul(Softmax(s, -1), heads(v, Tk))), [0, Tq, nh dh])
    // becomes ONE MultiHeadAttention(q, k, v) node (csrc/mha_attention.hip) under the final Reshape's name: the head split and merge are address arithmetic
    // and no score tensor exists.  The match is exact, operand order included: a Softmax on another axis, anything between the scale and the Softmax (an
    // additive mask), no scale or a non-constant one, another permutation or Reshape target, an intermediate with a second reader (or that is a graph output)
    // and a shape k::mha_attention_supported rejects keep the op-by-op route.  The q / k / v of the SVTR (pass 5), Swin (3b) and ViT (3d) blocks come from
    // rank-5 splits, not from heads(t), so this pass cannot take them.  OAR_FUSE_MHA_ATTENTION=0, read at load time, keeps the op-by-op route; the default is on
    // (the fused arm's whole range lies below the op-by-op arm's on the decoder and the AIFI layer at N = 1 and 8).  It runs before pass 4 so that
    // the block's residual Add folds into the projection behind it.
    void pass_3e_mha_attention() {
        const bool fuse = switch_on("OAR_FUSE_MHA_ATTENTION");
        scan();
        // heads(t, T): -> the Transpose and the Reshape, and (T, nh, dh); false where v is anything else
        auto heads = [&](const std::string& v, int& tr, int& rs, int64_t& T, int64_t& nh, int64_t& dh) {
            tr = prod1(v, "Transpose");
            if (tr < 0 || !perm_is(tr, {0, 2, 1, 3})) return false;
            rs = prod1(nodes[tr].in[0], "Reshape");
            if (rs < 0) return false;
            const V t = target(rs);
            if (t.size() != 4 || t[0] != 0 || t[1] < 1 || t[2] < 1 || t[3] < 1) return false;
            T = t[1]; nh = t[2]; dh = t[3];
            return true;
        };
        for (int i = 0; fuse && i < (int)nodes.size(); ++i) {
            if (nodes[i].op != "Softmax" || dead[i] || nodes[i].act.kind != k::ACT_NONE) continue;
            const int64_t sax = nodes[i].ai("axis", -1);
            if (sax != -1 && sax != 3) continue;
            // the scale: on the product, or on q in front of it
            const std::string& sv = nodes[i].in[0];
            int mul = prod1(sv, "Mul"), mm1 = -1, scale_pre = 0;
            if (mul >= 0) {
                mm1 = prod1(nodes[mul].in[0], "MatMul");
            } else {
                mm1 = prod1(sv, "MatMul");
                mul = mm1 < 0 ? -1 : prod1(nodes[mm1].in[0], "Mul");
                scale_pre = 1;
            }
            if (mm1 < 0 || mul < 0 || nodes[mul].in.size() != 2 || nodes[mm1].in.size() != 2) continue;
            const HostTensor* sct = f32_scalar(nodes[mul].in[1]);
            if (!sct) continue;
            const int tk = prod1(nodes[mm1].in[1], "Transpose");
            if (tk < 0 || !perm_is(tk, {0, 1, 3, 2})) continue;
            const int mm2 = reader1(nodes[i].out[0], "MatMul");
            if (mm2 < 0 || nodes[mm2].in.size() != 2) continue;
            int qt, qr, kt, kr, vt, vr;
            int64_t Tq, Tk, Tv, nh, nhk, nhv, dh, dhk, dhv;
            if (!heads(scale_pre ? nodes[mul].in[0] : nodes[mm1].in[0], qt, qr, Tq, nh, dh) || !heads(nodes[tk].in[0], kt, kr, Tk, nhk, dhk) ||
                !heads(nodes[mm2].in[1], vt, vr, Tv, nhv, dhv))
                continue;
            if (Tv != Tk || nhk != nh || nhv != nh || dhk != dh || dhv != dh || qt == kt || qt == vt || kt == vt) continue;
            // the merge: Transpose[0,2,1,3] -> Reshape[0, Tq, nh dh]
            const int o1 = reader1(nodes[mm2].out[0], "Transpose");
            if (o1 < 0 || !perm_is(o1, {0, 2, 1, 3})) continue;
            const int o2 = reader1(nodes[o1].out[0], "Reshape");
            if (o2 < 0 || !k::mha_attention_supported(1, Tq, Tk, nh, dh) || target(o2) != V{0, Tq, nh * dh}) continue;
            GNode ma;
            ma.op = "MultiHeadAttention";
            ma.in = {nodes[qr].in[0], nodes[kr].in[0], nodes[vr].in[0]};
            ma.out = {nodes[o2].out[0]};
            iattr(ma, "Tq", Tq); iattr(ma, "Tk", Tk); iattr(ma, "heads", nh); iattr(ma, "head_dim", dh); iattr(ma, "scale_pos", scale_pre ? 0 : 1);
            fattr(ma, "scale", sct->f[0]);
            for (int d : {i, mul, mm1, tk, mm2, qt, qr, kt, kr, vt, vr, o1}) dead[d] = true;
            nodes[o2] = std::move(ma);                   // the pattern's last node: every input is computed in front of it
        }
        sweep();
    }

    // ---- pass 4: Linear / Conv -> Add(residual): fold the residual into the producer's epilogue (no act between);
    // shapes are only known at plan time: op_conv / op_linear fall back to a separate add when they do not match
    void pass_4_residual() {
        scan();
        for (int i = 0; i < (int)nodes.size(); ++i) {
            GNode& ad = nodes[i];
            if (ad.op != "Add" || ad.act.kind != k::ACT_NONE) continue;
            for (int t = 0; t < 2; ++t) {
                auto pit = producer.find(ad.in[t]);
                if (pit == producer.end() || dead[pit->second]) continue;
                GNode& lin = nodes[pit->second];
                if ((lin.op != "Linear" && lin.op != "Conv") || lin.act.kind != k::ACT_NONE || !lin.residual.empty()) continue;
                if (cons[ad.in[t]].size() != 1 || graph_outs.count(ad.in[t])) continue;
                const std::string& other = ad.in[1 - t];
                if (is_init(other)) continue;
                // move the fused Linear to the Add's position so `other` is already computed
                GNode f = lin;
                f.residual = other;
                f.out[0] = ad.out[0];
                dead[pit->second] = true;
                nodes[i] = std::move(f);
                break;
            }
        }
        sweep();
    }

    // ---- pass 5: the SVTR global-attention block (EncoderWithSVTR), as the recognizer exports emit it:
    //   Reshape[0,-1,3,h,d] -> Transpose[2,0,3,1,4] -> Split(axis 0) -> 3 x Squeeze[0] -> (Mul by a scalar on q) ->
    //   MatMul(q, Transpose[0,1,3,2](k)) -> Softmax(-1) -> MatMul(., v) -> Transpose[0,2,1,3] -> Reshape[0,-1,h*d]
    // becomes ONE Attention node that reads the [n, T, 3*h*d] projection in place (12 glue kernels + 2 batched GEMMs +
    // softmax -> 1 kernel).  OAR_FUSE_ATTENTION=0 keeps the op-by-op path.
    void pass_5_svtr_attention() {
        const bool fuse = switch_on("OAR_FUSE_ATTENTION");
        scan();
        auto prod = [&](const std::string& v, const char* op) -> int {
            auto it = producer.find(v);
            if (it == producer.end() || dead[it->second] || nodes[it->second].op != op) return -1;
            return it->second;
        };
        auto single_use = [&](const std::string& v) { return cons[v].size() == 1 && !graph_outs.count(v); };
        auto ints_of = [&](const std::string& v) -> std::vector<int64_t> {
            auto it = inits.find(v);
            return it == inits.end() ? std::vector<int64_t>{} : it->second.i;
        };
        auto perm_is = [&](const GNode& t, std::initializer_list<int64_t> want) { return t.ais("perm") == std::vector<int64_t>(want); };
        auto squeeze0 = [&](const GNode& q) {
            std::vector<int64_t> ax = q.in.size() > 1 ? ints_of(q.in[1]) : q.ais("axes");
            return ax.size() == 1 && ax[0] == 0;
        };
        for (int i = 0; fuse && i < (int)nodes.size(); ++i) {
            if (nodes[i].op != "Softmax" || dead[i]) continue;
            const GNode& sm = nodes[i];
            const int64_t sax = sm.ai("axis", -1);
            if (sax != -1 && sax != 3) continue;
            const int mm1 = prod(sm.in[0], "MatMul");
            if (mm1 < 0 || !single_use(sm.in[0]) || !single_use(sm.out[0])) continue;
            const int mm2 = cons[sm.out[0]][0];
            if (nodes[mm2].op != "MatMul" || nodes[mm2].in[0] != sm.out[0]) continue;
            // q side: Squeeze [-> Mul scalar]
            float scale = 1.0f;
            std::string qv = nodes[mm1].in[0];
            int mul = prod(qv, "Mul");
            if (mul >= 0) {
                if (!single_use(qv)) continue;
                int ci = is_init(nodes[mul].in[1]) ? 1 : is_init(nodes[mul].in[0]) ? 0 : -1;
                if (ci < 0) continue;
                const HostTensor& sc = inits[nodes[mul].in[ci]];
                if (sc.dtype != DType::F32 || sc.f.size() != 1) continue;
                scale = sc.f[0];
                qv = nodes[mul].in[1 - ci];
            }
            const int sq_q = prod(qv, "Squeeze");
            const int tk = prod(nodes[mm1].in[1], "Transpose");
            if (sq_q < 0 || tk < 0 || !single_use(qv) || !single_use(nodes[mm1].in[1]) || !perm_is(nodes[tk], {0, 1, 3, 2})) continue;
            const int sq_k = prod(nodes[tk].in[0], "Squeeze");
            const int sq_v = prod(nodes[mm2].in[1], "Squeeze");
            if (sq_k < 0 || sq_v < 0 || !single_use(nodes[tk].in[0]) || !single_use(nodes[mm2].in[1])) continue;
            if (!squeeze0(nodes[sq_q]) || !squeeze0(nodes[sq_k]) || !squeeze0(nodes[sq_v])) continue;
            const int sp = prod(nodes[sq_q].in[0], "Split");
            if (sp < 0 || nodes[sp].out.size() != 3 || nodes[sp].ai("axis", 0) != 0) continue;
            if (nodes[sq_q].in[0] != nodes[sp].out[0] || nodes[sq_k].in[0] != nodes[sp].out[1] || nodes[sq_v].in[0] != nodes[sp].out[2]) continue;
            if (!single_use(nodes[sp].out[0]) || !single_use(nodes[sp].out[1]) || !single_use(nodes[sp].out[2])) continue;
            const int t1 = prod(nodes[sp].in[0], "Transpose");
            if (t1 < 0 || !single_use(nodes[sp].in[0]) || !perm_is(nodes[t1], {2, 0, 3, 1, 4})) continue;
            const int r1 = prod(nodes[t1].in[0], "Reshape");
            if (r1 < 0 || !single_use(nodes[t1].in[0]) || nodes[r1].in.size() < 2) continue;
            const std::vector<int64_t> shp = ints_of(nodes[r1].in[1]);
            if (shp.size() != 5 || shp[0] != 0 || shp[1] != -1 || shp[2] != 3 || shp[3] <= 0 || shp[4] <= 0 || shp[4] > 64) continue;
            // output side: Transpose[0,2,1,3] -> Reshape[0,-1,h*d]
            if (!single_use(nodes[mm2].out[0])) continue;
            const int t2 = cons[nodes[mm2].out[0]][0];
            if (nodes[t2].op != "Transpose" || !perm_is(nodes[t2], {0, 2, 1, 3}) || !single_use(nodes[t2].out[0])) continue;
            const int r2 = cons[nodes[t2].out[0]][0];
            if (nodes[r2].op != "Reshape" || nodes[r2].in.size() < 2) continue;
            const std::vector<int64_t> shp2 = ints_of(nodes[r2].in[1]);
            if (shp2.size() != 3 || shp2[0] != 0 || shp2[1] != -1 || shp2[2] != shp[3] * shp[4]) continue;
            GNode at;
            at.op = "Attention";
            at.in = {nodes[r1].in[0]};
            at.out = {nodes[r2].out[0]};
            Attr ah; ah.kind = Attr::I; ah.i = shp[3]; at.attrs["heads"] = ah;
            Attr ad; ad.kind = Attr::I; ad.i = shp[4]; at.attrs["head_dim"] = ad;
            Attr as; as.kind = Attr::F; as.f = scale; at.attrs["scale"] = as;
            for (int d : {r1, t1, sp, sq_q, sq_k, sq_v, tk, mm1, i, mm2, t2}) dead[d] = true;
            if (mul >= 0) dead[mul] = true;
            nodes[r2] = std::move(at);   // the last node of the block: its input is long computed
        }
        sweep();
    }

    // ---- pass 6: squeeze-excite gate: GlobalAveragePool -> Conv 1x1 (+act) -> Conv 1x1 (+act) on the pooled vector
    // becomes one SEGate node (two GEMVs per image in one kernel instead of two implicit-GEMM launches).
    void pass_6_se_gate() {
        const bool fuse = switch_on("OAR_FUSE_SE");
        scan();
        auto plain_1x1 = [&](const GNode& c) {
            if (c.op != "Conv" || c.in.size() < 2 || !is_init(c.in[1]) || !c.residual.empty() || c.ai("group", 1) != 1) return false;
            const HostTensor& w = inits[c.in[1]];
            if (w.dims.size() != 4 || w.dims[2] != 1 || w.dims[3] != 1) return false;
            for (auto v : c.ais("strides")) if (v != 1) return false;
            for (auto v : c.ais("pads")) if (v != 0) return false;
            return c.as("auto_pad", "NOTSET") == "NOTSET" && (c.in.size() < 3 || c.in[2].empty() || is_init(c.in[2]));
        };
        for (int i = 0; fuse && i < (int)nodes.size(); ++i) {
            if (dead[i] || nodes[i].op != "GlobalAveragePool") continue;
            const std::string& pooled = nodes[i].out[0];
            if (cons[pooled].size() != 1 || graph_outs.count(pooled)) continue;
            const int a = cons[pooled][0];
            if (!plain_1x1(nodes[a]) || nodes[a].in[0] != pooled) continue;
            const std::string& mid = nodes[a].out[0];
            if (cons[mid].size() != 1 || graph_outs.count(mid)) continue;
            const int b = cons[mid][0];
            if (!plain_1x1(nodes[b]) || nodes[b].in[0] != mid) continue;
            if (inits[nodes[b].in[1]].dims[1] != inits[nodes[a].in[1]].dims[0]) continue;
            GNode g;
            g.op = "SEGate";
            g.in = {pooled, nodes[a].in[1], nodes[a].in.size() > 2 ? nodes[a].in[2] : std::string(), nodes[b].in[1], nodes[b].in.size() > 2 ? nodes[b].in[2] : std::string()};
            g.out = {nodes[b].out[0]};
            g.act = nodes[b].act;
            Attr k1; k1.kind = Attr::I; k1.i = nodes[a].act.kind; g.attrs["act1"] = k1;
            Attr al; al.kind = Attr::F; al.f = nodes[a].act.alpha; g.attrs["act1_alpha"] = al;
            Attr be; be.kind = Attr::F; be.f = nodes[a].act.beta; g.attrs["act1_beta"] = be;
            dead[a] = true;
            nodes[b] = std::move(g);
        }
        sweep();
    }

    // ---- pass 7: depthwise-separable block: Conv (depthwise k x k, folded activation) -> Conv (1 x 1, folded activation /
    // residual) with nothing else reading the expanded tensor becomes ONE DSBlock node (csrc/dsblock.inc: the depthwise
    // output stays in LDS and feeds the matrix pipe).  Shapes are only known at plan time: op_dsblock falls back to the two
    // convolutions when dsblock_eligible() says no.  OAR_FUSE_DSBLOCK=0 keeps them apart.
    void pass_7_dsblock() {
        const bool fuse = switch_on("OAR_FUSE_DSBLOCK");
        scan();
        auto ints = [](const GNode& c, const char* k, int64_t dflt) { auto v = c.ais(k); return v.empty() ? std::vector<int64_t>{dflt, dflt} : v; };
        for (int i = 0; fuse && i < (int)nodes.size(); ++i) {
            const GNode& d = nodes[i];
            if (dead[i] || d.op != "Conv" || d.in.size() < 2 || !is_init(d.in[1]) || !d.residual.empty()) continue;
            const HostTensor& wd = inits[d.in[1]];
            if (wd.dims.size() != 4 || wd.dims[1] != 1 || wd.dims[2] != wd.dims[3] || (wd.dims[2] != 3 && wd.dims[2] != 5)) continue;
            if (d.ai("group", 1) != wd.dims[0] || wd.dims[0] < 8) continue;
            for (auto v : d.ais("dilations")) if (v != 1) goto next_node;
            if (d.as("auto_pad", "NOTSET") != "NOTSET" || (d.in.size() > 2 && !d.in[2].empty() && !is_init(d.in[2]))) continue;
            {
                const std::string& mid = d.out[0];
                if (graph_outs.count(mid) || cons[mid].size() != 1) continue;
                const int j = cons[mid][0];
                GNode& pw = nodes[j];
                if (dead[j] || pw.op != "Conv" || pw.in[0] != mid || pw.in.size() < 2 || !is_init(pw.in[1]) || pw.ai("group", 1) != 1) continue;
                const HostTensor& wp = inits[pw.in[1]];
                if (wp.dims.size() != 4 || wp.dims[2] != 1 || wp.dims[3] != 1 || wp.dims[1] != wd.dims[0]) continue;
                bool plain = pw.as("auto_pad", "NOTSET") == "NOTSET" && (pw.in.size() < 3 || pw.in[2].empty() || is_init(pw.in[2]));
                for (auto v : ints(pw, "strides", 1)) plain = plain && v == 1;
                for (auto v : pw.ais("pads")) plain = plain && v == 0;
                if (!plain) continue;
                GNode f;
                f.op = "DSBlock";
                f.in = {d.in[0], d.in[1], d.in.size() > 2 ? d.in[2] : std::string(), pw.in[1], pw.in.size() > 2 ? pw.in[2] : std::string()};
                f.out = {pw.out[0]};
                f.attrs = d.attrs;                      // strides / pads / kernel_shape of the depthwise conv
                f.act = pw.act; f.residual = pw.residual;
                Attr k1; k1.kind = Attr::I; k1.i = d.act.kind; f.attrs["act1"] = k1;
                Attr al; al.kind = Attr::F; al.f = d.act.alpha; f.attrs["act1_alpha"] = al;
                Attr be; be.kind = Attr::F; be.f = d.act.beta; f.attrs["act1_beta"] = be;
                Attr mn; mn.kind = Attr::S; mn.s = mid; f.attrs["mid_name"] = mn;
                dead[i] = true;
                nodes[j] = std::move(f);   // at the pointwise conv's position: a folded residual is computed by then
            }
        next_node:;
        }
        sweep();
    }

    // ---- pass 8: squeeze-excite scale into the pointwise conv behind it: Mul(x, SEGate(...)) whose only reader is a plain 1x1 Conv
    // becomes that Conv with the gate as a 4th input (csrc/igemm_ws_x6.hip multiplies it into the pixels as they are loaded: the scaled
    // feature map is never written or re-read).  Shapes / kernel choice are plan-time matters: op_conv runs the Mul after all when the
    // bf16x6 weight-stationary kernel does not take the layer.  OAR_FUSE_SE_SCALE=0 keeps the Mul.
    void pass_8_se_scale() {
        const bool fuse = switch_on("OAR_FUSE_SE_SCALE");
        scan();
        for (int i = 0; fuse && i < (int)nodes.size(); ++i) {
            const GNode& m = nodes[i];
            if (m.op != "Mul" || m.in.size() != 2 || m.act.kind != k::ACT_NONE || !m.residual.empty() || graph_outs.count(m.out[0])) continue;
            int gi = -1;
            for (int t = 0; t < 2; ++t) { auto pit = producer.find(m.in[t]); if (pit != producer.end() && nodes[pit->second].op == "SEGate") gi = t; }
            if (gi < 0 || cons[m.out[0]].size() != 1) continue;
            GNode& c = nodes[cons[m.out[0]][0]];
            if (c.op != "Conv" || c.in.size() < 2 || c.in.size() > 3 || c.in[0] != m.out[0] || !is_init(c.in[1]) || c.ai("group", 1) != 1) continue;
            const HostTensor& w = inits[c.in[1]];
            if (w.dims.size() != 4 || w.dims[2] != 1 || w.dims[3] != 1) continue;
            bool plain = c.as("auto_pad", "NOTSET") == "NOTSET";
            for (auto v : c.ais("strides")) plain = plain && v == 1;
            for (auto v : c.ais("pads")) plain = plain && v == 0;
            if (!plain) continue;
            c.in.resize(4);
            c.in[0] = m.in[1 - gi];
            c.in[3] = m.in[gi];
            dead[i] = true;
        }
        sweep();
    }

    // ---- pass 9: the squeeze of a squeeze-excite block from the depthwise conv's own epilogue: GlobalAveragePool(dw conv output) is
    // dropped and its output becomes a second output of the conv node (conv_dw_tiled_kernel<..., GAP> writes per-tile sums,
    // global_avgpool_finish reduces them: the feature map is not read a second time).  op_conv pools separately when the launched
    // depthwise variant has no pooled form.  OAR_FUSE_SE_POOL=0 keeps the GlobalAveragePool.
    void pass_9_se_pool() {
        const char* fe = getenv("OAR_FUSE_SE_POOL");
        const bool fuse = !fe || atoi(fe) != 0;
        scan();
        for (int i = 0; fuse && i < (int)nodes.size(); ++i) {
            const GNode& gp = nodes[i];
            if (gp.op != "GlobalAveragePool" || gp.in.size() != 1 || graph_outs.count(gp.out[0])) continue;
            auto pit = producer.find(gp.in[0]);
            if (pit == producer.end() || pit->second > i) continue;
            GNode& d = nodes[pit->second];
            if (d.op != "Conv" || d.out.size() != 1 || d.in.size() < 2 || d.in.size() > 3 || !is_init(d.in[1]) || !d.residual.empty()) continue;
            const HostTensor& wd = inits[d.in[1]];
            if (wd.dims.size() != 4 || wd.dims[1] != 1 || d.ai("group", 1) != wd.dims[0] || wd.dims[0] < 8) continue;   // depthwise
            d.out.push_back(gp.out[0]);
            dead[i] = true;
            // round 5: when the pooled vector only feeds a fused squeeze-excite gate the conv hands over its per-tile sums as they are and
            // se_fc reduces them (no global_avgpool_finish launch: 4 fewer 6 us kernels and kernel boundaries per recognition batch).
            // OAR_FUSE_SE_POOL=1 keeps the finishing launch.
            int readers = 0, gate = -1;
            for (int j = 0; j < (int)nodes.size(); ++j) {
                if (dead[j]) continue;
                for (size_t q = 0; q < nodes[j].in.size(); ++q) if (nodes[j].in[q] == gp.out[0]) { ++readers; if (nodes[j].op == "SEGate" && q == 0) gate = j; }
                if (nodes[j].residual == gp.out[0]) ++readers;
            }
            // (a pooled vector that is ALSO a graph output must exist as [N, C, 1, 1] means, not as raw tile sums: ADVICE r5)
            if (readers == 1 && gate >= 0 && !graph_outs.count(gp.out[0]) && !(fe && atoi(fe) == 1)) { Attr a; a.kind = Attr::I; a.i = 1; d.attrs["gap_raw"] = a; }
        }
        sweep();
    }

    // ---- pass 10: residual Add -> LayerNormalization.  Behind every pass above: an Add that pass 4 folded into its Linear is that Linear's
    // residual by now (one folded into a Conv stays there), one that pass 3 gave an activation is not plain.  Layouts, shapes and whether the sample-local chain takes the LayerNorm are known at plan time only, so this pass
    // just marks the pair: a LayerNormalization directly behind the plain Add it reads (where every exporter puts it), its scale and bias initializers or absent;
    // Planner::fuse_chains then replaces the two launches by ONE k::add_layernorm where the pair qualifies.  OAR_FUSE_ADD_LAYERNORM=0 keeps both.
    void pass_10_add_layernorm() {
        fuse_add_ln = switch_on("OAR_FUSE_ADD_LAYERNORM");
        for (int j = 1; fuse_add_ln && j < (int)nodes.size(); ++j) {
            GNode& ln = nodes[j];
            const GNode& ad = nodes[j - 1];
            if (ln.op != "LayerNormalization" || ln.in.empty() || ad.out.empty() || ad.out[0] != ln.in[0]) continue;
            // the Add itself, or the Linear that pass 4 folded it into (Linear(x) + residual, no activation: op_linear hands the residual back where that pays)
            const bool add = ad.op == "Add" && ad.in.size() == 2 && ad.residual.empty(), lin = ad.op == "Linear" && !ad.residual.empty();
            if ((!add && !lin) || ad.act.kind != k::ACT_NONE) continue;
            bool consts = true;
            for (size_t q = 1; q < ln.in.size(); ++q) consts = consts && (ln.in[q].empty() || is_init(ln.in[q]));
            if (!consts) continue;
            Attr a; a.kind = Attr::I; a.i = 1; ln.attrs["after_add"] = a;
        }
    }

    // the table of contents.  The order matters: 3b - 3e look for plain nodes, so they run before pass 4 attaches residuals (and so that a block's residual Add
    // folds into the projection they leave behind); pass 10 reads what every other pass left.
    RewrittenGraph run(OnnxModel& m) {
        inits = std::move(m.initializers);
        graph_outs = std::set<std::string>(m.outputs.begin(), m.outputs.end());
        opset = m.opset;
        for (auto& on : m.nodes) {
            if (on.op == "Constant") {
                auto it = on.attrs.find("value");
                OAR_CHECK(it != on.attrs.end() && it->second.kind == Attr::T, OAR_UNSUPPORTED_OP, "Constant without tensor value");
                HostTensor t = it->second.t;
                t.name = on.outputs[0];
                inits[t.name] = std::move(t);
                continue;
            }
            if (on.op == "Dropout") { on.op = "Identity"; on.outputs.resize(1); }
            GNode g;
            g.op = on.op; g.in = on.inputs; g.out = on.outputs; g.attrs = on.attrs;
            nodes.push_back(std::move(g));
        }
        pass_0_loops();
        pass_1_fold_batchnorm();
        pass_2_linear();
        pass_2b_gelu();
        pass_2c_layernorm();
        pass_3_activations();
        pass_3b_window_attention();
        pass_3d_relpos_attention();
        pass_3c_deformable_attention();
        pass_3e_mha_attention();
        pass_4_residual();
        pass_5_svtr_attention();
        pass_6_se_gate();
        pass_7_dsblock();
        pass_8_se_scale();
        pass_9_se_pool();
        pass_10_add_layernorm();
        for (int i = 0; i < (int)nodes.size(); ++i) nodes[i].id = i;
        RewrittenGraph g;
        g.nodes = std::move(nodes);
        g.inits = std::move(inits);
        g.ln_spelled = std::move(ln_spelled);
        g.fuse_add_ln = fuse_add_ln;
        return g;
    }
};

}  // namespace

RewrittenGraph rewrite_graph(OnnxModel& m) { return Rewriter().run(m); }

// -------------------------------------------------------------------------------------------------
// The listing behind oar_onnx_rewrite: what the rewriter made of a model, readable without a device.  Floats print as %a (exact), tensors as dtype / dims /
// 64-bit FNV-1a of the payload, graph attributes by a mark.
namespace {

std::string tensor_text(const HostTensor& t) {
    uint64_t h = 1469598103934665603ull;
    auto eat = [&](const void* p, size_t n) { for (size_t i = 0; i < n; ++i) { h ^= ((const unsigned char*)p)[i]; h *= 1099511628211ull; } };
    eat(t.f.data(), t.f.size() * sizeof(float));
    eat(t.i.data(), t.i.size() * sizeof(int64_t));
    std::string s = "dtype=" + std::to_string((int)t.dtype) + " dims=[";
    for (size_t i = 0; i < t.dims.size(); ++i) s += (i ? "," : "") + std::to_string(t.dims[i]);
    char b[32];
    snprintf(b, sizeof b, "%016llx", (unsigned long long)h);
    return s + "] fnv=" + b;
}

std::string float_text(float v) {
    char b[48];
    snprintf(b, sizeof b, "%a", (double)v);
    return b;
}

std::string names_text(const std::vector<std::string>& v) {
    std::string s = "[";
    for (size_t i = 0; i < v.size(); ++i) s += (i ? "," : "") + v[i];
    return s + "]";
}

std::string node_text(const GNode& n) {
    std::string s = n.op + " out=" + names_text(n.out) + " in=" + names_text(n.in) + " act=" + std::to_string(n.act.kind) + "," + float_text(n.act.alpha) + "," + float_text(n.act.beta) +
                    " bias=" + n.bias + " residual=" + n.residual + " attrs={";
    bool first = true;
    for (auto& kv : n.attrs) {
        const Attr& a = kv.second;
        s += (first ? "" : "; ") + kv.first + "=";
        first = false;
        switch (a.kind) {
            case Attr::F: s += "f:" + float_text(a.f); break;
            case Attr::I: s += "i:" + std::to_string(a.i); break;
            case Attr::S: s += "s:" + a.s; break;
            case Attr::T: s += "t:" + tensor_text(a.t); break;
            case Attr::FS: s += "fs:"; for (size_t i = 0; i < a.fs.size(); ++i) s += (i ? "," : "") + float_text(a.fs[i]); break;
            case Attr::IS: s += "is:"; for (size_t i = 0; i < a.is.size(); ++i) s += (i ? "," : "") + std::to_string(a.is[i]); break;
            case Attr::G: s += "g:<graph>"; break;
            default: s += "none"; break;
        }
    }
    return s + "}";
}

}  // namespace

std::string graph_listing(const RewrittenGraph& g) {
    std::string s;
    for (const GNode& n : g.nodes) s += "node " + std::to_string(n.id) + " " + node_text(n) + "\n";
    for (auto& kv : g.inits) s += "init " + kv.first + " " + tensor_text(kv.second) + "\n";
    for (auto& kv : g.ln_spelled) {
        s += "ln_spelled " + kv.first + " " + std::to_string(kv.second.size()) + "\n";
        for (const GNode& n : kv.second) s += "  " + node_text(n) + "\n";
    }
    s += "fuse_add_ln " + std::to_string(g.fuse_add_ln ? 1 : 0) + "\n";
    return s;
}

}  // namespace oar
