// engine_loops.cc -- pass 0 of the load-time rewriter (engine_rewrite.cc): the two Loop bodies the engine executes, recognised by their interface and matched
// node by node.  There is no generic sub-graph executor: a body that is not one of these in a spelling its matcher tolerates is refused with the name of the
// first body node that did not fit.  Host-only.
#include "graph_rewrite.h"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "common.h"

namespace oar {

namespace {
// What the Loop matchers share: the body's constants (body initializers, body Constant nodes, then the outer scope), the producer of every body value,
// the marks of the nodes a matcher has accounted for, and the refusal that names the Loop and the body node that did not fit.
struct LoopBody {
    const OnnxModel& body;
    const std::map<std::string, HostTensor>& outer;
    std::string prefix;   // "Loop (name): only ... is supported as a Loop body: "
    std::string step;     // what the body must be, for messages: "SLA step"
    std::map<std::string, HostTensor> local;
    std::map<std::string, int> producer;
    std::vector<bool> used;
    LoopBody(const OnnxModel& b, const std::map<std::string, HostTensor>& o, std::string pfx, std::string st)
        : body(b), outer(o), prefix(std::move(pfx)), step(std::move(st)), used(b.nodes.size(), false) {
        for (int i = 0; i < (int)body.nodes.size(); ++i) {
            const OnnxNode& bn = body.nodes[i];
            if (bn.op == "Constant") {
                auto it = bn.attrs.find("value");
                if (it != bn.attrs.end() && it->second.kind == Attr::T && !bn.outputs.empty()) { local[bn.outputs[0]] = it->second.t; used[i] = true; continue; }
            }
            for (auto& o2 : bn.outputs) producer[o2] = i;
        }
    }
    [[noreturn]] void refuse(const std::string& why) const { fail(OAR_UNSUPPORTED_OP, prefix + why); }
    const HostTensor* cst(const std::string& s) const {
        auto a = body.initializers.find(s);
        if (a != body.initializers.end()) return &a->second;
        auto b = local.find(s);
        if (b != local.end()) return &b->second;
        if (producer.count(s)) return nullptr;
        auto c = outer.find(s);
        return c == outer.end() ? nullptr : &c->second;
    }
    std::string node_desc(int i) const {
        const OnnxNode& bn = body.nodes[i];
        return "body node '" + (bn.name.empty() ? (bn.outputs.empty() ? std::string("?") : bn.outputs[0]) : bn.name) + "' (" + bn.op + ")";
    }
    // the node that produces `v`, which must be a `op`; marks it
    const OnnxNode& expect(const std::string& v, const char* op, const char* role) {
        auto it = producer.find(v);
        if (it == producer.end()) refuse(std::string("the ") + role + " '" + v + "' is not computed by a " + op + " in the body");
        const OnnxNode& bn = body.nodes[it->second];
        if (bn.op != op) refuse(node_desc(it->second) + " does not fit: the " + role + " must be a " + op);
        used[it->second] = true;
        return bn;
    }
    [[noreturn]] void bad(const OnnxNode& bn, const std::string& why) const { refuse(node_desc((int)(&bn - body.nodes.data())) + " does not fit: " + why); }
    bool is_op(const std::string& v, const char* op) const { auto it = producer.find(v); return it != producer.end() && body.nodes[it->second].op == op; }
    std::string strip_casts(std::string v) {
        while (is_op(v, "Cast")) { const int i = producer[v]; used[i] = true; v = body.nodes[i].inputs[0]; }
        return v;
    }
    std::vector<int64_t> ints_arg(const OnnxNode& bn, const char* attr, size_t input) const {
        if (bn.has(attr)) { auto& a = bn.attrs.at(attr); return a.kind == Attr::I ? std::vector<int64_t>{a.i} : a.is; }
        if (input < bn.inputs.size() && !bn.inputs[input].empty())
            if (const HostTensor* t = cst(bn.inputs[input])) return t->i;
        return {};
    }
    const HostTensor& f32c(const OnnxNode& bn, const std::string& s, size_t rank) const {
        const HostTensor* t = cst(s);
        if (!t || t->dtype != DType::F32 || t->dims.size() != rank || (int64_t)t->f.size() != t->numel() || t->numel() == 0) bad(bn, "'" + s + "' must be a constant f32 tensor of rank " + std::to_string(rank));
        return *t;
    }
    // y = x W^T + b as Gemm(x, W, b, transB) or [Add(] MatMul(x, W^T) [, b)]: W comes back as [N][K] row-major.  want_bias: 1 required, 0 refused, -1 optional
    struct Lin { std::string x; std::vector<float> w, b; int64_t N = 0, K = 0; };
    Lin lin(const std::string& v, const char* role, int want_bias) {
        Lin r;
        auto it = producer.find(v);
        if (it == producer.end()) refuse(std::string("the ") + role + " '" + v + "' is not computed in the body");
        const OnnxNode* bn = &body.nodes[it->second];
        used[it->second] = true;
        if (bn->op == "Gemm") {
            if (bn->inputs.size() < 2 || bn->af("alpha", 1.0f) != 1.0f || bn->af("beta", 1.0f) != 1.0f || bn->ai("transA", 0) != 0) bad(*bn, "Gemm with alpha / beta / transA");
            const HostTensor& W = f32c(*bn, bn->inputs[1], 2);
            const bool tb = bn->ai("transB", 0) != 0;
            r.N = tb ? W.dims[0] : W.dims[1]; r.K = tb ? W.dims[1] : W.dims[0];
            r.w.resize((size_t)(r.N * r.K));
            for (int64_t a = 0; a < r.N; ++a) for (int64_t k = 0; k < r.K; ++k) r.w[(size_t)(a * r.K + k)] = tb ? W.f[(size_t)(a * r.K + k)] : W.f[(size_t)(k * r.N + a)];
            if (bn->inputs.size() > 2 && !bn->inputs[2].empty()) { const HostTensor& b = f32c(*bn, bn->inputs[2], 1); if (b.numel() != r.N) bad(*bn, "bias length"); r.b = b.f; }
            r.x = bn->inputs[0];
        } else {
            const OnnxNode* mm = bn;
            if (bn->op == "Add") {
                if (bn->inputs.size() != 2) bad(*bn, "Add needs two inputs");
                const int mi = is_op(bn->inputs[0], "MatMul") ? 0 : is_op(bn->inputs[1], "MatMul") ? 1 : -1;
                if (mi < 0) bad(*bn, std::string("the ") + role + " must be a Gemm or MatMul + Add");
                const HostTensor& b = f32c(*bn, bn->inputs[1 - mi], 1);
                r.b = b.f;
                used[producer[bn->inputs[mi]]] = true;
                mm = &body.nodes[producer[bn->inputs[mi]]];
            } else if (bn->op != "MatMul") {
                bad(*bn, std::string("the ") + role + " must be a Gemm or MatMul [+ Add]");
            }
            if (mm->inputs.size() != 2) bad(*mm, "MatMul needs two inputs");
            const HostTensor& W = f32c(*mm, mm->inputs[1], 2);
            r.K = W.dims[0]; r.N = W.dims[1];
            r.w.resize((size_t)(r.N * r.K));
            for (int64_t a = 0; a < r.N; ++a) for (int64_t k = 0; k < r.K; ++k) r.w[(size_t)(a * r.K + k)] = W.f[(size_t)(k * r.N + a)];
            if (!r.b.empty() && (int64_t)r.b.size() != r.N) bad(*bn, "bias length");
            r.x = mm->inputs[0];
        }
        if (want_bias == 1 && r.b.empty()) bad(*bn, std::string("the ") + role + " needs a bias");
        if (want_bias == 0 && !r.b.empty()) bad(*bn, std::string("the ") + role + " has no bias in the " + step);
        return r;
    }
    void two(const OnnxNode& bn) const { if (bn.inputs.size() != 2) bad(bn, "needs two inputs"); }
};

}  // namespace

// -------------------------------------------------------------------------------------------------
// Loop -> SLADecode.  The body contract, with h [B,H], pre [B] the loop-carried state and fea [B,HW,C] from the outer scope:
//   hp = Gemm(h, W_h2h, b_h2h, transB=1)        e = MatMul(Tanh(Add(MatMul(fea, W_i2h^T), Unsqueeze(hp, [1]))), w_score^T)
//   ctx = Squeeze(MatMul(Transpose(Softmax(e, axis=1), [0,2,1]), fea), [1])      x = Concat(ctx, OneHot(pre, V, [0,1]), axis=1)
//   xr,xz,xc = Split(Gemm(x, W_ih, b_ih, transB=1))   hr,hz,hc = Split(Gemm(h, W_hh, b_hh, transB=1))
//   r = Sigmoid(xr+hr)  z = Sigmoid(xz+hz)  c = Tanh(xc + r*hc)  h_new = (h - c)*z + c
//   logits = Gemm(Gemm(h_new, W_s1, b_s1), W_s2, b_s2)   loc = Sigmoid(Gemm(Gemm(h_new, W_l1, b_l1), W_l2, b_l2))   pre_new = ArgMax(logits, axis=1, keepdims=0)
// Tolerated: MatMul(x, W^T) + Add(bias) for a Gemm, Cast around OneHot / ArgMax, weights as body or outer initializers (or Constant
// nodes), axes as attribute or input, cond_out as Identity(cond_in) or a constant true.
void match_sla_loop(const GNode& loop, std::map<std::string, HostTensor>& inits, int64_t opset, GNode& lin_out, GNode& dec_out) {
    const std::string where = "Loop (" + (loop.out.empty() ? std::string("?") : loop.out[0]) + ")";
    auto bit = loop.attrs.find("body");
    if (bit == loop.attrs.end() || bit->second.kind != Attr::G || !bit->second.g) fail(OAR_UNSUPPORTED_OP, where + ": only the SLA decode step is supported as a Loop body: the node has no body graph");
    const OnnxModel& body = *bit->second.g;
    LoopBody LB(body, inits, where + ": only the SLA decode step is supported as a Loop body: ", "SLA step");
    auto& producer = LB.producer;
    auto& used = LB.used;
    using Lin = LoopBody::Lin;
    auto refuse = [&](const std::string& why) { LB.refuse(why); };
    auto cst = [&](const std::string& s) { return LB.cst(s); };
    auto node_desc = [&](int i) { return LB.node_desc(i); };
    auto expect = [&](const std::string& v, const char* op, const char* role) -> const OnnxNode& { return LB.expect(v, op, role); };
    auto bad = [&](const OnnxNode& bn, const std::string& why) { LB.bad(bn, why); };
    auto is_op = [&](const std::string& v, const char* op) { return LB.is_op(v, op); };
    auto strip_casts = [&](std::string v) { return LB.strip_casts(std::move(v)); };
    auto ints_arg = [&](const OnnxNode& bn, const char* attr, size_t input) { return LB.ints_arg(bn, attr, input); };
    auto lin = [&](const std::string& v, const char* role, bool want_bias) { return LB.lin(v, role, want_bias ? 1 : 0); };
    auto two = [&](const OnnxNode& bn) { LB.two(bn); };

    if (body.inputs.size() != 4 || body.outputs.size() != 5) refuse("the body must have the inputs (i, cond, h, pre) and the outputs (cond, h, pre, logits, loc)");
    if (loop.in.size() != 4 || loop.out.size() != 4) refuse("the node must carry (M, cond, h0, pre0) and yield (h, pre, logits scan, loc scan)");
    if (opset < 13) refuse("Softmax / Split / Squeeze semantics below opset 13");
    const std::string &cond_in = body.inputs[1], &h = body.inputs[2], &pre = body.inputs[3];
    const std::string &cond_out = body.outputs[0], &h_new = body.outputs[1], &pre_new = body.outputs[2], &logits = body.outputs[3], &loc = body.outputs[4];
    // trip count and condition
    const HostTensor* mt = loop.in[0].empty() ? nullptr : [&]() -> const HostTensor* { auto it = inits.find(loop.in[0]); return it == inits.end() ? nullptr : &it->second; }();
    if (!mt || mt->dtype == DType::F32 || mt->i.size() != 1) refuse("the trip count M must be a constant integer scalar");
    const int64_t M = mt->i[0];
    if (!loop.in[1].empty()) {
        auto it = inits.find(loop.in[1]);
        if (it == inits.end() || it->second.i.size() != 1 || it->second.i[0] == 0) refuse("the loop condition must be absent or a constant true");
    }
    if (const HostTensor* ct = cst(cond_out)) {
        if (ct->i.size() != 1 || ct->i[0] == 0) refuse("cond_out must be Identity(cond_in) or a constant true");
    } else {
        const OnnxNode& id = expect(cond_out, "Identity", "loop condition");
        if (id.inputs.size() != 1 || id.inputs[0] != cond_in) bad(id, "cond_out must be Identity(cond_in)");
    }
    // greedy token
    {
        const OnnxNode& am = expect(strip_casts(pre_new), "ArgMax", "next token");
        if (am.inputs.size() != 1 || am.inputs[0] != logits) bad(am, "ArgMax must read the logits output");
        const int64_t ax = am.ai("axis", 0);
        if ((ax != 1 && ax != -1) || am.ai("keepdims", 1) != 0 || am.ai("select_last_index", 0) != 0) bad(am, "ArgMax must be axis=1, keepdims=0, first index");
    }
    // heads
    Lin s2 = lin(logits, "structure head", true), s1 = lin(s2.x, "structure head hidden layer", true);
    const OnnxNode& lsig = expect(loc, "Sigmoid", "location output");
    Lin l2 = lin(lsig.inputs[0], "location head", true), l1 = lin(l2.x, "location head hidden layer", true);
    if (s1.x != h_new || l1.x != h_new) refuse("both heads must read the new hidden state '" + h_new + "'");
    // GRU cell: h_new = Add(Mul(Sub(h, c), z), c)
    const OnnxNode& hadd = expect(h_new, "Add", "new hidden state");
    two(hadd);
    const int mi = is_op(hadd.inputs[0], "Mul") ? 0 : 1;
    const std::string cval = hadd.inputs[1 - mi];
    const OnnxNode& hmul = expect(hadd.inputs[mi], "Mul", "(h - c) * z");
    two(hmul);
    const int si = is_op(hmul.inputs[0], "Sub") ? 0 : 1;
    const OnnxNode& hsub = expect(hmul.inputs[si], "Sub", "h - c");
    two(hsub);
    if (hsub.inputs[0] != h || hsub.inputs[1] != cval) bad(hsub, "must be Sub(h, c)");
    const std::string zval = hmul.inputs[1 - si];
    const OnnxNode& ctanh = expect(cval, "Tanh", "candidate state c");
    const OnnxNode& cadd = expect(ctanh.inputs[0], "Add", "xc + r * hc");
    two(cadd);
    const int cm = is_op(cadd.inputs[0], "Mul") ? 0 : 1;
    const OnnxNode& rmul = expect(cadd.inputs[cm], "Mul", "r * hc");
    two(rmul);
    const std::string xc_or = cadd.inputs[1 - cm];
    const int ri = is_op(rmul.inputs[0], "Sigmoid") ? 0 : 1;
    const OnnxNode& rsig = expect(rmul.inputs[ri], "Sigmoid", "reset gate r");
    const std::string hc_v = rmul.inputs[1 - ri];
    const OnnxNode& radd = expect(rsig.inputs[0], "Add", "xr + hr");
    two(radd);
    const OnnxNode& zsig = expect(zval, "Sigmoid", "update gate z");
    const OnnxNode& zadd = expect(zsig.inputs[0], "Add", "xz + hz");
    two(zadd);
    const OnnxNode& hsplit = expect(hc_v, "Split", "hidden-side gate split");
    const OnnxNode& xsplit = expect(xc_or, "Split", "input-side gate split");
    for (const OnnxNode* sp : {&hsplit, &xsplit}) {
        const int64_t ax = sp->ai("axis", 0);
        if (sp->outputs.size() != 3 || sp->inputs.empty() || (ax != 1 && ax != -1)) bad(*sp, "Split must cut axis 1 into three");
        std::vector<int64_t> parts = ints_arg(*sp, "split", 1);
        if (!parts.empty() && (parts.size() != 3 || parts[0] != parts[1] || parts[1] != parts[2])) bad(*sp, "Split must cut three equal parts");
    }
    auto pair_is = [&](const OnnxNode& a, const std::string& u, const std::string& v) { return (a.inputs[0] == u && a.inputs[1] == v) || (a.inputs[0] == v && a.inputs[1] == u); };
    if (&hsplit == &xsplit || hc_v != hsplit.outputs[2] || xc_or != xsplit.outputs[2]) bad(cadd, "the candidate must combine the third parts of the two splits");
    if (!pair_is(radd, xsplit.outputs[0], hsplit.outputs[0])) bad(radd, "must be xr + hr");
    if (!pair_is(zadd, xsplit.outputs[1], hsplit.outputs[1])) bad(zadd, "must be xz + hz");
    Lin hh = lin(hsplit.inputs[0], "hidden-side gates", true), ih = lin(xsplit.inputs[0], "input-side gates", true);
    if (hh.x != h) refuse("the hidden-side gates must read the loop state '" + h + "'");
    // x = Concat(ctx, OneHot(pre))
    const OnnxNode& cat = expect(ih.x, "Concat", "GRU input");
    if (cat.inputs.size() != 2 || (cat.ai("axis", 0) != 1 && cat.ai("axis", 0) != -1)) bad(cat, "must be Concat(ctx, one-hot, axis=1)");
    const OnnxNode& oh = expect(strip_casts(cat.inputs[1]), "OneHot", "previous-token encoding");
    if (oh.inputs.size() != 3 || strip_casts(oh.inputs[0]) != pre || oh.ai("axis", -1) != -1) bad(oh, "must be OneHot(pre, V, [0, 1]) on the last axis");
    const HostTensor *dep = cst(oh.inputs[1]), *ohv = cst(oh.inputs[2]);
    auto cval_of = [](const HostTensor* t, size_t i) { return t->dtype == DType::F32 ? (double)t->f[i] : (double)t->i[i]; };
    if (!dep || dep->numel() != 1 || !ohv || ohv->numel() != 2 || cval_of(ohv, 0) != 0.0 || cval_of(ohv, 1) != 1.0) bad(oh, "depth must be a constant and values [0, 1]");
    const int64_t V = (int64_t)cval_of(dep, 0);
    // ctx = Squeeze(MatMul(Transpose(Softmax(e, 1), [0,2,1]), fea), [1])
    const OnnxNode& sq = expect(cat.inputs[0], "Squeeze", "context vector");
    if (ints_arg(sq, "axes", 1) != std::vector<int64_t>{1}) bad(sq, "must squeeze axis 1");
    const OnnxNode& cmm = expect(sq.inputs[0], "MatMul", "attention-weighted sum");
    two(cmm);
    const std::string fea = cmm.inputs[1];
    if (producer.count(fea) || cst(fea) || fea == h || fea == pre) bad(cmm, "the features must come from the outer scope");
    const OnnxNode& tr = expect(cmm.inputs[0], "Transpose", "attention weights");
    if (tr.ais("perm") != std::vector<int64_t>{0, 2, 1}) bad(tr, "must be perm [0, 2, 1]");
    const OnnxNode& sm = expect(tr.inputs[0], "Softmax", "attention weights");
    if (sm.ai("axis", -1) != 1) bad(sm, "must be Softmax over axis 1");
    Lin sc = lin(sm.inputs[0], "attention score", false);
    const OnnxNode& ttanh = expect(sc.x, "Tanh", "attention activation");
    const OnnxNode& tadd = expect(ttanh.inputs[0], "Add", "projected features + projected state");
    two(tadd);
    const int ui = is_op(tadd.inputs[0], "Unsqueeze") ? 0 : 1;
    const OnnxNode& un = expect(tadd.inputs[ui], "Unsqueeze", "projected state");
    if (ints_arg(un, "axes", 1) != std::vector<int64_t>{1}) bad(un, "must unsqueeze axis 1");
    Lin h2h = lin(un.inputs[0], "state projection", true);
    if (h2h.x != h) refuse("the state projection must read the loop state '" + h + "'");
    Lin i2h = lin(tadd.inputs[1 - ui], "feature projection", false);
    if (i2h.x != fea) refuse("the feature projection and the weighted sum must read the same features");
    for (int i = 0; i < (int)body.nodes.size(); ++i)
        if (!used[i]) refuse(node_desc(i) + " does not fit: it is not part of the SLA decode step");
    // dimensions
    const int64_t H = h2h.N, C = i2h.K, L = l2.N;
    auto shape_ok = h2h.K == H && i2h.N == H && sc.N == 1 && sc.K == H && hh.N == 3 * H && hh.K == H && ih.N == 3 * H && ih.K == C + V && s1.N == H && s1.K == H &&
                    s2.N == V && s2.K == H && l1.N == H && l1.K == H && l2.K == H;
    if (!shape_ok) refuse("the weights do not have the shapes of an SLA step with H = " + std::to_string(H) + ", C = " + std::to_string(C) + ", V = " + std::to_string(V));
    if (!k::sla_decode_supported(1, (int)std::min<int64_t>(C, 1 << 20), (int)std::min<int64_t>(H, 1 << 20), (int)std::min<int64_t>(V, 1 << 20), (int)std::min<int64_t>(L, 1 << 20),
                                 (int)std::min<int64_t>(std::max<int64_t>(M, 0), 1 << 20)))
        refuse("H = " + std::to_string(H) + ", C = " + std::to_string(C) + ", V = " + std::to_string(V) + ", L = " + std::to_string(L) + ", M = " + std::to_string(M) + " is outside H <= " +
               std::to_string(k::kSlaMaxH) + ", C <= " + std::to_string(k::kSlaMaxC) + ", V <= " + std::to_string(k::kSlaMaxV) + ", 1 <= L <= " + std::to_string(k::kSlaMaxL) + ", 1 <= M <= " +
               std::to_string(k::kSlaMaxM));
    // constants in the kernel's layout (kernels.h: SlaDecodeP): rows padded to a multiple of four floats
    const std::string pfx = "sla::" + loop.out[2] + "::";
    auto put = [&](const char* nm, std::vector<int64_t> dims, std::vector<float> v) {
        HostTensor t; t.name = pfx + nm; t.dtype = DType::F32; t.dims = std::move(dims); t.f = std::move(v);
        const std::string key = t.name;
        inits[key] = std::move(t);
        return key;
    };
    auto padded = [](const std::vector<const std::vector<float>*>& mats, int64_t col0, int64_t cols, int64_t ld) {   // rows of several [.][ld] matrices, columns [col0, col0 + cols) -> [rows][pad4(cols)]
        const int64_t Kp = (cols + 3) / 4 * 4;
        std::vector<float> o;
        for (auto* m : mats) {
            const int64_t rows = (int64_t)m->size() / ld;
            for (int64_t r = 0; r < rows; ++r) {
                for (int64_t c = 0; c < Kp; ++c) o.push_back(c < cols ? (*m)[(size_t)(r * ld + col0 + c)] : 0.0f);
            }
        }
        return o;
    };
    auto cat2 = [](const std::vector<float>& a, const std::vector<float>& b) { std::vector<float> o(a); o.insert(o.end(), b.begin(), b.end()); return o; };
    const int64_t Hp = (H + 3) / 4 * 4, Cp = (C + 3) / 4 * 4;
    std::vector<float> wi2h((size_t)(C * H));   // [C][H]: the Linear node's B
    for (int64_t c = 0; c < C; ++c) for (int64_t a = 0; a < H; ++a) wi2h[(size_t)(c * H + a)] = i2h.w[(size_t)(a * C + c)];
    std::vector<float> ihv((size_t)(V * 3 * H));   // [V][3H] = W_ih[:, C:]^T
    for (int64_t v = 0; v < V; ++v) for (int64_t r = 0; r < 3 * H; ++r) ihv[(size_t)(v * 3 * H + r)] = ih.w[(size_t)(r * (C + V) + C + v)];
    lin_out = GNode();
    lin_out.op = "Linear";
    lin_out.in = {fea, put("w_i2h", {C, H}, wi2h)};
    lin_out.out = {pfx + "proj"};
    dec_out = GNode();
    dec_out.op = "SLADecode";
    dec_out.in = {fea, lin_out.out[0], loop.in[2], loop.in[3],
                  put("w_h4", {4 * H, Hp}, padded({&h2h.w, &hh.w}, 0, H, H)), put("b_h4", {4 * H}, cat2(h2h.b, hh.b)), put("w_score", {Hp}, padded({&sc.w}, 0, H, H)),
                  put("w_ihc", {3 * H, Cp}, padded({&ih.w}, 0, C, C + V)), put("w_ihv", {V, 3 * H}, ihv), put("b_ih", {3 * H}, ih.b),
                  put("w_sl1", {2 * H, Hp}, padded({&s1.w, &l1.w}, 0, H, H)), put("b_sl1", {2 * H}, cat2(s1.b, l1.b)),
                  put("w_s2", {V, Hp}, padded({&s2.w}, 0, H, H)), put("b_s2", {V}, s2.b), put("w_l2", {L, Hp}, padded({&l2.w}, 0, H, H)), put("b_l2", {L}, l2.b)};
    dec_out.out = loop.out;
    auto iattr = [&](const char* k, int64_t v) { Attr a; a.kind = Attr::I; a.i = v; dec_out.attrs[k] = a; };
    iattr("steps", M); iattr("hidden", H); iattr("channels", C); iattr("vocab", V); iattr("loc", L);
}

// -------------------------------------------------------------------------------------------------
// Loop -> FormulaDecode.  The body contract: the greedy step of a pre-norm (MBart-order) transformer decoder with a key / value cache.
// Carried: tok [B] int64, then K_l [B, nh, t, dq], V_l [B, nh, t, dh] per layer; from the outer scope KmT_l [B, nh, dh, S] and Vm_l [B, nh, S, dh].
// Squeeze attention (UniMERNet's MBart decoder): the SELF-attention queries and keys may be narrower than the values, Wq / Wk [nh dq, D] with 1 <= dq <= 128,
// their Reshape targets [B, nh, 1, dq]; dq == dh is the plain head.  The cross attention is never squeezed.
//   x = LN_emb(Gather(E_tok, tok) * s_emb + Gather(E_pos, i + c_pos))
//   per layer:  y = LN1(x); q = lin(y) * dh^-0.5, k = lin(y), v = lin(y), each Reshape to [B, nh, 1, dh];  K' = Concat(K, k, 2), V' = Concat(V, v, 2)
//               x = x + lin(Reshape(MatMul(Softmax(MatMul(q, Transpose(K', [0,1,3,2]))), V'), [B, D]))
//               x = x + lin(Reshape(MatMul(Softmax(MatMul(Reshape(lin(LN2(x)) * dh^-0.5), KmT)), Vm), [B, D]))
//               x = x + lin(Gelu(lin(LN3(x))))
//   logits = lin(LN_f(x));  tok_new = ArgMax(logits, 1);  outputs (cond, tok_new, K_1', V_1', ..., scan tok_new [, scan logits])
// Tolerated: Gemm(transB=1) or MatMul [+ Add]; the query scale as a Mul on either side of the bias Add or absent; weights as body / outer constants;
// commuted Add / Mul; Cast around the Gather indices and the ArgMax; constant Reshape targets with 0 / -1 entries.
namespace {

// The formula decode step's matcher: the helpers of this body, and match(), which walks the body from its outputs back to the embedding.
struct FormulaBody {
    LoopBody& L;
    const OnnxModel& body;
    using Lin = LoopBody::Lin;
    struct LN { std::string x; std::vector<float> g, b; float eps; };
    struct Layer { LN ln1, ln2, ln3; Lin q, k, v, o, cq, co, f1, f2; int qm = 0, cqm = 0; float qs = 1.f, cqs = 1.f; std::string kmT, vm; };
    int64_t D = 0, nh = 0, dh = 0, dq = 0;
    bool scalar_f(const std::string& v, float& out) {
        const HostTensor* t = L.cst(v);
        if (!t || t->dtype != DType::F32 || t->f.size() != 1) return false;
        out = t->f[0];
        return true;
    }
    LN layer_norm(const std::string& v, const char* role) {
        const OnnxNode& n = L.expect(v, "LayerNormalization", role);
        if (n.inputs.size() != 3 || n.inputs[2].empty()) L.bad(n, "LayerNormalization needs a scale and a bias");
        const int64_t ax = n.ai("axis", -1);
        if (ax != -1 && ax != 1) L.bad(n, "LayerNormalization must normalise the last axis");
        LN r;
        r.x = n.inputs[0]; r.g = L.f32c(n, n.inputs[1], 1).f; r.b = L.f32c(n, n.inputs[2], 1).f; r.eps = n.af("epsilon", 1e-5f);
        if (r.g.size() != r.b.size()) L.bad(n, "scale and bias lengths differ");
        return r;
    }
    // is `v` the output of a lin (Gemm, MatMul by a constant, or Add of one and a constant)?
    bool const_matmul(const std::string& v) { auto it = L.producer.find(v); return it != L.producer.end() && body.nodes[it->second].op == "MatMul" && body.nodes[it->second].inputs.size() == 2 && L.cst(body.nodes[it->second].inputs[1]); }
    bool is_lin(const std::string& v) {
        if (L.is_op(v, "Gemm") || const_matmul(v)) return true;
        if (!L.is_op(v, "Add")) return false;
        const OnnxNode& a = body.nodes[L.producer[v]];
        return a.inputs.size() == 2 && ((const_matmul(a.inputs[0]) && L.cst(a.inputs[1])) || (const_matmul(a.inputs[1]) && L.cst(a.inputs[0])));
    }
    // v = Add(residual, lin(..)) in either order
    Lin residual(const std::string& v, const char* role, std::string& res) {
        const OnnxNode& a = L.expect(v, "Add", role);
        L.two(a);
        const int li = is_lin(a.inputs[1]) ? 1 : is_lin(a.inputs[0]) ? 0 : -1;
        if (li < 0) L.bad(a, std::string("the ") + role + " must add a Gemm or MatMul [+ Add] to the residual");
        res = a.inputs[1 - li];
        return L.lin(a.inputs[li], role, 1);
    }
    // a projection with the query scale: mode 0 none, 1 (x W^T + b) * s, 2 (x W^T) * s + b
    Lin scaled_lin(const std::string& v, const char* role, int& mode, float& scale) {
        mode = 0; scale = 1.0f;
        if (L.is_op(v, "Mul")) {
            const OnnxNode& m = L.expect(v, "Mul", role);
            L.two(m);
            const int ci = scalar_f(m.inputs[1], scale) ? 1 : scalar_f(m.inputs[0], scale) ? 0 : -1;
            if (ci < 0) L.bad(m, "the query scale must be a constant scalar");
            mode = 1;
            return L.lin(m.inputs[1 - ci], role, 1);
        }
        if (L.is_op(v, "Add")) {
            const OnnxNode& a = body.nodes[L.producer[v]];
            L.two(a);
            const int mi = L.is_op(a.inputs[0], "Mul") ? 0 : L.is_op(a.inputs[1], "Mul") ? 1 : -1;
            if (mi >= 0) {
                L.used[L.producer[v]] = true;
                const OnnxNode& m = L.expect(a.inputs[mi], "Mul", role);
                L.two(m);
                const int ci = scalar_f(m.inputs[1], scale) ? 1 : scalar_f(m.inputs[0], scale) ? 0 : -1;
                if (ci < 0) L.bad(m, "the query scale must be a constant scalar");
                Lin r = L.lin(m.inputs[1 - ci], role, 0);
                const HostTensor& b = L.f32c(a, a.inputs[1 - mi], 1);
                if ((int64_t)b.f.size() != r.N) L.bad(a, "bias length");
                r.b = b.f;
                mode = 2;
                return r;
            }
        }
        return L.lin(v, role, 1);
    }
    std::vector<int64_t> reshape_target(const OnnxNode& n) {
        if (n.inputs.size() < 2) L.bad(n, "Reshape needs a constant target");
        const HostTensor* t = L.cst(n.inputs[1]);
        if (!t || t->dtype == DType::F32 || t->i.empty()) L.bad(n, "the Reshape target must be a constant");
        return t->i;
    }
    // v = Reshape(u, [B, nh, 1, dh]): returns u.  kind 0: a value / cross-attention projection, nh x dh = D.  kind 1: the cross-attention query, the same, with
    // a word on squeeze attention where the product is not D.  kind 2: the self-attention query / key, [B, nh, 1, dq] with its own head size (squeeze attention:
    // dq need not be dh; an entry <= 0 is inferred from D as for the others)
    std::string split_heads(const std::string& v, const char* role, int kind = 0) {
        const OnnxNode& n = L.expect(v, "Reshape", role);
        std::vector<int64_t> t = reshape_target(n);
        if (t.size() != 4 || t[2] != 1) L.bad(n, "must reshape to [B, heads, 1, head size]");
        int64_t a = t[1], b = t[3];
        const bool explicit_qk = kind == 2 && a > 0 && b > 0;
        if (a <= 0 && b > 0 && D % b == 0) a = D / b;
        if (b <= 0 && a > 0 && D % a == 0) b = D / a;
        if (a <= 0 || b <= 0 || (a * b != D && !explicit_qk))
            L.bad(n, "heads x head size must be the model width " + std::to_string(D) +
                         (kind == 1 && a > 0 && b > 0 ? " (the cross-attention query is " + std::to_string(a * b) + " wide: squeeze attention is supported in the self-attention only)" : std::string()));
        if (nh == 0) { nh = a; dh = b; }
        if (kind == 2) {
            if (dq == 0) dq = b;
            if (a != nh || b != dq) L.bad(n, "every projection must split into the same heads");
        } else if (a != nh || b != dh) L.bad(n, "every projection must split into the same heads");
        return n.inputs[0];
    }
    // v = Reshape(MatMul(Softmax(MatMul(q4, keys), -1), values), [B, D]): returns q4 / keys / values
    void attention(const std::string& v, const char* role, std::string& q4, std::string& keys, std::string& values) {
        const OnnxNode& rs = L.expect(v, "Reshape", role);
        std::vector<int64_t> t = reshape_target(rs);
        if (t.size() != 2 || (t[1] != D && t[1] != -1)) L.bad(rs, "must reshape the attention output to [B, " + std::to_string(D) + "]");
        const OnnxNode& pv = L.expect(rs.inputs[0], "MatMul", "attention-weighted sum");
        L.two(pv);
        values = pv.inputs[1];
        const OnnxNode& sm = L.expect(pv.inputs[0], "Softmax", "attention weights");
        const int64_t ax = sm.ai("axis", -1);
        if (ax != -1 && ax != 3) L.bad(sm, "must be Softmax over the last axis");
        const OnnxNode& qk = L.expect(sm.inputs[0], "MatMul", "attention scores");
        L.two(qk);
        q4 = qk.inputs[0]; keys = qk.inputs[1];
    }
    void check_empty_caches(const GNode& loop, const std::vector<GNode>& outer_nodes, const std::map<std::string, HostTensor>& inits, const std::set<std::string>& graph_outs,
                            size_t n_state, std::vector<std::string>& dropped_inputs);
    void match(const GNode& loop, const std::vector<GNode>& outer_nodes, std::map<std::string, HostTensor>& inits, int64_t opset, const std::set<std::string>& graph_outs,
               GNode& dec_out, std::vector<std::string>& dropped_inputs);
};

// initial state: every cache starts empty, and nothing else may read it or the final caches
void FormulaBody::check_empty_caches(const GNode& loop, const std::vector<GNode>& outer_nodes, const std::map<std::string, HostTensor>& inits, const std::set<std::string>& graph_outs,
                                     size_t n_state, std::vector<std::string>& dropped_inputs) {
    auto producer_of = [&](const std::string& v) -> const GNode* {
        for (const GNode& n : outer_nodes) for (auto& o : n.out) if (o == v) return &n;
        return nullptr;
    };
    for (size_t c = 3; c < loop.in.size(); ++c) {
        const std::string& nm = loop.in[c];
        bool empty = false;
        auto it = inits.find(nm);
        if (it != inits.end()) empty = it->second.dims.size() == 4 && it->second.dims[2] == 0;
        else if (const GNode* cs = producer_of(nm)) {
            const GNode* cat = cs->op == "ConstantOfShape" && cs->in.size() == 1 ? producer_of(cs->in[0]) : nullptr;
            if (cat && cat->op == "Concat" && cat->in.size() == 4) {
                auto z = inits.find(cat->in[2]);
                empty = z != inits.end() && z->second.dtype != DType::F32 && z->second.i.size() == 1 && z->second.i[0] == 0;
            }
        }
        if (!empty) L.refuse("the initial cache '" + nm + "' must be empty: an initializer with dims[2] == 0, or ConstantOfShape over a Concat whose third element is the constant 0");
        int readers = 0;
        for (const GNode& n : outer_nodes) for (auto& s : n.in) if (s == nm) ++readers;
        if (readers != 1 || graph_outs.count(nm) != 0) L.refuse("the initial cache '" + nm + "' is read outside the Loop");
        dropped_inputs.push_back(nm);
    }
    for (size_t c = 1; c < n_state; ++c) {
        const std::string& nm = loop.out[c];
        if (nm.empty()) continue;
        bool read = graph_outs.count(nm) != 0;
        for (const GNode& n : outer_nodes) for (auto& s : n.in) if (s == nm) read = true;
        if (read) L.refuse("the final cache '" + nm + "' is read by the rest of the graph: the caches are not produced");
    }
}

void FormulaBody::match(const GNode& loop, const std::vector<GNode>& outer_nodes, std::map<std::string, HostTensor>& inits, int64_t opset, const std::set<std::string>& graph_outs,
                        GNode& dec_out, std::vector<std::string>& dropped_inputs) {
    const int64_t Ld = ((int64_t)body.inputs.size() - 3) / 2;
    const size_t n_state = (size_t)(1 + 2 * Ld);
    if (Ld < 1 || Ld > k::kFdMaxLayers) L.refuse("the body carries " + std::to_string(Ld) + " layers of caches, outside 1 <= Ld <= " + std::to_string(k::kFdMaxLayers));
    const bool with_logits = body.outputs.size() == n_state + 3;
    if (body.outputs.size() != n_state + 2 && !with_logits) L.refuse("the body must yield (cond, tok, K_1', V_1', ..., scan tok [, scan logits])");
    if (loop.in.size() != 2 + n_state || loop.out.size() != body.outputs.size() - 1) L.refuse("the node must carry (M, cond, tok0, K_1, V_1, ...) and yield (tok, K_1, V_1, ..., tok scan [, logits scan])");
    if (opset < 17) L.refuse("LayerNormalization needs opset 17");
    const std::string &iter = body.inputs[0], &cond_in = body.inputs[1], &tok = body.inputs[2];
    const std::string &cond_out = body.outputs[0], &tok_new = body.outputs[1];
    if (body.outputs[n_state + 1] != tok_new) L.refuse("the first scan output must be the new token '" + tok_new + "'");
    // trip count and condition
    const HostTensor* mt = nullptr;
    if (!loop.in[0].empty()) { auto it = inits.find(loop.in[0]); if (it != inits.end()) mt = &it->second; }
    if (!mt || mt->dtype == DType::F32 || mt->i.size() != 1) L.refuse("the trip count M must be a constant integer scalar");
    const int64_t M = mt->i[0];
    if (!loop.in[1].empty()) {
        auto it = inits.find(loop.in[1]);
        if (it == inits.end() || it->second.i.size() != 1 || it->second.i[0] == 0) L.refuse("the loop condition must be absent or a constant true");
    }
    if (const HostTensor* ct = L.cst(cond_out)) {
        if (ct->i.size() != 1 || ct->i[0] == 0) L.refuse("cond_out must be Identity(cond_in) or a constant true");
    } else {
        const OnnxNode& id = L.expect(cond_out, "Identity", "loop condition");
        if (id.inputs.size() != 1 || id.inputs[0] != cond_in) L.bad(id, "cond_out must be Identity(cond_in)");
    }
    // greedy token and output projection
    const OnnxNode& am = L.expect(L.strip_casts(tok_new), "ArgMax", "next token");
    {
        const int64_t ax = am.ai("axis", 0);
        if (am.inputs.size() != 1 || (ax != 1 && ax != -1) || am.ai("keepdims", 1) != 0 || am.ai("select_last_index", 0) != 0) L.bad(am, "ArgMax must be axis=1, keepdims=0, first index");
    }
    const std::string logits = am.inputs[0];
    if (with_logits && body.outputs[n_state + 2] != logits) L.refuse("the second scan output must be the logits '" + logits + "' the ArgMax reads");
    Lin lm = L.lin(logits, "output projection", -1);
    LN lnf = layer_norm(lm.x, "final LayerNorm");
    D = lm.K;
    const int64_t V = lm.N;
    if ((int64_t)lnf.g.size() != D) L.refuse("the final LayerNorm does not have the model width " + std::to_string(D));
    std::vector<Layer> layers((size_t)Ld);
    std::string x = lnf.x;
    int64_t F = 0;
    for (int64_t l = Ld - 1; l >= 0; --l) {
        Layer& Y = layers[(size_t)l];
        const std::string &Kin = body.inputs[(size_t)(3 + 2 * l)], &Vin = body.inputs[(size_t)(4 + 2 * l)];
        const std::string &Kout = body.outputs[(size_t)(2 + 2 * l)], &Vout = body.outputs[(size_t)(3 + 2 * l)];
        std::string x2, x1, x0;
        // feed-forward
        Y.f2 = residual(x, "feed-forward output", x2);
        const OnnxNode& ge = L.expect(Y.f2.x, "Gelu", "feed-forward activation");
        if (ge.as("approximate", "none") != "none") L.bad(ge, "Gelu must be approximate = none");
        Y.f1 = L.lin(ge.inputs[0], "feed-forward input", 1);
        Y.ln3 = layer_norm(Y.f1.x, "feed-forward LayerNorm");
        if (Y.ln3.x != x2) L.refuse("layer " + std::to_string(l + 1) + ": the feed-forward block must normalise its own residual '" + x2 + "'");
        // cross attention
        Y.co = residual(x2, "cross-attention output", x1);
        std::string q4, keys, values;
        attention(Y.co.x, "cross-attention output", q4, keys, values);
        for (const std::string* m : {&keys, &values})
            if (L.producer.count(*m) || L.cst(*m) || std::find(body.inputs.begin(), body.inputs.end(), *m) != body.inputs.end()) L.refuse("layer " + std::to_string(l + 1) + ": the memory keys / values '" + *m + "' must come from the outer scope");
        Y.kmT = keys; Y.vm = values;
        Y.cq = scaled_lin(split_heads(q4, "cross-attention query", 1), "cross-attention query", Y.cqm, Y.cqs);
        Y.ln2 = layer_norm(Y.cq.x, "cross-attention LayerNorm");
        if (Y.ln2.x != x1) L.refuse("layer " + std::to_string(l + 1) + ": the cross-attention block must normalise its own residual '" + x1 + "'");
        // self attention over the cache
        Y.o = residual(x1, "self-attention output", x0);
        attention(Y.o.x, "self-attention output", q4, keys, values);
        const OnnxNode& kt = L.expect(keys, "Transpose", "cached keys");
        if (kt.ais("perm") != std::vector<int64_t>{0, 1, 3, 2} || kt.inputs[0] != Kout) L.bad(kt, "must be Transpose(K', [0, 1, 3, 2]) of the new key cache '" + Kout + "'");
        if (values != Vout) L.refuse("layer " + std::to_string(l + 1) + ": the self-attention values must be the new value cache '" + Vout + "'");
        const OnnxNode& kcat = L.expect(Kout, "Concat", "new key cache");
        const OnnxNode& vcat = L.expect(Vout, "Concat", "new value cache");
        if (kcat.inputs.size() != 2 || kcat.ai("axis", 0) != 2 || kcat.inputs[0] != Kin) L.bad(kcat, "must be Concat('" + Kin + "', k, axis=2)");
        if (vcat.inputs.size() != 2 || vcat.ai("axis", 0) != 2 || vcat.inputs[0] != Vin) L.bad(vcat, "must be Concat('" + Vin + "', v, axis=2)");
        Y.q = scaled_lin(split_heads(q4, "self-attention query", 2), "self-attention query", Y.qm, Y.qs);
        Y.k = L.lin(split_heads(kcat.inputs[1], "self-attention key", 2), "self-attention key", 1);
        if (Y.q.N != Y.k.N) L.refuse("layer " + std::to_string(l + 1) + ": the self-attention keys have " + std::to_string(Y.k.N) + " columns, the queries " + std::to_string(Y.q.N) + ": Wq and Wk must have the same row count");
        Y.v = L.lin(split_heads(vcat.inputs[1], "self-attention value"), "self-attention value", 1);
        Y.ln1 = layer_norm(Y.q.x, "self-attention LayerNorm");
        if (Y.k.x != Y.q.x || Y.v.x != Y.q.x || Y.ln1.x != x0) L.refuse("layer " + std::to_string(l + 1) + ": q, k and v must read LN1 of the block's residual '" + x0 + "'");
        if (l == Ld - 1) F = Y.f1.N;
        auto shp = [&](const Lin& a, int64_t N, int64_t K) { return a.N == N && a.K == K; };
        if (!(shp(Y.q, nh * dq, D) && shp(Y.k, nh * dq, D) && shp(Y.v, D, D) && shp(Y.o, D, D) && shp(Y.cq, D, D) && shp(Y.co, D, D) && shp(Y.f1, F, D) && shp(Y.f2, D, F) &&
              (int64_t)Y.ln1.g.size() == D && (int64_t)Y.ln2.g.size() == D && (int64_t)Y.ln3.g.size() == D))
            L.refuse("layer " + std::to_string(l + 1) + ": the weights do not have the shapes of a decoder layer with D = " + std::to_string(D) + ", F = " + std::to_string(F));
        x = x0;
    }
    // embedding: x = LN_emb(Gather(E_tok, tok) * s_emb + Gather(E_pos, i + c_pos))
    LN lne = layer_norm(x, "embedding LayerNorm");
    const OnnxNode& eadd = L.expect(lne.x, "Add", "token + position embedding");
    L.two(eadd);
    const int mi = L.is_op(eadd.inputs[0], "Mul") ? 0 : 1;
    const OnnxNode& emul = L.expect(eadd.inputs[mi], "Mul", "scaled token embedding");
    L.two(emul);
    float s_emb = 1.0f;
    const int sci = scalar_f(emul.inputs[1], s_emb) ? 1 : scalar_f(emul.inputs[0], s_emb) ? 0 : -1;
    if (sci < 0) L.bad(emul, "the embedding scale must be a constant scalar");
    const OnnxNode& gt = L.expect(emul.inputs[1 - sci], "Gather", "token embedding");
    const OnnxNode& gp = L.expect(eadd.inputs[1 - mi], "Gather", "position embedding");
    if (gt.inputs.size() != 2 || gt.ai("axis", 0) != 0 || L.strip_casts(gt.inputs[1]) != tok) L.bad(gt, "must be Gather(E_tok, tok) on axis 0");
    if (gp.inputs.size() != 2 || gp.ai("axis", 0) != 0) L.bad(gp, "must be Gather(E_pos, i + c_pos) on axis 0");
    const HostTensor& Et = L.f32c(gt, gt.inputs[0], 2);
    const HostTensor& Ep = L.f32c(gp, gp.inputs[0], 2);
    int64_t c_pos = 0;
    {
        const std::string pi = L.strip_casts(gp.inputs[1]);
        if (pi != iter) {
            const OnnxNode& pa = L.expect(pi, "Add", "position index");
            L.two(pa);
            const int ii = L.strip_casts(pa.inputs[0]) == iter ? 0 : L.strip_casts(pa.inputs[1]) == iter ? 1 : -1;
            const HostTensor* c = ii < 0 ? nullptr : L.cst(pa.inputs[1 - ii]);
            if (!c || c->dtype == DType::F32 || c->i.size() != 1) L.bad(pa, "must be Add(i, c_pos) with a constant integer c_pos");
            c_pos = c->i[0];
        }
    }
    for (int i = 0; i < (int)body.nodes.size(); ++i)
        if (!L.used[i]) L.refuse(L.node_desc(i) + " does not fit: it is not part of the formula decode step");
    const int64_t P = Ep.dims[0];
    if (Et.dims[0] != V || Et.dims[1] != D || Ep.dims[1] != D || (int64_t)lne.g.size() != D || (!lm.b.empty() && (int64_t)lm.b.size() != V))
        L.refuse("the embeddings and the output projection do not agree on V = " + std::to_string(V) + ", D = " + std::to_string(D));
    auto cl = [](int64_t v) { return (int)std::min<int64_t>(std::max<int64_t>(v, 0), 1 << 26); };
    if (dq < 1 || dq > k::kFdMaxDh || nh * dq > k::kFdMaxD)
        L.refuse("the self-attention queries and keys have head size " + std::to_string(dq) + " in " + std::to_string(nh) + " heads, outside 1 <= dq <= " + std::to_string(k::kFdMaxDh) + ", heads x dq <= " + std::to_string(k::kFdMaxD));
    if (nh < 1 || !k::formula_decode_supported(cl(D), cl(nh), cl(F), cl(V), cl(Ld), cl(M), 1, cl(dq)) || c_pos < 0 || M + c_pos > P)
        L.refuse("D = " + std::to_string(D) + ", heads = " + std::to_string(nh) + ", F = " + std::to_string(F) + ", V = " + std::to_string(V) + ", Ld = " + std::to_string(Ld) + ", M = " + std::to_string(M) +
                 ", c_pos = " + std::to_string(c_pos) + ", P = " + std::to_string(P) + " is outside D <= " + std::to_string(k::kFdMaxD) + ", head size <= " + std::to_string(k::kFdMaxDh) + ", F <= " +
                 std::to_string(k::kFdMaxF) + ", 2 <= V < 2^24, 1 <= M <= " + std::to_string(k::kFdMaxM) + ", M + c_pos <= P");
    check_empty_caches(loop, outer_nodes, inits, graph_outs, n_state, dropped_inputs);
    // constants in the kernels' layout (kernels.h: FormulaDecodeP): matrix rows padded to a multiple of four floats
    const std::string pfx = "fd::" + loop.out[n_state] + "::";
    auto put = [&](const std::string& nm, std::vector<int64_t> dims, std::vector<float> v) {
        HostTensor t; t.name = pfx + nm; t.dtype = DType::F32; t.dims = std::move(dims); t.f = std::move(v);
        const std::string key = t.name;
        inits[key] = std::move(t);
        return key;
    };
    auto padded = [](const std::vector<const Lin*>& mats) {
        const int64_t K = mats[0]->K, Kp = (K + 3) / 4 * 4;
        std::vector<float> o;
        for (const Lin* m : mats)
            for (int64_t r = 0; r < m->N; ++r)
                for (int64_t c = 0; c < Kp; ++c) o.push_back(c < K ? m->w[(size_t)(r * K + c)] : 0.0f);
        return o;
    };
    auto cat3 = [](const std::vector<float>& a, const std::vector<float>& b, const std::vector<float>& c) { std::vector<float> o(a); o.insert(o.end(), b.begin(), b.end()); o.insert(o.end(), c.begin(), c.end()); return o; };
    const int64_t Dp = (D + 3) / 4 * 4, Fp = (F + 3) / 4 * 4, Dq = nh * dq;
    dec_out = GNode();
    dec_out.op = "FormulaDecode";
    dec_out.in = {loop.in[2]};
    for (auto& Y : layers) { dec_out.in.push_back(Y.kmT); dec_out.in.push_back(Y.vm); }
    dec_out.in.push_back(put("e_tok", {V, D}, Et.f));
    dec_out.in.push_back(put("e_pos", {P, D}, Ep.f));
    dec_out.in.push_back(put("lne_g", {D}, lne.g));
    dec_out.in.push_back(put("lne_b", {D}, lne.b));
    auto iattr = [&](const std::string& k, int64_t v) { Attr a; a.kind = Attr::I; a.i = v; dec_out.attrs[k] = a; };
    auto fattr = [&](const std::string& k, float v) { Attr a; a.kind = Attr::F; a.f = v; dec_out.attrs[k] = a; };
    for (size_t l = 0; l < layers.size(); ++l) {
        Layer& Y = layers[l];
        const std::string s = "l" + std::to_string(l) + "_";
        dec_out.in.push_back(put(s + "ln1_g", {D}, Y.ln1.g)); dec_out.in.push_back(put(s + "ln1_b", {D}, Y.ln1.b));
        dec_out.in.push_back(put(s + "w_qkv", {2 * Dq + D, Dp}, padded({&Y.q, &Y.k, &Y.v}))); dec_out.in.push_back(put(s + "b_qkv", {2 * Dq + D}, cat3(Y.q.b, Y.k.b, Y.v.b)));
        dec_out.in.push_back(put(s + "w_o", {D, Dp}, padded({&Y.o}))); dec_out.in.push_back(put(s + "b_o", {D}, Y.o.b));
        dec_out.in.push_back(put(s + "ln2_g", {D}, Y.ln2.g)); dec_out.in.push_back(put(s + "ln2_b", {D}, Y.ln2.b));
        dec_out.in.push_back(put(s + "w_cq", {D, Dp}, padded({&Y.cq}))); dec_out.in.push_back(put(s + "b_cq", {D}, Y.cq.b));
        dec_out.in.push_back(put(s + "w_co", {D, Dp}, padded({&Y.co}))); dec_out.in.push_back(put(s + "b_co", {D}, Y.co.b));
        dec_out.in.push_back(put(s + "ln3_g", {D}, Y.ln3.g)); dec_out.in.push_back(put(s + "ln3_b", {D}, Y.ln3.b));
        dec_out.in.push_back(put(s + "w_1", {F, Dp}, padded({&Y.f1}))); dec_out.in.push_back(put(s + "b_1", {F}, Y.f1.b));
        dec_out.in.push_back(put(s + "w_2", {D, Fp}, padded({&Y.f2}))); dec_out.in.push_back(put(s + "b_2", {D}, Y.f2.b));
        fattr(s + "eps1", Y.ln1.eps); fattr(s + "eps2", Y.ln2.eps); fattr(s + "eps3", Y.ln3.eps);
        iattr(s + "q_mode", Y.qm); fattr(s + "q_scale", Y.qs); iattr(s + "cq_mode", Y.cqm); fattr(s + "cq_scale", Y.cqs);
        Y = Layer();   // (the repacked copies are in inits now)
    }
    dec_out.in.push_back(put("lnf_g", {D}, lnf.g));
    dec_out.in.push_back(put("lnf_b", {D}, lnf.b));
    dec_out.in.push_back(put("w_lm", {V, Dp}, padded({&lm})));
    if (!lm.b.empty()) dec_out.in.push_back(put("b_lm", {V}, lm.b));
    dec_out.out = {loop.out[0], loop.out[n_state]};
    if (with_logits) dec_out.out.push_back(loop.out[n_state + 1]);
    iattr("steps", M); iattr("layers", Ld); iattr("width", D); iattr("heads", nh); iattr("ffn", F); iattr("vocab", V); iattr("positions", P); iattr("c_pos", c_pos);
    iattr("lm_bias", lm.b.empty() ? 0 : 1);
    if (dq != dh) iattr("qk_head", dq);   // (squeeze attention; absent: the head size)
    fattr("s_emb", s_emb); fattr("eps_e", lne.eps); fattr("eps_f", lnf.eps);
}

}  // namespace

void match_formula_loop(const GNode& loop, const std::vector<GNode>& outer_nodes, std::map<std::string, HostTensor>& inits, int64_t opset,
                        const std::set<std::string>& graph_outs, GNode& dec_out, std::vector<std::string>& dropped_inputs) {
    const std::string where = "Loop (" + (loop.out.empty() ? std::string("?") : loop.out[0]) + ")";
    const OnnxModel& body = *loop.attrs.at("body").g;
    LoopBody L(body, inits, where + ": only the formula decode step is supported as a Loop body with a key / value cache: ", "formula decode step");
    FormulaBody{L, body}.match(loop, outer_nodes, inits, opset, graph_outs, dec_out, dropped_inputs);
}

}  // namespace oar
