#include "engine.h"

#include "dsblock.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <set>
#include <sstream>

namespace oar {

using k::Act;

// =================================================================================================
// construction + load-time graph rewrites
// =================================================================================================
static int64_t numel(const std::vector<int64_t>& d) {
    int64_t n = 1;
    for (auto v : d) n *= v;
    return n;
}

Engine::Engine(const uint8_t* onnx, size_t len, int device_id, hipStream_t caller_stream) : device_(device_id) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        fail(OAR_DEVICE, "no HIP device visible: libOarMi355x has no CPU fallback");
    OAR_CHECK(device_id >= 0 && device_id < ndev, OAR_DEVICE, "device_id out of range");
    OAR_HIP(hipSetDevice(device_));
    if (caller_stream) { stream_ = caller_stream; owns_stream_ = false; }   // oar_engine_cfg.stream: the caller's stream, never destroyed here
    else OAR_HIP(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    OnnxModel m = parse_onnx(onnx, len);
    validate_model(m);
    input_name_ = m.inputs[0];
    output_names_ = m.outputs;
    input_infos_ = m.input_infos;
    output_infos_ = m.output_infos;
    if (const char* e = getenv("OAR_PLAN_CACHE")) { long v = atol(e); if (v >= 2) plan_cap_ = (size_t)v; }
    opset_ = m.opset;
    rewrite_graph(m);
    // fused-stem eligibility: the input is consumed once, by a group-1 convolution with 3 input channels and a small kernel
    {
        int uses = 0;
        const GNode* consumer = nullptr;
        for (const GNode& n : nodes_) {
            for (size_t i = 0; i < n.in.size(); ++i) if (n.in[i] == input_name_) { ++uses; consumer = &n; if (i != 0) uses += 100; }
            if (n.residual == input_name_) uses += 100;
        }
        for (auto& on : output_names_) if (on == input_name_) uses += 100;
        if (uses == 1 && consumer && consumer->op == "Conv" && consumer->ai("group", 1) == 1 && input_infos_.size() == 1) {
            auto it = inits_.find(consumer->in.size() > 1 ? consumer->in[1] : std::string());
            if (it != inits_.end() && it->second.dims.size() == 4 && it->second.dims[1] == 3 && it->second.dims[2] * it->second.dims[3] * 3 <= 128)
                stem_fusable_ = true;
        }
    }
}

Engine::~Engine() {
    (void)hipSetDevice(device_);
    if (stream_) (void)hipStreamSynchronize(stream_);
    clear_graphs();
    Profiler::get().drop_events();   // no pooled event may outlive the stream it was recorded on
    for (hipEvent_t ev : fd_.ev) if (ev) (void)hipEventDestroy(ev);
    if (fd_.state) (void)hipFree(fd_.state);
    if (fd_.fin) (void)hipHostFree(const_cast<unsigned*>(fd_.fin));
    if (fd_executed_) (void)hipHostFree(fd_executed_);
    for (void* p : dev_allocs_) (void)hipFree(p);
    if (stream_ && owns_stream_) (void)hipStreamDestroy(stream_);
    (void)hipGetLastError();
}

const float* Engine::upload_const(const std::string& key, const std::vector<float>& v) {
    auto it = dev_consts_.find(key);
    if (it != dev_consts_.end()) return it->second;
    void* p = nullptr;
    size_t bytes = std::max<size_t>(v.size() * sizeof(float), 16);
    OAR_HIP(hipMalloc(&p, bytes));
    dev_allocs_.push_back(p);
    if (!v.empty()) OAR_HIP(hipMemcpy(p, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice));
    dev_consts_[key] = (const float*)p;
    return (const float*)p;
}

// The operator table (behind the planner, where the columns are explained): ONE row per operator name the engine knows.  Engine::supported_ops(), what
// Planner::dispatch does with a plan-time input (device_data_inputs / reads_host_values) and which handler it calls are all read from it.
struct Planner;
enum class HostInputs { NONE, DATA0, DATA01, READS_HOST };
struct OpRow {
    const char* name;
    bool pub;
    HostInputs host_inputs;
    void (Planner::*plan)(const GNode&);
    int code;
};
static const OpRow* op_table(size_t& count);            // the rows, sorted by name
static const OpRow* find_op(const std::string& name);   // null: no such row

// activations that may be folded into a conv / linear / add epilogue (apply_act).  The other unary activations (the rows of the operator table that
// op_unary_act plans) only ever run as a stand-alone element-wise kernel (apply_unary): every extra case in apply_act costs registers in each conv epilogue --
// with all of them in, the depthwise kernel lost a wave per SIMD and a quarter of its bandwidth.
static bool is_fusable_act(const std::string& op) {
    return op == "Relu" || op == "HardSwish" || op == "HardSigmoid" || op == "Sigmoid" || op == "LeakyRelu" || op == "Tanh" || op == "Gelu";
}
static Act act_of(const GNode& n) {
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

// -------------------------------------------------------------------------------------------------
// Loop -> SLADecode.  The body contract, with h [B,H], pre [B] the loop-carried state and fea [B,HW,C] from the outer scope:
//   hp = Gemm(h, W_h2h, b_h2h, transB=1)        e = MatMul(Tanh(Add(MatMul(fea, W_i2h^T), Unsqueeze(hp, [1]))), w_score^T)
//   ctx = Squeeze(MatMul(Transpose(Softmax(e, axis=1), [0,2,1]), fea), [1])      x = Concat(ctx, OneHot(pre, V, [0,1]), axis=1)
//   xr,xz,xc = Split(Gemm(x, W_ih, b_ih, transB=1))   hr,hz,hc = Split(Gemm(h, W_hh, b_hh, transB=1))
//   r = Sigmoid(xr+hr)  z = Sigmoid(xz+hz)  c = Tanh(xc + r*hc)  h_new = (h - c)*z + c
//   logits = Gemm(Gemm(h_new, W_s1, b_s1), W_s2, b_s2)   loc = Sigmoid(Gemm(Gemm(h_new, W_l1, b_l1), W_l2, b_l2))   pre_new = ArgMax(logits, axis=1, keepdims=0)
// Tolerated: MatMul(x, W^T) + Add(bias) for a Gemm, Cast around OneHot / ArgMax, weights as body or outer initializers (or Constant
// nodes), axes as attribute or input, cond_out as Identity(cond_in) or a constant true.
void Engine::match_sla_loop(const GNode& loop, GNode& lin_out, GNode& dec_out) {
    const std::string where = "Loop (" + (loop.out.empty() ? std::string("?") : loop.out[0]) + ")";
    auto bit = loop.attrs.find("body");
    if (bit == loop.attrs.end() || bit->second.kind != Attr::G || !bit->second.g) fail(OAR_UNSUPPORTED_OP, where + ": only the SLA decode step is supported as a Loop body: the node has no body graph");
    const OnnxModel& body = *bit->second.g;
    LoopBody LB(body, inits_, where + ": only the SLA decode step is supported as a Loop body: ", "SLA step");
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
    if (opset_ < 13) refuse("Softmax / Split / Squeeze semantics below opset 13");
    const std::string &cond_in = body.inputs[1], &h = body.inputs[2], &pre = body.inputs[3];
    const std::string &cond_out = body.outputs[0], &h_new = body.outputs[1], &pre_new = body.outputs[2], &logits = body.outputs[3], &loc = body.outputs[4];
    // trip count and condition
    const HostTensor* mt = loop.in[0].empty() ? nullptr : [&]() -> const HostTensor* { auto it = inits_.find(loop.in[0]); return it == inits_.end() ? nullptr : &it->second; }();
    if (!mt || mt->dtype == DType::F32 || mt->i.size() != 1) refuse("the trip count M must be a constant integer scalar");
    const int64_t M = mt->i[0];
    if (!loop.in[1].empty()) {
        auto it = inits_.find(loop.in[1]);
        if (it == inits_.end() || it->second.i.size() != 1 || it->second.i[0] == 0) refuse("the loop condition must be absent or a constant true");
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
        inits_[key] = std::move(t);
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
void Engine::match_formula_loop(const GNode& loop, const std::vector<GNode>& outer_nodes, GNode& dec_out, std::vector<std::string>& dropped_inputs) {
    const std::string where = "Loop (" + (loop.out.empty() ? std::string("?") : loop.out[0]) + ")";
    const OnnxModel& body = *loop.attrs.at("body").g;
    LoopBody L(body, inits_, where + ": only the formula decode step is supported as a Loop body with a key / value cache: ", "formula decode step");
    using Lin = LoopBody::Lin;
    const int64_t Ld = ((int64_t)body.inputs.size() - 3) / 2;
    const size_t n_state = (size_t)(1 + 2 * Ld);
    if (Ld < 1 || Ld > k::kFdMaxLayers) L.refuse("the body carries " + std::to_string(Ld) + " layers of caches, outside 1 <= Ld <= " + std::to_string(k::kFdMaxLayers));
    const bool with_logits = body.outputs.size() == n_state + 3;
    if (body.outputs.size() != n_state + 2 && !with_logits) L.refuse("the body must yield (cond, tok, K_1', V_1', ..., scan tok [, scan logits])");
    if (loop.in.size() != 2 + n_state || loop.out.size() != body.outputs.size() - 1) L.refuse("the node must carry (M, cond, tok0, K_1, V_1, ...) and yield (tok, K_1, V_1, ..., tok scan [, logits scan])");
    if (opset_ < 17) L.refuse("LayerNormalization needs opset 17");
    const std::string &iter = body.inputs[0], &cond_in = body.inputs[1], &tok = body.inputs[2];
    const std::string &cond_out = body.outputs[0], &tok_new = body.outputs[1];
    if (body.outputs[n_state + 1] != tok_new) L.refuse("the first scan output must be the new token '" + tok_new + "'");
    // trip count and condition
    const HostTensor* mt = nullptr;
    if (!loop.in[0].empty()) { auto it = inits_.find(loop.in[0]); if (it != inits_.end()) mt = &it->second; }
    if (!mt || mt->dtype == DType::F32 || mt->i.size() != 1) L.refuse("the trip count M must be a constant integer scalar");
    const int64_t M = mt->i[0];
    if (!loop.in[1].empty()) {
        auto it = inits_.find(loop.in[1]);
        if (it == inits_.end() || it->second.i.size() != 1 || it->second.i[0] == 0) L.refuse("the loop condition must be absent or a constant true");
    }
    if (const HostTensor* ct = L.cst(cond_out)) {
        if (ct->i.size() != 1 || ct->i[0] == 0) L.refuse("cond_out must be Identity(cond_in) or a constant true");
    } else {
        const OnnxNode& id = L.expect(cond_out, "Identity", "loop condition");
        if (id.inputs.size() != 1 || id.inputs[0] != cond_in) L.bad(id, "cond_out must be Identity(cond_in)");
    }
    // helpers of this body
    auto scalar_f = [&](const std::string& v, float& out) {
        const HostTensor* t = L.cst(v);
        if (!t || t->dtype != DType::F32 || t->f.size() != 1) return false;
        out = t->f[0];
        return true;
    };
    struct LN { std::string x; std::vector<float> g, b; float eps; };
    auto layer_norm = [&](const std::string& v, const char* role) -> LN {
        const OnnxNode& n = L.expect(v, "LayerNormalization", role);
        if (n.inputs.size() != 3 || n.inputs[2].empty()) L.bad(n, "LayerNormalization needs a scale and a bias");
        const int64_t ax = n.ai("axis", -1);
        if (ax != -1 && ax != 1) L.bad(n, "LayerNormalization must normalise the last axis");
        LN r;
        r.x = n.inputs[0]; r.g = L.f32c(n, n.inputs[1], 1).f; r.b = L.f32c(n, n.inputs[2], 1).f; r.eps = n.af("epsilon", 1e-5f);
        if (r.g.size() != r.b.size()) L.bad(n, "scale and bias lengths differ");
        return r;
    };
    // is `v` the output of a lin (Gemm, MatMul by a constant, or Add of one and a constant)?
    auto const_matmul = [&](const std::string& v) { auto it = L.producer.find(v); return it != L.producer.end() && body.nodes[it->second].op == "MatMul" && body.nodes[it->second].inputs.size() == 2 && L.cst(body.nodes[it->second].inputs[1]); };
    auto is_lin = [&](const std::string& v) {
        if (L.is_op(v, "Gemm") || const_matmul(v)) return true;
        if (!L.is_op(v, "Add")) return false;
        const OnnxNode& a = body.nodes[L.producer[v]];
        return a.inputs.size() == 2 && ((const_matmul(a.inputs[0]) && L.cst(a.inputs[1])) || (const_matmul(a.inputs[1]) && L.cst(a.inputs[0])));
    };
    // v = Add(residual, lin(..)) in either order
    auto residual = [&](const std::string& v, const char* role, std::string& res) -> Lin {
        const OnnxNode& a = L.expect(v, "Add", role);
        L.two(a);
        const int li = is_lin(a.inputs[1]) ? 1 : is_lin(a.inputs[0]) ? 0 : -1;
        if (li < 0) L.bad(a, std::string("the ") + role + " must add a Gemm or MatMul [+ Add] to the residual");
        res = a.inputs[1 - li];
        return L.lin(a.inputs[li], role, 1);
    };
    // a projection with the query scale: mode 0 none, 1 (x W^T + b) * s, 2 (x W^T) * s + b
    auto scaled_lin = [&](const std::string& v, const char* role, int& mode, float& scale) -> Lin {
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
    };
    auto reshape_target = [&](const OnnxNode& n) -> std::vector<int64_t> {
        if (n.inputs.size() < 2) L.bad(n, "Reshape needs a constant target");
        const HostTensor* t = L.cst(n.inputs[1]);
        if (!t || t->dtype == DType::F32 || t->i.empty()) L.bad(n, "the Reshape target must be a constant");
        return t->i;
    };
    int64_t D = 0, nh = 0, dh = 0, dq = 0;
    // v = Reshape(u, [B, nh, 1, dh]): returns u.  kind 0: a value / cross-attention projection, nh x dh = D.  kind 1: the cross-attention query, the same, with
    // a word on squeeze attention where the product is not D.  kind 2: the self-attention query / key, [B, nh, 1, dq] with its own head size (squeeze attention:
    // dq need not be dh; an entry <= 0 is inferred from D as for the others)
    auto split_heads = [&](const std::string& v, const char* role, int kind = 0) -> std::string {
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
    };
    // v = Reshape(MatMul(Softmax(MatMul(q4, keys), -1), values), [B, D]): returns q4 / keys / values
    auto attention = [&](const std::string& v, const char* role, std::string& q4, std::string& keys, std::string& values) {
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
    };
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
    struct Layer { LN ln1, ln2, ln3; Lin q, k, v, o, cq, co, f1, f2; int qm = 0, cqm = 0; float qs = 1.f, cqs = 1.f; std::string kmT, vm; };
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
    // initial state: every cache starts empty, and nothing else may read it or the final caches
    auto producer_of = [&](const std::string& v) -> const GNode* {
        for (const GNode& n : outer_nodes) for (auto& o : n.out) if (o == v) return &n;
        return nullptr;
    };
    for (size_t c = 3; c < loop.in.size(); ++c) {
        const std::string& nm = loop.in[c];
        bool empty = false;
        auto it = inits_.find(nm);
        if (it != inits_.end()) empty = it->second.dims.size() == 4 && it->second.dims[2] == 0;
        else if (const GNode* cs = producer_of(nm)) {
            const GNode* cat = cs->op == "ConstantOfShape" && cs->in.size() == 1 ? producer_of(cs->in[0]) : nullptr;
            if (cat && cat->op == "Concat" && cat->in.size() == 4) {
                auto z = inits_.find(cat->in[2]);
                empty = z != inits_.end() && z->second.dtype != DType::F32 && z->second.i.size() == 1 && z->second.i[0] == 0;
            }
        }
        if (!empty) L.refuse("the initial cache '" + nm + "' must be empty: an initializer with dims[2] == 0, or ConstantOfShape over a Concat whose third element is the constant 0");
        int readers = 0;
        for (const GNode& n : outer_nodes) for (auto& s : n.in) if (s == nm) ++readers;
        if (readers != 1 || std::find(output_names_.begin(), output_names_.end(), nm) != output_names_.end()) L.refuse("the initial cache '" + nm + "' is read outside the Loop");
        dropped_inputs.push_back(nm);
    }
    for (size_t c = 1; c < n_state; ++c) {
        const std::string& nm = loop.out[c];
        if (nm.empty()) continue;
        bool read = std::find(output_names_.begin(), output_names_.end(), nm) != output_names_.end();
        for (const GNode& n : outer_nodes) for (auto& s : n.in) if (s == nm) read = true;
        if (read) L.refuse("the final cache '" + nm + "' is read by the rest of the graph: the caches are not produced");
    }
    // constants in the kernels' layout (kernels.h: FormulaDecodeP): matrix rows padded to a multiple of four floats
    const std::string pfx = "fd::" + loop.out[n_state] + "::";
    auto put = [&](const std::string& nm, std::vector<int64_t> dims, std::vector<float> v) {
        HostTensor t; t.name = pfx + nm; t.dtype = DType::F32; t.dims = std::move(dims); t.f = std::move(v);
        const std::string key = t.name;
        inits_[key] = std::move(t);
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
        Y = Layer();   // (the repacked copies are in inits_ now)
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

void Engine::rewrite_graph(OnnxModel& m) {
    inits_ = std::move(m.initializers);
    std::vector<GNode> nodes;
    for (auto& on : m.nodes) {
        if (on.op == "Constant") {
            auto it = on.attrs.find("value");
            OAR_CHECK(it != on.attrs.end() && it->second.kind == Attr::T, OAR_UNSUPPORTED_OP, "Constant without tensor value");
            HostTensor t = it->second.t;
            t.name = on.outputs[0];
            inits_[t.name] = std::move(t);
            continue;
        }
        if (on.op == "Dropout") { on.op = "Identity"; on.outputs.resize(1); }
        GNode g;
        g.op = on.op; g.in = on.inputs; g.out = on.outputs; g.attrs = on.attrs;
        nodes.push_back(std::move(g));
    }
    std::set<std::string> graph_outs(output_names_.begin(), output_names_.end());
    auto consumers = [&](const std::vector<GNode>& ns) {
        std::map<std::string, std::vector<int>> c;
        for (int i = 0; i < (int)ns.size(); ++i)
            for (auto& s : ns[i].in)
                if (!s.empty()) c[s].push_back(i);
        return c;
    };
    auto is_init = [&](const std::string& s) { return inits_.count(s) != 0; };

    // ---- pass 0: Loop.  There is no generic sub-graph executor: two bodies are recognised, by their interface, and replaced by fused operators.
    //   4 inputs / 5 outputs: the SLANet structure head's step (PaddleOCR SLAHead._decode: AttentionGRUCell + GRUCell + both output heads, greedy feedback
    //     of the arg max)  ->  Linear (the loop-invariant projection of the features) + ONE SLADecode node (match_sla_loop)
    //   3 + 2 Ld inputs: the greedy step of a transformer decoder with a key / value cache (PP-FormulaNet)  ->  ONE FormulaDecode node; the empty initial
    //     caches and their producers leave the graph (match_formula_loop)
    // Anything else, or a body that is not one of these in a spelling its matcher tolerates, is refused with the name of the first body node that did not fit.
    {
        std::vector<GNode> out;
        std::vector<std::string> dropped;
        for (size_t ni = 0; ni < nodes.size(); ++ni) {
            GNode& n = nodes[ni];
            if (n.op != "Loop") { out.push_back(n); continue; }
            auto bit = n.attrs.find("body");
            const OnnxModel* body = bit != n.attrs.end() && bit->second.kind == Attr::G && bit->second.g ? bit->second.g.get() : nullptr;
            if (!body || (body->inputs.size() == 4 && body->outputs.size() == 5)) {
                GNode lin, dec;
                match_sla_loop(n, lin, dec);
                out.push_back(std::move(lin));
                out.push_back(std::move(dec));
            } else if (body->inputs.size() >= 5 && body->inputs.size() % 2 == 1) {
                GNode dec;
                match_formula_loop(n, nodes, dec, dropped);
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
    {
        auto cons = consumers(nodes);
        std::map<std::string, int> producer;
        for (int i = 0; i < (int)nodes.size(); ++i) for (auto& o : nodes[i].out) producer[o] = i;
        std::vector<bool> dead(nodes.size(), false);
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
            const HostTensor& W = inits_[cv.in[1]];
            const auto &ga = inits_[bn.in[1]].f, &be = inits_[bn.in[2]].f, &mu = inits_[bn.in[3]].f, &va = inits_[bn.in[4]].f;
            float eps = bn.af("epsilon", 1e-5f);
            int64_t C = (int64_t)ga.size();
            OAR_CHECK(W.dtype == DType::F32 && W.dims.size() == 4, OAR_MODEL_LOAD, "BN fold: conv weight must be a rank-4 f32 initializer (" + cv.in[1] + ")");
            OAR_CHECK(C > 0 && (int64_t)be.size() == C && (int64_t)mu.size() == C && (int64_t)va.size() == C, OAR_MODEL_LOAD,
                      "BatchNormalization: scale / bias / mean / var must all have C elements (" + bn.out[0] + ")");
            if (cv.in.size() > 2 && !cv.in[2].empty())
                OAR_CHECK((int64_t)inits_[cv.in[2]].f.size() == C, OAR_MODEL_LOAD, "BN fold: conv bias must have C elements (" + cv.in[2] + ")");
            HostTensor W2 = W;
            std::vector<float> b2(C, 0.f);
            if (cv.in.size() > 2 && !cv.in[2].empty()) b2 = inits_[cv.in[2]].f;
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
            inits_[wn] = std::move(W2);
            HostTensor B; B.name = bnm; B.dtype = DType::F32; B.dims = {C}; B.f = b2;
            inits_[bnm] = std::move(B);
            cv.in.resize(3);
            cv.in[1] = wn; cv.in[2] = bnm;
            cv.out[0] = bn.out[0];
            producer[bn.out[0]] = pit->second;
            dead[i] = true;
        }
        std::vector<GNode> keep;
        for (int i = 0; i < (int)nodes.size(); ++i) if (!dead[i]) keep.push_back(std::move(nodes[i]));
        nodes.swap(keep);
    }

    // ---- pass 2: MatMul(x, Wconst) + Add(const bias)  ->  Linear
    {
        auto cons = consumers(nodes);
        std::vector<bool> dead(nodes.size(), false);
        for (int i = 0; i < (int)nodes.size(); ++i) {
            GNode& mm = nodes[i];
            if (mm.op != "MatMul" || !is_init(mm.in[1]) || inits_[mm.in[1]].dims.size() != 2) continue;
            mm.op = "Linear";
            auto& cs = cons[mm.out[0]];
            if (cs.size() != 1 || graph_outs.count(mm.out[0])) continue;
            GNode& ad = nodes[cs[0]];
            if (ad.op != "Add" || dead[cs[0]]) continue;
            int other = ad.in[0] == mm.out[0] ? 1 : 0;
            if (!is_init(ad.in[other])) continue;
            const HostTensor& b = inits_[ad.in[other]];
            if (numel(b.dims) != inits_[mm.in[1]].dims[1] || b.dims.empty() || b.dims.back() != numel(b.dims)) continue;
            mm.bias = ad.in[other];
            mm.out[0] = ad.out[0];
            dead[cs[0]] = true;
        }
        std::vector<GNode> keep;
        for (int i = 0; i < (int)nodes.size(); ++i) if (!dead[i]) keep.push_back(std::move(nodes[i]));
        nodes.swap(keep);
    }

    // ---- pass 2b: GELU as exporters below opset 20 spell it (SVTRv2's MLPs and conv stem): x * 0.5 * (1 + erf(x / sqrt(2))), in either association
    //   Mul(Mul(x, Add(Erf(Div(x, 1.41421)), 1)), 0.5)   or   Mul(Mul(x, 0.5), Add(Erf(..), 1));  x / sqrt(2) may also be Mul(x, 0.70711)
    // becomes ONE Gelu node (5 element-wise launches over the widest tensor of the block -> an epilogue of the producing Linear / Conv, pass 3).
    // OAR_FUSE_GELU=0 keeps the op-by-op path.
    {
        const char* fe = getenv("OAR_FUSE_GELU");
        const bool fuse = !fe || atoi(fe) != 0;
        auto cons = consumers(nodes);
        std::map<std::string, int> producer;
        for (int i = 0; i < (int)nodes.size(); ++i) for (auto& o : nodes[i].out) producer[o] = i;
        std::vector<bool> dead(nodes.size(), false);
        auto scalar_of = [&](const std::string& v, float& out) {
            auto it = inits_.find(v);
            if (it == inits_.end() || it->second.dtype != DType::F32 || it->second.f.size() != 1) return false;
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
        std::vector<GNode> keep;
        for (int i = 0; i < (int)nodes.size(); ++i) if (!dead[i]) keep.push_back(std::move(nodes[i]));
        nodes.swap(keep);
    }

    // ---- pass 2c: LayerNorm over the last axis as exporters below opset 17 spell it:
    //   m = ReduceMean(x, [a], keepdims 1);  d = Sub(x, m);  v = ReduceMean(Pow(d, 2) | Mul(d, d), [a], keepdims 1);  r = Sqrt(Add(v, eps))
    //   y = Div(d, r)  |  Mul(d, Reciprocal(r))  |  Mul(d, Div(1, r))        [-> Mul(y, gamma [C]) [-> Add(., beta [C])]]
    // becomes ONE LayerNormalization node (nine launches that pass the tensor through HBM about seven times -> one), so that an opset-13 and an opset-17 export
    // of the same block meet the same later passes.  Axes as an attribute or a constant input; Add and the Muls in either order; eps a positive f32 constant of
    // one element; gamma / beta f32 initializers of [C] or [1, .., 1, C], each folded only when the value in front of it has that single reader.  m, v, the
    // squares, the Add and the Sqrt must have one reader each, d exactly the square and the quotient, none a graph output.  a = -1 or a >= 0: the rank of x
    // is unknown here, so the replaced nodes are kept (ln_spelled_) and op_layernorm plans them instead when a turns out not to be the last axis (or x has
    // rank 1, or gamma / beta do not have x's last extent).  Anything else stays as it is.  OAR_FUSE_LAYERNORM=0 keeps the op-by-op route.
    {
        const char* fe = getenv("OAR_FUSE_LAYERNORM");
        const bool fuse = !fe || atoi(fe) != 0;
        auto cons = consumers(nodes);
        std::map<std::string, int> producer;
        for (int i = 0; i < (int)nodes.size(); ++i) for (auto& o : nodes[i].out) producer[o] = i;
        std::vector<bool> dead(nodes.size(), false);
        auto single_use = [&](const std::string& v) { return cons[v].size() == 1 && !graph_outs.count(v); };
        auto reader = [&](const std::string& v, const char* op) -> int {   // the only reader of v, a live two-input `op` (or -1)
            if (!single_use(v)) return -1;
            const int c = cons[v][0];
            return !dead[c] && nodes[c].op == op ? c : -1;
        };
        auto scalar_is = [&](const std::string& v, float want) {
            auto it = inits_.find(v);
            if (it == inits_.end()) return false;
            const HostTensor& t = it->second;
            return t.dtype == DType::F32 ? (t.f.size() == 1 && t.f[0] == want) : (t.i.size() == 1 && (float)t.i[0] == want);
        };
        auto mean_axis = [&](const GNode& q, int64_t& ax) {   // ReduceMean over ONE axis, keepdims 1
            if (q.op != "ReduceMean" || q.in.empty() || q.ai("keepdims", 1) != 1) return false;
            std::vector<int64_t> a;
            if (q.in.size() > 1 && !q.in[1].empty()) {
                auto it = inits_.find(q.in[1]);
                if (it == inits_.end() || it->second.dtype == DType::F32) return false;
                a = it->second.i;
            } else {
                a = q.ais("axes");
            }
            if (a.size() != 1 || a[0] < -1) return false;
            ax = a[0];
            return true;
        };
        auto affine_vec = [&](const std::string& v) -> int64_t {   // elements of an f32 initializer shaped [C] or [1, .., 1, C]; 0: not one
            auto it = inits_.find(v);
            if (it == inits_.end() || it->second.dtype != DType::F32 || it->second.dims.empty()) return 0;
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
            auto ei = inits_.find(epsn);
            if (ei == inits_.end() || ei->second.dtype != DType::F32 || ei->second.f.size() != 1 || ei->second.dims.size() > 1 || !(ei->second.f[0] > 0.0f)) continue;
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
            std::vector<GNode>& spelled = ln_spelled_[ln.out[0]];
            for (int p : parts) { spelled.push_back(nodes[p]); dead[p] = true; }
            dead[last] = false;
            nodes[last] = std::move(ln);   // the last node of the pattern: x is computed in front of it and every reader comes after it
        }
        std::vector<GNode> keep;
        for (int i = 0; i < (int)nodes.size(); ++i) if (!dead[i]) keep.push_back(std::move(nodes[i]));
        nodes.swap(keep);
    }

    // ---- pass 3: fuse activations into Conv / ConvTranspose / Linear / Gemm / Add
    {
        bool changed = true;
        while (changed) {
            changed = false;
            auto cons = consumers(nodes);
            std::vector<bool> dead(nodes.size(), false);
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
            std::vector<GNode> keep;
            for (int i = 0; i < (int)nodes.size(); ++i) if (!dead[i]) keep.push_back(std::move(nodes[i]));
            nodes.swap(keep);
        }
    }

    // ---- the matcher toolkit of passes 3b - 3e: declared once, by node index throughout.  scan() reads the current `nodes` at the head of a pass (readers,
    // producers, nobody dead) and sweep() drops what the pass killed.  Every node a helper returns is live and PLAIN: no fused activation (so far pass 3 alone
    // attaches one, to Conv / ConvTranspose / Linear / Gemm / Add) and no fused residual (pass 4, behind all four passes, is the first to attach one).
    using V = std::vector<int64_t>;
    std::map<std::string, std::vector<int>> cons;
    std::map<std::string, int> producer;
    std::vector<bool> dead;
    auto scan = [&] {
        cons = consumers(nodes);
        producer.clear();
        for (int i = 0; i < (int)nodes.size(); ++i) for (auto& o : nodes[i].out) producer[o] = i;
        dead.assign(nodes.size(), false);
    };
    auto sweep = [&] {
        std::vector<GNode> keep;
        for (int i = 0; i < (int)nodes.size(); ++i) if (!dead[i]) keep.push_back(std::move(nodes[i]));
        nodes.swap(keep);
    };
    auto plain = [&](int i, const char* op) { return !dead[i] && nodes[i].op == op && nodes[i].act.kind == k::ACT_NONE && nodes[i].residual.empty(); };
    auto single_use = [&](const std::string& v) { return cons[v].size() == 1 && !graph_outs.count(v); };
    auto prodn = [&](const std::string& v, const char* op) -> int {    // the producer `op` of v (v may have several readers)
        auto it = producer.find(v);
        return it != producer.end() && plain(it->second, op) ? it->second : -1;
    };
    auto prod1 = [&](const std::string& v, const char* op) -> int { return single_use(v) ? prodn(v, op) : -1; };   // ... and v read by nobody else
    auto reader1 = [&](const std::string& v, const char* op) -> int {  // the single consumer of v, an `op` reading it first
        if (!single_use(v)) return -1;
        const int c = cons[v][0];
        return plain(c, op) && nodes[c].in[0] == v ? c : -1;
    };
    auto ints = [&](const std::string& v) -> V {
        auto it = inits_.find(v);
        return it == inits_.end() || it->second.dtype == DType::F32 ? V{} : it->second.i;
    };
    auto target = [&](int r) -> V { return nodes[r].in.size() < 2 || nodes[r].ai("allowzero", 0) != 0 ? V{} : ints(nodes[r].in[1]); };   // of a Reshape
    auto perm_is = [&](int t, std::initializer_list<int64_t> want) { return nodes[t].ais("perm") == V(want); };
    auto axes_are = [&](int n, int64_t a, int64_t rank) {              // opset 13 input or the older attribute; a or a - rank
        const V ax = nodes[n].in.size() > 1 && !nodes[n].in[1].empty() ? ints(nodes[n].in[1]) : nodes[n].ais("axes");
        return ax.size() == 1 && (ax[0] == a || ax[0] == a - rank);
    };
    auto f32_scalar = [&](const std::string& v) -> const HostTensor* {
        auto it = inits_.find(v);
        return it != inits_.end() && it->second.dtype == DType::F32 && it->second.f.size() == 1 ? &it->second : nullptr;
    };
    auto iattr = [](GNode& n, const char* k, int64_t v) { Attr a; a.kind = Attr::I; a.i = v; n.attrs[k] = a; };
    auto fattr = [](GNode& n, const char* k, float v) { Attr a; a.kind = Attr::F; a.f = v; n.attrs[k] = a; };

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
    {
        const char* fe = getenv("OAR_FUSE_WINDOW_ATTENTION");
        const bool fuse = !fe || atoi(fe) != 0;
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
            const HostTensor& w = inits_[l.in[1]];
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
                const HostTensor& mk = inits_[maskn];
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
            const HostTensor& bias = inits_[nodes[ad].in[bi]];
            if (bias.dtype != DType::F32 || bias.dims.size() != 4 || bias.dims[0] != 1 || bias.dims[2] != bias.dims[3] || (int64_t)bias.f.size() != numel(bias.dims)) continue;
            const int64_t nh = bias.dims[1], N = bias.dims[2];
            int64_t nWm = 0;
            if (m3 >= 0) {
                const HostTensor& mk = inits_[maskn];
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
    {
        const char* fe = getenv("OAR_FUSE_RELPOS_ATTENTION");
        const bool fuse = fe && atoi(fe) != 0;           // opt-in until the three-arm speed measurement of DESIGN 4.35 exists: unset or 0 keeps the op-by-op route
        scan();
        auto table = [&](const std::string& v, int64_t n, int64_t dh) {  // a constant f32 [n, dh, n]
            auto it = inits_.find(v);
            return it != inits_.end() && it->second.dtype == DType::F32 && it->second.dims == V{n, dh, n} && (int64_t)it->second.f.size() == n * dh * n;
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
                const HostTensor& wq = inits_[nodes[lq].in[1]];
                if (wq.dims != V{C, 3 * C}) continue;
                if (!nodes[lq].bias.empty() && (!is_init(nodes[lq].bias) || inits_[nodes[lq].bias].dtype != DType::F32 || (int64_t)inits_[nodes[lq].bias].f.size() != 3 * C)) continue;
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
            if (pj < 0 || nodes[pj].in.size() < 2 || !is_init(nodes[pj].in[1]) || inits_[nodes[pj].in[1]].dims != V{C, C}) continue;
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
    {
        const char* fe = getenv("OAR_FUSE_DEFORMABLE_ATTENTION");
        const bool fuse = !fe || atoi(fe) != 0;
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
    {
        const char* fe = getenv("OAR_FUSE_MHA_ATTENTION");
        const bool fuse = !fe || atoi(fe) != 0;
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
    {
        auto cons = consumers(nodes);
        std::vector<bool> dead(nodes.size(), false);
        std::map<std::string, int> producer;
        for (int i = 0; i < (int)nodes.size(); ++i) for (auto& o : nodes[i].out) producer[o] = i;
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
        std::vector<GNode> keep;
        for (int i = 0; i < (int)nodes.size(); ++i) if (!dead[i]) keep.push_back(std::move(nodes[i]));
        nodes.swap(keep);
    }
    // ---- pass 5: the SVTR global-attention block (EncoderWithSVTR), as the recognizer exports emit it:
    //   Reshape[0,-1,3,h,d] -> Transpose[2,0,3,1,4] -> Split(axis 0) -> 3 x Squeeze[0] -> (Mul by a scalar on q) ->
    //   MatMul(q, Transpose[0,1,3,2](k)) -> Softmax(-1) -> MatMul(., v) -> Transpose[0,2,1,3] -> Reshape[0,-1,h*d]
    // becomes ONE Attention node that reads the [n, T, 3*h*d] projection in place (12 glue kernels + 2 batched GEMMs +
    // softmax -> 1 kernel).  OAR_FUSE_ATTENTION=0 keeps the op-by-op path.
    {
        const char* fe = getenv("OAR_FUSE_ATTENTION");
        const bool fuse = !fe || atoi(fe) != 0;
        auto cons = consumers(nodes);
        std::map<std::string, int> producer;
        for (int i = 0; i < (int)nodes.size(); ++i) for (auto& o : nodes[i].out) producer[o] = i;
        std::vector<bool> dead(nodes.size(), false);
        auto prod = [&](const std::string& v, const char* op) -> int {
            auto it = producer.find(v);
            if (it == producer.end() || dead[it->second] || nodes[it->second].op != op) return -1;
            return it->second;
        };
        auto single_use = [&](const std::string& v) { return cons[v].size() == 1 && !graph_outs.count(v); };
        auto ints_of = [&](const std::string& v) -> std::vector<int64_t> {
            auto it = inits_.find(v);
            return it == inits_.end() ? std::vector<int64_t>{} : it->second.i;
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
                const HostTensor& sc = inits_[nodes[mul].in[ci]];
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
        std::vector<GNode> keep;
        for (int i = 0; i < (int)nodes.size(); ++i) if (!dead[i]) keep.push_back(std::move(nodes[i]));
        nodes.swap(keep);
    }
    // ---- pass 6: squeeze-excite gate: GlobalAveragePool -> Conv 1x1 (+act) -> Conv 1x1 (+act) on the pooled vector
    // becomes one SEGate node (two GEMVs per image in one kernel instead of two implicit-GEMM launches).
    {
        const char* fe = getenv("OAR_FUSE_SE");
        const bool fuse = !fe || atoi(fe) != 0;
        auto cons = consumers(nodes);
        std::map<std::string, int> producer;
        for (int i = 0; i < (int)nodes.size(); ++i) for (auto& o : nodes[i].out) producer[o] = i;
        std::vector<bool> dead(nodes.size(), false);
        auto plain_1x1 = [&](const GNode& c) {
            if (c.op != "Conv" || c.in.size() < 2 || !is_init(c.in[1]) || !c.residual.empty() || c.ai("group", 1) != 1) return false;
            const HostTensor& w = inits_[c.in[1]];
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
            if (inits_[nodes[b].in[1]].dims[1] != inits_[nodes[a].in[1]].dims[0]) continue;
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
        std::vector<GNode> keep;
        for (int i = 0; i < (int)nodes.size(); ++i) if (!dead[i]) keep.push_back(std::move(nodes[i]));
        nodes.swap(keep);
    }
    // ---- pass 7: depthwise-separable block: Conv (depthwise k x k, folded activation) -> Conv (1 x 1, folded activation /
    // residual) with nothing else reading the expanded tensor becomes ONE DSBlock node (csrc/dsblock.inc: the depthwise
    // output stays in LDS and feeds the matrix pipe).  Shapes are only known at plan time: op_dsblock falls back to the two
    // convolutions when dsblock_eligible() says no.  OAR_FUSE_DSBLOCK=0 keeps them apart.
    {
        const char* fe = getenv("OAR_FUSE_DSBLOCK");
        const bool fuse = !fe || atoi(fe) != 0;
        auto cons = consumers(nodes);
        std::vector<bool> dead(nodes.size(), false);
        auto ints = [](const GNode& c, const char* k, int64_t dflt) { auto v = c.ais(k); return v.empty() ? std::vector<int64_t>{dflt, dflt} : v; };
        for (int i = 0; fuse && i < (int)nodes.size(); ++i) {
            const GNode& d = nodes[i];
            if (dead[i] || d.op != "Conv" || d.in.size() < 2 || !is_init(d.in[1]) || !d.residual.empty()) continue;
            const HostTensor& wd = inits_[d.in[1]];
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
                const HostTensor& wp = inits_[pw.in[1]];
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
        std::vector<GNode> keep;
        for (int i = 0; i < (int)nodes.size(); ++i) if (!dead[i]) keep.push_back(std::move(nodes[i]));
        nodes.swap(keep);
    }
    // ---- pass 8: squeeze-excite scale into the pointwise conv behind it: Mul(x, SEGate(...)) whose only reader is a plain 1x1 Conv
    // becomes that Conv with the gate as a 4th input (csrc/igemm_ws_x6.hip multiplies it into the pixels as they are loaded: the scaled
    // feature map is never written or re-read).  Shapes / kernel choice are plan-time matters: op_conv runs the Mul after all when the
    // bf16x6 weight-stationary kernel does not take the layer.  OAR_FUSE_SE_SCALE=0 keeps the Mul.
    {
        const char* fe = getenv("OAR_FUSE_SE_SCALE");
        const bool fuse = !fe || atoi(fe) != 0;
        auto cons = consumers(nodes);
        std::map<std::string, int> producer;
        for (int i = 0; i < (int)nodes.size(); ++i) for (auto& o : nodes[i].out) producer[o] = i;
        std::vector<bool> dead(nodes.size(), false);
        for (int i = 0; fuse && i < (int)nodes.size(); ++i) {
            const GNode& m = nodes[i];
            if (m.op != "Mul" || m.in.size() != 2 || m.act.kind != k::ACT_NONE || !m.residual.empty() || graph_outs.count(m.out[0])) continue;
            int gi = -1;
            for (int t = 0; t < 2; ++t) { auto pit = producer.find(m.in[t]); if (pit != producer.end() && nodes[pit->second].op == "SEGate") gi = t; }
            if (gi < 0 || cons[m.out[0]].size() != 1) continue;
            GNode& c = nodes[cons[m.out[0]][0]];
            if (c.op != "Conv" || c.in.size() < 2 || c.in.size() > 3 || c.in[0] != m.out[0] || !is_init(c.in[1]) || c.ai("group", 1) != 1) continue;
            const HostTensor& w = inits_[c.in[1]];
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
        std::vector<GNode> keep;
        for (int i = 0; i < (int)nodes.size(); ++i) if (!dead[i]) keep.push_back(std::move(nodes[i]));
        nodes.swap(keep);
    }
    // ---- pass 9: the squeeze of a squeeze-excite block from the depthwise conv's own epilogue: GlobalAveragePool(dw conv output) is
    // dropped and its output becomes a second output of the conv node (conv_dw_tiled_kernel<..., GAP> writes per-tile sums,
    // global_avgpool_finish reduces them: the feature map is not read a second time).  op_conv pools separately when the launched
    // depthwise variant has no pooled form.  OAR_FUSE_SE_POOL=0 keeps the GlobalAveragePool.
    {
        const char* fe = getenv("OAR_FUSE_SE_POOL");
        const bool fuse = !fe || atoi(fe) != 0;
        std::map<std::string, int> producer;
        for (int i = 0; i < (int)nodes.size(); ++i) for (auto& o : nodes[i].out) producer[o] = i;
        std::vector<bool> dead(nodes.size(), false);
        for (int i = 0; fuse && i < (int)nodes.size(); ++i) {
            const GNode& gp = nodes[i];
            if (gp.op != "GlobalAveragePool" || gp.in.size() != 1 || graph_outs.count(gp.out[0])) continue;
            auto pit = producer.find(gp.in[0]);
            if (pit == producer.end() || pit->second > i) continue;
            GNode& d = nodes[pit->second];
            if (d.op != "Conv" || d.out.size() != 1 || d.in.size() < 2 || d.in.size() > 3 || !is_init(d.in[1]) || !d.residual.empty()) continue;
            const HostTensor& wd = inits_[d.in[1]];
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
        std::vector<GNode> keep;
        for (int i = 0; i < (int)nodes.size(); ++i) if (!dead[i]) keep.push_back(std::move(nodes[i]));
        nodes.swap(keep);
    }
    // ---- pass 10: residual Add -> LayerNormalization.  Behind every pass above: an Add that pass 4 folded into its Linear is that Linear's
    // residual by now (one folded into a Conv stays there), one that pass 3 gave an activation is not plain.  Layouts, shapes and whether the sample-local chain takes the LayerNorm are known at plan time only, so this pass
    // just marks the pair: a LayerNormalization directly behind the plain Add it reads (where every exporter puts it), its scale and bias initializers or absent;
    // Planner::fuse_chains then replaces the two launches by ONE k::add_layernorm where the pair qualifies.  OAR_FUSE_ADD_LAYERNORM=0 keeps both.
    {
        const char* fe = getenv("OAR_FUSE_ADD_LAYERNORM");
        fuse_add_ln_ = !fe || atoi(fe) != 0;
        for (int j = 1; fuse_add_ln_ && j < (int)nodes.size(); ++j) {
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
    for (int i = 0; i < (int)nodes.size(); ++i) nodes[i].id = i;
    nodes_ = std::move(nodes);
}

// =================================================================================================
// planner
// =================================================================================================
struct TInfo {
    std::vector<int64_t> dims;  // logical
    Layout layout = Layout::NATIVE;
    Loc loc;
    bool host_int = false;           // value known at plan time (shape arithmetic): lives on the host, never in HBM
    std::vector<int64_t> hv;         //   as integers (floats truncated toward zero)
    bool host_f = false;             //   the host value is floating point: hd is authoritative
    std::vector<double> hd;
    const HostTensor* ht = nullptr;  // f32 initializer
    bool is_int = false;             // device tensor whose f32 values are integers by construction (ArgMax, integer Cast of one)
    bool is01 = false;               // device tensor whose values are 0.0f / 1.0f by construction (comparison, logic op, Not, bool Cast): a Cast to bool of it is an alias
    bool u8_stem = false;            // the graph input of a run_stem plan: u8 pages read by the fused stem, no f32 tensor behind it
    std::string root;                // storage root (for liveness)
    int gap_tiles = 0, gap_hw = 0;   // [n, tiles * C, 1, 1]: per-tile channel sums of a pooling depthwise conv, still to be reduced and divided by gap_hw (SEGate does)
    size_t bytes() const { return (size_t)std::max<int64_t>(numel(dims), 1) * 4; }
};

struct Arena {
    struct Blk { size_t off, sz; };
    std::vector<Blk> free_;
    size_t top = 0;
    static size_t al(size_t n) { return (n + 255) & ~(size_t)255; }
    size_t alloc(size_t n) {
        n = al(std::max<size_t>(n, 4));
        int best = -1;
        for (int i = 0; i < (int)free_.size(); ++i)
            if (free_[i].sz >= n && (best < 0 || free_[i].sz < free_[best].sz)) best = i;
        if (best >= 0) {
            size_t off = free_[best].off;
            if (free_[best].sz == n) free_.erase(free_.begin() + best);
            else { free_[best].off += n; free_[best].sz -= n; }
            return off;
        }
        size_t off = top;
        top += n;
        return off;
    }
    void release(size_t off, size_t n) {
        n = al(std::max<size_t>(n, 4));
        free_.push_back({off, n});
        std::sort(free_.begin(), free_.end(), [](const Blk& a, const Blk& b) { return a.off < b.off; });
        std::vector<Blk> m;
        for (auto& b : free_) {
            if (!m.empty() && m.back().off + m.back().sz == b.off) m.back().sz += b.sz;
            else m.push_back(b);
        }
        if (!m.empty() && m.back().off + m.back().sz == top) { top = m.back().off; m.pop_back(); }
        free_.swap(m);
    }
};

static std::vector<int64_t> clast_phys_dims(const std::vector<int64_t>& d) {  // [n,C,s...] -> [n,s...,C]
    std::vector<int64_t> p;
    p.push_back(d[0]);
    for (size_t i = 2; i < d.size(); ++i) p.push_back(d[i]);
    p.push_back(d[1]);
    return p;
}
static std::vector<int64_t> contig_strides(const std::vector<int64_t>& d) {
    std::vector<int64_t> s(d.size(), 1);
    for (int i = (int)d.size() - 2; i >= 0; --i) s[i] = s[i + 1] * d[i + 1];
    return s;
}

struct Planner {
    Engine& E;
    Plan& P;
    std::map<std::string, TInfo> vals;
    std::map<std::string, int> last_use;      // by root name
    std::map<std::string, size_t> root_bytes; // arena-resident roots
    std::map<std::string, size_t> root_off;
    Arena arena;
    int cur = 0;
    std::vector<std::pair<size_t, size_t>> temps;  // freed after the current node

    Planner(Engine& e, Plan& p) : E(e), P(p) { opset = e.opset_; }

    // ------------------------------------------------------------------ deferred nearest Resize
    // A Resize with exactly one consumer is not run where it stands: its consumer either absorbs it (Concat on the channel axis:
    // the resize writes straight into its slot of the concatenated tensor; Add: the sum reads the low-resolution operand through
    // the index map) or, failing that, runs it first.  compute_last_use keeps the resize's input alive until that consumer.
    struct PendingResize {
        Loc xin;
        std::vector<int64_t> dims;   // logical output dims [N, C, Ho, Wo]
        int N, H, W, C, Ho, Wo, imode, ictm, inm;
        float sh, sw;
        int fh = 0, fw = 0;          // > 0: the index map is exactly o / f (integer-factor nearest upsampling)
    };
    std::map<std::string, PendingResize> pending_resize;
    std::map<std::string, int> sole_consumer;   // Resize output -> index of its only consumer node
    void run_resize(const PendingResize& r, Loc yl, int64_t y_off, int y_ld) {
        const PendingResize q = r;
        step([=](const RunCtx& c) { k::resize(c.s, c.at(q.xin), c.mut(yl) + y_off, q.N, q.H, q.W, q.C, q.Ho, q.Wo, q.sh, q.sw, q.imode, q.ictm, q.inm, y_ld); }, 0,
             4.0 * ((double)q.N * q.H * q.W * q.C + (double)q.N * q.Ho * q.Wo * q.C));
    }
    // A 2x2 / stride-2 ConvTranspose whose only consumer is another one (the DB head's tail) is held back the same way: the
    // consumer runs both as k::convt2x2_pair, anything else runs it first.
    std::map<std::string, const GNode*> pending_convt;
    // Round 6: a plain channel concat of channels-last maps whose ONLY reader is a 1x1 convolution the output-stationary bf16x6 kernel can take (PP-HGNetV2's
    // aggregation: seven maps, up to 3328 channels) is not written at all: the convolution reads its K dimension out of the sources (ConvP::msrc).  Anything
    // else that asks for the value first gets the gather launch.  compute_last_use keeps the sources alive until that reader.
    struct PendingConcat { std::vector<Loc> src; std::vector<int> c; std::vector<int64_t> dims; };
    std::map<std::string, PendingConcat> pending_concat;
    std::map<std::string, int> concat_consumer;   // Concat output -> index of its only consumer node
    void emit_concat_gather(const PendingConcat& pc, Loc yl) {
        k::ConcatGatherP gp{};
        gp.n_src = (int)pc.src.size(); gp.N = (int)pc.dims[0]; gp.Ho = (int)pc.dims[2]; gp.Wo = (int)pc.dims[3]; gp.C = (int)pc.dims[1];
        int off = 0;
        for (size_t i = 0; i < pc.src.size(); ++i) { gp.c[i] = pc.c[i]; gp.off[i] = off; gp.fh[i] = 1; gp.fw[i] = 1; off += pc.c[i]; }
        const std::vector<Loc> src = pc.src;
        step([=](const RunCtx& c) {
            k::ConcatGatherP q = gp;
            for (int i = 0; i < q.n_src; ++i) q.x[i] = c.at(src[(size_t)i]);
            k::concat_gather(c.s, q, c.mut(yl));
        }, 0, 8.0 * (double)numel(pc.dims));
    }
    void materialise_concat(const std::string& name) {
        auto it = pending_concat.find(name);
        if (it == pending_concat.end()) return;
        const PendingConcat pc = it->second;
        pending_concat.erase(it);
        vals.erase(name);
        TInfo& y = new_out(name, pc.dims, Layout::CLAST);
        emit_concat_gather(pc, y.loc);
    }
    const PendingResize* peek_pending(const std::string& name) const {
        auto it = pending_resize.find(name);
        return it == pending_resize.end() ? nullptr : &it->second;
    }
    void materialise_pending(const std::string& name) {
        auto ct = pending_convt.find(name);
        if (ct != pending_convt.end()) {
            const GNode* node = ct->second;
            pending_convt.erase(ct);
            vals.erase(name);
            op_convt(*node, /*may_defer=*/false);
            return;
        }
        auto it = pending_resize.find(name);
        if (it == pending_resize.end()) return;
        const PendingResize r = it->second;
        pending_resize.erase(it);
        TInfo& y = new_out(name, r.dims, Layout::CLAST);
        run_resize(r, y.loc, 0, r.C);
    }

    // ------------------------------------------------------------------ values
    TInfo& get(const std::string& name) {
        if (!pending_resize.empty() || !pending_convt.empty()) materialise_pending(name);
        if (!pending_concat.empty()) materialise_concat(name);
        auto it = vals.find(name);
        if (it != vals.end()) return it->second;
        auto ii = E.inits_.find(name);
        OAR_CHECK(ii != E.inits_.end(), OAR_MODEL_LOAD, "graph references unknown value '" + name + "'");
        TInfo t;
        t.dims = ii->second.dims;
        if (ii->second.dtype == DType::F32) {
            t.ht = &ii->second;
            t.loc.kind = Loc::CONST;
            t.loc.cptr = E.upload_const("init:" + name, ii->second.f);
        } else {
            t.host_int = true;
            t.hv = ii->second.i;
        }
        return vals[name] = t;
    }
    bool has_input(const GNode& n, size_t i) const { return i < n.in.size() && !n.in[i].empty(); }

    Loc alloc_arena(size_t bytes, const std::string& root) {
        Loc l;
        l.kind = Loc::ARENA;
        l.off = (int64_t)arena.alloc(bytes);
        P.arena_bytes = std::max(P.arena_bytes, arena.top);
        if (!root.empty()) { root_bytes[root] = bytes; root_off[root] = (size_t)l.off; }
        return l;
    }
    Loc alloc_temp(size_t bytes) {
        Loc l = alloc_arena(bytes, "");
        temps.push_back({(size_t)l.off, bytes});
        return l;
    }
    // root -> the values whose bytes lie in it (kept for check_release: only the aliases of the roots being freed are looked at).  Stale entries (a value since
    // re-planned or re-rooted) are skipped by comparing the value's current root.
    std::map<std::string, std::vector<std::string>> root_aliases;
    TInfo& new_out(const std::string& name, const std::vector<int64_t>& dims, Layout lay) {
        TInfo t;
        t.dims = dims; t.layout = lay; t.root = name;
        t.loc = alloc_arena(t.bytes(), name);
        root_aliases[name].push_back(name);
        return vals[name] = t;
    }
    // A node planned as several operators leaves its result as a VIEW of a temporary (e.g. pool -> "out::kept" -> Squeeze -> "out"): the arena bytes are then booked
    // under the temporary's name, which compute_last_use() knows nothing about -- release_dead() would free them right after the node although "out" is read later.
    // The node's output takes the booking over (round 6; tools/op_fuzz.py found a reduce whose result was overwritten by the next node's output).
    // Every other value in those bytes moves to the new root with it.
    void adopt_root(const std::string& out, const std::string& tmp) {
        auto it = vals.find(out);
        if (it == vals.end() || tmp.empty() || tmp == out || it->second.root != tmp) return;
        auto rb = root_bytes.find(tmp);
        if (rb != root_bytes.end()) { root_bytes[out] = rb->second; root_off[out] = root_off[tmp]; root_bytes.erase(tmp); root_off.erase(tmp); }
        std::vector<std::string> moved;
        moved.swap(root_aliases[tmp]);
        root_aliases.erase(tmp);
        std::vector<std::string>& dst = root_aliases[out];
        for (auto& a : moved) {
            auto va = vals.find(a);
            if (va != vals.end() && va->second.root == tmp) { va->second.root = out; dst.push_back(a); }
        }
        it->second.root = out;
    }
    TInfo& alias_out(const std::string& name, const TInfo& src, const std::vector<int64_t>& dims, Layout lay, int64_t byte_off = 0) {
        TInfo t;
        t.dims = dims; t.layout = lay; t.root = src.root; t.loc = src.loc; t.ht = nullptr;
        t.is_int = src.is_int;   // a view of a device index tensor (Reshape / Squeeze / Unsqueeze / Slice of one) is still one
        t.is01 = src.is01;       // ... and a view of a 0/1 mask still a mask
        if (t.loc.kind == Loc::CONST) t.loc.cptr = (const float*)((const char*)t.loc.cptr + byte_off);
        else t.loc.off += byte_off;
        if (!t.root.empty()) root_aliases[t.root].push_back(name);
        return vals[name] = t;
    }
    std::string node_label() const {
        const GNode* g = cur >= 0 && cur < (int)E.nodes_.size() ? &E.nodes_[(size_t)cur] : nullptr;
        return g ? g->op + " -> " + (g->out.empty() ? std::string("?") : g->out[0]) : std::string("?");
    }
    void step(std::function<void(const RunCtx&)> f, double flops = 0, double bytes = 0) {
        P.steps.push_back(std::move(f));
        P.flops += flops; P.bytes += bytes; P.n_kernels++;
        step_chain.push_back(-1);
        step_node.push_back(cur);
        static const bool dbg_steps = [] { const char* e = getenv("OAR_DEBUG_STEPS"); return e && atoi(e) != 0; }();
        if (dbg_steps) {
            const GNode* g = cur >= 0 && cur < (int)E.nodes_.size() ? &E.nodes_[(size_t)cur] : nullptr;
            P.step_ops.push_back(g ? g->op + " -> " + (g->out.empty() ? std::string("?") : g->out[0]) : std::string("?"));
        }
    }

    // ------------------------------------------------------------------ sample-local chains (csrc/chain.hip)
    // Operators that only read rows of their own sample (1 x k convolutions over H == 1 maps, Linear, LayerNorm, the fused SVTR
    // attention, row copies of a channel concat) record a ChainRec next to their step.  While the newest step is such an operator,
    // build() releases nothing (every tensor a run touches stays allocated until the run ends, so no two of them share arena bytes
    // and the samples of a fused run may advance at different paces); fuse_chains() then replaces each run by ONE chain_run step.
    struct ChainRec {
        k::ChainOpD d;
        Loc in, out, res;
        int64_t rows = 0;                 // rows of the operator's tensors (all samples)
        int64_t fix_n = 0, fix_T = 0;     // > 0: the operator fixes the partition (n samples of T rows); 0: any partition of its rows
        std::function<std::vector<float>()> make_w;   // GEMM weights as [N][K] f32 (host), built only when a chain is really formed
        const float* dev_bias = nullptr;  // GEMM bias / LN beta (device constant of N floats)
        const float* dev_gamma = nullptr; // LN gamma
        double flops = 0, bytes = 0;
        int node = 0;                     // graph node the operator belongs to
        std::string out_root;             // storage root of the tensor it writes (liveness: is it read after the run?)
    };
    std::vector<int> step_chain;          // parallel to P.steps: index into chain_recs, -1 = not chainable
    std::vector<int> step_node;           // parallel to P.steps: the graph node that emitted the step
    std::vector<ChainRec> chain_recs;
    bool chain_on = [] { const char* e = getenv("OAR_FUSE_CHAIN"); return !e || atoi(e) != 0; }();
    static bool chain_loc_ok(const Loc& l) { return l.kind == Loc::ARENA || l.kind == Loc::INPUT || (l.kind == Loc::CONST && l.cptr); }
    static k::ChainRef chain_ref(const Loc& l) {
        k::ChainRef r;
        if (l.kind == Loc::ARENA) { r.kind = 1; r.v = (unsigned long long)l.off; }
        else if (l.kind == Loc::INPUT) { r.kind = 2; r.v = (unsigned long long)l.off; }
        else if (l.kind == Loc::CONST) { r.kind = 0; r.v = (unsigned long long)reinterpret_cast<uintptr_t>(l.cptr); }
        return r;
    }
    void step_chainable(std::function<void(const RunCtx&)> f, ChainRec rec, double flops, double bytes) {
        step(std::move(f), flops, bytes);
        if (!chain_on) return;
        rec.flops = flops; rec.bytes = bytes; rec.node = cur;
        step_chain.back() = (int)chain_recs.size();
        chain_recs.push_back(std::move(rec));
    }
    bool chain_run_open() const { return chain_on && !step_chain.empty() && step_chain.back() >= 0; }
    static std::vector<float> chain_weight_conv(const HostTensor& W) {   // [Cout][Cin][1][kw] -> [Cout][kw * Cin]
        const int64_t Co = W.dims[0], Ci = W.dims[1], kw = W.dims[3], K = kw * Ci;
        std::vector<float> w((size_t)Co * K);
        for (int64_t co = 0; co < Co; ++co)
            for (int64_t ci = 0; ci < Ci; ++ci)
                for (int64_t b = 0; b < kw; ++b) w[(size_t)co * K + b * Ci + ci] = W.f[(size_t)((co * Ci + ci) * kw + b)];
        return w;
    }
    static std::vector<float> chain_weight_linear(const HostTensor& B, bool transB) {   // -> [N][K]
        const int64_t K = transB ? B.dims[1] : B.dims[0], N = transB ? B.dims[0] : B.dims[1];
        std::vector<float> w((size_t)N * K);
        for (int64_t kk = 0; kk < K; ++kk)
            for (int64_t nn = 0; nn < N; ++nn) w[(size_t)nn * K + kk] = transB ? B.f[(size_t)(nn * K + kk)] : B.f[(size_t)(kk * N + nn)];
        return w;
    }
    static constexpr int kMinChain = 3;
    bool chain_live_after(const std::string& root, int last_node) const {   // is the tensor read by a node after `last_node` (or a graph output)?
        if (root == "\x01stage") return false;   // a staging copy of fuse_chains: lives inside the run by construction
        auto it = last_use.find(root);
        return root.empty() || it == last_use.end() || it->second > last_node;
    }
    // Tensors a chain writes and nobody reads after it live in the workgroup's LDS (one sample's rows, each row padded by 4 floats so
    // that the 16 rows of a B operand start in different banks): the operators' references are rewritten to LDS offsets (ChainRef
    // kind 3) and their row strides to the padded one.  Liveness-based first-fit over the operator order; when the budget is
    // exceeded the largest tensor goes back to the arena and the placement is redone.  Returns the dynamic LDS size of the launch.
    // Split-K partials live at LDS offset 0, but only DURING their operator: `op_scratch[j]` bytes are reserved for operator j alone (a pseudo tensor
    // pinned at offset 0 with the lifetime [j, j]), so a tensor that is dead by then -- or born later -- may occupy the same bytes (round 5: with the pooling
    // operator inside the chain its 40 KB output pushed the 80 KB concat back to the arena while 24 KB of partials that no operator near it uses sat idle).
    size_t chain_place_in_lds(std::vector<k::ChainOpD>& ops, const std::vector<std::string>& out_roots, int last_node, int64_t n, int64_t T, const std::vector<size_t>& op_scratch, size_t budget) {
        size_t scratch = 0;
        for (size_t b : op_scratch) scratch = std::max(scratch, b);
        const char* lds_env = getenv("OAR_CHAIN_LDS");   // read per plan: tests A/B the placements inside one process
        const bool lds_on = !lds_env || atoi(lds_env) != 0;
        if (!lds_on || scratch >= budget) return scratch;
        struct Use { int op; int which; int64_t off; int ld; int width; };   // which: 0 in, 1 out, 2 res; width: columns the view covers
        std::vector<Use> uses;
        for (int j = 0; j < (int)ops.size(); ++j) {
            const k::ChainOpD& d = ops[(size_t)j];
            const int win = d.type == k::CH_GEMM ? d.cin : d.type == k::CH_ATTN ? 3 * d.heads * d.hd : d.N;
            if (d.in.kind == 1 && d.type != k::CH_POOL) uses.push_back({j, 0, (int64_t)d.in.v, d.in_ld, win});   // (a pool reads the sample's whole map from HBM: not a [n T][ld] tensor of the run)
            if (d.out.kind == 1) uses.push_back({j, 1, (int64_t)d.out.v, d.out_ld, d.N});
            if (d.res.kind == 1) uses.push_back({j, 2, (int64_t)d.res.v, d.res_ld, d.N});
        }
        struct Root { int64_t base, end; int ld; bool bad = false, written = false, live_out = false, in_lds = false; int first = 1 << 30, last = -1; size_t bytes = 0, off = 0; };
        std::vector<Root> roots;
        std::vector<int> order(uses.size());
        for (size_t i = 0; i < order.size(); ++i) order[i] = (int)i;
        std::sort(order.begin(), order.end(), [&](int a, int b) { return uses[(size_t)a].off < uses[(size_t)b].off; });
        std::vector<int> root_of(uses.size(), -1);
        for (int ui : order) {
            const Use& u = uses[(size_t)ui];
            const int64_t end = u.off + ((n * T - 1) * u.ld + u.width) * 4;
            if (roots.empty() || u.off >= roots.back().end) { Root r; r.base = u.off; r.end = end; r.ld = u.ld; roots.push_back(r); }
            Root& r = roots.back();
            r.end = std::max(r.end, end);
            if (u.ld != r.ld || u.off - r.base >= (int64_t)r.ld * 4) r.bad = true;
            root_of[(size_t)ui] = (int)roots.size() - 1;
        }
        for (size_t ui = 0; ui < uses.size(); ++ui) {
            Root& r = roots[(size_t)root_of[ui]];
            const Use& u = uses[ui];
            r.first = std::min(r.first, u.op); r.last = std::max(r.last, u.op);
            if (u.which == 1) {
                r.written = true;
                if (chain_live_after(out_roots[(size_t)u.op], last_node)) r.live_out = true;
            }
        }
        for (Root& r : roots) {
            r.bytes = (size_t)T * (size_t)(r.ld + 4) * 4;
            r.in_lds = r.written && !r.live_out && !r.bad;
            // a tensor written in the run must be written before it is read there (it is: the planner emits in dependency order)
        }
        size_t peak = 0;
        for (;;) {
            // first-fit by first definition; a slot is reusable by an operator's OUTPUT only when its tensor's last use is an earlier operator.
            // Candidates a tensor must avoid: every tensor placed before it whose life reaches its first operator, and the partials of every
            // operator inside its own life.
            std::vector<int> idx;
            for (int i = 0; i < (int)roots.size(); ++i) if (roots[(size_t)i].in_lds) idx.push_back(i);
            std::sort(idx.begin(), idx.end(), [&](int a, int b) { return roots[(size_t)a].first < roots[(size_t)b].first; });
            std::vector<int> placed;
            peak = scratch;
            for (int i : idx) {
                Root& r = roots[(size_t)i];
                std::vector<std::pair<size_t, size_t>> busy;   // [begin, end) byte ranges taken while r lives
                for (int a : placed) if (roots[(size_t)a].last >= r.first) busy.push_back({roots[(size_t)a].off, roots[(size_t)a].off + roots[(size_t)a].bytes});
                size_t part = 0;
                for (int j = std::max(0, r.first); j <= r.last && j < (int)op_scratch.size(); ++j) part = std::max(part, op_scratch[(size_t)j]);
                if (part) busy.push_back({0, part});
                std::sort(busy.begin(), busy.end());
                size_t off = 0;
                for (auto& b : busy) { if (off + r.bytes <= b.first) break; off = std::max(off, b.second); }
                r.off = off;
                peak = std::max(peak, off + r.bytes);
                placed.push_back(i);
            }
            if (peak <= budget || idx.empty()) break;
            int big = idx[0];
            for (int i : idx) if (roots[(size_t)i].bytes > roots[(size_t)big].bytes) big = i;
            roots[(size_t)big].in_lds = false;
        }
        for (size_t ui = 0; ui < uses.size(); ++ui) {
            const Root& r = roots[(size_t)root_of[ui]];
            if (!r.in_lds) continue;
            const Use& u = uses[ui];
            k::ChainOpD& d = ops[(size_t)u.op];
            k::ChainRef ref; ref.kind = 3; ref.v = (unsigned long long)(r.off + (size_t)(u.off - r.base));
            if (u.which == 0) { d.in = ref; d.in_ld = r.ld + 4; }
            else if (u.which == 1) { d.out = ref; d.out_ld = r.ld + 4; }
            else { d.res = ref; d.res_ld = r.ld + 4; }
        }
        return peak;
    }
    void fuse_chains() {
        if ((!chain_on || chain_recs.empty()) && add_ln_at.empty()) return;
        const int ns = (int)P.steps.size();
        std::vector<std::function<void(const RunCtx&)>> out;
        int fused_away = 0;
        int a = 0;
        std::vector<std::string> out_ops;
        const bool names = P.step_ops.size() == P.steps.size();
        // Add + LayerNorm: a step that stays a launch of its own goes through keep().  A LayerNorm that does (no chain took it) and whose marked Add was
        // kept right in front of it becomes ONE add_layernorm launch in the Add's place (same operands, same arithmetic: bit-identical to the pair).  Where the
        // step in front is a Linear that carries the residual (op_linear), the pair stays two launches: the Linear alone, then add_layernorm
        int last_kept = -2;
        auto keep = [&](int i) {
            auto al = add_ln_at.find(i);
            if (al != add_ln_at.end() && last_kept == i - 1 && !out.empty() && al->second.lin) {
                // behind a Linear that carries the residual: the Linear writes its product alone, and add_layernorm takes the LayerNorm's place
                out.back() = std::move(al->second.lin);
                out.push_back(std::move(al->second.run)); if (names) out_ops.push_back(al->second.label);
                last_kept = i;
                return;
            }
            if (al != add_ln_at.end() && last_kept == i - 1 && !out.empty()) {
                out.back() = std::move(al->second.run);
                if (names) out_ops.back() = al->second.label;
                P.bytes -= al->second.bytes_saved;
                ++fused_away;
                last_kept = i;
                return;
            }
            out.push_back(std::move(P.steps[(size_t)i])); if (names) out_ops.push_back(P.step_ops[(size_t)i]);
            last_kept = i;
        };
        while (a < ns) {
            if (step_chain[(size_t)a] < 0) { keep(a++); continue; }
            int b = a;
            while (b < ns && step_chain[(size_t)b] >= 0) ++b;
            // run [a, b): chains grow around each operator that fixes the partition
            int i = a;
            while (i < b) {
                int kf = i;
                while (kf < b && chain_recs[(size_t)step_chain[(size_t)kf]].fix_n == 0) ++kf;
                if (kf == b) break;
                const int64_t n = chain_recs[(size_t)step_chain[(size_t)kf]].fix_n, T = chain_recs[(size_t)step_chain[(size_t)kf]].fix_T;
                auto compat = [&](int j) {
                    const ChainRec& r = chain_recs[(size_t)step_chain[(size_t)j]];
                    return r.fix_n ? (r.fix_n == n && r.fix_T == T) : (r.rows == n * T);
                };
                if (n <= 0 || T <= 0 || T > 4096 || !compat(kf)) { for (int j = i; j <= kf; ++j) keep(j); i = kf + 1; continue; }
                int lo = kf, hi = kf + 1;
                while (lo > i && compat(lo - 1)) --lo;
                while (hi < b && compat(hi)) ++hi;
                for (int j = i; j < lo; ++j) keep(j);
                // one workgroup (one CU's f32 matrix pipe: 0.6 TFLOP/s) per sample: beyond ~32 MFLOP per sample the operator-by-operator
                // kernels, which spread every product over the whole chip, win again (a server-size SVTR neck is ~120 MFLOP per line)
                double run_flops = 0;
                for (int j = lo; j < hi; ++j) run_flops += chain_recs[(size_t)step_chain[(size_t)j]].flops;
                const char* mf_env = getenv("OAR_CHAIN_MAX_MFLOP");   // (read per plan: the tests lift the cap for their long-line cases)
                const double max_mflop = mf_env ? atof(mf_env) : 32.0;
                if (hi - lo < kMinChain || run_flops / (double)n > max_mflop * 1e6) { for (int j = lo; j < hi; ++j) keep(j); i = hi; continue; }
                std::vector<k::ChainOpD> ops;
                std::vector<std::string> out_roots;
                std::vector<const ChainRec*> recs;
                double flops = 0, bytes = 0;
                int max_hd = 0;
                int last_node = chain_recs[(size_t)step_chain[(size_t)(hi - 1)]].node;
                if ((size_t)hi < step_node.size() && step_node[(size_t)hi] == last_node) --last_node;   // the run was cut inside a node: that node's tensors stay in the arena
                for (int j = lo; j < hi; ++j) {
                    ChainRec& r = chain_recs[(size_t)step_chain[(size_t)j]];
                    k::ChainOpD d = r.d;
                    d.in = chain_ref(r.in); d.out = chain_ref(r.out); d.res = chain_ref(r.res);
                    if (d.type == k::CH_ATTN) max_hd = std::max(max_hd, d.hd);
                    flops += r.flops; bytes += r.bytes;
                    ops.push_back(d); out_roots.push_back(r.out_root); recs.push_back(&r);
                }
                // copy elision: a Concat input produced inside the run by one operator and read by nothing else is written where the copy
                // would have put it (the producer gets the copy's destination view) and the copy disappears
                for (int j = 0; j < (int)ops.size();) {
                    const k::ChainOpD& cp = ops[(size_t)j];
                    int prod = -1, readers = 0;
                    if (cp.type == k::CH_COPY && cp.in.kind == 1) {
                        for (int q = 0; q < (int)ops.size(); ++q) {
                            const k::ChainOpD& o = ops[(size_t)q];
                            if (q < j && o.out.kind == 1 && o.out.v == cp.in.v && o.out_ld == cp.in_ld && o.N == cp.N && o.type != k::CH_COPY) prod = q;
                            if (q != j && ((o.in.kind == 1 && o.in.v == cp.in.v) || (o.res.kind == 1 && o.res.v == cp.in.v))) ++readers;
                        }
                    }
                    if (prod >= 0 && readers == 0 && !chain_live_after(out_roots[(size_t)prod], last_node)) {
                        ops[(size_t)prod].out = cp.out; ops[(size_t)prod].out_ld = cp.out_ld;
                        out_roots[(size_t)prod] = out_roots[(size_t)j];
                        ops.erase(ops.begin() + j); out_roots.erase(out_roots.begin() + j); recs.erase(recs.begin() + j);
                        continue;
                    }
                    ++j;
                }
                // the chain's constants in one allocation: biases / LayerNorm affine vectors first (the kernel keeps them in LDS), then weights
                std::vector<float> blob;
                auto fetch = [&](const float* dev, int cnt) {   // a device constant back to the host (plan time only)
                    const int at = (int)blob.size();
                    blob.resize((size_t)at + (size_t)((cnt + 3) & ~3), 0.f);
                    OAR_HIP(hipMemcpy(blob.data() + at, dev, (size_t)cnt * 4, hipMemcpyDeviceToHost));
                    return at;
                };
                for (size_t q = 0; q < ops.size(); ++q) {
                    if (recs[q]->dev_bias && ops[q].type != k::CH_COPY) ops[q].bias_l = fetch(recs[q]->dev_bias, ops[q].N);
                    if (recs[q]->dev_gamma && ops[q].type == k::CH_LN) ops[q].w_l = fetch(recs[q]->dev_gamma, ops[q].N);
                }
                const int small = (int)blob.size();
                // a product whose tokens come from HBM (the run's input) gets them staged into LDS first: a row copy in front of it, its
                // destination a transient LDS tensor (a made-up arena address far above the real arena names it for the placement below)
                const unsigned long long kStageBase = 1ull << 50;
                for (size_t q = 0; q < ops.size(); ++q) {
                    if (ops[q].type != k::CH_GEMM || (ops[q].in.kind != 1 && ops[q].in.kind != 2)) continue;
                    bool produced_here = false;   // (tensors written earlier in the run are placed in LDS as they are)
                    for (size_t e = 0; e < q && ops[q].in.kind == 1; ++e) {
                        if (ops[e].out.kind != 1) continue;
                        const unsigned long long a0 = ops[q].in.v, a1 = a0 + (unsigned long long)(((n * T - 1) * ops[q].in_ld + ops[q].cin) * 4);
                        const unsigned long long b0 = ops[e].out.v, b1 = b0 + (unsigned long long)(((n * T - 1) * ops[e].out_ld + ops[e].N) * 4);
                        produced_here = produced_here || (a0 < b1 && b0 < a1);
                    }
                    if (produced_here) continue;
                    k::ChainOpD cp;
                    cp.type = k::CH_COPY; cp.N = ops[q].in_ld; cp.in_ld = ops[q].in_ld; cp.out_ld = ops[q].in_ld;
                    cp.in = ops[q].in;
                    cp.out.kind = 1; cp.out.v = kStageBase + ((unsigned long long)q << 40);
                    ops[q].in = cp.out;
                    ops.insert(ops.begin() + (long)q, cp); out_roots.insert(out_roots.begin() + (long)q, std::string("\x01stage")); recs.insert(recs.begin() + (long)q, nullptr);
                    ++q;
                }
                const int MT = (int)((T + 15) / 16);
                std::vector<size_t> w_at(ops.size(), 0);
                for (size_t q = 0; q < ops.size(); ++q) {
                    k::ChainOpD& d = ops[q];
                    if (d.type != k::CH_GEMM) continue;
                    blob.resize((blob.size() + 63) & ~(size_t)63, 0.f);
                    w_at[q] = blob.size();
                    const std::vector<float> w = recs[q]->make_w();
                    OAR_CHECK(w.size() == (size_t)d.N * (size_t)d.K, OAR_INTERNAL, "chain: weight size");
                    blob.insert(blob.end(), w.begin(), w.end());
                    // work items = channel tiles x token groups (mb tiles each) x K slices: enough of them for the 16 waves, partials <= 24 KB
                    // narrow products whose 16 x 16 tiles fit one round of the 16 waves take one tile per item (shortest dependent chain);
                    // the others share each weight load between up to 3 token tiles
                    const int NT = d.N / 16, KB = d.K / 16;
                    d.mb = (NT * MT <= 16 && KB <= 8) ? 1 : (MT <= 3 ? MT : (MT % 3 == 0 ? 3 : (MT % 2 == 0 ? 2 : 3)));
                    const int MG = (MT + d.mb - 1) / d.mb;
                    // (a 48 KB cap -- 16 items instead of 8 for the two long products K = 768 / 1536 -> 32 -- was measured: no faster per product, and the
                    // partials then push the 80 KB concat out of LDS: profiles/r5/chain_r5_endgame.txt)
                    int ks = 1;
                    while (NT * MG * ks < 16 && KB / (ks * 2) >= 2 && NT * MG * d.mb * ks * 2 <= 24) ks *= 2;
                    d.ksplit = ks;
                }
                std::vector<size_t> op_scratch(ops.size(), 0);
                for (size_t q = 0; q < ops.size(); ++q) op_scratch[q] = (k::chain_lds_bytes(ops[q], (int)T) + 255) & ~(size_t)255;
                auto consts = std::make_shared<DevBuf>();
                consts->reserve(blob.size() * 4 + 256);
                OAR_HIP(hipMemcpy(consts->p, blob.data(), blob.size() * 4, hipMemcpyHostToDevice));
                for (size_t q = 0; q < ops.size(); ++q) if (ops[q].type == k::CH_GEMM) ops[q].w = consts->as<float>() + w_at[q];
                const size_t small_bytes = (((size_t)small * 4 + 255) & ~(size_t)255) + ((ops.size() * sizeof(k::ChainOpD) + 255) & ~(size_t)255);   // + the table copy
                const size_t tens_end = chain_place_in_lds(ops, out_roots, last_node, n, T, op_scratch, k::kChainLdsBudget - small_bytes);
                for (size_t q = 0; q + 1 < ops.size();) {   // a staging copy that found no room: drop it, the product reads HBM (slow path)
                    if (ops[q].type == k::CH_COPY && ops[q].out.kind == 1 && ops[q].out.v >= kStageBase) {
                        ops[q + 1].in = ops[q].in; ops[q + 1].in_ld = ops[q].in_ld;
                        ops.erase(ops.begin() + (long)q); out_roots.erase(out_roots.begin() + (long)q); recs.erase(recs.begin() + (long)q); w_at.erase(w_at.begin() + (long)q);
                        continue;
                    }
                    ++q;
                }
                const int small_l = (int)(((tens_end + 255) & ~(size_t)255) / 4);
                for (auto& d : ops) { if (d.bias_l >= 0) d.bias_l += small_l; if (d.w_l >= 0) d.w_l += small_l; }
                auto table = std::make_shared<DevBuf>();
                table->reserve(ops.size() * sizeof(k::ChainOpD));
                OAR_HIP(hipMemcpy(table->p, ops.data(), ops.size() * sizeof(k::ChainOpD), hipMemcpyHostToDevice));
                k::ChainLaunch L;
                L.ops = table->as<k::ChainOpD>(); L.n_ops = (int)ops.size(); L.n_samples = (int)n; L.T = (int)T; L.max_hd = max_hd;
                L.lds = (size_t)small_l * 4 + small_bytes;
                L.tab_l = small_l + (int)((((size_t)small * 4 + 255) & ~(size_t)255) / 4);
                L.consts = consts->as<float>(); L.small = small; L.total_consts = (int)blob.size(); L.small_l = small_l;
                L.bytes = bytes; L.flops = flops;
                const int n_ops = hi - lo;
                out.push_back([L, table, consts](const RunCtx& c) { k::chain_run(c.s, L, c.arena, reinterpret_cast<const char*>(c.input)); });
                if (names) out_ops.push_back("chain of " + std::to_string(hi - lo) + " steps from " + P.step_ops[(size_t)lo]);
                fused_away += n_ops - 1;
                i = hi;
            }
            for (int j = i; j < b; ++j) keep(j);
            a = b;
        }
        P.steps.swap(out);
        if (names) P.step_ops.swap(out_ops);
        P.n_kernels -= fused_away;
        step_chain.assign(P.steps.size(), -1);
        step_node.assign(P.steps.size(), -1);
    }

    // ------------------------------------------------------------------ layout conversions
    Loc to_clast_loc(const TInfo& t) {  // native [n,C,s..] -> channels-last copy in a temp
        if (t.host_int) { TInfo d = t; d.host_int = false; d.layout = Layout::NATIVE; d.loc = host_to_device("", t); return to_clast_loc(d); }   // a plan-time value has no device bytes yet
        OAR_CHECK(t.loc.kind != Loc::NONE, OAR_INTERNAL, "planner: a tensor without storage reaches a kernel (node " + node_label() + ")");
        if (t.layout == Layout::CLAST) return t.loc;
        OAR_CHECK(t.dims.size() >= 3 && t.dims.size() <= 5, OAR_UNSUPPORTED_OP, "channels-last conversion needs rank 3..5");
        int r = (int)t.dims.size();
        bool trivial = t.dims[1] == 1;
        int64_t sp = 1;
        for (int i = 2; i < r; ++i) sp *= t.dims[i];
        if (trivial || sp == 1) return t.loc;
        Loc tmp = alloc_temp(t.bytes());
        std::vector<int64_t> od = clast_phys_dims(t.dims);
        std::vector<int64_t> ns = contig_strides(t.dims), is(r);
        is[0] = ns[0];
        for (int i = 2; i < r; ++i) is[i - 1] = ns[i];
        is[r - 1] = ns[1];
        Loc src = t.loc;
        step([=](const RunCtx& c) { k::permute(c.s, c.at(src), c.mut(tmp), r, od.data(), is.data()); }, 0, 2.0 * t.bytes());
        return tmp;
    }
    Loc to_native_loc(const TInfo& t, Loc dst = Loc()) {
        if (t.host_int) { TInfo d = t; d.host_int = false; d.layout = Layout::NATIVE; d.loc = host_to_device("", t); return to_native_loc(d, dst); }   // a plan-time value has no device bytes yet
        OAR_CHECK(t.loc.kind != Loc::NONE, OAR_INTERNAL, "planner: a tensor without storage reaches a kernel (node " + node_label() + ")");
        bool need = t.layout == Layout::CLAST;
        int r = (int)t.dims.size();
        if (need) {
            int64_t sp = 1;
            for (int i = 2; i < r; ++i) sp *= t.dims[i];
            if (t.dims[1] == 1 || sp == 1) need = false;
        }
        if (!need) {
            if (dst.kind == Loc::NONE) return t.loc;
            Loc src = t.loc;
            int64_t n = numel(t.dims);
            step([=](const RunCtx& c) { k::copy2d(c.s, c.at(src), c.mut(dst), 1, (int)n, (int)n, (int)n); }, 0, 2.0 * t.bytes());
            return dst;
        }
        if (dst.kind == Loc::NONE) dst = alloc_temp(t.bytes());
        std::vector<int64_t> pd = clast_phys_dims(t.dims), ps = contig_strides(pd), is(r);
        is[0] = ps[0];
        is[1] = ps[r - 1];
        for (int i = 2; i < r; ++i) is[i] = ps[i - 1];
        std::vector<int64_t> od = t.dims;
        Loc src = t.loc;
        step([=](const RunCtx& c) { k::permute(c.s, c.at(src), c.mut(dst), r, od.data(), is.data()); }, 0, 2.0 * t.bytes());
        return dst;
    }

    // ------------------------------------------------------------------ weights
    // [rows][K] row-major GEMM weights -> MFMA fragment order Wf[rows/16][KC][lane][4]
    // (lane = (row & 15) + 16 * g holds k = 16*kc + 4*g + j, j = 0..3); rows padded to 64, K to 16.
    static std::vector<float> to_fragment_order(const std::vector<float>& w, int64_t rows, int64_t K) {
        int64_t Rp = (rows + 63) / 64 * 64, KC = (K + 15) / 16;
        std::vector<float> f((size_t)Rp * KC * 16, 0.f);
        for (int64_t r = 0; r < rows; ++r)
            for (int64_t k = 0; k < K; ++k) {
                int64_t nf = r / 16, c = r % 16, kc = k / 16, g = (k % 16) / 4, j = k % 4;
                f[(size_t)(((nf * KC + kc) * 64 + (c + 16 * g)) * 4 + j)] = w[(size_t)r * K + k];
            }
        return f;
    }
    // [rows][K] f32 GEMM weights -> bf16x6 fragment order Wx[rows/16][K/32][3 planes][lane][8 bf16]
    // (lane = (row & 15) + 16 * g holds k = 32*kc + 8*g + e, e = 0..7; plane 0/1/2 = the h/m/l truncation pieces)
    static std::vector<float> to_fragment_x6(const std::vector<float>& w, int64_t rows, int64_t K) {
        int64_t Rp = (rows + 63) / 64 * 64, KC = (K + 31) / 32;
        std::vector<uint16_t> f((size_t)Rp * KC * 32 * 3, 0);
        for (int64_t r = 0; r < rows; ++r)
            for (int64_t k = 0; k < K; ++k) {
                float x = w[(size_t)r * K + k];
                uint32_t u, um, ul;
                std::memcpy(&u, &x, 4);
                uint32_t uh = u & 0xFFFF0000u;
                float fh; std::memcpy(&fh, &uh, 4);
                float r1 = x - fh;
                std::memcpy(&um, &r1, 4); um &= 0xFFFF0000u;
                float fm; std::memcpy(&fm, &um, 4);
                float r2 = r1 - fm;
                std::memcpy(&ul, &r2, 4); ul &= 0xFFFF0000u;
                int64_t nf = r / 16, c = r % 16, kc = k / 32, g = (k % 32) / 8, e = k % 8;
                size_t lane = (size_t)(c + 16 * g);
                size_t base = (size_t)((nf * KC + kc) * 3) * 64 * 8;
                f[base + (0 * 64 + lane) * 8 + e] = (uint16_t)(uh >> 16);
                f[base + (1 * 64 + lane) * 8 + e] = (uint16_t)(um >> 16);
                f[base + (2 * 64 + lane) * 8 + e] = (uint16_t)(ul >> 16);
            }
        std::vector<float> out(f.size() / 2);
        std::memcpy(out.data(), f.data(), f.size() * 2);
        return out;
    }
    // [rows][K] f32 GEMM weights -> the bf16x6 fragments of the row-streaming separable block (dsblock_rs.inc): Wr[rows/16][KP][3 planes][lane][8 bf16],
    // KP = ceil(ceil(K/16)/2) k-steps of two 16-channel chunks; lane = (row & 15) + 16 * g holds, for e = 0..3, k = 32*kp + 4*g + e (first chunk) and,
    // for e = 4..7, k = 32*kp + 16 + 4*g + (e - 4) (second chunk) -- the order in which that kernel's lanes hold the depthwise outputs
    static std::vector<float> to_fragment_x6_rs(const std::vector<float>& w, int64_t rows, int64_t K) {
        int64_t Rp = (rows + 63) / 64 * 64, KP = ((K + 15) / 16 + 1) / 2;
        std::vector<uint16_t> f((size_t)Rp * KP * 32 * 3, 0);
        for (int64_t r = 0; r < rows; ++r)
            for (int64_t k = 0; k < K; ++k) {
                float x = w[(size_t)r * K + k];
                uint32_t u, um, ul;
                std::memcpy(&u, &x, 4);
                uint32_t uh = u & 0xFFFF0000u;
                float fh; std::memcpy(&fh, &uh, 4);
                float r1 = x - fh;
                std::memcpy(&um, &r1, 4); um &= 0xFFFF0000u;
                float fm; std::memcpy(&fm, &um, 4);
                float r2 = r1 - fm;
                std::memcpy(&ul, &r2, 4); ul &= 0xFFFF0000u;
                int64_t nf = r / 16, c = r % 16, kp = k / 32, half = (k % 32) / 16, g = (k % 16) / 4, e = half * 4 + k % 4;
                size_t lane = (size_t)(c + 16 * g);
                size_t base = (size_t)((nf * KP + kp) * 3) * 64 * 8;
                f[base + (0 * 64 + lane) * 8 + e] = (uint16_t)(uh >> 16);
                f[base + (1 * 64 + lane) * 8 + e] = (uint16_t)(um >> 16);
                f[base + (2 * 64 + lane) * 8 + e] = (uint16_t)(ul >> 16);
            }
        std::vector<float> out(f.size() / 2);
        std::memcpy(out.data(), f.data(), f.size() * 2);
        return out;
    }
    static std::vector<float> to_fragments(int fmt, const std::vector<float>& w, int64_t rows, int64_t K) {
        if (fmt == k::IGEMM_W_X6RS) return to_fragment_x6_rs(w, rows, K);
        return fmt == k::IGEMM_W_X6 ? to_fragment_x6(w, rows, K) : to_fragment_order(w, rows, K);
    }
    const float* conv_weight_igemm(const GNode& n, const HostTensor& W, int fmt) {
        std::string key = "igemm" + std::to_string(fmt) + ":" + n.in[1];
        auto it = E.dev_consts_.find(key);
        if (it != E.dev_consts_.end()) return it->second;
        int64_t Co = W.dims[0], Ci = W.dims[1], kh = W.dims[2], kw = W.dims[3];
        int64_t K = kh * kw * Ci, Cp = (Co + 63) / 64 * 64;
        std::vector<float> w((size_t)Cp * K, 0.f);
        for (int64_t co = 0; co < Co; ++co)
            for (int64_t ci = 0; ci < Ci; ++ci)
                for (int64_t a = 0; a < kh; ++a)
                    for (int64_t b = 0; b < kw; ++b)
                        w[(size_t)co * K + (a * kw + b) * Ci + ci] = W.f[((co * Ci + ci) * kh + a) * kw + b];
        (void)Cp;
        w.resize((size_t)Co * K);
        return E.upload_const(key, to_fragments(fmt, w, Co, K));
    }
    // IGEMM_W_X6CS (dsblock_cs.inc): one block per 16-channel chunk c --
    //   [tap t = 0 .. ks*ks-1 | bias][g = 0..3] float4 = depthwise weights / bias of channels 16 c + 4 g .. + 3        (rounded up to 1 KB)
    //   per cout fragment f: lane (g, m = cout 16 f + m) -> 8 bytes w_l, 8 bytes w_h  (1 KB), then 8 bytes w_m (512 B)   (rounded up to 1 KB)
    // and after the last block the pointwise bias [Cout]
    // where w_h / w_m / w_l are the bf16 truncation pieces of W_pw[16 f + m][16 c + 4 g + e], e = 0..3
    const float* conv_weight_cs(const GNode& dwn, const GNode& pwn, const HostTensor& WD, const HostTensor& WP, const std::vector<float>* bias_dw, const std::vector<float>* bias_pw) {
        std::string key = "dscs:" + dwn.in[1] + ":" + pwn.in[1];
        auto it = E.dev_consts_.find(key);
        if (it != E.dev_consts_.end()) return it->second;
        const int64_t C = WD.dims[0], ks = WD.dims[2], Co = WP.dims[0], nch = C / 16, nft = Co / 16;
        const size_t blk = k::dsblock_cs_block_bytes((int)ks, (int)nft), dwb = (size_t)(((ks * ks + 1) * 64 + 1023) / 1024 * 1024);
        std::vector<float> out(blk * (size_t)nch / 4 + (size_t)Co, 0.f);   // + the pointwise bias [Cout] (zeros when the block has none)
        if (bias_pw) std::copy(bias_pw->begin(), bias_pw->begin() + Co, out.begin() + (ptrdiff_t)(blk * (size_t)nch / 4));
        auto split = [](float x, uint16_t& h, uint16_t& m, uint16_t& l) {
            uint32_t u, um, ul;
            std::memcpy(&u, &x, 4);
            const uint32_t uh = u & 0xFFFF0000u;
            float fh; std::memcpy(&fh, &uh, 4);
            const float r1 = x - fh;
            std::memcpy(&um, &r1, 4); um &= 0xFFFF0000u;
            float fm; std::memcpy(&fm, &um, 4);
            const float r2 = r1 - fm;
            std::memcpy(&ul, &r2, 4);
            h = (uint16_t)(uh >> 16); m = (uint16_t)(um >> 16); l = (uint16_t)(ul >> 16);
        };
        for (int64_t c = 0; c < nch; ++c) {
            char* b = reinterpret_cast<char*>(out.data()) + (size_t)c * blk;
            float* dw = reinterpret_cast<float*>(b);
            for (int64_t t = 0; t <= ks * ks; ++t)
                for (int64_t q = 0; q < 16; ++q) {
                    const int64_t ch = c * 16 + q;
                    dw[t * 16 + q] = t < ks * ks ? WD.f[(size_t)(ch * ks * ks + t)] : (bias_dw ? (*bias_dw)[(size_t)ch] : 0.f);
                }
            for (int64_t f = 0; f < nft; ++f) {
                uint16_t* lh = reinterpret_cast<uint16_t*>(b + dwb + (size_t)f * 1536);
                uint16_t* md = reinterpret_cast<uint16_t*>(b + dwb + (size_t)f * 1536 + 1024);
                for (int64_t g = 0; g < 4; ++g)
                    for (int64_t m = 0; m < 16; ++m)
                        for (int64_t e = 0; e < 4; ++e) {
                            uint16_t h, mm, l;
                            split(WP.f[(size_t)((f * 16 + m) * C + c * 16 + g * 4 + e)], h, mm, l);
                            const size_t lane = (size_t)(g * 16 + m);
                            lh[lane * 8 + e] = l; lh[lane * 8 + 4 + e] = h; md[lane * 4 + e] = mm;
                        }
            }
        }
        return E.upload_const(key, out);
    }
    const float* conv_weight_dw(const GNode& n, const HostTensor& W) {
        std::string key = "dw:" + n.in[1];
        auto it = E.dev_consts_.find(key);
        if (it != E.dev_consts_.end()) return it->second;
        int64_t C = W.dims[0], kh = W.dims[2], kw = W.dims[3];
        std::vector<float> w((size_t)C * kh * kw);
        for (int64_t c = 0; c < C; ++c)
            for (int64_t a = 0; a < kh; ++a)
                for (int64_t b = 0; b < kw; ++b) w[(size_t)(a * kw + b) * C + c] = W.f[(c * kh + a) * kw + b];
        return E.upload_const(key, w);
    }
    const float* conv_weight_direct(const GNode& n, const HostTensor& W) {
        std::string key = "direct:" + n.in[1];
        auto it = E.dev_consts_.find(key);
        if (it != E.dev_consts_.end()) return it->second;
        int64_t Co = W.dims[0], cpg = W.dims[1], kh = W.dims[2], kw = W.dims[3];
        std::vector<float> w((size_t)Co * cpg * kh * kw);
        for (int64_t co = 0; co < Co; ++co)
            for (int64_t ci = 0; ci < cpg; ++ci)
                for (int64_t a = 0; a < kh; ++a)
                    for (int64_t b = 0; b < kw; ++b)
                        w[(size_t)(((a * kw + b) * cpg + ci) * Co + co)] = W.f[((co * cpg + ci) * kh + a) * kw + b];
        return E.upload_const(key, w);
    }
    const float* convt_weight(const GNode& n, const HostTensor& W, bool igemm, int fmt = 0) {
        std::string key = (igemm ? "convt_ig" + std::to_string(fmt) + ":" : std::string("convt_dir:")) + n.in[1];
        auto it = E.dev_consts_.find(key);
        if (it != E.dev_consts_.end()) return it->second;
        int64_t Ci = W.dims[0], Co = W.dims[1], kh = W.dims[2], kw = W.dims[3];
        std::vector<float> w;
        if (igemm) {
            int64_t rows = kh * kw * Co;
            w.assign((size_t)rows * Ci, 0.f);
            for (int64_t ci = 0; ci < Ci; ++ci)
                for (int64_t co = 0; co < Co; ++co)
                    for (int64_t a = 0; a < kh; ++a)
                        for (int64_t b = 0; b < kw; ++b)
                            w[(size_t)((a * kw + b) * Co + co) * Ci + ci] = W.f[((ci * Co + co) * kh + a) * kw + b];
            w = to_fragments(fmt, w, rows, Ci);
        } else {
            w.assign((size_t)kh * kw * Ci * Co, 0.f);
            for (int64_t ci = 0; ci < Ci; ++ci)
                for (int64_t co = 0; co < Co; ++co)
                    for (int64_t a = 0; a < kh; ++a)
                        for (int64_t b = 0; b < kw; ++b)
                            w[(size_t)(((a * kw + b) * Ci + ci) * Co + co)] = W.f[((ci * Co + co) * kh + a) * kw + b];
        }
        return E.upload_const(key, w);
    }
    const float* linear_weight(const std::string& name, const HostTensor& B, bool transB, int fmt) {
        std::string key = "lin" + std::to_string(fmt) + ":" + (transB ? "t:" : "") + name;
        auto it = E.dev_consts_.find(key);
        if (it != E.dev_consts_.end()) return it->second;
        int64_t K = transB ? B.dims[1] : B.dims[0], N = transB ? B.dims[0] : B.dims[1];
        std::vector<float> w((size_t)N * K, 0.f);
        for (int64_t kk = 0; kk < K; ++kk)
            for (int64_t nn = 0; nn < N; ++nn) w[(size_t)nn * K + kk] = transB ? B.f[nn * K + kk] : B.f[kk * N + nn];
        return E.upload_const(key, to_fragments(fmt, w, N, K));
    }

    // ------------------------------------------------------------------ ops
    void get_pads(const GNode& n, int64_t H, int64_t W, int64_t kh, int64_t kw, int64_t sh, int64_t sw, int64_t dh, int64_t dw,
                  int64_t& pt, int64_t& pl, int64_t& pb, int64_t& pr) {
        std::vector<int64_t> pads = n.ais("pads");
        pt = pl = pb = pr = 0;
        if (pads.size() == 4) { pt = pads[0]; pl = pads[1]; pb = pads[2]; pr = pads[3]; }
        std::string ap = n.as("auto_pad", "NOTSET");
        if (ap == "SAME_UPPER" || ap == "SAME_LOWER") {
            int64_t oh = (H + sh - 1) / sh, ow = (W + sw - 1) / sw;
            int64_t th = std::max<int64_t>((oh - 1) * sh + (kh - 1) * dh + 1 - H, 0), tw = std::max<int64_t>((ow - 1) * sw + (kw - 1) * dw + 1 - W, 0);
            if (ap == "SAME_UPPER") { pt = th / 2; pb = th - pt; pl = tw / 2; pr = tw - pl; }
            else { pb = th / 2; pt = th - pb; pr = tw / 2; pl = tw - pr; }
        }
    }

    void op_conv(const GNode& n) {
        if (n.in.size() > 3 && !n.in[3].empty()) {   // rewrite pass 8: a squeeze-excite gate rides on this 1x1 conv
            TInfo xg = get(n.in[0]), gt = get(n.in[3]);
            const TInfo& wg = get(n.in[1]);
            bool ok = xg.dims.size() == 4 && !xg.host_int && !gt.host_int && wg.ht && wg.ht->dims.size() == 4 && gt.loc.kind != Loc::NONE && n.residual.empty();
            if (ok) {
                const int64_t N = xg.dims[0], C = xg.dims[1], HW = xg.dims[2] * xg.dims[3];
                ok = numel(gt.dims) == N * C && gt.dims.size() >= 2 && gt.dims[0] == N && gt.dims[1] == C && wg.ht->dims[1] == C && C % 8 == 0 &&
                     k::conv_igemm_se_ok(N * HW, (int)C, (int)wg.ht->dims[0], (int)HW);
            }
            if (!ok) {   // the Mul after all, then the plain conv
                GNode mul;
                mul.op = "Mul"; mul.in = {n.in[0], n.in[3]}; mul.out = {n.out[0] + "::se"};
                op_binary(mul, 2);
                GNode c2 = n;
                c2.in.resize(3);
                c2.in[0] = mul.out[0];
                op_conv(c2);
                return;
            }
        }
        PendingConcat msrc;   // non-empty: the input is a deferred concat this convolution reads source by source
        {
            auto pit = pending_concat.find(n.in[0]);
            if (pit != pending_concat.end()) {
                auto wi = E.inits_.find(n.in.size() > 1 ? n.in[1] : std::string());
                const std::vector<int64_t>& pd = pit->second.dims;
                const bool still_ok = wi != E.inits_.end() && wi->second.dims.size() == 4 && wi->second.dims[2] == 1 && wi->second.dims[3] == 1 && n.residual.empty() &&
                                      !(n.in.size() > 3 && !n.in[3].empty()) && n.out.size() == 1 &&
                                      k::conv_msrc_ok((long)(pd[0] * pd[2] * pd[3]), (int)pd[1], (int)wi->second.dims[0]);
                if (still_ok) { msrc = pit->second; TInfo keep = vals[n.in[0]]; pending_concat.erase(pit); vals[n.in[0]] = keep; }
            }
        }
        TInfo x = get(n.in[0]);
        OAR_CHECK(x.dims.size() == 4, OAR_UNSUPPORTED_OP, "Conv: only 2-D convolutions are supported");
        const TInfo& wt = get(n.in[1]);
        OAR_CHECK(wt.ht, OAR_UNSUPPORTED_OP, "Conv: weights must be an initializer");
        const HostTensor& W = *wt.ht;
        OAR_CHECK(W.dims.size() == 4 && W.dims[0] > 0 && W.dims[1] > 0 && W.dims[2] > 0 && W.dims[3] > 0, OAR_MODEL_LOAD, "Conv: weight must be rank 4 with positive dims at " + n.out[0]);
        int64_t N = x.dims[0], Cin = x.dims[1], H = x.dims[2], Wd = x.dims[3];
        int64_t Cout = W.dims[0], kh = W.dims[2], kw = W.dims[3], g = n.ai("group", 1);
        OAR_CHECK(g >= 1 && W.dims[1] * g == Cin && Cout % g == 0, OAR_SHAPE_MISMATCH, "Conv: weight/input channel mismatch at " + n.out[0]);
        if (has_input(n, 2)) { const TInfo& bt = get(n.in[2]); OAR_CHECK(bt.ht && (int64_t)bt.ht->f.size() == Cout, OAR_MODEL_LOAD, "Conv: bias must be an f32 initializer of Cout elements at " + n.out[0]); }
        auto st = n.ais("strides"), dl = n.ais("dilations");
        int64_t sh = st.size() == 2 ? st[0] : 1, sw = st.size() == 2 ? st[1] : 1;
        int64_t dh = dl.size() == 2 ? dl[0] : 1, dw = dl.size() == 2 ? dl[1] : 1;
        int64_t pt, pl, pb, pr;
        get_pads(n, H, Wd, kh, kw, sh, sw, dh, dw, pt, pl, pb, pr);
        int64_t Ho = (H + pt + pb - dh * (kh - 1) - 1) / sh + 1, Wo = (Wd + pl + pr - dw * (kw - 1) - 1) / sw + 1;
        if (x.u8_stem) {   // Engine::run_stem: the stem reads the u8 pages and normalises on the fly (kernels.h StemU8)
            OAR_CHECK(g == 1 && Cin == 3 && kh * kw * 3 <= 128 && n.residual.empty(), OAR_INTERNAL, "run_stem on a graph whose first node is not an RGB stem");
            const float* sb = has_input(n, 2) ? get(n.in[2]).loc.cptr : nullptr;
            TInfo& ys = new_out(n.out[0], {N, Cout, Ho, Wo}, Layout::CLAST);
            k::ConvP sp{};
            sp.N = (int)N; sp.H = (int)H; sp.W = (int)Wd; sp.Cin = 3; sp.Ho = (int)Ho; sp.Wo = (int)Wo; sp.Cout = (int)Cout;
            sp.kh = (int)kh; sp.kw = (int)kw; sp.sh = (int)sh; sp.sw = (int)sw; sp.pt = (int)pt; sp.pl = (int)pl; sp.dh = (int)dh; sp.dw = (int)dw;
            sp.groups = 1; sp.act = n.act; sp.bias = sb; sp.y_ld = (int)Cout; sp.convt2x2 = 0;
            sp.w = conv_weight_direct(n, W);
            const Loc ysl = ys.loc;
            step([=](const RunCtx& c) {
                OAR_CHECK(c.stem != nullptr, OAR_INTERNAL, "stem plan run without pages");
                k::ConvP q = sp;
                q.y = c.mut(ysl);
                k::conv_smallcin_u8(c.s, q, *c.stem);
            }, 2.0 * N * Ho * Wo * Cout * 3 * kh * kw, 3.0 * N * H * Wd + 4.0 * N * Ho * Wo * Cout);
            return;
        }
        Loc xin = msrc.src.empty() ? to_clast_loc(x) : Loc();   // (a deferred concat has no storage of its own)
        const float* bias = has_input(n, 2) ? get(n.in[2]).loc.cptr : nullptr;
        Loc res;
        int res_up = 0;
        if (!n.residual.empty()) {
            // the other operand of the folded Add is a deferred nearest upsampling by an integer factor (the top-down path of an FPN): the
            // conv's epilogue reads the low-resolution tensor through the index map -- the upsampled tensor is never written or re-read
            const char* up_env = getenv("OAR_FUSE_RES_UP");   // (read per plan: the test compares both forms in one process)
            const bool up_on = !up_env || atoi(up_env) != 0;
            if (const PendingResize* pr = peek_pending(n.residual)) {
                const bool f32_tile = g == 1 && Cin % 4 == 0 && Cout % 4 == 0 &&
                                      k::igemm_weight_format((long)(N * Ho * Wo), (int)(kh * kw * Cin), (int)Cout, kh == 1 && kw == 1 && sh == 1 && sw == 1 && pt == 0 && pl == 0, (int)Cin) == k::IGEMM_W_K16;
                if (up_on && f32_tile && pr->fh > 1 && pr->fh == pr->fw && pr->N == N && pr->C == Cout && pr->Ho == Ho && pr->Wo == Wo && Ho % pr->fh == 0 && Wo % pr->fw == 0 &&
                    pr->H * pr->fh == Ho && pr->W * pr->fw == Wo && N * Ho * Wo < ((int64_t)1 << 31)) {
                    res = pr->xin;
                    res_up = pr->fh;
                    pending_resize.erase(n.residual);
                }
            }
        }
        if (!n.residual.empty() && res_up == 0) {
            TInfo r = get(n.residual);
            if (r.host_int || r.dims != std::vector<int64_t>{N, Cout, Ho, Wo}) {
                // the folded Add broadcasts: plan the conv and the add separately after all
                GNode pre = n;
                pre.residual.clear();
                pre.out[0] = n.out[0] + "::pre";
                op_conv(pre);
                GNode add;
                add.op = "Add"; add.in = {pre.out[0], n.residual}; add.out = {n.out[0]};
                op_binary(add, 0);
                return;
            }
            res = to_clast_loc(r);
        }
        TInfo& y = new_out(n.out[0], {N, Cout, Ho, Wo}, Layout::CLAST);
        k::ConvP p{};
        p.N = (int)N; p.H = (int)H; p.W = (int)Wd; p.Cin = (int)Cin; p.Ho = (int)Ho; p.Wo = (int)Wo; p.Cout = (int)Cout;
        p.kh = (int)kh; p.kw = (int)kw; p.sh = (int)sh; p.sw = (int)sw; p.pt = (int)pt; p.pl = (int)pl; p.dh = (int)dh; p.dw = (int)dw;
        p.groups = (int)g; p.act = n.act; p.bias = bias; p.y_ld = (int)Cout; p.convt2x2 = 0; p.res_up = res_up;
        int kind;  // 0 igemm, 1 dw, 2 direct, 3 grouped igemm
        // a grouped k x k convolution with wide groups (SVTRv2's local mixing: 5x5, 32 channels per group) is one implicit GEMM per group on the
        // output-stationary bf16x6 kernel, which reads its Cin / g channels out of the full tensor (ConvP::x_ld) and writes its Cout / g channels
        // into the full output (y_ld); the direct kernel it ran on before took 5.3 ms per layer (6.7 TFLOP/s).  OAR_GROUPED_X6=0 restores that
        const int64_t cg = Cin / g, og = Cout / g;
        const char* gx_env = getenv("OAR_GROUPED_X6");
        const bool grouped_x6 = g > 1 && g < Cin && cg % 8 == 0 && og % 4 == 0 && !(n.in.size() > 3 && !n.in[3].empty()) && res_up == 0 && !(gx_env && gx_env[0] == '0') &&
                                k::conv_grouped_x6_ok((long)(N * Ho * Wo), (int)(kh * kw * cg), (int)og, (int)cg);
        std::vector<const float*> wgrp;
        std::vector<int> slices3;
        if (grouped_x6) {
            kind = 3;
            p.w_fmt = k::IGEMM_W_X6;
            const size_t per = (size_t)(og * cg * kh * kw);
            for (int64_t gi = 0; gi < g; ++gi) {
                HostTensor Wg;
                Wg.dtype = DType::F32; Wg.dims = {og, cg, kh, kw};
                Wg.f.assign(W.f.begin() + (ptrdiff_t)(gi * per), W.f.begin() + (ptrdiff_t)((gi + 1) * per));
                GNode gn = n;
                gn.in[1] = n.in[1] + "::group" + std::to_string(gi);
                wgrp.push_back(conv_weight_igemm(gn, Wg, k::IGEMM_W_X6));
            }
        }
        else if (g == 1 && Cout <= 16 && Cin > 64 && kh == 3 && kw == 3 && sh == 1 && sw == 1 && pt == 1 && pl == 1 && dh == 1 && dw == 1 && Ho == H && Wo == Wd && n.residual.empty() &&
                 !(n.in.size() > 3 && !n.in[3].empty()) && !(slices3 = k::conv3x3_n16_slices((long)(N * Ho * Wo), (int)Cin, (int)Cout, (long)(H * Wd), (int)(4 * Cout))).empty()) {
            // the row-streaming bf16x6 kernel keeps a slice's weights in registers: 96 ... 256 input channels run as passes over 64- / 32-channel slices, every pass
            // after the first adding to the partial sums in y (the 0.445 M-parameter detector's neck: 96 -> 16 at quarter resolution ran on the f32 kernel, 201 us per 8 pages)
            kind = 4;
            p.w_fmt = k::IGEMM_W_X6;
            int64_t c0 = 0;
            for (int cs : slices3) {
                HostTensor Ws;
                Ws.dtype = DType::F32; Ws.dims = {Cout, (int64_t)cs, kh, kw};
                Ws.f.resize((size_t)(Cout * cs * 9));
                for (int64_t co = 0; co < Cout; ++co)
                    for (int64_t ci = 0; ci < cs; ++ci)
                        for (int64_t t = 0; t < 9; ++t) Ws.f[(size_t)((co * cs + ci) * 9 + t)] = W.f[(size_t)((co * Cin + c0 + ci) * 9 + t)];
                GNode gn = n;
                gn.in[1] = n.in[1] + "::slice" + std::to_string(c0);
                wgrp.push_back(conv_weight_igemm(gn, Ws, k::IGEMM_W_X6));
                c0 += cs;
            }
        }
        else if (g == 1 && Cin % 4 == 0) {
            kind = 0;
            const bool is1x1 = kh == 1 && kw == 1 && sh == 1 && sw == 1 && pt == 0 && pl == 0;
            const bool same3x3 = kh == 3 && kw == 3 && sh == 1 && sw == 1 && pt == 1 && pl == 1 && dh == 1 && dw == 1 && Ho == H && Wo == Wd && n.residual.empty();
            const bool lk_ok = !(n.in.size() > 3 && !n.in[3].empty()) && res_up == 0 &&
                               k::conv_lk_x6_eligible((int)kh, (int)kw, (int)sh, (int)sw, (int)pt, (int)pl, (int)dh, (int)dw, (int)H, (int)Wd, (int)Ho, (int)Wo, (int)Cin, (int)Cout, (int)(4 * Cout), (long)(N * Ho * Wo));
            p.w_fmt = k::igemm_weight_format((long)(N * Ho * Wo), (int)(kh * kw * Cin), (int)Cout, is1x1, (int)Cin, same3x3 ? (long)(H * Wd) : 0, lk_ok);
            p.w = conv_weight_igemm(n, W, p.w_fmt);
        }
        else if (g == Cin && g == Cout && Cout % 4 == 0) { kind = 1; p.w = conv_weight_dw(n, W); }
        else { kind = 2; p.w = conv_weight_direct(n, W); }
        Loc yl = y.loc;
        bool has_res = res.kind != Loc::NONE;
        Loc gate;   // [N][Cin] squeeze-excite gate folded into the load (checked above)
        if (n.in.size() > 3 && !n.in[3].empty()) {
            OAR_CHECK(kind == 0 && (p.w_fmt == k::IGEMM_W_X6 || p.w_fmt == k::IGEMM_W_K16), OAR_INTERNAL, "Conv: gate on a layer that is on neither gated kernel");
            gate = get(n.in[3]).loc;
        }
        const bool has_gate = gate.kind != Loc::NONE;
        double flops = 2.0 * N * Ho * Wo * Cout * (Cin / g) * kh * kw;
        double bytes = 4.0 * (N * H * Wd * Cin + N * Ho * Wo * Cout * (has_res ? 2 : 1) + numel(W.dims));
        if (n.out.size() > 1) {   // rewrite pass 9: out[1] = GlobalAveragePool(out[0])
            const int tiles = kind == 1 ? k::conv_dw_gap_tiles(p) : 0;
            if (tiles > 0 && Cout <= 1024 && n.ai("gap_raw", 0) != 0) {   // the only reader is an SEGate: it reduces the tile sums itself
                TInfo& gy = new_out(n.out[1], {N, (int64_t)tiles * Cout, 1, 1}, Layout::CLAST);
                gy.gap_tiles = tiles; gy.gap_hw = (int)(Ho * Wo);
                const Loc part = gy.loc;
                step([=](const RunCtx& c) {
                    k::ConvP q = p;
                    q.x = c.at(xin); q.y = c.mut(yl); q.residual = has_res ? c.at(res) : nullptr; q.gap_part = c.mut(part);
                    k::conv_dw(c.s, q);
                }, flops, bytes + 4.0 * N * tiles * Cout);
                return;
            }
            if (tiles > 0 && Cout <= 1024) {
                TInfo& gy = new_out(n.out[1], {N, Cout, 1, 1}, Layout::CLAST);
                const Loc gl = gy.loc, part = alloc_temp((size_t)N * tiles * Cout * sizeof(float));
                const int hw = (int)(Ho * Wo);
                step([=](const RunCtx& c) {
                    k::ConvP q = p;
                    q.x = c.at(xin); q.y = c.mut(yl); q.residual = has_res ? c.at(res) : nullptr; q.gap_part = c.mut(part);
                    k::conv_dw(c.s, q);
                }, flops, bytes + 4.0 * N * tiles * Cout);
                step([=](const RunCtx& c) { k::global_avgpool_finish(c.s, c.at(part), c.mut(gl), (int)N, tiles, (int)Cout, hw); }, 0, 4.0 * N * tiles * Cout);
                return;
            }
        }
        const bool from_concat = !msrc.src.empty();
        OAR_CHECK(!from_concat || (kind == 0 && p.w_fmt == k::IGEMM_W_X6), OAR_INTERNAL, "Conv: deferred concat in front of a layer that is not on the bf16x6 kernels");
        auto run = [=](const RunCtx& c) {
            k::ConvP q = p;
            q.y = c.mut(yl); q.residual = has_res ? c.at(res) : nullptr; q.se = has_gate ? c.at(gate) : nullptr;
            if (from_concat) {
                q.x = nullptr; q.n_msrc = (int)msrc.src.size();
                for (int i = 0; i < q.n_msrc; ++i) { q.msrc[i] = c.at(msrc.src[(size_t)i]); q.msrc_c[i] = msrc.c[(size_t)i]; }
            } else {
                q.x = c.at(xin);
            }
            if (kind == 3) {
                const int ng = p.groups, cgi = p.Cin / ng, ogi = p.Cout / ng;
                for (int gi = 0; gi < ng; ++gi) {
                    k::ConvP r = q;
                    r.groups = 1; r.Cin = cgi; r.Cout = ogi; r.x_ld = p.Cin;
                    r.x = q.x + (size_t)gi * cgi; r.y = q.y + (size_t)gi * ogi; r.w = wgrp[(size_t)gi];
                    r.bias = q.bias ? q.bias + (size_t)gi * ogi : nullptr;
                    r.residual = q.residual ? q.residual + (size_t)gi * ogi : nullptr;
                    k::conv_igemm(c.s, r);
                }
                return;
            }
            if (kind == 4) {
                int c0 = 0;
                for (size_t i = 0; i < slices3.size(); ++i) {
                    k::ConvP r = q;
                    r.Cin = slices3[i]; r.x_ld = p.Cin; r.x = q.x + c0; r.w = wgrp[i]; r.accum = i > 0 ? 1 : 0;
                    if (i > 0) r.bias = nullptr;
                    if (i + 1 < slices3.size()) r.act = k::Act{};
                    k::conv_igemm(c.s, r);
                    c0 += slices3[i];
                }
                return;
            }
            if (kind == 0) k::conv_igemm(c.s, q);
            else if (kind == 1) k::conv_dw(c.s, q);
            else k::conv_direct(c.s, q);
        };
        auto pool_after = [&]() {   // the pooled output without a pooled kernel variant: an ordinary GlobalAveragePool of out[0]
            if (n.out.size() < 2) return;
            GNode gp;
            gp.op = "GlobalAveragePool"; gp.in = {n.out[0]}; gp.out = {n.out[1]};
            op_gap(gp);
        };
        // a 1 x k convolution over a one-row map is a product over the rows of each sample: chainable (chain.hip)
        if (kind == 0 && !has_gate && H == 1 && Ho == 1 && kh == 1 && pt == 0 && pb == 0 && sw == 1 && dw == 1 && Wo == Wd && Cin % 16 == 0 && Cout % 16 == 0 && k::chain_act_ok(n.act.kind) &&
            chain_loc_ok(xin) && (!has_res || chain_loc_ok(res))) {
            ChainRec r;
            r.d.type = k::CH_GEMM; r.d.K = (int)(kw * Cin); r.d.N = (int)Cout; r.d.cin = (int)Cin; r.d.pad = (int)pl;
            r.d.in_ld = (int)Cin; r.d.out_ld = (int)Cout; r.d.res_ld = (int)Cout;
            r.d.act = n.act.kind; r.d.alpha = n.act.alpha; r.d.beta = n.act.beta; r.dev_bias = bias;
            r.in = xin; r.out = yl; if (has_res) r.res = res;
            r.rows = N * Wd; r.out_root = n.out[0];
            if (kw > 1) { r.fix_n = N; r.fix_T = Wd; }
            const HostTensor* Wp = &W;
            r.make_w = [Wp]() { return chain_weight_conv(*Wp); };
            step_chainable(run, std::move(r), flops, bytes);
            pool_after();
            return;
        }
        step(run, flops, bytes);
        pool_after();
    }

    // fused depthwise-separable block (rewrite pass 7)
    // shape part of a DSBlock node's parameters for an [N, C, H, W] input; false when the node is not a plain block
    bool dsblock_shape(const GNode& n, int64_t N, int64_t C, int64_t H, int64_t W, k::DsBlockP& p) {
        const TInfo &wdt = get(n.in[1]), &wpt = get(n.in[3]);
        if (!wdt.ht || !wpt.ht) return false;
        const HostTensor &WD = *wdt.ht, &WP = *wpt.ht;
        const int64_t ks = WD.dims[2], Cout = WP.dims[0];
        if (WD.dims[0] != C || WP.dims[1] != C) return false;
        auto st = n.ais("strides");
        const int64_t sh = st.size() == 2 ? st[0] : 1, sw = st.size() == 2 ? st[1] : 1;
        int64_t pt, pl, pb, pr;
        get_pads(n, H, W, ks, ks, sh, sw, 1, 1, pt, pl, pb, pr);
        const int64_t Ho = (H + pt + pb - (ks - 1) - 1) / sh + 1, Wo = (W + pl + pr - (ks - 1) - 1) / sw + 1;
        p = k::DsBlockP{};
        p.N = (int)N; p.H = (int)H; p.W = (int)W; p.C = (int)C; p.Ho = (int)Ho; p.Wo = (int)Wo; p.Cout = (int)Cout;
        p.ks = (int)ks; p.sh = (int)sh; p.sw = (int)sw; p.pt = (int)pt; p.pl = (int)pl;
        p.act1.kind = (int)n.ai("act1", 0); p.act1.alpha = n.af("act1_alpha", 0.f); p.act1.beta = n.af("act1_beta", 0.f);
        p.act2 = n.act; p.y_ld = (int)Cout;
        p.has_res = !n.residual.empty();
        return Ho > 0 && Wo > 0;
    }
    // DSBlock n followed by a DSBlock that is the ONLY reader of its output: one launch, the tensor between them never exists (csrc/dsblock_rs2.inc).
    // Decided here, at plan time, because eligibility depends on the shapes; the second node is then skipped by build().
    // May DSBlock node i be fused with node i + 1 as far as the GRAPH is concerned: i + 1 is a DSBlock reading i's output as its data input and nothing else does.
    bool dsblock_link_ok(int i) {
        if (i + 1 >= (int)E.nodes_.size()) return false;
        const GNode &n = E.nodes_[i], &m = E.nodes_[i + 1];
        if (n.op != "DSBlock" || m.op != "DSBlock" || !n.residual.empty() || !m.residual.empty() || m.in.empty() || m.in[0] != n.out[0]) return false;
        for (auto& o : E.output_names_) if (o == n.out[0]) return false;
        for (int j = 0; j < (int)E.nodes_.size(); ++j) {   // nobody else reads the intermediate tensor
            if (j == i + 1) continue;
            const GNode& q = E.nodes_[j];
            for (auto& s : q.in) if (s == n.out[0]) return false;
            if (q.residual == n.out[0]) return false;
        }
        for (size_t k = 1; k < m.in.size(); ++k) if (m.in[k] == n.out[0]) return false;
        return true;
    }
    // The pairing of a maximal run of chained DSBlocks, decided ONCE when its first block is planned (the round-5 rule decided per node --
    // "defer when the next pair is wider" -- and in a run of four or more blocks of growing width every block deferred, so only the last pair fused):
    // the set of disjoint adjacent pairs that keeps the most intermediate-tensor elements out of HBM (a three-line dynamic programme over the run).
    // OAR_DSBLOCK_RS2_FIRST=1: greedy from the front instead.
    std::map<int, bool> dsblock_pair_plan;   // node index -> fuse with the next node
    void plan_dsblock_run(int first, const TInfo& x) {
        std::vector<k::DsBlockP> ps;
        std::vector<bool> link;
        int64_t N = x.dims[0], C = x.dims[1], H = x.dims[2], W = x.dims[3];
        for (int i = first; i < (int)E.nodes_.size(); ++i) {
            const GNode& q = E.nodes_[i];
            k::DsBlockP p;
            if (q.op != "DSBlock" || q.in.size() < 5 || !dsblock_shape(q, N, C, H, W, p)) break;
            ps.push_back(p);
            C = p.Cout; H = p.Ho; W = p.Wo;
            const bool ok = dsblock_link_ok(i);
            link.push_back(ok);
            if (!ok) break;
        }
        const int R = (int)ps.size();
        std::vector<double> w(std::max(R - 1, 0), -1.0);   // elements of the tensor between block j and j + 1 when that pair can fuse
        for (int j = 0; j + 1 < R; ++j)
            if (link[j] && k::dsblock2_eligible(ps[j], ps[j + 1])) w[j] = (double)N * ps[j].Cout * ps[j].Ho * ps[j].Wo;
        static const bool greedy_first = [] { const char* e = getenv("OAR_DSBLOCK_RS2_FIRST"); return e && atoi(e) != 0; }();
        std::vector<bool> take(std::max(R - 1, 0), false);
        if (greedy_first) {
            for (int j = 0; j + 1 < R; ++j) if (w[j] > 0) { take[j] = true; ++j; }
        } else {
            std::vector<double> best(R + 1, 0.0);   // best[j]: blocks j.. of the run
            for (int j = R - 2; j >= 0; --j) best[j] = std::max(best[j + 1], w[j] > 0 ? w[j] + best[std::min(j + 2, R)] : 0.0);
            for (int j = 0; j + 1 < R;) {
                if (w[j] > 0 && w[j] + best[std::min(j + 2, R)] >= best[j + 1]) { take[j] = true; j += 2; }
                else ++j;
            }
        }
        for (int j = 0; j < R; ++j) dsblock_pair_plan[first + j] = j + 1 < R && take[j];
    }
    bool try_dsblock_pair(const GNode& n, const TInfo& x) {
        if (cur + 1 >= (int)E.nodes_.size() || !n.residual.empty() || x.dims.size() != 4 || x.host_int) return false;
        if (!dsblock_pair_plan.count(cur)) plan_dsblock_run(cur, x);
        if (!dsblock_pair_plan[cur]) return false;
        const GNode& m = E.nodes_[cur + 1];
        k::DsBlockP pa, pb;
        const int64_t N = x.dims[0], C = x.dims[1], H = x.dims[2], W = x.dims[3];
        if (!dsblock_shape(n, N, C, H, W, pa) || !dsblock_shape(m, N, pa.Cout, pa.Ho, pa.Wo, pb) || !k::dsblock2_eligible(pa, pb)) return false;
        auto weights = [&](const GNode& d, k::DsBlockP& p) {
            const HostTensor &WD = *get(d.in[1]).ht, &WP = *get(d.in[3]).ht;
            GNode dwn, pwn;
            dwn.op = "Conv"; dwn.in = {d.in[0], d.in[1]};
            pwn.op = "Conv"; pwn.in = {d.out[0] + "::dw", d.in[3]};
            if (!d.in[2].empty()) OAR_CHECK((int64_t)get(d.in[2]).ht->f.size() == p.C, OAR_MODEL_LOAD, "DSBlock: depthwise bias size");
            if (!d.in[4].empty()) OAR_CHECK((int64_t)get(d.in[4]).ht->f.size() == p.Cout, OAR_MODEL_LOAD, "DSBlock: pointwise bias size");
            p.wd = conv_weight_dw(dwn, WD);
            p.bd = d.in[2].empty() ? nullptr : get(d.in[2]).loc.cptr;
            p.wp = conv_weight_igemm(pwn, WP, k::IGEMM_W_X6RS);
            p.bp = d.in[4].empty() ? nullptr : get(d.in[4]).loc.cptr;
        };
        weights(n, pa);
        weights(m, pb);
        Loc xin = to_clast_loc(x);
        TInfo& y = new_out(m.out[0], {N, (int64_t)pb.Cout, (int64_t)pb.Ho, (int64_t)pb.Wo}, Layout::CLAST);
        Loc yl = y.loc;
        const double px = (double)N * H * W;
        const double flops = 2.0 * px * (pa.C * (9.0 + pa.Cout) + pb.C * (9.0 + pb.Cout));
        const double bytes = 4.0 * px * (pa.C + pb.Cout);
        step([=](const RunCtx& c) {
            k::DsBlockP qa = pa, qb = pb;
            qa.x = c.at(xin); qb.y = c.mut(yl);
            k::dsblock2(c.s, qa, qb);
        }, flops, bytes);
        fused_into_prev.insert(cur + 1);
        return true;
    }

    void op_dsblock(const GNode& n) {
        TInfo x = get(n.in[0]);
        if (try_dsblock_pair(n, x)) return;
        const TInfo &wdt = get(n.in[1]), &wpt = get(n.in[3]);
        OAR_CHECK(wdt.ht && wpt.ht, OAR_UNSUPPORTED_OP, "DSBlock: weights must be initializers");
        const HostTensor &WD = *wdt.ht, &WP = *wpt.ht;
        // the two convolutions this node stands for (used when the fused kernel does not take the shape)
        GNode dwn, pwn;
        dwn.op = "Conv"; dwn.in = {n.in[0], n.in[1]}; if (!n.in[2].empty()) dwn.in.push_back(n.in[2]);
        dwn.out = {n.as("mid_name", n.out[0] + "::dw")}; dwn.attrs = n.attrs;
        dwn.act.kind = (int)n.ai("act1", 0); dwn.act.alpha = n.af("act1_alpha", 0.f); dwn.act.beta = n.af("act1_beta", 0.f);
        pwn.op = "Conv"; pwn.in = {dwn.out[0], n.in[3]}; if (!n.in[4].empty()) pwn.in.push_back(n.in[4]);
        pwn.out = n.out; pwn.act = n.act; pwn.residual = n.residual;
        Attr g1; g1.kind = Attr::I; g1.i = 1; pwn.attrs["group"] = g1;
        auto unfused = [&]() { op_conv(dwn); op_conv(pwn); };
        if (x.dims.size() != 4 || x.host_int) return unfused();
        const int64_t N = x.dims[0], C = x.dims[1], H = x.dims[2], W = x.dims[3], ks = WD.dims[2], Cout = WP.dims[0];
        OAR_CHECK(WD.dims[0] == C && WP.dims[1] == C, OAR_SHAPE_MISMATCH, "DSBlock: channel mismatch at " + n.out[0]);
        auto st = n.ais("strides");
        const int64_t sh = st.size() == 2 ? st[0] : 1, sw = st.size() == 2 ? st[1] : 1;
        int64_t pt, pl, pb, pr;
        get_pads(n, H, W, ks, ks, sh, sw, 1, 1, pt, pl, pb, pr);
        const int64_t Ho = (H + pt + pb - (ks - 1) - 1) / sh + 1, Wo = (W + pl + pr - (ks - 1) - 1) / sw + 1;
        k::DsBlockP p{};
        p.N = (int)N; p.H = (int)H; p.W = (int)W; p.C = (int)C; p.Ho = (int)Ho; p.Wo = (int)Wo; p.Cout = (int)Cout;
        p.ks = (int)ks; p.sh = (int)sh; p.sw = (int)sw; p.pt = (int)pt; p.pl = (int)pl;
        p.act1 = dwn.act; p.act2 = n.act; p.y_ld = (int)Cout;
        p.has_res = !n.residual.empty();
        Loc res;
        if (!n.residual.empty()) {
            TInfo r = get(n.residual);
            if (r.host_int || r.dims != std::vector<int64_t>{N, Cout, Ho, Wo}) return unfused();   // broadcasting add: op_conv splits it off
        }
        if (Ho <= 0 || Wo <= 0 || !k::dsblock_eligible(p)) return unfused();
        if (!n.residual.empty()) res = to_clast_loc(get(n.residual));
        Loc xin = to_clast_loc(x);
        if (!n.in[2].empty()) OAR_CHECK((int64_t)get(n.in[2]).ht->f.size() == C, OAR_MODEL_LOAD, "DSBlock: depthwise bias size");
        if (!n.in[4].empty()) OAR_CHECK((int64_t)get(n.in[4]).ht->f.size() == Cout, OAR_MODEL_LOAD, "DSBlock: pointwise bias size");
        p.wd = conv_weight_dw(dwn, WD);
        p.bd = n.in[2].empty() ? nullptr : get(n.in[2]).loc.cptr;
        const int wfmt = k::dsblock_wp_format(p);
        p.wp = wfmt == k::IGEMM_W_X6CS ? conv_weight_cs(dwn, pwn, WD, WP, n.in[2].empty() ? nullptr : &get(n.in[2]).ht->f, n.in[4].empty() ? nullptr : &get(n.in[4]).ht->f) : conv_weight_igemm(pwn, WP, wfmt);
        p.bp = n.in[4].empty() ? nullptr : get(n.in[4]).loc.cptr;
        TInfo& y = new_out(n.out[0], {N, Cout, Ho, Wo}, Layout::CLAST);
        Loc yl = y.loc;
        const bool has_res = res.kind != Loc::NONE;
        const double flops = 2.0 * N * Ho * Wo * C * (ks * ks + (double)Cout);
        const double bytes = 4.0 * (N * H * W * C + N * Ho * Wo * Cout * (has_res ? 2 : 1) + numel(WD.dims) + numel(WP.dims));
        step([=](const RunCtx& c) {
            k::DsBlockP q = p;
            q.x = c.at(xin); q.y = c.mut(yl); q.residual = has_res ? c.at(res) : nullptr;
            k::dsblock(c.s, q);
        }, flops, bytes);
    }

    // shape facts of a ConvTranspose node that decide whether it is the plain 2x2 / stride-2 kind
    bool convt_is_2x2s2(const GNode& n, int64_t& cin, int64_t& cout) {
        auto wi = E.inits_.find(n.in.size() > 1 ? n.in[1] : std::string());
        if (wi == E.inits_.end() || wi->second.dtype != DType::F32 || wi->second.dims.size() != 4) return false;
        const auto& d = wi->second.dims;
        auto st = n.ais("strides"), dl = n.ais("dilations"), pads = n.ais("pads"), op = n.ais("output_padding");
        const bool s2 = st.size() == 2 && st[0] == 2 && st[1] == 2;
        bool zero = true;
        for (auto v : pads) zero = zero && v == 0;
        for (auto v : op) zero = zero && v == 0;
        for (auto v : dl) zero = zero && v == 1;
        cin = d[0]; cout = d[1];
        return d[2] == 2 && d[3] == 2 && s2 && zero && n.ai("group", 1) == 1 && n.residual.empty();
    }
    void op_convt(const GNode& n, bool may_defer = true) {
        static const bool pair_on = [] { const char* e = getenv("OAR_FUSE_CONVT_PAIR"); return !e || atoi(e) != 0; }();
        // (a) this node's input is a held-back ConvTranspose: run the pair as one kernel
        if (pair_on && !n.in.empty() && pending_convt.count(n.in[0])) {
            const GNode& a = *pending_convt[n.in[0]];
            int64_t c0 = 0, c1 = 0, c1b = 0, c2 = 0;
            if (convt_is_2x2s2(a, c0, c1) && convt_is_2x2s2(n, c1b, c2) && c1 == c1b && k::convt2x2_pair_supported((int)c0, (int)c1, (int)c2)) {
                TInfo x = get(a.in[0]);
                if (x.dims.size() == 4 && x.dims[1] == c0 && x.layout == Layout::CLAST && !x.host_int) {
                    pending_convt.erase(n.in[0]);
                    vals.erase(n.in[0]);
                    const HostTensor& W1 = E.inits_.at(a.in[1]);
                    const HostTensor& W2 = E.inits_.at(n.in[1]);
                    auto pack = [&](const std::string& key, const HostTensor& W) {   // [Cin][Cout][2][2] -> [Cin][a * 2 + b][Cout]
                        auto it = E.dev_consts_.find(key);
                        if (it != E.dev_consts_.end()) return it->second;
                        const int64_t Ci = W.dims[0], Co = W.dims[1];
                        std::vector<float> w((size_t)Ci * 4 * Co);
                        for (int64_t ci = 0; ci < Ci; ++ci)
                            for (int64_t co = 0; co < Co; ++co)
                                for (int64_t q = 0; q < 4; ++q) w[(size_t)((ci * 4 + q) * Co + co)] = W.f[(size_t)((ci * Co + co) * 4 + q)];
                        return E.upload_const(key, w);
                    };
                    k::ConvT2Pair cp{};
                    cp.w1 = pack("convt_pair1:" + a.in[1], W1);
                    cp.w2 = pack("convt_pair2:" + n.in[1], W2);
                    cp.b1 = has_input(a, 2) ? get(a.in[2]).loc.cptr : nullptr;
                    cp.b2 = has_input(n, 2) ? get(n.in[2]).loc.cptr : nullptr;
                    cp.N = (int)x.dims[0]; cp.H = (int)x.dims[2]; cp.W = (int)x.dims[3]; cp.C0 = (int)c0; cp.C1 = (int)c1; cp.C2 = (int)c2;
                    cp.act1 = a.act; cp.act2 = n.act;
                    const Loc xin = x.loc;
                    TInfo& y = new_out(n.out[0], {x.dims[0], c2, x.dims[2] * 4, x.dims[3] * 4}, Layout::CLAST);
                    const Loc yl = y.loc;
                    const double px = (double)x.dims[0] * x.dims[2] * x.dims[3];
                    step([=](const RunCtx& c) { k::ConvT2Pair q = cp; q.x = c.at(xin); q.y = c.mut(yl); k::convt2x2_pair(c.s, q); },
                         2.0 * px * 4.0 * ((double)c0 * c1 + 4.0 * c1 * c2), 4.0 * px * (c0 + 16.0 * c2));
                    return;
                }
            }
        }
        // (b) this node may itself be held back for its consumer
        if (pair_on && may_defer && sole_consumer.count(n.out[0]) && E.nodes_[sole_consumer[n.out[0]]].op == "ConvTranspose") {
            int64_t c0 = 0, c1 = 0, c1b = 0, c2 = 0;
            const GNode& b = E.nodes_[sole_consumer[n.out[0]]];
            const bool feeds_first = !b.in.empty() && b.in[0] == n.out[0];
            auto xi = vals.find(n.in[0]);
            if (feeds_first && convt_is_2x2s2(n, c0, c1) && convt_is_2x2s2(b, c1b, c2) && c1 == c1b && k::convt2x2_pair_supported((int)c0, (int)c1, (int)c2) &&
                xi != vals.end() && !peek_pending(n.in[0]) && !pending_convt.count(n.in[0]) && xi->second.dims.size() == 4 && xi->second.layout == Layout::CLAST) {
                pending_convt[n.out[0]] = &n;
                TInfo t;   // known shape, no storage
                t.dims = {xi->second.dims[0], c1, xi->second.dims[2] * 2, xi->second.dims[3] * 2};
                t.layout = Layout::CLAST; t.root = "";
                vals[n.out[0]] = t;
                return;
            }
        }
        TInfo x = get(n.in[0]);
        OAR_CHECK(x.dims.size() == 4, OAR_UNSUPPORTED_OP, "ConvTranspose: only 2-D");
        const TInfo& wt = get(n.in[1]);
        OAR_CHECK(wt.ht, OAR_UNSUPPORTED_OP, "ConvTranspose: weights must be an initializer");
        const HostTensor& W0 = *wt.ht;
        OAR_CHECK(W0.dims.size() == 4 && W0.dims[0] == x.dims[1] && W0.dims[1] > 0 && W0.dims[2] > 0 && W0.dims[3] > 0, OAR_MODEL_LOAD, "ConvTranspose: weight must be [Cin, Cout / group, kh, kw] at " + n.out[0]);
        const int64_t grp = n.ai("group", 1);
        OAR_CHECK(grp >= 1 && x.dims[1] % grp == 0, OAR_SHAPE_MISMATCH, "ConvTranspose: group must divide Cin at " + n.out[0]);
        // group > 1 (round 6; no PP-OCR graph has one): the weights as the block-diagonal [Cin, group * Cout / group, kh, kw] tensor of the equivalent dense layer
        HostTensor Wg;
        if (grp > 1) {
            const int64_t cig = W0.dims[0] / grp, cog = W0.dims[1], kk = W0.dims[2] * W0.dims[3];
            Wg.dtype = W0.dtype; Wg.dims = {W0.dims[0], grp * cog, W0.dims[2], W0.dims[3]};
            Wg.f.assign((size_t)(W0.dims[0] * grp * cog * kk), 0.f);
            for (int64_t ci = 0; ci < W0.dims[0]; ++ci)
                for (int64_t co = 0; co < cog; ++co)
                    for (int64_t t = 0; t < kk; ++t) Wg.f[(size_t)((ci * grp * cog + (ci / cig) * cog + co) * kk + t)] = W0.f[(size_t)((ci * cog + co) * kk + t)];
        }
        const HostTensor& W = grp > 1 ? Wg : W0;
        if (has_input(n, 2)) { const TInfo& bt = get(n.in[2]); OAR_CHECK(bt.ht && (int64_t)bt.ht->f.size() == W.dims[1], OAR_MODEL_LOAD, "ConvTranspose: bias must be an f32 initializer of Cout elements at " + n.out[0]); }
        int64_t N = x.dims[0], Cin = x.dims[1], H = x.dims[2], Wd = x.dims[3];
        int64_t Cout = W.dims[1], kh = W.dims[2], kw = W.dims[3];
        auto st = n.ais("strides"), dl = n.ais("dilations"), pads = n.ais("pads"), op = n.ais("output_padding");
        int64_t sh = st.size() == 2 ? st[0] : 1, sw = st.size() == 2 ? st[1] : 1;
        int64_t dh = dl.size() == 2 ? dl[0] : 1, dw = dl.size() == 2 ? dl[1] : 1;
        int64_t pt = pads.size() == 4 ? pads[0] : 0, pl = pads.size() == 4 ? pads[1] : 0, pb = pads.size() == 4 ? pads[2] : 0, pr = pads.size() == 4 ? pads[3] : 0;
        int64_t oph = op.size() == 2 ? op[0] : 0, opw = op.size() == 2 ? op[1] : 0;
        int64_t Ho = (H - 1) * sh - pt - pb + dh * (kh - 1) + oph + 1, Wo = (Wd - 1) * sw - pl - pr + dw * (kw - 1) + opw + 1;
        Loc xin = to_clast_loc(x);
        const float* bias = has_input(n, 2) ? get(n.in[2]).loc.cptr : nullptr;
        TInfo& y = new_out(n.out[0], {N, Cout, Ho, Wo}, Layout::CLAST);
        bool fast = kh == 2 && kw == 2 && sh == 2 && sw == 2 && pt == 0 && pl == 0 && pb == 0 && pr == 0 && oph == 0 && opw == 0 && Cin % 4 == 0 && dh == 1 && dw == 1;
        k::ConvP p{};
        p.N = (int)N; p.H = (int)H; p.W = (int)Wd; p.Cin = (int)Cin; p.Ho = (int)Ho; p.Wo = (int)Wo; p.Cout = (int)Cout;
        p.kh = (int)kh; p.kw = (int)kw; p.sh = (int)sh; p.sw = (int)sw; p.pt = (int)pt; p.pl = (int)pl; p.dh = (int)dh; p.dw = (int)dw;
        p.groups = 1; p.act = n.act; p.bias = bias; p.y_ld = (int)Cout; p.convt2x2 = fast ? 1 : 0;
        p.w_fmt = 0;   // the 2x2 scatter epilogue runs on the f32 kernels
        p.w = convt_weight(n, W, fast, p.w_fmt);
        Loc yl = y.loc;
        double flops = 2.0 * N * H * Wd * Cin * Cout * kh * kw;
        double bytes = 4.0 * (N * H * Wd * Cin + N * Ho * Wo * Cout + numel(W.dims));
        step([=](const RunCtx& c) {
            k::ConvP q = p;
            q.x = c.at(xin); q.y = c.mut(yl);
            if (fast) k::conv_igemm(c.s, q); else k::convt_direct(c.s, q);
        }, flops, bytes);
    }

    void op_bn(const GNode& n) {  // leftover BN: per-channel affine as a 1x1 depthwise conv
        TInfo x = get(n.in[0]);
        OAR_CHECK(x.dims.size() == 4, OAR_UNSUPPORTED_OP, "BatchNormalization: rank-4 only");
        const auto &ga = get(n.in[1]), &be = get(n.in[2]), &mu = get(n.in[3]), &va = get(n.in[4]);
        OAR_CHECK(ga.ht && be.ht && mu.ht && va.ht, OAR_UNSUPPORTED_OP, "BatchNormalization: params must be initializers");
        int64_t C = x.dims[1];
        OAR_CHECK((int64_t)ga.ht->f.size() == C && (int64_t)be.ht->f.size() == C && (int64_t)mu.ht->f.size() == C && (int64_t)va.ht->f.size() == C, OAR_MODEL_LOAD,
                  "BatchNormalization: scale / bias / mean / var must all have C elements (" + n.out[0] + ")");
        float eps = n.af("epsilon", 1e-5f);
        std::vector<float> sc(C), sh(C);
        for (int64_t c = 0; c < C; ++c) { sc[c] = ga.ht->f[c] / std::sqrt(va.ht->f[c] + eps); sh[c] = be.ht->f[c] - mu.ht->f[c] * sc[c]; }
        const float* dsc = E.upload_const("bn_sc:" + n.out[0], sc);
        const float* dsh = E.upload_const("bn_sh:" + n.out[0], sh);
        Loc xin = to_clast_loc(x);
        TInfo& y = new_out(n.out[0], x.dims, Layout::CLAST);
        k::ConvP p{};
        p.N = (int)x.dims[0]; p.H = p.Ho = (int)x.dims[2]; p.W = p.Wo = (int)x.dims[3]; p.Cin = p.Cout = (int)C;
        p.kh = p.kw = p.sh = p.sw = p.dh = p.dw = 1; p.groups = (int)C; p.act = n.act; p.w = dsc; p.bias = dsh; p.y_ld = (int)C;
        Loc yl = y.loc;
        bool dwok = C % 4 == 0;
        step([=](const RunCtx& c) {
            k::ConvP q = p; q.x = c.at(xin); q.y = c.mut(yl);
            if (dwok) k::conv_dw(c.s, q); else k::conv_direct(c.s, q);
        }, 0, 8.0 * numel(x.dims));
    }

    void op_unary(const GNode& n, Act a) {
        TInfo x = get(n.in[0]);
        TInfo& y = new_out(n.out[0], x.dims, x.layout);
        y.is01 = a.kind == k::ACT_NOT;
        Loc xl = x.loc, yl = y.loc;
        int64_t cnt = numel(x.dims);
        step([=](const RunCtx& c) { k::unary(c.s, c.at(xl), c.mut(yl), cnt, a); }, 0, 8.0 * cnt);
    }

    // host permutation of a constant to channels-last physical order
    const float* const_clast(const std::string& name, const HostTensor& t, const std::vector<int64_t>& dims_aligned) {
        std::string key = "clast:" + name + ":" + std::to_string(dims_aligned.size());
        auto it = E.dev_consts_.find(key);
        if (it != E.dev_consts_.end()) return it->second;
        int r = (int)dims_aligned.size();
        std::vector<int64_t> pd = clast_phys_dims(dims_aligned), ns = contig_strides(dims_aligned), is(r);
        is[0] = ns[0];
        for (int i = 2; i < r; ++i) is[i - 1] = ns[i];
        is[r - 1] = ns[1];
        int64_t total = numel(pd);
        std::vector<float> out((size_t)total);
        std::vector<int64_t> idx(r, 0);
        for (int64_t i = 0; i < total; ++i) {
            int64_t rem = i, off = 0;
            for (int d = r - 1; d >= 0; --d) { int64_t q = rem / pd[d]; off += (rem - q * pd[d]) * is[d]; rem = q; }
            out[i] = t.f[off];
        }
        return E.upload_const(key, out);
    }

    void op_binary(const GNode& n, int op) {
        // a + upsample(b) (FPN top-down path): the sum reads b at (oh / f, ow / f) -- no upsampled tensor
        if (op == 0 && !pending_resize.empty() && n.act.kind == k::ACT_NONE) {
            for (int side = 0; side < 2; ++side) {
                const PendingResize* pr = peek_pending(n.in[side]);
                if (!pr || peek_pending(n.in[1 - side]) || !pr->fh || (pr->C & 3)) continue;
                const TInfo& o = get(n.in[1 - side]);
                if (o.host_int || o.ht || o.layout != Layout::CLAST || o.dims != pr->dims) continue;
                const PendingResize r = *pr;
                pending_resize.erase(n.in[side]);
                Loc al = o.loc;
                TInfo& y = new_out(n.out[0], r.dims, Layout::CLAST);
                Loc yl = y.loc;
                const double cnt = (double)numel(r.dims);
                step([=](const RunCtx& c) { k::binary_upsampled(c.s, c.at(al), c.at(r.xin), c.mut(yl), r.N, r.Ho, r.Wo, r.C, r.fh, r.fw, 0); }, cnt,
                     4.0 * (2.0 * cnt + cnt / (r.fh * r.fw)));
                return;
            }
        }
        TInfo a = get(n.in[0]), b = get(n.in[1]);
        const bool ints_in = (a.host_int ? !a.host_f : a.is_int) && (b.host_int ? !b.host_f : b.is_int);
        const bool f32_native = !a.host_int && !b.host_int && !a.is_int && !b.is_int && a.layout == Layout::NATIVE && b.layout == Layout::NATIVE;
        // a plan-time value meeting a device tensor (e.g. a scale computed from Shape): materialise it as an f32 constant
        if (a.host_int) { a.loc = host_to_device(n.in[0], a); a.host_int = false; a.layout = Layout::NATIVE; }
        if (b.host_int) { b.loc = host_to_device(n.in[1], b); b.host_int = false; b.layout = Layout::NATIVE; }
        int r = (int)std::max(a.dims.size(), b.dims.size());
        auto align = [&](const std::vector<int64_t>& d) { std::vector<int64_t> o(r - d.size(), 1); o.insert(o.end(), d.begin(), d.end()); return o; };
        std::vector<int64_t> ad = align(a.dims), bd = align(b.dims), od(r);
        for (int i = 0; i < r; ++i) {
            OAR_CHECK(ad[i] == bd[i] || ad[i] == 1 || bd[i] == 1, OAR_SHAPE_MISMATCH, "binary: shapes do not broadcast at " + n.out[0]);
            od[i] = std::max(ad[i], bd[i]);
        }
        bool clast = (a.layout == Layout::CLAST && (int)a.dims.size() == r) || (b.layout == Layout::CLAST && (int)b.dims.size() == r);
        Loc al = a.loc, bl = b.loc;
        std::vector<int64_t> pad, pbd, pod;  // physical dims
        if (clast) {
            auto fix = [&](TInfo& t, const std::vector<int64_t>& d, const std::string& nm, Loc& l) {
                if (t.layout == Layout::CLAST && (int)t.dims.size() == r) return;
                // count non-1 dims: with <= 1 the memory order is unaffected by the permutation
                int non1 = 0;
                for (auto v : d) if (v != 1) ++non1;
                if (non1 <= 1) return;
                if (t.ht) { l.kind = Loc::CONST; l.cptr = const_clast(nm, *t.ht, d); return; }
                TInfo tmp = t; tmp.dims = d; tmp.layout = Layout::NATIVE;
                l = to_clast_loc(tmp);
            };
            fix(a, ad, n.in[0], al);
            fix(b, bd, n.in[1], bl);
            pad = clast_phys_dims(ad); pbd = clast_phys_dims(bd); pod = clast_phys_dims(od);
        } else {
            if (a.layout == Layout::CLAST) { al = to_native_loc(a); }
            if (b.layout == Layout::CLAST) { bl = to_native_loc(b); }
            pad = ad; pbd = bd; pod = od;
        }
        auto bstr = [&](const std::vector<int64_t>& d) {
            std::vector<int64_t> s = contig_strides(d);
            for (size_t i = 0; i < d.size(); ++i) if (d[i] == 1) s[i] = 0;
            return s;
        };
        std::vector<int64_t> sa = bstr(pad), sb = bstr(pbd);
        // commutative ops: put the full-size operand first (fast paths key on `a`)
        bool commut = op == 0 || op == 2 || op == 6 || op == 7 || op == 8 || op == 11 || op == 12;
        if (commut && numel(pad) < numel(pbd)) { std::swap(al, bl); std::swap(sa, sb); }
        TInfo& y = new_out(n.out[0], od, clast ? Layout::CLAST : Layout::NATIVE);
        y.is_int = ints_in && (op == 0 || op == 1 || op == 2 || op == 6 || op == 7) && n.act.kind == k::ACT_NONE;   // index arithmetic (idx + offset, idx - dim) stays an index tensor
        y.is01 = op >= 8 && op <= 12 && n.act.kind == k::ACT_NONE;   // Equal / Less / Greater / And / Or write 0.0f or 1.0f
        Loc yl = y.loc;
        Act post = n.act;
        int64_t cnt = numel(od);
        step([=](const RunCtx& c) { k::binary(c.s, c.at(al), c.at(bl), c.mut(yl), op, r, pod.data(), sa.data(), sb.data(), post); }, (double)cnt, 12.0 * cnt);
        // a plain Add of two f32 device tensors in NATIVE layout, the second one the same shape or [1, .., 1, d_k, .., C] (its rows repeat with period b_rows):
        // what k::add_layernorm can take over when a marked LayerNormalization is the next step (op_layernorm, fuse_chains)
        last_add = AddRec();
        if (op == 0 && E.fuse_add_ln_ && post.kind == k::ACT_NONE && f32_native && !clast && r >= 1 && od[(size_t)r - 1] > 0) {
            const bool swapped = numel(ad) < numel(bd);
            const std::vector<int64_t>& full = swapped ? bd : ad;
            const std::vector<int64_t>& part = swapped ? ad : bd;
            int lead = 0;
            while (lead < r - 1 && part[(size_t)lead] == 1) ++lead;
            bool ok = full == od;
            for (int i = lead; i < r; ++i) ok = ok && part[(size_t)i] == od[(size_t)i];
            // (an operand that starts off a 16-byte boundary -- a view into a larger tensor -- would put the fused launch on its one-wave form where the pair's
            // LayerNorm, reading the aligned sum, takes the half-wave form: within tolerance of each other but not the same bits.  Such a pair stays a pair.)
            if (ok && loc_on_16(al) && loc_on_16(bl)) {
                last_add.node = cur; last_add.step = (int)P.steps.size() - 1; last_add.out = n.out[0]; last_add.a = al; last_add.b = bl; last_add.sum = yl;
                last_add.C = od[(size_t)r - 1]; last_add.rows = cnt / last_add.C; last_add.b_rows = numel(part) / last_add.C;
            }
        }
    }
    // the newest plain Add (see op_binary) and the Add + LayerNormalization pairs that fuse_chains turns into one launch
    // provably on a 16-byte boundary at run time: the arena and the graph inputs are device allocations, so the byte offset decides
    static bool loc_on_16(const Loc& l) { return l.kind == Loc::CONST ? (reinterpret_cast<uintptr_t>(l.cptr) & 15) == 0 : l.kind != Loc::NONE && (l.off & 15) == 0; }
    struct AddRec { int node = -2, step = -1; std::string out; Loc a, b, sum; int64_t rows = 0, C = 0, b_rows = 0; std::function<void(const RunCtx&)> lin; };
    AddRec last_add;
    struct AddLnRec { std::function<void(const RunCtx&)> run, lin; double bytes_saved = 0; std::string label; };   // lin: the step in front is a Linear; this is it without its residual
    std::map<int, AddLnRec> add_ln_at;   // by the step index of the LayerNorm; its Add is the step in front of it

    // ReduceMean / ReduceSum / ReduceMax / ReduceMin / ReduceProd over the trailing axes (decomposed LayerNorm / softmax
    // exports), or ReduceMean over the spatial axes of an NCHW tensor (= GlobalAveragePool).  mode: k::reduce_lastdim's.
    void op_reduce(const GNode& n, int mode) {
        TInfo x = get(n.in[0]);
        const int r = (int)x.dims.size();
        std::vector<int64_t> axes = has_input(n, 1) ? get(n.in[1]).hv : n.ais("axes");
        if (axes.empty() && n.ai("noop_with_empty_axes", 0) == 0) for (int i = 0; i < r; ++i) axes.push_back(i);
        for (auto& a : axes) if (a < 0) a += r;
        std::sort(axes.begin(), axes.end());
        const bool keep = n.ai("keepdims", 1) != 0;
        bool spatial = mode == 0 && r == 4 && axes.size() == 2 && axes[0] == 2 && axes[1] == 3;
        if (spatial) {
            if (keep) return op_gap(n);
            GNode gp = n;   // keepdims = 0: the pooled [N, C, 1, 1] map, squeezed
            gp.out = {n.out[0] + "::kept"};
            op_gap(gp);
            GNode sq;
            sq.op = "Squeeze"; sq.in = {gp.out[0]}; sq.out = {n.out[0]};
            Attr ax; ax.kind = Attr::IS; ax.is = {2, 3}; sq.attrs["axes"] = ax;
            op_squeeze(sq);
            adopt_root(n.out[0], gp.out[0]);
            return;
        }
        bool trailing = !axes.empty();
        for (size_t i = 0; i < axes.size(); ++i) trailing = trailing && axes[i] == r - (int64_t)axes.size() + (int64_t)i;
        if (!trailing && (mode == 0 || mode == 2) && r == 4 && axes.size() == 1 && (axes[0] == 2 || axes[0] == 3) && !x.host_int) {
            // mean / max over ONE spatial axis of a feature map (SVTRv2's `x.mean(2)` in front of its CTC head): a pooling window as tall (wide)
            // as the map, on the channels-last tensor where it lies; keepdims = 0 is then a Squeeze of a channels-last view
            GNode pl;
            pl.op = mode == 0 ? "AveragePool" : "MaxPool"; pl.in = {n.in[0]}; pl.out = {keep ? n.out[0] : n.out[0] + "::kept"};
            Attr ks; ks.kind = Attr::IS; ks.is = axes[0] == 2 ? std::vector<int64_t>{x.dims[2], 1} : std::vector<int64_t>{1, x.dims[3]};
            pl.attrs["kernel_shape"] = ks; pl.attrs["strides"] = ks;
            op_pool(pl, mode == 2);
            if (!keep) {
                GNode sq;
                sq.op = "Squeeze"; sq.in = {pl.out[0]}; sq.out = {n.out[0]};
                Attr ax; ax.kind = Attr::IS; ax.is = {axes[0]}; sq.attrs["axes"] = ax;
                op_squeeze(sq);
                adopt_root(n.out[0], pl.out[0]);
            }
            return;
        }
        if (!trailing && !axes.empty() && !x.host_int) {
            // any other axis set (round 6; no PP-OCR graph has one -- tools/op_fuzz.py asked): the reduced axes are moved behind the others by a Transpose, reduced as
            // trailing axes, and keepdims = 1 is a view of the result with the ones back in place
            std::vector<int64_t> perm, od;
            for (int i = 0; i < r; ++i) if (!std::binary_search(axes.begin(), axes.end(), (int64_t)i)) perm.push_back(i);
            for (auto a : axes) perm.push_back(a);
            for (int i = 0; i < r; ++i) { if (!std::binary_search(axes.begin(), axes.end(), (int64_t)i)) od.push_back(x.dims[i]); else if (keep) od.push_back(1); }
            GNode tr;
            tr.op = "Transpose"; tr.in = {n.in[0]}; tr.out = {n.out[0] + "::moved"};
            Attr pa; pa.kind = Attr::IS; pa.is = perm; tr.attrs["perm"] = pa;
            op_transpose(tr);
            GNode rd = n;
            rd.in = {tr.out[0]}; rd.out = {keep ? n.out[0] + "::reduced" : n.out[0]};
            std::vector<int64_t> tail;
            for (size_t i = 0; i < axes.size(); ++i) tail.push_back(r - (int64_t)axes.size() + (int64_t)i);
            Attr ta; ta.kind = Attr::IS; ta.is = tail; rd.attrs["axes"] = ta;
            Attr kd; kd.kind = Attr::I; kd.i = 0; rd.attrs["keepdims"] = kd;
            op_reduce(rd, mode);
            if (keep) { GNode v; v.op = "Reshape"; v.in = {rd.out[0]}; v.out = {n.out[0]}; view_native(v, get(rd.out[0]), od); adopt_root(n.out[0], rd.out[0]); }
            return;
        }
        OAR_CHECK(trailing, OAR_UNSUPPORTED_OP, n.op + ": only the trailing axes (or H, W / one of them for ReduceMean / ReduceMax of an NCHW tensor) are supported");
        Loc xin = to_native_loc(x);
        int64_t C = 1;
        for (auto a : axes) C *= x.dims[a];
        const int64_t rows = numel(x.dims) / std::max<int64_t>(C, 1);
        std::vector<int64_t> od(x.dims.begin(), x.dims.end() - (int64_t)axes.size());
        if (keep) for (size_t i = 0; i < axes.size(); ++i) od.push_back(1);
        TInfo& y = new_out(n.out[0], od, Layout::NATIVE);
        Loc yl = y.loc;
        step([=](const RunCtx& c) { k::reduce_lastdim(c.s, c.at(xin), c.mut(yl), rows, (int)C, mode); }, (double)rows * C, 4.0 * rows * (C + 1));
    }

    // ArgMax / ArgMin over the last axis
    void op_argreduce(const GNode& n, bool is_min) {
        TInfo x = get(n.in[0]);
        const int r = (int)x.dims.size();
        int64_t axis = n.ai("axis", 0);
        if (axis < 0) axis += r;
        OAR_CHECK(r >= 1 && axis == r - 1, OAR_UNSUPPORTED_OP, n.op + ": only the last axis is supported");
        Loc xin = to_native_loc(x);
        const int64_t C = x.dims[axis], rows = numel(x.dims) / std::max<int64_t>(C, 1);
        OAR_CHECK(C >= 1 && C < (1 << 24), OAR_UNSUPPORTED_OP, n.op + ": axis length must be in [1, 2^24)");
        std::vector<int64_t> od(x.dims.begin(), x.dims.end() - 1);
        if (n.ai("keepdims", 1) != 0) od.push_back(1);
        const bool last = n.ai("select_last_index", 0) != 0;
        TInfo& y = new_out(n.out[0], od, Layout::NATIVE);
        y.is_int = true;
        Loc yl = y.loc;
        step([=](const RunCtx& c) { k::argreduce_lastdim(c.s, c.at(xin), c.mut(yl), rows, (int)C, is_min, last); }, (double)rows * C, 4.0 * rows * (C + 1));
    }

    // ------------------------------------------------------------------ broadcast copies (Expand / Tile)
    // y (contiguous, dims od) = x read through `in_strides` (0 = broadcast); dims of size 1 are dropped and neighbours that
    // are contiguous in x are merged so that real-world ranks fit the 6-d permute kernel
    void strided_copy(const std::string& out, Loc xin, std::vector<int64_t> od_full, std::vector<int64_t> vd, std::vector<int64_t> vs, bool is_int = false) {
        std::vector<int64_t> d, st;
        for (size_t i = 0; i < vd.size(); ++i) {
            if (vd[i] == 1) continue;
            if (!d.empty() && st.back() == vs[i] * vd[i] && vs[i] != 0) { d.back() *= vd[i]; st.back() = vs[i]; }
            else if (!d.empty() && st.back() == 0 && vs[i] == 0) d.back() *= vd[i];
            else { d.push_back(vd[i]); st.push_back(vs[i]); }
        }
        if (d.empty()) { d.push_back(1); st.push_back(0); }
        OAR_CHECK(d.size() <= 6, OAR_UNSUPPORTED_OP, "Expand / Tile: more than 6 effective dimensions at " + out);
        TInfo& y = new_out(out, od_full, Layout::NATIVE);
        y.is_int = is_int;
        Loc yl = y.loc;
        const int r = (int)d.size();
        step([=](const RunCtx& c) { k::permute(c.s, c.at(xin), c.mut(yl), r, d.data(), st.data()); }, 0, 8.0 * numel(od_full));
    }
    void op_expand(const GNode& n) {
        TInfo x = get(n.in[0]);
        const TInfo& sh = get(n.in[1]);
        OAR_CHECK(sh.host_int, OAR_UNSUPPORTED_OP, "Expand: shape must be known on the host");
        const int r = (int)std::max(x.dims.size(), sh.hv.size());
        std::vector<int64_t> xd(r - x.dims.size(), 1), td(r - sh.hv.size(), 1), od(r);
        xd.insert(xd.end(), x.dims.begin(), x.dims.end());
        td.insert(td.end(), sh.hv.begin(), sh.hv.end());
        for (int i = 0; i < r; ++i) {
            OAR_CHECK(xd[i] == td[i] || xd[i] == 1 || td[i] == 1, OAR_SHAPE_MISMATCH, "Expand: shapes do not broadcast at " + n.out[0]);
            od[i] = std::max(xd[i], td[i]);
        }
        Loc xin = to_native_loc(x);
        std::vector<int64_t> st = contig_strides(xd);
        for (int i = 0; i < r; ++i) if (xd[i] == 1) st[i] = 0;
        strided_copy(n.out[0], xin, od, od, st, x.is_int);
    }
    void op_tile(const GNode& n) {
        TInfo x = get(n.in[0]);
        const TInfo& rp = get(n.in[1]);
        OAR_CHECK(rp.host_int && rp.hv.size() == x.dims.size(), OAR_UNSUPPORTED_OP, "Tile: repeats must be host ints, one per axis");
        Loc xin = to_native_loc(x);
        std::vector<int64_t> xs = contig_strides(x.dims), od, vd, vs;
        for (size_t i = 0; i < x.dims.size(); ++i) {
            OAR_CHECK(rp.hv[i] >= 1, OAR_INVALID_INPUT, "Tile: repeats must be >= 1");
            od.push_back(x.dims[i] * rp.hv[i]);
            vd.push_back(rp.hv[i]); vs.push_back(0);          // [repeat][extent] with stride [0][s]
            vd.push_back(x.dims[i]); vs.push_back(xs[i]);
        }
        strided_copy(n.out[0], xin, od, vd, vs, x.is_int);
    }
    void op_constant_of_shape(const GNode& n) {
        const TInfo& sh = get(n.in[0]);
        OAR_CHECK(sh.host_int, OAR_UNSUPPORTED_OP, "ConstantOfShape: shape must be known on the host");
        double v = 0.0; bool is_f = true;
        auto it = n.attrs.find("value");
        if (it != n.attrs.end() && it->second.kind == Attr::T) {
            const HostTensor& t = it->second.t;
            if (t.dtype == DType::F32) v = t.f.empty() ? 0.0 : t.f[0];
            else { v = t.i.empty() ? 0.0 : (double)t.i[0]; is_f = false; }
        }
        for (auto d : sh.hv) OAR_CHECK(d >= 0 && d <= (int64_t)1 << 28, OAR_SHAPE_MISMATCH, "ConstantOfShape: negative or unreasonable dimension");   // (two negative dims would multiply to a plausible count)
        const int64_t cnt = numel(sh.hv);
        OAR_CHECK(cnt >= 0 && cnt <= (int64_t)1 << 28, OAR_SHAPE_MISMATCH, "ConstantOfShape: unreasonable element count");
        if (!is_f || cnt <= 64) {   // shape plumbing stays on the host
            TInfo o; o.host_int = true; o.dims = sh.hv; o.host_f = is_f;
            o.hv.assign((size_t)cnt, (int64_t)v); o.hd.assign((size_t)cnt, v);
            vals[n.out[0]] = o; return;
        }
        TInfo t;
        t.dims = sh.hv; t.layout = Layout::NATIVE; t.loc.kind = Loc::CONST;
        t.loc.cptr = E.upload_const("cos:" + std::to_string(v) + ":" + std::to_string(cnt), std::vector<float>((size_t)cnt, (float)v));
        vals[n.out[0]] = t;
    }
    // device value of a host-known tensor (a bool / int mask or scalar that a device op consumes)
    Loc host_to_device(const std::string& name, const TInfo& t) {
        OAR_CHECK(!t.hv.empty() && (int64_t)t.hv.size() == numel(t.dims), OAR_UNSUPPORTED_OP, "an empty plan-time value feeds a device operator (node " + node_label() + ")");
        std::vector<float> f(t.hv.size());
        for (size_t i = 0; i < f.size(); ++i) f[i] = t.host_f && i < t.hd.size() ? (float)t.hd[i] : (float)t.hv[i];
        std::string key = "hostval:" + name + ":";
        for (float v : f) key += std::to_string(v) + ",";
        Loc l; l.kind = Loc::CONST; l.cptr = E.upload_const(key, f);
        return l;
    }
    void op_where(const GNode& n) {
        TInfo c = get(n.in[0]), a = get(n.in[1]), b = get(n.in[2]);
        auto dev = [&](const std::string& nm, TInfo& t) -> Loc { return t.host_int ? host_to_device(nm, t) : to_native_loc(t); };
        Loc cl, al = dev(n.in[1], a), bl = dev(n.in[2], b);
        if (c.host_int) cl = host_to_device(n.in[0], c);
        else if (c.ht == nullptr && c.loc.kind != Loc::NONE) cl = to_native_loc(c);
        else cl = c.loc;   // a bool initializer arrives as host ints (handled above); f32 0/1 masks as constants
        const int r = (int)std::max({c.dims.size(), a.dims.size(), b.dims.size()});
        OAR_CHECK(r <= 6, OAR_UNSUPPORTED_OP, "Where: rank > 6");
        auto align = [&](const std::vector<int64_t>& d) { std::vector<int64_t> o(r - d.size(), 1); o.insert(o.end(), d.begin(), d.end()); return o; };
        std::vector<int64_t> cd = align(c.dims), ad = align(a.dims), bd = align(b.dims), od(r);
        for (int i = 0; i < r; ++i) {
            od[i] = std::max({cd[i], ad[i], bd[i]});
            OAR_CHECK((cd[i] == od[i] || cd[i] == 1) && (ad[i] == od[i] || ad[i] == 1) && (bd[i] == od[i] || bd[i] == 1), OAR_SHAPE_MISMATCH, "Where: shapes do not broadcast at " + n.out[0]);
        }
        auto bstr = [&](const std::vector<int64_t>& d) { std::vector<int64_t> st = contig_strides(d); for (size_t i = 0; i < d.size(); ++i) if (d[i] == 1) st[i] = 0; return st; };
        std::vector<int64_t> sc = bstr(cd), sa = bstr(ad), sb = bstr(bd);
        TInfo& y = new_out(n.out[0], od, Layout::NATIVE);
        Loc yl = y.loc;
        step([=](const RunCtx& cx) { k::where(cx.s, cx.at(cl), cx.at(al), cx.at(bl), cx.mut(yl), r, od.data(), sc.data(), sa.data(), sb.data()); }, 0, 16.0 * numel(od));
    }

    // ------------------------------------------------------------------ host evaluation (shape arithmetic)
    // Paddle2ONNX / torch exports compute Reshape / Resize / Slice arguments with little integer (and sometimes float)
    // graphs hanging off Shape nodes.  Every value reachable from Shape + constants only is evaluated here, at plan time,
    // with numpy broadcasting; nothing of it is ever launched.
    static std::vector<double> host_values(const TInfo& t) {
        std::vector<double> v;
        if (t.host_int) {
            if (t.host_f && t.hd.size() == t.hv.size()) return t.hd;
            v.assign(t.hv.begin(), t.hv.end());
        } else if (t.ht) {
            v.assign(t.ht->f.begin(), t.ht->f.end());
        }
        return v;
    }
    bool host_evaluable(const TInfo& t) const { return t.host_int || (t.ht && t.ht->f.size() <= 64); }
    void set_host(const std::string& name, const std::vector<int64_t>& dims, const std::vector<double>& v, bool is_float) {
        TInfo o;
        o.host_int = true; o.host_f = is_float; o.dims = dims; o.hd = v;
        o.hv.resize(v.size());
        for (size_t i = 0; i < v.size(); ++i) o.hv[i] = (int64_t)v[i];   // truncation toward zero, like Cast
        vals[name] = o;
    }
    static bool float_like(const TInfo& t) { return t.host_int ? t.host_f : t.ht != nullptr; }
    // returns true when the node was evaluated on the host
    bool op_host(const GNode& n) {
        const std::string& op = n.op;
        std::vector<TInfo> in;
        for (auto& sname : n.in) in.push_back(sname.empty() ? TInfo() : get(sname));
        auto bin = [&](int code) {
            const TInfo &a = in[0], &b = in[1];
            std::vector<double> av = host_values(a), bv = host_values(b);
            const int r = (int)std::max(a.dims.size(), b.dims.size());
            std::vector<int64_t> ad(r - a.dims.size(), 1), bd(r - b.dims.size(), 1), od(r);
            ad.insert(ad.end(), a.dims.begin(), a.dims.end());
            bd.insert(bd.end(), b.dims.begin(), b.dims.end());
            for (int i = 0; i < r; ++i) {
                OAR_CHECK(ad[i] == bd[i] || ad[i] == 1 || bd[i] == 1, OAR_SHAPE_MISMATCH, "host " + op + ": shapes do not broadcast at " + n.out[0]);
                od[i] = std::max(ad[i], bd[i]);
            }
            std::vector<int64_t> sa = contig_strides(ad), sb = contig_strides(bd);
            const bool fl = (float_like(a) || float_like(b)) && code <= 6;
            std::vector<double> out((size_t)numel(od));
            for (int64_t i = 0; i < (int64_t)out.size(); ++i) {
                int64_t rem = i, oa = 0, ob = 0;
                for (int d = r - 1; d >= 0; --d) { const int64_t q = rem / od[d], ix = rem - q * od[d]; rem = q; oa += (ad[d] == 1 ? 0 : ix) * sa[d]; ob += (bd[d] == 1 ? 0 : ix) * sb[d]; }
                const double x = av[(size_t)oa], y = bv[(size_t)ob];
                double v = 0;
                switch (code) {
                    case 0: v = x + y; break;
                    case 1: v = x - y; break;
                    case 2: v = x * y; break;
                    case 3: v = fl ? x / y : (y != 0 ? (double)((int64_t)x / (int64_t)y) : 0.0); break;   // integer Div truncates
                    case 4: v = std::pow(x, y); break;
                    case 5: v = std::max(x, y); break;
                    case 6: v = std::min(x, y); break;
                    case 7: v = x == y; break;
                    case 8: v = x < y; break;
                    case 9: v = x > y; break;
                    case 10: v = (x != 0) && (y != 0); break;
                    default: v = (x != 0) || (y != 0); break;
                }
                out[(size_t)i] = fl ? (double)(float)v : v;   // f32 tensors stay f32
            }
            set_host(n.out[0], od, out, fl);
            return true;
        };
        auto un = [&](double (*f)(double)) {
            std::vector<double> v = host_values(in[0]);
            for (auto& e : v) e = f(e);
            set_host(n.out[0], in[0].dims, v, float_like(in[0]));
            return true;
        };
        if (op == "Add") return bin(0);
        if (op == "Sub") return bin(1);
        if (op == "Mul") return bin(2);
        if (op == "Div") return bin(3);
        if (op == "Pow") return bin(4);
        if (op == "Max") return bin(5);
        if (op == "Min") return bin(6);
        if (op == "Equal") return bin(7);
        if (op == "Less") return bin(8);
        if (op == "Greater") return bin(9);
        if (op == "And") return bin(10);
        if (op == "Or") return bin(11);
        if (op == "Neg") return un([](double v) { return -v; });
        if (op == "Abs") return un([](double v) { return std::fabs(v); });
        if (op == "Floor") return un([](double v) { return std::floor(v); });
        if (op == "Ceil") return un([](double v) { return std::ceil(v); });
        if (op == "Round") return un([](double v) { return std::nearbyint(v); });
        if (op == "Sqrt") return un([](double v) { return (double)std::sqrt((float)v); });
        if (op == "Not") return un([](double v) { return v != 0 ? 0.0 : 1.0; });
        if (op == "Identity") { set_host(n.out[0], in[0].dims, host_values(in[0]), float_like(in[0])); return true; }
        if (op == "Cast") {
            const int64_t to = n.ai("to", 1);
            std::vector<double> v = host_values(in[0]);
            const bool to_f = to == 1 || to == 10 || to == 11 || to == 16;
            if (!to_f) for (auto& e : v) e = to == 9 ? (double)(e != 0) : (double)(int64_t)e;
            else if (to == 1) for (auto& e : v) e = (double)(float)e;
            set_host(n.out[0], in[0].dims, v, to_f);
            return true;
        }
        if (op == "Where") {   // numpy broadcasting over the aligned dims, like bin above (matching element COUNTS say nothing: [3,1] and [1,3] give [3,3])
            std::vector<double> v[3] = {host_values(in[0]), host_values(in[1]), host_values(in[2])};
            size_t r = 0;
            for (int q = 0; q < 3; ++q) r = std::max(r, in[q].dims.size());
            std::vector<int64_t> d[3], st[3], od(r, 1);
            for (int q = 0; q < 3; ++q) {
                if ((int64_t)v[q].size() != numel(in[q].dims)) return false;
                d[q].assign(r - in[q].dims.size(), 1);
                d[q].insert(d[q].end(), in[q].dims.begin(), in[q].dims.end());
                st[q] = contig_strides(d[q]);
                for (size_t i = 0; i < r; ++i) od[i] = std::max(od[i], d[q][i]);
            }
            for (int q = 0; q < 3; ++q)
                for (size_t i = 0; i < r; ++i) if (d[q][i] != od[i] && d[q][i] != 1) return false;   // op_where reports the mismatch
            std::vector<double> out((size_t)numel(od));
            for (int64_t i = 0; i < (int64_t)out.size(); ++i) {
                int64_t rem = i, o[3] = {0, 0, 0};
                for (int k = (int)r - 1; k >= 0; --k) {
                    const int64_t q = rem / od[k], ix = rem - q * od[k];
                    rem = q;
                    for (int t = 0; t < 3; ++t) o[t] += (d[t][k] == 1 ? 0 : ix) * st[t][k];
                }
                out[(size_t)i] = v[0][(size_t)o[0]] != 0 ? v[1][(size_t)o[1]] : v[2][(size_t)o[2]];
            }
            set_host(n.out[0], od, out, float_like(in[1]) || float_like(in[2]));
            return true;
        }
        if (op == "Expand") {
            if (!in[1].host_int) return false;
            std::vector<double> v = host_values(in[0]);
            const int64_t cnt = numel(in[1].hv);
            if (!(v.size() == 1 || ((int64_t)v.size() == cnt && in[0].dims.size() <= 1)) || cnt > 4096) return false;   // real data: device path
            std::vector<double> out((size_t)cnt);
            for (int64_t i = 0; i < cnt; ++i) out[(size_t)i] = v[v.size() == 1 ? 0 : (size_t)i];
            set_host(n.out[0], in[1].hv, out, float_like(in[0]));
            return true;
        }
        if (op == "Tile") {
            if (!(in[0].dims.size() <= 1 && in[1].hv.size() == 1 && in[1].host_int)) return false;   // real data: device path
            std::vector<double> v = host_values(in[0]), out;
            // (a shape-arithmetic vector: the repeat count comes from the model file -- bounded, and never negative)
            OAR_CHECK(in[1].hv[0] >= 0 && in[1].hv[0] * (int64_t)std::max<size_t>(v.size(), 1) <= 4096, OAR_MODEL_LOAD, "Tile: unreasonable repeat count of a host vector at " + n.out[0]);
            for (int64_t k = 0; k < in[1].hv[0]; ++k) out.insert(out.end(), v.begin(), v.end());
            set_host(n.out[0], {(int64_t)out.size()}, out, float_like(in[0]));
            return true;
        }
        if (op == "Range") {
            const double a = host_values(in[0])[0], lim = host_values(in[1])[0], d = host_values(in[2])[0];
            OAR_CHECK(d != 0, OAR_INVALID_INPUT, "Range: delta 0");
            std::vector<double> out;
            const int64_t cnt = std::max<int64_t>((int64_t)std::ceil((lim - a) / d), 0);
            OAR_CHECK(cnt <= 1 << 20, OAR_SHAPE_MISMATCH, "Range: too long");
            for (int64_t i = 0; i < cnt; ++i) out.push_back(a + (double)i * d);
            set_host(n.out[0], {cnt}, out, float_like(in[0]));
            return true;
        }
        if (op == "ReduceProd" || op == "ReduceSum" || op == "ReduceMax" || op == "ReduceMin") {
            std::vector<double> v = host_values(in[0]);
            if (in[0].dims.size() > 1) return false;
            double acc = op == "ReduceProd" ? 1.0 : op == "ReduceSum" ? 0.0 : op == "ReduceMax" ? -INFINITY : INFINITY;
            for (double e : v) acc = op == "ReduceProd" ? acc * e : op == "ReduceSum" ? acc + e : op == "ReduceMax" ? std::max(acc, e) : std::min(acc, e);
            set_host(n.out[0], n.ai("keepdims", 1) ? std::vector<int64_t>{1} : std::vector<int64_t>{}, {acc}, float_like(in[0]));
            return true;
        }
        return false;
    }

    // GridSample (UVDoc's final un-warp): X [N,C,H,W], grid [N,Ho,Wo,2] -> [N,C,Ho,Wo]
    void op_grid_sample(const GNode& n) {
        TInfo x = get(n.in[0]), g = get(n.in[1]);
        OAR_CHECK(x.dims.size() == 4 && g.dims.size() == 4 && g.dims[3] == 2 && g.dims[0] == x.dims[0], OAR_UNSUPPORTED_OP, "GridSample: 4-D input and [N,Ho,Wo,2] grid only");
        const std::string mode = n.as("mode", "linear"), pad = n.as("padding_mode", "zeros");
        const int imode = (mode == "linear" || mode == "bilinear") ? 0 : mode == "nearest" ? 1 : -1;
        const int ipad = pad == "zeros" ? 0 : pad == "border" ? 1 : pad == "reflection" ? 2 : -1;
        OAR_CHECK(imode >= 0 && ipad >= 0, OAR_UNSUPPORTED_OP, "GridSample: mode " + mode + " / padding_mode " + pad);
        const int align = (int)n.ai("align_corners", 0);
        Loc xin = to_clast_loc(x), gin = to_native_loc(g);
        const int64_t N = x.dims[0], C = x.dims[1], H = x.dims[2], W = x.dims[3], Ho = g.dims[1], Wo = g.dims[2];
        TInfo& y = new_out(n.out[0], {N, C, Ho, Wo}, Layout::CLAST);
        Loc yl = y.loc;
        step([=](const RunCtx& c) { k::grid_sample(c.s, c.at(xin), c.at(gin), c.mut(yl), (int)N, (int)H, (int)W, (int)C, (int)Ho, (int)Wo, imode, ipad, align); },
             8.0 * N * Ho * Wo * C, 4.0 * N * Ho * Wo * (2 + 5 * C));
    }

    // fused squeeze-excite gate (rewrite pass 6): pooled [n,C,1,1] -> [n,Cout,1,1]
    void op_se_gate(const GNode& n) {
        TInfo x = get(n.in[0]);
        OAR_CHECK(x.dims.size() == 4 && x.dims[2] == 1 && x.dims[3] == 1, OAR_SHAPE_MISMATCH, "SEGate: input must be [n, C, 1, 1]");
        const TInfo &w1 = get(n.in[1]), &w2 = get(n.in[3]);
        OAR_CHECK(w1.ht && w2.ht, OAR_UNSUPPORTED_OP, "SEGate: weights must be initializers");
        const int tiles = x.gap_tiles, gap_hw = x.gap_hw;   // > 0: the input still is the producing conv's tile sums
        const int64_t N = x.dims[0], C = tiles > 0 ? x.dims[1] / tiles : x.dims[1], Cmid = w1.ht->dims[0], Cout = w2.ht->dims[0];
        OAR_CHECK(w1.ht->dims[1] == C && w2.ht->dims[1] == Cmid, OAR_SHAPE_MISMATCH, "SEGate: weight shapes");
        const float* b1 = has_input(n, 2) ? get(n.in[2]).loc.cptr : nullptr;
        const float* b2 = has_input(n, 4) ? get(n.in[4]).loc.cptr : nullptr;
        const float* w1p = w1.loc.cptr;
        std::vector<float> w2t((size_t)(Cmid * Cout));   // [Cout][Cmid] -> [Cmid][Cout]: the kernel's threads run along Cout
        for (int64_t c = 0; c < Cout; ++c)
            for (int64_t j = 0; j < Cmid; ++j) w2t[(size_t)(j * Cout + c)] = w2.ht->f[(size_t)(c * Cmid + j)];
        const float* w2p = E.upload_const("segate_w2t:" + n.in[3], w2t);
        Act a1; a1.kind = (int)n.ai("act1", 0); a1.alpha = n.af("act1_alpha", 0.f); a1.beta = n.af("act1_beta", 0.f);
        Act a2 = n.act;
        Loc xin = x.loc;   // [n, C, 1, 1]: the same bytes in either layout
        TInfo& y = new_out(n.out[0], {N, Cout, 1, 1}, Layout::CLAST);
        Loc yl = y.loc;
        step([=](const RunCtx& c) { k::se_fc(c.s, c.at(xin), w1p, b1, a1, w2p, b2, a2, c.mut(yl), (int)N, (int)C, (int)Cmid, (int)Cout, tiles, gap_hw); },
             2.0 * N * Cmid * (C + Cout), 4.0 * (N * (C + Cout) + Cmid * (C + Cout)));
    }

    // Pad (UVDoc's reflect-padded convolutions export as Pad(reflect) + Conv).  Works on the physical layout: a
    // channels-last tensor is padded in place of a conversion (the pads are permuted with the dims).
    void op_pad(const GNode& n) {
        TInfo x = get(n.in[0]);
        const int r = (int)x.dims.size();
        std::vector<int64_t> pads = has_input(n, 1) ? get(n.in[1]).hv : n.ais("pads");
        std::vector<int64_t> axes;
        if (has_input(n, 3)) axes = get(n.in[3]).hv;
        std::vector<int64_t> before(r, 0), after(r, 0);
        if (axes.empty()) {
            OAR_CHECK((int)pads.size() == 2 * r, OAR_SHAPE_MISMATCH, "Pad: pads must have 2 * rank entries");
            for (int d = 0; d < r; ++d) { before[d] = pads[d]; after[d] = pads[r + d]; }
        } else {
            OAR_CHECK(pads.size() == 2 * axes.size(), OAR_SHAPE_MISMATCH, "Pad: pads must have 2 * len(axes) entries");
            for (size_t k = 0; k < axes.size(); ++k) { int64_t a = axes[k] < 0 ? axes[k] + r : axes[k]; before[a] = pads[k]; after[a] = pads[axes.size() + k]; }
        }
        const std::string mode = n.as("mode", "constant");
        const int imode = mode == "constant" ? 0 : mode == "reflect" ? 1 : mode == "edge" ? 2 : -1;
        OAR_CHECK(imode >= 0, OAR_UNSUPPORTED_OP, "Pad: mode " + mode);
        float value = n.af("value", 0.0f);
        if (has_input(n, 2)) { const TInfo& v = get(n.in[2]); if (v.ht && !v.ht->f.empty()) value = v.ht->f[0]; }
        std::vector<int64_t> od(r);
        for (int d = 0; d < r; ++d) {
            od[d] = x.dims[d] + before[d] + after[d];
            OAR_CHECK(od[d] >= 0, OAR_SHAPE_MISMATCH, "Pad: negative output dimension");
            // (negative pads crop first: the reflection is taken on what is left of the axis, so it has to stay inside that)
            const int64_t kept = std::max<int64_t>(x.dims[d] + std::min<int64_t>(before[d], 0) + std::min<int64_t>(after[d], 0), 1);
            OAR_CHECK(imode != 1 || (before[d] < kept && after[d] < kept) || x.dims[d] == 1, OAR_UNSUPPORTED_OP, "Pad: reflect padding wider than the axis");
        }
        const bool clast = x.layout == Layout::CLAST && r >= 3;
        std::vector<int64_t> pin = clast ? clast_phys_dims(x.dims) : x.dims, pout = clast ? clast_phys_dims(od) : od, pbef = clast ? clast_phys_dims(before) : before;
        Loc xin = x.loc;
        TInfo& y = new_out(n.out[0], od, clast ? Layout::CLAST : Layout::NATIVE);
        Loc yl = y.loc;
        step([=](const RunCtx& c) { k::pad_nd(c.s, c.at(xin), c.mut(yl), r, pin.data(), pout.data(), pbef.data(), imode, value); }, 0, 8.0 * numel(od));
    }

    void op_gap(const GNode& n) {
        TInfo x = get(n.in[0]);
        OAR_CHECK(x.dims.size() == 4, OAR_UNSUPPORTED_OP, "GlobalAveragePool: rank-4 only");
        Loc xin = to_clast_loc(x);
        int64_t N = x.dims[0], C = x.dims[1], HW = x.dims[2] * x.dims[3];
        TInfo& y = new_out(n.out[0], {N, C, 1, 1}, Layout::CLAST);
        Loc yl = y.loc;
        const int splits = k::global_avgpool_splits((int)N, (int)HW, (int)C);
        Loc part;
        if (splits > 1) part = alloc_temp((size_t)N * splits * C * sizeof(float));
        step([=](const RunCtx& c) { k::global_avgpool(c.s, c.at(xin), c.mut(yl), (int)N, (int)HW, (int)C, splits > 1 ? c.mut(part) : nullptr); }, 0, 4.0 * numel(x.dims));
    }

    void op_pool(const GNode& n, bool is_max) {
        TInfo x = get(n.in[0]);
        OAR_CHECK(x.dims.size() == 4, OAR_UNSUPPORTED_OP, "Pool: rank-4 only");
        auto ks = n.ais("kernel_shape"), st = n.ais("strides");
        OAR_CHECK(ks.size() == 2, OAR_UNSUPPORTED_OP, "Pool: kernel_shape");
        int64_t kh = ks[0], kw = ks[1], sh = st.size() == 2 ? st[0] : 1, sw = st.size() == 2 ? st[1] : 1;
        int64_t pt, pl, pb, pr;
        get_pads(n, x.dims[2], x.dims[3], kh, kw, sh, sw, 1, 1, pt, pl, pb, pr);
        bool ceil_mode = n.ai("ceil_mode", 0) != 0;
        auto od = [&](int64_t in, int64_t k_, int64_t s_, int64_t p0, int64_t p1) {
            int64_t t = in + p0 + p1 - k_;
            int64_t o = (ceil_mode ? (t + s_ - 1) / s_ : t / s_) + 1;
            if (ceil_mode && (o - 1) * s_ >= in + p0) --o;
            return o;
        };
        int64_t Ho = od(x.dims[2], kh, sh, pt, pb), Wo = od(x.dims[3], kw, sw, pl, pr);
        Loc xin = to_clast_loc(x);
        TInfo& y = new_out(n.out[0], {x.dims[0], x.dims[1], Ho, Wo}, Layout::CLAST);
        k::PoolP p{};
        p.N = (int)x.dims[0]; p.H = (int)x.dims[2]; p.W = (int)x.dims[3]; p.C = (int)x.dims[1]; p.Ho = (int)Ho; p.Wo = (int)Wo;
        p.kh = (int)kh; p.kw = (int)kw; p.sh = (int)sh; p.sw = (int)sw; p.pt = (int)pt; p.pl = (int)pl; p.pb = (int)pb; p.pr = (int)pr;
        p.is_max = is_max; p.count_include_pad = (int)n.ai("count_include_pad", 0);
        Loc yl = y.loc;
        auto run = [=](const RunCtx& c) { k::PoolP q = p; q.x = c.at(xin); q.y = c.mut(yl); k::pool2d(c.s, q); };
        const double bytes = 4.0 * (numel(x.dims) + numel(y.dims));
        // round 5: an average pool that leaves ONE row of tokens per sample (the recognizer's [6, 2] pool in front of the SVTR neck) only
        // reads its own sample: as the first operator of a sample-local chain (chain.hip CH_POOL) it costs no launch.  OAR_CHAIN_POOL=0 keeps it apart.
        const char* cpe = getenv("OAR_CHAIN_POOL");
        if (!(cpe && cpe[0] == '0') && !is_max && !ceil_mode && Ho == 1 && kh == x.dims[2] && kw == sw && kw * Wo <= x.dims[3] && x.dims[3] - kw * Wo < kw && pt == 0 && pl == 0 && pb == 0 && pr == 0 &&
            (p.C & 3) == 0 && kh * kw <= 64 && chain_loc_ok(xin)) {
            ChainRec r;
            r.d.type = k::CH_POOL; r.d.K = (int)kh; r.d.cin = (int)kw; r.d.pad = (int)x.dims[3]; r.d.N = p.C; r.d.in_ld = p.C; r.d.out_ld = p.C;
            r.in = xin; r.out = yl; r.rows = x.dims[0] * Wo; r.fix_n = x.dims[0]; r.fix_T = Wo; r.out_root = n.out[0];
            step_chainable(run, std::move(r), 0, bytes);
        } else {
            step(run, 0, bytes);
        }
    }

    void op_resize(const GNode& n) {
        TInfo x = get(n.in[0]);
        OAR_CHECK(x.dims.size() == 4, OAR_UNSUPPORTED_OP, "Resize: rank-4 only");
        int64_t H = x.dims[2], W = x.dims[3], Ho, Wo;
        float sh, sw;
        if (has_input(n, 3)) {
            const TInfo& sz = get(n.in[3]);
            OAR_CHECK(sz.host_int && sz.hv.size() == 4, OAR_UNSUPPORTED_OP, "Resize: sizes must be a host int tensor");
            Ho = sz.hv[2]; Wo = sz.hv[3]; sh = (float)Ho / (float)H; sw = (float)Wo / (float)W;
        } else {
            OAR_CHECK(has_input(n, 2), OAR_UNSUPPORTED_OP, "Resize: neither scales nor sizes");
            const TInfo& sc = get(n.in[2]);
            std::vector<double> scv = host_values(sc);   // an initializer, or computed from Shape on the host
            OAR_CHECK(host_evaluable(sc) && scv.size() == 4, OAR_UNSUPPORTED_OP, "Resize: scales must be 4 floats known at plan time");
            sh = (float)scv[2]; sw = (float)scv[3];
            Ho = (int64_t)std::floor((float)H * sh); Wo = (int64_t)std::floor((float)W * sw);
        }
        std::string mode = n.as("mode", "nearest"), ctm = n.as("coordinate_transformation_mode", "half_pixel"), nm = n.as("nearest_mode", "round_prefer_floor");
        int imode = mode == "nearest" ? 0 : 1;
        OAR_CHECK(mode == "nearest" || mode == "linear", OAR_UNSUPPORTED_OP, "Resize: mode " + mode);
        int ictm = ctm == "asymmetric" ? 0 : ctm == "half_pixel" ? 1 : ctm == "align_corners" ? 2 : ctm == "pytorch_half_pixel" ? 3 : -1;
        OAR_CHECK(ictm >= 0, OAR_UNSUPPORTED_OP, "Resize: coordinate_transformation_mode " + ctm);
        int inm = nm == "floor" ? 0 : nm == "round_prefer_floor" ? 1 : nm == "round_prefer_ceil" ? 2 : 3;
        static const bool defer_on = [] { const char* e = getenv("OAR_DEFER_RESIZE"); return !e || atoi(e) != 0; }();
        if (defer_on && imode == 0 && x.layout == Layout::CLAST && sole_consumer.count(n.out[0])) {
            PendingResize r;
            r.xin = x.loc; r.dims = {x.dims[0], x.dims[1], Ho, Wo};
            r.N = (int)x.dims[0]; r.H = (int)H; r.W = (int)W; r.C = (int)x.dims[1]; r.Ho = (int)Ho; r.Wo = (int)Wo;
            r.imode = imode; r.ictm = ictm; r.inm = inm; r.sh = sh; r.sw = sw;
            // integer-factor upsampling whose index map is o / f: checked on the map itself, whatever the attributes say
            auto factor = [&](int in, int out, float scale) {
                if (in <= 0 || out % in != 0) return 0;
                const int f = out / in;
                for (int o = 0; o < out; ++o) if (k::resize_nearest_index(o, scale, in, out, ictm, inm) != o / f) return 0;
                return f;
            };
            r.fh = factor(r.H, r.Ho, sh); r.fw = factor(r.W, r.Wo, sw);
            if (!r.fh || !r.fw) r.fh = r.fw = 0;
            pending_resize[n.out[0]] = r;
            TInfo t;   // known shape, no storage yet
            t.dims = r.dims; t.layout = Layout::CLAST; t.root = "";
            vals[n.out[0]] = t;
            return;
        }
        Loc xin = to_clast_loc(x);
        TInfo& y = new_out(n.out[0], {x.dims[0], x.dims[1], Ho, Wo}, Layout::CLAST);
        Loc yl = y.loc;
        int N = (int)x.dims[0], C = (int)x.dims[1];
        step([=](const RunCtx& c) { k::resize(c.s, c.at(xin), c.mut(yl), N, (int)H, (int)W, C, (int)Ho, (int)Wo, sh, sw, imode, ictm, inm, C); }, 0,
             4.0 * (numel(x.dims) + numel(y.dims)));
    }

    void op_concat(const GNode& n) {
        // deferred resizes among the inputs: absorbed when this is a channel concat of channels-last tensors with float4-aligned
        // slots, run on the spot otherwise
        bool absorb = false;
        if (!pending_resize.empty()) {
            int64_t axis0 = n.ai("axis", 0);
            bool ok = true, any = false;
            int64_t total_c = 0;
            for (auto& s : n.in) {
                const PendingResize* pr = peek_pending(s);
                any = any || pr;
                auto it = vals.find(s);
                if (it == vals.end() || it->second.dims.size() != 4 || it->second.layout != Layout::CLAST || it->second.host_int) { ok = false; break; }
                if ((it->second.dims[1] & 3) != 0) ok = false;
                total_c += it->second.dims[1];
            }
            absorb = any && ok && (axis0 == 1 || axis0 == -3) && (total_c & 3) == 0;
            if (!absorb) for (auto& s : n.in) materialise_pending(s);
        }
        std::vector<TInfo> xs;
        for (auto& s : n.in) { auto it = vals.find(s); xs.push_back(absorb && peek_pending(s) ? it->second : get(s)); }
        bool all_host = true, any_host = false, any_f = false;
        for (auto& t : xs) { all_host = all_host && host_evaluable(t) && t.dims.size() <= 1; any_host = any_host || t.host_int; any_f = any_f || float_like(t); }
        if (all_host && any_host) {   // 1-D shape / scale vectors
            std::vector<double> v;
            for (auto& t : xs) { std::vector<double> e = host_values(t); v.insert(v.end(), e.begin(), e.end()); }
            set_host(n.out[0], {(int64_t)v.size()}, v, any_f);
            return;
        }
        int r = (int)xs[0].dims.size();
        int64_t axis = n.ai("axis", 0);
        if (axis < 0) axis += r;
        bool clast = false;
        for (auto& t : xs) clast = clast || (t.layout == Layout::CLAST);
        std::vector<int64_t> od = xs[0].dims;
        od[axis] = 0;
        for (auto& t : xs) od[axis] += t.dims[axis];
        if (clast && r >= 3) {
            // physical axis of the logical axis
            int pax = axis == 0 ? 0 : (axis == 1 ? r - 1 : (int)axis - 1);
            std::vector<int64_t> pod = clast_phys_dims(od);
            int64_t outer = 1, inner = 1;
            for (int i = 0; i < pax; ++i) outer *= pod[i];
            for (int i = pax + 1; i < r; ++i) inner *= pod[i];
            std::vector<Loc> ins;
            for (size_t i = 0; i < xs.size(); ++i) ins.push_back(absorb && peek_pending(n.in[i]) ? Loc() : to_clast_loc(xs[i]));
            int64_t coff = 0, total = pod[pax] * inner;
            // round 5: every absorbed resize an integer-factor nearest upsampling (the DB neck: up8 / up4 / up2 of three pyramid levels next to
            // the finest one) -> the whole concat is ONE gather launch instead of one launch per input.  OAR_CONCAT_GATHER=0 restores those.
            // round 6: the same launch for a plain channel concat of three or more maps (PP-HGNetV2's blocks concatenate seven: one gather instead of seven
            // strided copies)
            bool plain = !absorb && r == 4 && inner == 1 && xs.size() >= 3 && (od[1] & 3) == 0;
            for (auto& t : xs) plain = plain && t.dims.size() == 4 && (t.dims[1] & 3) == 0;
            // (round 6, later) ... or no launch at all when the only reader is a 1x1 convolution that can read the sources itself (pending_concat above)
            static const bool defer_on = [] { const char* e = getenv("OAR_CONCAT_DEFER"); return !(e && e[0] == '0'); }();
            if (plain && defer_on && xs.size() <= 8 && concat_consumer.count(n.out[0])) {
                const GNode& cn = E.nodes_[concat_consumer[n.out[0]]];
                auto wi = E.inits_.find(cn.in.size() > 1 ? cn.in[1] : std::string());
                auto attr_ok = [&](const char* a, int64_t want) { auto v = cn.ais(a); for (auto e : v) if (e != want) return false; return true; };
                bool ok = wi != E.inits_.end() && wi->second.dims.size() == 4 && wi->second.dims[2] == 1 && wi->second.dims[3] == 1 && wi->second.dims[1] == od[1] && cn.ai("group", 1) == 1 &&
                          attr_ok("strides", 1) && attr_ok("pads", 0) && attr_ok("dilations", 1) && cn.residual.empty() && !(cn.in.size() > 3 && !cn.in[3].empty()) &&
                          cn.as("auto_pad", "NOTSET") == "NOTSET";
                for (auto& t : xs) ok = ok && t.layout == Layout::CLAST && (t.dims[1] & 7) == 0 && t.dims[0] == od[0] && t.dims[2] == od[2] && t.dims[3] == od[3] && !t.host_int;   // (channels-last already: a converted copy would be a temporary of THIS node)
                ok = ok && k::conv_msrc_ok((long)(od[0] * od[2] * od[3]), (int)od[1], (int)wi->second.dims[0]) && (wi->second.dims[0] & 3) == 0;
                if (ok) {
                    PendingConcat pc;
                    for (size_t i = 0; i < xs.size(); ++i) { pc.src.push_back(ins[i]); pc.c.push_back((int)xs[i].dims[1]); }
                    pc.dims = od;
                    TInfo t;
                    t.dims = od; t.layout = Layout::CLAST;
                    vals[n.out[0]] = t;          // shape only: no storage unless somebody materialises it
                    pending_concat[n.out[0]] = std::move(pc);
                    return;
                }
            }
            TInfo& y = new_out(n.out[0], od, Layout::CLAST);   // (below the deferral: a deferred concat owns no storage)
            Loc yl = y.loc;
            if ((absorb || plain) && r == 4 && inner == 1 && xs.size() <= 8) {
                static const bool gather_on = [] { const char* e = getenv("OAR_CONCAT_GATHER"); return !(e && e[0] == '0'); }();
                bool ok = gather_on;
                for (size_t i = 0; ok && i < xs.size(); ++i) {
                    const PendingResize* pr = peek_pending(n.in[i]);
                    if (pr) ok = pr->fh > 0 && pr->fw > 0 && pr->imode == 0 && pr->Ho == od[2] && pr->Wo == od[3] && pr->H * pr->fh == pr->Ho && pr->W * pr->fw == pr->Wo && pr->N == od[0];
                    else ok = xs[i].dims[0] == od[0] && xs[i].dims[2] == od[2] && xs[i].dims[3] == od[3];
                }
                if (ok) {
                    k::ConcatGatherP gp{};
                    std::vector<Loc> src(xs.size());
                    gp.n_src = (int)xs.size(); gp.N = (int)od[0]; gp.Ho = (int)od[2]; gp.Wo = (int)od[3]; gp.C = (int)od[1];
                    double bytes = 4.0 * (double)numel(od);
                    for (size_t i = 0; i < xs.size(); ++i) {
                        const PendingResize* pr = peek_pending(n.in[i]);
                        src[i] = pr ? pr->xin : ins[i];
                        gp.c[i] = (int)xs[i].dims[1]; gp.off[i] = (int)coff; gp.fh[i] = pr ? pr->fh : 1; gp.fw[i] = pr ? pr->fw : 1;
                        bytes += 4.0 * (double)numel(xs[i].dims) / (gp.fh[i] * gp.fw[i]);
                        coff += xs[i].dims[1];
                    }
                    for (auto& nm : n.in) pending_resize.erase(nm);
                    step([=](const RunCtx& c) {
                        k::ConcatGatherP q = gp;
                        for (int i = 0; i < q.n_src; ++i) q.x[i] = c.at(src[(size_t)i]);
                        k::concat_gather(c.s, q, c.mut(yl));
                    }, 0, bytes);
                    return;
                }
            }
            for (size_t i = 0; i < xs.size(); ++i) {
                int64_t w = xs[i].dims[axis] * inner;
                Loc il = ins[i];
                int64_t off = coff;
                if (absorb && peek_pending(n.in[i])) {   // the resize writes its pixels' channel group in place
                    run_resize(*peek_pending(n.in[i]), yl, off, (int)total);
                    pending_resize.erase(n.in[i]);
                } else {
                    concat_copy_step(il, yl, off, outer, w, total, n.out[0]);
                }
                coff += w;
            }
            return;
        }
        int64_t outer = 1, inner = 1;
        for (int i = 0; i < axis; ++i) outer *= od[i];
        for (int i = (int)axis + 1; i < r; ++i) inner *= od[i];
        std::vector<Loc> ins;
        for (auto& t : xs) ins.push_back(to_native_loc(t));
        bool all_int = true;   // index tensors concatenated stay an index tensor
        for (auto& t : xs) all_int = all_int && t.is_int;
        TInfo& y = new_out(n.out[0], od, Layout::NATIVE);
        y.is_int = all_int;
        Loc yl = y.loc;
        int64_t coff = 0, total = od[axis] * inner;
        for (size_t i = 0; i < xs.size(); ++i) {
            int64_t w = xs[i].dims[axis] * inner;
            Loc il = ins[i];
            int64_t off = coff;
            concat_copy_step(il, yl, off, outer, w, total, n.out[0]);
            coff += w;
        }
    }
    // one input of a Concat: `outer` rows of w floats into columns [off, off + w) of rows of `total` floats
    void concat_copy_step(Loc il, Loc yl, int64_t off, int64_t outer, int64_t w, int64_t total, const std::string& out_name) {
        auto run = [=](const RunCtx& c) { k::copy2d(c.s, c.at(il), c.mut(yl) + off, outer, (int)w, (int)w, (int)total); };
        if ((w & 3) == 0 && (total & 3) == 0 && (off & 3) == 0 && chain_loc_ok(il) && yl.kind == Loc::ARENA) {
            ChainRec r;
            r.d.type = k::CH_COPY; r.d.N = (int)w; r.d.in_ld = (int)w; r.d.out_ld = (int)total;
            r.in = il; r.out = yl; r.out.off += off * 4; r.rows = outer; r.out_root = out_name;
            step_chainable(run, std::move(r), 0, 8.0 * outer * w);
        } else {
            step(run, 0, 8.0 * outer * w);
        }
    }

    // Reshape-like ops produce views of the native buffer.
    void view_native(const GNode& n, const TInfo& x, const std::vector<int64_t>& od) {
        OAR_CHECK(numel(od) == numel(x.dims), OAR_SHAPE_MISMATCH, "reshape: element count mismatch at " + n.out[0]);
        if (x.layout == Layout::CLAST) {
            int r = (int)x.dims.size();
            int64_t sp = 1;
            for (int i = 2; i < r; ++i) sp *= x.dims[i];
            // [n, C, spatial...] -> [n, C, other spatial grouping] (SVTRv2's map <-> token moves: Reshape [n,C,H,W] -> [n,C,H*W] in front of a
            // Transpose to [n,H*W,C], and back): channels-last keeps the spatial positions in row-major order whatever their grouping -- a view
            if (od.size() >= 3 && od[0] == x.dims[0] && od[1] == x.dims[1] && !x.ht) { alias_out(n.out[0], x, od, Layout::CLAST); return; }
            if (x.dims[1] != 1 && sp != 1) {  // genuine transpose needed
                TInfo& y = new_out(n.out[0], od, Layout::NATIVE);
                to_native_loc(x, y.loc);
                return;
            }
        }
        alias_out(n.out[0], x, od, Layout::NATIVE);
    }

    void op_reshape(const GNode& n) {
        TInfo x = get(n.in[0]);
        const TInfo& sh = get(n.in[1]);
        OAR_CHECK(sh.host_int, OAR_UNSUPPORTED_OP, "Reshape: shape must be known on the host");
        if (x.host_int) { TInfo o = x; o.dims.assign(sh.hv.begin(), sh.hv.end()); vals[n.out[0]] = o; return; }
        std::vector<int64_t> od(sh.hv.size());
        int64_t known = 1; int infer = -1;
        for (size_t i = 0; i < od.size(); ++i) {
            int64_t v = sh.hv[i];
            if (v == 0 && n.ai("allowzero", 0) == 0) v = x.dims[i];
            if (v == -1) { infer = (int)i; v = 1; }
            od[i] = v; known *= v;
        }
        if (infer >= 0) od[infer] = numel(x.dims) / std::max<int64_t>(known, 1);
        view_native(n, x, od);
    }

    void op_flatten(const GNode& n) {
        TInfo x = get(n.in[0]);
        int64_t ax = n.ai("axis", 1);
        if (ax < 0) ax += (int64_t)x.dims.size();
        int64_t a = 1, b = 1;
        for (int i = 0; i < (int)x.dims.size(); ++i) (i < ax ? a : b) *= x.dims[i];
        view_native(n, x, {a, b});
    }

    std::vector<int64_t> axes_of(const GNode& n, size_t input_idx) {
        if (has_input(n, input_idx)) { const TInfo& a = get(n.in[input_idx]); OAR_CHECK(a.host_int, OAR_UNSUPPORTED_OP, "axes must be host ints"); return a.hv; }
        return n.ais("axes");
    }

    void op_squeeze(const GNode& n) {
        TInfo x = get(n.in[0]);
        std::vector<int64_t> axes = axes_of(n, 1);
        int r = (int)x.dims.size();
        std::set<int> ax;
        if (axes.empty()) { for (int i = 0; i < r; ++i) if (x.dims[i] == 1) ax.insert(i); }
        for (auto a : axes) ax.insert((int)(a < 0 ? a + r : a));
        std::vector<int64_t> od;
        for (int i = 0; i < r; ++i) if (!ax.count(i)) od.push_back(x.dims[i]);
        if (x.host_int) { TInfo o = x; o.dims = od; vals[n.out[0]] = o; return; }
        // channels-last stays channels-last when only spatial axes are removed and rank stays >= 3
        if (x.layout == Layout::CLAST && !ax.count(0) && !ax.count(1) && od.size() >= 3) { alias_out(n.out[0], x, od, Layout::CLAST); return; }
        view_native(n, x, od);
    }

    void op_unsqueeze(const GNode& n) {
        TInfo x = get(n.in[0]);
        std::vector<int64_t> axes = axes_of(n, 1);
        int r = (int)x.dims.size() + (int)axes.size();
        std::set<int> ax;
        for (auto a : axes) ax.insert((int)(a < 0 ? a + r : a));
        std::vector<int64_t> od;
        size_t j = 0;
        for (int i = 0; i < r; ++i) od.push_back(ax.count(i) ? 1 : x.dims[j++]);
        if (x.host_int) { TInfo o = x; o.dims = od; vals[n.out[0]] = o; return; }
        if (x.layout == Layout::CLAST && !ax.count(0) && !ax.count(1) && r <= 5) { alias_out(n.out[0], x, od, Layout::CLAST); return; }
        view_native(n, x, od);
    }

    void op_transpose(const GNode& n) {
        TInfo x = get(n.in[0]);
        int r = (int)x.dims.size();
        std::vector<int64_t> perm = n.ais("perm");
        if (perm.empty()) for (int i = r - 1; i >= 0; --i) perm.push_back(i);
        std::vector<int64_t> od(r);
        for (int i = 0; i < r; ++i) od[i] = x.dims[perm[i]];
        // lazy channels-last moves: [n,C,s..] <-> [n,s..,C]
        bool to_last = r >= 3 && perm[0] == 0 && perm[r - 1] == 1;
        if (to_last) for (int i = 1; i < r - 1; ++i) to_last = to_last && perm[i] == i + 1;
        bool from_last = r >= 3 && perm[0] == 0 && perm[1] == r - 1;
        if (from_last) for (int i = 2; i < r; ++i) from_last = from_last && perm[i] == i - 1;
        if (x.layout == Layout::CLAST && to_last) { alias_out(n.out[0], x, od, Layout::NATIVE); return; }
        if (x.layout == Layout::NATIVE && from_last && r <= 5 && !x.ht) { alias_out(n.out[0], x, od, Layout::CLAST); return; }
        Loc xin = to_native_loc(x);
        std::vector<int64_t> ns = contig_strides(x.dims), is(r);
        for (int i = 0; i < r; ++i) is[i] = ns[perm[i]];
        TInfo& y = new_out(n.out[0], od, Layout::NATIVE);
        y.is_int = x.is_int;
        Loc yl = y.loc;
        step([=](const RunCtx& c) { k::permute(c.s, c.at(xin), c.mut(yl), r, od.data(), is.data()); }, 0, 8.0 * numel(od));
    }

    // strided sub-tensor copy (or alias when the slice is a contiguous prefix-dim block)
    void slice_out(const std::string& out, const TInfo& x, Loc xin, int axis, int64_t start, int64_t len) {
        std::vector<int64_t> od = x.dims;
        od[axis] = len;
        std::vector<int64_t> ns = contig_strides(x.dims);
        bool outer_all_one = true;
        for (int i = 0; i < axis; ++i) outer_all_one = outer_all_one && x.dims[i] == 1;
        if (outer_all_one) {
            TInfo tmp = x; tmp.loc = xin; tmp.layout = Layout::NATIVE;
            if (xin.kind != x.loc.kind || xin.off != x.loc.off) tmp.root = "";  // temp buffers cannot be aliased safely
            if (!tmp.root.empty() || xin.kind == Loc::CONST) { alias_out(out, tmp, od, Layout::NATIVE, start * ns[axis] * 4); return; }
        }
        TInfo& y = new_out(out, od, Layout::NATIVE);
        y.is_int = x.is_int;
        Loc yl = y.loc;
        int r = (int)od.size();
        int64_t off = start * ns[axis];
        step([=](const RunCtx& c) { k::permute(c.s, c.at(xin) + off, c.mut(yl), r, od.data(), ns.data()); }, 0, 8.0 * numel(od));
    }

    void op_split(const GNode& n) {
        TInfo x = get(n.in[0]);
        int r = (int)x.dims.size();
        int64_t axis = n.ai("axis", 0);
        if (axis < 0) axis += r;
        std::vector<int64_t> parts;
        if (has_input(n, 1)) parts = get(n.in[1]).hv;
        else if (n.has("split")) parts = n.ais("split");
        else parts.assign(n.out.size(), x.dims[axis] / (int64_t)n.out.size());
        Loc xin = to_native_loc(x);
        int64_t start = 0;
        for (size_t i = 0; i < n.out.size(); ++i) { slice_out(n.out[i], x, xin, (int)axis, start, parts[i]); start += parts[i]; }
    }

    void op_slice(const GNode& n) {
        TInfo x = get(n.in[0]);
        std::vector<int64_t> starts = get(n.in[1]).hv, ends = get(n.in[2]).hv, axes, steps;
        if (has_input(n, 3)) axes = get(n.in[3]).hv; else for (size_t i = 0; i < starts.size(); ++i) axes.push_back((int64_t)i);
        if (has_input(n, 4)) steps = get(n.in[4]).hv; else steps.assign(starts.size(), 1);
        int r = (int)x.dims.size();
        if (x.host_int) {
            OAR_CHECK(r == 1 && axes.size() == 1 && steps[0] == 1, OAR_UNSUPPORTED_OP, "Slice: host tensors support 1-D unit-step only");
            int64_t d = x.dims[0], s = starts[0] < 0 ? starts[0] + d : starts[0], e = ends[0] < 0 ? ends[0] + d : ends[0];
            s = std::min(std::max<int64_t>(s, 0), d); e = std::min(std::max<int64_t>(e, 0), d);
            std::vector<double> xv = host_values(x);
            set_host(n.out[0], {std::max<int64_t>(e - s, 0)}, std::vector<double>(xv.begin() + s, xv.begin() + std::max(s, e)), x.host_f);
            return;
        }
        OAR_CHECK(axes.size() == 1 && steps[0] == 1, OAR_UNSUPPORTED_OP, "Slice: single axis, unit step only");
        int64_t ax = axes[0] < 0 ? axes[0] + r : axes[0], d = x.dims[ax];
        int64_t s = starts[0] < 0 ? starts[0] + d : starts[0], e = ends[0] < 0 ? ends[0] + d : ends[0];
        s = std::min(std::max<int64_t>(s, 0), d); e = std::min(std::max<int64_t>(e, 0), d);
        Loc xin = to_native_loc(x);
        slice_out(n.out[0], x, xin, (int)ax, s, std::max<int64_t>(e - s, 0));
    }

    void op_gather(const GNode& n) {
        TInfo x = get(n.in[0]);
        const TInfo& idx = get(n.in[1]);
        int64_t axis = n.ai("axis", 0);
        if (!idx.host_int || (!x.host_int && idx.hv.size() != 1)) return op_gather_device(n);   // device indices, or several host ints
        if (x.host_int) {
            OAR_CHECK(x.dims.size() <= 1, OAR_UNSUPPORTED_OP, "Gather: host data rank > 1");
            std::vector<double> xv = host_values(x), ov;
            for (auto i : idx.hv) {
                const int64_t j = i < 0 ? i + (int64_t)xv.size() : i;
                OAR_CHECK(j >= 0 && j < (int64_t)xv.size(), OAR_SHAPE_MISMATCH, "Gather: index out of range at " + n.out[0]);
                ov.push_back(xv[(size_t)j]);
            }
            set_host(n.out[0], idx.dims, ov, x.host_f);
            return;
        }
        int r = (int)x.dims.size();
        if (axis < 0) axis += r;
        OAR_CHECK(idx.hv.size() == 1, OAR_UNSUPPORTED_OP, "Gather: only a single index is supported on device tensors");
        int64_t i = idx.hv[0] < 0 ? idx.hv[0] + x.dims[axis] : idx.hv[0];
        Loc xin = to_native_loc(x);
        std::string tmpn = n.out[0] + "::gather_slice";
        slice_out(tmpn, x, xin, (int)axis, i, 1);
        TInfo s = vals[tmpn];
        std::vector<int64_t> od;
        for (int d = 0; d < r; ++d) if (d != axis || !idx.dims.empty()) od.push_back(d == axis ? 1 : x.dims[d]);
        alias_out(n.out[0], s, od, Layout::NATIVE);
        adopt_root(n.out[0], tmpn);   // (when the slice was a copy: the bytes are this node's output)
    }

    // ------------------------------------------------------------------ device-side selection (index_ops.hip)
    // An index operand: a device index tensor (is_int) or host ints, range-checked here and uploaded once as f32.
    // dim_of(i): the extent the i-th index addresses.
    template <typename F>
    Loc index_operand(const GNode& n, size_t in_idx, const TInfo& idx, F dim_of) {
        if (idx.host_int) {
            OAR_CHECK(!idx.host_f, OAR_UNSUPPORTED_OP, n.op + ": indices must be integers at " + n.out[0]);
            for (size_t i = 0; i < idx.hv.size(); ++i) {
                const int64_t d = dim_of(i), v = idx.hv[i] < 0 ? idx.hv[i] + d : idx.hv[i];
                OAR_CHECK(v >= 0 && v < d, OAR_SHAPE_MISMATCH, n.op + ": index out of range at " + n.out[0]);
            }
            return host_to_device(n.in[in_idx], idx);
        }
        OAR_CHECK(idx.is_int && idx.loc.kind != Loc::NONE, OAR_UNSUPPORTED_OP, n.op + ": indices must be an integer tensor at " + n.out[0]);
        return to_native_loc(idx);
    }
    // data operand of a gather: device tensor, or a plan-time value materialised as one
    Loc gather_data(const GNode& n, const TInfo& x, bool& is_int) {
        for (auto d : x.dims) OAR_CHECK(d < (1 << 24), OAR_UNSUPPORTED_OP, n.op + ": a dimension of 2^24 or more cannot be addressed by f32-coded indices");
        is_int = x.host_int ? !x.host_f : x.is_int;
        return x.host_int ? host_to_device(n.in[0], x) : to_native_loc(x);
    }

    // TopK over the last axis, K known at plan time
    void op_topk(const GNode& n) {
        TInfo x = get(n.in[0]);
        OAR_CHECK(n.in.size() >= 2 && !n.in[1].empty(), OAR_UNSUPPORTED_OP, "TopK: K must be input 1 (opset >= 10)");
        const TInfo& kt = get(n.in[1]);
        OAR_CHECK(kt.host_int && kt.hv.size() == 1, OAR_UNSUPPORTED_OP, "TopK: K must be known on the host");
        OAR_CHECK(!x.host_int && !x.dims.empty(), OAR_UNSUPPORTED_OP, "TopK: input must be a device tensor of rank >= 1");
        const int r = (int)x.dims.size();
        int64_t axis = n.ai("axis", -1);
        if (axis < 0) axis += r;
        OAR_CHECK(axis == r - 1, OAR_UNSUPPORTED_OP, "TopK: only the last axis is supported");
        const int64_t C = x.dims[axis], K = kt.hv[0], rows = numel(x.dims) / std::max<int64_t>(C, 1);
        OAR_CHECK(C >= 1 && C <= k::kTopKMaxC, OAR_UNSUPPORTED_OP, "TopK: row length " + std::to_string(C) + " is outside [1, " + std::to_string(k::kTopKMaxC) + "]");
        OAR_CHECK(K >= 1 && K <= C, OAR_SHAPE_MISMATCH, "TopK: K = " + std::to_string(K) + " is outside [1, " + std::to_string(C) + "] at " + n.out[0]);
        const bool largest = n.ai("largest", 1) != 0;   // (sorted = 0 leaves the order free: sorted results are a valid answer)
        Loc xin = to_native_loc(x);
        std::vector<int64_t> od = x.dims;
        od[axis] = K;
        auto out = [&](size_t i, bool is_int) -> Loc {
            if (i >= n.out.size() || n.out[i].empty()) return alloc_temp((size_t)std::max<int64_t>(numel(od), 1) * 4);
            TInfo& y = new_out(n.out[i], od, Layout::NATIVE);
            y.is_int = is_int;
            return y.loc;
        };
        Loc vl = out(0, x.is_int), il = out(1, true);
        step([=](const RunCtx& c) { k::topk_lastdim(c.s, c.at(xin), c.mut(vl), c.mut(il), rows, (int)C, (int)K, largest); }, 0, 4.0 * rows * (C + 2.0 * K));
    }

    // The SLANet structure head (rewrite pass 0): every step of the greedy decode in one launch (sla_decode.hip).  Nothing is allocated or read back at
    // run time, so the plan stays capturable; all `steps` steps run (exact Loop semantics), the host decoder stops at eos.
    void op_sla_decode(const GNode& n) {
        TInfo fea = get(n.in[0]), proj = get(n.in[1]), h0 = get(n.in[2]), pre0 = get(n.in[3]);
        const int64_t M = n.ai("steps", 0), H = n.ai("hidden", 0), C = n.ai("channels", 0), V = n.ai("vocab", 0), L = n.ai("loc", 0);
        OAR_CHECK(!fea.host_int && fea.dims.size() == 3 && fea.dims[2] == C, OAR_SHAPE_MISMATCH, "SLADecode: the features must be [B, HW, " + std::to_string(C) + "] at " + n.out[2]);
        const int64_t B = fea.dims[0], HW = fea.dims[1];
        OAR_CHECK(B >= 1 && B < (1 << 20), OAR_SHAPE_MISMATCH, "SLADecode: batch out of range at " + n.out[2]);
        OAR_CHECK(k::sla_decode_supported((int)std::min<int64_t>(HW, 1 << 20), (int)C, (int)H, (int)V, (int)L, (int)M), OAR_UNSUPPORTED_OP,
                  "Loop (" + n.out[2] + "): HW = " + std::to_string(HW) + " is outside 1 <= HW <= " + std::to_string(k::kSlaMaxHW));
        OAR_CHECK(proj.dims == (std::vector<int64_t>{B, HW, H}), OAR_INTERNAL, "SLADecode: projection shape");
        OAR_CHECK(numel(h0.dims) == B * H && numel(pre0.dims) == B, OAR_SHAPE_MISMATCH, "SLADecode: the initial state must be h0 [B, H] and pre0 [B] at " + n.out[2]);
        OAR_CHECK(pre0.host_int ? !pre0.host_f : pre0.is_int, OAR_UNSUPPORTED_OP, "SLADecode: pre0 must be an integer tensor at " + n.out[2]);
        auto dev = [&](const std::string& nm, const TInfo& t) -> Loc { return t.host_int ? host_to_device(nm, t) : to_native_loc(t); };
        Loc fl = to_native_loc(fea), pl = to_native_loc(proj), hl = dev(n.in[2], h0), p0 = dev(n.in[3], pre0);
        k::SlaDecodeP p{};
        p.B = (int)B; p.HW = (int)HW; p.C = (int)C; p.H = (int)H; p.V = (int)V; p.L = (int)L; p.M = (int)M;
        const float** w[12] = {&p.w_h4, &p.b_h4, &p.w_score, &p.w_ihc, &p.w_ihv, &p.b_ih, &p.w_sl1, &p.b_sl1, &p.w_s2, &p.b_s2, &p.w_l2, &p.b_l2};
        for (int i = 0; i < 12; ++i) {
            const TInfo& t = get(n.in[(size_t)(4 + i)]);
            OAR_CHECK(t.ht && t.loc.kind == Loc::CONST, OAR_INTERNAL, "SLADecode: weight is not a constant");
            *w[i] = t.loc.cptr;
        }
        auto out = [&](size_t i, std::vector<int64_t> od, bool is_int) -> Loc {
            if (i >= n.out.size() || n.out[i].empty()) return alloc_temp((size_t)numel(od) * 4);
            TInfo& y = new_out(n.out[i], od, Layout::NATIVE);
            y.is_int = is_int;
            return y.loc;
        };
        Loc ho = out(0, {B, H}, false), po = out(1, {B}, true), lo = out(2, {M, B, V}, false), bo = out(3, {M, B, L}, false);
        const double macs = 4.0 * H * H + (double)HW * H + (double)HW * C + 3.0 * H * C + 2.0 * H * H + ((double)V + L) * H;   // per step and image
        step([=](const RunCtx& c) {
            k::SlaDecodeP q = p;
            q.fea = c.at(fl); q.proj = c.at(pl); q.h0 = c.at(hl); q.pre0 = c.at(p0);
            q.h_out = c.mut(ho); q.pre_out = c.mut(po); q.logits = c.mut(lo); q.loc = c.mut(bo);
            k::sla_decode(c.s, q);
        }, 2.0 * macs * M * B, 4.0 * (macs + 3.0 * H + V + L) * M * B);
    }

    // The formula decode head (rewrite pass 0): M steps of 8 Ld + 2 short launches per chunk of 16 images (formula_decode.hip).  By default all `steps` steps run
    // (exact Loop semantics with a constant-true condition; the host stops at eos) and nothing is allocated, read back or synchronised between them, so the plan
    // stays capturable.  With Engine::set_decode_stop on (read at run time, not planned) a chunk ends once each of its images has emitted the stop token: outside
    // a capture the host waits on an event kFdLookahead steps back, reads one mapped word and stops enqueuing at most kFdLookahead steps late; inside a capture
    // all steps are enqueued and skipped on the device.  The cost below stays the full-M figure: an upper bound in that mode.
    void op_formula_decode(const GNode& n) {
        const int64_t M = n.ai("steps", 0), Ld = n.ai("layers", 0), D = n.ai("width", 0), nh = n.ai("heads", 1), F = n.ai("ffn", 0), V = n.ai("vocab", 0), P = n.ai("positions", 0);
        const int64_t dh = D / nh, dq = n.ai("qk_head", dh), Dq = nh * dq;
        const std::string& name = n.out[1];
        TInfo tok0 = get(n.in[0]);
        const int64_t B = numel(tok0.dims);
        OAR_CHECK(B >= 1 && B < (1 << 20), OAR_SHAPE_MISMATCH, "FormulaDecode: batch out of range at " + name);
        OAR_CHECK(tok0.host_int ? !tok0.host_f : tok0.is_int, OAR_UNSUPPORTED_OP, "FormulaDecode: the start tokens must be an integer tensor at " + name);
        Loc t0 = tok0.host_int ? host_to_device(n.in[0], tok0) : to_native_loc(tok0);
        std::vector<Loc> mem;
        int64_t S = 0;
        for (int64_t l = 0; l < Ld; ++l) {
            TInfo kt = get(n.in[(size_t)(1 + 2 * l)]), vm = get(n.in[(size_t)(2 + 2 * l)]);
            OAR_CHECK(!kt.host_int && !vm.host_int && kt.dims.size() == 4 && vm.dims.size() == 4, OAR_SHAPE_MISMATCH, "FormulaDecode: the memory keys / values must be rank-4 tensors at " + name);
            if (l == 0) S = kt.dims[3];
            OAR_CHECK(S >= 1 && S <= k::kFdMaxS, OAR_UNSUPPORTED_OP, "Loop (" + name + "): S = " + std::to_string(S) + " is outside 1 <= S <= " + std::to_string(k::kFdMaxS));
            OAR_CHECK(kt.dims == (std::vector<int64_t>{B, nh, dh, S}) && vm.dims == (std::vector<int64_t>{B, nh, S, dh}), OAR_SHAPE_MISMATCH,
                      "FormulaDecode: layer " + std::to_string(l + 1) + " needs KmT [B, " + std::to_string(nh) + ", " + std::to_string(dh) + ", S] and Vm [B, " + std::to_string(nh) + ", S, " + std::to_string(dh) + "] at " + name);
            mem.push_back(to_native_loc(kt));
            mem.push_back(to_native_loc(vm));
        }
        k::FormulaDecodeP p{};
        p.B = (int)B; p.D = (int)D; p.nh = (int)nh; p.F = (int)F; p.V = (int)V; p.Ld = (int)Ld; p.S = (int)S; p.M = (int)M; p.P = (int)P; p.c_pos = (int)n.ai("c_pos", 0);
        p.dq = (int)dq;
        p.s_emb = n.af("s_emb", 1.0f); p.eps_e = n.af("eps_e", 1e-5f); p.eps_f = n.af("eps_f", 1e-5f);
        size_t ci = (size_t)(1 + 2 * Ld);
        auto cw = [&]() -> const float* {
            const TInfo& t = get(n.in[ci++]);
            OAR_CHECK(t.ht && t.loc.kind == Loc::CONST, OAR_INTERNAL, "FormulaDecode: weight is not a constant");
            return t.loc.cptr;
        };
        p.e_tok = cw(); p.e_pos = cw(); p.lne_g = cw(); p.lne_b = cw();
        for (int64_t l = 0; l < Ld; ++l) {
            k::FdLayerP& Y = p.layer[l];
            const std::string s = "l" + std::to_string(l) + "_";
            Y.ln1_g = cw(); Y.ln1_b = cw(); Y.w_qkv = cw(); Y.b_qkv = cw(); Y.w_o = cw(); Y.b_o = cw(); Y.ln2_g = cw(); Y.ln2_b = cw(); Y.w_cq = cw(); Y.b_cq = cw(); Y.w_co = cw(); Y.b_co = cw();
            Y.ln3_g = cw(); Y.ln3_b = cw(); Y.w_1 = cw(); Y.b_1 = cw(); Y.w_2 = cw(); Y.b_2 = cw();
            Y.eps1 = n.af((s + "eps1").c_str(), 1e-5f); Y.eps2 = n.af((s + "eps2").c_str(), 1e-5f); Y.eps3 = n.af((s + "eps3").c_str(), 1e-5f);
            Y.q_scale_mode = (int)n.ai((s + "q_mode").c_str(), 0); Y.q_scale = n.af((s + "q_scale").c_str(), 1.0f);
            Y.cq_scale_mode = (int)n.ai((s + "cq_mode").c_str(), 0); Y.cq_scale = n.af((s + "cq_scale").c_str(), 1.0f);
        }
        p.lnf_g = cw(); p.lnf_b = cw(); p.w_lm = cw();
        p.b_lm = n.ai("lm_bias", 0) ? cw() : nullptr;
        OAR_CHECK(k::formula_decode_supported((int)D, (int)nh, (int)F, (int)V, (int)Ld, (int)M, (int)S, (int)dq), OAR_UNSUPPORTED_OP, "Loop (" + name + "): shape outside the formula decode kernels' limits");
        TInfo& ty = new_out(n.out[1], {M, B}, Layout::NATIVE);
        ty.is_int = true;
        const Loc tl = ty.loc;
        Loc ll;
        const bool with_logits = n.out.size() > 2 && !n.out[2].empty();
        if (with_logits) ll = new_out(n.out[2], {M, B, V}, Layout::NATIVE).loc;
        if (!n.out[0].empty()) alias_out(n.out[0], get(n.out[1]), {B}, Layout::NATIVE, (M - 1) * B * 4);   // the final token: the last row of the scan
        Loc ws = alloc_temp(k::formula_decode_ws_floats((int)B, (int)D, (int)F, (int)V, (int)Ld, (int)M, (int)Dq) * 4);
        const int64_t chunks = (B + k::kFdChunk - 1) / k::kFdChunk;
        const double Dp = (double)((D + 3) / 4 * 4), Fp = (double)((F + 3) / 4 * 4);
        // (squeeze attention: Wq / Wk have Dq rows and the key cache is Dq wide; Dq == D gives the figures of the plain head)
        const double w_floats = Ld * ((4.0 * D + 2.0 * Dq) * Dp + F * Dp + D * Fp + 13.0 * D + 2.0 * Dq + F) + V * Dp + V + 4.0 * D;          // weights one step streams
        const double macs = Ld * ((4.0 * D + 2.0 * Dq) * D + 2.0 * F * D + (double)S * D * 2.0 + (double)(M + 1) * (Dq + D) / 2.0) + (double)V * D;   // per step and image (self attention at its mean length)
        this->P.decode_steps += M * chunks;
        Engine* const eng = &E;
        step([=](const RunCtx& c) {
            k::FormulaDecodeP q = p;
            q.stop = eng->fd_.token >= 0 ? &eng->fd_ : nullptr;
            q.stats = &eng->fd_stats_;
            q.tok0 = c.at(t0);
            for (int l = 0; l < q.Ld; ++l) { q.layer[l].kmT = c.at(mem[(size_t)(2 * l)]); q.layer[l].vm = c.at(mem[(size_t)(2 * l + 1)]); }
            q.ws = c.mut(ws); q.tokens = c.mut(tl); q.logits = with_logits ? c.mut(ll) : nullptr;
            k::formula_decode(c.s, q);
        }, 2.0 * macs * M * B, 4.0 * (w_floats * chunks + (double)B * (2.0 * Ld * S * D + (with_logits ? V : 0))) * M);
    }

    // Gather with a tensor of indices: y = x[..., idx, ...] along `axis`
    void op_gather_device(const GNode& n) {
        TInfo x = get(n.in[0]), idx = get(n.in[1]);
        const int r = (int)x.dims.size();
        int64_t axis = n.ai("axis", 0);
        if (axis < 0) axis += r;
        OAR_CHECK(r >= 1 && axis >= 0 && axis < r, OAR_SHAPE_MISMATCH, "Gather: axis out of range at " + n.out[0]);
        bool is_int = false;
        Loc xin = gather_data(n, x, is_int);
        const int64_t D = x.dims[axis];
        Loc iin = index_operand(n, 1, idx, [&](size_t) { return D; });
        k::GatherRowsP p{};
        int64_t outer = 1, inner = 1;
        for (int i = 0; i < axis; ++i) outer *= x.dims[i];
        for (int i = (int)axis + 1; i < r; ++i) inner *= x.dims[i];
        const int64_t J = numel(idx.dims);
        p.slices = outer * J; p.inner = inner; p.group = std::max<int64_t>(J, 1); p.group_stride = D * inner; p.idx_mod = J; p.m = 1;
        p.dims[0] = D; p.strides[0] = inner;
        std::vector<int64_t> od(x.dims.begin(), x.dims.begin() + axis);
        od.insert(od.end(), idx.dims.begin(), idx.dims.end());
        od.insert(od.end(), x.dims.begin() + axis + 1, x.dims.end());
        TInfo& y = new_out(n.out[0], od, Layout::NATIVE);
        y.is_int = is_int;
        Loc yl = y.loc;
        step([=](const RunCtx& c) { k::gather_rows(c.s, c.at(xin), c.at(iin), c.mut(yl), p); }, 0, 8.0 * numel(od) + 4.0 * J);
    }

    // GatherND: the last axis of `indices` holds tuples of m leading coordinates (after batch_dims shared ones)
    void op_gather_nd(const GNode& n) {
        TInfo x = get(n.in[0]), idx = get(n.in[1]);
        const int64_t b = n.ai("batch_dims", 0);
        OAR_CHECK(b == 0 || b == 1, OAR_UNSUPPORTED_OP, "GatherND: batch_dims > 1 is not supported");
        const int r = (int)x.dims.size(), q = (int)idx.dims.size();
        OAR_CHECK(r >= 1 && q >= 1 && b < r && b < q, OAR_SHAPE_MISMATCH, "GatherND: rank of data / indices at " + n.out[0]);
        const int64_t m = idx.dims[q - 1];
        OAR_CHECK(m >= 1 && m <= r - b && m <= 6, OAR_SHAPE_MISMATCH, "GatherND: index tuples of length " + std::to_string(m) + " for data of rank " + std::to_string(r) + " at " + n.out[0]);
        for (int i = 0; i < b; ++i) OAR_CHECK(x.dims[i] == idx.dims[i], OAR_SHAPE_MISMATCH, "GatherND: batch dimensions of data and indices differ at " + n.out[0]);
        bool is_int = false;
        Loc xin = gather_data(n, x, is_int);
        Loc iin = index_operand(n, 1, idx, [&](size_t i) { return x.dims[(size_t)b + i % (size_t)m]; });
        const std::vector<int64_t> xs = contig_strides(x.dims);
        k::GatherRowsP p{};
        int64_t batch = 1;
        for (int i = 0; i < b; ++i) batch *= x.dims[i];
        std::vector<int64_t> od(idx.dims.begin(), idx.dims.end() - 1);
        p.slices = numel(od);
        od.insert(od.end(), x.dims.begin() + b + m, x.dims.end());
        p.inner = 1;
        for (int i = (int)(b + m); i < r; ++i) p.inner *= x.dims[i];
        p.group = std::max<int64_t>(p.slices / std::max<int64_t>(batch, 1), 1);
        p.group_stride = b > 0 ? xs[(size_t)b - 1] : 0;
        p.idx_mod = 0; p.m = (int)m;
        for (int i = 0; i < m; ++i) { p.dims[i] = x.dims[(size_t)(b + i)]; p.strides[i] = xs[(size_t)(b + i)]; }
        TInfo& y = new_out(n.out[0], od, Layout::NATIVE);
        y.is_int = is_int;
        Loc yl = y.loc;
        step([=](const RunCtx& c) { k::gather_rows(c.s, c.at(xin), c.at(iin), c.mut(yl), p); }, 0, 8.0 * numel(od) + 4.0 * numel(idx.dims));
    }

    // GatherElements: y[i...] = x[i... with coordinate `axis` replaced by idx[i...]]; y has the shape of idx
    void op_gather_elements(const GNode& n) {
        TInfo x = get(n.in[0]), idx = get(n.in[1]);
        const int r = (int)x.dims.size();
        OAR_CHECK(r >= 1 && r <= 6, OAR_UNSUPPORTED_OP, "GatherElements: rank must be in [1, 6]");
        OAR_CHECK((int)idx.dims.size() == r, OAR_SHAPE_MISMATCH, "GatherElements: data and indices differ in rank at " + n.out[0]);
        int64_t axis = n.ai("axis", 0);
        if (axis < 0) axis += r;
        OAR_CHECK(axis >= 0 && axis < r, OAR_SHAPE_MISMATCH, "GatherElements: axis out of range at " + n.out[0]);
        for (int i = 0; i < r; ++i) OAR_CHECK(i == axis || idx.dims[i] <= x.dims[i], OAR_SHAPE_MISMATCH, "GatherElements: indices exceed the data's shape at " + n.out[0]);
        bool is_int = false;
        Loc xin = gather_data(n, x, is_int);
        const int64_t D = x.dims[axis];
        Loc iin = index_operand(n, 1, idx, [&](size_t) { return D; });
        const std::vector<int64_t> xs = contig_strides(x.dims);
        k::GatherElemP p{};
        p.total = numel(idx.dims); p.axis_dim = D; p.rank = r; p.axis = (int)axis;
        for (int i = 0; i < r; ++i) { p.dims[i] = idx.dims[i]; p.xstrides[i] = xs[(size_t)i]; }
        TInfo& y = new_out(n.out[0], idx.dims, Layout::NATIVE);
        y.is_int = is_int;
        Loc yl = y.loc;
        step([=](const RunCtx& c) { k::gather_elements(c.s, c.at(xin), c.at(iin), c.mut(yl), p); }, 0, 12.0 * (double)p.total);
    }

    // true when `name` is consumed by nothing but the Softmax that produces graph output 0
    bool feeds_final_softmax(const std::string& name) {
        int users = 0; bool ok = false;
        for (const GNode& m : E.nodes_)
            for (const std::string& in : m.in)
                if (in == name) { ++users; ok = m.op == "Softmax" && !m.out.empty() && m.out[0] == E.output_names_[0]; }
        for (const std::string& on : E.output_names_) if (on == name) return false;
        return users == 1 && ok;
    }
    void op_linear(const GNode& n, bool gemm) {
        TInfo a = get(n.in[0]);
        const TInfo& bt = get(n.in[1]);
        OAR_CHECK(bt.ht, OAR_UNSUPPORTED_OP, "Linear: B must be an initializer");
        OAR_CHECK(bt.ht->dims.size() == 2 && !a.dims.empty(), OAR_MODEL_LOAD, "Linear: B must be a rank-2 initializer at " + n.out[0]);
        bool transB = gemm && n.ai("transB", 0) != 0;
        OAR_CHECK(!gemm || n.ai("transA", 0) == 0, OAR_UNSUPPORTED_OP, "Gemm: transA");
        int64_t K = transB ? bt.ht->dims[1] : bt.ht->dims[0], N = transB ? bt.ht->dims[0] : bt.ht->dims[1];
        OAR_CHECK(a.dims.back() == K, OAR_SHAPE_MISMATCH, "Linear: inner dimension mismatch at " + n.out[0]);
        Loc ain = to_native_loc(a);
        int64_t M = numel(a.dims) / K;
        std::vector<int64_t> od = a.dims;
        od.back() = N;
        const float* bias = nullptr;
        float alpha = gemm ? n.af("alpha", 1.0f) : 1.0f;
        if (!n.bias.empty()) { const TInfo& bb = get(n.bias); OAR_CHECK(bb.ht && (int64_t)bb.ht->f.size() == N, OAR_MODEL_LOAD, "Linear: bias must have N elements at " + n.out[0]); bias = bb.loc.cptr; }
        if (gemm && has_input(n, 2)) {
            const TInfo& c = get(n.in[2]);
            OAR_CHECK(c.ht && numel(c.dims) == N, OAR_UNSUPPORTED_OP, "Gemm: C must be a constant of N elements");
            const float beta = n.af("beta", 1.0f);
            if (beta == 1.0f) bias = c.loc.cptr;
            else if (beta != 0.0f) {   // beta * C folded into a constant of its own (round 6)
                std::vector<float> bc(c.ht->f);
                for (auto& v : bc) v *= beta;
                bias = E.upload_const("gemm_beta_c:" + n.out[0], bc);
            }
        }
        Loc res;
        if (!n.residual.empty()) { TInfo r = get(n.residual); OAR_CHECK(numel(r.dims) == M * N, OAR_SHAPE_MISMATCH, "Linear: residual shape"); res = to_native_loc(r); }
        bool has_res = res.kind != Loc::NONE;
        // Logits that only feed the fused softmax+argmax tail are produced with their row padded to a multiple of 16
        // channels (zero weight rows, zero bias): every store is a full float4 and the wide layer qualifies for the
        // weight-stationary kernel; the tail reads the first N columns of each row (Plan::logits_valid).
        int64_t Np = N;
        if (skip_final_softmax && !has_res && K % 4 == 0 && alpha == 1.0f && (N & 15) != 0 && feeds_final_softmax(n.out[0])) {
            Np = (N + 15) / 16 * 16;
            od.back() = Np;
            P.logits_valid = (int)N;
            if (bias) {
                std::string key = "biaspad:" + n.out[0];
                auto it = E.dev_consts_.find(key);
                if (it == E.dev_consts_.end()) {
                    const HostTensor* hb = !n.bias.empty() ? get(n.bias).ht : get(n.in[2]).ht;
                    OAR_CHECK(hb, OAR_INTERNAL, "Linear: bias initializer missing");
                    std::vector<float> bp((size_t)Np, 0.f);
                    for (int64_t i = 0; i < N; ++i) bp[(size_t)i] = hb->f[(size_t)i];
                    bias = E.upload_const(key, bp);
                } else bias = it->second;
            }
        }
        TInfo& y = new_out(n.out[0], od, Layout::NATIVE);
        Loc yl = y.loc;
        Act act = n.act;
        double flops = 2.0 * M * N * K, bytes = 4.0 * (M * K + M * N * (has_res ? 2 : 1) + K * N);
        // A residual that rewrite pass 4 folded into this Linear, with a marked LayerNormalization as the next node (pass 10): where nobody else reads the sum,
        // the Linear can write its product alone and k::add_layernorm add the residual in registers -- the same two launches and the same bytes as the epilogue
        // route, and the sum never reaches HBM.  A sum that is read again stays in the epilogue, which has to store it anyway.  fuse_chains decides (a chain
        // that takes either step keeps both as they are); last_add.lin is this Linear without its residual.
        last_add = AddRec();
        const bool give_back = has_res && E.fuse_add_ln_ && act.kind == k::ACT_NONE && N > 0 && yl.kind == Loc::ARENA && cur + 1 < (int)E.nodes_.size() &&
                               E.nodes_[(size_t)cur + 1].op == "LayerNormalization" && E.nodes_[(size_t)cur + 1].ai("after_add", 0) != 0 &&
                               E.nodes_[(size_t)cur + 1].in[0] == n.out[0] && read_after(n.out[0]) <= cur + 1 && loc_on_16(yl) && loc_on_16(res);
        if (K % 4 == 0 && alpha == 1.0f) {
            // (a CTC head with a short K runs on the output-stationary bf16x6 kernel, ctc_head_x6.hip: bf16x6 fragments whatever igemm_weight_format says)
            const bool ctc_head = P.logits_valid > 0 && od.back() == Np && n.act.kind == k::ACT_NONE && !has_res && k::ctc_head_x6_supported((long)M, (int)K, (int)Np) &&
                                  k::ctc_partials_supported_x6((int)K) && [] { const char* e = getenv("OAR_CTC_PARTIALS"); return !e || atoi(e) != 0; }();
            const int fmt = ctc_head ? k::IGEMM_W_X6 : k::igemm_weight_format((long)M, (int)K, (int)Np, true);
            const float* w = linear_weight(n.in[1], *bt.ht, transB, fmt);
            k::ConvP p{};
            p.w_fmt = fmt;
            N = Np;
            // CTC head: when the logits only feed the fused tail, do not even write them -- per-tile softmax partials
            Loc part;
            if (P.logits_valid > 0 && od.back() == Np && act.kind == k::ACT_NONE &&
                (fmt == k::IGEMM_W_K16 ? k::ctc_partials_supported((int)K) : k::ctc_partials_supported_x6((int)K))) {
                static const bool on = [] { const char* e = getenv("OAR_CTC_PARTIALS"); return !e || atoi(e) != 0; }();
                if (on) {
                    P.ctc_tiles = k::ctc_tiles((int)Np);
                    part = alloc_arena((size_t)M * P.ctc_tiles * 16, "");   // no root: stays allocated until the end of the plan
                    P.ctc_part = part;
                }
            }
            const bool has_part = part.kind != Loc::NONE;
            p.ctc_valid = P.logits_valid;
            p.N = 1; p.H = 1; p.W = (int)M; p.Cin = (int)K; p.Ho = 1; p.Wo = (int)M; p.Cout = (int)N;
            p.kh = p.kw = p.sh = p.sw = p.dh = p.dw = 1; p.groups = 1; p.act = act; p.w = w; p.bias = bias; p.y_ld = (int)N;
            auto run = [=](const RunCtx& c) { k::ConvP q = p; q.x = c.at(ain); q.y = c.mut(yl); q.residual = has_res ? c.at(res) : nullptr; q.ctc_part = has_part ? c.mut(part) : nullptr; k::conv_igemm(c.s, q); };
            if (!has_part && P.logits_valid == 0 && K % 16 == 0 && N % 16 == 0 && k::chain_act_ok(act.kind) && chain_loc_ok(ain) && (!has_res || chain_loc_ok(res))) {
                ChainRec r;   // rows x K times K x N: any partition of the rows into samples will do
                r.d.type = k::CH_GEMM; r.d.K = (int)K; r.d.N = (int)N; r.d.cin = (int)K; r.d.pad = 0;
                r.d.in_ld = (int)K; r.d.out_ld = (int)N; r.d.res_ld = (int)N;
                r.d.act = act.kind; r.d.alpha = act.alpha; r.d.beta = act.beta; r.dev_bias = bias;
                r.in = ain; r.out = yl; if (has_res) r.res = res;
                r.rows = M; r.out_root = n.out[0];
                const HostTensor* Bp = bt.ht;
                r.make_w = [Bp, transB]() { return chain_weight_linear(*Bp, transB); };
                step_chainable(run, std::move(r), flops, bytes);
            } else {
                step(run, flops, bytes);
            }
            if (give_back) last_add.lin = [=](const RunCtx& c) { k::ConvP q = p; q.x = c.at(ain); q.y = c.mut(yl); q.residual = nullptr; k::conv_igemm(c.s, q); };
        } else {
            const float* w = bt.loc.cptr;
            k::GemmP g{};
            g.batch = 1; g.M = (int)M; g.N = (int)N; g.K = (int)K; g.transB = transB; g.alpha = alpha; g.B = w; g.bias = bias; g.act = act;
            step([=](const RunCtx& c) { k::GemmP q = g; q.A = c.at(ain); q.C = c.mut(yl); q.residual = has_res ? c.at(res) : nullptr; k::gemm_batched(c.s, q); }, flops, bytes);
            if (give_back) last_add.lin = [=](const RunCtx& c) { k::GemmP q = g; q.A = c.at(ain); q.C = c.mut(yl); q.residual = nullptr; k::gemm_batched(c.s, q); };
        }
        // (the Linear is this node's last step: op_layernorm asks for exactly that)
        if (give_back) {
            last_add.node = cur; last_add.step = (int)P.steps.size() - 1; last_add.out = n.out[0]; last_add.a = yl; last_add.b = res; last_add.sum = yl;
            last_add.C = N; last_add.rows = M; last_add.b_rows = M;
        }
    }

    void op_matmul(const GNode& n) {
        TInfo a = get(n.in[0]), b = get(n.in[1]);
        OAR_CHECK(a.dims.size() >= 2 && b.dims.size() >= 2, OAR_UNSUPPORTED_OP, "MatMul: rank < 2");
        Loc al = to_native_loc(a), bl = to_native_loc(b);
        int64_t M = a.dims[a.dims.size() - 2], K = a.dims.back(), N = b.dims.back();
        OAR_CHECK(b.dims[b.dims.size() - 2] == K, OAR_SHAPE_MISMATCH, "MatMul: inner dimension mismatch at " + n.out[0]);
        std::vector<int64_t> ba(a.dims.begin(), a.dims.end() - 2), bb(b.dims.begin(), b.dims.end() - 2);
        int64_t na = numel(ba), nb = numel(bb);
        OAR_CHECK(na == nb || nb == 1 || na == 1, OAR_UNSUPPORTED_OP, "MatMul: general batch broadcasting is not supported");
        std::vector<int64_t> od = na >= nb ? ba : bb;
        od.push_back(M); od.push_back(N);
        int64_t batch = std::max(na, nb);
        TInfo& y = new_out(n.out[0], od, Layout::NATIVE);
        Loc yl = y.loc;
        k::GemmP g{};
        g.batch = (int)batch; g.M = (int)M; g.N = (int)N; g.K = (int)K; g.transB = 0; g.alpha = 1.0f;
        g.sA = na == 1 ? 0 : M * K; g.sB = nb == 1 ? 0 : K * N; g.sC = M * N; g.act = n.act;
        step([=](const RunCtx& c) { k::GemmP q = g; q.A = c.at(al); q.B = c.at(bl); q.C = c.mut(yl); k::gemm_batched(c.s, q); },
             2.0 * batch * M * N * K, 4.0 * batch * (M * K + K * N + M * N));
    }

    void op_softmax(const GNode& n) {
        TInfo x = get(n.in[0]);
        int r = (int)x.dims.size();
        int64_t axis = n.ai("axis", E_opset13() ? -1 : 1);
        if (axis < 0) axis += r;
        Loc xin = to_native_loc(x);
        int64_t C, rows;
        if (E_opset13() && axis != r - 1 && !x.host_int) {
            // an inner axis (round 6): Transpose it to the end, soft-max there, Transpose back
            std::vector<int64_t> perm;
            for (int i = 0; i < r; ++i) if (i != axis) perm.push_back(i);
            perm.push_back(axis);
            std::vector<int64_t> inv(r);
            for (int i = 0; i < r; ++i) inv[perm[i]] = i;
            GNode t1; t1.op = "Transpose"; t1.in = {n.in[0]}; t1.out = {n.out[0] + "::moved"};
            Attr p1; p1.kind = Attr::IS; p1.is = perm; t1.attrs["perm"] = p1;
            op_transpose(t1);
            GNode sm = n; sm.in = {t1.out[0]}; sm.out = {n.out[0] + "::sm"};
            Attr la; la.kind = Attr::I; la.i = -1; sm.attrs["axis"] = la;
            op_softmax(sm);
            GNode t2; t2.op = "Transpose"; t2.in = {sm.out[0]}; t2.out = {n.out[0]};
            Attr p2; p2.kind = Attr::IS; p2.is = inv; t2.attrs["perm"] = p2;
            op_transpose(t2);
            adopt_root(n.out[0], sm.out[0]);   // (axis 1 at rank 3..5: the result is a channels-last view of "::sm")
            return;
        }
        if (E_opset13()) {
            OAR_CHECK(axis == r - 1, OAR_UNSUPPORTED_OP, "Softmax: only the last axis is supported");
            C = x.dims.back(); rows = numel(x.dims) / std::max<int64_t>(C, 1);
        } else {  // opset < 13: flatten to 2-D at `axis`
            rows = 1; C = 1;
            for (int i = 0; i < r; ++i) (i < axis ? rows : C) *= x.dims[i];
        }
        TInfo& y = new_out(n.out[0], x.dims, Layout::NATIVE);
        Loc yl = y.loc;
        step([=](const RunCtx& c) { k::softmax_lastdim(c.s, c.at(xin), c.mut(yl), rows, (int)C); }, 4.0 * rows * C, 8.0 * rows * C);
    }
    // fused SVTR attention (rewrite pass 5): x [n, T, 3*h*d] (q | k | v, each [h][d]) -> [n, T, h*d]
    void op_attention(const GNode& n) {
        TInfo x = get(n.in[0]);
        const int64_t h = n.ai("heads", 1), d = n.ai("head_dim", 1);
        OAR_CHECK(x.dims.size() == 3 && x.dims[2] == 3 * h * d, OAR_SHAPE_MISMATCH, "Attention: input must be [n, T, 3*heads*head_dim]");
        const int64_t N = x.dims[0], T = x.dims[1];
        OAR_CHECK(k::attention_fits((int)T, (int)h, (int)d), OAR_UNSUPPORTED_OP, "Attention: head_dim must be in 1..=64");
        Loc xin = to_native_loc(x);
        TInfo& y = new_out(n.out[0], {N, T, h * d}, Layout::NATIVE);
        Loc yl = y.loc;
        const float scale = n.af("scale", 1.0f);
        auto run = [=](const RunCtx& c) { k::attention(c.s, c.at(xin), c.mut(yl), (int)N, (int)T, (int)h, (int)d, scale); };
        const double flops = 4.0 * N * h * T * T * d, bytes = 4.0 * N * T * 4 * h * d;
        if (d <= k::kChainMaxHd && d % 4 == 0 && chain_loc_ok(xin)) {
            ChainRec r;
            r.d.type = k::CH_ATTN; r.d.heads = (int)h; r.d.hd = (int)d; r.d.scale = scale; r.d.N = (int)(h * d);
            r.d.in_ld = (int)(3 * h * d); r.d.out_ld = (int)(h * d);
            r.in = xin; r.out = yl; r.rows = N * T; r.fix_n = N; r.fix_T = T; r.out_root = n.out[0];
            step_chainable(run, std::move(r), flops, bytes);
        } else {
            step(run, flops, bytes);
        }
    }
    // fused Swin window attention (rewrite pass 3b): q, k, v [B, H W, heads * head_dim] in image order, bias [1, heads, N, N] -> [B, H W, heads * head_dim] in image order.
    // Optional inputs 4 .. 6: the per-window mask [1, nW, 1, N, N] and the k / v Linears' biases of a block that pads
    void op_window_attention(const GNode& n) {
        TInfo q = get(n.in[0]), kk = get(n.in[1]), v = get(n.in[2]);
        const TInfo& bt = get(n.in[3]);
        const int64_t ws = n.ai("ws", 1), H = n.ai("H", 1), W = n.ai("W", 1), h = n.ai("heads", 1), d = n.ai("head_dim", 1), N = ws * ws, C = h * d;
        const int64_t Hp = n.ai("Hp", H), Wp = n.ai("Wp", W), shift = n.ai("shift", 0);
        OAR_CHECK(k::window_attention_supported((int)ws, (int)h, (int)d) && H >= 1 && W >= 1 && Hp % ws == 0 && Wp % ws == 0 && Hp >= H && Wp >= W && Hp - H < ws && Wp - W < ws &&
                      shift >= 0 && shift < std::min(Hp, Wp), OAR_INTERNAL, "WindowAttention: the rewrite let an unsupported shape through at " + n.out[0]);
        OAR_CHECK(!q.host_int && !q.dims.empty() && q.dims.back() == C && numel(q.dims) % (H * W * C) == 0 && kk.dims == q.dims && v.dims == q.dims, OAR_SHAPE_MISMATCH,
                  "WindowAttention: q, k and v must be [B, " + std::to_string(H * W) + ", " + std::to_string(C) + "] at " + n.out[0]);
        OAR_CHECK(bt.ht && bt.loc.kind == Loc::CONST && (int64_t)bt.ht->f.size() == h * N * N, OAR_INTERNAL, "WindowAttention: the bias is not a constant of heads x N x N values at " + n.out[0]);
        const int64_t B = numel(q.dims) / (H * W * C), nW = (Hp / ws) * (Wp / ws);
        OAR_CHECK(B >= 1 && B * H * W < (int64_t)1 << 31 && B * nW < (int64_t)1 << 31, OAR_SHAPE_MISMATCH, "WindowAttention: batch out of range at " + n.out[0]);
        k::WindowAttnP p{};
        auto constant = [&](size_t i, int64_t count, const char* what) -> const float* {   // an optional constant input of `count` floats
            if (!has_input(n, i)) return nullptr;
            const TInfo& t = get(n.in[i]);
            OAR_CHECK(t.ht && t.loc.kind == Loc::CONST && (int64_t)t.ht->f.size() == count, OAR_INTERNAL, std::string("WindowAttention: ") + what + " is not a constant of the expected size at " + n.out[0]);
            return t.loc.cptr;
        };
        p.mask = constant(4, nW * N * N, "the mask");
        p.kbias = constant(5, C, "the k bias");
        p.vbias = constant(6, C, "the v bias");
        Loc ql = to_native_loc(q), kl = to_native_loc(kk), vl = to_native_loc(v);
        TInfo& y = new_out(n.out[0], {B, H * W, C}, Layout::NATIVE);   // (what the window reverse's last Reshape gives, whatever the rank of q)
        Loc yl = y.loc;
        p.bias = bt.loc.cptr; p.ldq = p.ldk = p.ldv = p.ldo = (int)C; p.B = (int)B; p.H = (int)H; p.W = (int)W; p.ws = (int)ws; p.nh = (int)h; p.dh = (int)d;
        p.scale = n.af("scale", 1.0f); p.scale_div = (int)n.ai("scale_div", 0);
        p.shift = (int)shift; p.Hp = (int)Hp; p.Wp = (int)Wp; p.nW = (int)nW;
        const double tokens = (double)B * H * W, windows = (double)B * nW;   // real tokens only: a padding token costs neither a query nor a row of q, k, v or o
        step([=](const RunCtx& c) { k::WindowAttnP r = p; r.q = c.at(ql); r.k = c.at(kl); r.v = c.at(vl); r.o = c.mut(yl); k::window_attention(c.s, r); },
             4.0 * tokens * N * C, 4.0 * (4.0 * tokens * C + windows * h * N * N * (p.mask ? 2 : 1)));
    }
    // fused ViT attention with the decomposed relative-position bias (rewrite pass 3d): qkv [B, H W, 3 heads head_dim] in image order, RhT [h, head_dim, h],
    // RwT [w, head_dim, w] with (h, w) the key grid -> [B, H W, heads * head_dim] in image order.  Optional input 3: the fused Linear's bias of a block that pads
    void op_relpos_attention(const GNode& n) {
        TInfo x = get(n.in[0]);
        const TInfo& rh = get(n.in[1]);
        const TInfo& rw = get(n.in[2]);
        const int64_t H = n.ai("H", 1), W = n.ai("W", 1), ws = n.ai("ws", 0), h = n.ai("heads", 1), d = n.ai("head_dim", 1), C = h * d;
        OAR_CHECK(k::relpos_attention_supported(1, H, W, ws, h, d), OAR_INTERNAL, "RelPosAttention: the rewrite let an unsupported shape through at " + n.out[0]);
        const int64_t gh = ws ? ws : H, gw = ws ? ws : W;
        OAR_CHECK(!x.host_int && !x.dims.empty() && x.dims.back() == 3 * C && numel(x.dims) % (H * W * 3 * C) == 0, OAR_SHAPE_MISMATCH,
                  "RelPosAttention: qkv must be [B, " + std::to_string(H * W) + ", " + std::to_string(3 * C) + "] at " + n.out[0]);
        OAR_CHECK(rh.ht && rh.loc.kind == Loc::CONST && (int64_t)rh.ht->f.size() == gh * d * gh && rw.ht && rw.loc.kind == Loc::CONST && (int64_t)rw.ht->f.size() == gw * d * gw, OAR_INTERNAL,
                  "RelPosAttention: RhT / RwT are not constants of h x head_dim x h and w x head_dim x w values at " + n.out[0]);
        const int64_t B = numel(x.dims) / (H * W * 3 * C);
        OAR_CHECK(B >= 1 && k::relpos_attention_supported(B, H, W, ws, h, d), OAR_SHAPE_MISMATCH, "RelPosAttention: batch out of range at " + n.out[0]);
        k::RelPosAttnP p{};
        if (has_input(n, 3)) {
            const TInfo& t = get(n.in[3]);
            OAR_CHECK(t.ht && t.loc.kind == Loc::CONST && (int64_t)t.ht->f.size() == 3 * C, OAR_INTERNAL, "RelPosAttention: the qkv bias is not a constant of the expected size at " + n.out[0]);
            p.bqkv = t.loc.cptr;
        }
        Loc xl = to_native_loc(x);
        TInfo& y = new_out(n.out[0], {B, H * W, C}, Layout::NATIVE);
        Loc yl = y.loc;
        p.rh = rh.loc.cptr; p.rw = rw.loc.cptr; p.B = (int)B; p.H = (int)H; p.W = (int)W; p.ws = (int)ws; p.nh = (int)h; p.dh = (int)d;
        p.scale = n.af("scale", 1.0f); p.scale_pre = n.ai("scale_pos", 0) == 0;
        const double N = (double)gh * gw, sets = (double)B * (ws ? (double)((H + ws - 1) / ws) * (double)((W + ws - 1) / ws) : 1.0) * h, tokens = (double)B * H * W;
        step([=](const RunCtx& c) { k::RelPosAttnP r = p; r.qkv = c.at(xl); r.o = c.mut(yl); k::relpos_attention(c.s, r); },
             sets * N * (4.0 * N * d + 2.0 * (gh + gw) * d), 4.0 * (4.0 * tokens * C + sets * std::ceil(N / k::kRpQueries) * 2.0 * N * d));
    }
    // fused multi-head attention with separate sources (rewrite pass 3e): q [N, Tq, heads * head_dim], k and v [N, Tk, heads * head_dim] -> [N, Tq, heads * head_dim]
    void op_mha_attention(const GNode& n) {
        TInfo q = get(n.in[0]), kk = get(n.in[1]), v = get(n.in[2]);
        const int64_t Tq = n.ai("Tq", 1), Tk = n.ai("Tk", 1), h = n.ai("heads", 1), d = n.ai("head_dim", 1), D = h * d;
        OAR_CHECK(k::mha_attention_supported(1, Tq, Tk, h, d), OAR_INTERNAL, "MultiHeadAttention: the rewrite let an unsupported shape through at " + n.out[0]);
        // (the graph's Reshape [0, T, heads, head_dim] keeps the first dimension and needs the rest to hold T heads head_dim values, whatever the rank)
        OAR_CHECK(!q.host_int && !kk.host_int && !v.host_int && !q.dims.empty() && q.dims[0] >= 1 && numel(q.dims) == q.dims[0] * Tq * D, OAR_SHAPE_MISMATCH,
                  "MultiHeadAttention: q must be [N, " + std::to_string(Tq) + ", " + std::to_string(D) + "] at " + n.out[0]);
        const int64_t N = q.dims[0];
        OAR_CHECK(!kk.dims.empty() && kk.dims[0] == N && numel(kk.dims) == N * Tk * D && !v.dims.empty() && v.dims[0] == N && numel(v.dims) == N * Tk * D, OAR_SHAPE_MISMATCH,
                  "MultiHeadAttention: k and v must be [N, " + std::to_string(Tk) + ", " + std::to_string(D) + "] at " + n.out[0]);
        OAR_CHECK(k::mha_attention_supported(N, Tq, Tk, h, d), OAR_SHAPE_MISMATCH, "MultiHeadAttention: batch out of range at " + n.out[0]);
        Loc ql = to_native_loc(q), kl = to_native_loc(kk), vl = to_native_loc(v);
        TInfo& y = new_out(n.out[0], {N, Tq, D}, Layout::NATIVE);
        Loc yl = y.loc;
        k::MhaAttnP p{};
        p.N = (int)N; p.Tq = (int)Tq; p.Tk = (int)Tk; p.nh = (int)h; p.dh = (int)d; p.ldq = p.ldk = p.ldv = (int)D;
        p.scale = n.af("scale", 1.0f); p.scale_pre = n.ai("scale_pos", 0) == 0;
        const double sets = (double)N * h;
        step([=](const RunCtx& c) { k::MhaAttnP r = p; r.q = c.at(ql); r.k = c.at(kl); r.v = c.at(vl); r.o = c.mut(yl); k::mha_attention(c.s, r); },
             sets * 4.0 * Tq * Tk * d, 4.0 * (2.0 * N * Tq * D + sets * std::ceil((double)Tq / k::kMhaQueries) * 2.0 * Tk * d));
    }
    // fused multi-scale deformable attention (rewrite pass 3c): value [N, Lv, heads * c], loc [N, Q, heads, L, P, 2], logits or weights [N, Q, heads * L * P]
    // -> [N, Q, heads * c]
    void op_deformable_attention(const GNode& n) {
        TInfo v = get(n.in[0]), lc = get(n.in[1]), w = get(n.in[2]);
        const std::vector<int64_t> lv = n.ais("levels");
        const int64_t nh = n.ai("heads", 1), P = n.ai("points", 1), L = (int64_t)lv.size() / 2;
        OAR_CHECK(L >= 1 && L <= k::kDefMaxLevels && lv.size() == (size_t)(2 * L) && !v.host_int && !lc.host_int && !w.host_int, OAR_INTERNAL, "DeformableAttention: bad node at " + n.out[0]);
        OAR_CHECK(lc.dims.size() == 6 && lc.dims[2] == nh && lc.dims[3] == L && lc.dims[4] == P && lc.dims[5] == 2 && lc.dims[0] >= 1 && lc.dims[1] >= 1, OAR_SHAPE_MISMATCH,
                  "DeformableAttention: the locations must be [N, Q, heads, levels, points, 2] at " + n.out[0]);
        const int64_t N = lc.dims[0], Q = lc.dims[1];
        k::DeformAttnP p{};
        int64_t Lv = 0;
        for (int64_t l = 0; l < L; ++l) { p.h[l] = (int)lv[(size_t)(2 * l)]; p.wd[l] = (int)lv[(size_t)(2 * l + 1)]; p.start[l] = (int)Lv; Lv += lv[(size_t)(2 * l)] * lv[(size_t)(2 * l + 1)]; }
        const int64_t per = N * Lv * nh, c = per > 0 && numel(v.dims) % per == 0 ? numel(v.dims) / per : 0;
        OAR_CHECK(c >= 1 && numel(w.dims) == N * Q * nh * L * P, OAR_SHAPE_MISMATCH,
                  "DeformableAttention: value must hold N x " + std::to_string(Lv) + " x heads x c floats and the weights N x Q x heads x levels x points at " + n.out[0]);
        OAR_CHECK(k::deformable_attention_supported(N, Q, nh, c, L, P, Lv), OAR_UNSUPPORTED_OP, "DeformableAttention: batch or query count outside the kernel's limits at " + n.out[0]);
        Loc vl = to_native_loc(v), ll = to_native_loc(lc), wl = to_native_loc(w);
        TInfo& y = new_out(n.out[0], {N, Q, nh * c}, Layout::NATIVE);
        Loc yl = y.loc;
        p.N = (int)N; p.Q = (int)Q; p.nh = (int)nh; p.c = (int)c; p.L = (int)L; p.P = (int)P; p.Lv = (int)Lv; p.softmax = (int)n.ai("softmax", 1);
        const double samples = (double)N * Q * nh * L * P;
        step([=](const RunCtx& cx) { k::DeformAttnP r = p; r.value = cx.at(vl); r.loc = cx.at(ll); r.w = cx.at(wl); r.y = cx.mut(yl); k::deformable_attention(cx.s, r); },
             samples * (9.0 * c + 24.0), 4.0 * (samples * (4.0 * c + 3.0) + (double)N * Q * nh * c));
    }
    bool E_opset13() const { return opset >= 13 || opset == 0; }
    int64_t opset = 17;

    void op_layernorm(const GNode& n) {
        TInfo x = get(n.in[0]);
        int r = (int)x.dims.size();
        int64_t axis = n.ai("axis", -1);
        if (axis < 0) axis += r;
        // a LayerNormalization that rewrite pass 2c put together without knowing x's rank: where it turns out not to be one over the last axis of a rank >= 2
        // tensor with [C] scale and bias, the exporter's own nodes are planned instead (their intermediates are per-node temporaries of this node)
        if (auto sp = E.ln_spelled_.find(n.out[0]); sp != E.ln_spelled_.end()) {
            bool fits = r >= 2 && axis == r - 1;
            // (scale / bias of another extent broadcast differently, and a [1, .., 1, C] one of a higher rank than x gives the exporter's result that rank)
            for (size_t q = 1; fits && q < 3; ++q) fits = !has_input(n, q) || (numel(get(n.in[q]).dims) == x.dims.back() && (int)get(n.in[q]).dims.size() <= r);
            // The kept nodes run inside this node: their intermediates are allocations of node `cur` like any node's temporaries, none is read after it (pass 2c
            // took the pattern only where every intermediate had its readers inside it and none was a graph output), and only the last one writes n.out[0].
            // Passes 3 and later never saw them, so they are planned exactly as the exporter wrote them.
            if (!fits) {
                for (const GNode& g : sp->second) dispatch(g);
                return;
            }
        }
        OAR_CHECK(axis == r - 1, OAR_UNSUPPORTED_OP, "LayerNormalization: only the last axis is supported");
        Loc xin = to_native_loc(x);
        const float* g = has_input(n, 1) ? get(n.in[1]).loc.cptr : nullptr;
        const float* b = has_input(n, 2) ? get(n.in[2]).loc.cptr : nullptr;
        int64_t C = x.dims.back(), rows = numel(x.dims) / std::max<int64_t>(C, 1);
        float eps = n.af("epsilon", 1e-5f);
        TInfo& y = new_out(n.out[0], x.dims, Layout::NATIVE);
        Loc yl = y.loc;
        auto run = [=](const RunCtx& c) { k::layernorm(c.s, c.at(xin), g, b, c.mut(yl), rows, (int)C, eps); };
        // the residual Add in front of it (rewrite pass 10): both steps are planned as they are, and fuse_chains replaces them by one launch unless
        // the sample-local chain takes this LayerNorm.  The sum is stored only when somebody reads it after this node (or it is a graph output).
        if (n.ai("after_add", 0) != 0 && last_add.node == cur - 1 && last_add.step == (int)P.steps.size() - 1 && last_add.out == n.in[0] && last_add.rows == rows && last_add.C == C &&
            xin.kind == Loc::ARENA && xin.off == last_add.sum.off && C > 0 && C < (1ll << 31)) {
            const AddRec ad = last_add;
            const bool keep_sum = read_after(n.in[0]) > cur;
            AddLnRec rec;
            rec.run = [=](const RunCtx& c) { k::add_layernorm(c.s, c.at(ad.a), c.at(ad.b), ad.b_rows, g, b, keep_sum ? c.mut(ad.sum) : nullptr, c.mut(yl), rows, (int)C, eps); };
            rec.bytes_saved = ad.lin ? 0.0 : 4.0 * rows * C * (keep_sum ? 1.0 : 3.0);   // behind a Linear the residual's read only moves from one launch to the other
            rec.lin = ad.lin;
            rec.label = "AddLayerNormalization -> " + n.out[0];
            add_ln_at[(int)P.steps.size()] = std::move(rec);
        }
        if (chain_loc_ok(xin) && C > 0) {
            ChainRec r;
            r.d.type = k::CH_LN; r.d.N = (int)C; r.d.in_ld = (int)C; r.d.out_ld = (int)C; r.d.eps = eps; r.dev_gamma = g; r.dev_bias = b;
            r.in = xin; r.out = yl; r.rows = rows; r.out_root = n.out[0];
            step_chainable(run, std::move(r), 8.0 * rows * C, 8.0 * rows * C);
        } else {
            step(run, 8.0 * rows * C, 8.0 * rows * C);
        }
    }

    void op_host_arith(const GNode& n, int op) {
        const TInfo &a = get(n.in[0]), &b = get(n.in[1]);
        TInfo o; o.host_int = true;
        size_t cnt = std::max(a.hv.size(), b.hv.size());
        for (size_t i = 0; i < cnt; ++i) {
            int64_t x = a.hv[a.hv.size() == 1 ? 0 : i], y = b.hv[b.hv.size() == 1 ? 0 : i], v = 0;
            switch (op) { case 0: v = x + y; break; case 1: v = x - y; break; case 2: v = x * y; break; default: v = y ? x / y : 0; }
            o.hv.push_back(v);
        }
        o.dims = a.hv.size() >= b.hv.size() ? a.dims : b.dims;
        vals[n.out[0]] = o;
    }

    // ------------------------------------------------------------------ driver
    void compute_last_use() {
        static const std::set<std::string> alias_ops = {"Reshape", "Flatten", "Squeeze", "Unsqueeze", "Transpose", "Identity", "Split", "Slice", "Gather", "Cast"};
        std::map<std::string, int> lu;
        for (int i = 0; i < (int)E.nodes_.size(); ++i) {
            const GNode& n = E.nodes_[i];
            for (auto& s : n.in) if (!s.empty()) lu[s] = i;
            if (!n.residual.empty()) lu[n.residual] = i;
        }
        for (auto& o : E.output_names_) lu[o] = 1 << 30;
        // a Resize with a single consumer may run at that consumer (PendingResize): its input has to live until then
        sole_consumer.clear();
        {
            std::map<std::string, std::pair<int, int>> uses;   // value -> (count, last consumer)
            for (int i = 0; i < (int)E.nodes_.size(); ++i) {
                const GNode& n = E.nodes_[i];
                for (auto& s : n.in) if (!s.empty()) { auto& u = uses[s]; ++u.first; u.second = i; }
                if (!n.residual.empty()) { auto& u = uses[n.residual]; ++u.first; u.second = i; }
            }
            for (int i = 0; i < (int)E.nodes_.size(); ++i) {
                const GNode& n = E.nodes_[i];
                if ((n.op != "Resize" && n.op != "ConvTranspose") || n.out.empty() || n.in.empty()) continue;
                auto u = uses.find(n.out[0]);
                if (u == uses.end() || u->second.first != 1) continue;
                if (std::find(E.output_names_.begin(), E.output_names_.end(), n.out[0]) != E.output_names_.end()) continue;
                sole_consumer[n.out[0]] = u->second.second;
                int& l = lu[n.in[0]];
                l = std::max(l, u->second.second);
            }
        }
        concat_consumer.clear();
        {
            std::map<std::string, std::pair<int, int>> uses;
            for (int i = 0; i < (int)E.nodes_.size(); ++i) {
                const GNode& n = E.nodes_[i];
                for (auto& s : n.in) if (!s.empty()) { auto& u = uses[s]; ++u.first; u.second = i; }
                if (!n.residual.empty()) { auto& u = uses[n.residual]; ++u.first; u.second = i; }
            }
            for (int i = 0; i < (int)E.nodes_.size(); ++i) {
                const GNode& n = E.nodes_[i];
                if (n.op != "Concat" || n.out.empty() || n.in.size() < 3) continue;
                auto u = uses.find(n.out[0]);
                if (u == uses.end() || u->second.first != 1) continue;
                if (std::find(E.output_names_.begin(), E.output_names_.end(), n.out[0]) != E.output_names_.end()) continue;
                const GNode& cn = E.nodes_[u->second.second];
                if (cn.op != "Conv" || cn.in.empty() || cn.in[0] != n.out[0]) continue;
                concat_consumer[n.out[0]] = u->second.second;
                for (auto& sname : n.in) { int& l = lu[sname]; l = std::max(l, u->second.second); }   // the sources live until the convolution that reads them
            }
        }
        // an Add whose LayerNormalization may take it over (rewrite pass 10): the fused launch reads the Add's operands while it writes the LayerNorm's output,
        // so they stay allocated through the LayerNormalization node -- its output can never be placed in their bytes
        for (int i = 1; i < (int)E.nodes_.size(); ++i) {
            if (E.nodes_[i].op != "LayerNormalization" || E.nodes_[i].ai("after_add", 0) == 0) continue;
            if (E.nodes_[i - 1].residual.empty()) for (auto& s : E.nodes_[i - 1].in) if (!s.empty()) { int& l = lu[s]; l = std::max(l, i); }
            if (!E.nodes_[i - 1].residual.empty()) { int& l = lu[E.nodes_[i - 1].residual]; l = std::max(l, i); }
        }
        for (int i = (int)E.nodes_.size() - 1; i >= 0; --i) {
            const GNode& n = E.nodes_[i];
            if (!alias_ops.count(n.op) || n.in.empty()) continue;
            int m = lu.count(n.in[0]) ? lu[n.in[0]] : i;
            for (auto& o : n.out) if (lu.count(o)) m = std::max(m, lu[o]);
            lu[n.in[0]] = m;
        }
        last_use = lu;
    }

    // Liveness invariant, checked at plan time (plans are cached per shape): bytes handed back to the arena hold no value that a later node (or the caller, for
    // a graph output) still reads, and every arena value produced since the last release that is read later sits in a root that stays booked -- not in a
    // per-node temp and not in the bytes of an internal temporary whose name compute_last_use() does not know (the "out::sm" / "out::kept" class of defect).
    int read_after(const std::string& v) const { auto it = last_use.find(v); return it == last_use.end() ? -1 : it->second; }
    std::string node_desc(int i) const {
        const GNode& g = E.nodes_[(size_t)i];
        return "node " + std::to_string(i) + " (" + g.op + " -> " + (g.out.empty() ? std::string("?") : g.out[0]) + ")";
    }
    int checked_upto = -1;   // nodes whose outputs check_release has seen
    void check_release(const std::vector<std::string>& dead, int i) {
        for (auto& d : dead) {
            auto al = root_aliases.find(d);
            if (al == root_aliases.end()) continue;
            for (auto& v : al->second) {
                auto vi = vals.find(v);
                if (vi == vals.end() || vi->second.root != d || vi->second.loc.kind != Loc::ARENA) continue;
                const int r = read_after(v);
                OAR_CHECK(r <= i, OAR_INTERNAL, "plan liveness: " + node_desc(i) + " frees root '" + d + "' but '" + v + "' lives in it and is read " +
                          (r >= (1 << 30) ? std::string("as a graph output") : "at node " + std::to_string(r)));
            }
        }
        for (int j = checked_upto + 1; j <= i; ++j) {
            for (auto& o : E.nodes_[(size_t)j].out) {
                auto vi = vals.find(o);
                if (vi == vals.end() || vi->second.loc.kind != Loc::ARENA || read_after(o) <= i) continue;
                const std::string& rt = vi->second.root;
                OAR_CHECK(!rt.empty() && root_bytes.count(rt), OAR_INTERNAL, "plan liveness: '" + o + "' of " + node_desc(j) + " is read after " + node_desc(i) +
                          (rt.empty() ? std::string(" but lives in a per-node temp") : " but its root '" + rt + "' is not booked"));
            }
        }
        checked_upto = i;
    }
    void release_dead(int i) {
        for (auto& t : temps) arena.release(t.first, t.second);
        temps.clear();
        std::vector<std::string> dead;
        for (auto& rb : root_bytes) {
            auto it = last_use.find(rb.first);
            int lu = it == last_use.end() ? i : it->second;
            if (lu <= i) dead.push_back(rb.first);
        }
        for (auto& d : dead) { arena.release(root_off[d], root_bytes[d]); root_bytes.erase(d); root_off.erase(d); }
        check_release(dead, i);
        for (auto& d : dead) root_aliases.erase(d);
    }

    bool skip_final_softmax = false;
    std::set<int> fused_into_prev;   // node indices whose work was planned by their predecessor
    bool stem_u8 = false;
    void build(const std::vector<int64_t>& in_dims, bool in_clast, const std::vector<std::vector<int64_t>>* extra_dims) {
        compute_last_use();
        TInfo in;
        in.u8_stem = stem_u8;
        in.dims = in_dims;
        in.layout = (in_clast && in_dims.size() >= 3) ? Layout::CLAST : Layout::NATIVE;
        in.loc.kind = Loc::INPUT;
        in.root = "";
        vals[E.input_name_] = in;
        for (size_t i = 1; extra_dims && i < extra_dims->size() && i < E.input_infos_.size(); ++i) {
            TInfo ex;
            ex.dims = (*extra_dims)[i];
            ex.layout = Layout::NATIVE;
            ex.loc.kind = Loc::EXTRA;
            ex.loc.idx = (int)i;
            ex.root = "";
            vals[E.input_infos_[i].name] = ex;
        }
        for (int i = 0; i < (int)E.nodes_.size(); ++i) {
            const GNode& n = E.nodes_[i];
            cur = i;
            if (last_add.node != i - 1) last_add = AddRec();   // only the node directly in front may hand its Add to a LayerNormalization: nothing older survives
            if (fused_into_prev.count(i)) { release_dead(i); continue; }   // planned together with the node before it (op_dsblock: two blocks, one launch)
            if (skip_final_softmax && n.op == "Softmax" && !n.out.empty() && n.out[0] == E.output_names_[0]) {
                TInfo x = get(n.in[0]);
                int r = (int)x.dims.size();
                int64_t axis = n.ai("axis", -1);
                if (axis < 0) axis += r;
                if (E_opset13() && axis == r - 1 && x.layout == Layout::NATIVE) {
                    alias_out(n.out[0], x, x.dims, Layout::NATIVE);
                    adopt_root(n.out[0], x.root);   // the output is a view of the logits: it takes their booking over, they live until the caller reads it
                    P.skipped_softmax = true;
                    release_dead(i);
                    continue;
                }
            }
            dispatch(n);
            if (!chain_run_open()) release_dead(i);   // an open run of chainable operators keeps its tensors (see ChainRec)
        }
        for (size_t oi = 0; oi < E.output_names_.size(); ++oi) {
            const std::string& on = E.output_names_[oi];
            auto it = vals.find(on);
            OAR_CHECK(it != vals.end(), OAR_MODEL_LOAD, "graph output '" + on + "' was never produced");
            TInfo t = it->second;
            PlanOutput po;
            po.name = on; po.dims = t.dims;
            const int declared = oi < E.output_infos_.size() ? E.output_infos_[oi].elem_type : 0;
            if (t.host_int) {   // known at plan time (Shape and friends): TensorOutput::I64 unless the value is a float
                po.on_host = true;
                po.dtype = t.host_f ? 1 : 7;
                if (t.host_f) po.host_vals = t.hd;
                else po.host_vals.assign(t.hv.begin(), t.hv.end());
                OAR_CHECK((int64_t)po.host_vals.size() == numel(t.dims), OAR_INTERNAL, "host output '" + on + "': value / shape mismatch");
                P.outputs.push_back(po);
                continue;
            }
            po.dtype = (t.is_int || declared == 7 || declared == 6) ? 7 : 1;
            // (the layout conversions below allocate arena bytes: an output whose root was released could be overwritten by the next output's)
            OAR_CHECK(t.loc.kind != Loc::ARENA || (!t.root.empty() && root_bytes.count(t.root)), OAR_INTERNAL,
                      "plan liveness: graph output '" + on + "' lives in " + (t.root.empty() ? std::string("a per-node temp") : "root '" + t.root + "', which was released"));
            if (t.layout == Layout::CLAST) { po.has_clast = true; po.loc_clast = t.loc; }
            Loc nat = to_native_loc(t);
            if (nat.kind == Loc::ARENA && nat.off != t.loc.off) {
                // keep the converted copy alive: move it out of the temp list
                for (auto it2 = temps.begin(); it2 != temps.end(); ++it2)
                    if ((int64_t)it2->first == nat.off) { temps.erase(it2); break; }
            }
            po.loc = nat;
            P.outputs.push_back(po);
        }
        P.arena_bytes = std::max<size_t>(P.arena_bytes, 256);
        fuse_chains();
    }

    // data inputs of the operators that only exist on the device (their other inputs are plan-time parameters: shapes, axes, pads, K)
    static const std::vector<int>* device_data_inputs(const std::string& op) {
        static const std::vector<int> first{0}, both{0, 1};
        const OpRow* r = find_op(op);
        return !r ? nullptr : r->host_inputs == HostInputs::DATA0 ? &first : r->host_inputs == HostInputs::DATA01 ? &both : nullptr;
    }
    static bool reads_host_values(const std::string& op) {
        const OpRow* r = find_op(op);
        return r && r->host_inputs == HostInputs::READS_HOST;
    }
    std::string device_shadow(const std::string& name) {
        const std::string sn = name + "::dev";
        if (!vals.count(sn)) {
            const TInfo& t = get(name);
            TInfo d;
            d.dims = t.dims; d.layout = Layout::NATIVE; d.root = ""; d.is_int = !t.host_f;
            d.loc = host_to_device(name, t);
            vals[sn] = d;
        }
        return sn;
    }

    void dispatch(const GNode& n) {
        const std::string& op = n.op;
        // shape / kind of an input without forcing a deferred Resize to run (its consumer decides that)
        auto info = [&](const std::string& s) -> const TInfo& { return (peek_pending(s) || pending_convt.count(s) || pending_concat.count(s)) ? vals.find(s)->second : get(s); };
        bool host_inputs = !n.in.empty();
        for (auto& s : n.in) if (!s.empty()) host_inputs = host_inputs && info(s).host_int;
        if (op == "Shape") {
            const TInfo& x = get(n.in[0]);
            TInfo o; o.host_int = true; o.hv = x.dims; o.dims = {(int64_t)x.dims.size()};
            vals[n.out[0]] = o; return;
        }
        // shape arithmetic: every input is a host value or a small constant, and at least one really is a host value
        bool evaluable = !n.in.empty(), any_host = false;
        for (auto& s : n.in) if (!s.empty()) { const TInfo& t = info(s); evaluable = evaluable && host_evaluable(t); any_host = any_host || t.host_int; }
        if (evaluable && (any_host || op == "Range") && op_host(n)) return;
        (void)host_inputs;
        // A plan-time value that reaches an operator which exists only as a kernel has no device bytes (Loc::NONE: RunCtx::at gives nullptr for it): it is uploaded once as
        // an f32 constant and the operator planned on that.  Operators that read host values themselves (the binary family, Where, the views, Gather, Concat, ...) are not listed.
        if (const std::vector<int>* di = device_data_inputs(op)) {
            GNode m;
            bool any = false;
            for (int i : *di)
                if (has_input(n, (size_t)i) && info(n.in[(size_t)i]).host_int) { if (!any) { m = n; any = true; } m.in[(size_t)i] = device_shadow(n.in[(size_t)i]); }
            if (any) return dispatch(m);
        } else if (!reads_host_values(op) && !n.in.empty() && !n.in[0].empty()) {
            OAR_CHECK(!info(n.in[0]).host_int, OAR_UNSUPPORTED_OP, "plan-time value '" + n.in[0] + "' feeds the device operator " + node_label());
        }
        // every stored input has a place to be read from (the captured Loc of a step cannot be inspected afterwards: this is where it is known)
        for (auto& s : n.in) {
            if (s.empty() || peek_pending(s) || pending_convt.count(s) || pending_concat.count(s)) continue;
            const TInfo& t = info(s);
            OAR_CHECK(t.host_int || t.loc.kind != Loc::NONE, OAR_INTERNAL, "planner: input '" + s + "' of " + node_label() + " has no storage");
        }
        const OpRow* row = find_op(op);
        if (row && row->plan) { row_code = row->code; return (this->*row->plan)(n); }
        fail(OAR_UNSUPPORTED_OP, "operator '" + op + "' is not implemented (node output " + (n.out.empty() ? "?" : n.out[0]) + ")");
    }

    // ------------------------------------------------------------------ handlers of the operator table that have no op_* of their own above
    void op_unary_act(const GNode& n) { op_unary(n, act_of(n)); }
    int row_code = 0;   // the `code` of the row dispatch() is calling through
    void op_binary_code(const GNode& n) { op_binary(n, row_code); }
    void op_reduce_code(const GNode& n) { op_reduce(n, row_code); }
    void op_argmax(const GNode& n) { op_argreduce(n, false); }
    void op_argmin(const GNode& n) { op_argreduce(n, true); }
    void op_average_pool(const GNode& n) { op_pool(n, false); }
    void op_max_pool(const GNode& n) { op_pool(n, true); }
    void op_conv_transpose(const GNode& n) { op_convt(n); }
    void op_linear_node(const GNode& n) { op_linear(n, false); }
    void op_gemm(const GNode& n) { op_linear(n, true); }
    void op_clip(const GNode& n) {
        // an absent bound is no bound: from opset 11 on (bounds as inputs) +-inf pass through; the attribute form (opset 6) defaults to +-FLT_MAX by its own text
        const float none = (opset >= 11 || opset == 0) ? INFINITY : 3.402823466e38f;
        Act a; a.kind = k::ACT_CLIP; a.alpha = n.af("min", -none); a.beta = n.af("max", none);
        if (has_input(n, 1)) { const TInfo& t = get(n.in[1]); OAR_CHECK(t.ht, OAR_UNSUPPORTED_OP, "Clip: dynamic min"); a.alpha = t.ht->f[0]; }
        if (has_input(n, 2)) { const TInfo& t = get(n.in[2]); OAR_CHECK(t.ht, OAR_UNSUPPORTED_OP, "Clip: dynamic max"); a.beta = t.ht->f[0]; }
        return op_unary(n, a);
    }
    void op_identity(const GNode& n) { const TInfo& x = get(n.in[0]); if (x.host_int) { vals[n.out[0]] = x; } else { TInfo xx = x; alias_out(n.out[0], xx, xx.dims, xx.layout); } return; }
    void op_cast(const GNode& n) {   // device tensors are f32 whatever they are called: float <-> bool casts of 0/1 masks are aliases
        const TInfo& x = get(n.in[0]);
        const int64_t to = n.ai("to", 1);
        OAR_CHECK(to == 1 || to == 9 || to == 10 || to == 11 || x.is_int, OAR_UNSUPPORTED_OP, "Cast of a device tensor to an integer type");
        bool mask = x.is01;
        if (to == 9 && !mask && x.ht) { mask = true; for (float v : x.ht->f) mask = mask && (v == 1.0f || (v == 0.0f && !std::signbit(v))); }   // (-0.0 would come back as -0.0)
        if (to == 9 && !mask) {   // any other float: bool(x) is x != 0, one launch of the flat binary kernel as Or(x, x)
            const TInfo xx = x;
            TInfo& y = new_out(n.out[0], xx.dims, xx.layout);
            y.is01 = true;
            const Loc xl = xx.loc, yl = y.loc;
            const int64_t cnt = numel(xx.dims);
            const std::vector<int64_t> d{cnt}, st{1};
            step([=](const RunCtx& c) { k::binary(c.s, c.at(xl), c.at(xl), c.mut(yl), 12, 1, d.data(), st.data(), st.data(), Act()); }, (double)cnt, 8.0 * cnt);
            return;
        }
        TInfo xx = x;
        TInfo& y = alias_out(n.out[0], xx, xx.dims, xx.layout);
        y.is_int = x.is_int && !(to == 1 || to == 10 || to == 11);   // (a float Cast of an index tensor is a float tensor: views keep the mark now)
        y.is01 = mask;
        return;
    }
};

// ---- the operator table: one row per operator name the engine knows, sorted by name (find_op searches it).
//   pub          the name may stand in a model file: Engine::supported_ops() is the rows that have it.  The other names are made by the load-time rewrites only.
//   host_inputs  what dispatch() does where an input's value is known at plan time (TInfo::host_int) and so has no device bytes:
//                  DATA0, DATA01  the operator exists only as a kernel: data input 0 / inputs 0 and 1 are uploaded once (device_shadow); its other inputs are
//                                 plan-time parameters (shapes, axes, pads, K)
//                  READS_HOST     the operator reads host values itself (the binary family, Where, the views, Gather, Concat, ...)
//                  NONE           neither: a plan-time value in input 0 is refused
//   plan         the planner's handler.  Null: the name never reaches a handler -- Constant, Dropout and Loop leave the graph at load time, Shape is dispatch()'s
//                first case and Range exists only as a plan-time evaluation (op_host)
//   code         what op_binary_code / op_reduce_code hand on: k::binary's operator, k::reduce_lastdim's mode
// A new operator is one row here (and, for a unary activation, its case in act_of).  The rows live inside a host function: a table at namespace scope would be
// emitted for the device too, where the handlers do not exist.
static const OpRow* op_table(size_t& count) {
    constexpr HostInputs NONE = HostInputs::NONE, DATA0 = HostInputs::DATA0, DATA01 = HostInputs::DATA01, READS_HOST = HostInputs::READS_HOST;
    static const OpRow rows[] = {
        {"Abs",                 true,  DATA0,      &Planner::op_unary_act},
        {"Add",                 true,  READS_HOST, &Planner::op_binary_code, 0},
        {"And",                 true,  READS_HOST, &Planner::op_binary_code, 11},
        {"ArgMax",              true,  DATA0,      &Planner::op_argmax},
        {"ArgMin",              true,  DATA0,      &Planner::op_argmin},
        {"Attention",           false, NONE,       &Planner::op_attention},
        {"AveragePool",         true,  DATA0,      &Planner::op_average_pool},
        {"BatchNormalization",  true,  NONE,       &Planner::op_bn},
        {"Cast",                true,  READS_HOST, &Planner::op_cast},
        {"Ceil",                true,  DATA0,      &Planner::op_unary_act},
        {"Clip",                true,  DATA0,      &Planner::op_clip},
        {"Concat",              true,  READS_HOST, &Planner::op_concat},
        {"Constant",            true,  NONE,       nullptr},
        {"ConstantOfShape",     true,  READS_HOST, &Planner::op_constant_of_shape},
        {"Conv",                true,  NONE,       &Planner::op_conv},
        {"ConvTranspose",       true,  NONE,       &Planner::op_conv_transpose},
        {"DSBlock",             false, NONE,       &Planner::op_dsblock},
        {"DeformableAttention", false, NONE,       &Planner::op_deformable_attention},
        {"Div",                 true,  READS_HOST, &Planner::op_binary_code, 3},
        {"Dropout",             true,  NONE,       nullptr},
        {"Equal",               true,  READS_HOST, &Planner::op_binary_code, 8},
        {"Erf",                 true,  DATA0,      &Planner::op_unary_act},
        {"Exp",                 true,  DATA0,      &Planner::op_unary_act},
        {"Expand",              true,  DATA0,      &Planner::op_expand},
        {"Flatten",             true,  DATA0,      &Planner::op_flatten},
        {"Floor",               true,  DATA0,      &Planner::op_unary_act},
        {"FormulaDecode",       false, READS_HOST, &Planner::op_formula_decode},
        {"Gather",              true,  READS_HOST, &Planner::op_gather},
        {"GatherElements",      true,  READS_HOST, &Planner::op_gather_elements},
        {"GatherND",            true,  READS_HOST, &Planner::op_gather_nd},
        {"Gelu",                true,  DATA0,      &Planner::op_unary_act},
        {"Gemm",                true,  DATA0,      &Planner::op_gemm},
        {"GlobalAveragePool",   true,  DATA0,      &Planner::op_gap},
        {"Greater",             true,  READS_HOST, &Planner::op_binary_code, 10},
        {"GridSample",          true,  DATA01,     &Planner::op_grid_sample},
        {"HardSigmoid",         true,  DATA0,      &Planner::op_unary_act},
        {"HardSwish",           true,  DATA0,      &Planner::op_unary_act},
        {"Identity",            true,  READS_HOST, &Planner::op_identity},
        {"LayerNormalization",  true,  DATA0,      &Planner::op_layernorm},
        {"LeakyRelu",           true,  DATA0,      &Planner::op_unary_act},
        {"Less",                true,  READS_HOST, &Planner::op_binary_code, 9},
        {"Linear",              false, DATA0,      &Planner::op_linear_node},
        {"Log",                 true,  DATA0,      &Planner::op_unary_act},
        {"Loop",                true,  NONE,       nullptr},
        {"MatMul",              true,  DATA01,     &Planner::op_matmul},
        {"Max",                 true,  READS_HOST, &Planner::op_binary_code, 6},
        {"MaxPool",             true,  DATA0,      &Planner::op_max_pool},
        {"Min",                 true,  READS_HOST, &Planner::op_binary_code, 7},
        {"Mul",                 true,  READS_HOST, &Planner::op_binary_code, 2},
        {"MultiHeadAttention",  false, NONE,       &Planner::op_mha_attention},
        {"Neg",                 true,  DATA0,      &Planner::op_unary_act},
        {"Not",                 true,  DATA0,      &Planner::op_unary_act},
        {"Or",                  true,  READS_HOST, &Planner::op_binary_code, 12},
        {"PRelu",               true,  READS_HOST, &Planner::op_binary_code, 5},
        {"Pad",                 true,  DATA0,      &Planner::op_pad},
        {"Pow",                 true,  READS_HOST, &Planner::op_binary_code, 4},
        {"Range",               true,  READS_HOST, nullptr},
        {"Reciprocal",          true,  DATA0,      &Planner::op_unary_act},
        {"ReduceMax",           true,  DATA0,      &Planner::op_reduce_code, 2},
        {"ReduceMean",          true,  DATA0,      &Planner::op_reduce_code, 0},
        {"ReduceMin",           true,  DATA0,      &Planner::op_reduce_code, 3},
        {"ReduceProd",          true,  DATA0,      &Planner::op_reduce_code, 4},
        {"ReduceSum",           true,  DATA0,      &Planner::op_reduce_code, 1},
        {"RelPosAttention",     false, NONE,       &Planner::op_relpos_attention},
        {"Relu",                true,  DATA0,      &Planner::op_unary_act},
        {"Reshape",             true,  READS_HOST, &Planner::op_reshape},
        {"Resize",              true,  DATA0,      &Planner::op_resize},
        {"Round",               true,  DATA0,      &Planner::op_unary_act},
        {"SEGate",              false, NONE,       &Planner::op_se_gate},
        {"SLADecode",           false, READS_HOST, &Planner::op_sla_decode},
        {"Shape",               true,  READS_HOST, nullptr},
        {"Sigmoid",             true,  DATA0,      &Planner::op_unary_act},
        {"Slice",               true,  READS_HOST, &Planner::op_slice},
        {"Softmax",             true,  DATA0,      &Planner::op_softmax},
        {"Softplus",            true,  DATA0,      &Planner::op_unary_act},
        {"Split",               true,  DATA0,      &Planner::op_split},
        {"Sqrt",                true,  DATA0,      &Planner::op_unary_act},
        {"Squeeze",             true,  READS_HOST, &Planner::op_squeeze},
        {"Sub",                 true,  READS_HOST, &Planner::op_binary_code, 1},
        {"Tanh",                true,  DATA0,      &Planner::op_unary_act},
        {"Tile",                true,  DATA0,      &Planner::op_tile},
        {"TopK",                true,  DATA0,      &Planner::op_topk},
        {"Transpose",           true,  DATA0,      &Planner::op_transpose},
        {"Unsqueeze",           true,  READS_HOST, &Planner::op_unsqueeze},
        {"Where",               true,  READS_HOST, &Planner::op_where},
        {"WindowAttention",     false, NONE,       &Planner::op_window_attention},
    };
    count = sizeof(rows) / sizeof(rows[0]);
    static const bool sorted = [&] {   // checked once, at the first look-up: find_op searches by name
        OAR_CHECK(std::is_sorted(rows, rows + count, [](const OpRow& a, const OpRow& b) { return std::strcmp(a.name, b.name) < 0; }), OAR_INTERNAL,
                  "the operator table is not sorted by name");
        return true;
    }();
    (void)sorted;
    return rows;
}

static const OpRow* find_op(const std::string& name) {
    size_t count = 0;
    const OpRow* rows = op_table(count);
    const OpRow* r = std::lower_bound(rows, rows + count, name, [](const OpRow& a, const std::string& b) { return b.compare(a.name) > 0; });
    return r != rows + count && name == r->name ? r : nullptr;
}

std::vector<float> igemm_to_fragments(int fmt, const std::vector<float>& w, int64_t rows, int64_t K) { return Planner::to_fragments(fmt, w, rows, K); }

// Host-only structural checks of the initializers the load-time rewrites and the planner index by their DECLARED dims
// (a malformed file must end in OAR_MODEL_LOAD, not in an out-of-bounds read).
void Engine::validate_model(const OnnxModel& m) {
    auto init = [&](const std::string& name) -> const HostTensor* {
        auto it = m.initializers.find(name);
        return it == m.initializers.end() ? nullptr : &it->second;
    };
    auto in = [&](const OnnxNode& n, size_t i) -> const HostTensor* { return i < n.inputs.size() && !n.inputs[i].empty() ? init(n.inputs[i]) : nullptr; };
    for (const OnnxNode& n : m.nodes) {
        const std::string at = " (node output " + (n.outputs.empty() ? std::string("?") : n.outputs[0]) + ")";
        OAR_CHECK(!n.outputs.empty(), OAR_MODEL_LOAD, "onnx: node '" + n.op + "' without outputs");
        if (n.op == "Conv" || n.op == "ConvTranspose") {
            OAR_CHECK(n.inputs.size() >= 2, OAR_MODEL_LOAD, n.op + ": needs at least 2 inputs" + at);
            if (const HostTensor* w = in(n, 1)) {
                OAR_CHECK(w->dtype == DType::F32 && w->dims.size() == 4, OAR_MODEL_LOAD, n.op + ": weight must be a rank-4 f32 tensor" + at);
                for (int64_t d : w->dims) OAR_CHECK(d > 0, OAR_MODEL_LOAD, n.op + ": weight has an empty dimension" + at);
                if (const HostTensor* b = in(n, 2)) {
                    const int64_t cout = n.op == "Conv" ? w->dims[0] : w->dims[1] * n.ai("group", 1);
                    OAR_CHECK(b->dtype == DType::F32 && (int64_t)b->f.size() == cout, OAR_MODEL_LOAD, n.op + ": bias must hold Cout f32 values" + at);
                }
            }
        } else if (n.op == "BatchNormalization") {
            OAR_CHECK(n.inputs.size() >= 5, OAR_MODEL_LOAD, "BatchNormalization: needs 5 inputs" + at);
            int64_t c = -1;
            for (size_t i = 1; i < 5; ++i)
                if (const HostTensor* t = in(n, i)) {
                    OAR_CHECK(t->dtype == DType::F32 && !t->f.empty(), OAR_MODEL_LOAD, "BatchNormalization: parameters must be non-empty f32 tensors" + at);
                    if (c < 0) c = (int64_t)t->f.size();
                    OAR_CHECK((int64_t)t->f.size() == c, OAR_MODEL_LOAD, "BatchNormalization: scale / bias / mean / var differ in length" + at);
                }
        } else if (n.op == "Gemm" || n.op == "MatMul") {
            OAR_CHECK(n.inputs.size() >= 2, OAR_MODEL_LOAD, n.op + ": needs 2 inputs" + at);
            if (const HostTensor* b = in(n, 1)) {
                OAR_CHECK(b->dtype == DType::F32 && b->dims.size() >= 1, OAR_MODEL_LOAD, n.op + ": constant B must be an f32 tensor" + at);
                if (n.op == "Gemm") OAR_CHECK(b->dims.size() == 2, OAR_MODEL_LOAD, "Gemm: B must be rank 2" + at);
            }
        } else if (n.op == "PRelu" || n.op == "LayerNormalization") {
            OAR_CHECK(n.inputs.size() >= 2, OAR_MODEL_LOAD, n.op + ": needs 2 inputs" + at);
        }
    }
}

// every operator name a model file may hold: the public rows of the operator table -- oar_onnx_inspect reports the rest
// (Loop: the SLA decode step and the formula decode step only, see match_sla_loop / match_formula_loop)
const std::set<std::string>& Engine::supported_ops() {
    static const std::set<std::string> ops = [] {
        std::set<std::string> s;
        size_t count = 0;
        const OpRow* rows = op_table(count);
        for (size_t i = 0; i < count; ++i) if (rows[i].pub) s.insert(rows[i].name);
        return s;
    }();
    return ops;
}

const Plan& Engine::plan_for(const std::vector<int64_t>& dims, bool in_clast, bool skip_final_softmax,
                             const std::vector<std::vector<int64_t>>* extra_dims, bool stem_u8) {
    std::ostringstream key;
    key << (in_clast ? "L" : "N") << (skip_final_softmax ? "S" : "") << (stem_u8 ? "U" : "");
    for (auto d : dims) key << "x" << d;
    for (size_t i = 1; extra_dims && i < extra_dims->size(); ++i) {
        key << "|";
        for (auto d : (*extra_dims)[i]) key << "x" << d;
    }
    auto it = plans_.find(key.str());
    if (it != plans_.end()) { it->second->last_used = ++tick_; last_returned_ = it->second.get(); return *it->second; }
    OAR_HIP(hipSetDevice(device_));
    std::unique_ptr<Plan> p(new Plan());
    Planner pl(*this, *p);
    pl.skip_final_softmax = skip_final_softmax;
    pl.stem_u8 = stem_u8;
    pl.build(dims, in_clast, extra_dims);
    evict_plans();
    p->last_used = ++tick_;
    const Plan& ref = *p;
    plans_[key.str()] = std::move(p);
    last_returned_ = &ref;
    return ref;
}

// The plan cache is keyed on exact input dims (every (batch, Wt) pair of the recognizer, every (sub-batch, rh, rw) of the
// detector), so a long-running server on heterogeneous pages would grow it without bound: keep at most plan_cap_ plans,
// least-recently-used out first.  The plan returned by the PREVIOUS plan_for / run call is never the victim, so a `const
// Plan&` stays valid across one further call on the same engine (callers copy what they need before that).
void Engine::evict_plans() {
    while (plans_.size() >= plan_cap_) {
        auto victim = plans_.end();
        for (auto it = plans_.begin(); it != plans_.end(); ++it) {
            if (it->second.get() == last_returned_) continue;
            if (victim == plans_.end() || it->second->last_used < victim->second->last_used) victim = it;
        }
        if (victim == plans_.end()) return;
        const Plan* dead = victim->second.get();
        bool synced = false;
        for (auto g = graphs_.begin(); g != graphs_.end();) {   // captured graphs of the evicted plan go with it
            if (std::get<0>(g->first) != dead) { ++g; continue; }
            if (!synced) { OAR_HIP(hipStreamSynchronize(stream_)); synced = true; }
            if (g->second.events) Profiler::get().release(*g->second.events);
            if (g->second.exec) (void)hipGraphExecDestroy(g->second.exec);
            g = graphs_.erase(g);
        }
        plans_.erase(victim);
        ++plans_evicted_;
    }
}

void Engine::set_decode_stop(int64_t token) {
    int64_t V = -1;
    for (const GNode& n : nodes_) if (n.op == "FormulaDecode") { V = n.ai("vocab", 0); break; }
    OAR_CHECK(V >= 0, OAR_INVALID_INPUT, "set_decode_stop: the graph has no FormulaDecode node (no greedy decode Loop was recognised)");
    OAR_CHECK(token < V, OAR_INVALID_INPUT, "set_decode_stop: token " + std::to_string(token) + " is outside the decode node's vocabulary (V = " + std::to_string(V) + ")");
    const int tok = token < 0 ? -1 : (int)token;
    if (tok == fd_.token) return;
    OAR_HIP(hipSetDevice(device_));
    OAR_HIP(hipStreamSynchronize(stream_));
    clear_graphs();   // their kernel arguments hold the old setting
    if (tok >= 0 && !fd_.state) {   // everything goes into locals and is committed at the end: a failure half way leaves the engine as it was
        void *d = nullptr, *fin = nullptr, *fin_dev = nullptr, *exe = nullptr;
        hipEvent_t ev[k::kFdLookahead + 1] = {};
        try {
            OAR_HIP(hipMalloc(&d, sizeof(k::FdStopState)));
            OAR_HIP(hipMemset(d, 0, sizeof(k::FdStopState)));
            OAR_HIP(hipHostMalloc(&fin, 64, hipHostMallocMapped | hipHostMallocCoherent));
            std::memset(fin, 0, 64);
            OAR_HIP(hipHostGetDevicePointer(&fin_dev, fin, 0));
            OAR_HIP(hipHostMalloc(&exe, 64, hipHostMallocDefault));
            std::memset(exe, 0, 64);
            for (hipEvent_t& e : ev) OAR_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        } catch (...) {
            for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
            if (exe) (void)hipHostFree(exe);
            if (fin) (void)hipHostFree(fin);
            if (d) (void)hipFree(d);
            throw;
        }
        fd_.fin = static_cast<volatile unsigned*>(fin);
        fd_.fin_dev = static_cast<unsigned*>(fin_dev);
        fd_executed_ = static_cast<unsigned long long*>(exe);
        for (int i = 0; i <= k::kFdLookahead; ++i) fd_.ev[i] = ev[i];
        fd_.state = static_cast<k::FdStopState*>(d);
    }
    fd_.token = tok;
}

Engine::DecodeStats Engine::decode_stats() {
    DecodeStats d;
    d.steps_limit = fd_stats_.steps_limit;
    d.steps_enqueued = fd_stats_.steps_enqueued;
    d.steps_executed = fd_stats_.steps_enqueued;
    if (d.steps_limit == 0) return d;
    d.lookahead = k::kFdLookahead;
    if (fd_executed_valid_) {
        OAR_HIP(hipSetDevice(device_));
        OAR_HIP(hipStreamSynchronize(stream_));
        d.steps_executed = (int64_t)*fd_executed_;
    }
    return d;
}

void Engine::begin_run() {
    fd_stats_ = k::FdRunStats{};
    fd_.first_chunk = true;
    fd_executed_valid_ = false;
}

// replayed: an existing graph was launched, so no step lambda ran and the plan's own figure stands in for the host's count (a replay enqueues every step)
void Engine::end_run(const Plan& p, bool replayed) {
    if (replayed && fd_stats_.steps_limit == 0) fd_stats_.steps_limit = fd_stats_.steps_enqueued = p.decode_steps;
    if (fd_.token >= 0 && p.decode_steps > 0) {   // read back with the outputs: the caller's fetch synchronises the stream
        OAR_HIP(hipMemcpyAsync(fd_executed_, &fd_.state->steps_executed, sizeof(unsigned long long), hipMemcpyDeviceToHost, stream_));
        fd_executed_valid_ = true;
    }
}

void Engine::clear_graphs() {
    for (auto& kv : graphs_) {
        if (kv.second.events) Profiler::get().release(*kv.second.events);
        if (kv.second.exec) (void)hipGraphExecDestroy(kv.second.exec);
    }
    graphs_.clear();
}

// Replays (capturing first if needed) the plan as a hipGraph.  Returns false when the plan has to be enqueued kernel by
// kernel (first run, graphs disabled, capture failed).
bool Engine::replay(const Plan& p, const RunCtx& c) {
    // Opt-in (OAR_HIP_GRAPH=1).  Measured on ROCm 7.2 / MI355X with bench.py: 22.8-22.9 ms per step with replay vs
    // 21.9-23.0 ms without.  The rocprofv3 kernel trace explains it: dependent kernels enqueued one by one already start
    // back to back (median gap 0.00 us), so a graph of kernel nodes has no dispatch gap left to remove; with external
    // event-record nodes (profiler on) replay is 6 % slower.
    if (!graphs_requested() || !graphs_ok_ || p.runs == 0) return false;
    Profiler& prof = Profiler::get();
    const auto key = std::make_tuple(&p, (const void*)c.input, (const void*)c.arena);
    auto it = graphs_.find(key);
    if (it != graphs_.end() && it->second.epoch != prof.epoch) {
        if (it->second.events) prof.release(*it->second.events);
        (void)hipGraphExecDestroy(it->second.exec);
        graphs_.erase(it);
        it = graphs_.end();
    }
    if (it == graphs_.end()) {
        if (graphs_.size() >= 64) { OAR_HIP(hipStreamSynchronize(stream_)); clear_graphs(); }
        GraphEntry ge;
        ge.events = std::make_shared<Profiler::GraphEvents>();
        ge.epoch = prof.epoch;
        if (hipStreamBeginCapture(stream_, hipStreamCaptureModeThreadLocal) != hipSuccess) { (void)hipGetLastError(); graphs_ok_ = false; return false; }
        Profiler::capturing = ge.events.get();
        hipGraph_t g = nullptr;
        bool ok = true;
        try {
            for (auto& st : p.steps) st(c);
        } catch (...) {
            ok = false;
        }
        Profiler::capturing = nullptr;
        if (hipStreamEndCapture(stream_, &g) != hipSuccess || !g) ok = false;
        if (ok && hipGraphInstantiate(&ge.exec, g, nullptr, nullptr, 0) != hipSuccess) ok = false;
        if (g) (void)hipGraphDestroy(g);
        if (!ok) {   // fall back to plain launches for the lifetime of this engine
            (void)hipGetLastError();
            prof.release(*ge.events);
            graphs_ok_ = false;
            return false;
        }
        {
            std::lock_guard<std::mutex> lk(prof.mu);
            prof.graphs.push_back(ge.events);
        }
        it = graphs_.emplace(key, ge).first;
    }
    GraphEntry& ge = it->second;
    if (ge.events->launched) prof.harvest(*ge.events);   // the replay below re-records the same events
    OAR_HIP(hipGraphLaunch(ge.exec, stream_));
    if (!ge.events->ev.empty()) ge.events->launched = true;
    return true;
}

const Plan& Engine::run(const float* d_in, const std::vector<int64_t>& dims, bool in_clast, bool skip_final_softmax) {
    const Plan& p = plan_for(dims, in_clast, skip_final_softmax);
    OAR_HIP(hipSetDevice(device_));
    if (arena_.cap < p.arena_bytes) {
        OAR_HIP(hipStreamSynchronize(stream_));
        clear_graphs();   // they bake the old arena base into their kernel arguments
        arena_.reserve(p.arena_bytes);
    }
    RunCtx c{stream_, d_in, arena_.as<char>()};
    last_input_ = d_in;
    begin_run();
    const bool replayed = replay(p, c);
    if (!replayed) {
        begin_run();   // (a capture that failed half way has already counted some steps)
        if (!p.step_ops.empty() && p.step_ops.size() == p.steps.size()) {   // OAR_DEBUG_STEPS=1 (and no chain fusion re-indexing): which step leaves a HIP error behind?
            for (size_t i = 0; i < p.steps.size(); ++i) {
                p.steps[i](c);
                const hipError_t e = hipGetLastError();
                if (e != hipSuccess) fail(OAR_DEVICE, "HIP error after step " + std::to_string(i) + " (" + p.step_ops[i] + "): " + hipGetErrorString(e));
            }
        } else {
            for (auto& st : p.steps) st(c);
        }
        ++p.runs;
    }
    end_run(p, replayed);
    OAR_HIP(hipGetLastError());
    return p;
}

const Plan& Engine::run_multi(const std::vector<const float*>& d_ins, const std::vector<std::vector<int64_t>>& dims) {
    OAR_CHECK(!d_ins.empty() && d_ins.size() == dims.size() && d_ins.size() == input_infos_.size(), OAR_INVALID_INPUT,
              "run_multi: one tensor per declared graph input is required");
    if (d_ins.size() == 1) return run(d_ins[0], dims[0], false);
    const Plan& p = plan_for(dims[0], false, false, &dims);
    OAR_HIP(hipSetDevice(device_));
    if (arena_.cap < p.arena_bytes) {
        OAR_HIP(hipStreamSynchronize(stream_));
        clear_graphs();
        arena_.reserve(p.arena_bytes);
    }
    last_extra_ = d_ins;
    RunCtx c{stream_, d_ins[0], arena_.as<char>(), last_extra_.data()};
    last_input_ = d_ins[0];
    begin_run();
    for (auto& st : p.steps) st(c);   // no hipGraph replay here: a captured graph bakes in one input pointer only
    end_run(p, false);
    ++p.runs;
    OAR_HIP(hipGetLastError());
    return p;
}

const Plan& Engine::run_stem(const k::StemU8& st, const std::vector<int64_t>& dims, bool skip_final_softmax) {
    OAR_CHECK(stem_fusable_, OAR_INTERNAL, "run_stem on a graph without a fusable RGB stem");
    OAR_CHECK(dims.size() == 4 && dims[1] == 3 && dims[0] >= 1 && (st.dev || dims[0] <= 32), OAR_INVALID_INPUT, "run_stem: dims must be {n, 3, H, W} (n <= 32 pages by value)");
    const Plan& p = plan_for(dims, true, skip_final_softmax, nullptr, true);
    OAR_HIP(hipSetDevice(device_));
    if (arena_.cap < p.arena_bytes) {
        OAR_HIP(hipStreamSynchronize(stream_));
        clear_graphs();
        arena_.reserve(p.arena_bytes);
    }
    RunCtx c{stream_, nullptr, arena_.as<char>(), nullptr, &st};
    last_input_ = nullptr;
    begin_run();
    for (auto& stp : p.steps) stp(c);   // no hipGraph replay: the page pointers change from call to call
    end_run(p, false);
    ++p.runs;
    OAR_HIP(hipGetLastError());
    return p;
}

const float* Engine::out_ptr(const Loc& l) const {
    RunCtx c{stream_, last_input_, arena_.as<char>(), last_extra_.empty() ? nullptr : last_extra_.data()};
    return c.at(l);
}

}  // namespace oar
