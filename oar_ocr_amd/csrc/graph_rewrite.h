// graph_rewrite.h -- everything that happens to a model before the first plan: ONNX nodes -> GNodes, the load-time rewrite passes (engine_rewrite.cc,
// Rewriter::run is the list of them, in order) and the two Loop matchers of pass 0 (engine_loops.cc).  Host-only: nothing here touches the device.
#pragma once
#include <cstdint>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "kernels.h"
#include "onnx_parse.h"

namespace oar {

struct GNode {  // graph node after load-time rewrites
    std::string op;
    std::vector<std::string> in, out;
    std::map<std::string, Attr> attrs;
    k::Act act;                 // fused activation
    std::string bias;           // fused bias initializer (Linear)
    std::string residual;       // fused residual input
    int id = 0;
    int64_t ai(const char* k, int64_t d) const { auto it = attrs.find(k); return it == attrs.end() ? d : it->second.i; }
    float af(const char* k, float d) const { auto it = attrs.find(k); return it == attrs.end() ? d : it->second.f; }
    std::string as(const char* k, const std::string& d) const { auto it = attrs.find(k); return it == attrs.end() ? d : it->second.s; }
    std::vector<int64_t> ais(const char* k) const { auto it = attrs.find(k); return it == attrs.end() ? std::vector<int64_t>{} : it->second.is; }
    bool has(const char* k) const { return attrs.count(k) != 0; }
};

struct RewrittenGraph {
    std::vector<GNode> nodes;                                  // ids assigned
    std::map<std::string, HostTensor> inits;                   // the file's, the Constant nodes', the rewrites' own
    std::map<std::string, std::vector<GNode>> ln_spelled;      // pass 2c
    bool fuse_add_ln = true;                                   // pass 10
};
RewrittenGraph rewrite_graph(OnnxModel& m);                    // no device; throws what the engine's constructor throws for the model
// what oar_onnx_rewrite prints: every node, initializer and ln_spelled entry of `g`, one per line (an inspection aid, the format may change)
std::string graph_listing(const RewrittenGraph& g);

// activations that may be folded into a conv / linear / add epilogue (apply_act).  The other unary activations (the rows of the operator table that
// op_unary_act plans) only ever run as a stand-alone element-wise kernel (apply_unary): every extra case in apply_act costs registers in each conv epilogue --
// with all of them in, the depthwise kernel lost a wave per SIMD and a quarter of its bandwidth.
bool is_fusable_act(const std::string& op);
k::Act act_of(const GNode& n);

inline int64_t numel(const std::vector<int64_t>& d) {
    int64_t n = 1;
    for (auto v : d) n *= v;
    return n;
}

// pass 0 (engine_loops.cc).  `inits` receives the fused operators' repacked constants; `graph_outs` are the names of the graph outputs.
// a Loop whose body is the SLA decode step -> Linear + SLADecode; throws OAR_UNSUPPORTED_OP otherwise
void match_sla_loop(const GNode& loop, std::map<std::string, HostTensor>& inits, int64_t opset, GNode& linear, GNode& decode);
// a Loop whose body is the greedy step of a transformer decoder with a key / value cache -> FormulaDecode; `dropped_inputs` receives the (empty) initial caches,
// which leave the graph; throws OAR_UNSUPPORTED_OP otherwise
void match_formula_loop(const GNode& loop, const std::vector<GNode>& outer_nodes, std::map<std::string, HostTensor>& inits, int64_t opset,
                        const std::set<std::string>& graph_outs, GNode& decode, std::vector<std::string>& dropped_inputs);

}  // namespace oar
