// kernels.h -- launchers for the gfx950 NN kernels (all activations f32, NHWC for rank-4 feature maps).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

namespace oar {
namespace k {

// ACT_RELU and NaN: the implicit-GEMM epilogue (igemm_dev.h) and apply_act (kernels_dev.h: element-wise kernel, row-streaming 3x3, large-kernel and direct
// convolutions) keep a NaN, as max(0, x) of the ONNX operator does -- tests/test_gpu_x6_accuracy.py pins that.  The fused dsblock kernels (dsblock*.inc) and the
// sample-local chain (chain.hip) apply their own `x > 0 ? x : 0` / fmaxf(x, 0), which make 0 of a NaN: whether a graph's Relu passes a NaN on therefore depends on
// the kernel the planner picks for its layer.  No result on finite values differs.
enum ActKind : int { ACT_NONE = 0, ACT_RELU, ACT_HSWISH, ACT_HSIGMOID, ACT_SIGMOID, ACT_SWISH, ACT_LEAKY, ACT_CLIP, ACT_TANH, ACT_GELU_ERF,
                     // element-wise math (decomposed GELU / LayerNorm exports, UVDoc)
                     ACT_ERF, ACT_SQRT, ACT_EXP, ACT_ABS, ACT_NEG, ACT_RECIP, ACT_LOG, ACT_GELU_TANH, ACT_SOFTPLUS, ACT_FLOOR, ACT_CEIL, ACT_ROUND, ACT_NOT };
struct Act {
    int kind = ACT_NONE;
    float alpha = 0.f, beta = 0.f;  // HardSigmoid(alpha,beta) / LeakyRelu(alpha) / Clip(alpha=min,beta=max)
};

struct ConvP {
    int N, H, W, Cin;       // input NHWC
    int Ho, Wo, Cout;       // output NHWC
    int kh, kw, sh, sw, pt, pl, dh, dw, groups;
    Act act;
    const float* x;
    const float* w;         // layout depends on the kernel (see each launcher)
    const float* bias;      // may be null
    const float* residual;  // may be null; same shape/ld as y
    float* y;
    int y_ld;               // channel stride of the output buffer (>= Cout); y points at channel offset already
    int convt2x2;           // igemm only: output scatter of a 2x2/stride-2 ConvTranspose (Cout is the real Cout)
    int w_fmt;              // igemm only: weight fragment layout, one of IGEMM_W_* (chosen by igemm_weight_format)
    float* ctc_part;        // igemm only, Linear feeding the fused CTC tail: softmax partials [rows][ctc_tiles()] float4
    int ctc_valid;          //   instead of logits (y is not written); ctc_valid = number of real classes
    const float* se;        // igemm only (bf16x6 weight-stationary 1x1): squeeze-excite gate [N][Cin] multiplied into the input on load
    int res_up;             // igemm only (f32 per-tile kernels): f > 1 => `residual` is [N][Ho / f][Wo / f][Cout], added through the nearest index map (h / f, w / f)
                            // -- the top-down sum of an FPN without materialising the upsampled tensor
    int n_msrc;             // igemm only, output-stationary bf16x6 kernel, 1x1 layers: > 0 => the input is the channel concat of n_msrc channels-last maps that was never
    const float* msrc[8];   //   materialised (PP-HGNetV2's 7-way aggregation): source i has msrc_c[i] channels (8 | msrc_c[i]) at msrc[i], pixel stride msrc_c[i];
    int msrc_c[8];          //   x is ignored, Cin = the sum
    int accum;              // igemm only, row-streaming 3x3 kernel: 1 = add to what y already holds (a later pass over a channel slice of the input, ConvP::x_ld)
    int x_ld;               // igemm only, output-stationary bf16x6 kernel / row-streaming 3x3 kernel: floats between two pixels of x when that is not Cin (0 = Cin): one group of a
                            // grouped convolution reads its Cin channels out of the full tensor
    float* gap_part;        // depthwise only (conv_dw_gap_tiles(p) > 0): per-tile sums of the activated output, [N][tiles][Cout] -- the squeeze of an
                            // SE block without a second read of the feature map (global_avgpool_finish reduces them)
};
enum : int { IGEMM_W_K16 = 0, IGEMM_W_X6 = 1, IGEMM_W_X6RS = 2, IGEMM_W_X6CS = 3 };   // X6CS: per-chunk weight blocks of dsblock_cs.inc (depthwise taps + bias + pointwise pieces)
//   // X6RS: the bf16x6 fragments of dsblock_rs.inc (k-step = two 16-channel chunks)

// Implicit-GEMM conv on the matrix cores. groups == 1, Cin % 4 == 0. Weight layouts (ConvP::w_fmt):
//   K16: f32 fragments  Wf[cout/16][K/16][lane][4 f32]              -> v_mfma_f32_16x16x4_f32 (exact f32 FMA chain)
//   X6 : bf16x6 fragments Wx[cout/16][K/32][3 planes][lane][8 bf16] -> v_mfma_f32_16x16x32_bf16 x 6 (f32-equivalent),
//        weight-stationary kernel only (wide 1x1 / Linear layers)
// Rows are padded to 64 couts, K to the chunk size, with zeros.
// prof_class: the profiler class of this launch instead of the kernel's own (null: `conv_igemm*` by kernel, as ever) -- a host that is not the engine names its Linears
void conv_igemm(hipStream_t s, const ConvP& p, const char* prof_class = nullptr);
// chosen per layer AND input shape at plan time: M = GEMM rows (pixels), N = couts
// same3x3_px: pixels of ONE image when the layer is a 3x3 / stride 1 / pad 1 / dilation 1 convolution without residual (0 otherwise): the row-streaming
// bf16x6 kernel of igemm_rs3_x6.hip takes such layers with <= 16 output channels
int igemm_weight_format(long M, int K, int N, bool is1x1, int Cin = 0, long same3x3_px = 0, bool lk_ok = false);
// may a 1x1 layer keep bf16x6 (IGEMM_W_X6) weights and still be launched with ANY row count?  Only where the weight-stationary bf16x6 kernel takes it (its LDS tile fits this K):
// the output-stationary kernel, which igemm_weight_format also answers IGEMM_W_X6 for, refuses small row counts
bool igemm_x6_serves_any_rows(int K, int N);
// lk_ok: conv_lk_x6_eligible said yes for this layer (large-kernel same convolution from an LDS-staged halo tile, igemm_lk_x6.hip)
bool conv_lk_x6_eligible(int kh, int kw, int sh, int sw, int pt, int pl, int dh, int dw, int H, int W, int Ho, int Wo, int Cin, int Cout, int y_ld, long M);
// one group of a grouped k x k convolution (ConvP::x_ld) as its own implicit GEMM on the output-stationary bf16x6 kernel: M pixels, K = kh * kw * Cin_g, N = Cout_g >= 32
bool conv_grouped_x6_ok(long M, int K, int N, int Cin);
// may a 1x1 layer of this shape read a never-materialised channel concat (ConvP::msrc)?  It then runs on the output-stationary bf16x6 kernel whatever its K
bool conv_msrc_ok(long M, int K, int N);
// a 3x3 / stride 1 / pad 1 convolution with <= 16 output channels and 96 ... 256 input channels as passes of the row-streaming bf16x6 kernel over 64- / 32-channel
// slices of the input (ConvP::x_ld, ConvP::accum): the slice widths, empty when the layer is not eligible.  img_px = pixels of one image
std::vector<int> conv3x3_n16_slices(long M, int Cin, int Cout, long img_px, int y_ld);
// may a 1x1 conv of this shape take ConvP::se (the gate of a squeeze-excite block folded into its input load)?  hw = pixels per image
bool conv_igemm_se_ok(long M, int K, int N, int hw);   // Cin: input channels of a k x k conv (0: treat as not eligible for the x6 path)
// Depthwise conv. w: [kh][kw][C]. C % 4 == 0.
void conv_dw(hipStream_t s, const ConvP& p);
// tiles per image of the variant conv_dw will launch for p when it can also emit ConvP::gap_part (0: it cannot -- pool separately)
int conv_dw_gap_tiles(const ConvP& p);
// mean over the feature map from conv_dw's per-tile sums: y[n][c] = (sum over tiles of part[n][t][c]) / hw, fixed order
void global_avgpool_finish(hipStream_t s, const float* part, float* y, int N, int tiles, int C, int hw);
// Direct conv for everything else (small Cin, odd channels, grouped). w: [kh][kw][Cin/g][Cout].
void conv_direct(hipStream_t s, const ConvP& p);
// RGB stem with the page normalisation folded in: the stem reads the u8 HWC pages themselves and computes
// (float)v * alpha[c] + beta[c] for tensor channel c = page channel src[c] on the fly -- the same two f32 operations
// pp::normalize performs, so the result is bit-identical to normalize + conv -- instead of a 12-bytes-per-pixel f32 tensor
// being written and read back.  Up to 32 separately allocated pages per launch.
// `dev` == nullptr: st.pages[0..n) are H x W x 3 pages of one size, normalised as x * alpha + beta (the detector).  `dev` != nullptr
// (the recognizer): image i is dev[i].ptr, H rows of dev[i].w <= W pixels -- columns past its own width read as zero AFTER
// normalisation, which is how the CRNN input is padded (crnn.rs:98-121) -- and a byte v becomes ((v / 255 - 0.5) / 0.5), the
// recognizer's expression, through a 256-entry table.
struct StemImg { const uint8_t* ptr; int32_t w; int32_t pad; };
struct StemU8 { const uint8_t* pages[32]; int src[3]; float alpha[3], beta[3]; const StemImg* dev = nullptr; };
void conv_smallcin_u8(hipStream_t s, const ConvP& p, const StemU8& st);
// Two stacked ConvTranspose 2x2 / stride 2 layers as one kernel -- the tail of the DB head (C/4 -> C/4 -> 1 channels): the
// intermediate map, 4x the input's pixels, never leaves the registers.  x: [N, H, W, C0] NHWC; w1: [C0][4][C1] (4 = a * 2 + b of
// the first layer), w2: [C1][4][C2]; y: [N, 4H, 4W, C2] NHWC.  C0, C1 % 4 == 0, C1 <= 32, C2 <= 4.
struct ConvT2Pair {
    const float* x; float* y;
    const float *w1, *b1, *w2, *b2;   // biases may be null
    int N, H, W, C0, C1, C2;
    Act act1, act2;
};
bool convt2x2_pair_supported(int C0, int C1, int C2);
void convt2x2_pair(hipStream_t s, const ConvT2Pair& p);
// General ConvTranspose (gather form). w: [kh][kw][Cin][Cout] (groups == 1), output_padding folded in Ho/Wo.
void convt_direct(hipStream_t s, const ConvP& p);

struct PoolP {
    int N, H, W, C, Ho, Wo, kh, kw, sh, sw, pt, pl;
    int pb, pr;              // bottom / right padding: the divisor of count_include_pad counts padding, not the ceil_mode overhang beyond it
    int is_max, count_include_pad;
    const float* x;
    float* y;
};
void pool2d(hipStream_t s, const PoolP& p);
// partial: scratch of N * global_avgpool_splits(N, HW, C) * C floats (may be null when the split count is 1)
int global_avgpool_splits(int N, int HW, int C);
void global_avgpool(hipStream_t s, const float* x, float* y, int N, int HW, int C, float* partial = nullptr);

// Resize NHWC. mode 0 = nearest, 1 = bilinear. ctm: 0 = asymmetric, 1 = half_pixel, 2 = align_corners,
// 3 = pytorch_half_pixel. nearest_mode: 0 = floor, 1 = round_prefer_floor, 2 = round_prefer_ceil, 3 = ceil.
// source index of output index o for mode = nearest (host evaluation of the kernel's own index map)
int resize_nearest_index(int o, float scale, int in, int out, int ctm, int nearest_mode);
// y = a op nearest_upsample(b), integer factors (fh, fw), NHWC, C % 4 == 0: b is [N, Ho / fh, Wo / fw, C]
void binary_upsampled(hipStream_t s, const float* a, const float* b, float* y, int N, int Ho, int Wo, int C, int fh, int fw, int op);
void resize(hipStream_t s, const float* x, float* y, int N, int H, int W, int C, int Ho, int Wo, float scale_h,
            float scale_w, int mode, int ctm, int nearest_mode, int y_ld);
// Channel concat of channels-last maps in ONE launch: source i contributes c[i] channels (c[i] % 4 == 0) at channel offset off[i], read at
// pixel (oh / fh[i], ow / fw[i]) of its [N][Ho / fh][Wo / fw][c] map (integer-factor nearest upsampling with coordinate mode asymmetric /
// floor; f = 1: a plain copy).  The DB neck's Concat(up8(p5), up4(p4), up2(p3), p2) was three resize launches and a copy.
struct ConcatGatherP { const float* x[8]; int c[8], off[8], fh[8], fw[8]; int n_src, N, Ho, Wo, C; };
void concat_gather(hipStream_t s, const ConcatGatherP& p, float* y);

void unary(hipStream_t s, const float* x, float* y, int64_t n, Act act, const char* prof_class = nullptr);   // prof_class: as for conv_igemm
// y = op(a, b) with numpy broadcasting over up to 6 dims. op: 0 add, 1 sub, 2 mul, 3 div, 4 pow, 5 prelu, 6 max, 7 min,
// 8 equal, 9 less, 10 greater, 11 and, 12 or (comparisons / logic give 1.0f or 0.0f: bool tensors live as f32 on the device). Strides in elements
// (0 for broadcast dims); output is contiguous with dims `dims`.
void binary(hipStream_t s, const float* a, const float* b, float* y, int op, int rank, const int64_t* dims,
            const int64_t* sa, const int64_t* sb, Act post);
// Copies `rows` rows of `c` floats from x (ld x_ld) to y (ld y_ld): channel concat / strided views.
void copy2d(hipStream_t s, const float* x, float* y, int64_t rows, int c, int x_ld, int y_ld);
// Generic permute: y (contiguous, dims out_dims) = x indexed with in_strides (already permuted), rank <= 6.
void permute(hipStream_t s, const float* x, float* y, int rank, const int64_t* out_dims, const int64_t* in_strides);

// Batched GEMM, row-major: C[b] (MxN) = alpha * A[b] (MxK) * B[b] (KxN or NxK if transB) (+ bias[N]) (+ residual) then act.
// batch strides in elements (0 = shared). VALU-tiled kernel for the small attention products.
struct GemmP {
    int batch, M, N, K, transB;
    int64_t sA, sB, sC;
    float alpha;
    const float *A, *B, *bias, *residual;
    float* C;
    Act act;
};
void gemm_batched(hipStream_t s, const GemmP& p);

void layernorm(hipStream_t s, const float* x, const float* gamma, const float* beta, float* y, int64_t rows, int C, float eps, const char* prof_class = nullptr);   // prof_class: as for conv_igemm
// add_layernorm.hip: s = a + b (row r of b is b[(r % b_rows) * C ...], b_rows | rows), y = LN(s) * gamma + beta; s is stored only when sum_out != null.
// Bit-identical to binary (Add) followed by layernorm.  gamma / beta may be null; y and sum_out must not overlap a, b or each other.
void add_layernorm(hipStream_t s, const float* a, const float* b, int64_t b_rows, const float* gamma, const float* beta, float* sum_out, float* y, int64_t rows, int C, float eps);
void softmax_lastdim(hipStream_t s, const float* x, float* y, int64_t rows, int C);
// squeeze-excite gate on a pooled vector: y[n] = act2(W2 act1(W1 x[n] + b1) + b2); w1 = W1 [Cmid][C], w2 = W2 TRANSPOSED [Cmid][Cout]
// tiles > 0: x is not the pooled vector but the per-tile channel sums a pooling depthwise conv left ([N][tiles][C], conv_dw with gap_part);
// the kernel reduces them itself, in global_avgpool_finish's order, and divides by hw -- the squeeze costs no launch of its own
void se_fc(hipStream_t s, const float* x, const float* w1, const float* b1, Act act1, const float* w2, const float* b2, Act act2, float* y, int N, int C,
           int Cmid, int Cout, int tiles = 0, int hw = 0);
// ONNX Pad on a contiguous tensor of rank <= 6: out_dims[d] = in_dims[d] + before[d] + after[d] (negative = crop);
// mode 0 constant (value), 1 reflect, 2 edge
void pad_nd(hipStream_t s, const float* x, float* y, int rank, const int64_t* in_dims, const int64_t* out_dims, const int64_t* before, int mode, float value);
// reduction over the last axis: x [rows][C] -> y [rows]; mode 0 mean, 1 sum, 2 max, 3 min, 4 prod
void reduce_lastdim(hipStream_t s, const float* x, float* y, int64_t rows, int C, int mode);
void argreduce_lastdim(hipStream_t s, const float* x, float* y, int64_t rows, int C, bool is_min, bool select_last);
// index_ops.hip: TopK over the last axis, x [rows][C] -> values / indices [rows][K], sorted (largest: descending), ties to the lower column
// (np.argsort(kind="stable")); indices are f32-coded.  1 <= K <= C <= kTopKMaxC.  One workgroup per row, the row resident in LDS.
constexpr int kTopKMaxC = 16384;
size_t topk_lds_bytes(int C, int K);
void topk_lastdim(hipStream_t s, const float* x, float* values, float* indices, int64_t rows, int C, int K, bool largest);
// y[s][0 .. inner) = x[row(s)][0 .. inner) for s in [0, slices): the index tuple of slice s is idx[(idx_mod > 0 ? s % idx_mod : s) * m + q], q < m, f32-coded;
// row(s) = (s / group) * group_stride + sum_q wrap(tuple[q], dims[q]) * strides[q] (elements).  Gather: m = 1, idx_mod = number of indices, group = the same,
// group_stride = dims[0] * inner; GatherND: idx_mod = 0, group = slices per batch.  A negative index wraps once; one still out of range zero-fills the slice.
struct GatherRowsP { long slices, inner, group, group_stride, idx_mod; int m; long dims[6], strides[6]; };
void gather_rows(hipStream_t s, const float* x, const float* idx, float* y, const GatherRowsP& p);
// GatherElements: y[w] = x[coords of w with coordinate `axis` replaced by idx[w]]; dims = the index / output dims, xstrides = the data's strides (elements)
struct GatherElemP { long total, axis_dim; int rank, axis; long dims[6], xstrides[6]; };
void gather_elements(hipStream_t s, const float* x, const float* idx, float* y, const GatherElemP& p);
// sla_decode.hip: the SLANet structure head, all `M` greedy steps of every image in one launch (one workgroup per image).
//   fea [B][HW][C], proj [B][HW][H] (= fea W_i2h^T), h0 [B][H], pre0 [B] (f32-coded token)
//   w_h4 [4H][Hp] = W_h2h ; W_hh with b_h4 [4H];  w_score [Hp];  w_ihc [3H][Cp] = W_ih[:, :C], w_ihv [V][3H] = W_ih[:, C:]^T, b_ih [3H];
//   w_sl1 [2H][Hp] = W_s1 ; W_l1 with b_sl1 [2H];  w_s2 [V][Hp], b_s2 [V];  w_l2 [L][Hp], b_l2 [L]      (Hp / Cp: H / C rounded up to 4, zero filled)
//   -> h_out [B][H], pre_out [B] (f32-coded), logits [M][B][V], loc [M][B][L] (after the sigmoid)
constexpr int kSlaMaxH = 512, kSlaMaxC = 512, kSlaMaxV = 1024, kSlaMaxHW = 1024, kSlaMaxL = 16, kSlaMaxM = 4096;
struct SlaDecodeP {
    int B, HW, C, H, V, L, M;
    const float *fea, *proj, *h0, *pre0;
    const float *w_h4, *b_h4, *w_score, *w_ihc, *w_ihv, *b_ih, *w_sl1, *b_sl1, *w_s2, *b_s2, *w_l2, *b_l2;
    float *h_out, *pre_out, *logits, *loc;
};
bool sla_decode_supported(int HW, int C, int H, int V, int L, int M);
size_t sla_decode_lds_bytes(int HW, int C, int H, int V);
void sla_decode(hipStream_t s, const SlaDecodeP& p);
// formula_decode.hip: the greedy decode of a PP-FormulaNet-style head (pre-norm transformer decoder with a key / value cache), `M` steps of
// 8 Ld + 2 short launches each per chunk of <= kFdChunk images (no grid-wide barrier; see the file's header for the chain).
//   tok0 [B] (f32-coded start token); e_tok [V][D], e_pos [P][D]; per layer the matrices with rows padded to a multiple of four floats:
//   w_qkv [2Dq + D][Dp] = Wq ; Wk ; Wv with b_qkv [2Dq + D] (Dq = nh dq: the q . k width of squeeze attention, dq = D / nh without it), w_o / w_cq / w_co [D][Dp], w_1 [F][Dp], w_2 [D][Fp]; kmT [B][nh][dh][S], vm [B][nh][S][dh];
//   w_lm [V][Dp], b_lm [V] or null.  q_scale_mode / cq_scale_mode: 0 none, 1 (x W^T + b) * s, 2 (x W^T) * s + b -- where the graph had the Mul.
//   -> tokens [M][B] (f32-coded), logits [M][B][V] when not null.  ws: formula_decode_ws_floats(...) floats of scratch (caches [l]{k [b][nh][M][dq], v [b][nh][M][dh]} + rows).
constexpr int kFdMaxD = 1024, kFdMaxDh = 128, kFdMaxF = 4096, kFdMaxLayers = 12, kFdMaxV = 1 << 24, kFdMaxM = 4096, kFdMaxS = 4096, kFdChunk = 16;
struct FdLayerP {
    const float *ln1_g, *ln1_b, *w_qkv, *b_qkv, *w_o, *b_o, *ln2_g, *ln2_b, *w_cq, *b_cq, *w_co, *b_co, *ln3_g, *ln3_b, *w_1, *b_1, *w_2, *b_2;
    float eps1, eps2, eps3, q_scale, cq_scale;
    int q_scale_mode, cq_scale_mode;
    const float *kmT, *vm;
};
// Stop token (opt-in; formula_decode.hip's header has the protocol).  FdStopState: the per-chunk state, device memory the engine owns for its lifetime.
// FdStop: what one run needs on top -- the host side of the look-ahead and the run's counters.  kFdLookahead: how many steps the host may be ahead of the
// last step it knows to have ended.  4 is the best of the 2 / 4 / 8 / 16 sweep on the S-shaped head (Speed; profiles/r8/formula_decode_stop.txt).  Every
// translation unit must see the same value: it sizes FdStop::ev.
#ifndef OAR_FD_LOOKAHEAD
#define OAR_FD_LOOKAHEAD 4
#endif
constexpr int kFdLookahead = OAR_FD_LOOKAHEAD;
struct FdStopState { int done[kFdChunk]; int alive; int pad; unsigned long long steps_executed; };
struct FdStop {
    int token = -1;                      // 0 <= token < V
    FdStopState* state = nullptr;        // device
    volatile unsigned* fin = nullptr;    // mapped, coherent host word: the generation of the last chunk that finished early
    unsigned* fin_dev = nullptr;         // the same word as the device sees it
    hipEvent_t ev[kFdLookahead + 1] = {};// ring: ev[t % (kFdLookahead + 1)] is recorded after step t
    unsigned gen = 0;                    // one per chunk, never 0
    bool first_chunk = true;             // the next chunk is the first of its run: its start launch clears the device's step counter
};
struct FdRunStats { int64_t steps_limit = 0, steps_enqueued = 0; };
struct FormulaDecodeP {
    int B, D, nh, F, V, Ld, S, M, P, c_pos;
    int dq;                              // head width of the self-attention queries / keys, 1 <= dq <= kFdMaxDh, nh dq <= kFdMaxD; below, at or above D / nh (D / nh: no squeeze)
    float s_emb, eps_e, eps_f;
    const float *tok0, *e_tok, *e_pos, *lne_g, *lne_b, *lnf_g, *lnf_b, *w_lm, *b_lm;
    FdLayerP layer[kFdMaxLayers];
    float *ws, *tokens, *logits;
    FdStop* stop;                        // null: off
    FdRunStats* stats;                   // null, or the counters this call adds to (host side only)
};
bool formula_decode_supported(int D, int nh, int F, int V, int Ld, int M, int S, int dq);
int formula_decode_lm_workgroups(int V);          // (value, index) partials per image of the arg max
int formula_decode_launches_per_step(int Ld);     // 8 Ld + 2, per chunk of kFdChunk images
size_t formula_decode_ws_floats(int B, int D, int F, int V, int Ld, int M, int Dq);
void formula_decode(hipStream_t s, const FormulaDecodeP& p);
// window_attention.hip: the attention of one Swin block, one launch.  q, k, v [B H W][nh dh] in IMAGE order (token (b, y, x) is row
// (b H + y) W + x, row strides ldq / ldk / ldv floats), bias [nh][N][N] with N = ws^2 (the relative-position bias, added to the scaled scores);
// o [B H W][nh dh] in image order.  A window's tokens are gathered and scattered by address: no partitioned copy exists.
// scale_div: scores / scale (the graph's Div) instead of scores * scale (its Mul).
// The windows tile the grid padded at the bottom / right to Hp x Wp (multiples of ws, Hp - H < ws, Wp - W < ws) and rolled by -shift on both axes
// (window_token_row below).  A padding token is a key whose k / v rows are kbias / vbias (null: zeros) -- the graph pads in front of the Linears --
// and is skipped as a query.  mask: null, or [nW][N][N] with nW = (Hp / ws) (Wp / ws), added to the scores behind the bias.
struct WindowAttnP {
    const float *q, *k, *v, *bias;
    float* o;
    int ldq, ldk, ldv, ldo;
    int B, H, W, ws, nh, dh;
    float scale; int scale_div;
    int shift, Hp, Wp, nW;
    const float *mask, *kbias, *vbias;
};
// The address map of a Swin window: local token n = (r, c) of window (wy, wx) sits at (Y, X) = (wy ws + r, wx ws + c) of the padded, rolled grid and comes
// from (y, x) = ((Y + shift) mod Hp, (X + shift) mod Wp) of the padded grid.  Returns the token's row y W + x within its image, or -1 for padding
// (y >= H or x >= W).  The reverse roll and the crop are the inverse map, so the output goes to the same row.  (tests/test_swin_shift_cpu.py compiles this)
__host__ __device__ inline int window_token_row(int wy, int wx, int n, int ws, int H, int W, int Hp, int Wp, int shift) {
    const int r = n / ws, c = n - r * ws;
    int y = wy * ws + r + shift, x = wx * ws + c + shift;
    if (y >= Hp) y -= Hp;
    if (x >= Wp) x -= Wp;
    return y < H && x < W ? y * W + x : -1;
}
constexpr int kWinThreads = 256, kWinWaves = kWinThreads / 64, kWinMaxN = 256, kWinMaxDh = 64, kWinMaxNd = 8192;
bool window_attention_supported(int ws, int heads, int head_dim);   // N = ws^2 <= kWinMaxN, head_dim <= kWinMaxDh, N head_dim <= kWinMaxNd
// the kernel's LDS, all of it dynamic: K [N][dh | 1], V [N][dh], one q row and one row of probabilities per wave (tests/test_unimernet_cpu.py compiles this)
inline size_t window_attention_lds_bytes(int N, int head_dim) {
    return ((size_t)N * (size_t)(head_dim | 1) + (size_t)N * head_dim + (size_t)kWinWaves * kWinMaxDh + (size_t)kWinWaves * N) * sizeof(float);
}
void window_attention(hipStream_t s, const WindowAttnP& p);
// deformable_attention.hip: multi-scale deformable attention (RT-DETR's decoder), one launch.  value [N][Lv][nh][c] with Lv = sum of h w over the levels,
// level l starting at row start[l]; loc [N][Q][nh][L][P][2] = (x, y) in units of the level's width / height; w [N][Q][nh][L P]: logits (softmax = 1: the
// kernel takes their softmax over L P) or the weights themselves; y [N][Q][nh c].  Every sample is a bilinear tap with zero padding (GridSample, align_corners
// = 0): a corner outside [0, w) x [0, h) is tested in float, contributes 0 and never becomes an address.
constexpr int kDefMaxLevels = 4, kDefMaxSamples = 32, kDefMaxC = 64, kDefThreads = 256;
struct DeformAttnP {
    const float *value, *loc, *w;
    float* y;
    int N, Q, nh, c, L, P, Lv, softmax;
    int h[kDefMaxLevels], wd[kDefMaxLevels], start[kDefMaxLevels];
};
// c % 4 == 0, c <= kDefMaxC, L <= kDefMaxLevels, L P <= kDefMaxSamples, and token / thread counts that fit 32 bits (N = Q = 1: the static part of the question)
bool deformable_attention_supported(int64_t N, int64_t Q, int64_t nh, int64_t c, int64_t L, int64_t P, int64_t Lv);
void deformable_attention(hipStream_t s, const DeformAttnP& p);
// flash_f32_dev.h: the flash-attention core relpos_attention.hip and mha_attention.hip share -- ONE layout: a workgroup of kFlashThreads owns kFlashQueries
// queries, K and V stream through LDS in blocks of kFlashKeys keys, rows padded to kFlashLd floats, head_dim <= kFlashMaxDh.
constexpr int kFlashThreads = 256, kFlashQueries = 64, kFlashKeys = 32, kFlashLd = 68, kFlashMaxDh = 64;
// the K and V blocks [2 stages][kFlashKeys][kFlashLd] each, in front of whatever else a kernel keeps in its dynamic LDS
inline size_t flash_kv_lds_bytes() { return (size_t)4 * kFlashKeys * kFlashLd * sizeof(float); }
// relpos_attention.hip: the attention of one SAM / Vary ViT block with the decomposed relative-position bias, one launch.
// qkv [B H W][3][nh][dh]: the fused projection of the UNPADDED tokens in IMAGE order (token (b, y, x) is row (b H + y) W + x); o [B H W][nh dh] in image order.
// ws = 0: every query attends to the whole H x W grid; ws > 0: inside ws x ws windows of the grid padded at the bottom / right to multiples of ws.  A padding
// token is a key whose k / v rows are bqkv's (null: zeros) -- the graph pads in front of the Linear -- and takes part in the soft-max (there is no mask); as a
// query it is skipped.  With (gh, gw) = (ws, ws) or (H, W) the key grid: rh [gh][dh][gh], rw [gw][dh][gw] (query row / column, component, key row / column), and
//   score[(qy, qx), (ky, kx)] = scaled q . k + q . rh[qy][:][ky] + q . rw[qx][:][kx]   with the UNSCALED q in both rel terms;
// scale_pre: q is multiplied by `scale` in front of the product (the graph's Mul on q), otherwise the product is (its Mul on the scores).
// The key set is streamed in blocks of kFlashKeys with a running maximum and sum: no score row exists in memory and gh gw has no upper limit.
struct RelPosAttnP {
    const float *qkv, *rh, *rw, *bqkv;
    float* o;
    int B, H, W, ws, nh, dh;
    float scale; int scale_pre;
};
constexpr int kRpQueries = kFlashQueries, kRpMaxDh = kFlashMaxDh, kRpMaxGrid = 64;
// head_dim % 4 == 0 and <= kRpMaxDh; key grid sides <= kRpMaxGrid (ws <= 64, or H, W <= 64 when ws = 0); token and workgroup counts that fit 32 bits (B = 1: the
// static part of the question)
bool relpos_attention_supported(int64_t B, int64_t H, int64_t W, int64_t ws, int64_t heads, int64_t head_dim);
// the kernel's LDS, all of it dynamic: the K and V blocks, the blocks' key coordinates [2][kFlashKeys], and rh / rw of the workgroup's queries
// [kRpQueries][gh | 1], [kRpQueries][gw | 1] (tests/test_vit_relpos_cpu.py compiles this)
inline size_t relpos_attention_lds_bytes(int gh, int gw) {
    return flash_kv_lds_bytes() + ((size_t)2 * kFlashKeys + (size_t)kRpQueries * ((size_t)(gh | 1) + (size_t)(gw | 1))) * sizeof(float);
}
void relpos_attention(hipStream_t s, const RelPosAttnP& p);
// mha_attention.hip: multi-head attention with separate q / k / v sources, one launch.  q is viewed as [N][Tq][nh][dh] with a row stride of ldq
// floats (image b starts at b Tq ldq), k and v as [N][Tk][nh][dh] with ldk / ldv: a q / k pair may live in one [N, T, 2 nh dh] Linear output (ld = 2 nh dh, k's
// pointer advanced by nh dh).  o [N][Tq][nh dh] is contiguous, in token order.  o = softmax(scaled q k^T) v per (image, head);
// scale_pre: q is multiplied by `scale` in front of the product (the graph's Mul on q), otherwise the product is (its Mul on the scores).
// The keys are streamed in blocks of kFlashKeys with a running maximum and sum: no score row exists in memory and Tq, Tk have no upper limit.
struct MhaAttnP {
    const float *q, *k, *v;
    float* o;
    int N, Tq, Tk, nh, dh;
    int ldq, ldk, ldv;
    float scale; int scale_pre;
};
constexpr int kMhaQueries = kFlashQueries, kMhaMaxDh = kFlashMaxDh;
// head_dim % 4 == 0 and <= kMhaMaxDh; token and workgroup counts that fit 32 bits (N = 1: the static part of the question)
bool mha_attention_supported(int64_t N, int64_t Tq, int64_t Tk, int64_t heads, int64_t head_dim);
// the kernel's LDS, all of it dynamic: the K and V blocks.  The rows are padded for the largest head whatever head_dim is, so the answer does not depend
// on it (tests/test_mha_attention_cpu.py compiles this)
inline size_t mha_attention_lds_bytes(int head_dim) {
    (void)head_dim;
    return flash_kv_lds_bytes();
}
void mha_attention(hipStream_t s, const MhaAttnP& p);
// vis_attention.hip: the attention of one layer of the PaddleOCR-VL vision encoder, one launch.  The patches of several images are packed back
// to back as T rows; qkv [T][ld] is the fused projection (row t: q [nh][dh] at column 0, k at nh dh, v at 2 nh dh; ld >= 3 nh dh), cos / sin [T][dh / 2]
// the rotary tables, o [T][nh dh] in token order.  Segment i is rows [start, start + len) and a query attends exactly to the keys of its own segment:
//   q'[c] = q[c] cos[c] - q[c + dh/2] sin[c],  q'[c + dh/2] = q[c + dh/2] cos[c] + q[c] sin[c]   (c < dh/2; the same for k),  o = softmax(scale q' k'^T) v.
// The rotation happens in registers when the q fragments are loaded and when a key block is staged; the scores are scaled after the product.
// tiles: one (segment, head, query tile of kFlashQueries) entry per workgroup, built on the host, so the grid is flat over segments of different lengths.
struct VisSeg { int start, len; };
struct VisTile { int seg, head, qt, pad; };
struct VisAttnP {
    const float *qkv, *cos, *sin;
    float* o;
    const VisSeg* segs;
    const VisTile* tiles;
    int n_tiles, nh, dh, ld;
    float scale;
};
constexpr int kVisMinDh = 8, kVisMaxDh = 80, kVisLd5 = 84;   // head_dim % 8 == 0 (the rotary partner of a float4 group is a float4 group); the LDS row stride at DH16 = 5
inline bool vis_attention_supported(int64_t heads, int64_t head_dim) {
    return heads >= 1 && heads < ((int64_t)1 << 20) && head_dim >= kVisMinDh && head_dim <= kVisMaxDh && head_dim % 8 == 0;
}
// the kernel's LDS, all of it dynamic: the K and V blocks [2][kFlashKeys][ld] each with ld = kFlashLd up to head size 64 and kVisLd5 above
// (tests/test_vision_resources_cpu.py compiles this)
inline size_t vis_attention_lds_bytes(int head_dim) {
    return (size_t)4 * kFlashKeys * (head_dim > kFlashMaxDh ? kVisLd5 : kFlashLd) * sizeof(float);
}
inline int64_t vis_attention_tile_count(const int32_t* lens, int n_segs, int heads) {
    int64_t n = 0;
    for (int i = 0; i < n_segs; ++i) n += (int64_t)heads * ((lens[i] + kFlashQueries - 1) / kFlashQueries);
    return n;
}
// segs [n_segs] and tiles [vis_attention_tile_count] in the order (segment, head, query tile)
inline void vis_attention_tables(const int32_t* lens, int n_segs, int heads, VisSeg* segs, VisTile* tiles) {
    int start = 0;
    for (int i = 0; i < n_segs; ++i) {
        segs[i] = VisSeg{start, lens[i]};
        start += lens[i];
        for (int h = 0; h < heads; ++h)
            for (int qt = 0; qt < (lens[i] + kFlashQueries - 1) / kFlashQueries; ++qt) *tiles++ = VisTile{i, h, qt, 0};
    }
}
// what one launch moves and computes: q, o and the tables once, k and v once per query tile; 4 len^2 dh flops per (segment, head)
inline void vis_attention_cost(const int32_t* lens, int n_segs, int heads, int head_dim, double* bytes, double* flops) {
    double b = 0.0, f = 0.0;
    for (int i = 0; i < n_segs; ++i) {
        const double len = lens[i], tiles = (lens[i] + kFlashQueries - 1) / kFlashQueries;
        b += 4.0 * heads * head_dim * len * (2.0 + 2.0 * tiles) + 4.0 * len * head_dim * (1.0 + tiles);
        f += 4.0 * heads * len * len * head_dim;
    }
    *bytes = b; *flops = f;
}
void vis_attention(hipStream_t s, const VisAttnP& p, double bytes, double flops);
// vis_misc.hip: the small steps of the vision encoder.  Up to kVisMaxImages images of one call, image i being rows [start[i], start[i + 1]) with an
// h[i] x w[i] grid of patches.
constexpr int kVisMaxImages = 16;
struct VisGrids { int n; int start[kVisMaxImages + 1]; int h[kVisMaxImages], w[kVisMaxImages]; };
// out [T][D]: the learned position table [G G][D] resampled bilinearly to every image's grid (align_corners = false: source coordinate
// ((o + 0.5) G / out - 0.5) in f32, clamped to [0, G - 1]; weights wy wx, sum in the order 00, 01, 10, 11).  h = w = G gives the table itself.  D % 4 == 0
void vis_pos_embed(hipStream_t s, const float* table, float* out, const VisGrids& g, int G, int D);
// out [T / m^2][m^2 D]: row (image, hb, wb) is the concatenation over (mi, mj) of x's rows (image, hb m + mi, wb m + mj).  D % 4 == 0, m | h, w
void vis_merge_gather(hipStream_t s, const float* x, float* out, const VisGrids& g, int m, int D);
inline void reduce_mean_lastdim(hipStream_t s, const float* x, float* y, int64_t rows, int C) { reduce_lastdim(s, x, y, rows, C, 0); }
// y = cond != 0 ? a : b with numpy broadcasting over up to 6 dims (strides in elements, 0 = broadcast)
void where(hipStream_t s, const float* cond, const float* a, const float* b, float* y, int rank, const int64_t* dims, const int64_t* sc, const int64_t* sa, const int64_t* sb);
// ONNX GridSample (4-D): x [N][H][W][C] channels-last, grid [N][Ho][Wo][2] (x, y in [-1, 1]) -> y [N][Ho][Wo][C].
// mode 0 bilinear / 1 nearest; padding 0 zeros / 1 border / 2 reflection
void grid_sample(hipStream_t s, const float* x, const float* grid, float* y, int N, int H, int W, int C, int Ho, int Wo, int mode, int padding, int align_corners);
// softmax(scale * q k^T) v per (image, head); qkv [n][T][3][heads][hd] row-major, out [n][T][heads][hd]; hd <= 64
void attention(hipStream_t s, const float* qkv, float* out, int n, int T, int heads, int hd, float scale);
// attention_x6.hip: the same operator flash-style on the bf16 matrix pipe (bf16x6 products), any T, head dim 32 -- what `attention` launches for
// hd == 32 unless OAR_ATTN_X6=0; attention_fits(T, hd): can `attention` run this shape at all (either kernel)?
bool attention_x6_supported(int T, int heads, int hd);
void attention_x6(hipStream_t s, const float* qkv, float* out, int n, int T, int heads, int hd, float scale);
bool attention_fits(int T, int heads, int hd);
// A run of sample-local operators as one launch (chain.hip): one workgroup per sample walks the table.  Every tensor is a row-major
// [n_samples * T rows][ld floats] view; sample s owns rows [s * T, (s + 1) * T).
enum ChainType : int { CH_GEMM = 0, CH_LN = 1, CH_ATTN = 2, CH_COPY = 3, CH_POOL = 4 };   // CH_POOL: AveragePool K x cin (rows x columns per token) that leaves one row: in = the sample's [K][pad][N] map, pad = its width >= cin * T
struct ChainRef { unsigned long long v = 0; int kind = -1; };   // kind: -1 none, 0 absolute device pointer, 1 arena-relative byte offset, 2 primary-input-relative
struct ChainOpD {
    int type = 0;
    int K = 0, N = 0;            // GEMM: reduction length (taps * cin) / output channels; LN, COPY: N = row length
    int cin = 0, pad = 0;        // GEMM over a 1 x k convolution: k = K / cin taps, input row t + tap - pad (zero outside the sample)
    int ksplit = 1;              // GEMM: K slices reduced through LDS
    int mb = 1;                  // GEMM: token tiles (of 16 rows) one work item covers, 1..3 (4 would spill)
    int in_ld = 0, out_ld = 0, res_ld = 0;
    int act = 0; float alpha = 0.f, beta = 0.f;
    float eps = 0.f, scale = 0.f;   // LN epsilon / attention scale
    int heads = 0, hd = 0;
    ChainRef in, out, res;
    const float* w = nullptr;    // GEMM: [N][K] f32, K index = tap * cin + c (inside the chain's constant blob)
    int bias_l = -1;             // GEMM bias [N] / LN beta: float offset in LDS (the kernel copies the small constants there), -1 = none
    int w_l = -1;                // LN gamma: float offset in LDS, -1 = none
};
static_assert(sizeof(ChainOpD) % 4 == 0, "ChainOpD is copied to LDS word by word");
// The kernel's three device-side choices, restated for the name of what ran: Planner::fuse_chains builds the launch's path signature from them.  The `switch`
// at the bottom of chain_kernel keeps its own spelling of the same conditions (calling these there changes its generated code), and
// tests/test_chain_cases_cpu.py reads both sources and holds them, and oar_ocr_amd/synth/chain_cases.py's Python restatement, to each other.
enum ChainGemmPath : int { CH_G_SHORT = 0, CH_G_LDS1 = 1, CH_G_LDS2 = 2, CH_G_LDS3 = 3, CH_G_HBM = 4 };
// product: tokens in HBM -> the general path; one token tile per item and a K slice of fewer than four 16-wide steps -> the guarded short loop; else mb tiles per item
__host__ __device__ inline int chain_gemm_path(bool in_lds, int mb, int K, int ksplit) {
    if (in_lds && mb == 1 && ((K >> 4) + ksplit - 1) / ksplit < 4) return CH_G_SHORT;
    if (in_lds && mb == 1) return CH_G_LDS1;
    if (in_lds && mb == 2) return CH_G_LDS2;
    if (in_lds) return CH_G_LDS3;
    return CH_G_HBM;
}
// LayerNorm: the row as float4s in registers, or float by float
__host__ __device__ inline bool chain_ln_float4(int C) { return C <= 256 && (C & 3) == 0; }
// attention: 1..4 = ch_attention_mfma<token tiles>, 0 = ch_attention_any
__host__ __device__ inline int chain_attn_tiles(int T, int hd) {
    if (T <= 64 && (hd & 3) == 0) return T <= 16 ? 1 : T <= 32 ? 2 : T <= 48 ? 3 : 4;
    return 0;
}
struct ChainLaunch {
    const ChainOpD* ops = nullptr; int n_ops = 0, n_samples = 0, T = 0, max_hd = 0;
    size_t lds = 0;              // dynamic LDS: split-K scratch | resident tensors | small constants | operator table
    const float* consts = nullptr; int small = 0, total_consts = 0, small_l = 0;   // constant blob (floats): [0, small) -> LDS at float offset small_l
    int tab_l = 0;               // float offset in LDS of the operator table copy
    double bytes = 0, flops = 0;
    std::string sig;             // the path of every operator, one token each in table order (chain_op_token), space-separated: the OAR_PROF_DETAIL name
};
// One operator's token: products gs / g1 / g2 / g3 / gh (chain_gemm_path) + k<ksplit> when split + r with a residual + the activation's letter
// (R relu, H hard-swish, G hard-sigmoid, S sigmoid, W swish); LayerNorm n4 / n1; attention a1..a4 / aa + d<head size>; p pool; c copy.
std::string chain_op_token(const ChainOpD& op, int T);
// "chain n=.. T=.. <tokens>" for the profiler's 96-byte names: the tokens as a list; where that does not fit, each distinct token once, in the order of its first
// appearance, with x<count>; where that does not fit either, the count of every token family.  Never truncated.
std::string chain_detail_name(int n_samples, int T, const std::string& sig);
constexpr size_t kChainLdsBudget = 159 * 1024;   // LDS a chain may plan with (the launch adds 640 bytes of debug stamps)
constexpr int kChainMaxHd = 16;   // attention head size the chain kernel is instantiated for (a 32-wide variant spills: wider heads stay unfused)
inline bool chain_act_ok(int kind) { return kind == ACT_NONE || kind == ACT_RELU || kind == ACT_HSWISH || kind == ACT_HSIGMOID || kind == ACT_SIGMOID || kind == ACT_SWISH; }
size_t chain_lds_bytes(const ChainOpD& op, int T);
void chain_run(hipStream_t s, const ChainLaunch& L, char* arena, const char* input);
// softmax over the last dim fused with CTC argmax (last max index wins) -- see kernels.hip
// CTC head without logits: conv_igemm with ConvP::ctc_part set writes {max, sum exp, last arg max} per (row, cout tile
// of 128 columns); ctc_combine merges the tiles of each row into the arg max index and its softmax probability.
int ctc_tiles(int n_padded);   // cout tiles per row for a (16-padded) class count
bool ctc_partials_supported(int K);
bool ctc_partials_supported_x6(int K);
void ctc_combine(hipStream_t s, const float* part, int64_t rows, int tiles, int64_t* idx, float* prob);
// ctc_head_x6.hip: the CTC head as an output-stationary bf16x6 kernel (K = 32 / 64; IGEMM_W_X6 weights; same partials as above)
bool ctc_head_x6_supported(long M, int K, int n_padded);
void ctc_head_x6(hipStream_t s, const float* x, const float* w_x6, const float* bias, float* part, long M, int K, int n_padded, int valid);
void softmax_argmax(hipStream_t s, const float* logits, int64_t rows, int C, int ld, int64_t* idx, float* prob);   // ld = row stride

}  // namespace k
}  // namespace oar
