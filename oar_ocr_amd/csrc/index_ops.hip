// index_ops.hip -- device-side selection for the engine: TopK over the last axis and the three ONNX gathers
// (Gather, GatherND, GatherElements).  Index tensors are f32-coded on the device, like ArgMax's output: an index is the
// float of an integer below 2^24 and the boundary (c_api.cc) converts to i64.
//
// TopK
//   One workgroup per row.  A float becomes a u32 that sorts like the float (sign flip for positives, complement for
//   negatives; -0.0 is folded into +0.0 first, so the two compare equal), complemented once more for largest = 1, so that
//   the wanted elements are always the SMALLEST keys.  The 64-bit sort key is (that u32 << 32) | column: among equal
//   values the lower column wins the comparison itself -- ONNX Runtime's tie rule, np.argsort(kind="stable") -- and no
//   second pass is needed.  The padding key ~0 loses against every real key (a real key's low half is a column < 2^14).
//   Values are re-read from the input by the winning column: bit copies, including the sign of a zero.
//   NaN: outside the contract.  A NaN is ordered by its bit pattern: one with the sign bit clear sorts above +inf, one
//   with it set below -inf; nothing faults and the index output stays a permutation of distinct columns.
//
//   Kp = K rounded up to a power of two, Cp likewise for the row length C.
//   * Kp <  Cp ("few of many": 300 of 8400): radix SELECT, then sort the survivors.  The row's u32 keys stay in LDS
//     (4 B per column: the column is the position).  Four passes over the value byte by byte, most significant first, each
//     with a 256-bin LDS histogram that one wave scans, find the value of the K-th smallest key; if more columns hold
//     that value than are still wanted, two more passes over the column's 14 bits find the last column taken.  Exactly K
//     keys are <= the threshold; they are compacted (any order) into a Kp-slot buffer and bitonic-sorted there.
//     LDS: 4 C + 8 Kp bytes (C = 16384, Kp = 8192: 128 KB).
//   * Kp == Cp ("all of them": the final sort by score): bitonic sort of Cp 64-bit keys.  LDS: 8 Cp <= 128 KB.
//   Both stay inside the 150 KB the other LDS-staged row kernels (softmax, attention) plan with.
//   Bitonic strides: a compare-exchange reads two ds_read_b64 at distance j.  For j >= 32 the 32 lanes of a half-wave read
//   32 consecutive 8-byte words, 64 distinct banks, conflict-free; for j < 32 consecutive lanes skip every other run of j
//   words, so a half-wave spans two 256-byte bank rows, a 2-way conflict -- 5 of the log2(n) strides of each merge, accepted.
//
// Gathers
//   gather_rows: y[s][0..inner) = x[row(s)][0..inner) for Gather and GatherND -- the index tuple of an output slice is
//   folded into ONE row offset, the contiguous inner run is copied with 16-byte accesses when its length and both base
//   addresses allow, scalar otherwise.  gather_elements: one index per output element.
//   A negative index wraps once (i + dim).  An index that is still out of range is never turned into an address: the
//   output element (Gather / GatherND: the whole slice) is written as 0.0f.
#include "common.h"
#include "kernels.h"

namespace oar {
namespace k {

namespace {

__device__ __forceinline__ unsigned topk_key(float v, bool largest) {
    unsigned u = __float_as_uint(v);
    if ((u << 1) == 0u) u = 0u;                               // -0.0 == +0.0
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);           // ascending like the float order
    return largest ? ~u : u;                                  // the wanted end is always the small one
}

// ascending bitonic sort of n = 2^p keys in LDS by the whole workgroup; ends with a barrier
__device__ __forceinline__ void bitonic_sort_lds(unsigned long long* b, int n) {
    const int tid = (int)threadIdx.x, nt = (int)blockDim.x;
    for (int k = 2; k <= n; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (n >> 1); t += nt) {
                const int i = 2 * t - (t & (j - 1));          // lower element of pair t at distance j
                const unsigned long long a = b[i], c = b[i + j];
                const bool asc = (i & k) == 0;
                if ((a > c) == asc) { b[i] = c; b[i + j] = a; }
            }
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(1024) void topk_lastdim_kernel(const float* __restrict__ x, float* __restrict__ values, float* __restrict__ indices, int C, int K, int Kp,
                                                            int Cp, int largest) {
    extern __shared__ unsigned long long topk_lds[];          // sort buffer [Kp or Cp] | u32 keys [C] (select path only)
    __shared__ unsigned hist[256];
    __shared__ unsigned sel[3];                               // digit, still wanted, columns in the chosen bin
    __shared__ unsigned fill;
    const int tid = (int)threadIdx.x, nt = (int)blockDim.x;
    const float* xr = x + (size_t)blockIdx.x * C;
    unsigned long long* sortb = topk_lds;
    int n_sort;
    if (Kp < Cp) {
        unsigned* keys = reinterpret_cast<unsigned*>(topk_lds + Kp);
        for (int i = tid; i < C; i += nt) keys[i] = topk_key(xr[i], largest != 0);
        for (int i = tid; i < Kp; i += nt) sortb[i] = ~0ull;
        if (tid == 0) fill = 0u;
        unsigned long long prefix = 0ull, mask = 0xFFFF0000ull;   // bits 16 .. 31 of a key are zero (a column is below 2^14): decided from the start
        unsigned need = (unsigned)K;
        bool whole_bin = false;                               // every column that matches the prefix is wanted
        for (int pass = 0; pass < 6 && !whole_bin; ++pass) {
            const int shift = pass < 4 ? 56 - 8 * pass : (pass == 4 ? 8 : 0);
            for (int i = tid; i < 256; i += nt) hist[i] = 0u;
            __syncthreads();
            for (int i = tid; i < C; i += nt) {
                const unsigned long long key = ((unsigned long long)keys[i] << 32) | (unsigned)i;
                if ((key & mask) == prefix) atomicAdd(&hist[(unsigned)(key >> shift) & 255u], 1u);
            }
            __syncthreads();
            if (tid < 64) {                                   // wave 0: lane l owns bins 4l .. 4l + 3
                const unsigned h0 = hist[4 * tid], h1 = hist[4 * tid + 1], h2 = hist[4 * tid + 2], h3 = hist[4 * tid + 3];
                const unsigned mine = h0 + h1 + h2 + h3;
                unsigned incl = mine;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) { const unsigned v = __shfl_up(incl, o, 64); if (tid >= o) incl += v; }
                const unsigned excl = incl - mine;
                if (excl < need && need <= incl) {            // exactly one lane: the bins hold >= need columns in all
                    unsigned below = excl, d = 0, c = h0;
                    if (below + c < need) { below += c; d = 1; c = h1; }
                    if (d == 1 && below + c < need) { below += c; d = 2; c = h2; }
                    if (d == 2 && below + c < need) { below += c; d = 3; c = h3; }
                    sel[0] = 4u * (unsigned)tid + d; sel[1] = need - below; sel[2] = c;
                }
            }
            __syncthreads();
            prefix |= (unsigned long long)sel[0] << shift;
            mask |= 0xFFull << shift;
            need = sel[1];
            whole_bin = need == sel[2];
        }
        // whole_bin: the threshold is the largest key with this prefix; otherwise all six passes ran and prefix is the K-th key itself
        const unsigned long long thr = whole_bin ? (prefix | ~mask) : prefix;
        for (int i = tid; i < C; i += nt) {
            const unsigned long long key = ((unsigned long long)keys[i] << 32) | (unsigned)i;
            if (key <= thr) {
                const unsigned pos = atomicAdd(&fill, 1u);
                if (pos < (unsigned)Kp) sortb[pos] = key;
            }
        }
        __syncthreads();
        n_sort = Kp;
    } else {
        for (int i = tid; i < Cp; i += nt) sortb[i] = i < C ? (((unsigned long long)topk_key(xr[i], largest != 0) << 32) | (unsigned)i) : ~0ull;
        __syncthreads();
        n_sort = Cp;
    }
    bitonic_sort_lds(sortb, n_sort);
    float* vr = values + (size_t)blockIdx.x * K;
    float* ir = indices + (size_t)blockIdx.x * K;
    for (int j = tid; j < K; j += nt) {
        const unsigned col = (unsigned)sortb[j];
        const bool ok = col < (unsigned)C;                    // (always, for the first K keys; a padding key never becomes an address)
        vr[j] = ok ? xr[col] : 0.0f;
        ir[j] = ok ? (float)col : 0.0f;
    }
}

__device__ __forceinline__ long wrap_index(float f, long dim) {
    long i = (long)f;
    if (i < 0) i += dim;
    return (i >= 0 && i < dim) ? i : -1;
}

template <int VEC>
__global__ __launch_bounds__(256) void gather_rows_kernel(const float* __restrict__ x, const float* __restrict__ idx, float* __restrict__ y, GatherRowsP p) {
    const long per_row = p.inner / VEC, total = p.slices * per_row;
    for (long w = (long)blockIdx.x * blockDim.x + threadIdx.x; w < total; w += (long)gridDim.x * blockDim.x) {
        const long s = w / per_row, c = (w - s * per_row) * VEC;
        const long g = s / p.group;
        const float* t = idx + (p.idx_mod > 0 ? s % p.idx_mod : s) * p.m;
        long off = g * p.group_stride;
        bool ok = true;
        for (int q = 0; q < p.m; ++q) {
            const long i = wrap_index(t[q], p.dims[q]);
            ok = ok && i >= 0;
            off += (i < 0 ? 0 : i) * p.strides[q];
        }
        if (VEC == 4) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (ok) v = *reinterpret_cast<const float4*>(x + off + c);
            *reinterpret_cast<float4*>(y + s * p.inner + c) = v;
        } else {
            y[s * p.inner + c] = ok ? x[off + c] : 0.0f;
        }
    }
}

__global__ __launch_bounds__(256) void gather_elements_kernel(const float* __restrict__ x, const float* __restrict__ idx, float* __restrict__ y, GatherElemP p) {
    for (long w = (long)blockIdx.x * blockDim.x + threadIdx.x; w < p.total; w += (long)gridDim.x * blockDim.x) {
        long rem = w, off = 0;
        for (int d = p.rank - 1; d >= 0; --d) {
            const long q = rem / p.dims[d], c = rem - q * p.dims[d];
            rem = q;
            if (d != p.axis) off += c * p.xstrides[d];
        }
        const long i = wrap_index(idx[w], p.axis_dim);
        y[w] = i >= 0 ? x[off + i * p.xstrides[p.axis]] : 0.0f;
    }
}

inline int pow2_ceil(int v) { int p = 1; while (p < v) p <<= 1; return p; }

}  // namespace

size_t topk_lds_bytes(int C, int K) {
    const int Kp = pow2_ceil(K), Cp = pow2_ceil(C);
    return Kp < Cp ? (size_t)Kp * 8 + (size_t)C * 4 : (size_t)Cp * 8;
}

void topk_lastdim(hipStream_t s, const float* x, float* values, float* indices, int64_t rows, int C, int K, bool largest) {
    OAR_CHECK(C >= 1 && C <= kTopKMaxC, OAR_UNSUPPORTED_OP, "TopK: row length must be in [1, " + std::to_string(kTopKMaxC) + "]");
    OAR_CHECK(K >= 1 && K <= C, OAR_SHAPE_MISMATCH, "TopK: K must be in [1, row length]");
    if (rows == 0) return;
    const int Kp = pow2_ceil(K), Cp = pow2_ceil(C);
    const size_t lds = topk_lds_bytes(C, K);
    OAR_CHECK(lds <= 150 * 1024, OAR_INTERNAL, "TopK: LDS plan exceeds the staging budget");
    if (lds > 48 * 1024) OAR_MAX_LDS_ONCE(topk_lastdim_kernel, 150 * 1024);
    // select path: a thread per 4 columns; sort path: a thread per pair
    const int want = Kp < Cp ? std::max(Cp / 4, Kp / 2) : Cp / 2;
    const int threads = std::min(1024, std::max(64, want));   // a power of two >= 64: whole waves
    ProfScope ps(s, "topk", 4.0 * (double)rows * (C + 2.0 * K), 0.0);
    hipLaunchKernelGGL(topk_lastdim_kernel, dim3((unsigned)rows), dim3((unsigned)threads), lds, s, x, values, indices, C, K, Kp, Cp, largest ? 1 : 0);
}

void gather_rows(hipStream_t s, const float* x, const float* idx, float* y, const GatherRowsP& p) {
    if (p.slices == 0 || p.inner == 0) return;
    const bool vec = (p.inner & 3) == 0 && (p.group_stride & 3) == 0 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15) == 0;
    // (strides[q] are multiples of inner: with inner % 4 == 0 every row offset keeps the 16-byte alignment of the bases)
    const long work = p.slices * (vec ? p.inner / 4 : p.inner);
    const unsigned blocks = (unsigned)std::min<long>((work + 255) / 256, 65535);
    ProfScope ps(s, "gather", 8.0 * (double)p.slices * p.inner + 4.0 * (double)p.slices * p.m, 0.0);
    if (vec) hipLaunchKernelGGL(gather_rows_kernel<4>, dim3(blocks), dim3(256), 0, s, x, idx, y, p);
    else hipLaunchKernelGGL(gather_rows_kernel<1>, dim3(blocks), dim3(256), 0, s, x, idx, y, p);
}

void gather_elements(hipStream_t s, const float* x, const float* idx, float* y, const GatherElemP& p) {
    if (p.total == 0) return;
    const unsigned blocks = (unsigned)std::min<long>((p.total + 255) / 256, 65535);
    ProfScope ps(s, "gather", 12.0 * (double)p.total, 0.0);
    hipLaunchKernelGGL(gather_elements_kernel, dim3(blocks), dim3(256), 0, s, x, idx, y, p);
}

}  // namespace k
}  // namespace oar
