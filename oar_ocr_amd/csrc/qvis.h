// qvis.h -- the launchers of qvis_misc.hip: the steps the Qwen2-VL / Qwen2.5-VL vision towers need beyond the SigLIP chain.  Kept out of
// kernels.h so that no other translation unit sees a changed header.  All three are bandwidth kernels: 16-byte accesses, no atomics (two runs give the
// same bytes), nothing outside the rows given is read or written.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace oar {
namespace k {

enum QvisAct : int { QVIS_QUICK_GELU = 0, QVIS_SILU = 1, QVIS_GELU_ERF = 2 };   // x sigmoid(1.702 x); x sigmoid(x); the erf GELU through the implicit-GEMM epilogue's erf_rational
inline bool qvis_act_known(int act) { return act == QVIS_QUICK_GELU || act == QVIS_SILU || act == QVIS_GELU_ERF; }

// y [T][D] = x[t] / sqrt(mean(x[t]^2) + eps) * g.  D % 4 == 0, all pointers 16-byte aligned; one wave per row, the sum of squares in a fixed order (a lane's
// float4s in turn, then a butterfly over the 64 lanes).  y may be x.  prof_class: the profiler class the launch is counted under (null: "qvis_rmsnorm").
void qvis_rmsnorm(hipStream_t s, const float* x, const float* g, float* y, int64_t rows, int D, float eps, const char* prof_class = nullptr);
// gated == 0: out [T][F] = act(in [T][F]) (out may be in).  gated != 0: in is the stacked gate / up result [T][2 F], out [T][F] = act(in[t][f]) in[t][F + f];
// out must not overlap in.  F % 4 == 0, both pointers 16-byte aligned.
void qvis_act(hipStream_t s, const float* in, float* out, int64_t rows, int F, int act, int gated, const char* prof_class = nullptr);
// out [n_rows][row_floats] = in[idx[r]] row by row; row_floats % 4 == 0, idx [n_rows] on the device with every entry in [0, n_in_rows) (entries outside copy
// nothing: the launcher's callers check the table on the host, the kernel guards the read all the same).  out must not overlap in.
void qvis_row_gather(hipStream_t s, const float* in, const int32_t* idx, float* out, int64_t n_rows, int64_t n_in_rows, int row_floats, const char* prof_class = nullptr);

}  // namespace k
}  // namespace oar
