// The total gradient norm out of the partial rows of k_grad_norm (clip.hip), shared by the update kernels that clip
// (k_sgd_clip in clip.hip, the grouped SGD and Adam kernels in optim.hip): every workgroup reduces the rows in the same
// fixed order, so all of them hold the same total and the same coefficient.
#pragma once

namespace {

constexpr int GN_NT = 256;

// INF: max that keeps a NaN (torch's max does);  else: sum
template <bool INF>
__device__ __forceinline__ double gn_comb(double a, double b) {
  if (INF) return (a > b || a != a) ? a : b;
  return a + b;
}

template <bool INF>
__device__ __forceinline__ double gn_term(double a, float x) {
  const double v = (double)x;
  if (INF) return gn_comb<true>(a, fabs(v));
  return fma(v, v, a);                             // v * v is exact in fp64: this is a + v*v rounded once
}

// all threads get the combination of the 256 values, in the order of a binary LDS tree
template <bool INF>
__device__ __forceinline__ double gn_block(double v, double* red, int tid) {
  red[tid] = v;
  __syncthreads();
#pragma unroll
  for (int s = GN_NT / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] = gn_comb<INF>(red[tid], red[tid + s]);
    __syncthreads();
  }
  return red[0];
}

// -> clip_grad_norm_'s coefficient min(1, max_norm / (total + 1e-6)) in fp32; total: the norm before clipping, in fp32
__device__ __forceinline__ float gn_clip_coef(const double* __restrict__ partial, int rows, int inf, float max_norm,
                                              double* red, int tid, float& total) {
  double a = 0.;
  if (inf) {
    for (long r = tid; r < rows; r += GN_NT) a = gn_comb<true>(a, partial[r]);
    total = (float)gn_block<true>(a, red, tid);
  } else {
    for (long r = tid; r < rows; r += GN_NT) a = gn_comb<false>(a, partial[r]);
    total = (float)sqrt(gn_block<false>(a, red, tid));
  }
  return fminf(1.f, max_norm / (total + 1e-6f));
}

}  // namespace
