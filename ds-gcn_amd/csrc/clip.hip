// Gradient clipping by total norm, folded into the optimizer launch (mmcv OptimizerHook.clip_grads =
// torch.nn.utils.clip_grad_norm_ before optimizer.step(); configs/_init_/lr_schedual.py:24 carries
// grad_clip=dict(max_norm=45, norm_type=2) beside the active grad_clip=None).  The gradients already lie in one flat
// buffer, so the norm is one extra read of it:
//   k_grad_norm   workgroup r reduces the fixed slice [r * GN_SLICE, (r + 1) * GN_SLICE) of g in fp64 -> partial[r]
//                 (L2: sum of g*g, every square exact in fp64;  inf: max |g|)
//   k_sgd_clip    every workgroup reduces the partial rows in the same fixed order (so all of them hold the same
//                 coefficient), then runs k_sgd's update (head.hip) on g * coef and writes g * coef back
// Fixed grids, fixed order, no atomics: the same bits on every run and every box.
#include "common.h"
#include "grad_norm.h"
#include "sgd_update.h"

namespace {

constexpr int GN_VPT = 8;                          // float4 per thread of a norm slice
constexpr int GN_SLICE = GN_NT * GN_VPT * 4;       // elements per workgroup: 8192 (32 KB)
constexpr int SC_VPT = 4;                          // float4 per thread of the update

// thread t of workgroup r takes the float4s t, t + 256, ... of the slice, elements in ascending order
template <bool INF>
__global__ __launch_bounds__(GN_NT) void k_grad_norm(const float* __restrict__ g, long n, double* __restrict__ partial) {
  __shared__ double red[GN_NT];
  const int tid = threadIdx.x;
  const long base = (long)blockIdx.x * GN_SLICE;
  double a = 0.;
  if (base + GN_SLICE <= n) {                      // a whole slice: all loads in flight before the first term
    const f32x4* __restrict__ g4 = reinterpret_cast<const f32x4*>(g + base);
    f32x4 v[GN_VPT];
#pragma unroll
    for (int k = 0; k < GN_VPT; ++k) v[k] = g4[k * GN_NT + tid];
#pragma unroll
    for (int k = 0; k < GN_VPT; ++k)
#pragma unroll
      for (int e = 0; e < 4; ++e) a = gn_term<INF>(a, v[k][e]);
  } else {                                         // the ragged last slice: same assignment of elements to threads
    for (int k = 0; k < GN_VPT; ++k) {
      const long j0 = base + 4L * (k * GN_NT + tid);
      for (int e = 0; e < 4; ++e)
        if (j0 + e < n) a = gn_term<INF>(a, g[j0 + e]);
    }
  }
  a = gn_block<INF>(a, red, tid);
  if (tid == 0) partial[blockIdx.x] = a;
}

// k_sgd (head.hip) on g * coef.  coef == 1: the product is g itself, p and buf come out as k_sgd leaves them.
__device__ __forceinline__ void sgd_clip_flat(float* __restrict__ p, float* __restrict__ g, float* __restrict__ buf,
                                              const float* __restrict__ lr, const double* __restrict__ partial, int rows,
                                              int inf, float max_norm, float* __restrict__ grad_norm, float mom, float wd,
                                              int nesterov, long n4, long n, double* red) {
  const int tid = threadIdx.x;
  float total;
  // torch.nn.utils.clip_grad_norm_: clip_coef = max_norm / (total_norm + 1e-6), clamped to 1
  const float coef = gn_clip_coef(partial, rows, inf, max_norm, red, tid, total);
  if (blockIdx.x == 0 && tid == 0) grad_norm[0] = total;
  const float rate = lr[0];
  auto one = [&](float pv, float gv, float& bv) { return sgd_update(pv, gv, bv, buf != nullptr, rate, mom, wd, nesterov); };
  const long i0 = (long)blockIdx.x * (GN_NT * SC_VPT) + tid;
  if (i0 + (SC_VPT - 1) * GN_NT < n4) {            // all SC_VPT float4 of this thread exist: loads first
    f32x4 pv[SC_VPT], gv[SC_VPT], bv[SC_VPT];
#pragma unroll
    for (int k = 0; k < SC_VPT; ++k) {
      pv[k] = reinterpret_cast<f32x4*>(p)[i0 + k * GN_NT];
      gv[k] = reinterpret_cast<f32x4*>(g)[i0 + k * GN_NT];
      bv[k] = buf ? reinterpret_cast<f32x4*>(buf)[i0 + k * GN_NT] : f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int k = 0; k < SC_VPT; ++k) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float be = bv[k][e];
        gv[k][e] = __fmul_rn(gv[k][e], coef);      // rounded on its own: never fused into the weight-decay add
        pv[k][e] = one(pv[k][e], gv[k][e], be);
        bv[k][e] = be;
      }
      reinterpret_cast<f32x4*>(p)[i0 + k * GN_NT] = pv[k];
      reinterpret_cast<f32x4*>(g)[i0 + k * GN_NT] = gv[k];
      if (buf) reinterpret_cast<f32x4*>(buf)[i0 + k * GN_NT] = bv[k];
    }
    return;
  }
  for (int k = 0; k < SC_VPT; ++k) {
    const long i = i0 + (long)k * GN_NT;
    if (i < n4) {
      f32x4 pv = reinterpret_cast<f32x4*>(p)[i];
      f32x4 gv = reinterpret_cast<f32x4*>(g)[i];
      f32x4 bv = buf ? reinterpret_cast<f32x4*>(buf)[i] : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float be = bv[e];
        gv[e] = __fmul_rn(gv[e], coef);
        pv[e] = one(pv[e], gv[e], be);
        bv[e] = be;
      }
      reinterpret_cast<f32x4*>(p)[i] = pv;
      reinterpret_cast<f32x4*>(g)[i] = gv;
      if (buf) reinterpret_cast<f32x4*>(buf)[i] = bv;
    } else if (i == n4) {                          // the tail (n % 4 elements)
      for (long j = 4 * n4; j < n; ++j) {
        float bv = buf ? buf[j] : 0.f;
        const float gc = __fmul_rn(g[j], coef);
        p[j] = one(p[j], gc, bv);
        g[j] = gc;
        if (buf) buf[j] = bv;
      }
    }
  }
}

__global__ __launch_bounds__(GN_NT) void k_sgd_clip(float* __restrict__ p, float* __restrict__ g, float* __restrict__ buf,
                                                    const float* __restrict__ lr, const double* __restrict__ partial,
                                                    int rows, int inf, float max_norm, float* __restrict__ grad_norm,
                                                    float mom, float wd, int nesterov, long n4, long n) {
  __shared__ double red[GN_NT];
  sgd_clip_flat(p, g, buf, lr, partial, rows, inf, max_norm, grad_norm, mom, wd, nesterov, n4, n, red);
}

// k_sgd_clip with the momentum read on the device (head.hip k_sgd_hyper: one scalar load per wave; 0 leaves buf alone)
__global__ __launch_bounds__(GN_NT) void k_sgd_clip_hyper(float* __restrict__ p, float* __restrict__ g,
                                                          float* __restrict__ buf, const float* __restrict__ lr,
                                                          const double* __restrict__ partial, int rows, int inf,
                                                          float max_norm, float* __restrict__ grad_norm,
                                                          const double* __restrict__ hyper, float wd, int nesterov,
                                                          long n4, long n) {
  __shared__ double red[GN_NT];
  const float mom = uniform_f32((float)hyper[0]);
  sgd_clip_flat(p, g, mom != 0.f ? buf : nullptr, lr, partial, rows, inf, max_norm, grad_norm, mom, wd, nesterov, n4, n,
                red);
}

}  // namespace

extern "C" {

int dsgcn_grad_norm_rows(long long n) {
  if (n <= 0) return DSGCN_EINVAL;
  const long long rows = (n + GN_SLICE - 1) / GN_SLICE;
  if (rows > 0x7fffffffLL) return DSGCN_EUNSUPPORTED;
  return (int)rows;
}

int dsgcn_grad_norm_partials(const float* g, long long n, int norm_type, double* partial, void* stream) {
  if (!g || !partial || n <= 0 || (norm_type != 0 && norm_type != 2)) return DSGCN_EINVAL;
  if (((uintptr_t)g & 15) || ((uintptr_t)partial & 7)) return DSGCN_EINVAL;
  const int rows = dsgcn_grad_norm_rows(n);
  if (rows < 0) return rows;
  if (norm_type == 0)
    hipLaunchKernelGGL(k_grad_norm<true>, dim3((unsigned)rows), dim3(GN_NT), 0, (hipStream_t)stream, g, (long)n, partial);
  else
    hipLaunchKernelGGL(k_grad_norm<false>, dim3((unsigned)rows), dim3(GN_NT), 0, (hipStream_t)stream, g, (long)n, partial);
  DSGCN_LAUNCH_CHECK();
  return 0;
}

int dsgcn_sgd_step_clip(float* p, float* g, float* buf, const float* lr, const double* partial, int rows, int norm_type,
                        float max_norm, float* grad_norm_out, float momentum, float weight_decay, int nesterov,
                        long long n, void* stream) {
  if (!p || !g || !lr || !partial || !grad_norm_out || n <= 0 || rows <= 0 || (momentum != 0.f && !buf))
    return DSGCN_EINVAL;
  if ((norm_type != 0 && norm_type != 2) || !(max_norm >= 0.f)) return DSGCN_EINVAL;
  if ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)buf) & 15) || ((uintptr_t)partial & 7)) return DSGCN_EINVAL;
  const long n4 = (long)(n / 4);
  const long per = (long)GN_NT * SC_VPT;
  const long blocks = (n4 + 1 + per - 1) / per;
  if (blocks > 0x7fffffffL) return DSGCN_EUNSUPPORTED;
  hipLaunchKernelGGL(k_sgd_clip, dim3((unsigned)blocks), dim3(GN_NT), 0, (hipStream_t)stream, p, g,
                     momentum != 0.f ? buf : nullptr, lr, partial, rows, norm_type == 0 ? 1 : 0, max_norm, grad_norm_out,
                     momentum, weight_decay, nesterov, n4, (long)n);
  DSGCN_LAUNCH_CHECK();
  return 0;
}

int dsgcn_sgd_step_clip_hyper(float* p, float* g, float* buf, const float* lr, const double* partial, int rows,
                              int norm_type, float max_norm, float* grad_norm_out, const double* hyper, float weight_decay,
                              int nesterov, long long n, void* stream) {
  if (!p || !g || !buf || !lr || !partial || !grad_norm_out || !hyper || n <= 0 || rows <= 0) return DSGCN_EINVAL;
  if ((norm_type != 0 && norm_type != 2) || !(max_norm >= 0.f)) return DSGCN_EINVAL;
  if ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)buf) & 15) || (((uintptr_t)partial | (uintptr_t)hyper) & 7))
    return DSGCN_EINVAL;
  const long n4 = (long)(n / 4);
  const long per = (long)GN_NT * SC_VPT;
  const long blocks = (n4 + 1 + per - 1) / per;
  if (blocks > 0x7fffffffL) return DSGCN_EUNSUPPORTED;
  hipLaunchKernelGGL(k_sgd_clip_hyper, dim3((unsigned)blocks), dim3(GN_NT), 0, (hipStream_t)stream, p, g, buf, lr, partial,
                     rows, norm_type == 0 ? 1 : 0, max_norm, grad_norm_out, hyper, weight_decay, nesterov, n4, (long)n);
  DSGCN_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
