// Gradient accumulation over the flat gradient buffer (mmcv GradientCumulativeOptimizerHook: k backward passes per
// optimizer step, the reference's 8 ranks x 16 clips followed on fewer GPUs).  Two elementwise passes:
//   k_accum<false>   acc += g                                  a micro-iteration (no update follows)
//   k_accum<true>    g = (acc + g) * factor[0];  acc = 0       the stepping iteration: the averaged gradient lands where
//                                                              the all-reduce, the clip and k_sgd / k_sgd_clip read it
// Element i is touched by exactly one thread and every operation is a single rounded fp32 add or multiply: no atomics,
// no reduction, the same bits on every run.  The buffers need not be 16-byte aligned: the elements before the first
// 16-byte boundary (the head) and the n % 4 rest (the tail) go one float at a time, everything between 16 bytes at a time.
#include "common.h"

namespace {

constexpr int AC_NT = 256;
constexpr int AC_VPT = 4;                          // float4 per thread and buffer: 64 B per lane in flight per stream
constexpr int AC_CHUNK = AC_NT * AC_VPT;           // float4 per workgroup and round
constexpr int AC_MAX_BLOCKS = 2048;                // 256 CUs x 8; larger buffers go round the grid-stride loop

template <bool FINISH>
__device__ __forceinline__ void ac_one(float& a, float& gv, float f) {
  if (FINISH) {
    gv = __fmul_rn(__fadd_rn(a, gv), f);
    a = 0.f;
  } else {
    a = __fadd_rn(a, gv);
  }
}

// acc / g: the buffers;  head: elements before the 16-byte body;  n4: float4 of the body;  n: all elements.
// The body is acc + head .. acc + head + 4 * n4 (16-byte aligned in both buffers), the scalar set is the rest.
template <bool FINISH>
__global__ __launch_bounds__(AC_NT) void k_accum(float* __restrict__ acc, float* __restrict__ g,
                                                 const float* __restrict__ factor, long head, long n4, long n) {
  const int tid = threadIdx.x;
  const float f = FINISH ? factor[0] : 1.f;
  f32x4* __restrict__ a4 = reinterpret_cast<f32x4*>(acc + head);
  f32x4* __restrict__ g4 = reinterpret_cast<f32x4*>(g + head);
  for (long base = (long)blockIdx.x * AC_CHUNK; base < n4; base += (long)gridDim.x * AC_CHUNK) {
    const long i0 = base + tid;
    if (base + AC_CHUNK <= n4) {                   // a whole chunk: all loads in flight before the first store
      f32x4 av[AC_VPT], gv[AC_VPT];
#pragma unroll
      for (int k = 0; k < AC_VPT; ++k) {
        av[k] = a4[i0 + k * AC_NT];
        gv[k] = g4[i0 + k * AC_NT];
      }
#pragma unroll
      for (int k = 0; k < AC_VPT; ++k) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float a = av[k][e], x = gv[k][e];
          ac_one<FINISH>(a, x, f);
          av[k][e] = a;
          gv[k][e] = x;
        }
        a4[i0 + k * AC_NT] = av[k];
        if (FINISH) g4[i0 + k * AC_NT] = gv[k];
      }
    } else {                                       // the ragged last chunk
      for (int k = 0; k < AC_VPT; ++k) {
        const long i = i0 + (long)k * AC_NT;
        if (i < n4) {
          f32x4 av = a4[i], gv = g4[i];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float a = av[e], x = gv[e];
            ac_one<FINISH>(a, x, f);
            av[e] = a;
            gv[e] = x;
          }
          a4[i] = av;
          if (FINISH) g4[i] = gv;
        }
      }
    }
  }
  // head and tail: scalar element j of the n - 4 * n4 that the body leaves out
  const long ns = n - 4 * n4;
  for (long j = (long)blockIdx.x * AC_NT + tid; j < ns; j += (long)gridDim.x * AC_NT) {
    const long i = j < head ? j : j + 4 * n4;
    float a = acc[i], x = g[i];
    ac_one<FINISH>(a, x, f);
    acc[i] = a;
    if (FINISH) g[i] = x;
  }
}

// head / n4 of a pair of buffers; both must leave the same distance to a 16-byte boundary for a 16-byte body to exist
inline void ac_split(const float* acc, const float* g, long long n, long* head, long* n4) {
  const uintptr_t ma = (uintptr_t)acc & 15, mg = (uintptr_t)g & 15;
  if (ma != mg) {                                  // no common boundary: every element goes the scalar way
    *head = (long)n;
    *n4 = 0;
    return;
  }
  long h = (long)(((16 - ma) & 15) / 4);
  if (h > n) h = (long)n;
  *head = h;
  *n4 = (long)((n - h) / 4);
}

template <bool FINISH>
int ac_launch(float* acc, float* g, const float* factor, long long n, void* stream) {
  if (!acc || !g || n <= 0 || (FINISH && !factor)) return DSGCN_EINVAL;
  if ((((uintptr_t)acc | (uintptr_t)g | (uintptr_t)factor) & 3)) return DSGCN_EINVAL;
  const uintptr_t a0 = (uintptr_t)acc, g0 = (uintptr_t)g, bytes = (uintptr_t)n * sizeof(float);
  if (a0 < g0 + bytes && g0 < a0 + bytes) return DSGCN_EINVAL;                  // the two ranges overlap
  long head, n4;
  ac_split(acc, g, n, &head, &n4);
  const long ns = (long)n - 4 * n4;
  long blocks = (n4 + AC_CHUNK - 1) / AC_CHUNK;
  const long sblocks = (ns + AC_NT - 1) / AC_NT;
  if (sblocks > blocks) blocks = sblocks;
  if (blocks > AC_MAX_BLOCKS) blocks = AC_MAX_BLOCKS;
  hipLaunchKernelGGL(k_accum<FINISH>, dim3((unsigned)blocks), dim3(AC_NT), 0, (hipStream_t)stream, acc, g, factor, head, n4,
                     (long)n);
  DSGCN_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" {

int dsgcn_grad_accum(float* acc, const float* g, long long n, void* stream) {
  return ac_launch<false>(acc, const_cast<float*>(g), nullptr, n, stream);      // (k_accum<false> only reads g)
}

int dsgcn_grad_accum_finish(float* acc, float* g, const float* factor, long long n, void* stream) {
  return ac_launch<true>(acc, g, factor, n, stream);
}

}  // extern "C"
