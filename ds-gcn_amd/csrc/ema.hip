// Exponential moving average of the weights over the flat parameter buffer (mmcv's EMAHook), and the in-place exchange of
// two flat buffers that puts the averaged weights under the model at an epoch end and takes them out again.
//   k_ema    m = hyper[0] (ONE fp64 value in device memory), mf = (float)m, nf = (float)(1 - m), both rounded once:
//              m == 0          ema is neither read nor written (a gated-off iteration: bit-unchanged, whatever p holds)
//              nf == 0         ema[i] = p[i]                              (m == 1: a copy, whatever ema held)
//              otherwise       ema[i] = fmaf(mf, p[i], nf * ema[i])       one rounded product, one fused multiply-add
//            Against the exact (1 - m) ema + m p one update is off by at most 4 * 2^-24 * max(|ema|, |p|): the roundings of
//            mf and nf, the product and the sum.
//   k_swap   a[i] <-> b[i]
// Element i is touched by exactly one thread: no atomics, no reduction, the same bits on every run and on an eager launch
// as on a replayed one.  The value of m is read by the kernel, so a launch captured in a hipGraph follows the hook's
// warm-up and its interval gating on replay.  The buffers need 4-byte alignment only: the elements before the first
// 16-byte boundary (the head) and the n % 4 rest (the tail) go one float at a time, everything between 16 bytes at a time.
#include "common.h"

namespace {

constexpr int EM_NT = 256;
constexpr int EM_VPT = 4;                          // float4 per thread and buffer: 64 B per lane in flight per stream
constexpr int EM_CHUNK = EM_NT * EM_VPT;           // float4 per workgroup and round
constexpr int EM_BLOCKS_PER_CU = 8;                // larger buffers go round the grid-stride loop

enum { EM_EMA = 0, EM_COPY = 1, EM_SWAP = 2 };

// a: ema (or the first buffer of a swap), b: p (or the second)
template <int OP>
__device__ __forceinline__ void em_one(float& a, float& b, float mf, float nf) {
  if (OP == EM_EMA) {
    a = fmaf(mf, b, __fmul_rn(nf, a));
  } else if (OP == EM_COPY) {
    a = b;
  } else {
    const float t = a;
    a = b;
    b = t;
  }
}

// head: elements before the 16-byte body;  n4: float4 of the body;  n: all elements.  The body is a + head ..
// a + head + 4 * n4 (16-byte aligned in both buffers), the scalar set is the rest.
template <int OP>
__device__ __forceinline__ void em_pass(float* __restrict__ a, float* __restrict__ b, float mf, float nf, long head, long n4,
                                        long n) {
  const int tid = threadIdx.x;
  f32x4* __restrict__ a4 = reinterpret_cast<f32x4*>(a + head);
  f32x4* __restrict__ b4 = reinterpret_cast<f32x4*>(b + head);
  for (long base = (long)blockIdx.x * EM_CHUNK; base < n4; base += (long)gridDim.x * EM_CHUNK) {
    const long i0 = base + tid;
    if (base + EM_CHUNK <= n4) {                   // a whole chunk: all loads in flight before the first store
      f32x4 av[EM_VPT], bv[EM_VPT];
#pragma unroll
      for (int k = 0; k < EM_VPT; ++k) {
        if (OP != EM_COPY) av[k] = a4[i0 + k * EM_NT];
        bv[k] = b4[i0 + k * EM_NT];
      }
#pragma unroll
      for (int k = 0; k < EM_VPT; ++k) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float x = OP != EM_COPY ? av[k][e] : 0.f, y = bv[k][e];
          em_one<OP>(x, y, mf, nf);
          av[k][e] = x;
          bv[k][e] = y;
        }
        a4[i0 + k * EM_NT] = av[k];
        if (OP == EM_SWAP) b4[i0 + k * EM_NT] = bv[k];
      }
    } else {                                       // the ragged last chunk
      for (int k = 0; k < EM_VPT; ++k) {
        const long i = i0 + (long)k * EM_NT;
        if (i < n4) {
          f32x4 av, bv = b4[i];
          if (OP != EM_COPY) av = a4[i];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float x = OP != EM_COPY ? av[e] : 0.f, y = bv[e];
            em_one<OP>(x, y, mf, nf);
            av[e] = x;
            bv[e] = y;
          }
          a4[i] = av;
          if (OP == EM_SWAP) b4[i] = bv;
        }
      }
    }
  }
  // head and tail: scalar element j of the n - 4 * n4 that the body leaves out
  const long ns = n - 4 * n4;
  for (long j = (long)blockIdx.x * EM_NT + tid; j < ns; j += (long)gridDim.x * EM_NT) {
    const long i = j < head ? j : j + 4 * n4;
    float x = OP != EM_COPY ? a[i] : 0.f, y = b[i];
    em_one<OP>(x, y, mf, nf);
    a[i] = x;
    if (OP == EM_SWAP) b[i] = y;
  }
}

__global__ __launch_bounds__(EM_NT) void k_ema(float* __restrict__ ema, const float* __restrict__ p,
                                               const double* __restrict__ hyper, long head, long n4, long n) {
  const double m = hyper[0];                       // wave-uniform: every branch below is taken by the whole launch
  if (m == 0.0) return;
  const float mf = (float)m, nf = (float)(1.0 - m);
  float* pw = const_cast<float*>(p);               // (only EM_SWAP writes its second buffer)
  if (nf == 0.f) em_pass<EM_COPY>(ema, pw, mf, nf, head, n4, n);
  else em_pass<EM_EMA>(ema, pw, mf, nf, head, n4, n);
}

__global__ __launch_bounds__(EM_NT) void k_swap(float* __restrict__ a, float* __restrict__ b, long head, long n4, long n) {
  em_pass<EM_SWAP>(a, b, 0.f, 0.f, head, n4, n);
}

// head / n4 of a pair of buffers; both must leave the same distance to a 16-byte boundary for a 16-byte body to exist
inline void em_split(const float* a, const float* b, long long n, long* head, long* n4) {
  const uintptr_t ma = (uintptr_t)a & 15, mb = (uintptr_t)b & 15;
  if (ma != mb) {                                  // no common boundary: every element goes the scalar way
    *head = (long)n;
    *n4 = 0;
    return;
  }
  long h = (long)(((16 - ma) & 15) / 4);
  if (h > n) h = (long)n;
  *head = h;
  *n4 = (long)((n - h) / 4);
}

// EM_BLOCKS_PER_CU workgroups per compute unit of the CURRENT device (256 CUs when the runtime cannot say), looked up
// once per device of the process
long em_max_blocks() {
  constexpr int MAX_DEV = 64;
  static int cus[MAX_DEV] = {};                    // (a benign race: every thread stores the same value in a slot)
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) {
    (void)hipGetLastError();
    return 256L * EM_BLOCKS_PER_CU;
  }
  const bool slot = dev >= 0 && dev < MAX_DEV;
  int v = slot ? cus[dev] : 0;
  if (v == 0) {
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) {
      (void)hipGetLastError();
      v = 256;
    }
    if (slot) cus[dev] = v;
  }
  return (long)v * EM_BLOCKS_PER_CU;
}

// argument checks shared by the two entry points -> 0, or the error code; n == 0 is the caller's no-op
int em_check(const float* a, const float* b, long long n) {
  if (!a || !b || n < 0) return DSGCN_EINVAL;
  if ((((uintptr_t)a | (uintptr_t)b) & 3)) return DSGCN_EINVAL;
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b, bytes = (uintptr_t)n * sizeof(float);
  if (n > 0 && a0 < b0 + bytes && b0 < a0 + bytes) return DSGCN_EINVAL;         // the two ranges overlap
  return 0;
}

long em_grid(long n4, long ns) {
  long blocks = (n4 + EM_CHUNK - 1) / EM_CHUNK;
  const long sblocks = (ns + EM_NT - 1) / EM_NT;
  if (sblocks > blocks) blocks = sblocks;
  const long top = em_max_blocks();
  return blocks > top ? top : blocks;
}

}  // namespace

extern "C" {

int dsgcn_ema_update(float* ema, const float* p, long long n, const double* hyper, void* stream) {
  if (!hyper || ((uintptr_t)hyper & 7)) return DSGCN_EINVAL;
  const int rc = em_check(ema, p, n);
  if (rc != 0 || n == 0) return rc;
  long head, n4;
  em_split(ema, p, n, &head, &n4);
  const long blocks = em_grid(n4, (long)n - 4 * n4);
  hipLaunchKernelGGL(k_ema, dim3((unsigned)blocks), dim3(EM_NT), 0, (hipStream_t)stream, ema, p, hyper, head, n4, (long)n);
  DSGCN_LAUNCH_CHECK();
  return 0;
}

int dsgcn_ema_swap(float* a, float* b, long long n, void* stream) {
  const int rc = em_check(a, b, n);
  if (rc != 0 || n == 0) return rc;
  long head, n4;
  em_split(a, b, n, &head, &n4);
  const long blocks = em_grid(n4, (long)n - 4 * n4);
  hipLaunchKernelGGL(k_swap, dim3((unsigned)blocks), dim3(EM_NT), 0, (hipStream_t)stream, a, b, head, n4, (long)n);
  DSGCN_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
