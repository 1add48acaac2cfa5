// The head of the training step for the losses beyond unit-weight hard-label cross entropy (csrc/head.hip keeps that one):
// per-class weights, soft labels and multi-label binary cross entropy, in the same three launches.
//   k_htarget_fwd<MODE> / k_htarget_fin / k_htarget_bwd
//       person mean + Linear as k_head_fwd, then per clip a numerator L_n, a denominator D_n and dscore / g:
//       MODE 0  hard label y, class weight w:   L = w_y (logsumexp(s) - s_y)        D = w_y            w_y (p_k - [k = y])
//               (F.cross_entropy(weight=): pyskl/models/losses/cross_entropy_loss.py:76-82) + top-1 / top-5 accuracy
//       MODE 1  soft label q (N, K):            L = -sum_k q_k w_k log p_k          D = sum_k q_k w_k  p_k sum_j q_j w_j - q_k w_k
//               (cross_entropy_loss.py:53-74; without class weights D = 1)
//       MODE 2  multi-label q (N, K):           L = sum_k w_k bce(s_k, q_k)         D = K              w_k (sigmoid(s_k) - q_k)
//               (F.binary_cross_entropy_with_logits(weight=): cross_entropy_loss.py:118-123)
//       loss = loss_weight * sum_n L_n / sum_n D_n (base.py:38-44); the finishing launch leaves sum_n D_n in a one-float
//       device buffer for the backward: g = gloss * loss_weight / sum_n D_n, nothing goes through the host.
// All sums run in a fixed order (no atomics): two launches on the same input give the same bits.
#include "common.h"

namespace {

constexpr int HT_NT = 256;

// One workgroup per clip n.  LDS: pl[C] pooled features, sc[K] scores (the front half is k_head_fwd's, op for op: the
// scores of the two kernels are the same bits).  clip[n] = (L_n, D_n, top-1 hit, top-5 hit); ds[n, k] = dscore / g.
template <int MODE>
__global__ __launch_bounds__(HT_NT) void k_htarget_fwd(const float* __restrict__ feat, const float* __restrict__ w,
                                                       const float* __restrict__ b, const float* __restrict__ cw,
                                                       const void* __restrict__ target, int M, int C, int K, int vec,
                                                       float* __restrict__ pooled, float* __restrict__ score,
                                                       float* __restrict__ ds, float* __restrict__ clip) {
  extern __shared__ float hs[];
  __shared__ float red[4];
  float* pl = hs;
  float* sc = hs + C;
  const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float invM = 1.f / (float)M;
  for (int c = tid; c < C; c += HT_NT) {
    float s = 0.f;
    for (int m = 0; m < M; ++m) s += feat[((size_t)n * M + m) * C + c];
    s *= invM;
    pl[c] = s;
    pooled[(size_t)n * C + c] = s;
  }
  __syncthreads();
  // wave w takes classes w, w + 4, ...: eight of them per pass, all their loads issued before the first product
  for (int k0 = wave; k0 < K; k0 += 32) {
    float a[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] = 0.f;
    if (vec) {
      for (int c = 4 * lane; c < C; c += 256) {
        f32x4 wv[8];
#pragma unroll
        for (int j = 0; j < 8; ++j)
          wv[j] = (k0 + 4 * j < K) ? *reinterpret_cast<const f32x4*>(w + (size_t)(k0 + 4 * j) * C + c) : f32x4{0.f, 0.f, 0.f, 0.f};
        const f32x4 p = *reinterpret_cast<const f32x4*>(pl + c);
#pragma unroll
        for (int j = 0; j < 8; ++j) a[j] += (p.x * wv[j].x + p.y * wv[j].y) + (p.z * wv[j].z + p.w * wv[j].w);
      }
    } else {
      for (int c = lane; c < C; c += 64) {
        float wv[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) wv[j] = (k0 + 4 * j < K) ? w[(size_t)(k0 + 4 * j) * C + c] : 0.f;
        const float p = pl[c];
#pragma unroll
        for (int j = 0; j < 8; ++j) a[j] = fmaf(p, wv[j], a[j]);
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float s = wave_sum(a[j]);
      if (lane == 0 && k0 + 4 * j < K) sc[k0 + 4 * j] = s + (b ? b[k0 + 4 * j] : 0.f);
    }
  }
  __syncthreads();
  float* __restrict__ srow = score + (size_t)n * K;
  float* __restrict__ drow = ds + (size_t)n * K;
  if (MODE == 2) {
    const float* __restrict__ q = reinterpret_cast<const float*>(target) + (size_t)n * K;
    float part = 0.f;
    for (int k = tid; k < K; k += HT_NT) {
      const float s = sc[k], qk = q[k], wk = cw ? cw[k] : 1.f;
      const float e = expf(-fabsf(s));                              // in (0, 1]: neither branch below overflows
      part += wk * ((fmaxf(s, 0.f) - s * qk) + log1pf(e));
      const float sg = s >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
      srow[k] = s;
      drow[k] = wk * (sg - qk);
    }
    part = block_sum(part, red, tid);
    if (tid == 0) {
      clip[n * 4 + 0] = part;
      clip[n * 4 + 1] = (float)K;
      clip[n * 4 + 2] = 0.f;
      clip[n * 4 + 3] = 0.f;
    }
    return;
  }
  float mx = -__builtin_inff();
  for (int k = tid; k < K; k += HT_NT) mx = fmaxf(mx, sc[k]);
  mx = block_max(mx, red, tid);
  float se = 0.f;
  for (int k = tid; k < K; k += HT_NT) se += expf(sc[k] - mx);
  se = block_sum(se, red, tid);
  const float inv = 1.f / se, lse = logf(se) + mx;
  if (MODE == 0) {
    const long long lb = reinterpret_cast<const long long*>(target)[n];
    const bool valid = lb >= 0 && lb < K;
    const float nan = __builtin_nanf("");
    const float sl = valid ? sc[lb] : nan;
    const float wy = valid ? (cw ? cw[lb] : 1.f) : nan;             // (the weight of a label outside [0, K) is never read)
    float rk = 0.f;
    for (int k = tid; k < K; k += HT_NT) {
      const float s = sc[k];
      rk += (s > sl || (s == sl && k > lb)) ? 1.f : 0.f;
      srow[k] = s;
      drow[k] = wy * (expf(s - mx) * inv - (k == lb ? 1.f : 0.f));
    }
    rk = block_sum(rk, red, tid);
    if (tid == 0) {
      clip[n * 4 + 0] = wy * (lse - sl);
      clip[n * 4 + 1] = wy;
      clip[n * 4 + 2] = (valid && rk < 1.f) ? 1.f : 0.f;
      clip[n * 4 + 3] = (valid && rk < 5.f) ? 1.f : 0.f;
    }
  } else {
    const float* __restrict__ q = reinterpret_cast<const float*>(target) + (size_t)n * K;
    float part = 0.f, qs = 0.f;
    for (int k = tid; k < K; k += HT_NT) {
      const float qw = q[k] * (cw ? cw[k] : 1.f);
      part = fmaf(qw, lse - sc[k], part);
      qs += qw;
    }
    part = block_sum(part, red, tid);
    qs = block_sum(qs, red, tid);
    for (int k = tid; k < K; k += HT_NT) {
      const float s = sc[k];
      srow[k] = s;
      drow[k] = fmaf(expf(s - mx) * inv, qs, -(q[k] * (cw ? cw[k] : 1.f)));
    }
    if (tid == 0) {
      clip[n * 4 + 0] = part;
      clip[n * 4 + 1] = cw ? qs : 1.f;
      clip[n * 4 + 2] = 0.f;
      clip[n * 4 + 3] = 0.f;
    }
  }
}

// loss = loss_weight * sum_n L_n / sum_n D_n (f32; 0 / 0 = NaN as F.cross_entropy), den = sum_n D_n (f32), acc = mean_n
// hits (f64, when asked for): one wave, fp64, fixed order
__global__ __launch_bounds__(64) void k_htarget_fin(const float* __restrict__ clip, int N, float loss_weight,
                                                    float* __restrict__ loss, float* __restrict__ den,
                                                    double* __restrict__ acc) {
  double s0 = 0., s1 = 0., s2 = 0., s3 = 0.;
  for (int n = threadIdx.x; n < N; n += 64) {
    s0 += (double)clip[n * 4];
    s1 += (double)clip[n * 4 + 1];
    s2 += (double)clip[n * 4 + 2];
    s3 += (double)clip[n * 4 + 3];
  }
  s0 = wave_sum_d(s0); s1 = wave_sum_d(s1); s2 = wave_sum_d(s2); s3 = wave_sum_d(s3);
  if (threadIdx.x == 0) {
    loss[0] = (float)((double)loss_weight * s0 / s1);
    den[0] = (float)s1;
    if (acc) {
      acc[0] = s2 / N;
      acc[1] = s3 / N;
    }
  }
}

// Blocks [0, N): dfeat rows of clip n (every person gets dpooled / M);  blocks [N, N + K): row k of dW and db[k].
// dscore[n, k] = ds[n, k] * gloss * loss_weight / den.
__global__ __launch_bounds__(HT_NT) void k_htarget_bwd(const float* __restrict__ ds, const float* __restrict__ pooled,
                                                       const float* __restrict__ w, const float* __restrict__ gloss,
                                                       const float* __restrict__ den, float loss_weight, int N, int M, int C,
                                                       int K, float* __restrict__ dfeat, float* __restrict__ dw,
                                                       float* __restrict__ db) {
  extern __shared__ float hs[];
  __shared__ float red[4];
  const int tid = threadIdx.x;
  const float g = gloss[0] * loss_weight / den[0];
  if ((int)blockIdx.x < N) {
    const int n = blockIdx.x;
    for (int k = tid; k < K; k += HT_NT) hs[k] = ds[(size_t)n * K + k] * g;
    __syncthreads();
    const float invM = 1.f / (float)M;
    for (int c = tid; c < C; c += HT_NT) {
      float a0 = 0.f, a1 = 0.f;
      int k = 0;
      for (; k + 1 < K; k += 2) {
        a0 = fmaf(hs[k], w[(size_t)k * C + c], a0);
        a1 = fmaf(hs[k + 1], w[(size_t)(k + 1) * C + c], a1);
      }
      if (k < K) a0 = fmaf(hs[k], w[(size_t)k * C + c], a0);
      const float d = (a0 + a1) * invM;
      for (int m = 0; m < M; ++m) dfeat[((size_t)n * M + m) * C + c] = d;
    }
  } else {
    const int k = blockIdx.x - N;
    float part = 0.f;
    for (int n = tid; n < N; n += HT_NT) {
      const float d = ds[(size_t)n * K + k] * g;
      hs[n] = d;
      part += d;
    }
    part = block_sum(part, red, tid);                               // (its barriers also publish hs)
    if (tid == 0) db[k] = part;
    for (int c = tid; c < C; c += HT_NT) {
      float a0 = 0.f, a1 = 0.f;
      int n = 0;
      for (; n + 1 < N; n += 2) {
        a0 = fmaf(hs[n], pooled[(size_t)n * C + c], a0);
        a1 = fmaf(hs[n + 1], pooled[(size_t)(n + 1) * C + c], a1);
      }
      if (n < N) a0 = fmaf(hs[n], pooled[(size_t)n * C + c], a0);
      dw[(size_t)k * C + c] = a0 + a1;
    }
  }
}

}  // namespace

extern "C" {

int dsgcn_head_target_fwd(const float* feat, const float* w, const float* b, const float* class_weight, const void* target,
                          int mode, int N, int M, int C, int K, float loss_weight, float* pooled, float* score,
                          float* dscore, float* clip, float* loss, float* den, double* acc, void* stream) {
  if (!feat || !w || !target || !pooled || !score || !dscore || !clip || !loss || !den || N <= 0 || M <= 0 || C <= 0 ||
      K <= 0 || mode < 0 || mode > 2 || (mode == 0 && !acc))
    return DSGCN_EINVAL;
  const size_t lds = (size_t)(C + K) * sizeof(float);
  if (lds > 60 * 1024) return DSGCN_EUNSUPPORTED;
  const int vec = (C & 3) == 0 && ((uintptr_t)w & 15) == 0;
  const dim3 grid((unsigned)N), block(HT_NT);
  hipStream_t st = (hipStream_t)stream;
  if (mode == 0)
    hipLaunchKernelGGL(k_htarget_fwd<0>, grid, block, lds, st, feat, w, b, class_weight, target, M, C, K, vec, pooled, score,
                       dscore, clip);
  else if (mode == 1)
    hipLaunchKernelGGL(k_htarget_fwd<1>, grid, block, lds, st, feat, w, b, class_weight, target, M, C, K, vec, pooled, score,
                       dscore, clip);
  else
    hipLaunchKernelGGL(k_htarget_fwd<2>, grid, block, lds, st, feat, w, b, class_weight, target, M, C, K, vec, pooled, score,
                       dscore, clip);
  DSGCN_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_htarget_fin, dim3(1), dim3(64), 0, st, clip, N, loss_weight, loss, den, mode == 0 ? acc : nullptr);
  DSGCN_LAUNCH_CHECK();
  return 0;
}

int dsgcn_head_target_bwd(const float* dscore, const float* pooled, const float* w, const float* gloss, const float* den,
                          int N, int M, int C, int K, float loss_weight, float* dfeat, float* dw, float* db, void* stream) {
  if (!dscore || !pooled || !w || !gloss || !den || !dfeat || !dw || !db || N <= 0 || M <= 0 || C <= 0 || K <= 0)
    return DSGCN_EINVAL;
  const size_t lds = (size_t)(K > N ? K : N) * sizeof(float);
  if (lds > 60 * 1024) return DSGCN_EUNSUPPORTED;
  hipLaunchKernelGGL(k_htarget_bwd, dim3((unsigned)(N + K)), dim3(HT_NT), lds, (hipStream_t)stream, dscore, pooled, w, gloss,
                     den, loss_weight, N, M, C, K, dfeat, dw, db);
  DSGCN_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
