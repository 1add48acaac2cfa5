// The arithmetic of the test-time head for ONE video of ONE model, shared by csrc/head_test.hip (one model per launch) and
// csrc/head_ensemble.hip (several models' heads through the same LDS, one after another): both launches run this code, so
// a stream's row of the ensemble launch has the bits of the single launch.
#pragma once
#include "common.h"

constexpr int HT_NT = 256;        // four waves
constexpr int HT_J = 8;           // classes a wave has in flight per pass

// the LDS a video takes: pl[clips][C] + sc[clips][K]
__host__ __device__ inline size_t ht_lds_bytes(int clips, int C, int K) {
  return (size_t)clips * ((size_t)C + (size_t)K) * sizeof(float);
}

// LDS: pl[clips][C] pooled features, sc[clips][K] scores (mode 0: overwritten by the probabilities).
//   pl[q, c] = (1/M) sum_m feat[((n*clips + q)*M + m), c]
//   sc[q, k] = <pl[q], W[k]> + b[k]      wave w takes classes w, w + 4, ...: HT_J of them per pass, lanes split C; the
//                                         weight loads of a pass are all issued before the first product
//   mode 0: sc[q] <- softmax_k(sc[q])    (a wave per clip: max, denominator, in lane-strided order)
// On return (every thread of the workgroup, behind a barrier) sc holds what the clip mean is taken of; mode 2 returns
// after clip_score.  VEC: C % 4 == 0 and w 16-byte aligned: 16-byte loads of the weight rows and of pl.
template <bool VEC>
__device__ __forceinline__ void ht_video_scores(const float* __restrict__ feat, const float* __restrict__ w,
                                                const float* __restrict__ b, int n, int clips, int M, int C, int K,
                                                int mode, float* __restrict__ clip_score, float* pl, float* sc) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float invM = 1.f / (float)M;
  const float* __restrict__ fn = feat + (size_t)n * clips * M * C;
  for (int i = tid; i < clips * C; i += HT_NT) {
    const int q = i / C, c = i - q * C;
    float s = 0.f;
    for (int m = 0; m < M; ++m) s += fn[((size_t)q * M + m) * C + c];
    pl[i] = s * invM;
  }
  __syncthreads();
  constexpr int CW = VEC ? 256 : 64;                      // channels a wave covers per chunk
  for (int k0 = wave; k0 < K; k0 += 4 * HT_J) {
    for (int cb = 0; cb < C; cb += CW) {
      const int c = cb + (VEC ? 4 * lane : lane);
      const bool in = c < C;
      f32x4 wv[HT_J];
#pragma unroll
      for (int j = 0; j < HT_J; ++j) {
        const int k = k0 + 4 * j;
        wv[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (in && k < K) {
          if (VEC) wv[j] = *reinterpret_cast<const f32x4*>(w + (size_t)k * C + c);
          else wv[j].x = w[(size_t)k * C + c];
        }
      }
      for (int q = 0; q < clips; ++q) {
        f32x4 p = f32x4{0.f, 0.f, 0.f, 0.f};
        if (in) {
          if (VEC) p = *reinterpret_cast<const f32x4*>(pl + (size_t)q * C + c);
          else p.x = pl[(size_t)q * C + c];
        }
#pragma unroll
        for (int j = 0; j < HT_J; ++j) {
          const int k = k0 + 4 * j;
          const float a = VEC ? (p.x * wv[j].x + p.y * wv[j].y) + (p.z * wv[j].z + p.w * wv[j].w) : p.x * wv[j].x;
          const float s = wave_sum(a);
          // chunk 0 starts the score at the bias, later chunks add to it: one lane, chunk order
          if (lane == 0 && k < K) sc[(size_t)q * K + k] = (cb == 0 ? (b ? b[k] : 0.f) : sc[(size_t)q * K + k]) + s;
        }
      }
    }
  }
  __syncthreads();
  if (clip_score) {
    float* __restrict__ cs = clip_score + (size_t)n * clips * K;
    for (int i = tid; i < clips * K; i += HT_NT) cs[i] = sc[i];
  }
  if (mode == 2) return;
  if (mode == 0) {
    __syncthreads();                                      // (clip_score has read the scores the softmax overwrites)
    for (int q = wave; q < clips; q += 4) {
      float* __restrict__ row = sc + (size_t)q * K;
      float mx = -__builtin_inff();
      for (int k = lane; k < K; k += 64) mx = fmaxf(mx, row[k]);
      mx = wave_max(mx);
      float se = 0.f;
      for (int k = lane; k < K; k += 64) {
        const float e = expf(row[k] - mx);                // a NaN score: fmaxf skips it, the difference keeps it
        row[k] = e;
        se += e;
      }
      se = wave_sum(se);
      const float inv = 1.f / se;
      for (int k = lane; k < K; k += 64) row[k] *= inv;
    }
    __syncthreads();
  }
}

// out[n, k]: the mean over the clips of sc[., k], clip order
__device__ __forceinline__ float ht_clip_mean(const float* sc, int clips, int K, int k) {
  float s = 0.f;
  for (int q = 0; q < clips; ++q) s += sc[(size_t)q * K + k];
  return s / (float)clips;
}
