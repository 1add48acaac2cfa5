// The test-time head in one launch: what RecognizerGCN.forward_test does after the backbone
// (pyskl/models/heads/simple_head.py:88-98 person mean + fc_cls, then recognizers/recognizergcn.py's average_clips step:
// softmax(dim=2).mean(dim=1) for 'prob', .mean(dim=1) for 'score', the per-clip scores for None) — about eight framework
// launches and an (N*clips, K) round trip there.  One launch here, so that a whole test pass replays as one hipGraph.
//   k_head_test   one workgroup per VIDEO: its clips' pooled features and scores stay in LDS, every weight row is read
//                 once per workgroup and reused by all clips.
// Every sum runs in a fixed order (person mean, dot products, softmax denominator, clip mean; no atomics): two launches
// on the same input give the same bits.
#include "common.h"

namespace {

constexpr int HT_NT = 256;        // four waves
constexpr int HT_J = 8;           // classes a wave has in flight per pass

// LDS: pl[clips][C] pooled features, sc[clips][K] scores (mode 0: overwritten by the probabilities).
//   pl[q, c] = (1/M) sum_m feat[((n*clips + q)*M + m), c]
//   sc[q, k] = <pl[q], W[k]> + b[k]      wave w takes classes w, w + 4, ...: HT_J of them per pass, lanes split C; the
//                                         weight loads of a pass are all issued before the first product
//   mode 0: out[n, k] = (1/clips) sum_q softmax_k(sc[q])[k]   (a wave per clip: max, denominator, in lane-strided order)
//   mode 1: out[n, k] = (1/clips) sum_q sc[q, k]              mode 2: nothing but clip_score
// VEC: C % 4 == 0 and w 16-byte aligned: 16-byte loads of the weight rows and of pl.
template <bool VEC>
__global__ __launch_bounds__(HT_NT) void k_head_test(const float* __restrict__ feat, const float* __restrict__ w,
                                                     const float* __restrict__ b, int clips, int M, int C, int K, int mode,
                                                     float* __restrict__ clip_score, float* __restrict__ out) {
  extern __shared__ float hs[];
  float* pl = hs;
  float* sc = hs + (size_t)clips * C;
  const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
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
  const float fclips = (float)clips;
  for (int k = tid; k < K; k += HT_NT) {
    float s = 0.f;
    for (int q = 0; q < clips; ++q) s += sc[(size_t)q * K + k];
    out[(size_t)n * K + k] = s / fclips;
  }
}

}  // namespace

extern "C" {

int dsgcn_head_test_fwd(const float* feat, const float* w, const float* b, int N, int clips, int M, int C, int K, int mode,
                        float* clip_score, float* out, void* stream) {
  if (!feat || !w || N <= 0 || clips <= 0 || M <= 0 || C <= 0 || K <= 0 || mode < 0 || mode > 2) return DSGCN_EINVAL;
  if (!clip_score && (!out || mode == 2)) return DSGCN_EINVAL;      // nothing to write
  if (!out) mode = 2;                                                 // only the per-clip scores were asked for
  const size_t lds = (size_t)clips * ((size_t)C + (size_t)K) * sizeof(float);
  if (lds > 60 * 1024) return DSGCN_EUNSUPPORTED;
  const bool vec = (C & 3) == 0 && ((uintptr_t)w & 15) == 0;
  if (vec)
    hipLaunchKernelGGL(k_head_test<true>, dim3((unsigned)N), dim3(HT_NT), lds, (hipStream_t)stream, feat, w, b, clips, M, C,
                       K, mode, clip_score, out);
  else
    hipLaunchKernelGGL(k_head_test<false>, dim3((unsigned)N), dim3(HT_NT), lds, (hipStream_t)stream, feat, w, b, clips, M, C,
                       K, mode, clip_score, out);
  DSGCN_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
