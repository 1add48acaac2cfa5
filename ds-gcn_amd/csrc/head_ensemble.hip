// The heads of S recognizers and their weighted sum in one launch: the end of the reference's multi-stream workflow
// (joint + bone + joint-motion + bone-motion, configs/*/README.md note 2) — S runs of RecognizerGCN.forward_test's tail
// (simple_head.py:88-98 + the average_clips step) followed by a host-side weighted sum of the S result files.
//   k_head_ensemble   one workgroup per VIDEO; the streams go through the same LDS one after another, each by
//                     ht_video_scores / ht_clip_mean of head_test_core.h — the code dsgcn_head_test_fwd runs, so row
//                     (s, n) of stream_out has the bits of that launch on stream s alone.
//   out[n, k] = (...((0 + weight[0] p_0) + weight[1] p_1) ...) in fp32, every product and every sum rounded by itself
//   (no FMA): numpy's `sum(stack(s) * float32(w) for s, w in ...)` on the host.
// Thread tid owns classes tid, tid + 256, ... in every stream: the running sum of a class is read back by the thread that
// wrote it (no atomics, no cross-thread traffic); repeated launches give the same bits.
#include "head_test_core.h"

namespace {

constexpr int HE_MAX = 8;         // streams per launch (include/dsgcn.h)

struct HeArgs {
  const float* feat[HE_MAX];
  const float* w[HE_MAX];
  const float* b[HE_MAX];
  const float* weight;
  float* stream_out;
  float* out;
  int S, N, clips, M, C, K, mode, vecmask;
};

__global__ __launch_bounds__(HT_NT) void k_head_ensemble(HeArgs a) {
  extern __shared__ float hs[];
  float* pl = hs;
  float* sc = hs + (size_t)a.clips * a.C;
  const int n = blockIdx.x;
  float* __restrict__ on = a.out + (size_t)n * a.K;
  for (int s = 0; s < a.S; ++s) {
    if (s) __syncthreads();                               // the previous stream's clip means have read sc
    if ((a.vecmask >> s) & 1)
      ht_video_scores<true>(a.feat[s], a.w[s], a.b[s], n, a.clips, a.M, a.C, a.K, a.mode, nullptr, pl, sc);
    else
      ht_video_scores<false>(a.feat[s], a.w[s], a.b[s], n, a.clips, a.M, a.C, a.K, a.mode, nullptr, pl, sc);
    const float ws = a.weight[s];
    float* __restrict__ so = a.stream_out ? a.stream_out + ((size_t)s * a.N + n) * a.K : nullptr;
    for (int k = threadIdx.x; k < a.K; k += HT_NT) {
      const float p = ht_clip_mean(sc, a.clips, a.K, k);
      if (so) so[k] = p;
      const float acc = s ? on[k] : 0.f;
      // __fmul_rn / __fadd_rn are plain * and + to this compiler and would contract to one FMA: the product is pinned
      // in a register of its own first, so it is rounded before the sum
      float prod = __fmul_rn(ws, p);
      asm volatile("" : "+v"(prod));
      on[k] = __fadd_rn(acc, prod);
    }
  }
}

}  // namespace

extern "C" int dsgcn_head_ensemble_fwd(const float* const* feat, const float* const* w, const float* const* b,
                                       const float* weight, int S, int N, int clips, int M, int C, int K, int mode,
                                       float* stream_out, float* out, void* stream) {
  if (!feat || !w || !weight || !out || S < 1 || S > HE_MAX) return DSGCN_EINVAL;
  if (N <= 0 || clips <= 0 || M <= 0 || C <= 0 || K <= 0 || mode < 0 || mode > 1) return DSGCN_EINVAL;
  HeArgs a{};
  for (int s = 0; s < S; ++s) {
    if (!feat[s] || !w[s]) return DSGCN_EINVAL;
    a.feat[s] = feat[s];
    a.w[s] = w[s];
    a.b[s] = b ? b[s] : nullptr;
    // per stream, what dsgcn_head_test_fwd would pick for it
    if ((C & 3) == 0 && ((uintptr_t)w[s] & 15) == 0) a.vecmask |= 1 << s;
  }
  const size_t lds = ht_lds_bytes(clips, C, K);
  if (lds > 60 * 1024) return DSGCN_EUNSUPPORTED;
  a.weight = weight; a.stream_out = stream_out; a.out = out;
  a.S = S; a.N = N; a.clips = clips; a.M = M; a.C = C; a.K = K; a.mode = mode;
  hipLaunchKernelGGL(k_head_ensemble, dim3((unsigned)N), dim3(HT_NT), lds, (hipStream_t)stream, a);
  DSGCN_LAUNCH_CHECK();
  return 0;
}
