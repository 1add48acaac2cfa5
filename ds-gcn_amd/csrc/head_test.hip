// The test-time head in one launch: what RecognizerGCN.forward_test does after the backbone
// (pyskl/models/heads/simple_head.py:88-98 person mean + fc_cls, then recognizers/recognizergcn.py's average_clips step:
// softmax(dim=2).mean(dim=1) for 'prob', .mean(dim=1) for 'score', the per-clip scores for None) — about eight framework
// launches and an (N*clips, K) round trip there.  One launch here, so that a whole test pass replays as one hipGraph.
//   k_head_test   one workgroup per VIDEO: its clips' pooled features and scores stay in LDS, every weight row is read
//                 once per workgroup and reused by all clips.
// Every sum runs in a fixed order (person mean, dot products, softmax denominator, clip mean; no atomics): two launches
// on the same input give the same bits.
#include "head_test_core.h"

namespace {

// The arithmetic lives in head_test_core.h (ht_video_scores: person mean, scores, softmax; ht_clip_mean), shared with the
// ensemble launch of csrc/head_ensemble.hip.
//   mode 0: out[n, k] = (1/clips) sum_q softmax_k(sc[q])[k]
//   mode 1: out[n, k] = (1/clips) sum_q sc[q, k]              mode 2: nothing but clip_score
template <bool VEC>
__global__ __launch_bounds__(HT_NT) void k_head_test(const float* __restrict__ feat, const float* __restrict__ w,
                                                     const float* __restrict__ b, int clips, int M, int C, int K, int mode,
                                                     float* __restrict__ clip_score, float* __restrict__ out) {
  extern __shared__ float hs[];
  float* pl = hs;
  float* sc = hs + (size_t)clips * C;
  const int n = blockIdx.x;
  ht_video_scores<VEC>(feat, w, b, n, clips, M, C, K, mode, clip_score, pl, sc);
  if (mode == 2) return;
  for (int k = threadIdx.x; k < K; k += HT_NT) out[(size_t)n * K + k] = ht_clip_mean(sc, clips, K, k);
}

}  // namespace

extern "C" {

int dsgcn_head_test_fwd(const float* feat, const float* w, const float* b, int N, int clips, int M, int C, int K, int mode,
                        float* clip_score, float* out, void* stream) {
  if (!feat || !w || N <= 0 || clips <= 0 || M <= 0 || C <= 0 || K <= 0 || mode < 0 || mode > 2) return DSGCN_EINVAL;
  if (!clip_score && (!out || mode == 2)) return DSGCN_EINVAL;      // nothing to write
  if (!out) mode = 2;                                                 // only the per-clip scores were asked for
  const size_t lds = ht_lds_bytes(clips, C, K);
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
