// Feature and score-map extraction at test time in one launch: what RecognizerGCN.forward_test does with the last block's
// activation under test_cfg['feat_ext'] / ['score_ext'] (pyskl/models/recognizers/recognizergcn.py:68-93): a chain of
// x.mean(axis, keepdim=True) over the clip / person / frame / joint axes named in pool_opt, then — score_ext — fc_cls at
// every remaining position (einsum('nmctv,oc->nmotv') + bias), then the cast to float16.  Up to four reductions, the
// einsum's permutes, the bias add and the cast there, with the pooled tensor written and read back between them.
//   k_feat_ext<false>   feature mode: a block pools 32 positions x a slice of the channels and stores them.
//   k_feat_ext<true>    score mode: a block pools 32 positions x ALL channels into LDS ([C][32], the pooled tensor never
//                       reaches HBM), then its four waves take the class tiles: v_mfma_f32_32x32x2_f32 (true fp32) when a
//                       video has a whole tile of positions, wave dot products (fp64 partial sums) otherwise.
// A "position" is one kept (clip', person', frame', joint') index of a video, joint fastest.  x is read once.
// Every sum runs in a fixed order (pooling: clip, person, frame, joint nest — or lane-strided plane sums + the xor tree;
// projection: channel order within four interleaved accumulators and their pairwise sum — or lane-strided partial sums
// + the xor tree —, the bias last; no atomics): two launches on the same input give the same bits.
#include "common.h"

namespace {

constexpr int FX_NT = 256;        // four waves
constexpr int FX_PT = 32;         // positions per block = one MFMA tile edge
constexpr int FX_J = 8;           // positions a wave has in flight per pass of the dot-product form
constexpr int FX_CU = 4;          // channels a thread pools at a time

struct FxShape {
  int clips, M, C, T, V, K;
  int nq, nm, nt, nv;             // pooled extents (1 where the axis is kept)
  int me, te, ve;                 // kept extents of person, frame, joint (1 where pooled)
  int P, Sp;                      // positions per video; kept (frame, joint) extent = the output's inner stride
  int planes;                     // 1: frames and joints are both pooled -> a wave reduces whole (T, V) planes
  int cchunk;                     // channels per block in feature mode (grid.y slices)
  int ld;                         // score mode: row stride of the LDS tile (32 for the MFMA form, odd below)
};

// means over the pooled axes of one position in FX_CU channels c0, c0 + 8, ... (one per pass of the block's 8 channel
// rows; those below c_hi): fp64 accumulators, ONE rounding to fp32 each (exact whenever the reference's chain of fp32 means
// is exact).  The FX_CU sums advance together so that as many loads are in flight.  xp: channel 0 at pooled offsets 0.
__device__ __forceinline__ void fx_pool_thread(const float* __restrict__ xp, int c0, int c_hi, const FxShape& s, size_t TV,
                                               float (&out)[FX_CU]) {
  const float* __restrict__ xc[FX_CU];
#pragma unroll
  for (int j = 0; j < FX_CU; ++j) xc[j] = xp + (size_t)(c0 + 8 * j < c_hi ? c0 + 8 * j : c0) * TV;
  const int cnt = s.nq * s.nm * s.nt * s.nv;
  if (cnt == 1) {
#pragma unroll
    for (int j = 0; j < FX_CU; ++j) out[j] = xc[j][0];
    return;
  }
  double a[FX_CU];
#pragma unroll
  for (int j = 0; j < FX_CU; ++j) a[j] = 0.0;
  for (int q = 0; q < s.nq; ++q)
    for (int m = 0; m < s.nm; ++m) {
      const size_t plane = ((size_t)q * s.M + m) * s.C * TV;
      for (int t = 0; t < s.nt; ++t)
        for (int v = 0; v < s.nv; ++v) {
#pragma unroll
          for (int j = 0; j < FX_CU; ++j) a[j] += (double)xc[j][plane + t * s.V + v];
        }
    }
#pragma unroll
  for (int j = 0; j < FX_CU; ++j) out[j] = (float)(a[j] / (double)cnt);
}

// the same for whole planes: lanes stride the contiguous (T, V) plane, then the wave's xor tree
__device__ __forceinline__ float fx_pool_wave(const float* __restrict__ xb, const FxShape& s, int TV, int lane) {
  double a = 0.0;
  for (int q = 0; q < s.nq; ++q)
    for (int m = 0; m < s.nm; ++m) {
      const float* __restrict__ pl = xb + ((size_t)q * s.M + m) * s.C * (size_t)TV;
      for (int i = lane; i < TV; i += 64) a += (double)pl[i];
    }
  a = wave_sum_d(a);
  return (float)(a / ((double)s.nq * s.nm * TV));
}

__device__ __forceinline__ void fx_store(float* __restrict__ o32, void* __restrict__ o16, size_t i, float v) {
  if (o32) o32[i] = v;
  if (o16) static_cast<_Float16*>(o16)[i] = (_Float16)v;  // v_cvt_f16_f32: round to nearest even, subnormals kept
}

// out (videos, n', m', Co, t', v'): Co = C (feature) or K (score); position p = (n' m' index) * Sp + (t' v' index)
template <bool SCORE>
__global__ __launch_bounds__(FX_NT) void k_feat_ext(const float* __restrict__ x, const float* __restrict__ w,
                                                    const float* __restrict__ b, FxShape s, int tiles, int wvec,
                                                    float* __restrict__ out32, void* __restrict__ out16) {
  extern __shared__ __attribute__((aligned(16))) float pl[];            // score mode: pl[c * ld + position in tile]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int vid = blockIdx.x / tiles, p0 = (blockIdx.x - vid * tiles) * FX_PT;
  const int np = min(FX_PT, s.P - p0);
  const int c_lo = SCORE ? 0 : blockIdx.y * s.cchunk;
  const int c_hi = SCORE ? s.C : min(s.C, c_lo + s.cchunk);
  const size_t TV = (size_t)s.T * s.V;
  const float* __restrict__ xv = x + (size_t)vid * s.clips * s.M * s.C * TV;
  const size_t orow = (size_t)vid * (s.P / s.Sp);          // (video, n', m') row of the output
  const int Co = SCORE ? s.K : s.C;

  // ---- pooling ----
  if (s.planes) {
    // position = (clip', person'); a wave per (channel, position), channel-major
    for (int e = wave; e < (c_hi - c_lo) * np; e += FX_NT / 64) {
      const int ci = e / np, pp = e - ci * np, c = c_lo + ci, p = p0 + pp;
      const int qq = p / s.me, mm = p - qq * s.me;
      const float v = fx_pool_wave(xv + (((size_t)qq * s.M + mm) * s.C + c) * TV, s, (int)TV, lane);
      if (lane == 0) {
        if (SCORE) pl[c * s.ld + pp] = v;
        else fx_store(out32, out16, (orow + p) * Co + c, v);
      }
    }
  } else {
    // lanes along the positions (the kept inner axis), 8 channels per pass
    const int pp = tid & (FX_PT - 1);
    if (pp < np) {
      const int p = p0 + pp;
      const int vv = p % s.ve;
      int r = p / s.ve;
      const int tt = r % s.te;
      r /= s.te;
      const int mm = r % s.me, qq = r / s.me;
      const float* __restrict__ xp = xv + ((size_t)qq * s.M + mm) * s.C * TV + (size_t)tt * s.V + vv;
      const int pr = p / s.Sp, ps = p - pr * s.Sp;
      for (int c0 = c_lo + (tid >> 5); c0 < c_hi; c0 += 8 * FX_CU) {
        float v[FX_CU];
        fx_pool_thread(xp, c0, c_hi, s, TV, v);
#pragma unroll
        for (int j = 0; j < FX_CU; ++j) {
          const int c = c0 + 8 * j;
          if (c < c_hi) {
            if (SCORE) pl[c * s.ld + pp] = v[j];
            else fx_store(out32, out16, ((orow + pr) * Co + c) * s.Sp + ps, v[j]);
          }
        }
      }
    }
  }
  if (!SCORE) return;
  __syncthreads();

  // ---- projection: score[k, p] = sum_c w[k, c] pl[c, p] + b[k] ----
  const int C = s.C, K = s.K;
  if (s.ld == FX_PT) {
    // i = class, j = position, k = channel.  A column of the tile past np holds whatever LDS held: it only reaches
    // output columns that are not stored.
    const int mi = lane & 31, mk = lane >> 5;
    const int steps = (C + 1) >> 1;
    for (int k0 = wave * 32; k0 < K; k0 += 32 * (FX_NT / 64)) {
      const int kr = k0 + mi;
      const bool kin = kr < K;
      const float* __restrict__ wr = w + (size_t)(kin ? kr : K - 1) * C;
      f32x16 acc[4];
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[j][i] = 0.f;
      for (int s0 = 0; s0 < steps; s0 += 4) {
        float a[4], bb[4];
        if (wvec) {                                       // C % 8 == 0, w 16-byte aligned: the 8 channels of 4 steps
          const f32x4 lo = *reinterpret_cast<const f32x4*>(wr + 2 * s0);
          const f32x4 hi = *reinterpret_cast<const f32x4*>(wr + 2 * s0 + 4);
          a[0] = mk ? lo.y : lo.x;
          a[1] = mk ? lo.w : lo.z;
          a[2] = mk ? hi.y : hi.x;
          a[3] = mk ? hi.w : hi.z;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            bb[j] = pl[(2 * (s0 + j) + mk) * FX_PT + mi];
            a[j] = kin ? a[j] : 0.f;
          }
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int c = 2 * (s0 + j) + mk;
            const bool ok = c < C;
            const int cc = ok ? c : C - 1;
            const float av = wr[cc], bv = pl[cc * FX_PT + mi];
            a[j] = (ok && kin) ? av : 0.f;
            bb[j] = ok ? bv : 0.f;
          }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], bb[j], acc[j], 0, 0, 0);
      }
      if (mi < np) {
        const int p = p0 + mi, pr = p / s.Sp, ps = p - pr * s.Sp;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int k = k0 + mfma_row32(r, mk);
          if (k < K) {
            const float v = ((acc[0][r] + acc[1][r]) + (acc[2][r] + acc[3][r])) + (b ? b[k] : 0.f);
            fx_store(out32, out16, ((orow + pr) * K + k) * s.Sp + ps, v);
          }
        }
      }
    }
  } else {
    // fewer positions than one tile (np == P): a wave per class, lanes split the channels, FX_J positions per pass.  The
    // products are exact in fp64 and there are few of them: fp64 partial sums, the xor tree, the bias, ONE rounding.
    const int ld = s.ld;
    for (int k = wave; k < K; k += FX_NT / 64) {
      const float* __restrict__ wr = w + (size_t)k * C;
      const double bias = b ? (double)b[k] : 0.0;
      for (int pg = 0; pg < np; pg += FX_J) {
        const int nj = min(FX_J, np - pg);                // (uniform: a single position costs a single sum)
        double a[FX_J];
#pragma unroll
        for (int j = 0; j < FX_J; ++j) a[j] = 0.0;
        for (int c = lane; c < C; c += 64) {
          const double wv = (double)wr[c];
#pragma unroll
          for (int j = 0; j < FX_J; ++j)
            if (j < nj) a[j] = fma(wv, (double)pl[c * ld + pg + j], a[j]);
        }
#pragma unroll
        for (int j = 0; j < FX_J; ++j) {
          if (j < nj) {
            const float v = (float)(wave_sum_d(a[j]) + bias);
            if (lane == 0) {
              const int p = pg + j, pr = p / s.Sp, ps = p - pr * s.Sp;
              fx_store(out32, out16, ((orow + pr) * K + k) * s.Sp + ps, v);
            }
          }
        }
      }
    }
  }
}

}  // namespace

extern "C" {

int dsgcn_feat_ext_fwd(const float* x, const float* w, const float* b, int videos, int clips, int M, int C, int T, int V,
                       int K, int pool_mask, float* out32, void* out16, void* stream) {
  if (!x || videos <= 0 || clips <= 0 || M <= 0 || C <= 0 || T <= 0 || V <= 0) return DSGCN_EINVAL;
  if (w && K <= 0) return DSGCN_EINVAL;
  if ((!out32 && !out16) || (pool_mask & ~15)) return DSGCN_EINVAL;
  // pooling an axis of extent 1 is the identity
  const bool pn = (pool_mask & 1) && clips > 1, pm = (pool_mask & 2) && M > 1;
  const bool pt = (pool_mask & 4) && T > 1, pv = (pool_mask & 8) && V > 1;
  FxShape s;
  s.clips = clips, s.M = M, s.C = C, s.T = T, s.V = V, s.K = w ? K : 0;
  s.nq = pn ? clips : 1, s.nm = pm ? M : 1, s.nt = pt ? T : 1, s.nv = pv ? V : 1;
  s.me = pm ? 1 : M, s.te = pt ? 1 : T, s.ve = pv ? 1 : V;
  const long long P = (long long)(pn ? 1 : clips) * s.me * s.te * s.ve;
  if (P > 0x7fffffffLL || (long long)T * V > 0x7fffffffLL) return DSGCN_EUNSUPPORTED;
  s.P = (int)P, s.Sp = s.te * s.ve;
  s.planes = pt && pv && (long long)T * V >= 32;
  s.cchunk = s.planes ? 4 : 32;
  s.ld = P >= FX_PT ? FX_PT : ((int)P | 1);
  const long long tiles = (P + FX_PT - 1) / FX_PT;
  if (tiles * videos > 0x7fffffffLL) return DSGCN_EUNSUPPORTED;
  const dim3 grid((unsigned)(tiles * videos), w ? 1u : (unsigned)((C + s.cchunk - 1) / s.cchunk));
  if (grid.y > 65535u) return DSGCN_EUNSUPPORTED;
  if (w) {
    const size_t lds = (size_t)C * FX_PT * sizeof(float);
    if (lds > 64 * 1024) return DSGCN_EUNSUPPORTED;
    const int wvec = (C & 7) == 0 && ((uintptr_t)w & 15) == 0;
    hipLaunchKernelGGL(k_feat_ext<true>, grid, dim3(FX_NT), lds, (hipStream_t)stream, x, w, b, s, (int)tiles, wvec, out32,
                       out16);
  } else {
    hipLaunchKernelGGL(k_feat_ext<false>, grid, dim3(FX_NT), 0, (hipStream_t)stream, x, w, b, s, (int)tiles, 0, out32,
                       out16);
  }
  DSGCN_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
