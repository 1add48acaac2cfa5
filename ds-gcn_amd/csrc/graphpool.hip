// Per-video mean of a layer's dynamic adjacency over person-samples and channels (test_cfg['graph_ext']).
//
//   ahat (videos*group, K, mid, V, V)  ->  out[video, layer, k, u, w] = mean over the `group` person-samples n of the video
//                                           and the `mid` channels c of ahat[video*group + n, k, c, u, w]
//
// out is the caller's (videos, L, K, V, V) buffer; only the slice of `layer` is written.  ahat is read once and never
// copied.  No atomics: the planes of one (video, k) are dealt to `splits` workgroups in contiguous runs, each adds its run
// in plane order into registers, and (splits > 1) a second launch adds the `splits` partial planes in a fixed order in fp64
// (eight interleaved lanes, then the lanes in order), divides once and rounds once.  With splits == 1 the first launch divides and writes the result itself.
//
// A plane is V*V floats (625 at V = 25: no multiple of 4) and a plane's start is only 4-byte aligned, whatever the base
// pointer's alignment.  Every lane owns four consecutive elements of the plane and reads them with ONE 16-byte load at
// 4-byte alignment (global memory takes that; the f32x4_a4 type tells the compiler); the lane whose four elements would cross
// the plane's end reads its 1-3 elements one by one, so nothing past the last plane is touched.
#include "common.h"

namespace {

constexpr int GP_THREADS = 256;        // x 4 elements: V*V <= 1024
constexpr int GP_MIN_PLANES = 4;       // planes a workgroup adds at least (below that the partial planes outweigh the input)
constexpr int GP_FLIGHT = 8;           // 16-byte loads a lane has in flight
constexpr int GP_TARGET_WGS = 1024;    // workgroups of the first launch where the input allows (256 CUs x 4)
constexpr int GP_FIN_ELEMS = 32, GP_FIN_LANES = 8;
constexpr int GP_FIN_THREADS = GP_FIN_ELEMS * GP_FIN_LANES;

typedef float f32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));      // 16 bytes at a 4-byte boundary

// FULL: the lane's four elements lie inside the plane -> one 16-byte load; otherwise its `left` (1-3) elements one by one
template <bool FULL>
__device__ __forceinline__ f32x4 gp_load(const float* __restrict__ p, int left) {
  if constexpr (FULL) return *reinterpret_cast<const f32x4_a4*>(p);
  f32x4 r = {0.f, 0.f, 0.f, 0.f};
  r.x = p[0];
  if (left > 1) r.y = p[1];
  if (left > 2) r.z = p[2];
  return r;
}

// the sum, in plane order, of the lane's four elements over planes [p0, p1) of (video, k); base: the (video, k = 0,
// person-sample 0) plane + the lane's element offset
template <bool FULL>
__device__ __forceinline__ f32x4 gp_sum(const float* __restrict__ base, int p0, int p1, int K, int k, int mid, int VV,
                                        int left) {
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  int n = p0 / mid, c = p0 - n * mid;          // plane p = (person-sample n, channel c)
  for (int p = p0; p < p1; p += GP_FLIGHT) {
    f32x4 v[GP_FLIGHT];
#pragma unroll
    for (int q = 0; q < GP_FLIGHT; ++q) {      // these loads are in flight together, the adds below keep plane order
      v[q] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (p + q < p1) {
        const size_t plane = ((size_t)n * K + k) * mid + c;
        v[q] = gp_load<FULL>(base + plane * VV, left);
        if (++c == mid) { c = 0; ++n; }
      }
    }
#pragma unroll
    for (int q = 0; q < GP_FLIGHT; ++q) acc += v[q];
  }
  return acc;
}

// grid: (videos*K) * splits workgroups; workgroup ((video, k), s) adds planes [s*ppw, min((s+1)*ppw, group*mid)) of its
// (video, k) — plane p = (person-sample p / mid, channel p % mid) — and writes V*V floats at
// dst + video*vstride + k*kstride + s*VV, divided by `div` (1 for a partial plane: exact).
__global__ __launch_bounds__(GP_THREADS) void k_graph_pool(const float* __restrict__ ahat, float* __restrict__ dst,
                                                           int group, int K, int mid, int VV, int splits, int ppw,
                                                           long vstride, long kstride, float div) {
  const int s = blockIdx.x % splits;
  const int vk = blockIdx.x / splits;
  const int k = vk % K, video = vk / K;
  const int e0 = threadIdx.x * 4;
  if (e0 >= VV) return;
  const int left = VV - e0;
  const int p0 = s * ppw;
  const int p1 = min(p0 + ppw, group * mid);
  const float* base = ahat + (size_t)video * group * K * mid * VV + e0;
  const f32x4 acc = left >= 4 ? gp_sum<true>(base, p0, p1, K, k, mid, VV, left)
                              : gp_sum<false>(base, p0, p1, K, k, mid, VV, left);
  float* o = dst + (size_t)video * vstride + (size_t)k * kstride + (size_t)s * VV + e0;
  o[0] = acc.x / div;
  if (left > 1) o[1] = acc.y / div;
  if (left > 2) o[2] = acc.z / div;
  if (left > 3) o[3] = acc.w / div;
}

// grid: (videos*K, ceil(VV / 32)), 256 threads = 32 elements x 8 split lanes.  Lane j of an element adds the partial planes
// s = j, j + 8, ... in that order in fp64 (eight loads in flight at a time: the sum must not wait for `splits` memory
// round trips one after another), then the eight lane sums are added in lane order, divided once and rounded once:
// out[video, layer, k, e] = (sum over s of ws[(video, k), s, e]) / R
__global__ __launch_bounds__(GP_FIN_THREADS) void k_graph_pool_finish(const float* __restrict__ ws, float* __restrict__ out,
                                                                      int K, int VV, int splits, long vstride, double R) {
  __shared__ double part[GP_FIN_LANES][GP_FIN_ELEMS];
  const int el = threadIdx.x % GP_FIN_ELEMS, j = threadIdx.x / GP_FIN_ELEMS;
  const int e = blockIdx.y * GP_FIN_ELEMS + el;
  const int vk = blockIdx.x;
  double sum = 0.0;
  if (e < VV) {
    const float* src = ws + (size_t)vk * splits * VV + e;
    for (int s0 = j; s0 < splits; s0 += 8 * GP_FIN_LANES) {
      float v[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int s = s0 + q * GP_FIN_LANES;
        v[q] = s < splits ? src[(size_t)s * VV] : 0.f;
      }
#pragma unroll
      for (int q = 0; q < 8; ++q) sum += (double)v[q];
    }
  }
  part[j][el] = sum;
  __syncthreads();
  if (j == 0 && e < VV) {
    double total = part[0][el];
#pragma unroll
    for (int q = 1; q < GP_FIN_LANES; ++q) total += part[q][el];
    const int k = vk % K, video = vk / K;
    out[(size_t)video * vstride + (size_t)k * VV + e] = (float)(total / R);
  }
}

int gp_check(int videos, int group, int K, int mid, int V) {
  if (videos < 1 || group < 1 || K < 1 || mid < 1 || V < 1) return DSGCN_EINVAL;
  if (V > 32 || mid > 64 || K > 16) return DSGCN_EUNSUPPORTED;
  // every plane index of the input and every workgroup index of the launch is an int
  if ((double)videos * group * K * mid > 2147483647.0 || (long)group * mid > 2147483647L) return DSGCN_EUNSUPPORTED;
  return 0;
}

int gp_splits(int videos, int group, int K, int mid) {
  const long planes = (long)group * mid;
  const long total = planes * videos * K;
  long ppw = (total + GP_TARGET_WGS - 1) / GP_TARGET_WGS;
  if (ppw < GP_MIN_PLANES) ppw = GP_MIN_PLANES;
  return (int)((planes + ppw - 1) / ppw);
}

}  // namespace

extern "C" int dsgcn_graph_pool_splits(int videos, int group, int K, int mid, int V) {
  const int rc = gp_check(videos, group, K, mid, V);
  return rc ? rc : gp_splits(videos, group, K, mid);
}

extern "C" int dsgcn_graph_pool(const float* ahat, float* out, float* ws, int videos, int group, int K, int mid, int V,
                                int L, int layer, void* stream) {
  if (!ahat || !out || L < 1 || layer < 0 || layer >= L) return DSGCN_EINVAL;
  const int rc = gp_check(videos, group, K, mid, V);
  if (rc) return rc;
  const int splits = gp_splits(videos, group, K, mid);
  if (splits > 1 && !ws) return DSGCN_EINVAL;
  const int VV = V * V;
  const int planes = group * mid;
  const int ppw = (planes + splits - 1) / splits;
  const long out_vstride = (long)L * K * VV;
  float* slice = out + (size_t)layer * K * VV;
  hipStream_t st = (hipStream_t)stream;
  const unsigned grid = (unsigned)videos * K * splits;
  if (splits == 1) {
    k_graph_pool<<<grid, GP_THREADS, 0, st>>>(ahat, slice, group, K, mid, VV, 1, ppw, out_vstride, (long)VV, (float)planes);
    DSGCN_LAUNCH_CHECK();
    return 0;
  }
  k_graph_pool<<<grid, GP_THREADS, 0, st>>>(ahat, ws, group, K, mid, VV, splits, ppw, (long)K * splits * VV,
                                            (long)splits * VV, 1.f);
  DSGCN_LAUNCH_CHECK();
  k_graph_pool_finish<<<dim3((unsigned)videos * K, (VV + GP_FIN_ELEMS - 1) / GP_FIN_ELEMS), GP_FIN_THREADS, 0, st>>>(
      ws, slice, K, VV, splits, out_vstride, (double)planes);
  DSGCN_LAUNCH_CHECK();
  return 0;
}
