// K-B plain: the dynamic adjacency of dggcn, the original DG-STGCN unit (reference: pyskl/models/gcns/utils/gcn.py:1445-1584),
// for any number of subsets K (graph_cfg num_filter).  No node-typed select, no edge-typed linear (those are
// csrc/dynadj.hip, dynadj_typed.hip and dynadj_flags.hip, all three with K = 3 compiled in).
//
//   proj (n, 2*K*mid, ld) = [conv1 | conv2] applied to xbar (one K-C launch), row k*mid + c, joint stride ld >= V
//   x1[k,c,v] = conv1 row k*mid + c,  x2[k,c,v] = conv2 row k*mid + c
//   G_k[u,w]      = sum_c x1[k,c,u] x2[k,c,w]                                            (c ascending, fma)
//   Ahat[k,c,u,w] = A[k,u,w] + alpha_k tanh(x1[k,c,u] - x2[k,c,w]) + beta_k softmax_u(G_k)[u,w]
//
// A workgroup is one (sample, subset) pair, so K is a run-time value and nothing is shared between subsets.  Its LDS
// image is x1, x2 (mid x V each), the softmax (V x V) and the column statistics: ~20 KB at the largest supported shape
// forward, ~57 KB backward, so several 256-thread workgroups share a CU.
// Forward: (sample, subset, channel window) writes the window's Ahat rows.  Backward: (sample, subset) over all channels
// (the softmax couples them), CH channels per round: dD = alpha_k (1 - tanh^2) dAhat goes to an LDS tile whose row /
// column sums are d x1 / -d x2 — no global workspace.  The Ahat / dAhat rows of a workgroup are one contiguous run of
// floats; it is walked in 16-byte slots laid on the 16-byte grid of the address space, so the slots that lie wholly inside
// the run are one 16-byte store / load each whatever the run's own alignment (mid * V * V % 4 != 0 only makes the first
// and last slot partial: those go element by element).
// Partials per sample [sum_c dAhat (K*V*V) | dalpha (K) | dbeta (K)], summed by dsgcn_colsum.  The Gram, the softmax, its
// backward and the scalar reduce are dynadj_common.h's; the 16-byte-slot walk is this file's.
#include "dynadj_common.h"

namespace {

constexpr int NT = 256;
constexpr int NW = NT / DSGCN_WAVE;
constexpr int MAXK = 16, MAXM = 64, MAXV = 32;
constexpr int CH = 4;            // channels per round of the backward (CH * V * V % 4 == 0: every round has the same slots)

struct PlainDims { int n, K, mid, V, ld; };

__host__ __device__ constexpr int up4(int x) { return (x + 3) & ~3; }

// X1 / X2 of subset k (mid x V, X2 right behind X1) from proj, then S = softmax_u(sum_c X1[c,u] X2[c,w])
__device__ __forceinline__ void plain_prepare(const PlainDims& d, int k, const float* __restrict__ proj_n, float* X1,
                                              float* S, float* cst) {
  const int tid = threadIdx.x, m = d.mid, V = d.V;
  const float* X2 = X1 + m * V;
  for (int o = tid; o < 2 * m * V; o += NT) {
    const int second = o >= m * V, r = o - second * m * V;
    const int c = r / V, v = r - c * V;
    X1[o] = proj_n[((size_t)(second * d.K + k) * m + c) * d.ld + v];
  }
  __syncthreads();
  kb_gram(m, V, NT, X1, X2, S);
  __syncthreads();
  kb_col_softmax(V, NT, S, cst, cst + 1, 2);      // column w: max in cst[2w], 1 / sum in cst[2w + 1]
}

// (channel, u, w) of a float offset inside a run of (channels, V, V), and the step to the next float
struct Cuw {
  int c, u, w;
  __device__ __forceinline__ Cuw(int f, int V, int VV) {
    c = f / VV;
    const int r = f - c * VV;
    u = r / V;
    w = r - u * V;
  }
  __device__ __forceinline__ void next(int V) {
    if (++w == V) {
      w = 0;
      if (++u == V) { u = 0; ++c; }
    }
  }
};

// grid (n*K, windows): workgroup = (sample, subset, channel window)
template <int VT>
__global__ __launch_bounds__(NT) void k_dynplain_fwd(PlainDims d, const float* __restrict__ proj,
                                                     const float* __restrict__ A, const float* __restrict__ alpha,
                                                     const float* __restrict__ beta, float* __restrict__ ahat) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  if (VT) d.V = VT;
  const int tid = threadIdx.x, m = d.mid, V = d.V, VV = V * V;
  const int b = blockIdx.x, n = b / d.K, k = b - n * d.K;
  int pc0, pm;
  kb_window(m, (int)blockIdx.y, (int)gridDim.y, pc0, pm);
  float* X1 = lds;
  const float* X2 = X1 + m * V;
  float* S = lds + up4(2 * m * V);
  float* Ak = S + up4(VV);
  float* cst = Ak + up4(VV);
  for (int i = tid; i < VV; i += NT) Ak[i] = A[(size_t)k * VV + i];
  plain_prepare(d, k, proj + (size_t)n * 2 * d.K * m * d.ld, X1, S, cst);
  const float al = alpha[k], bt = beta[k];
  float* out = ahat + ((size_t)b * m + pc0) * VV;
  const int total = pm * VV;
  const int off = (int)((reinterpret_cast<uintptr_t>(out) >> 2) & 3);      // floats past a 16-byte boundary
  const int ns = (off + total + 3) >> 2;
  for (int j = tid; j < ns; j += NT) {
    const int f0 = 4 * j - off;
    Cuw p(max(f0, 0), V, VV);
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int f = f0 + e;
      v[e] = 0.f;
      if (f >= 0) {
        if (f < total) {
          const int c = pc0 + p.c, r = p.u * V + p.w;
          v[e] = Ak[r] + al * tanhf(X1[c * V + p.u] - X2[c * V + p.w]) + bt * S[r];
        }
        p.next(V);
      }
    }
    if (f0 >= 0 && f0 + 3 < total) {
      *reinterpret_cast<f32x4*>(out + f0) = f32x4{v[0], v[1], v[2], v[3]};
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (f0 + e >= 0 && f0 + e < total) out[f0 + e] = v[e];
    }
  }
}

// LDS carve of the backward (floats)
__host__ __device__ constexpr int bwd_lds_floats(int m, int V) {
  return up4(2 * m * V) + 2 * up4(V * V) + up4(2 * V) + up4(2 * m * V) + CH * V * V + 8;
}
__host__ __device__ constexpr int fwd_lds_floats(int m, int V) { return up4(2 * m * V) + 2 * up4(V * V) + up4(2 * V); }

// grid (n*K): workgroup = (sample, subset), all channels.  Outputs: dproj (n, 2*K*mid, ld) rows of this subset (padding
// columns zero) and the sample's partial row [sum_c dAhat (K*V*V) | dalpha (K) | dbeta (K)].
template <int VT>
__global__ __launch_bounds__(NT) void k_dynplain_bwd(PlainDims d, const float* __restrict__ proj,
                                                     const float* __restrict__ alpha, const float* __restrict__ beta,
                                                     const float* __restrict__ dahat, float* __restrict__ dproj,
                                                     float* __restrict__ ppar, int pstride) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  __shared__ float red[2][NW];
  if (VT) d.V = VT;
  const int tid = threadIdx.x;
  const int m = d.mid, V = d.V, VV = V * V, K = d.K;
  const int b = blockIdx.x, n = b / K, k = b - n * K;
  float* X1 = lds;
  const float* X2 = X1 + m * V;
  float* S = lds + up4(2 * m * V);
  float* SC = S + up4(VV);              // sum_c dAhat, then dG
  float* cst = SC + up4(VV);
  float* dX1 = cst + up4(2 * V);        // row sums of dD  (d x1 without the Gram term)
  float* dX2 = dX1 + m * V;             // -column sums    (d x2 without the Gram term)
  float* DD = dX1 + up4(2 * m * V);     // the round's dD tile, laid on the 16-byte grid of dAhat: element f at DD[off + f]
  plain_prepare(d, k, proj + (size_t)n * 2 * K * m * d.ld, X1, S, cst);
  const float* g_k = dahat + (size_t)b * m * VV;
  float* par = ppar + (size_t)n * pstride;
  const float al = alpha[k], bk = beta[k];
  const int off = (int)((reinterpret_cast<uintptr_t>(g_k) >> 2) & 3);      // the same for every round: CH * VV % 4 == 0
  const int ns = (off + CH * VV + 3) >> 2;
  constexpr int SL = ((VT ? VT * VT : MAXV * MAXV) + 1 + NT - 1) / NT;     // slots per thread (ns <= V*V + 1)

  // rounds of CH channels.  Slot j of a round is the same (channel mod CH, u, w) quadruple in every round, so the thread
  // that owns it keeps its share of sum_c dAhat in registers.
  float acc[SL][4];
#pragma unroll
  for (int s = 0; s < SL; ++s)
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[s][e] = 0.f;
  float pal = 0.f;
  for (int c0 = 0; c0 < m; c0 += CH) {
    const int len = min(CH, m - c0) * VV;                  // floats of this round
    const float* gt = g_k + (size_t)c0 * VV;
#pragma unroll
    for (int s = 0; s < SL; ++s) {
      const int j = tid + s * NT;
      if (j < ns) {
        const int f0 = 4 * j - off;
        float g[4];
        if (f0 >= 0 && f0 + 3 < len) {
          const f32x4 q = *reinterpret_cast<const f32x4*>(gt + f0);
          g[0] = q.x; g[1] = q.y; g[2] = q.z; g[3] = q.w;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) g[e] = (f0 + e >= 0 && f0 + e < len) ? gt[f0 + e] : 0.f;
        }
        Cuw p(max(f0, 0), V, VV);
        float dd[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int f = f0 + e;
          dd[e] = 0.f;
          if (f >= 0) {
            if (f < len) {
              const int c = c0 + p.c;
              const float th = tanhf(X1[c * V + p.u] - X2[c * V + p.w]);
              acc[s][e] += g[e];
              pal = fmaf(th, g[e], pal);
              dd[e] = al * (1.f - th * th) * g[e];
            }
            p.next(V);
          }
        }
        *reinterpret_cast<f32x4*>(DD + 4 * j) = f32x4{dd[0], dd[1], dd[2], dd[3]};
      }
    }
    __syncthreads();
    if (tid < 2 * CH * V) {                                // thread = (row | column, channel of the round, joint)
      const int col = tid >= CH * V, q = tid - col * CH * V;
      const int cl = q / V, j = q - cl * V, c = c0 + cl;
      if (c < m) {
        const float* t = DD + off + cl * VV;
        float sum = 0.f;
        if (!col) {
          for (int w = 0; w < V; ++w) sum += t[j * V + w];
          dX1[c * V + j] = sum;
        } else {
          for (int u = 0; u < V; ++u) sum += t[u * V + j];
          dX2[c * V + j] = -sum;
        }
      }
    }
    __syncthreads();
  }
  // sum_c dAhat: the CH register shares of every (u, w) through the tile, added in channel order
#pragma unroll
  for (int s = 0; s < SL; ++s) {
    const int j = tid + s * NT;
    if (j < ns) *reinterpret_cast<f32x4*>(DD + 4 * j) = f32x4{acc[s][0], acc[s][1], acc[s][2], acc[s][3]};
  }
  __syncthreads();
  float pbe = 0.f;
  for (int r = tid; r < VV; r += NT) {
    float sc = 0.f;
#pragma unroll
    for (int cl = 0; cl < CH; ++cl) sc += DD[off + cl * VV + r];
    SC[r] = sc;
    par[k * VV + r] = sc;
    pbe = fmaf(S[r], sc, pbe);
  }
  __syncthreads();
  if (tid < V) kb_softmax_bwd(V, tid, S, SC, bk);
  __syncthreads();
  // this subset's dproj rows: Gram backward + the row / column sums of dD; thread = (x1 | x2, c, joint), padding zero
  {
    const int ld = d.ld;
    float* dp_n = dproj + (size_t)n * 2 * K * m * ld;
    for (int o = tid; o < 2 * m * ld; o += NT) {
      const int q = o / ld, j = o - q * ld;
      const int second = q >= m, c = q - second * m;
      float val = 0.f;
      if (j < V) {
        float g = 0.f;
        if (!second) {
          for (int w = 0; w < V; ++w) g = fmaf(SC[j * V + w], X2[c * V + w], g);      // d x1[c,j]
          val = dX1[c * V + j] + g;
        } else {
          for (int u = 0; u < V; ++u) g = fmaf(SC[u * V + j], X1[c * V + u], g);      // d x2[c,j]
          val = g + dX2[c * V + j];
        }
      }
      dp_n[((size_t)(second * K + k) * m + c) * ld + j] = val;
    }
  }
  kb_reduce2_put(pal, pbe, red);
  __syncthreads();
  kb_reduce2_get(red, par, K * VV + k, K);
}

bool dims_ok(int n, int K, int mid, int V, int ld) {
  return n > 0 && n <= (1 << 24) && K >= 1 && K <= MAXK && mid >= 1 && mid <= MAXM && V >= 1 && V <= MAXV && ld >= V;
}

}  // namespace

extern "C" {

int dsgcn_dynplain_partial_stride(int K, int V) { return K * V * V + 2 * K; }

int dsgcn_dynplain_fwd(const float* proj, const float* A, const float* alpha, const float* beta, float* ahat, int n, int K,
                       int mid, int V, int ld, void* stream) {
  if (!proj || !A || !alpha || !beta || !ahat) return DSGCN_EINVAL;
  if (!dims_ok(n, K, mid, V, ld)) return DSGCN_EINVAL;
  // channel windows of >= 8 channels while the launch has fewer than ~2048 workgroups (each recomputes the subset's Gram)
  int windows = 1;
  while (windows < 8 && (long)n * K * windows < 2048 && mid / (2 * windows) >= 8) windows *= 2;
  const size_t lds = sizeof(float) * fwd_lds_floats(mid, V);
  PlainDims d{n, K, mid, V, ld};
#define PLAIN_FWD(VT)                                                                                                  \
  hipLaunchKernelGGL((k_dynplain_fwd<VT>), dim3(n * K, windows), dim3(NT), lds, (hipStream_t)stream, d, proj, A, alpha, \
                     beta, ahat);
  KB_DISPATCH_V(PLAIN_FWD)
#undef PLAIN_FWD
  DSGCN_LAUNCH_CHECK();
  return 0;
}

int dsgcn_dynplain_bwd(const float* proj, const float* alpha, const float* beta, const float* dahat, float* dproj,
                       float* ppar, int pstride, int n, int K, int mid, int V, int ld, void* stream) {
  if (!proj || !alpha || !beta || !dahat || !dproj || !ppar) return DSGCN_EINVAL;
  if (!dims_ok(n, K, mid, V, ld)) return DSGCN_EINVAL;
  if (pstride < dsgcn_dynplain_partial_stride(K, V)) return DSGCN_EINVAL;
  static_assert(sizeof(float) * bwd_lds_floats(MAXM, MAXV) <= 64 * 1024, "the backward's LDS image fits the default limit");
  const size_t lds = sizeof(float) * bwd_lds_floats(mid, V);
  PlainDims d{n, K, mid, V, ld};
#define PLAIN_BWD(VT)                                                                                                  \
  hipLaunchKernelGGL((k_dynplain_bwd<VT>), dim3(n * K), dim3(NT), lds, (hipStream_t)stream, d, proj, alpha, beta, dahat, \
                     dproj, ppar, pstride);
  KB_DISPATCH_V(PLAIN_BWD)
#undef PLAIN_BWD
  DSGCN_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
