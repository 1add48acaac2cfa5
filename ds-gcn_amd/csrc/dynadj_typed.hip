// K-B typed: the dynamic adjacency of dghgcn (reference: pyskl/models/gcns/utils/gcn.py:1586-1806), where every one of
// the K = 3 subsets carries the node-typed projections and the edge-typed attention (dgphgcn1's K-B, csrc/dynadj.hip, types
// one subset out of three and keeps the edge linear block-diagonal to it).
//
//   proj (n, 2*K*mid*P, ld) = [conv1 | conv2] applied to xbar (one K-C launch), row (k*mid + c)*P + p  (P = 1: untyped)
//   x12  (n, K*mid, 2, 32): slot 0 = x1[k,c,v] = conv1 row (k*mid+c)*P + tau(v), slot 1 = x2 the same from conv2
//        (the node-typed select: dsgcn_dyntyped_select_*; joints >= V are zero)
//   pq   (n, E*K*mid, 2, 32) = We . x12 (one K-C launch, We = edge_linears (E*K*mid, K*mid): it mixes all K*mid channels)
//        row k*E*mid + e*mid + c; slot 0 = P_e without the bias, slot 1 = Q_e
//   D[k,c,u,w] = (pq0[k,eps(u,w),c,u] + be[k,eps,c]) - pq1[k,eps(u,w),c,w]  (+ x1[k,c,u] - x2[k,c,w] under add_type);
//                x1[k,c,u] - x2[k,c,w] without edge attention
//   Ahat[k,c,u,w] = A[k,u,w] + alpha_k tanh(D) + beta_k softmax_u(sum_c x1[k,c,u] x2[k,c,w])
//
// Forward: workgroup = (sample, subset, channel window).  Backward: workgroup = (sample, subset) over all channels; dD goes
// to the workspace dd (stays in L2), the class bins give dpq (its K-C backward gives We^T dP / We^T dQ and dWe), the direct
// path (no edge attention, or add_type) and the Gram backward give dx12.  Partials per sample [sum_c dAhat (K*V*V) |
// dalpha (K) | dbeta (K) | dbe (E*K*mid)], summed by dsgcn_colsum.  The passes themselves are dynadj_common.h's; this file
// has the node-typed select, D and CH = 8.
#include "dynadj_common.h"

namespace {

constexpr int KSUB = 3;
constexpr int LDT = KB_LDT;
constexpr int NTF = 256;         // forward workgroup
constexpr int NTB = 1024;        // backward workgroup: thread = joint pair (V*V <= 1024)
constexpr int NWB = NTB / DSGCN_WAVE;
constexpr int MAXM = 64, MAXV = 32, MAXE = 16;
constexpr int CH = 8;            // channels per round of the backward's class bins
constexpr int F_EDGE = 1, F_ADD = 2;

struct TypDims { int n, mid, V, E, flags; };

__global__ __launch_bounds__(256) void k_dyntyped_select_fwd(const float* __restrict__ proj,
                                                             const int* __restrict__ node_type, float* __restrict__ x12,
                                                             int n, int KM, int P, int V, int ld) {
  const size_t total = (size_t)n * KM * 2 * LDT;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int v = (int)(i & (LDT - 1));
    const size_t q = i >> 5;                       // (sample, row, slot)
    const int s = (int)(q & 1);
    const size_t nr = q >> 1;
    const int r = (int)(nr % KM);
    const size_t nn = nr / KM;
    float val = 0.f;
    if (v < V) {
      const int p = P > 1 ? node_type[v] : 0;
      val = proj[(nn * 2 * KM * P + (size_t)s * KM * P + (size_t)r * P + p) * ld + v];
    }
    x12[i] = val;
  }
}

// dproj: only row (r*P + tau(v)) of joint v is non-zero; padding columns are zero
__global__ __launch_bounds__(256) void k_dyntyped_select_bwd(const float* __restrict__ dx12,
                                                             const int* __restrict__ node_type, float* __restrict__ dproj,
                                                             int n, int KM, int P, int V, int ld) {
  const size_t rows = (size_t)2 * KM * P, total = (size_t)n * rows * ld;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int v = (int)(i % ld);
    const size_t q = i / ld;
    const int row = (int)(q % rows);
    const size_t nn = q / rows;
    const int s = row / (KM * P), rr = row - s * KM * P, r = rr / P, p = rr - r * P;
    float val = 0.f;
    if (v < V && (P == 1 || node_type[v] == p)) val = dx12[((nn * KM + r) * 2 + s) * LDT + v];
    dproj[i] = val;
  }
}

// X1 / X2 of subset k (mid x V, LDS) from x12, then S = softmax_u(sum_c X1[c,u] X2[c,w]) (fixed c order)
__device__ __forceinline__ void typed_prepare(int m, int V, int nt, const float* __restrict__ xs, float* X1, float* X2,
                                              float* S, float* cmx, float* cinv) {
  for (int o = threadIdx.x; o < m * V; o += nt) {
    const int c = o / V, v = o - c * V;
    X1[o] = xs[c * 2 * LDT + v];
    X2[o] = xs[c * 2 * LDT + LDT + v];
  }
  __syncthreads();
  kb_gram(m, V, nt, X1, X2, S);
  __syncthreads();
  kb_col_softmax(V, nt, S, cmx, cinv, 1);
}

// D of (c, u, w) for subset k
__device__ __forceinline__ float typed_D(const TypDims& d, int k, int c, int u, int w, int e, const float* X1,
                                         const float* X2, const float* __restrict__ pq_n, const float* __restrict__ be) {
  const int m = d.mid, V = d.V;
  const float diff = X1[c * V + u] - X2[c * V + w];
  if (!(d.flags & F_EDGE)) return diff;
  const int row = (k * d.E + e) * m + c;
  const float* p = pq_n + (size_t)row * 2 * LDT;
  const float att = (p[u] + be[row]) - p[LDT + w];
  return (d.flags & F_ADD) ? diff + att : att;
}

// grid (n, 3, windows)
template <int VT>
__global__ __launch_bounds__(NTF) void k_dyntyped_fwd(TypDims d, const float* __restrict__ x12,
                                                      const float* __restrict__ pq, const float* __restrict__ be,
                                                      const float* __restrict__ A, const float* __restrict__ alpha,
                                                      const float* __restrict__ beta, const int* __restrict__ edge_type,
                                                      float* __restrict__ ahat) {
  __shared__ float X1[MAXM * MAXV], X2[MAXM * MAXV], S[MAXV * MAXV], cmx[MAXV], cinv[MAXV];
  __shared__ int ET[MAXV * MAXV];
  if (VT) d.V = VT;
  const int m = d.mid, V = d.V, VV = V * V;
  const int n = blockIdx.x, k = blockIdx.y;
  int pc0, pm;
  kb_window(m, (int)blockIdx.z, (int)gridDim.z, pc0, pm);
  if (d.flags & F_EDGE)
    for (int i = threadIdx.x; i < VV; i += NTF) ET[i] = edge_type[i];
  typed_prepare(m, V, NTF, x12 + ((size_t)n * KSUB + k) * m * 2 * LDT, X1, X2, S, cmx, cinv);
  const float* pq_n = (d.flags & F_EDGE) ? pq + (size_t)n * d.E * KSUB * m * 2 * LDT : nullptr;
  kb_ahat_window(V, NTF, pc0, pm, d.flags & F_EDGE, ET, A + k * VV, alpha[k], beta[k], S,
                 ahat + ((size_t)n * KSUB + k) * m * VV,
                 [&](int c, int u, int w, int e) { return typed_D(d, k, c, u, w, e, X1, X2, pq_n, be); });
}

// grid (n, 3): workgroup = (sample, subset), all channels
template <int VT>
__global__ __launch_bounds__(NTB) void k_dyntyped_bwd(TypDims d, const float* __restrict__ x12,
                                                      const float* __restrict__ pq, const float* __restrict__ be,
                                                      const float* __restrict__ alpha, const float* __restrict__ beta,
                                                      const int* __restrict__ edge_type, const float* __restrict__ dahat,
                                                      float* dd, float* __restrict__ dx12, float* __restrict__ dpq,
                                                      float* __restrict__ ppar, int pstride) {
  __shared__ float X1[MAXM * MAXV], X2[MAXM * MAXV], S[MAXV * MAXV], SC[MAXV * MAXV], cmx[MAXV], cinv[MAXV];
  __shared__ int ET[MAXV * MAXV];
  __shared__ float bins[MAXE * CH * MAXV];
  __shared__ float red[2][NWB];
  if (VT) d.V = VT;
  const int tid = threadIdx.x;
  const int m = d.mid, V = d.V, VV = V * V, E = d.E;
  const bool edge = d.flags & F_EDGE, direct = !edge || (d.flags & F_ADD);
  const int n = blockIdx.x, k = blockIdx.y;
  if (edge)
    for (int i = tid; i < VV; i += NTB) ET[i] = edge_type[i];
  typed_prepare(m, V, NTB, x12 + ((size_t)n * KSUB + k) * m * 2 * LDT, X1, X2, S, cmx, cinv);
  const float* pq_n = edge ? pq + (size_t)n * E * KSUB * m * 2 * LDT : nullptr;
  const float* g_k = dahat + ((size_t)n * KSUB + k) * m * VV;
  float* dd_k = dd + ((size_t)n * KSUB + k) * m * VV;
  float* par = ppar + (size_t)n * pstride;
  const float al = alpha[k], bk = beta[k];

  float pal = 0.f, pbe = 0.f;
  kb_pass1(m, V, NTB, edge, ET, g_k, dd_k, al, S, SC, par, k * VV,
           [&](int c, int u, int w, int e) { return typed_D(d, k, c, u, w, e, X1, X2, pq_n, be); }, pal, pbe);
  __syncthreads();                 // (also: the dd_k writes of this workgroup are visible to it below)
  if (tid < V) kb_softmax_bwd(V, tid, S, SC, bk);
  __syncthreads();
  // dx12 of this subset: Gram backward (+ the direct row / column sums of dD); thread = (c, j), padding columns zero
  float* dxs = dx12 + ((size_t)n * KSUB + k) * m * 2 * LDT;
  for (int o = tid; o < m * LDT; o += NTB) {
    const int c = o / LDT, j = o - c * LDT;
    float v1 = 0.f, v2 = 0.f;
    if (j < V) {
      float rs, cs, g1, g2;
      kb_gram_bwd(V, c, j, direct, dd_k, SC, X1, X2, rs, cs, g1, g2);
      v1 = rs + g1;
      v2 = g2 - cs;
    }
    dxs[c * 2 * LDT + j] = v1;
    dxs[c * 2 * LDT + LDT + j] = v2;
  }
  if (edge)
    kb_edge_bins<CH>(m, V, E, NTB, ET, dd_k, bins, dpq + (size_t)n * E * KSUB * m * 2 * LDT, par + KSUB * VV + 2 * KSUB,
                     k * E);
  kb_reduce2_put(pal, pbe, red);
  __syncthreads();
  kb_reduce2_get(red, par, KSUB * VV + k, KSUB);
}

int grid_1d(size_t total) {
  const size_t b = (total + 255) / 256;
  return (int)(b < 65536 ? (b ? b : 1) : 65536);
}

bool dims_ok(int n, int mid, int V, int E, int flags) {
  return n > 0 && mid > 0 && mid <= MAXM && V > 0 && V <= MAXV && (!(flags & F_EDGE) || (E > 0 && E <= MAXE)) &&
         flags >= 0 && flags <= (F_EDGE | F_ADD);
}

}  // namespace

extern "C" {

int dsgcn_dyntyped_select_fwd(const float* proj, const int* node_type, float* x12, int n, int KM, int P, int V, int ld,
                              void* stream) {
  if (!proj || !x12 || n <= 0 || KM <= 0 || P <= 0 || V <= 0 || V > LDT || ld < V || (P > 1 && !node_type))
    return DSGCN_EINVAL;
  hipLaunchKernelGGL(k_dyntyped_select_fwd, dim3(grid_1d((size_t)n * KM * 2 * LDT)), dim3(256), 0, (hipStream_t)stream,
                     proj, node_type, x12, n, KM, P, V, ld);
  DSGCN_LAUNCH_CHECK();
  return 0;
}

int dsgcn_dyntyped_select_bwd(const float* dx12, const int* node_type, float* dproj, int n, int KM, int P, int V, int ld,
                              void* stream) {
  if (!dx12 || !dproj || n <= 0 || KM <= 0 || P <= 0 || V <= 0 || V > LDT || ld < V || (P > 1 && !node_type))
    return DSGCN_EINVAL;
  hipLaunchKernelGGL(k_dyntyped_select_bwd, dim3(grid_1d((size_t)n * 2 * KM * P * ld)), dim3(256), 0,
                     (hipStream_t)stream, dx12, node_type, dproj, n, KM, P, V, ld);
  DSGCN_LAUNCH_CHECK();
  return 0;
}

int dsgcn_dyntyped_partial_stride(int mid, int V, int E, int flags) {
  return KSUB * V * V + 2 * KSUB + ((flags & F_EDGE) ? E * KSUB * mid : 0);
}

int dsgcn_dyntyped_fwd(const float* x12, const float* pq, const float* be, const float* A, const float* alpha,
                       const float* beta, const int* edge_type, float* ahat, int n, int mid, int V, int E, int flags,
                       void* stream) {
  if (!x12 || !A || !alpha || !beta || !ahat) return DSGCN_EINVAL;
  if ((flags & F_EDGE) && (!pq || !be || !edge_type)) return DSGCN_EINVAL;
  if (!dims_ok(n, mid, V, E, flags)) return DSGCN_EUNSUPPORTED;
  const int windows = (mid + 7) / 8;      // channel windows of <= 8 channels: 3 * n * windows workgroups
  TypDims d{n, mid, V, E, flags};
#define TYP_FWD(VT)                                                                                                    \
  hipLaunchKernelGGL((k_dyntyped_fwd<VT>), dim3(n, KSUB, windows), dim3(NTF), 0, (hipStream_t)stream, d, x12, pq, be, \
                     A, alpha, beta, edge_type, ahat);
  KB_DISPATCH_V(TYP_FWD)
#undef TYP_FWD
  DSGCN_LAUNCH_CHECK();
  return 0;
}

int dsgcn_dyntyped_bwd(const float* x12, const float* pq, const float* be, const float* alpha, const float* beta,
                       const int* edge_type, const float* dahat, float* dd_ws, float* dx12, float* dpq, float* ppar,
                       int pstride, int n, int mid, int V, int E, int flags, void* stream) {
  if (!x12 || !alpha || !beta || !dahat || !dd_ws || !dx12 || !ppar) return DSGCN_EINVAL;
  if ((flags & F_EDGE) && (!pq || !be || !edge_type || !dpq)) return DSGCN_EINVAL;
  if (!dims_ok(n, mid, V, E, flags)) return DSGCN_EUNSUPPORTED;
  if (pstride < dsgcn_dyntyped_partial_stride(mid, V, E, flags)) return DSGCN_EINVAL;
  TypDims d{n, mid, V, E, flags};
#define TYP_BWD(VT)                                                                                                    \
  hipLaunchKernelGGL((k_dyntyped_bwd<VT>), dim3(n, KSUB), dim3(NTB), 0, (hipStream_t)stream, d, x12, pq, be, alpha,   \
                     beta, edge_type, dahat, dd_ws, dx12, dpq, ppar, pstride);
  KB_DISPATCH_V(TYP_BWD)
#undef TYP_BWD
  DSGCN_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
