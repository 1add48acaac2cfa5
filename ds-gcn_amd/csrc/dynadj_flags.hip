// K-B flags: the dynamic adjacency of dgphgcn1 (reference: pyskl/models/gcns/utils/gcn.py:2074-2370) for the flag sets
// other than the shipped one (which stays on csrc/dynadj.hip): the DS-GCN ablation arms.  One kernel pair, specialised at
// compile time by a flag word F:
//   F & 3  (SEM)   0 = decompose off: three plain subsets, proj rows [conv1 (3*mid) | conv2 (3*mid)]
//                  1 = decompose, untyped semantic rows: proj rows [conv1 (2*mid) | conv2 (2*mid) | conv1_se (mid)]
//                  2 = decompose, node-typed semantic rows: conv1_se has mid*P rows, joint v keeps row c*P + tau(v)
//                  Under decompose subset 2 pairs the conv1_se rows with THEMSELVES (the reference never calls conv2_se).
//   F & 4  (EDGE)  the edge-typed linear on subset 1: pq (n, E*mid, 2, 32) = We . [x1_1 | x2_1] (one K-C launch, no bias),
//                  D[1,c,u,w] = (pq0[eps(u,w),c,u] + be[eps,c]) - pq1[eps(u,w),c,w].  Absent: plain differences, no pq, no
//                  be partials, no class bins.
//   F & 8  (ADA)   the class-mixed Gram: G'[k,u,w] = sum_k' Wa[k*E + eps(u,w), k'] G[k',u,w] + ba[k*E + eps(u,w)] before
//                  the softmax over u; the backward gives dWa (3E, 3), dba (3E) and dG.
//   F & 16 (SW)    per-subset alpha / beta (alpha[k]); absent: alpha[0] / beta[0] scale every subset.
//   Ahat[k,c,u,w] = A[k,u,w] + alpha tanh(D[k,c,u,w]) + beta softmax_u(G'[k])[u,w]
//
// Forward: workgroup = (sample, subset, channel window).  Backward: workgroup = (sample, subset), or (sample) over the three
// subsets in order under ADA (the mix couples them).  Partials per sample [sum_c dAhat (3*V*V) | dalpha_k (3) | dbeta_k (3) |
// dbe (E*mid, EDGE) | dWa (9E) | dba (3E) (ADA)], summed by dsgcn_colsum.  The Gram, the softmax and the backward passes are
// dynadj_common.h's; this file has the row layouts, the class mix, the fp64 row / column sums of dD and CH = 8 / 4.
#include "dynadj_common.h"

namespace {

constexpr int KSUB = 3;
constexpr int LDT = KB_LDT;
constexpr int NTF = 256;         // forward workgroup
constexpr int NTB = 1024;        // backward workgroup
constexpr int NWB = NTB / DSGCN_WAVE;
constexpr int MAXM = 64, MAXV = 32, MAXE = 16, MAXP = 16;
constexpr int F_SEM = 3, F_EDGE = 4, F_ADA = 8, F_SW = 16;

struct FlagDims { int n, mid, V, E, P, ld; };

// proj rows of (subset k, channel c): x1 / x2; tau = node type of the joint (0 unless SEM == 2)
template <int SEM>
__device__ __forceinline__ void flag_rows(int m, int P, int k, int c, int tau, int& r1, int& r2) {
  if (SEM == 0) {
    r1 = k * m + c;
    r2 = KSUB * m + k * m + c;
  } else if (k < 2) {
    r1 = k * m + c;
    r2 = 2 * m + k * m + c;
  } else {
    r1 = r2 = 4 * m + (SEM == 2 ? c * P + tau : c);
  }
}

template <int SEM>
__device__ __forceinline__ void flag_load(const FlagDims& d, int k, int nt, const float* __restrict__ pn,
                                          const unsigned char* NT, float* X1, float* X2) {
  const int m = d.mid, V = d.V;
  for (int o = threadIdx.x; o < m * V; o += nt) {
    const int c = o / V, v = o - c * V;
    int r1, r2;
    flag_rows<SEM>(m, d.P, k, c, SEM == 2 ? (int)NT[v] : 0, r1, r2);
    X1[o] = pn[(size_t)r1 * d.ld + v];
    X2[o] = pn[(size_t)r2 * d.ld + v];
  }
}

__device__ __forceinline__ void flag_types(const FlagDims& d, bool want_et, bool want_nt, int nt,
                                           const int* __restrict__ edge_type, const int* __restrict__ node_type,
                                           unsigned char* ET, unsigned char* NT) {
  if (want_et)
    for (int i = threadIdx.x; i < d.V * d.V; i += nt) ET[i] = (unsigned char)min(max(edge_type[i], 0), d.E - 1);
  if (want_nt)
    for (int i = threadIdx.x; i < d.V; i += nt) NT[i] = (unsigned char)min(max(node_type[i], 0), d.P - 1);
}

template <bool EDGE>
__device__ __forceinline__ float flag_D(int m, int V, int k, int c, int u, int w, int e, const float* X1, const float* X2,
                                        const float* __restrict__ pq_n, const float* __restrict__ be) {
  if (EDGE && k == 1) {
    const int row = e * m + c;
    const float* p = pq_n + (size_t)row * 2 * LDT;
    return (p[u] + be[row]) - p[LDT + w];
  }
  return X1[c * V + u] - X2[c * V + w];
}

// grid (n, 3, windows)
template <int F, int VT>
__global__ __launch_bounds__(NTF) void k_dynflag_fwd(FlagDims d, const float* __restrict__ proj,
                                                     const float* __restrict__ pq, const float* __restrict__ be,
                                                     const float* __restrict__ wa, const float* __restrict__ ba,
                                                     const float* __restrict__ A, const float* __restrict__ alpha,
                                                     const float* __restrict__ beta, const int* __restrict__ node_type,
                                                     const int* __restrict__ edge_type, float* __restrict__ ahat) {
  constexpr int SEM = F & F_SEM;
  constexpr bool EDGE = (F & F_EDGE) != 0, ADA = (F & F_ADA) != 0, SW = (F & F_SW) != 0;
  constexpr int KG = ADA ? KSUB : 1;
  __shared__ float X1[MAXM * MAXV], X2[MAXM * MAXV], S[MAXV * MAXV], GR[KG * MAXV * MAXV], cmx[MAXV], cinv[MAXV];
  __shared__ unsigned char ET[MAXV * MAXV], NT[MAXV];
  if (VT) d.V = VT;
  const int m = d.mid, V = d.V, VV = V * V;
  const int n = blockIdx.x, k = blockIdx.y;
  int pc0, pm;
  kb_window(m, (int)blockIdx.z, (int)gridDim.z, pc0, pm);
  const int R = SEM == 0 ? 2 * KSUB * m : 4 * m + m * d.P;
  const float* pn = proj + (size_t)n * R * d.ld;
  flag_types(d, EDGE || ADA, SEM == 2, NTF, edge_type, node_type, ET, NT);
  __syncthreads();
  if (ADA) {
    for (int kk = 0; kk < KSUB; ++kk) {
      flag_load<SEM>(d, kk, NTF, pn, NT, X1, X2);
      __syncthreads();
      kb_gram(m, V, NTF, X1, X2, GR + kk * VV);
      __syncthreads();
    }
    flag_load<SEM>(d, k, NTF, pn, NT, X1, X2);
    for (int i = threadIdx.x; i < VV; i += NTF) {
      const int row = k * d.E + ET[i];
      float g = ba[row];
      for (int kk = 0; kk < KSUB; ++kk) g = fmaf(wa[row * KSUB + kk], GR[kk * VV + i], g);
      S[i] = g;
    }
  } else {
    flag_load<SEM>(d, k, NTF, pn, NT, X1, X2);
    __syncthreads();
    kb_gram(m, V, NTF, X1, X2, S);
  }
  __syncthreads();
  kb_col_softmax(V, NTF, S, cmx, cinv, 1);
  const float* pq_n = EDGE ? pq + (size_t)n * d.E * m * 2 * LDT : nullptr;
  kb_ahat_window(V, NTF, pc0, pm, EDGE, ET, A + k * VV, alpha[SW ? k : 0], beta[SW ? k : 0], S,
                 ahat + ((size_t)n * KSUB + k) * m * VV,
                 [&](int c, int u, int w, int e) { return flag_D<EDGE>(m, V, k, c, u, w, e, X1, X2, pq_n, be); });
}

// grid (n, 3), or (n, 1) under ADA
template <int F, int VT>
__global__ __launch_bounds__(NTB) void k_dynflag_bwd(FlagDims d, const float* __restrict__ proj,
                                                     const float* __restrict__ pq, const float* __restrict__ be,
                                                     const float* __restrict__ wa, const float* __restrict__ ba,
                                                     const float* __restrict__ alpha, const float* __restrict__ beta,
                                                     const int* __restrict__ node_type, const int* __restrict__ edge_type,
                                                     const float* __restrict__ dahat, float* dd, float* __restrict__ dproj,
                                                     float* __restrict__ dpq, float* __restrict__ ppar, int pstride) {
  constexpr int SEM = F & F_SEM;
  constexpr bool EDGE = (F & F_EDGE) != 0, ADA = (F & F_ADA) != 0, SW = (F & F_SW) != 0;
  constexpr int KG = ADA ? KSUB : 1;
  constexpr int CH = ADA ? 4 : 8;          // channels per round of the class bins (LDS budget under ADA)
  constexpr int PL = MAXV * MAXV;
  __shared__ float X1[MAXM * MAXV], X2[MAXM * MAXV], S[KG * PL], SC[KG * PL], GR[ADA ? KSUB * PL : 1];
  __shared__ float cmx[MAXV], cinv[MAXV];
  __shared__ unsigned char ET[MAXV * MAXV], NT[MAXV];
  __shared__ float bins[EDGE ? MAXE * CH * MAXV : 1];
  __shared__ float red[2][NWB];
  if (VT) d.V = VT;
  const int tid = threadIdx.x;
  const int m = d.mid, V = d.V, VV = V * V, E = d.E, P = d.P, ld = d.ld;
  const int n = blockIdx.x;
  const int R = SEM == 0 ? 2 * KSUB * m : 4 * m + m * P;
  const float* pn = proj + (size_t)n * R * ld;
  float* dpn = dproj + (size_t)n * R * ld;
  const float* pq_n = EDGE ? pq + (size_t)n * E * m * 2 * LDT : nullptr;
  float* par = ppar + (size_t)n * pstride;
  flag_types(d, EDGE || ADA, SEM == 2, NTB, edge_type, node_type, ET, NT);
  __syncthreads();

  if (ADA) {
    // raw Grams of the three subsets, then the class mix and the softmax of each
#pragma unroll 1
    for (int kk = 0; kk < KSUB; ++kk) {
      flag_load<SEM>(d, kk, NTB, pn, NT, X1, X2);
      __syncthreads();
      kb_gram(m, V, NTB, X1, X2, GR + kk * PL);
      __syncthreads();
    }
#pragma unroll 1
    for (int kq = 0; kq < KSUB; ++kq) {
      for (int i = tid; i < VV; i += NTB) {
        const int row = kq * E + ET[i];
        float g = ba[row];
        for (int kk = 0; kk < KSUB; ++kk) g = fmaf(wa[row * KSUB + kk], GR[kk * PL + i], g);
        S[kq * PL + i] = g;
      }
      __syncthreads();
      kb_col_softmax(V, NTB, S + kq * PL, cmx, cinv, 1);
    }
  }

  const int k_lo = ADA ? 0 : (int)blockIdx.y, k_hi = ADA ? KSUB : k_lo + 1;
  // phase 1 per subset: dD -> workspace, sum_c dAhat, dalpha / dbeta partials, softmax backward (SC <- dG')
#pragma unroll 1
  for (int k = k_lo; k < k_hi; ++k) {
    float* Sk = S + (ADA ? k : 0) * PL;
    float* SCk = SC + (ADA ? k : 0) * PL;
    flag_load<SEM>(d, k, NTB, pn, NT, X1, X2);
    __syncthreads();
    if (!ADA) {
      kb_gram(m, V, NTB, X1, X2, Sk);
      __syncthreads();
      kb_col_softmax(V, NTB, Sk, cmx, cinv, 1);
    }
    const float* g_k = dahat + ((size_t)n * KSUB + k) * m * VV;
    float* dd_k = dd + ((size_t)n * KSUB + k) * m * VV;
    const float al = alpha[SW ? k : 0], bk = beta[SW ? k : 0];
    float pal = 0.f, pbe = 0.f;
    kb_pass1(m, V, NTB, EDGE, ET, g_k, dd_k, al, Sk, SCk, par, k * VV,
             [&](int c, int u, int w, int e) { return flag_D<EDGE>(m, V, k, c, u, w, e, X1, X2, pq_n, be); }, pal, pbe);
    kb_reduce2_put(pal, pbe, red);
    __syncthreads();                 // (also: the dd_k writes of this workgroup are visible to it below)
    kb_reduce2_get(red, par, KSUB * VV + k, KSUB);
    if (tid >= 64 && tid < 64 + V) kb_softmax_bwd(V, tid - 64, Sk, SCk, bk);
    __syncthreads();
  }

  if (ADA) {
    // the mix backward: dWa[k*E+e, k'] = sum_{eps=e} dG'[k] G[k'], dba[k*E+e] = sum_{eps=e} dG'[k] (pairs in order), then
    // dG[k'] = sum_k Wa[k*E+eps, k'] dG'[k] -> S (free after the softmax backward)
    float* pwa = par + KSUB * VV + 2 * KSUB + (EDGE ? E * m : 0);
    for (int o = tid; o < KSUB * E * (KSUB + 1); o += NTB) {
      const int row = o / (KSUB + 1), j = o - row * (KSUB + 1), kq = row / E, e = row - kq * E;
      float acc = 0.f;
      if (j < KSUB) {
#pragma unroll 4
        for (int i = 0; i < VV; ++i)
          if (ET[i] == e) acc = fmaf(SC[kq * PL + i], GR[j * PL + i], acc);
        pwa[row * KSUB + j] = acc;
      } else {
#pragma unroll 4
        for (int i = 0; i < VV; ++i)
          if (ET[i] == e) acc += SC[kq * PL + i];
        pwa[KSUB * E * KSUB + row] = acc;
      }
    }
    for (int i = tid; i < VV; i += NTB) {
      const int e = ET[i];
      for (int kk = 0; kk < KSUB; ++kk) {
        float g = 0.f;
        for (int kq = 0; kq < KSUB; ++kq) g = fmaf(wa[(kq * E + e) * KSUB + kk], SC[kq * PL + i], g);
        S[kk * PL + i] = g;
      }
    }
    __syncthreads();
  }

  // phase 2 per subset: dproj rows (Gram backward + the direct row / column sums of dD), the edge bins of subset 1
#pragma unroll 1
  for (int k = k_lo; k < k_hi; ++k) {
    const float* dG = ADA ? S + k * PL : SC;
    const float* dd_k = dd + ((size_t)n * KSUB + k) * m * VV;
    if (ADA) {
      __syncthreads();
      flag_load<SEM>(d, k, NTB, pn, NT, X1, X2);
      __syncthreads();
    }
    const bool direct = !(EDGE && k == 1);
    const bool sem = SEM != 0 && k == 2;
    for (int o = tid; o < m * LDT; o += NTB) {
      const int c = o / LDT, j = o - c * LDT;
      float v1 = 0.f, v2 = 0.f, v12 = 0.f;
      if (j < V) {
        // row / column sums of dD in fp64: on the semantic subset both land on the same conv1_se row, where their sums
        // over the joints cancel exactly in exact arithmetic (a shift of xs leaves xs[u] - xs[w] alone) — the bias
        // gradient is what is left of the Gram term, so the difference is formed before it is rounded to fp32
        double rs, cs;
        float g1, g2;
        kb_gram_bwd(V, c, j, direct, dd_k, dG, X1, X2, rs, cs, g1, g2);
        v1 = (float)rs + g1;
        v2 = g2 - (float)cs;
        v12 = (float)(rs - cs) + (g1 + g2);
      }
      if (j < ld) {
        if (!sem) {
          int r1, r2;
          flag_rows<SEM>(m, P, k, c, 0, r1, r2);
          dpn[(size_t)r1 * ld + j] = v1;
          dpn[(size_t)r2 * ld + j] = v2;
        } else if (SEM == 1) {
          dpn[(size_t)(4 * m + c) * ld + j] = v12;
        } else {
          const int tau = j < V ? (int)NT[j] : -1;
          for (int p = 0; p < P; ++p) dpn[(size_t)(4 * m + c * P + p) * ld + j] = p == tau ? v12 : 0.f;
        }
      }
    }
    // joint columns beyond 32 of a wider row stride
    for (int o = tid; o < m * (ld - LDT); o += NTB) {
      const int c = o / (ld - LDT), j = LDT + o - c * (ld - LDT);
      if (!sem) {
        int r1, r2;
        flag_rows<SEM>(m, P, k, c, 0, r1, r2);
        dpn[(size_t)r1 * ld + j] = 0.f;
        dpn[(size_t)r2 * ld + j] = 0.f;
      } else {
        const int PP = SEM == 2 ? P : 1;
        for (int p = 0; p < PP; ++p) dpn[(size_t)(4 * m + c * PP + p) * ld + j] = 0.f;
      }
    }
    if (EDGE && k == 1)
      kb_edge_bins<CH>(m, V, E, NTB, ET, dd_k, bins, dpq + (size_t)n * E * m * 2 * LDT, par + KSUB * VV + 2 * KSUB,
                       0);
  }
}

bool flags_ok(int flags) {
  const int sem = flags & F_SEM;
  return flags >= 0 && flags < 32 && sem <= 2 && !((flags & F_EDGE) && sem == 0);
}

bool dims_ok(int n, int mid, int V, int E, int P, int ld, int flags) {
  if (!flags_ok(flags)) return false;
  if (!(n > 0 && mid > 0 && mid <= MAXM && V > 0 && V <= MAXV && ld >= V)) return false;
  if ((flags & (F_EDGE | F_ADA)) && !(E > 0 && E <= MAXE)) return false;
  if ((flags & F_SEM) == 2 ? !(P > 0 && P <= MAXP) : P != 1) return false;
  return true;
}

}  // namespace

// every valid flag word (SEM 0 has no EDGE); V = 25 specialised, except the mixed-Gram backward (the specialised form
// of its three-subset loop needs more than the 128 registers a 1024-thread workgroup has)
#define FLAG_PLAIN(L, VT)                                                                                              \
    case 0: L(0, VT) break;   case 1: L(1, VT) break;   case 2: L(2, VT) break;   case 5: L(5, VT) break;              \
    case 6: L(6, VT) break;   case 16: L(16, VT) break; case 17: L(17, VT) break; case 18: L(18, VT) break;            \
    case 21: L(21, VT) break; case 22: L(22, VT) break;
#define FLAG_MIXED(L, VT)                                                                                              \
    case 8: L(8, VT) break;   case 9: L(9, VT) break;   case 10: L(10, VT) break; case 13: L(13, VT) break;            \
    case 14: L(14, VT) break; case 24: L(24, VT) break; case 25: L(25, VT) break; case 26: L(26, VT) break;            \
    case 29: L(29, VT) break; case 30: L(30, VT) break;
#define FLAG_DISPATCH_FWD(L)                                                                                           \
  if (V == 25) { switch (flags) { FLAG_PLAIN(L, 25) FLAG_MIXED(L, 25) default: return DSGCN_EUNSUPPORTED; } }          \
  else { switch (flags) { FLAG_PLAIN(L, 0) FLAG_MIXED(L, 0) default: return DSGCN_EUNSUPPORTED; } }
#define FLAG_DISPATCH_BWD(L)                                                                                           \
  if (V == 25 && !(flags & F_ADA)) { switch (flags) { FLAG_PLAIN(L, 25) default: return DSGCN_EUNSUPPORTED; } }        \
  else { switch (flags) { FLAG_PLAIN(L, 0) FLAG_MIXED(L, 0) default: return DSGCN_EUNSUPPORTED; } }

extern "C" {

int dsgcn_dynflag_partial_stride(int mid, int V, int E, int flags) {
  return KSUB * V * V + 2 * KSUB + ((flags & F_EDGE) ? E * mid : 0) + ((flags & F_ADA) ? KSUB * E * (KSUB + 1) : 0);
}

int dsgcn_dynflag_fwd(const float* proj, const float* pq, const float* be, const float* wa, const float* ba,
                      const float* A, const float* alpha, const float* beta, const int* node_type, const int* edge_type,
                      float* ahat, int n, int mid, int V, int ld, int P, int E, int flags, void* stream) {
  if (!proj || !A || !alpha || !beta || !ahat) return DSGCN_EINVAL;
  if (!dims_ok(n, mid, V, E, P, ld, flags)) return DSGCN_EUNSUPPORTED;
  if ((flags & F_EDGE) && (!pq || !be)) return DSGCN_EINVAL;
  if ((flags & F_ADA) && (!wa || !ba)) return DSGCN_EINVAL;
  if ((flags & (F_EDGE | F_ADA)) && !edge_type) return DSGCN_EINVAL;
  if ((flags & F_SEM) == 2 && !node_type) return DSGCN_EINVAL;
  const int windows = (mid + 7) / 8;      // channel windows of <= 8 channels: 3 * n * windows workgroups
  FlagDims d{n, mid, V, E, P, ld};
#define FLAG_FWD(FW, VT)                                                                                               \
  hipLaunchKernelGGL((k_dynflag_fwd<FW, VT>), dim3(n, KSUB, windows), dim3(NTF), 0, (hipStream_t)stream, d, proj, pq,  \
                     be, wa, ba, A, alpha, beta, node_type, edge_type, ahat);
  FLAG_DISPATCH_FWD(FLAG_FWD)
#undef FLAG_FWD
  DSGCN_LAUNCH_CHECK();
  return 0;
}

int dsgcn_dynflag_bwd(const float* proj, const float* pq, const float* be, const float* wa, const float* ba,
                      const float* alpha, const float* beta, const int* node_type, const int* edge_type,
                      const float* dahat, float* dd_ws, float* dproj, float* dpq, float* ppar, int pstride, int n,
                      int mid, int V, int ld, int P, int E, int flags, void* stream) {
  if (!proj || !alpha || !beta || !dahat || !dd_ws || !dproj || !ppar) return DSGCN_EINVAL;
  if (!dims_ok(n, mid, V, E, P, ld, flags)) return DSGCN_EUNSUPPORTED;
  if ((flags & F_EDGE) && (!pq || !be || !dpq)) return DSGCN_EINVAL;
  if ((flags & F_ADA) && (!wa || !ba)) return DSGCN_EINVAL;
  if ((flags & (F_EDGE | F_ADA)) && !edge_type) return DSGCN_EINVAL;
  if ((flags & F_SEM) == 2 && !node_type) return DSGCN_EINVAL;
  if (pstride < dsgcn_dynflag_partial_stride(mid, V, E, flags)) return DSGCN_EINVAL;
  FlagDims d{n, mid, V, E, P, ld};
#define FLAG_BWD(FW, VT)                                                                                               \
  hipLaunchKernelGGL((k_dynflag_bwd<FW, VT>), dim3(n, (FW & F_ADA) ? 1 : KSUB), dim3(NTB), 0, (hipStream_t)stream, d,  \
                     proj, pq, be, wa, ba, alpha, beta, node_type, edge_type, dahat, dd_ws, dproj, dpq, ppar, pstride);
  FLAG_DISPATCH_BWD(FLAG_BWD)
#undef FLAG_BWD
  DSGCN_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
