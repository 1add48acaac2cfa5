// The passes the typed / flags / plain K-B variants (dynadj_typed.hip, dynadj_flags.hip, dynadj_plain.hip) have in
// common, one statement of each.  Where the variants differ in behaviour the difference is a parameter: the LDS type of
// the edge classes (ET_t), the accumulator of the direct row / column sums (Acc), the channels per bin round (CH), the
// first row of the subset's edge-linear outputs (e0) and D itself (DFn: (c, u, w, e) -> D[c,u,w] of the workgroup's subset).
// Every sum runs in a fixed order (c, u, w ascending); `nt` is the workgroup size.  csrc/dynadj.hip (the shipped flag
// set: MFMA tiles, hosted BatchNorm jobs) shares none of this.
#pragma once
#include "common.h"

constexpr int KB_LDT = 32;       // joint stride of the x12 / pq rows

#define KB_DISPATCH_V(L)  \
  if (V == 25) L(25)      \
  else if (V == 17) L(17) \
  else L(0)

// channel window `idx` of `cnt` over m channels: [pc0, pc0 + pm)
__device__ __forceinline__ void kb_window(int m, int idx, int cnt, int& pc0, int& pm) {
  pc0 = (m * idx) / cnt;
  pm = (m * (idx + 1)) / cnt - pc0;
}

// G[u,w] = sum_c X1[c,u] X2[c,w] (fma, c ascending); no barrier
__device__ __forceinline__ void kb_gram(int m, int V, int nt, const float* X1, const float* X2, float* G) {
  for (int i = threadIdx.x; i < V * V; i += nt) {
    const int u = i / V, w = i - u * V;
    float g = 0.f;
    for (int c = 0; c < m; ++c) g = fmaf(X1[c * V + u], X2[c * V + w], g);
    G[i] = g;
  }
}

// S <- softmax over u of each column w, in place; column w keeps its max in cmx[w * stride], 1 / sum in cinv[w * stride]
__device__ __forceinline__ void kb_col_softmax(int V, int nt, float* S, float* cmx, float* cinv, int stride) {
  const int tid = threadIdx.x;
  if (tid < V) {
    const int w = tid;
    float mx = -INFINITY;
    for (int u = 0; u < V; ++u) mx = fmaxf(mx, S[u * V + w]);
    float ssum = 0.f;
    for (int u = 0; u < V; ++u) ssum += expf(S[u * V + w] - mx);
    cmx[w * stride] = mx;
    cinv[w * stride] = 1.f / ssum;
  }
  __syncthreads();
  for (int i = tid; i < V * V; i += nt) {
    const int w = i % V;
    S[i] = expf(S[i] - cmx[w * stride]) * cinv[w * stride];
  }
  __syncthreads();
}

// the forward tail over the channel window [pc0, pc0 + pm): out[c,u,w] = A[u,w] + al tanh(D[c,u,w]) + bt S[u,w]
template <class ET_t, class DFn>
__device__ __forceinline__ void kb_ahat_window(int V, int nt, int pc0, int pm, bool edge, const ET_t* ET, const float* Ak,
                                               float al, float bt, const float* S, float* out, DFn D) {
  const int VV = V * V;
  for (int i = threadIdx.x; i < pm * VV; i += nt) {
    const int cl = i / VV, r = i - cl * VV;
    const int u = r / V, w = r - u * V, c = pc0 + cl;
    const float dk = D(c, u, w, edge ? (int)ET[r] : 0);
    out[(size_t)c * VV + r] = Ak[r] + al * tanhf(dk) + bt * S[r];
  }
}

// backward pass 1: thread = (u, w), channels in order: dD -> dd_k, sum_c dAhat -> SC and par[p0 + r]; the thread's dalpha /
// dbeta partials are added to pal / pbe
template <class ET_t, class DFn>
__device__ __forceinline__ void kb_pass1(int m, int V, int nt, bool edge, const ET_t* ET, const float* g_k, float* dd_k,
                                         float al, const float* S, float* SC, float* par, int p0, DFn D,
                                         float& pal, float& pbe) {
  const int VV = V * V;
  for (int r = threadIdx.x; r < VV; r += nt) {
    const int u = r / V, w = r - u * V, e = edge ? (int)ET[r] : 0;
    float sc = 0.f, pa = 0.f;
    for (int c = 0; c < m; ++c) {
      const float gv = g_k[(size_t)c * VV + r];
      const float th = tanhf(D(c, u, w, e));
      sc += gv;
      pa = fmaf(th, gv, pa);
      dd_k[(size_t)c * VV + r] = al * (1.f - th * th) * gv;
    }
    SC[r] = sc;
    par[p0 + r] = sc;
    pbe = fmaf(S[r], sc, pbe);
    pal += pa;
  }
}

// softmax backward of column w: SC <- dG = S * (bk*SC - sum_u S*bk*SC)
__device__ __forceinline__ void kb_softmax_bwd(int V, int w, const float* S, float* SC, float bk) {
  float dot = 0.f;
  for (int u = 0; u < V; ++u) dot = fmaf(S[u * V + w], bk * SC[u * V + w], dot);
  for (int u = 0; u < V; ++u) SC[u * V + w] = S[u * V + w] * (bk * SC[u * V + w] - dot);
}

// (c, j) of the Gram backward: g1 = sum_w dG[j,w] X2[c,w], g2 = sum_u dG[u,j] X1[c,u], and under `direct` the row / column
// sums rs / cs of dD[c] accumulated in Acc
template <class Acc>
__device__ __forceinline__ void kb_gram_bwd(int V, int c, int j, bool direct, const float* dd_k, const float* dG,
                                            const float* X1, const float* X2, Acc& rs, Acc& cs, float& g1, float& g2) {
  rs = cs = 0;
  if (direct) {
    const float* dk = dd_k + (size_t)c * (V * V);
    for (int w = 0; w < V; ++w) rs += (Acc)dk[j * V + w];
    for (int u = 0; u < V; ++u) cs += (Acc)dk[u * V + j];
  }
  g1 = g2 = 0.f;
  for (int w = 0; w < V; ++w) g1 = fmaf(dG[j * V + w], X2[c * V + w], g1);
  for (int u = 0; u < V; ++u) g2 = fmaf(dG[u * V + j], X1[c * V + u], g2);
}

// the edge linear's gradients from dD: class-masked row (slot 0: dP_e[c,u]) / column (slot 1: dQ_e[c,w] = -sum) sums, CH
// channels per round; thread (cl, x) owns bins[*][cl][x] (E * CH * V floats).  Row (e0 + e) * m + c of dpq_n (2 x 32 floats,
// padding columns zero) and of dbe (= sum_u dP_e[c,u]).  Barriers inside: every thread of the workgroup calls it.
template <int CH, class ET_t>
__device__ __forceinline__ void kb_edge_bins(int m, int V, int E, int nt, const ET_t* ET, const float* dd_k, float* bins,
                                             float* dpq_n, float* dbe, int e0) {
  const int tid = threadIdx.x, VV = V * V;
  for (int c0 = 0; c0 < m; c0 += CH) {
    for (int slot = 0; slot < 2; ++slot) {
      if (tid < CH * V) {
        const int cl = tid / V, x = tid - cl * V, c = c0 + cl;
        for (int e = 0; e < E; ++e) bins[(e * CH + cl) * V + x] = 0.f;
        if (c < m) {
          const float* dk = dd_k + (size_t)c * VV;
          if (slot == 0) {
            for (int y = 0; y < V; ++y) bins[(ET[x * V + y] * CH + cl) * V + x] += dk[x * V + y];
          } else {
            for (int y = 0; y < V; ++y) bins[(ET[y * V + x] * CH + cl) * V + x] -= dk[y * V + x];
          }
        }
      }
      __syncthreads();
      for (int o = tid; o < E * CH * KB_LDT; o += nt) {
        const int x = o & (KB_LDT - 1), q = o >> 5, e = q / CH, cl = q - e * CH, c = c0 + cl;
        if (c < m)
          dpq_n[((size_t)(e0 + e) * m + c) * 2 * KB_LDT + slot * KB_LDT + x] = x < V ? bins[(e * CH + cl) * V + x] : 0.f;
      }
      if (slot == 0) {
        for (int o = tid; o < E * CH; o += nt) {
          const int e = o / CH, cl = o - e * CH, c = c0 + cl;
          if (c < m) {
            float acc = 0.f;
            for (int x = 0; x < V; ++x) acc += bins[(e * CH + cl) * V + x];
            dbe[(e0 + e) * m + c] = acc;
          }
        }
      }
      __syncthreads();
    }
  }
}

// block sum of two per-thread scalars, waves added in order: kb_reduce2_put, a barrier of the caller's, kb_reduce2_get
// (thread t < 2 writes sum t to out[o0 + t * stride])
template <int NW>
__device__ __forceinline__ void kb_reduce2_put(float a, float b, float (*red)[NW]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float ra = wave_sum(a), rb = wave_sum(b);
  if (lane == 0) { red[0][wave] = ra; red[1][wave] = rb; }
}

template <int NW>
__device__ __forceinline__ void kb_reduce2_get(const float (*red)[NW], float* out, int o0, int stride) {
  const int tid = threadIdx.x;
  if (tid < 2) {
    float r = 0.f;
    for (int i = 0; i < NW; ++i) r += red[tid][i];
    out[o0 + tid * stride] = r;
  }
}
