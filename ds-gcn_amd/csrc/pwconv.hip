// K-C: 1x1 channel mix ("pointwise conv") on the f32 matrix core, with the surrounding train-mode BatchNorm /
// ReLU / residual work folded into its load prologue and store epilogue.
// Replaces, per call, the reference's Conv2d(1x1) + BatchNorm2d + ReLU (+ residual add) ATen chains:
//   pyskl/models/gcns/utils/gcn.py:2165-2169,2209-2215,2236,2363-2365 (pre / post / down / bn of dgphgcn1)
//   pyskl/models/gcns/utils/tcn.py:379-404,409,422,427 (dgmstcn branch 1x1 convs, global joint, transform, bn)
//   pyskl/models/gcns/utils/tcn.py:21-28 with kernel_size=1 (block residual, dgstgcn.py:59)
//
//   v[n,ci,t,v]  = relu?( x1*s1[ci]+h1[ci] (+ x2*s2[ci]+h2[ci] | + x2) )        "virtual input": deferred BN of the
//   z[n,co,t',v] = sum_ci W[co,ci] * v[n,ci,t'*stride,v] + b[co]                 producer applied while loading
//   zaug[n,co,t'] = mean_v z  (= W . mean_v v + b: the dgmstcn "global joint" column, by linearity)
//   partial[blk,co,0:2] = sum / sum of squares of this block's outputs (incl. zaug)  -> batch statistics
//
// Work decomposition (k_pwconv_fwd2 / _dgrad2, below): wave-independent — each wave owns one 32-position tile of one
// sample and <= 64 output channels; the B operand comes straight from HBM in MFMA fragment shape (raw buffer loads), only
// the weights pass through LDS; per-channel sums leave through an LDS transpose, one partial row per block
// (deterministic two-stage BN statistics, finalised in fp64 by k_bn_finalize: reduce.hip).  wgrad stages both operands in
// LDS.  Bound: HBM for Ci,Co <= 64 (16 FLOP/B), f32 MFMA above (32-64 FLOP/B vs ridge ~20).
//
// This file, top to bottom: the first-generation kernels with the conv's own epilogue / prologue kernels (k_rowmean_stats,
// k_dz_eff_aug); the dispatch functions that choose between them and the family's later forms (pw4.hip, wgrad.hip,
// bwd64.hip, reached through kc.h); the C entry points of include/dsgcn.h, each of which fills the operand structs of kc.h
// once and hands them down.  The column sums and the BatchNorm reductions the conv's partial rows feed are in reduce.hip.
#include "kc.h"

namespace {

constexpr int KCH = 16;            // input channels per LDS chunk
constexpr int WSTR = KCH + 1;      // W tile row stride (odd)
constexpr int NTW = 2;             // N-tiles per wave (NPpad <= 256)
constexpr int PW_NT = 256;
constexpr int XCH = KCH / 4;       // channels staged per wave per chunk

struct PwArgs {
  const float* x1; const float* s1; const float* h1;
  const float* x2; const float* s2; const float* h2;
  int relu;
  const float* w; const float* bias;
  float* z; float* zaug; float* partial;
  int n, Ci, Co, T, V, Tout, stride, aug, TR, NPpad, vec, stats, roll, nbx, cc;
};

__device__ __forceinline__ float virt1(float a, float b, bool has2, float s1, float h1, float s2, float h2,
                                       int relu) {
  float v = fmaf(a, s1, h1);
  if (has2) v += fmaf(b, s2, h2);
  return relu ? fmaxf(v, 0.f) : v;
}

// ------------------------------------------------------------------------------------------------------------
// Wave-independent formulation (product path).  Each wave owns NW consecutive 32-position tiles of one sample and ALL
// output channels of its block (MT 32-channel tiles): the B operand (virtual input) comes straight from HBM in MFMA
// fragment shape — lane (pos, k-half) loads x[ci = k+half][pos]: two 128-B coalesced segments per instruction — with
// UNR k-steps in flight per wave, the deferred BN/ReLU/residual applied in registers; only the weights go through LDS
// (64-channel K chunks, shared by the 4 waves).  No barrier inside a K chunk, every input element is read once.
// ------------------------------------------------------------------------------------------------------------
constexpr int KW = 64;             // K (input-channel) chunk of the LDS weight tile
constexpr int KWS = KW + 1;

// MODE 0: v = x1 ; 1: v = relu?(x1*s1+h1) ; 2: v = relu?(x1*s1+h1 + x2*s2+h2)
// K is walked in groups of UNR k-steps (2 channels each) with two register sets in ping-pong: the loads of group
// g+1 are issued before the MFMAs of group g.  No per-step branches (they made hipcc sink every load next to its
// use: one full HBM round trip per k-step): the chunk is padded to a multiple of 4*UNR channels — padded channels
// have zero weights in Ws and read either valid memory or past the buffer (raw-buffer OOB -> 0).
constexpr int F2_UNR = 4;          // k-steps per register set for narrow inputs (Ci < 48)
constexpr int F2_UNRW = 4;         // ... for wide inputs: 16 k-steps x MFMAs ~ 4096 cycles of cover per set

template <int NW, int MODE, int UNR>
__device__ __forceinline__ void f2_load(float (&xb)[UNR][NW], float (&yb)[UNR][NW], __amdgpu_buffer_rsrc_t r1,
                                        __amdgpu_buffer_rsrc_t r2, const int (&voff)[NW], int cbase, int cstride4) {
#pragma unroll
  for (int u = 0; u < UNR; ++u) {
    const int soff = (cbase + 2 * u) * cstride4;              // wave-uniform: SGPR operand of the buffer load
#pragma unroll
    for (int j = 0; j < NW; ++j) {
      xb[u][j] = buf_load<1>(r1, voff[j], soff);
      if (MODE == 2) yb[u][j] = buf_load<1>(r2, voff[j], soff);
    }
  }
}

template <int MT, int NW, int MODE, int UNR>
__device__ __forceinline__ void f2_compute(const PwArgs& a, f32x16 (&acc)[MT][NW], const float* Ws, const f32x4* Ps4,
                                           const float (&xb)[UNR][NW], const float (&yb)[UNR][NW], int c0,
                                           int kbase, int kc, int half, int l31) {
#pragma unroll
  for (int u = 0; u < UNR; ++u) {
    const int kl = kbase + 2 * u + half;
    const bool cok = kl < kc;
    float av[MT], bv[NW];
#pragma unroll
    for (int m = 0; m < MT; ++m) av[m] = Ws[(32 * m + l31) * KWS + kl];
    f32x4 p = {1.f, 0.f, 1.f, 0.f};
    if (MODE != 0) p = Ps4[cok ? c0 + kl : 0];
#pragma unroll
    for (int j = 0; j < NW; ++j) {
      float v = xb[u][j];
      if (MODE != 0) {
        v = fmaf(v, p.x, p.y);
        if (MODE == 2) v += fmaf(yb[u][j], p.z, p.w);
        if (a.relu) v = fmaxf(v, 0.f);
      }
      bv[j] = cok ? v : 0.f;
    }
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int j = 0; j < NW; ++j)
        acc[m][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[m], bv[j], acc[m][j], 0, 0, 0);
  }
}

template <int MT, int NW, int MODE, int UNR>
__device__ __forceinline__ void fwd2_chunk(const PwArgs& a, f32x16 (&acc)[MT][NW], const float* Ws, const f32x4* Ps4,
                                           __amdgpu_buffer_rsrc_t r1, __amdgpu_buffer_rsrc_t r2, const int (&voff)[NW],
                                           int c0, int kc, int cstride4, int half, int l31) {
  constexpr int G = 2 * UNR;                                  // channels per register set
  float xa[UNR][NW], ya[UNR][NW], xb[UNR][NW], yb[UNR][NW];
  f2_load<NW, MODE, UNR>(xa, ya, r1, r2, voff, c0, cstride4);
  for (int k0 = 0; k0 < kc; k0 += 2 * G) {
    f2_load<NW, MODE, UNR>(xb, yb, r1, r2, voff, c0 + k0 + G, cstride4);
    f2_compute<MT, NW, MODE, UNR>(a, acc, Ws, Ps4, xa, ya, c0, k0, kc, half, l31);
    f2_load<NW, MODE, UNR>(xa, ya, r1, r2, voff, c0 + k0 + 2 * G, cstride4);
    if (k0 + G < kc) f2_compute<MT, NW, MODE, UNR>(a, acc, Ws, Ps4, xb, yb, c0, k0 + G, kc, half, l31);
  }
}

// XCD-aware block decode for the wave-independent kernels: the CC blocks that read the same input tile (one per 64-channel
// output chunk) get consecutive slots on the SAME XCD (blockIdx % 8 labels the XCD group, MI355X_MICROARCH.md), so the
// tile's lines are still in that XCD's L2 when the second..CC-th reader arrives; with the plain (x,y,z) order the readers
// are a whole tensor pass apart and every one of them goes to HBM / Infinity Cache.
struct PwBlk { int bx, n, cz; bool live; };
__device__ __forceinline__ PwBlk pw_decode(int nbx, int ntiles, int cc) {
  const int id = blockIdx.x;
  const int xcd = id & 7, slot = id >> 3;
  const int cz = slot % cc;
  const int tile = (slot / cc) * 8 + xcd;
  PwBlk b;
  b.live = tile < ntiles;
  b.cz = cz;
  b.n = tile / nbx;
  b.bx = tile - b.n * nbx;
  return b;
}

// Whole-chunk rolling prefetch (Ci a multiple of 64, one position tile per wave): the 32 B-operand registers of a
// 64-channel chunk are all in flight at once; each is refilled with the same k-step of the NEXT chunk right after its
// MFMAs have consumed it, and the next chunk's weight rows are fetched into registers during the MFMA phase, so a
// chunk boundary costs two raw s_barriers and an LDS write, not a memory round trip (the 4-k-step ping-pong above
// covers only ~512 cycles per set and re-exposes the latency at every chunk: MFMA pipe 40 % busy at 256 channels).
// The barriers are raw s_barrier + lgkmcnt(0): __syncthreads() would drain vmcnt(0) and with it the prefetch.
template <int MT, int MODE>
__device__ __forceinline__ void fwd2_roll(const PwArgs& a, f32x16 (&acc)[MT][1], float* Ws, const f32x4* Ps4,
                                          __amdgpu_buffer_rsrc_t r1, __amdgpu_buffer_rsrc_t r2, int voff, int coBase,
                                          int cstride4, int tid, int half, int l31) {
  const int Ci = a.Ci, Co = a.Co;
  const int nch = Ci / KW;
  float xr[32], yr[MODE == 2 ? 32 : 1];
  f32x4 wr[2 * MT];
  auto loadW = [&](int c0) {
#pragma unroll
    for (int q = 0; q < 2 * MT; ++q) {
      const int f = tid + PW_NT * q;
      const int rowi = f >> 4, kq = (f & 15) * 4;
      const int co = coBase + rowi;
      wr[q] = co < Co ? *reinterpret_cast<const f32x4*>(a.w + (size_t)co * Ci + c0 + kq) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
  };
#pragma unroll
  for (int u = 0; u < 32; ++u) {
    xr[u] = buf_load<1>(r1, voff, (2 * u) * cstride4);
    if (MODE == 2) yr[u] = buf_load<1>(r2, voff, (2 * u) * cstride4);
  }
  loadW(0);
  for (int c = 0; c < nch; ++c) {
    block_lds_sync();                 // the previous chunk's weight tile is consumed (first: Ps4 written)
#pragma unroll
    for (int q = 0; q < 2 * MT; ++q) {
      const int f = tid + PW_NT * q;
      const int rowi = f >> 4, kq = (f & 15) * 4;
#pragma unroll
      for (int e = 0; e < 4; ++e) Ws[rowi * KWS + kq + e] = wr[q][e];
    }
    block_lds_sync();
    const bool more = c + 1 < nch;
    const int cn = (c + 1) * KW;
    if (more) loadW(cn);
#pragma unroll
    for (int u = 0; u < 32; ++u) {
      const int kl = 2 * u + half;
      float av[MT];
#pragma unroll
      for (int m = 0; m < MT; ++m) av[m] = Ws[(32 * m + l31) * KWS + kl];
      float v = xr[u];
      if (MODE != 0) {
        const f32x4 p = Ps4[c * KW + kl];
        v = fmaf(v, p.x, p.y);
        if (MODE == 2) v += fmaf(yr[u], p.z, p.w);
        if (a.relu) v = fmaxf(v, 0.f);
      }
      if (more) {
        xr[u] = buf_load<1>(r1, voff, (cn + 2 * u) * cstride4);
        if (MODE == 2) yr[u] = buf_load<1>(r2, voff, (cn + 2 * u) * cstride4);
      }
#pragma unroll
      for (int m = 0; m < MT; ++m) acc[m][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[m], v, acc[m][0], 0, 0, 0);
    }
  }
}

template <int MT, int NW, bool ROLL>
__global__ __launch_bounds__(PW_NT) void k_pwconv_fwd2(PwArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* Ws = lds;                               // [32*MT][KWS]
  f32x4* Ps4 = reinterpret_cast<f32x4*>(lds + ((32 * MT * KWS + 3) & ~3));   // [Ci] : (s1,h1,s2,h2)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int half = lane >> 5, l31 = lane & 31;
  const PwBlk bk = pw_decode(a.nbx, a.nbx * a.n, a.cc);
  if (!bk.live) return;
  const int n = bk.n;
  const int coBase = bk.cz * 32 * MT;
  const int V = a.V, Ci = a.Ci, Co = a.Co;
  const int L = a.Tout * V;                      // output positions per (sample, channel)
  const int tile0 = (bk.bx * 4 + wave) * NW;
  const bool has2 = a.x2 != nullptr;
  const bool aff1 = a.s1 != nullptr, aff2 = a.s2 != nullptr;
  const bool wvec = (Ci & 3) == 0;
  const int cstride = a.T * V;

  // per-lane byte offsets of the NW position tiles inside channel (n, half); out-of-range lanes read as 0 (OOB)
  int voff[NW];
  bool pok[NW];
#pragma unroll
  for (int j = 0; j < NW; ++j) {
    const int pos = (tile0 + j) * 32 + l31;
    pok[j] = pos < L;
    const int pc = pok[j] ? pos : 0;
    const int row = pc / V;
    const int goff = (row * a.stride) * V + (pc - row * V);
    voff[j] = pok[j] ? (int)(((size_t)n * Ci + half) * cstride + goff) * 4 : BUF_OOB;
  }
  for (int i = tid; i < Ci; i += PW_NT) {
    f32x4 p;
    p.x = aff1 ? a.s1[i] : 1.f;
    p.y = aff1 ? a.h1[i] : 0.f;
    p.z = aff2 ? a.s2[i] : 1.f;
    p.w = aff2 ? a.h2[i] : 0.f;
    Ps4[i] = p;
  }
  const size_t xbytes = (size_t)a.n * Ci * cstride * 4;
  const __amdgpu_buffer_rsrc_t r1 = buf_rsrc(a.x1, xbytes);
  const __amdgpu_buffer_rsrc_t r2 = buf_rsrc(has2 ? a.x2 : a.x1, xbytes);

  f32x16 acc[MT][NW];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int j = 0; j < NW; ++j)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[m][j][i] = 0.f;

  const int mode = has2 ? 2 : ((aff1 || a.relu) ? 1 : 0);
  if (NW == 1 && ROLL) {
    if (mode == 0) fwd2_roll<MT, 0>(a, reinterpret_cast<f32x16 (&)[MT][1]>(acc), Ws, Ps4, r1, r2, voff[0], coBase, cstride * 4, tid, half, l31);
    else if (mode == 1) fwd2_roll<MT, 1>(a, reinterpret_cast<f32x16 (&)[MT][1]>(acc), Ws, Ps4, r1, r2, voff[0], coBase, cstride * 4, tid, half, l31);
    else fwd2_roll<MT, 2>(a, reinterpret_cast<f32x16 (&)[MT][1]>(acc), Ws, Ps4, r1, r2, voff[0], coBase, cstride * 4, tid, half, l31);
  } else
  for (int c0 = 0; c0 < Ci; c0 += KW) {
    const int kc = min(KW, Ci - c0);
    __syncthreads();                             // previous chunk's W fully consumed (and Ps written, first time)
    {
      // all 2*MT float4 loads of this thread are issued before the first LDS write (a plain load/store loop gets one
      // HBM round trip per iteration from hipcc: measured 16 us per chunk)
      f32x4 wr[2 * MT];
#pragma unroll
      for (int q = 0; q < 2 * MT; ++q) {
        const int f = tid + PW_NT * q;
        const int rowi = f >> 4, kq = (f & 15) * 4;
        const int co = coBase + rowi, ci = c0 + kq;
        if (wvec) {
          wr[q] = (co < Co && ci < Ci) ? *reinterpret_cast<const f32x4*>(a.w + (size_t)co * Ci + ci)
                                       : f32x4{0.f, 0.f, 0.f, 0.f};
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) wr[q][e] = (co < Co && ci + e < Ci) ? a.w[(size_t)co * Ci + ci + e] : 0.f;
        }
      }
#pragma unroll
      for (int q = 0; q < 2 * MT; ++q) {
        const int f = tid + PW_NT * q;
        const int rowi = f >> 4, kq = (f & 15) * 4;
#pragma unroll
        for (int e = 0; e < 4; ++e) Ws[rowi * KWS + kq + e] = wr[q][e];
      }
    }
    __syncthreads();
    if (Ci >= 48) {
      if (mode == 0) fwd2_chunk<MT, NW, 0, F2_UNRW>(a, acc, Ws, Ps4, r1, r2, voff, c0, kc, cstride * 4, half, l31);
      else if (mode == 1) fwd2_chunk<MT, NW, 1, F2_UNRW>(a, acc, Ws, Ps4, r1, r2, voff, c0, kc, cstride * 4, half, l31);
      else fwd2_chunk<MT, NW, 2, F2_UNRW>(a, acc, Ws, Ps4, r1, r2, voff, c0, kc, cstride * 4, half, l31);
    } else {
      if (mode == 0) fwd2_chunk<MT, NW, 0, F2_UNR>(a, acc, Ws, Ps4, r1, r2, voff, c0, kc, cstride * 4, half, l31);
      else if (mode == 1) fwd2_chunk<MT, NW, 1, F2_UNR>(a, acc, Ws, Ps4, r1, r2, voff, c0, kc, cstride * 4, half, l31);
      else fwd2_chunk<MT, NW, 2, F2_UNR>(a, acc, Ws, Ps4, r1, r2, voff, c0, kc, cstride * 4, half, l31);
    }
  }
  __syncthreads();
  // ---- epilogue: bias, coalesced stores; per-channel sum / sum of squares via an LDS transpose of each tile
  //      (a shuffle tree costs 160 ds_bpermute per tile and made the LDS pipe the bottleneck: measured) ----
  float* Tw = lds + wave * (32 * 36);            // per-wave 32x32 tile, row stride 36 (conflict-free b128 row reads)
  double* Ss = reinterpret_cast<double*>(lds + 4 * 32 * 36);   // [4 waves][32][2]; fp64: var = E[z^2]-mean^2 downstream
  const size_t blk = (size_t)bk.n * a.nbx + bk.bx;
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    double sv = 0.0, qv = 0.0;                   // fp64 (full rate on CDNA): the variance formula amplifies sum errors
#pragma unroll
    for (int j = 0; j < NW; ++j) {
      const int pos = (tile0 + j) * 32 + l31;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = mfma_row32(r, half);
        const int co = coBase + 32 * m + row;
        float val = 0.f;
        if (co < Co && pok[j]) {
          val = acc[m][j][r] + (a.bias ? a.bias[co] : 0.f);
          a.z[(size_t)(n * Co + co) * L + pos] = val;
        }
        if (a.stats) Tw[row * 36 + l31] = val;
      }
      if (a.stats) {
        wave_lds_sync();
        const f32x4* rowp = reinterpret_cast<const f32x4*>(Tw + l31 * 36 + half * 16);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const f32x4 v = rowp[q];
          sv += ((double)v.x + (double)v.y) + ((double)v.z + (double)v.w);
          qv = fma((double)v.x, (double)v.x, qv); qv = fma((double)v.y, (double)v.y, qv);
          qv = fma((double)v.z, (double)v.z, qv); qv = fma((double)v.w, (double)v.w, qv);
        }
        wave_lds_sync();
      }
    }
    if (a.stats) {
      sv += __shfl_xor(sv, 32, 64);
      qv += __shfl_xor(qv, 32, 64);              // (double overload: two dword shuffles)
      if (half == 0) {
        Ss[(wave * 32 + l31) * 2 + 0] = sv;
        Ss[(wave * 32 + l31) * 2 + 1] = qv;
      }
      __syncthreads();
      if (tid < 32) {
        const int co = coBase + 32 * m + tid;
        if (co < Co) {
          double s4 = 0.0, q4 = 0.0;
#pragma unroll
          for (int w = 0; w < 4; ++w) { s4 += Ss[(w * 32 + tid) * 2]; q4 += Ss[(w * 32 + tid) * 2 + 1]; }
          a.partial[(blk * Co + co) * 2 + 0] = (float)s4;
          a.partial[(blk * Co + co) * 2 + 1] = (float)q4;
        }
      }
      __syncthreads();
    }
  }
}

// zaug[n,c,t] = mean_v z[n,c,t,:] plus the global-joint column's share of the batch statistics.
// One wave per (n,c) plane: coalesced plane read into LDS, lanes = frames for the row means; partial row `n` of the
// extra block holds per-channel sum / sum of squares of zaug.
__global__ __launch_bounds__(64) void k_rowmean_stats(const float* __restrict__ z, float* __restrict__ zaug,
                                                      float* __restrict__ partial, int C, int T, int V) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int lane = threadIdx.x;
  const long plane = blockIdx.x;
  const int L = T * V;
  const float* __restrict__ pz = z + (size_t)plane * L;
  if ((L & 3) == 0) {
    plane_to_lds(pz, lds, L >> 2, lane);
  } else {
#pragma unroll 4
    for (int i = lane; i < L; i += 64) lds[i] = pz[i];
  }
  wave_lds_sync();
  const float invV = 1.f / (float)V;
  double sv = 0.0, qv = 0.0;
  for (int t = lane; t < T; t += 64) {
    float m = 0.f;
    for (int v = 0; v < V; ++v) m += lds[t * V + v];
    m *= invV;
    zaug[(size_t)plane * T + t] = m;
    sv += (double)m;
    qv = fma((double)m, (double)m, qv);
  }
  if (partial) {
    sv = wave_sum_d(sv);
    qv = wave_sum_d(qv);
    if (lane == 0) {
      partial[(size_t)plane * 2 + 0] = (float)sv;       // rows [n][C][2]
      partial[(size_t)plane * 2 + 1] = (float)qv;
    }
  }
}

// dz_eff (n,Co,T,V) materialised for convs with the global-joint column (the dgmstcn branch conv): folds the BN
// statistics terms and the zaug gradient once so that dgrad / wgrad run in their plain (single-stream) mode.
//   dz_eff = gz + A0 + B0*z + (gzaug + A0 + B0*zaug)/V
__global__ __launch_bounds__(64) void k_dz_eff_aug(const float* __restrict__ gz, const float* __restrict__ z,
                                                   const float* __restrict__ gzaug, const float* __restrict__ zaug,
                                                   const float* __restrict__ A0, const float* __restrict__ B0,
                                                   float* __restrict__ out, int C, int T, int V) {
  const int lane = threadIdx.x;
  const long plane = blockIdx.x;
  const int c = (int)(plane % C);
  const int L = T * V;
  const float a0 = A0 ? A0[c] : 0.f, b0 = A0 ? B0[c] : 0.f;
  const float invV = 1.f / (float)V;
  const float* __restrict__ pg = gz ? gz + (size_t)plane * L : nullptr;
  const float* __restrict__ pz = z + (size_t)plane * L;
  const float* __restrict__ pga = gzaug ? gzaug + (size_t)plane * T : nullptr;
  const float* __restrict__ pza = zaug + (size_t)plane * T;
  float* __restrict__ po = out + (size_t)plane * L;
#pragma unroll 4
  for (int i = lane; i < L; i += 64) {
    const int t = i / V;
    const float e = (pga ? pga[t] : 0.f) + fmaf(b0, pza[t], a0);
    po[i] = (pg ? pg[i] : 0.f) + fmaf(b0, pz[i], a0) + e * invV;
  }
}

// 16-byte form of k_dz_eff_aug (T*V % 4 == 0): per-frame term e[t] staged in LDS, planes streamed as float4 with
// all loads of a 256-float4 chunk issued before the arithmetic
__global__ __launch_bounds__(64) void k_dz_eff_aug4(const float* __restrict__ gz, const float* __restrict__ z,
                                                    const float* __restrict__ gzaug, const float* __restrict__ zaug,
                                                    const float* __restrict__ A0, const float* __restrict__ B0,
                                                    float* __restrict__ out, int C, int T, int V) {
  extern __shared__ __attribute__((aligned(16))) float lds[];       // [T] e
  const int lane = threadIdx.x;
  const long plane = blockIdx.x;
  const int c = (int)(plane % C);
  const int L = T * V, L4 = L >> 2;
  const float a0 = A0 ? A0[c] : 0.f, b0 = A0 ? B0[c] : 0.f;
  const float invV = 1.f / (float)V;
  for (int t = lane; t < T; t += 64)
    lds[t] = ((gzaug ? gzaug[(size_t)plane * T + t] : 0.f) + fmaf(b0, zaug[(size_t)plane * T + t], a0)) * invV;
  wave_lds_sync();
  const f32x4* __restrict__ pg = gz ? reinterpret_cast<const f32x4*>(gz + (size_t)plane * L) : nullptr;
  const f32x4* __restrict__ pz = reinterpret_cast<const f32x4*>(z + (size_t)plane * L);
  f32x4* __restrict__ po = reinterpret_cast<f32x4*>(out + (size_t)plane * L);
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  for (int base = 0; base < L4; base += 256) {
    f32x4 g4[4], z4[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = base + q * 64 + lane;
      const bool ok = i < L4;
      g4[q] = (ok && pg) ? pg[i] : zero4;
      z4[q] = ok ? pz[i] : zero4;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = base + q * 64 + lane;
      if (i >= L4) break;
      const float gg[4] = {g4[q].x, g4[q].y, g4[q].z, g4[q].w};
      const float zz[4] = {z4[q].x, z4[q].y, z4[q].z, z4[q].w};
      int t, v;
      divmod_small(4 * i, V, invV, t, v);
      float r[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        r[k] = gg[k] + fmaf(b0, zz[k], a0) + lds[t];
        if (++v == V) { v = 0; ++t; }
      }
      po[i] = f32x4{r[0], r[1], r[2], r[3]};
    }
  }
}

// ------------------------------------------------------------------------------------------------------------
// Backward.
//   dz_eff[co,pos] = g_z + A0[co] + B0[co]*z                     (the BN-statistics terms: d mean / d var of this conv's
//                    (+ (g_zaug[row] + A0 + B0*zaug[row]) / V     own output, folded into the load prologue)
//   dgrad:  dv[ci,pos] = sum_co W[co,ci] dz_eff[co,pos];  through the ReLU mask / affine of the virtual input:
//           d_x1 = dv*m*s1, d_x2 = dv*m*s2, partial sums of dv*m*x1, dv*m, dv*m*x2 (-> d s1, d h1=d h2, d s2)
//   wgrad:  dW[co,ci] = sum_pos dz_eff[co,pos] v[ci,pos];  db[co] = sum_pos dz_eff[co,pos]
// ------------------------------------------------------------------------------------------------------------

struct PwBwdArgs {
  // forward operands
  const float* x1; const float* s1; const float* h1;
  const float* x2; const float* s2; const float* h2;
  int relu;
  const float* w;
  // saved output + incoming gradients
  const float* z; const float* zaug;
  const float* gz; const float* gzaug;
  const float* A0; const float* B0;        // per Co, may be NULL (no batch-stat terms)
  // outputs
  float* dx1; float* dx2; float* ipart;    // ipart [nblk][Ci][3]
  float* dwp; float* dbp;                  // [ksplit][Co][Ci], [ksplit][Co]
  int n, Ci, Co, T, V, Tout, stride, aug, TR, NPpad, vec;
  int chunks_per_split, total_chunks, nb_per_sample, roll, nbx, cc;
  int pstride;                             // floats between consecutive k-splits in dwp / dbp
};

__device__ __forceinline__ float dz_eff_at(const PwBwdArgs& a, size_t gi, size_t gaug, int co, float invV) {
  float d = a.gz ? a.gz[gi] : 0.f;
  if (a.A0) d += fmaf(a.B0[co], a.z[gi], a.A0[co]);
  if (a.aug) {
    float e = a.gzaug ? a.gzaug[gaug] : 0.f;
    if (a.A0) e += fmaf(a.B0[co], a.zaug[gaug], a.A0[co]);
    d = fmaf(e, invV, d);
  }
  return d;
}

// Wave-independent dgrad (product path): same structure as k_pwconv_fwd2 with B = dz_eff straight from HBM
// (gz, z [, gzaug, zaug] via raw buffer loads, coefficients A0/B0 from LDS) and A = W^T from LDS.
template <int NW, bool AUG>
__device__ __forceinline__ void d2_load(float (&g)[F2_UNR][NW], float (&zz)[F2_UNR][NW], float (&ga)[F2_UNR][NW],
                                        float (&za)[F2_UNR][NW], __amdgpu_buffer_rsrc_t rg, __amdgpu_buffer_rsrc_t rz,
                                        __amdgpu_buffer_rsrc_t rga, __amdgpu_buffer_rsrc_t rza, const int (&voff)[NW],
                                        const int (&voffa)[NW], int cbase, int cstride4, int astride4, bool has_g,
                                        bool has_c) {
#pragma unroll
  for (int u = 0; u < F2_UNR; ++u) {
    const int soff = (cbase + 2 * u) * cstride4;
    const int soffa = (cbase + 2 * u) * astride4;
#pragma unroll
    for (int j = 0; j < NW; ++j) {
      g[u][j] = has_g ? buf_load<1>(rg, voff[j], soff) : 0.f;
      zz[u][j] = has_c ? buf_load<1>(rz, voff[j], soff) : 0.f;
      if (AUG) {
        ga[u][j] = buf_load<1>(rga, voffa[j], soffa);
        za[u][j] = has_c ? buf_load<1>(rza, voffa[j], soffa) : 0.f;
      }
    }
  }
}

template <int MT, int NW, bool AUG>
__device__ __forceinline__ void d2_compute(f32x16 (&acc)[MT][NW], const float* Ws, const float2* Cs,
                                           const float (&g)[F2_UNR][NW], const float (&zz)[F2_UNR][NW],
                                           const float (&ga)[F2_UNR][NW], const float (&za)[F2_UNR][NW], int kbase,
                                           int kc, int c0, float invV, int half, int l31) {
  constexpr int WS2 = 32 * MT + 1;
#pragma unroll
  for (int u = 0; u < F2_UNR; ++u) {
    const int kl = kbase + 2 * u + half;
    const bool cok = kl < kc;
    float av[MT], bv[NW];
#pragma unroll
    for (int m = 0; m < MT; ++m) av[m] = Ws[kl * WS2 + 32 * m + l31];
    const float2 cf = Cs[cok ? c0 + kl : 0];                  // (A0, B0)
#pragma unroll
    for (int j = 0; j < NW; ++j) {
      float d = g[u][j] + fmaf(cf.y, zz[u][j], cf.x);
      if (AUG) d = fmaf(ga[u][j] + fmaf(cf.y, za[u][j], cf.x), invV, d);
      bv[j] = cok ? d : 0.f;
    }
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int j = 0; j < NW; ++j)
        acc[m][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[m], bv[j], acc[m][j], 0, 0, 0);
  }
}

// Rolling whole-chunk prefetch for the data gradient (Co a multiple of 64, no global-joint column): see fwd2_roll.
template <int MT>
__device__ __forceinline__ void dgrad2_roll(const PwBwdArgs& a, f32x16 (&acc)[MT][1], float* Ws, const float2* Cs,
                                            __amdgpu_buffer_rsrc_t rg, __amdgpu_buffer_rsrc_t rz, int voff, int ciBase,
                                            int cstride4, bool has_g, bool has_c, int tid, int half, int l31) {
  constexpr int WS2 = 32 * MT + 1;
  const int Ci = a.Ci, Co = a.Co;
  const int nch = Co / KW;
  float gr[32], zr[32];
  f32x4 wr[2 * MT];
  auto loadW = [&](int c0) {
#pragma unroll
    for (int q = 0; q < 2 * MT; ++q) {
      const int f = tid + PW_NT * q;
      const int rowi = f / (8 * MT), cq = (f - rowi * (8 * MT)) * 4;
      const int ci = ciBase + cq;
      wr[q] = ci < Ci ? *reinterpret_cast<const f32x4*>(a.w + (size_t)(c0 + rowi) * Ci + ci) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
  };
#pragma unroll
  for (int u = 0; u < 32; ++u) {
    gr[u] = has_g ? buf_load<1>(rg, voff, (2 * u) * cstride4) : 0.f;
    zr[u] = has_c ? buf_load<1>(rz, voff, (2 * u) * cstride4) : 0.f;
  }
  loadW(0);
  for (int c = 0; c < nch; ++c) {
    block_lds_sync();
#pragma unroll
    for (int q = 0; q < 2 * MT; ++q) {
      const int f = tid + PW_NT * q;
      const int rowi = f / (8 * MT), cq = (f - rowi * (8 * MT)) * 4;
#pragma unroll
      for (int e = 0; e < 4; ++e) Ws[rowi * WS2 + cq + e] = wr[q][e];
    }
    block_lds_sync();
    const bool more = c + 1 < nch;
    const int cn = (c + 1) * KW;
    if (more) loadW(cn);
#pragma unroll
    for (int u = 0; u < 32; ++u) {
      const int kl = 2 * u + half;
      float av[MT];
#pragma unroll
      for (int m = 0; m < MT; ++m) av[m] = Ws[kl * WS2 + 32 * m + l31];
      const float2 cf = Cs[c * KW + kl];                      // (A0, B0)
      const float d = gr[u] + fmaf(cf.y, zr[u], cf.x);
      if (more) {
        gr[u] = has_g ? buf_load<1>(rg, voff, (cn + 2 * u) * cstride4) : 0.f;
        zr[u] = has_c ? buf_load<1>(rz, voff, (cn + 2 * u) * cstride4) : 0.f;
      }
#pragma unroll
      for (int m = 0; m < MT; ++m) acc[m][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[m], d, acc[m][0], 0, 0, 0);
    }
  }
}

template <int MT, int NW, bool AUG, bool ROLL, bool PREX>
__global__ __launch_bounds__(PW_NT) void k_pwconv_dgrad2(PwBwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int WS2 = 32 * MT + 1;
  float* Ws = lds;                               // [KW][WS2]  W[co chunk][ci tile]
  float2* Cs = reinterpret_cast<float2*>(lds + ((KW * WS2 + 3) & ~3));     // [Co] (A0, B0)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int half = lane >> 5, l31 = lane & 31;
  const PwBlk bk = pw_decode(a.nbx, a.nbx * a.n, a.cc);
  if (!bk.live) return;
  const int n = bk.n;
  const int ciBase = bk.cz * 32 * MT;
  const int V = a.V, Ci = a.Ci, Co = a.Co;
  const int L = a.Tout * V;
  const int tile0 = (bk.bx * 4 + wave) * NW;
  const bool has_g = a.gz != nullptr, has_c = a.A0 != nullptr;
  const bool wvec = (Ci & 3) == 0;
  const float invV = 1.f / (float)V;

  int voff[NW], voffa[NW], goff[NW];
  bool pok[NW];
#pragma unroll
  for (int j = 0; j < NW; ++j) {
    const int pos = (tile0 + j) * 32 + l31;
    pok[j] = pos < L;
    const int pc = pok[j] ? pos : 0;
    const int row = pc / V;
    goff[j] = (row * a.stride) * V + (pc - row * V);
    voff[j] = pok[j] ? (int)(((size_t)n * Co + half) * L + pc) * 4 : BUF_OOB;
    voffa[j] = pok[j] ? (int)(((size_t)n * Co + half) * a.Tout + row) * 4 : BUF_OOB;
  }
  for (int i = tid; i < Co; i += PW_NT) Cs[i] = has_c ? float2{a.A0[i], a.B0[i]} : float2{0.f, 0.f};
  const size_t zbytes = (size_t)a.n * Co * L * 4, abytes = (size_t)a.n * Co * a.Tout * 4;
  const __amdgpu_buffer_rsrc_t rg = buf_rsrc(has_g ? a.gz : a.x1, has_g ? zbytes : 0);
  const __amdgpu_buffer_rsrc_t rz = buf_rsrc(has_c ? a.z : a.x1, has_c ? zbytes : 0);
  const __amdgpu_buffer_rsrc_t rga = buf_rsrc((AUG && a.gzaug) ? a.gzaug : a.x1, (AUG && a.gzaug) ? abytes : 0);
  const __amdgpu_buffer_rsrc_t rza = buf_rsrc((AUG && has_c) ? a.zaug : a.x1, (AUG && has_c) ? abytes : 0);

  f32x16 acc[MT][NW];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int j = 0; j < NW; ++j)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[m][j][i] = 0.f;

  // PREX: the epilogue's operands (the forward input at this tile, for the ReLU mask / affine / partial sums) are
  // fetched before the K loop instead of after it, where their latency is fully exposed
  // a plain input (no affine, no ReLU, no second operand — `pre`, `down`, the projections) is not needed at all here
  const bool need_x = a.relu || a.s1 != nullptr || a.x2 != nullptr;
  float xpre[PREX ? MT : 1][PREX ? 16 : 1], ypre[PREX ? MT : 1][PREX ? 16 : 1];
  if (PREX && need_x) {
    const size_t cst = (size_t)a.T * V;
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int ci = ciBase + 32 * m + mfma_row32(r, half);
        const bool ok = ci < Ci && pok[0];
        const size_t g = ((size_t)n * Ci + (ok ? ci : 0)) * cst + (ok ? goff[0] : 0);
        xpre[m][r] = ok ? a.x1[g] : 0.f;
        ypre[m][r] = (ok && a.x2) ? a.x2[g] : 0.f;
      }
  }
  constexpr int G = 2 * F2_UNR;
  if (NW == 1 && !AUG && ROLL) {
    dgrad2_roll<MT>(a, reinterpret_cast<f32x16 (&)[MT][1]>(acc), Ws, Cs, rg, rz, voff[0], ciBase, L * 4, has_g, has_c, tid,
                    half, l31);
  } else
  for (int c0 = 0; c0 < Co; c0 += KW) {
    const int kc = min(KW, Co - c0);
    __syncthreads();
    {
      f32x4 wr[2 * MT];
#pragma unroll
      for (int q = 0; q < 2 * MT; ++q) {
        const int f = tid + PW_NT * q;
        const int rowi = f / (8 * MT), cq = (f - rowi * (8 * MT)) * 4;
        const int co = c0 + rowi, ci = ciBase + cq;
        if (wvec) {
          wr[q] = (co < Co && ci < Ci) ? *reinterpret_cast<const f32x4*>(a.w + (size_t)co * Ci + ci)
                                       : f32x4{0.f, 0.f, 0.f, 0.f};
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) wr[q][e] = (co < Co && ci + e < Ci) ? a.w[(size_t)co * Ci + ci + e] : 0.f;
        }
      }
#pragma unroll
      for (int q = 0; q < 2 * MT; ++q) {
        const int f = tid + PW_NT * q;
        const int rowi = f / (8 * MT), cq = (f - rowi * (8 * MT)) * 4;
#pragma unroll
        for (int e = 0; e < 4; ++e) Ws[rowi * WS2 + cq + e] = wr[q][e];
      }
    }
    __syncthreads();
    const int kpad = (kc + 2 * G - 1) / (2 * G) * (2 * G);
    float ga_[F2_UNR][NW], za_[F2_UNR][NW], gaa[F2_UNR][NW], zaa[F2_UNR][NW];
    float gb_[F2_UNR][NW], zb_[F2_UNR][NW], gab[F2_UNR][NW], zab[F2_UNR][NW];
    d2_load<NW, AUG>(ga_, za_, gaa, zaa, rg, rz, rga, rza, voff, voffa, c0, L * 4, a.Tout * 4, has_g, has_c);
    for (int k0 = 0; k0 < kpad; k0 += 2 * G) {
      d2_load<NW, AUG>(gb_, zb_, gab, zab, rg, rz, rga, rza, voff, voffa, c0 + k0 + G, L * 4, a.Tout * 4, has_g, has_c);
      d2_compute<MT, NW, AUG>(acc, Ws, Cs, ga_, za_, gaa, zaa, k0, kc, c0, invV, half, l31);
      d2_load<NW, AUG>(ga_, za_, gaa, zaa, rg, rz, rga, rza, voff, voffa, c0 + k0 + 2 * G, L * 4, a.Tout * 4, has_g,
                       has_c);
      d2_compute<MT, NW, AUG>(acc, Ws, Cs, gb_, zb_, gab, zab, k0 + G, kc, c0, invV, half, l31);
    }
  }
  __syncthreads();
  // ---- epilogue: ReLU mask / affine of the virtual input, coalesced stores, 3 per-channel partial sums ----
  float* Tw = lds + wave * (32 * 36);
  float* Ss = lds + 4 * 32 * 36;                 // [4 waves][32][3]
  const size_t blk = (size_t)bk.n * a.nbx + bk.bx;
  const size_t cstride = (size_t)a.T * V;
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    float u0 = 0.f, u1 = 0.f, u2 = 0.f;
#pragma unroll
    for (int j = 0; j < NW; ++j) {
      float dvv[16], xav[16], xbv[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int ci = ciBase + 32 * m + mfma_row32(r, half);
        float dv = 0.f, xa = 0.f, xb = 0.f;
        if (ci < Ci && pok[j]) {
          const size_t g = ((size_t)n * Ci + ci) * cstride + goff[j];
          xa = !need_x ? 0.f : (PREX ? xpre[m][r] : a.x1[g]);
          const float sa = a.s1 ? a.s1[ci] : 1.f;
          float pre = a.s1 ? fmaf(xa, sa, a.h1[ci]) : xa;
          float sb = 1.f;
          if (a.x2) {
            xb = PREX ? ypre[m][r] : a.x2[g];
            if (a.s2) { sb = a.s2[ci]; pre += fmaf(xb, sb, a.h2[ci]); } else pre += xb;
          }
          dv = (!a.relu || pre > 0.f) ? acc[m][j][r] : 0.f;
          a.dx1[g] = dv * sa;
          if (a.dx2) a.dx2[g] = dv * sb;
        }
        dvv[r] = dv; xav[r] = xa; xbv[r] = xb;
      }
      if (a.ipart) {
        // three LDS-transposed row sums: dv*x1, dv, dv*x2
#pragma unroll
        for (int which = 0; which < 3; ++which) {
          if (which == 2 && !a.x2) continue;
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const float val = which == 0 ? dvv[r] * xav[r] : (which == 1 ? dvv[r] : dvv[r] * xbv[r]);
            Tw[mfma_row32(r, half) * 36 + l31] = val;
          }
          wave_lds_sync();
          const f32x4* rowp = reinterpret_cast<const f32x4*>(Tw + l31 * 36 + half * 16);
          float sacc = 0.f;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const f32x4 v = rowp[q];
            sacc += (v.x + v.y) + (v.z + v.w);
          }
          if (which == 0) u0 += sacc; else if (which == 1) u1 += sacc; else u2 += sacc;
          wave_lds_sync();
        }
      }
    }
    if (a.ipart) {
      u0 += __shfl_xor(u0, 32, 64);
      u1 += __shfl_xor(u1, 32, 64);
      u2 += __shfl_xor(u2, 32, 64);
      if (half == 0) {
        float* q = Ss + (wave * 32 + l31) * 3;
        q[0] = u0; q[1] = u1; q[2] = u2;
      }
      __syncthreads();
      if (tid < 32) {
        const int ci = ciBase + 32 * m + tid;
        if (ci < Ci) {
          float v0 = 0.f, v1 = 0.f, v2 = 0.f;
#pragma unroll
          for (int w = 0; w < 4; ++w) {
            const float* q = Ss + (w * 32 + tid) * 3;
            v0 += q[0]; v1 += q[1]; v2 += q[2];
          }
          float* o = a.ipart + (blk * Ci + ci) * 3;
          o[0] = v0; o[1] = v1; o[2] = v2;
        }
      }
      __syncthreads();
    }
  }
}

// wgrad: block = (64 co x 64 ci output tile, k-split); K = positions of `chunks_per_split` (sample, TR-row) chunks.
// Thread (row = tid/4, quarter = tid%4) stages positions 16*j + 4*quarter + {0..3}, j < 7, of tile row `row` for both
// operands (dz_eff of channel coBase+row and the virtual input of channel ciBase+row): all loads of a chunk are issued
// before the MFMAs of the previous chunk.  LDS rows have an odd stride so the per-lane column reads
// (A[i=co][k=pos], B[k=pos][j=ci]) are conflict-free.
constexpr int WG_J = 7;            // float4 slots per thread per operand: covers 4*4*7 = 112 >= TR*V positions
constexpr int WG_TR = 4;           // frames per wgrad chunk (multiple of 4 keeps every chunk 16-B aligned)
template <bool VEC, bool HAS2>
__global__ __launch_bounds__(PW_NT) void k_pwconv_wgrad(PwBwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int V = a.V, TR = a.TR, Co = a.Co, Ci = a.Ci;
  const int TRV = TR * V;
  const int KP = (TRV + 1) & ~1;                 // positions per chunk, even
  const int LS = KP | 1;                         // odd row stride
  float* Ds = lds;                               // [64][LS] dz_eff
  float* Xs = lds + 64 * LS;                     // [64][LS] virtual input
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int half = lane >> 5, l31 = lane & 31;
  // XCD-aware decode of a 1-D grid when a layer has several (co, ci) tiles: the tiles of one K-split read the same dz /
  // input chunks, so they get consecutive slots on one XCD (blockIdx % 8 labels the XCD group) and share its L2.
  int bxx = blockIdx.x, byy = blockIdx.y, bzz = blockIdx.z;
  if (a.cc > 0) {
    const int id = blockIdx.x, xcd = id & 7, slot = id >> 3;
    const int tiles = a.cc * a.nbx;                    // nbx = co tiles, cc = ci tiles
    const int tile = slot % tiles;
    bzz = (slot / tiles) * 8 + xcd;
    bxx = tile % a.nbx;
    byy = tile / a.nbx;
  }
  const int coBase = bxx * 64, ciBase = byy * 64;
  const int split = bzz;
  const int mt = wave >> 1, ntile = wave & 1;
  const float invV = 1.f / (float)V;
  const int row = tid >> 2, quarter = tid & 3;
  const int co = coBase + row, ci = ciBase + row;
  const bool has_g = a.gz != nullptr, has_c = a.A0 != nullptr;
  constexpr bool has2 = HAS2;
  const float A0c = (has_c && co < Co) ? a.A0[co] : 0.f, B0c = (has_c && co < Co) ? a.B0[co] : 0.f;
  const float s1 = (a.s1 && ci < Ci) ? a.s1[ci] : 1.f, h1 = (a.s1 && ci < Ci) ? a.h1[ci] : 0.f;
  const float s2 = (a.s2 && ci < Ci) ? a.s2[ci] : 1.f, h2 = (a.s2 && ci < Ci) ? a.h2[ci] : 0.f;
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  float dbacc = 0.f;
  f32x4 gr[WG_J], zr[WG_J], xr[WG_J], yr[HAS2 ? WG_J : 1];
  const int ch0 = split * a.chunks_per_split;
  const int ch1 = min(a.total_chunks, ch0 + a.chunks_per_split);

  auto issue = [&](int ch) {
    const int n = ch / a.nb_per_sample;
    const int r0 = (ch - n * a.nb_per_sample) * TR;
    const int nvalid = min(TR, a.Tout - r0) * V;
    const size_t gzb = ((size_t)(n * Co + co) * a.Tout + r0) * V;
    const size_t gxb = ((size_t)(n * Ci + ci) * a.T + (size_t)r0 * a.stride) * V;
#pragma unroll
    for (int j = 0; j < WG_J; ++j) {
      const int p = 16 * j + 4 * quarter;
      if (VEC) {
        if (p < nvalid) {
          if (co < Co) {
            if (has_g) gr[j] = *reinterpret_cast<const f32x4*>(a.gz + gzb + p);
            if (has_c) zr[j] = *reinterpret_cast<const f32x4*>(a.z + gzb + p);
          }
          if (ci < Ci) {
            xr[j] = *reinterpret_cast<const f32x4*>(a.x1 + gxb + p);
            if (HAS2) yr[HAS2 ? j : 0] = *reinterpret_cast<const f32x4*>(a.x2 + gxb + p);
          }
        }
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int pe = p + e;
          if (pe < nvalid) {
            if (co < Co) {
              if (has_g) gr[j][e] = a.gz[gzb + pe];
              if (has_c) zr[j][e] = a.z[gzb + pe];
            }
            if (ci < Ci) {
              const int rl = (int)(((float)pe + 0.5f) * invV);
              const size_t g = gxb + (size_t)rl * a.stride * V + (pe - rl * V);
              xr[j][e] = a.x1[g];
              if (HAS2) yr[HAS2 ? j : 0][e] = a.x2[g];
            }
          }
        }
      }
    }
  };

  auto commit = [&](int ch) {
    const int n = ch / a.nb_per_sample;
    const int r0 = (ch - n * a.nb_per_sample) * TR;
    const int nvalid = min(TR, a.Tout - r0) * V;
    float dsum = 0.f;
#pragma unroll
    for (int j = 0; j < WG_J; ++j) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int pe = 16 * j + 4 * quarter + e;
        if (pe < KP) {
          float d = 0.f, x = 0.f;
          if (pe < nvalid) {
            if (co < Co) {
              d = has_g ? gr[j][e] : 0.f;
              if (has_c) d += fmaf(B0c, zr[j][e], A0c);
              if (a.aug) {
                const int rl = (int)(((float)pe + 0.5f) * invV);
                const size_t ga = (size_t)(n * Co + co) * a.Tout + r0 + rl;
                float ea = a.gzaug ? a.gzaug[ga] : 0.f;
                if (has_c) ea += fmaf(B0c, a.zaug[ga], A0c);
                d = fmaf(ea, invV, d);
              }
            }
            if (ci < Ci) x = virt1(xr[j][e], HAS2 ? yr[HAS2 ? j : 0][e] : 0.f, has2, s1, h1, s2, h2, a.relu);
          }
          Ds[row * LS + pe] = d;
          Xs[row * LS + pe] = x;
          dsum += d;
        }
      }
    }
    dsum += __shfl_xor(dsum, 1, 64);
    dsum += __shfl_xor(dsum, 2, 64);
    dbacc += dsum;
  };

  if (ch0 < ch1) issue(ch0);
  for (int ch = ch0; ch < ch1; ++ch) {
    commit(ch);
    __syncthreads();
    if (ch + 1 < ch1) issue(ch + 1);
    for (int kk = 0; kk < KP; kk += 2) {
      const float av = Ds[(32 * mt + l31) * LS + kk + half];
      const float bv = Xs[(32 * ntile + l31) * LS + kk + half];
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
    }
    __syncthreads();
  }
  // D[i=co][j=ci]
  const int cio = ciBase + 32 * ntile + l31;
  if (cio < Ci) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int coo = coBase + 32 * mt + mfma_row32(r, half);
      if (coo < Co) a.dwp[(size_t)split * a.pstride + (size_t)coo * Ci + cio] = acc[r];
    }
  }
  if (byy == 0 && quarter == 0 && co < Co) a.dbp[(size_t)split * a.pstride + co] = dbacc;
}

// ------------------------------------------------------------------------------------------------------------
// Dispatch.  Knobs first (lab: dsgcn_pwconv_tuning keys 1-3; the values are the product's).
// ------------------------------------------------------------------------------------------------------------
int g_pw_maxmt = 2;        // measured (round-1 ablation): small per-wave tiles + more resident waves win
int g_pw_roll = 13;        // bit 0: rolling prefetch in the forward (on), bit 1: in the data gradient (off: 64 more VGPRs halve
                           // the occupancy, measured -4 % on the step: round-1 A/B), bit 2: dgrad epilogue operands
                           // fetched before the K loop (on: +0.5 %), bit 3: XCD-aware block order in wgrad (on: +0.5 %)
int g_pw4 = 15;            // bit 0: wide-load forward (pw4.hip), bit 1: wide-load data gradient, bit 2: blocked wgrad (wgrad.hip),
                           // bit 3: one-pass narrow backward (bwd64.hip)

// workgroup rows of the statistics / input-affine partial buffers for a (K -> M) mix over n planes of L positions
int pw_conv_rows(int n, int K, int M, int T, int V, int stride, int which) {
  const int Tout = (T + stride - 1) / stride;
  const int L = Tout * V;
  if (stride == 1 && (g_pw4 & which)) {
    const int g = dsgcn_p4_groups(n, K, M, L, which == 2 ? 1 : 0);
    if (g > 0) return g;
  }
  return n * ((L + 4 * 32 - 1) / (4 * 32));
}

// the first-generation kernels address the whole tensor with 32-bit byte offsets (the wide-load kernels carry the sample
// base in the buffer resource): what they cannot address is refused instead of wrapping silently
bool pw_gen1_addressable(int n, int Ci, int Co, int T, int V) {
  return (long)n * Ci * T * V * 4 < (1L << 31) - 64 && (long)n * Co * T * V * 4 < (1L << 31) - 64;
}

bool pw_guest_ok(const dsgcn_guest_conv* g) {
  return !g || (g->in && g->w && g->out && g->n > 0 && g->Ci > 0 && g->Co > 0 && g->L > 0);
}

// The forward.  guest: a conv for the launch to carry (*hosted: set to 1 when it did).
int pw_fwd(const KcIn& in, const float* w, const float* bias, float* z, float* zaug, float* partial, int n, int Ci, int Co,
           int T, int V, int stride, int aug, int stats, const void* ws, const dsgcn_guest_conv* guest, int* hosted,
           void* stream) {
  if (!in.x1 || !w || !z || n <= 0 || Ci <= 0 || Co <= 0 || T <= 0 || V <= 0 || stride <= 0) return DSGCN_EINVAL;
  if ((aug && !zaug) || (stats && !partial) || (in.s1 && !in.h1) || (in.s2 && !in.h2)) return DSGCN_EINVAL;
  const int Tout = (T + stride - 1) / stride;
  hipStream_t st = (hipStream_t)stream;
  const int L = Tout * V;
  const int conv_rows = pw_conv_rows(n, Ci, Co, T, V, stride, 1);
  int fast = 0;
  if (stride == 1 && (g_pw4 & 1)) {
    fast = dsgcn_p4_fwd(in, w, bias, z, stats ? partial : nullptr, n, Ci, Co, L, st, ws, guest, hosted);
    if (fast != 0 && fast != 1) return fast;
  }
  if (!fast) {
    if (!pw_gen1_addressable(n, Ci, Co, T, V)) return DSGCN_EUNSUPPORTED;
    PwArgs a = {};
    a.x1 = in.x1; a.s1 = in.s1; a.h1 = in.h1; a.x2 = in.x2; a.s2 = in.s2; a.h2 = in.h2; a.relu = in.relu;
    a.w = w; a.bias = bias; a.z = z; a.zaug = zaug; a.partial = partial;
    a.n = n; a.Ci = Ci; a.Co = Co; a.T = T; a.V = V; a.Tout = Tout; a.stride = stride; a.aug = aug;
    a.stats = stats;
    a.roll = ((g_pw_roll & 1) && Ci % KW == 0) ? 1 : 0;
    const int mtiles = (Co + 31) / 32;
    const int MT = mtiles >= g_pw_maxmt ? g_pw_maxmt : mtiles;
    const int NW = 1;
    const int nbx = (L + 4 * NW * 32 - 1) / (4 * NW * 32);
    a.nbx = nbx;
    a.cc = (mtiles + MT - 1) / MT;
    dim3 grid((unsigned)(((long)nbx * n + 7) / 8 * 8 * a.cc));
    size_t ldsf = (size_t)32 * MT * KWS + 4 + (size_t)4 * Ci;
    if (ldsf < (size_t)4 * 32 * 36 + 512) ldsf = (size_t)4 * 32 * 36 + 512;
    const size_t lds = ldsf * sizeof(float);
#define PW_FWD2(MTV)                                                                                  \
  if (a.roll) hipLaunchKernelGGL((k_pwconv_fwd2<MTV, 1, true>), grid, dim3(PW_NT), lds, st, a);       \
  else hipLaunchKernelGGL((k_pwconv_fwd2<MTV, 1, false>), grid, dim3(PW_NT), lds, st, a)
    switch (MT) {
      case 1: PW_FWD2(1); break;
      case 2: PW_FWD2(2); break;
      case 3: PW_FWD2(3); break;
      default: PW_FWD2(4); break;
    }
#undef PW_FWD2
    DSGCN_LAUNCH_CHECK();
  }
  if (aug) {
    const size_t l2 = (size_t)Tout * V * sizeof(float);
    if (l2 > 64 * 1024) return DSGCN_EUNSUPPORTED;
    hipLaunchKernelGGL(k_rowmean_stats, dim3((unsigned)((long)n * Co)), dim3(64), l2, st, z, zaug,
                       stats ? partial + (size_t)conv_rows * Co * 2 : (float*)nullptr, Co, Tout, V);
    DSGCN_LAUNCH_CHECK();
  }
  return 0;
}

// The data gradient (guest, hosted: as pw_fwd).  zaug / gzaug: the global-joint column's share of d (aug).
int pw_dgrad(const KcIn& in, const float* w, const KcDz& d, const float* zaug, const float* gzaug, float* dx1, float* dx2,
             float* ipart, int n, int Ci, int Co, int T, int V, int stride, int aug, const void* ws,
             const dsgcn_guest_conv* guest, int* hosted, void* stream) {
  if (!in.x1 || !w || !dx1 || n <= 0 || Ci <= 0 || Co <= 0 || T <= 0 || V <= 0 || stride <= 0) return DSGCN_EINVAL;
  if ((d.A0 && (!d.B0 || !d.z)) || (aug && d.A0 && !zaug) || (in.x2 && !dx2)) return DSGCN_EINVAL;
  // dsgcn_pwconv_ipart_rows sizes `ipart` for the wide-load plan, which needs gz: a NULL gz would drop to the scalar
  // kernels and their (larger) row count — refuse instead of writing past the caller's buffer
  if (!d.gz && ipart) return DSGCN_EINVAL;
  const int Tout = (T + stride - 1) / stride;
  hipStream_t st = (hipStream_t)stream;
  if (stride > 1) {
    hipError_t e = hipMemsetAsync(dx1, 0, (size_t)n * Ci * T * V * sizeof(float), st);
    if (e != hipSuccess) return (int)e;
    if (dx2) {
      e = hipMemsetAsync(dx2, 0, (size_t)n * Ci * T * V * sizeof(float), st);
      if (e != hipSuccess) return (int)e;
    }
  }
  const int L = Tout * V;
  if (stride == 1 && !aug && (g_pw4 & 2)) {
    const int fast = dsgcn_p4_dgrad(in, w, d, dx1, dx2, ipart, n, Ci, Co, L, st, ws, guest, hosted);
    if (fast == 1) return 0;
    if (fast != 0) return fast;
  }
  if (!pw_gen1_addressable(n, Ci, Co, T, V)) return DSGCN_EUNSUPPORTED;
  PwBwdArgs a = {};
  a.x1 = in.x1; a.s1 = in.s1; a.h1 = in.h1; a.x2 = in.x2; a.s2 = in.s2; a.h2 = in.h2; a.relu = in.relu; a.w = w;
  a.z = d.z; a.zaug = zaug; a.gz = d.gz; a.gzaug = gzaug; a.A0 = d.A0; a.B0 = d.B0;
  a.dx1 = dx1; a.dx2 = dx2; a.ipart = ipart;
  a.n = n; a.Ci = Ci; a.Co = Co; a.T = T; a.V = V; a.Tout = Tout; a.stride = stride; a.aug = aug;
  a.roll = ((g_pw_roll & 2) && Co % KW == 0 && (Ci & 3) == 0) ? 1 : 0;
  const int mtiles = (Ci + 31) / 32;
  const int MT = mtiles >= g_pw_maxmt ? g_pw_maxmt : mtiles;
  const int NW = 1;
  const int nbx = (L + 4 * NW * 32 - 1) / (4 * NW * 32);
  a.nbx = nbx;
  a.cc = (mtiles + MT - 1) / MT;
  dim3 grid((unsigned)(((long)nbx * n + 7) / 8 * 8 * a.cc));
  size_t ldsf = (size_t)KW * (32 * MT + 1) + 4 + (size_t)2 * Co;
  if (ldsf < (size_t)4 * 32 * 36 + 4 * 32 * 3) ldsf = (size_t)4 * 32 * 36 + 4 * 32 * 3;
  const size_t lds = ldsf * sizeof(float);
#define DSGCN_DGRAD(MTv, NWv)                                                                        \
  do {                                                                                               \
    if (aug) hipLaunchKernelGGL((k_pwconv_dgrad2<MTv, NWv, true, false, false>), grid, dim3(PW_NT), lds, st, a);   \
    else if (a.roll) hipLaunchKernelGGL((k_pwconv_dgrad2<MTv, NWv, false, true, false>), grid, dim3(PW_NT), lds, st, a);   \
    else if (g_pw_roll & 4) hipLaunchKernelGGL((k_pwconv_dgrad2<MTv, NWv, false, false, (NWv == 1)>), grid, dim3(PW_NT), lds, st, a);      \
    else hipLaunchKernelGGL((k_pwconv_dgrad2<MTv, NWv, false, false, false>), grid, dim3(PW_NT), lds, st, a);      \
  } while (0)
  switch (MT) {
    case 1: DSGCN_DGRAD(1, 1); break;
    case 2: DSGCN_DGRAD(2, 1); break;
    case 3: DSGCN_DGRAD(3, 1); break;
    default: DSGCN_DGRAD(4, 1); break;
  }
#undef DSGCN_DGRAD
  DSGCN_LAUNCH_CHECK();
  return 0;
}

// A guest record (dsgcn_jobs.h) launched on its own, when the host's launch did not carry it.  Forward: in = x, out = z.
int pw_guest_fwd(const dsgcn_guest_conv* g, void* stream) {
  return pw_fwd(KcIn{g->in}, g->w, g->bias, g->out, nullptr, nullptr, g->n, g->Ci, g->Co, 1, g->L, 1, 0, 0, nullptr, nullptr,
                nullptr, stream);
}
// Backward: the data gradient of a small plain conv — in = gz (n, Co, L), out = dx (n, Ci, L), bias unused.
// (x1 only has to be non-NULL: a plain conv — no ReLU, no input affine, no second stream — never reads its forward input
// in the data gradient, so the record carries none and dx stands in for it)
int pw_guest_dgrad(const dsgcn_guest_conv* g, void* stream) {
  return pw_dgrad(KcIn{g->out}, g->w, KcDz{nullptr, g->in}, nullptr, nullptr, g->out, nullptr, nullptr, g->n, g->Ci, g->Co, 1,
                  g->L, 1, 0, nullptr, nullptr, nullptr, stream);
}

// k-split plan of the weight gradient: the number of splits (size of dim 0 of dwp / dbp)
int pw_wgrad_splits(int n, int Ci, int Co, int T, int V, int stride) {
  const int Tout = (T + stride - 1) / stride;
  if (stride == 1 && (g_pw4 & 4)) {
    const int s = dsgcn_wg2_splits(n, Ci, Co, T * V);
    if (s > 0) return s;
  }
  const int TR = Tout >= WG_TR ? WG_TR : Tout;
  const int chunks = n * ((Tout + TR - 1) / TR);
  const int tiles = ((Co + 63) / 64) * ((Ci + 63) / 64);
  int splits = 512 / tiles;
  if (splits < 1) splits = 1;
  if (splits > chunks) splits = chunks;
  const int per = (chunks + splits - 1) / splits;
  return (chunks + per - 1) / per;
}

// The weight gradient with the BatchNorm coefficient jobs `jt` (checked by the caller; jt.n may be 0): the jobs ride in
// the blocked kernel's launch as extra workgroups, or go out as one launch ahead of the first-generation kernel.
int pw_wgrad(const KcIn& in, const KcDz& d, const float* zaug, const float* gzaug, float* dwp, float* dbp, int pstride, int n,
             int Ci, int Co, int T, int V, int stride, int aug, const BnCoefTable& jt, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (stride == 1 && !aug && (g_pw4 & 4)) {
    if (pstride < Co * Ci) return DSGCN_EINVAL;
    const int fast = dsgcn_wg2(in, d, dwp, dbp, pstride, n, Ci, Co, T * V, st, &jt);
    if (fast == 1) return 0;
    if (fast != 0) return fast;
  }
  if (jt.n) {                                      // not hosted: one launch for the jobs, then the weight gradient
    const int rc = bnj_coef_launch(jt, st);
    if (rc != 0) return rc;
  }
  if (!pw_gen1_addressable(n, Ci, Co, T, V)) return DSGCN_EUNSUPPORTED;
  const int Tout = (T + stride - 1) / stride;
  const int TR = Tout >= WG_TR ? WG_TR : Tout;
  if (TR * V > 16 * WG_J) return DSGCN_EUNSUPPORTED;
  if (pstride < Co * Ci) return DSGCN_EINVAL;
  PwBwdArgs a = {};
  a.x1 = in.x1; a.s1 = in.s1; a.h1 = in.h1; a.x2 = in.x2; a.s2 = in.s2; a.h2 = in.h2; a.relu = in.relu;
  a.z = d.z; a.zaug = zaug; a.gz = d.gz; a.gzaug = gzaug; a.A0 = d.A0; a.B0 = d.B0; a.dwp = dwp; a.dbp = dbp;
  a.pstride = pstride;
  a.n = n; a.Ci = Ci; a.Co = Co; a.T = T; a.V = V; a.Tout = Tout; a.stride = stride; a.aug = aug; a.TR = TR;
  a.nb_per_sample = (Tout + TR - 1) / TR;
  a.total_chunks = n * a.nb_per_sample;
  a.vec = (stride == 1 && (T * V) % 4 == 0 && (Tout * V) % 4 == 0 && (TR * V) % 4 == 0 &&
           ((Tout % TR) * V) % 4 == 0) ? 1 : 0;
  const int splits = pw_wgrad_splits(n, Ci, Co, T, V, stride);
  a.chunks_per_split = (a.total_chunks + splits - 1) / splits;
  const int KP = (TR * V + 1) & ~1;
  const int LS = KP | 1;
  const size_t lds = (size_t)2 * 64 * LS * sizeof(float);
  dim3 grid((unsigned)((Co + 63) / 64), (unsigned)((Ci + 63) / 64), (unsigned)splits);
  a.nbx = a.cc = 0;
  if (grid.x * grid.y > 1 && splits % 8 == 0 && (g_pw_roll & 8)) {
    a.nbx = (int)grid.x; a.cc = (int)grid.y;
    grid = dim3(grid.x * grid.y * (unsigned)splits);
  }
  if (a.vec && in.x2) hipLaunchKernelGGL((k_pwconv_wgrad<true, true>), grid, dim3(PW_NT), lds, st, a);
  else if (a.vec) hipLaunchKernelGGL((k_pwconv_wgrad<true, false>), grid, dim3(PW_NT), lds, st, a);
  else if (in.x2) hipLaunchKernelGGL((k_pwconv_wgrad<false, true>), grid, dim3(PW_NT), lds, st, a);
  else hipLaunchKernelGGL((k_pwconv_wgrad<false, false>), grid, dim3(PW_NT), lds, st, a);
  DSGCN_LAUNCH_CHECK();
  return 0;
}

// the sizes the three grouped entry points accept
bool pw_group_dims_ok(int ngroup, int n, int Ci, int Co, int T, int V) {
  return ngroup >= 1 && ngroup <= 3 && n > 0 && Ci > 0 && Co > 0 && T > 0 && V > 0;
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------
// The C ABI (include/dsgcn.h).  An entry point that is another one with a NULL stands right under it.
// ------------------------------------------------------------------------------------------------------------
extern "C" {

#ifdef DSGCN_LAB
int dsgcn_pwconv_tuning(int key, int value) {
  if (key == 1) { g_pw_maxmt = value; return 0; }
  if (key == 2) { g_pw_roll = value; return 0; }
  if (key == 3) { g_pw4 = value; return 0; }
  if (key >= 4 && key <= 6) return dsgcn_p4_tuning(key - 4, value);
  if (key >= 7 && key <= 9) return dsgcn_wg2_tuning(key - 7, value);
  if (key >= 10 && key <= 12) return dsgcn_p4_tuning(key - 7, value);      // GEMM form: bits, min K, min plane
  if (key == 13) return dsgcn_wg2_tuning(3, value);                        // weight gradient: bf16 terms on / off
  if (key == 14) return dsgcn_p4_tuning(6, value);                         // pre-split weight image: 0 off, 1 k_pwg2, 2 k_pwg3
  if (key >= 15 && key <= 17) return dsgcn_wg2_tuning(key - 11, value);    // wide weight gradient (k_wg3) on / off, split target, co tile
  if (key == 18) return dsgcn_bwd64_tuning(value);                         // one-pass narrow backward: 1 bf16 terms, 0 fp32 MFMA
  if (key == 19) return dsgcn_p4_tuning(7, value);                         // tiny-plane launches: K split over the four waves on / off
  if (key == 22) return dsgcn_p4_tuning(9, value);                         // wide convs on 128-row workgroups (lab)
  if (key == 20) return dsgcn_p4_tuning(8, value);                         // under-filled launches: one row tile per wave on / off
  return DSGCN_EINVAL;
}
#endif

int dsgcn_pwconv_plan(int Tout, int V, int aug, int* TR, int* NPpad, int* nblk_per_sample) {
  int tr = Tout >= 32 ? 8 : 4;
  if (tr > Tout) tr = Tout;
  int np = tr * (V + (aug ? 1 : 0));
  while (np > 256 && tr > 1) { tr >>= 1; np = tr * (V + (aug ? 1 : 0)); }
  if (np > 256) return DSGCN_EUNSUPPORTED;
  *TR = tr;
  *NPpad = (np + 31) & ~31;
  *nblk_per_sample = (Tout + tr - 1) / tr;
  return 0;
}

// ---- forward ----

// Rows of the `partial` buffer the forward writes for a given shape (conv blocks [+ global-joint rows when aug]).
int dsgcn_pwconv_partial_rows(int n, int Ci, int Co, int T, int V, int stride, int aug) {
  int rows = pw_conv_rows(n, Ci, Co, T, V, stride, 1);
  if (aug) rows += n;
  return rows;
}

// Forward.  x2/s1/h1/s2/h2/bias/zaug/partial may be NULL as allowed by the flags.
// partial: (dsgcn_pwconv_partial_rows(...), Co, 2).
// ws: NULL, or the pre-split weight image of dsgcn_pwconv_wsplit (same w): the GEMM-form launches then skip the split of
// the weight tile (csrc/pw4.hip, k_pwg2).
// guest: NULL, or a GUEST conv for the launch's leading workgroups (csrc/pw4.hip: P4Guest).  A pair that is not hosted (the
// host falls to a first-generation kernel or takes another form than the `pre` conv's, the guest is not a tiny-plane plain
// conv, LDS) launches the guest on its own from this call: it is never dropped.  *hosted (may be NULL) = 1 when the host's
// launch carried it, 0 when it went out alone.
int dsgcn_pwconv_fwd_ws_guest(const float* x1, const float* s1, const float* h1, const float* x2, const float* s2,
                              const float* h2, int relu, const float* w, const float* bias, float* z, float* zaug,
                              float* partial, int n, int Ci, int Co, int T, int V, int stride, int aug, int stats,
                              const void* ws, const dsgcn_guest_conv* guest, int* hosted, void* stream) {
  if (hosted) *hosted = 0;
  if (!pw_guest_ok(guest)) return DSGCN_EINVAL;
  int took = 0;
  const int rc = pw_fwd(KcIn{x1, s1, h1, x2, s2, h2, relu}, w, bias, z, zaug, partial, n, Ci, Co, T, V, stride, aug, stats,
                        ws, guest, &took, stream);
  if (rc != 0 || !guest) return rc;
  if (hosted) *hosted = took;
  return took ? 0 : pw_guest_fwd(guest, stream);
}
int dsgcn_pwconv_fwd_ws(const float* x1, const float* s1, const float* h1, const float* x2, const float* s2,
                        const float* h2, int relu, const float* w, const float* bias, float* z, float* zaug,
                        float* partial, int n, int Ci, int Co, int T, int V, int stride, int aug, int stats,
                        const void* ws, void* stream) {
  return dsgcn_pwconv_fwd_ws_guest(x1, s1, h1, x2, s2, h2, relu, w, bias, z, zaug, partial, n, Ci, Co, T, V, stride, aug,
                                   stats, ws, nullptr, nullptr, stream);
}
int dsgcn_pwconv_fwd(const float* x1, const float* s1, const float* h1, const float* x2, const float* s2,
                     const float* h2, int relu, const float* w, const float* bias, float* z, float* zaug,
                     float* partial, int n, int Ci, int Co, int T, int V, int stride, int aug, int stats,
                     void* stream) {
  return dsgcn_pwconv_fwd_ws(x1, s1, h1, x2, s2, h2, relu, w, bias, z, zaug, partial, n, Ci, Co, T, V, stride, aug, stats,
                             nullptr, stream);
}

// 1 = the (Ci -> Co) conv of this shape hosts `guest` (with the weight image passed whenever dsgcn_pwconv_wsplit_bytes asks
// for one), 0 = the guest would go out on its own.  dir 0: dsgcn_pwconv_fwd_ws_guest with a plain operand; dir 1: the
// backward of a plain-input conv with batch-statistics terms (A0 / B0) — dsgcn_pwconv_bwd_guest where dsgcn_pwconv_bwd_rows
// is non-zero, dsgcn_pwconv_dgrad_ws_guest otherwise.
int dsgcn_pwconv_guest_hosted(int dir, int n, int Ci, int Co, int T, int V, int stride, const dsgcn_guest_conv* guest) {
  if (!guest || n <= 0 || Ci <= 0 || Co <= 0 || T <= 0 || V <= 0 || stride != 1 || (dir != 0 && dir != 1)) return 0;
  const int have_ws = (g_pw4 & 3) == 3 && dsgcn_p4_ws_bytes(n, Ci, Co, T * V) != 0;
  if (dir == 0) return (g_pw4 & 1) ? dsgcn_p4_fwd_hosts(n, Ci, Co, T * V, have_ws, guest) : 0;
  if ((g_pw4 & 8) && dsgcn_bwd64_splits(n, Ci, Co, T * V) > 0) return dsgcn_bwd64_hosts(n, Ci, Co, T * V, guest);
  return (g_pw4 & 2) ? dsgcn_p4_dgrad_hosts(n, Ci, Co, T * V, have_ws, guest) : 0;
}

// bf16 products per fp32 product of the launch this shape takes under the CURRENT matmul precision level (dir: 0 forward,
// 1 data gradient, 2 weight gradient): 6 (highest) or 3 (high), 0 = the shape runs an fp32 MFMA form.  Mirrors the
// dispatch of pw_fwd / pw_dgrad / pw_wgrad and the one-pass backward (dsgcn_pwconv_bwd_rows != 0: six terms at both
// levels), for a plain conv (no global-joint column) with the weight image passed wherever dsgcn_pwconv_wsplit_bytes asks
// for one.
int dsgcn_pwconv_terms(int dir, int n, int Ci, int Co, int T, int V, int stride) {
  if (dir < 0 || dir > 2 || n <= 0 || Ci <= 0 || Co <= 0 || T <= 0 || V <= 0 || stride != 1) return 0;
  const int L = T * V;
  if (dir == 0) return (g_pw4 & 3) == 3 ? dsgcn_p4_terms(n, Ci, Co, L, 0) : 0;
  if ((g_pw4 & 8) && dsgcn_bwd64_splits(n, Ci, Co, L) > 0) return dsgcn_bwd64_terms(n, Ci, Co, L);
  if (dir == 1) return (g_pw4 & 3) == 3 ? dsgcn_p4_terms(n, Co, Ci, L, 1) : 0;
  return (g_pw4 & 4) ? dsgcn_wg2_terms(n, Ci, Co, L) : 0;
}

// Bytes of the pre-split weight image (three bf16 terms of W and of W^T, zero-padded to whole tiles) that the forward /
// data gradient of this conv can use; 0 = neither takes the GEMM form (narrow convs, strided convs, tiny planes).
size_t dsgcn_pwconv_wsplit_bytes(int n, int Ci, int Co, int T, int V, int stride) {
  if (n <= 0 || Ci <= 0 || Co <= 0 || T <= 0 || V <= 0 || stride != 1 || (g_pw4 & 3) != 3) return 0;
  return dsgcn_p4_ws_bytes(n, Ci, Co, T * V);
}

int dsgcn_pwconv_wsplit(const float* w, int Ci, int Co, void* ws, void* stream) {
  if (!w || !ws || Ci <= 0 || Co <= 0) return DSGCN_EINVAL;
  return dsgcn_p4_wsplit(w, Ci, Co, ws, (hipStream_t)stream);
}

int dsgcn_pwconv_wsplit_multi(const float* const* w, void* const* ws, const int* Ci, const int* Co, int njobs,
                              void* stream) {
  if (!w || !ws || !Ci || !Co || njobs <= 0) return DSGCN_EINVAL;
  for (int j = 0; j < njobs; ++j)
    if (!w[j] || !ws[j] || Ci[j] <= 0 || Co[j] <= 0) return DSGCN_EINVAL;
  return dsgcn_p4_wsplit_multi(w, ws, Ci, Co, njobs, (hipStream_t)stream);
}

// ---- backward, data path ----

// Rows of the `ipart` buffer the data gradient writes for a given shape.
int dsgcn_pwconv_ipart_rows(int n, int Ci, int Co, int T, int V, int stride) {
  return pw_conv_rows(n, Co, Ci, T, V, stride, 2);
}

// Backward, data path.  gz/gzaug/A0/B0/x2/s*/h*/dx2/ipart may be NULL as in the forward.  dx1 (and dx2) are fully
// written (zero rows where stride skips frames).  ipart: (dsgcn_pwconv_ipart_rows(...), Ci, 3) = [sum dv*x1, sum dv,
// sum dv*x2].  ws: as in the forward.  guest: NULL, or a guest data gradient for the launch's leading workgroups (see
// dsgcn_pwconv_fwd_ws_guest) — guest->in = gz (n, Co, L), guest->out = dx (n, Ci, L), guest->bias unused; launched on its
// own from the same call when the pair is not hosted.
int dsgcn_pwconv_dgrad_ws_guest(const float* x1, const float* s1, const float* h1, const float* x2, const float* s2,
                                const float* h2, int relu, const float* w, const float* z, const float* zaug,
                                const float* gz, const float* gzaug, const float* A0, const float* B0, float* dx1,
                                float* dx2, float* ipart, int n, int Ci, int Co, int T, int V, int stride, int aug,
                                const void* ws, const dsgcn_guest_conv* guest, int* hosted, void* stream) {
  if (hosted) *hosted = 0;
  if (!pw_guest_ok(guest)) return DSGCN_EINVAL;
  int took = 0;
  const int rc = pw_dgrad(KcIn{x1, s1, h1, x2, s2, h2, relu}, w, KcDz{z, gz, A0, B0}, zaug, gzaug, dx1, dx2, ipart, n, Ci, Co,
                          T, V, stride, aug, ws, guest, &took, stream);
  if (rc != 0 || !guest) return rc;
  if (hosted) *hosted = took;
  return took ? 0 : pw_guest_dgrad(guest, stream);
}
int dsgcn_pwconv_dgrad_ws(const float* x1, const float* s1, const float* h1, const float* x2, const float* s2,
                          const float* h2, int relu, const float* w, const float* z, const float* zaug,
                          const float* gz, const float* gzaug, const float* A0, const float* B0, float* dx1, float* dx2,
                          float* ipart, int n, int Ci, int Co, int T, int V, int stride, int aug, const void* ws,
                          void* stream) {
  return dsgcn_pwconv_dgrad_ws_guest(x1, s1, h1, x2, s2, h2, relu, w, z, zaug, gz, gzaug, A0, B0, dx1, dx2, ipart, n, Ci, Co,
                                     T, V, stride, aug, ws, nullptr, nullptr, stream);
}
int dsgcn_pwconv_dgrad(const float* x1, const float* s1, const float* h1, const float* x2, const float* s2,
                       const float* h2, int relu, const float* w, const float* z, const float* zaug,
                       const float* gz, const float* gzaug, const float* A0, const float* B0, float* dx1, float* dx2,
                       float* ipart, int n, int Ci, int Co, int T, int V, int stride, int aug, void* stream) {
  return dsgcn_pwconv_dgrad_ws(x1, s1, h1, x2, s2, h2, relu, w, z, zaug, gz, gzaug, A0, B0, dx1, dx2, ipart, n, Ci, Co, T,
                               V, stride, aug, nullptr, stream);
}

// out (n,Co,T,V) = gz + A0 + B0*z + (gzaug + A0 + B0*zaug)/V   (gz, gzaug, A0/B0 may be NULL = zero)
int dsgcn_dz_eff_aug(const float* gz, const float* z, const float* gzaug, const float* zaug, const float* A0,
                     const float* B0, float* out, int n, int C, int T, int V, void* stream) {
  if (!z || !zaug || !out || n <= 0 || C <= 0 || T <= 0 || V <= 0) return DSGCN_EINVAL;
  if ((T * V) % 4 == 0 && T <= 8192) {
    hipLaunchKernelGGL(k_dz_eff_aug4, dim3((unsigned)((long)n * C)), dim3(64), (size_t)T * 4, (hipStream_t)stream, gz, z,
                       gzaug, zaug, A0, B0, out, C, T, V);
    DSGCN_LAUNCH_CHECK();
    return 0;
  }
  hipLaunchKernelGGL(k_dz_eff_aug, dim3((unsigned)((long)n * C)), dim3(64), 0, (hipStream_t)stream, gz, z, gzaug, zaug,
                     A0, B0, out, C, T, V);
  DSGCN_LAUNCH_CHECK();
  return 0;
}

// ---- backward, weight path ----

// k-split plan of the weight gradient: returns the number of splits (size of dim 0 of dwp / dbp).
int dsgcn_pwconv_wgrad_splits(int n, int Ci, int Co, int T, int V, int stride) {
  return pw_wgrad_splits(n, Ci, Co, T, V, stride);
}

// Backward, weight path.  Partial sums per k-split: split s writes dW at dwp + s*pstride (Co*Ci floats) and db at
// dbp + s*pstride (Co floats); one dsgcn_colsum over (splits, pstride) rows finishes both when they share a buffer.
// The weight gradient carrying BatchNorm coefficient jobs (dsgcn_jobs.h) of the conv's INPUT BatchNorms: their partial rows
// were written by the data gradient launched before this call, nothing on the critical chain waits for the weight gradient,
// so the jobs ride in its launch as extra workgroups (the blocked kernels) or go out as one launch ahead of it (the
// first-generation kernels).  njobs = 0: dsgcn_pwconv_wgrad.
int dsgcn_pwconv_wgrad_jobs(const float* x1, const float* s1, const float* h1, const float* x2, const float* s2,
                            const float* h2, int relu, const float* z, const float* zaug, const float* gz,
                            const float* gzaug, const float* A0, const float* B0, float* dwp, float* dbp, int pstride, int n,
                            int Ci, int Co, int T, int V, int stride, int aug, const dsgcn_bn_coef_job* jobs, int njobs,
                            void* stream) {
  if (!x1 || !dwp || !dbp || n <= 0 || Ci <= 0 || Co <= 0 || T <= 0 || V <= 0 || stride <= 0) return DSGCN_EINVAL;
  if ((A0 && (!B0 || !z)) || (aug && A0 && !zaug)) return DSGCN_EINVAL;
  if (njobs < 0 || njobs > BNJ_MAX || (njobs > 0 && !jobs)) return DSGCN_EINVAL;
  BnCoefTable jt = {};
  jt.n = njobs;
  for (int i = 0; i < njobs; ++i) {
    const dsgcn_bn_coef_job& q = jobs[i];
    jt.j[i] = BnCoefJob{q.part, q.mean, q.var, q.gamma, q.coef, q.count, q.eps, q.R, q.C, q.k, q.i_ds, q.i_dh, q.c_affine,
                        q.accumulate};
  }
  if (!bnj_coef_ok(jt)) return DSGCN_EINVAL;
  return pw_wgrad(KcIn{x1, s1, h1, x2, s2, h2, relu}, KcDz{z, gz, A0, B0}, zaug, gzaug, dwp, dbp, pstride, n, Ci, Co, T, V,
                  stride, aug, jt, stream);
}
int dsgcn_pwconv_wgrad(const float* x1, const float* s1, const float* h1, const float* x2, const float* s2,
                       const float* h2, int relu, const float* z, const float* zaug, const float* gz,
                       const float* gzaug, const float* A0, const float* B0, float* dwp, float* dbp, int pstride, int n,
                       int Ci, int Co, int T, int V, int stride, int aug, void* stream) {
  return dsgcn_pwconv_wgrad_jobs(x1, s1, h1, x2, s2, h2, relu, z, zaug, gz, gzaug, A0, B0, dwp, dbp, pstride, n, Ci, Co, T, V,
                                 stride, aug, nullptr, 0, stream);
}

// ---- one-pass backward ----

// Fused backward (data gradient + weight gradient + input-affine partial sums in one pass over gz, z and the input) for
// narrow convs: stride 1, no global-joint column, Ci and Co <= 64, T*V % 4 == 0 (one or two input streams).
// dsgcn_pwconv_bwd_rows: rows of the partial buffers (dwp/dbp as in dsgcn_pwconv_wgrad with this many splits, ipart
// (rows, Ci, 3)); 0 = shape not covered (use dsgcn_pwconv_dgrad + dsgcn_pwconv_wgrad).
int dsgcn_pwconv_bwd_rows(int n, int Ci, int Co, int T, int V, int stride) {
  if (stride != 1 || !(g_pw4 & 8) || n <= 0 || T <= 0 || V <= 0) return 0;
  return dsgcn_bwd64_splits(n, Ci, Co, T * V);
}

// guest: NULL, or a guest data gradient for the launch's leading workgroups (see dsgcn_pwconv_dgrad_ws_guest)
int dsgcn_pwconv_bwd_guest(const float* x1, const float* s1, const float* h1, const float* x2, const float* s2,
                           const float* h2, int relu, const float* w, const float* z, const float* gz, const float* A0,
                           const float* B0, float* dx1, float* dx2, float* ipart, float* dwp, float* dbp, int pstride, int n,
                           int Ci, int Co, int T, int V, const dsgcn_guest_conv* guest, int* hosted, void* stream) {
  if (hosted) *hosted = 0;
  if (!x1 || !w || !gz || !dx1 || !dwp || !dbp || n <= 0 || Ci <= 0 || Co <= 0 || T <= 0 || V <= 0) return DSGCN_EINVAL;
  if ((A0 && (!B0 || !z)) || (s1 && !h1) || (s2 && !h2) || (x2 && !dx2) || pstride < Co * Ci) return DSGCN_EINVAL;
  if (!pw_guest_ok(guest)) return DSGCN_EINVAL;
  int took = 0;
  const int rc = dsgcn_bwd64(KcIn{x1, s1, h1, x2, s2, h2, relu}, w, KcDz{z, gz, A0, B0}, dx1, dx2, dwp, dbp, pstride, ipart, n,
                             Ci, Co, T * V, (hipStream_t)stream, guest, &took);
  if (rc != 1) return rc == 0 ? DSGCN_EUNSUPPORTED : rc;
  if (!guest) return 0;
  if (hosted) *hosted = took;
  return took ? 0 : pw_guest_dgrad(guest, stream);
}
int dsgcn_pwconv_bwd(const float* x1, const float* s1, const float* h1, const float* x2, const float* s2, const float* h2,
                     int relu, const float* w, const float* z, const float* gz, const float* A0, const float* B0,
                     float* dx1, float* dx2, float* ipart, float* dwp, float* dbp, int pstride, int n, int Ci, int Co,
                     int T, int V, void* stream) {
  return dsgcn_pwconv_bwd_guest(x1, s1, h1, x2, s2, h2, relu, w, z, gz, A0, B0, dx1, dx2, ipart, dwp, dbp, pstride, n, Ci, Co,
                                T, V, nullptr, nullptr, stream);
}

// ---- grouped convs ----

// Up to three 1x1 convs of ONE shape in one launch each way (host arrays of ngroup device pointers): z_g = W_g . (x1_g * s1_g +
// h1_g), no bias / second stream / statistics, stride 1 — CTR-GCN's three conv4's per unit (gcn.py:655-657, one per subset),
// each of which alone leaves the chip under-filled.  dsgcn_pwconv_group_ok: 1 when the shape takes the grouped form (else
// the caller launches the convs one by one); the data gradient writes dx1_g and the input-scale rows ipart_g
// (dsgcn_pwconv_ipart_rows, or NULL for all).
int dsgcn_pwconv_group_ok(int n, int Ci, int Co, int T, int V) {
  if (n <= 0 || Ci <= 0 || Co <= 0 || T <= 0 || V <= 0) return 0;
  return ((g_pw4 & 3) == 3) ? dsgcn_p4_group_ok(n, Ci, Co, T * V) : 0;
}

int dsgcn_pwconv_fwd_group(const float* const* x1, const float* const* s1, const float* const* h1, int relu,
                           const float* const* w, float* const* z, int ngroup, int n, int Ci, int Co, int T, int V,
                           void* stream) {
  if (!x1 || !s1 || !h1 || !w || !z || !pw_group_dims_ok(ngroup, n, Ci, Co, T, V)) return DSGCN_EINVAL;
  for (int g = 0; g < ngroup; ++g)
    if (!x1[g] || !w[g] || !z[g] || ((s1[g] == nullptr) != (h1[g] == nullptr))) return DSGCN_EINVAL;
  if (!dsgcn_pwconv_group_ok(n, Ci, Co, T, V)) return DSGCN_EUNSUPPORTED;
  const int rc = dsgcn_p4_fwd_group(x1, s1, h1, relu, w, z, ngroup, n, Ci, Co, T * V, (hipStream_t)stream);
  return rc == 1 ? 0 : (rc == 0 ? DSGCN_EUNSUPPORTED : rc);
}

int dsgcn_pwconv_dgrad_group(const float* const* x1, const float* const* s1, const float* const* h1, int relu,
                             const float* const* w, const float* const* gz, float* const* dx1, float* const* ipart,
                             int ngroup, int n, int Ci, int Co, int T, int V, void* stream) {
  if (!x1 || !s1 || !h1 || !w || !gz || !dx1 || !ipart || !pw_group_dims_ok(ngroup, n, Ci, Co, T, V)) return DSGCN_EINVAL;
  for (int g = 0; g < ngroup; ++g)
    if (!x1[g] || !w[g] || !gz[g] || !dx1[g] || ((s1[g] == nullptr) != (h1[g] == nullptr))) return DSGCN_EINVAL;
  if (!dsgcn_pwconv_group_ok(n, Ci, Co, T, V)) return DSGCN_EUNSUPPORTED;
  const int rc = dsgcn_p4_dgrad_group(x1, s1, h1, relu, w, gz, dx1, ipart, ngroup, n, Ci, Co, T * V, (hipStream_t)stream);
  return rc == 1 ? 0 : (rc == 0 ? DSGCN_EUNSUPPORTED : rc);
}

// the weight gradients of the same group (dwp_g / dbp_g: partial rows as dsgcn_pwconv_wgrad, dsgcn_pwconv_wgrad_splits rows each)
int dsgcn_pwconv_wgrad_group(const float* const* x1, const float* const* s1, const float* const* h1, int relu,
                             const float* const* gz, float* const* dwp, float* const* dbp, int pstride, int ngroup, int n,
                             int Ci, int Co, int T, int V, void* stream) {
  if (!x1 || !s1 || !h1 || !gz || !dwp || !dbp || !pw_group_dims_ok(ngroup, n, Ci, Co, T, V)) return DSGCN_EINVAL;
  for (int g = 0; g < ngroup; ++g)
    if (!x1[g] || !gz[g] || !dwp[g] || !dbp[g] || ((s1[g] == nullptr) != (h1[g] == nullptr)) ||
        ((s1[g] == nullptr) != (s1[0] == nullptr)))
      return DSGCN_EINVAL;
  if (pstride < Co * Ci || !(g_pw4 & 4)) return pstride < Co * Ci ? DSGCN_EINVAL : DSGCN_EUNSUPPORTED;
  BnCoefTable none = {};
  const int fast = dsgcn_wg2(KcIn{x1[0], s1[0], h1[0], nullptr, nullptr, nullptr, relu}, KcDz{nullptr, gz[0]}, dwp[0], dbp[0],
                             pstride, n, Ci, Co, T * V, (hipStream_t)stream, &none, ngroup, x1, s1, h1, gz, dwp, dbp);
  return fast == 1 ? 0 : (fast == 0 ? DSGCN_EUNSUPPORTED : fast);
}

}  // extern "C"
