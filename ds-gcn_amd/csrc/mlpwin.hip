// The mlp-window stage of dgmsmlp (reference: pyskl/models/gcns/utils/tcn.py:432-523 over unitmlp, tcn.py:525-614) between
// branch_act / tapconv and combine, as ONE launch per direction.  h is (n, C, T, V1), o and u are (n, C, T', V1), V1 = V + 1
// (the global joint is one more column).  Per channel window:
//   mlp  window : dw[c,t',x] = b[c] + sum_j w[c,j] * h[c, t'*s - (KM-1-j)*d, x]      (frames < 0 read as zero; KM = (k+1)/2)
//                 add = 0 : u = W1.dw + b1                 (no dilated conv beside the taps)
//                 add = 1 : u = W1.(dw + o) + b1           (o = alpha * dilated conv of h, written by tapconv)
//                 add = 2 : u = W1.dw + b1 + o
//   copy window : u = o                                    (max-pool / strided pass-through, written by tapconv)
// A channel of o that no window names is never read.  Replaces dsgcn_dwcausal + a C x C block-diagonal dsgcn_pwconv + an
// add (six plane passes) by: read h, read o, write u.
//
// The bc x bc mix (bc <= 64, odd widths) runs on v_mfma_f32_16x16x4_f32 (fp32 in, fp32 accumulate: exact fp32, the
// library's 'highest' class; the matmul-precision switch does not reach this file).  W1 is staged once per workgroup in LDS,
// zero padded to whole 16-row tiles (never in HBM); a tile is 64 consecutive positions of the (T', V1) plane, whose dw values
// are formed straight from h (each h element is read KM times, from L1/L2) and kept in LDS as the B operand.
//
// Backward: one workgroup owns (sample, window) and walks the tiles, so dW1 = du.dw^T (dw recomputed from h) and db1 stay
// in registers until the end; g = W1^T.du goes to global memory (do itself under add = 1, a work buffer otherwise) and is
// read back by the same workgroup for the transposed taps (dh) and the tap gradients.  Every workgroup writes its own
// segment of partial row n — [dtap (C*KM) | dtap bias (C) | per mlp window: dW1 (bc*bc), db1 (bc)] — and dsgcn_colsum sums
// the rows: no float atomics, bit-identical run to run.
#include "common.h"

namespace {

constexpr int MW_NT = 256;
constexpr int MW_MAXWIN = 8;
constexpr int MW_P = 64;         // positions per tile
constexpr int MW_SW = 66;        // row stride of a W1 image: A operand (row on lane&15, k on lane>>4), 32 banks: 2*row + k
constexpr int MW_SX = 80;        // forward dw image [k][p]: B operand (k on lane>>4, p on lane&15): 16*k + p
constexpr int MW_SU = 81;        // backward du image [o][p]: read as B over o and as A over p: 17 is free of conflicts both ways
constexpr int MW_SD = 66;        // backward dw image [c][p]: B operand with k = p

struct MWin {
  int type;            // 0 mlp, 1 copy
  int c0, bc, dil;
  int add;             // 0 none, 1 before the mix, 2 after it
  int poff;            // offset of [dW1 | db1] in a partial row
  const float* w1;     // (bc, bc)
  const float* b1;     // (bc) or NULL
};

struct MArgs {
  const float* h;      // (n, C, T, V1)
  const float* o;      // (n, C, Tout, V1)
  const float* du;     // gradient of u
  const float* tapw;   // (C, KM)
  const float* tapb;   // (C) or NULL
  float* u;
  float* dh;
  float* dout;         // gradient of o
  float* gbuf;         // (n, C, Tout, V1) work buffer for g = W1^T.du
  float* part;         // (n, pstride)
  int n, C, T, Tout, V1, stride, KM, nwin, pstride, chunks;
  MWin win[MW_MAXWIN];
};

// taps of one channel in LDS: [0..4] w (zero past KM), [5] bias
__device__ __forceinline__ float mw_dw(const float* __restrict__ hc, const float* tp, int t0, int v, int V1, int KM,
                                       int dil) {
  float acc = tp[5];
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    const int t = t0 - (KM - 1 - j) * dil;
    if (j < KM && t >= 0) acc = fmaf(tp[j], hc[(size_t)t * V1 + v], acc);
  }
  return acc;
}

// g is written and read back by one workgroup, but a 128-byte line at the edge of its planes is shared with a neighbour
// that may have pulled it into this CU's L1 earlier: read it back from L2.
__device__ __forceinline__ float mw_ld_l2(const float* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void mw_stage_taps(const MArgs& a, const MWin& w, float* taps) {
  for (int i = threadIdx.x; i < w.bc * 6; i += MW_NT) {
    const int c = i / 6, j = i - c * 6;
    float v = 0.f;
    if (j < a.KM) v = a.tapw[(size_t)(w.c0 + c) * a.KM + j];
    else if (j == 5 && a.tapb) v = a.tapb[w.c0 + c];
    taps[i] = v;
  }
}

__global__ __launch_bounds__(MW_NT) void k_mlpwin_fwd(MArgs a) {
  __shared__ float W1s[64 * MW_SW];
  __shared__ float Xs[64 * MW_SX];
  __shared__ float taps[64 * 6];
  __shared__ float b1s[64];
  const int tid = threadIdx.x;
  const int chunk = blockIdx.x % a.chunks;
  const int rest = blockIdx.x / a.chunks;
  const int wi = rest % a.nwin, n = rest / a.nwin;
  const MWin& w = a.win[wi];
  const int V1 = a.V1, L = a.Tout * V1, ntiles = (L + MW_P - 1) / MW_P;
  const size_t planeI = (size_t)a.T * V1, planeO = (size_t)L;
  const int bc = w.bc;
  const int pl = tid & 63, kr = tid >> 6;
  if (w.type != 0) {
    for (int tile = chunk; tile < ntiles; tile += a.chunks) {
      const int pos = tile * MW_P + pl;
      if (pos >= L) continue;
      for (int c = kr; c < bc; c += 4) {
        const size_t idx = ((size_t)n * a.C + w.c0 + c) * planeO + pos;
        a.u[idx] = a.o[idx];
      }
    }
    return;
  }
  const int M16 = (bc + 15) & ~15;
  for (int i = tid; i < M16 * M16; i += MW_NT) {
    const int r = i / M16, c = i - r * M16;
    W1s[r * MW_SW + c] = (r < bc && c < bc) ? w.w1[r * bc + c] : 0.f;
  }
  mw_stage_taps(a, w, taps);
  if (tid < 64) b1s[tid] = (tid < bc && w.b1) ? w.b1[tid] : 0.f;
  __syncthreads();
  const int lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lk = lane >> 4;
  for (int tile = chunk; tile < ntiles; tile += a.chunks) {
    {
      const int pos = tile * MW_P + pl;
      const bool valid = pos < L;
      const int tp = pos / V1, v = pos - tp * V1;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int ch = kr + 4 * i;
        if (ch < M16) {
          float x = 0.f;
          if (valid && ch < bc) {
            const size_t pc = (size_t)n * a.C + w.c0 + ch;
            x = mw_dw(a.h + pc * planeI, taps + ch * 6, tp * a.stride, v, V1, a.KM, w.dil);
            if (w.add == 1) x += a.o[pc * planeO + pos];
          }
          Xs[ch * MW_SX + pl] = x;
        }
      }
    }
    __syncthreads();
    f32x4 acc[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) acc[m] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < M16; k0 += 4) {
      const float b = Xs[(k0 + lk) * MW_SX + wave * 16 + lr];
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        if (m * 16 < M16) {
          const float av = W1s[(m * 16 + lr) * MW_SW + k0 + lk];
          acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b, acc[m], 0, 0, 0);
        }
      }
    }
    // D[i = 4*(lane>>4) + r][j = lane&15]: i = output channel of the tile, j = position
    const int opos = tile * MW_P + wave * 16 + lr;
    if (opos < L) {
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        if (m * 16 < M16) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int ch = m * 16 + 4 * lk + r;
            if (ch < bc) {
              const size_t idx = ((size_t)n * a.C + w.c0 + ch) * planeO + opos;
              float val = acc[m][r] + b1s[ch];
              if (w.add == 2) val += a.o[idx];
              a.u[idx] = val;
            }
          }
        }
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(MW_NT) void k_mlpwin_bwd(MArgs a) {
  __shared__ float W1T[64 * MW_SW];     // [c][o] = W1[o][c]
  __shared__ float Us[64 * MW_SU];      // du [o][p]
  __shared__ float Ds[64 * MW_SD];      // dw (+ o under add = 1) [c][p]
  __shared__ float taps[64 * 6];
  const int tid = threadIdx.x;
  const int wi = blockIdx.x % a.nwin, n = blockIdx.x / a.nwin;
  const MWin& w = a.win[wi];
  const int V1 = a.V1, L = a.Tout * V1, LI = a.T * V1, ntiles = (L + MW_P - 1) / MW_P;
  const size_t planeI = (size_t)LI, planeO = (size_t)L;
  const int bc = w.bc, KM = a.KM;
  const int pl = tid & 63, kr = tid >> 6;
  float* __restrict__ prow = a.part + (size_t)n * a.pstride;
  if (w.type != 0) {
    // copy window: do = du, dh = 0, no tap gradients
    for (int c = kr; c < bc; c += 4) {
      const size_t pc = (size_t)n * a.C + w.c0 + c;
      for (int i = pl; i < L; i += 64) a.dout[pc * planeO + i] = a.du[pc * planeO + i];
      for (int i = pl; i < LI; i += 64) a.dh[pc * planeI + i] = 0.f;
    }
    for (int i = tid; i < bc * KM; i += MW_NT) prow[(size_t)w.c0 * KM + i] = 0.f;
    for (int i = tid; i < bc; i += MW_NT) prow[(size_t)a.C * KM + w.c0 + i] = 0.f;
    return;
  }
  const int M16 = (bc + 15) & ~15;
  for (int i = tid; i < M16 * M16; i += MW_NT) {
    const int c = i / M16, o = i - c * M16;
    W1T[c * MW_SW + o] = (c < bc && o < bc) ? w.w1[o * bc + c] : 0.f;
  }
  mw_stage_taps(a, w, taps);
  __syncthreads();
  const int lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lk = lane >> 4;
  float* __restrict__ gp = w.add == 1 ? a.dout : a.gbuf;
  float dbacc[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) dbacc[i] = 0.f;
  f32x4 accw[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) accw[m] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int tile = 0; tile < ntiles; ++tile) {
    {
      const int pos = tile * MW_P + pl;
      const bool valid = pos < L;
      const int tp = pos / V1, v = pos - tp * V1;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int ch = kr + 4 * i;
        if (ch < M16) {
          float g = 0.f, x = 0.f;
          if (valid && ch < bc) {
            const size_t pc = (size_t)n * a.C + w.c0 + ch;
            g = a.du[pc * planeO + pos];
            x = mw_dw(a.h + pc * planeI, taps + ch * 6, tp * a.stride, v, V1, KM, w.dil);
            if (w.add == 1) x += a.o[pc * planeO + pos];
            else a.dout[pc * planeO + pos] = w.add == 2 ? g : 0.f;
          }
          dbacc[i] += g;
          Us[ch * MW_SU + pl] = g;
          Ds[ch * MW_SD + pl] = x;
        }
      }
    }
    __syncthreads();
    // g[c][p] = sum_o W1[o][c] du[o][p]: wave = 16 positions, m = 16 channels c
    {
      f32x4 acc[4];
#pragma unroll
      for (int m = 0; m < 4; ++m) acc[m] = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int k0 = 0; k0 < M16; k0 += 4) {
        const float b = Us[(k0 + lk) * MW_SU + wave * 16 + lr];
#pragma unroll
        for (int m = 0; m < 4; ++m) {
          if (m * 16 < M16) {
            const float av = W1T[(m * 16 + lr) * MW_SW + k0 + lk];
            acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b, acc[m], 0, 0, 0);
          }
        }
      }
      const int opos = tile * MW_P + wave * 16 + lr;
      if (opos < L) {
#pragma unroll
        for (int m = 0; m < 4; ++m) {
          if (m * 16 < M16) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int ch = m * 16 + 4 * lk + r;
              if (ch < bc) gp[((size_t)n * a.C + w.c0 + ch) * planeO + opos] = acc[m][r];
            }
          }
        }
      }
    }
    // dW1[o][c] += sum_p du[o][p] dw[c][p]: wave = 16 rows o, m = 16 columns c, k = the tile's 64 positions
    if (wave * 16 < M16) {
      for (int k0 = 0; k0 < MW_P; k0 += 4) {
        const float av = Us[(wave * 16 + lr) * MW_SU + k0 + lk];
#pragma unroll
        for (int m = 0; m < 4; ++m) {
          if (m * 16 < M16) {
            const float b = Ds[(m * 16 + lr) * MW_SD + k0 + lk];
            accw[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b, accw[m], 0, 0, 0);
          }
        }
      }
    }
    __syncthreads();
  }
  // dW1, db1 -> this window's segment of row n
  if (wave * 16 < M16) {
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      if (m * 16 < M16) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int o = wave * 16 + 4 * lk + r, c = m * 16 + lr;
          if (o < bc && c < bc) prow[(size_t)w.poff + o * bc + c] = accw[m][r];
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int ch = kr + 4 * i;
    if (ch < bc) {                           // (uniform over the wave)
      const float s = wave_sum(dbacc[i]);
      if (lane == 0) prow[(size_t)w.poff + bc * bc + ch] = s;
    }
  }
  // the stores of g above are this workgroup's own: in L2 after the fence, read back from there (mw_ld_l2)
  __threadfence();
  __syncthreads();
  // one wave per channel: tap gradients over the output positions, then dh = transposed taps over the input positions
  for (int ch = wave; ch < bc; ch += 4) {
    const size_t pc = (size_t)n * a.C + w.c0 + ch;
    const float* __restrict__ ph = a.h + pc * planeI;
    const float* pg = gp + pc * planeO;
    const float* tp6 = taps + ch * 6;
    float sw[5], sb = 0.f;
#pragma unroll
    for (int j = 0; j < 5; ++j) sw[j] = 0.f;
    for (int i = lane; i < L; i += 64) {
      const int tp = i / V1, v = i - tp * V1;
      const float g = mw_ld_l2(pg + i);
      sb += g;
#pragma unroll
      for (int j = 0; j < 5; ++j) {
        const int t = tp * a.stride - (KM - 1 - j) * w.dil;
        if (j < KM && t >= 0) sw[j] = fmaf(g, ph[(size_t)t * V1 + v], sw[j]);
      }
    }
#pragma unroll
    for (int j = 0; j < 5; ++j) sw[j] = wave_sum(sw[j]);
    sb = wave_sum(sb);
    if (lane == 0) {
#pragma unroll
      for (int j = 0; j < 5; ++j)
        if (j < KM) prow[(size_t)(w.c0 + ch) * KM + j] = sw[j];
      prow[(size_t)a.C * KM + w.c0 + ch] = sb;
    }
    float* __restrict__ pdh = a.dh + pc * planeI;
    for (int i = lane; i < LI; i += 64) {
      const int t = i / V1, v = i - t * V1;
      float acc = 0.f;
#pragma unroll
      for (int j = 0; j < 5; ++j) {
        const int num = t + (KM - 1 - j) * w.dil;
        if (j < KM && num % a.stride == 0) {
          const int tp = num / a.stride;
          if (tp < a.Tout) acc = fmaf(tp6[j], mw_ld_l2(pg + (size_t)tp * V1 + v), acc);
        }
      }
      pdh[i] = acc;
    }
  }
}

// 1 = in range; 0 = not (the caller takes the staged form); fills the windows when `a` is given
int mw_plan(MArgs* a, int n, int C, int T, int V1, int stride, int KM, int nwin, const int* type, const int* c0,
            const int* width, const int* dil, const int* add) {
  if (n <= 0 || C <= 0 || T <= 0 || V1 <= 0 || nwin <= 0 || !type || !c0 || !width || !dil || !add) return 0;
  if (nwin > MW_MAXWIN || V1 > 33 || (stride != 1 && stride != 2) || (KM != 2 && KM != 3 && KM != 5)) return 0;
  const int Tout = (T + stride - 1) / stride;
  if ((size_t)n * C * T * V1 >= ((size_t)1 << 40)) return 0;
  int next = 0, poff = C * KM + C, nmlp = 0;
  for (int i = 0; i < nwin; ++i) {
    if (c0[i] != next || width[i] <= 0) return 0;           // the windows tile [0, C) in order
    next += width[i];
    if (type[i] == 0) {
      if (width[i] > 64 || dil[i] < 1 || add[i] < 0 || add[i] > 2) return 0;
      ++nmlp;
    } else if (type[i] != 1 || add[i] != 0) {
      return 0;
    }
    if (a) {
      MWin& w = a->win[i];
      w.type = type[i]; w.c0 = c0[i]; w.bc = width[i]; w.dil = dil[i]; w.add = add[i];
      w.poff = type[i] == 0 ? poff : 0;
    }
    if (type[i] == 0) poff += width[i] * width[i] + width[i];
  }
  if (next != C || nmlp == 0) return 0;
  if (a) {
    a->n = n; a->C = C; a->T = T; a->Tout = Tout; a->V1 = V1; a->stride = stride; a->KM = KM; a->nwin = nwin;
    a->pstride = poff;
  }
  return 1;
}

}  // namespace

extern "C" {

// Window tables as parallel host arrays (nwin <= 8, the windows tile [0, C) in order): type (0 mlp / 1 copy), first channel,
// width, dilation, add (0 none / 1 before the mix / 2 after it; 0 for copy windows).
int dsgcn_mlpwin_supported(int n, int C, int T, int V1, int stride, int KM, int nwin, const int* type, const int* c0,
                           const int* width, const int* dil, const int* add) {
  return mw_plan(nullptr, n, C, T, V1, stride, KM, nwin, type, c0, width, dil, add);
}

int dsgcn_mlpwin_partial_stride(int C, int KM, int nwin, const int* type, const int* width) {
  if (C <= 0 || KM <= 0 || nwin <= 0 || nwin > MW_MAXWIN || !type || !width) return DSGCN_EINVAL;
  int p = C * KM + C;
  for (int i = 0; i < nwin; ++i)
    if (type[i] == 0) p += width[i] * width[i] + width[i];
  return p;
}

int dsgcn_mlpwin_fwd(const float* h, const float* o, float* u, const float* tapw, const float* tapb, int n, int C, int T,
                     int V1, int stride, int KM, int nwin, const int* type, const int* c0, const int* width, const int* dil,
                     const int* add, const float* const* w1, const float* const* b1, void* stream) {
  if (!h || !u || !tapw || !w1 || !type || !c0 || !width || !dil || !add || n <= 0 || C <= 0 || T <= 0 || V1 <= 0 ||
      stride <= 0 || nwin <= 0)
    return DSGCN_EINVAL;
  MArgs a = {};
  if (!mw_plan(&a, n, C, T, V1, stride, KM, nwin, type, c0, width, dil, add)) return DSGCN_EUNSUPPORTED;
  for (int i = 0; i < nwin; ++i) {
    a.win[i].w1 = w1[i]; a.win[i].b1 = b1 ? b1[i] : nullptr;
    if (type[i] == 0 && !w1[i]) return DSGCN_EINVAL;
    if ((type[i] != 0 || add[i] != 0) && !o) return DSGCN_EINVAL;
  }
  a.h = h; a.o = o; a.u = u; a.tapw = tapw; a.tapb = tapb;
  const int ntiles = (a.Tout * V1 + MW_P - 1) / MW_P;
  a.chunks = ntiles < 8 ? ntiles : 8;
  const size_t blocks = (size_t)n * nwin * a.chunks;
  if (blocks >= ((size_t)1 << 31)) return DSGCN_EUNSUPPORTED;
  hipLaunchKernelGGL(k_mlpwin_fwd, dim3((unsigned)blocks), dim3(MW_NT), 0, (hipStream_t)stream, a);
  DSGCN_LAUNCH_CHECK();
  return 0;
}

// dh (n,C,T,V1), dout (n,C,T',V1) and part (n, pstride = dsgcn_mlpwin_partial_stride) are written whole; gbuf (n,C,T',V1)
// is a work buffer (needed unless every mlp window has add = 1); o is read under add = 1 only; tapb (NULL = none) is
// the forward's: dW1 takes the recomputed dw.
int dsgcn_mlpwin_bwd(const float* h, const float* o, const float* du, const float* tapw, const float* tapb, float* dh,
                     float* dout, float* gbuf, float* part, int n, int C, int T, int V1, int stride, int KM, int nwin, const int* type,
                     const int* c0, const int* width, const int* dil, const int* add, const float* const* w1, int pstride,
                     void* stream) {
  if (!h || !du || !tapw || !dh || !dout || !part || !w1 || !type || !c0 || !width || !dil || !add || n <= 0 || C <= 0 ||
      T <= 0 || V1 <= 0 || stride <= 0 || nwin <= 0)
    return DSGCN_EINVAL;
  MArgs a = {};
  if (!mw_plan(&a, n, C, T, V1, stride, KM, nwin, type, c0, width, dil, add)) return DSGCN_EUNSUPPORTED;
  if (pstride != a.pstride) return DSGCN_EINVAL;
  for (int i = 0; i < nwin; ++i) {
    a.win[i].w1 = w1[i];
    if (type[i] == 0 && !w1[i]) return DSGCN_EINVAL;
    if (type[i] == 0 && add[i] == 1 && !o) return DSGCN_EINVAL;
    if (type[i] == 0 && add[i] != 1 && !gbuf) return DSGCN_EINVAL;
  }
  a.h = h; a.o = o; a.du = du; a.tapw = tapw; a.tapb = tapb; a.dh = dh; a.dout = dout; a.gbuf = gbuf; a.part = part;
  const size_t blocks = (size_t)n * nwin;
  if (blocks >= ((size_t)1 << 31)) return DSGCN_EUNSUPPORTED;
  hipLaunchKernelGGL(k_mlpwin_bwd, dim3((unsigned)blocks), dim3(MW_NT), 0, (hipStream_t)stream, a);
  DSGCN_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
