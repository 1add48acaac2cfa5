// Position-typed 1x1 conv (CTRHGC's target_specific / full_channels arms, gcn.py:737-766):
//
//   y[n, o, pos] = sum_c W[type(pos)][o][c] * x[n, c, pos] + b[type(pos)][o],   type(pos) = table[pos % L]
//
// The reference computes it as a conv to P x the channels followed by a per-position select; here every position is
// multiplied by the one weight matrix of its type.  An MFMA tile needs ONE weight matrix, so the host sorts the positions
// of a chunk (G periods of the table) by type once (kernels_typedconv.typed_plan): `perm` lists the chunk's positions
// type by type, every type's run padded with -1 to whole 32-column tiles, `tile_type` names the type of each tile and
// `tile_off` (17 entries) the first tile of each type.  The kernels gather the columns of a tile through `perm` into
// LDS, multiply on v_mfma_f32_32x32x2_f32 (fp32 in, out and accumulate at both matmul precision levels) and scatter the
// result back through the same `perm`.  Every position of a chunk is in exactly one tile, so y / dx are written completely.
//
//   k_typedconv<0>   forward:        rows = Co, depth = Ci, A = W[p] (row-major)
//   k_typedconv<1>   data gradient:  rows = Ci, depth = Co, A = W[p]^T   (the same body, the weight read transposed)
//   k_typedconv_wgrad               dW[p] = sum over the positions of type p of dy x^T, db[p] = sum dy: per split of the
//                                    samples one partial (P, Co, Ci) + (P, Co); the caller adds the splits in order
//                                    (dsgcn_colsum) — no float atomics, the same bits every run.  x carries a virtual
//                                    channel Ci of ones whose column of the product is db.
// All global accesses are single dwords: the operands may sit at any 4-byte-aligned address.
#include "common.h"

namespace {

constexpr int TC_TILE = 32;                    // positions of one type per tile
constexpr int TC_NS = 4;                       // samples per workgroup: the same tile of each shares the weight fragment
constexpr int TC_ROWS = 128;                   // output rows per workgroup (4 waves x 32)
constexpr int TC_KC = 32;                      // reduction depth per LDS stage
constexpr int TC_XS = TC_NS * TC_TILE + 32;    // LDS row of the gathered columns: the two lane halves hit disjoint banks
constexpr int TC_WS = TC_KC + 2;               // LDS row of the weights: 34 l mod 64 is distinct and even for l < 32
constexpr int TC_OFF = 17;                     // tile_off entries in front of tile_type (P <= 16)

// x (n, K, TV), W (P, M, K) [TRANS: (P, K, M)], b (P, M) or NULL -> y (n, M, TV)
template <int TRANS>
__global__ __launch_bounds__(256) void k_typedconv(const float* __restrict__ x, const float* __restrict__ W,
                                                   const float* __restrict__ b, const int* __restrict__ tile_type,
                                                   const int* __restrict__ perm, float* __restrict__ y, int n, int K,
                                                   int M, int TV, int chunk, int nchunks, int P) {
  __shared__ float Xs[TC_KC * TC_XS];
  __shared__ float Ws[TC_ROWS * TC_WS];
  const int tile = blockIdx.x;
  const int chunk_i = blockIdx.y % nchunks;
  const int n0 = (blockIdx.y / nchunks) * TC_NS;
  const int m0 = blockIdx.z * TC_ROWS;
  const int base = chunk_i * chunk;
  const int p = tile_type[tile];
  if ((unsigned)p >= (unsigned)P) return;
  const int first = perm[tile * TC_TILE];                  // a type's run is ascending: nothing of this tile is in the plane
  if (first < 0 || base + first >= TV) return;             // (uniform over the workgroup, before any barrier)

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, half = lane >> 5;
  // gather: this thread owns column `col` (sample col / 32, tile column col % 32), channels crow, crow + 2, ...
  const int col = tid & 127, crow = tid >> 7;
  const int gs = n0 + (col >> 5);
  const int gp = perm[tile * TC_TILE + (col & 31)];
  const bool gok = gp >= 0 && base + gp < TV && gs < n;
  const float* __restrict__ xcol = x + ((size_t)(gok ? gs : 0) * K) * TV + (gok ? base + gp : 0);
  const bool wave_on = m0 + 32 * wave < M;

  f32x16 acc[TC_NS];
#pragma unroll
  for (int s = 0; s < TC_NS; ++s)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[s][r] = 0.f;

  for (int k0 = 0; k0 < K; k0 += TC_KC) {
    float xr[TC_KC / 2], wr[16];
#pragma unroll
    for (int i = 0; i < TC_KC / 2; ++i) {
      const int c = k0 + crow + 2 * i;
      xr[i] = (gok && c < K) ? xcol[(size_t)c * TV] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      int r, kk;
      if (TRANS) { r = tid & 127; kk = (tid >> 7) + 2 * i; }
      else { kk = tid & 31; r = (tid >> 5) + 8 * i; }
      const int m = m0 + r, k = k0 + kk;
      float v = 0.f;
      if (m < M && k < K) v = TRANS ? W[((size_t)p * K + k) * M + m] : W[((size_t)p * M + m) * K + k];
      wr[i] = v;
    }
    __syncthreads();                                       // the previous stage's fragments are read
#pragma unroll
    for (int i = 0; i < TC_KC / 2; ++i) Xs[(crow + 2 * i) * TC_XS + col] = xr[i];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      int r, kk;
      if (TRANS) { r = tid & 127; kk = (tid >> 7) + 2 * i; }
      else { kk = tid & 31; r = (tid >> 5) + 8 * i; }
      Ws[r * TC_WS + kk] = wr[i];
    }
    __syncthreads();
    if (wave_on) {
#pragma unroll 4
      for (int kk = 0; kk < TC_KC; kk += 2) {
        const float av = Ws[(32 * wave + l31) * TC_WS + kk + half];
#pragma unroll
        for (int s = 0; s < TC_NS; ++s) {
          const float bv = Xs[(kk + half) * TC_XS + 32 * s + l31];
          acc[s] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[s], 0, 0, 0);
        }
      }
    }
  }
  if (!wave_on) return;
  // D[i = row][j = tile column]: lane = column, registers = rows
  const int op = perm[tile * TC_TILE + l31];
  if (op < 0 || base + op >= TV) return;
  float bias[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int m = m0 + 32 * wave + mfma_row32(r, half);
    bias[r] = (b && m < M) ? b[(size_t)p * M + m] : 0.f;
  }
#pragma unroll
  for (int s = 0; s < TC_NS; ++s) {
    if (n0 + s >= n) break;
    float* __restrict__ ycol = y + ((size_t)(n0 + s) * M) * TV + base + op;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = m0 + 32 * wave + mfma_row32(r, half);
      if (m < M) ycol[(size_t)m * TV] = acc[s][r] + bias[r];
    }
  }
}

// One workgroup: the 64 x 64 block (co0, ci0) of dW[p] (channel Ci of x = ones: db) over the samples of split blockIdx.z.
// part: (S, P*Co*Ci + P*Co).
__global__ __launch_bounds__(256) void k_typedconv_wgrad(const float* __restrict__ x, const float* __restrict__ dy,
                                                         const int* __restrict__ tile_off, const int* __restrict__ perm,
                                                         float* __restrict__ part, int n, int Ci, int Co, int TV,
                                                         int chunk, int nchunks, int P, int per, int ci_blocks,
                                                         int ntiles, size_t pstride) {
  __shared__ float Ds[64 * TC_WS];
  __shared__ float Xs[64 * TC_WS];
  const int p = blockIdx.y;
  const int ci0 = (blockIdx.x % ci_blocks) * 64, co0 = (blockIdx.x / ci_blocks) * 64;
  const int s0 = blockIdx.z * per, s1 = min(n, s0 + per);
  const int t0 = max(tile_off[p], 0), t1 = min(tile_off[p + 1], ntiles);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, half = lane >> 5;
  const int wm = wave & 1, wn = wave >> 1;
  const int j = tid & 31, r0 = tid >> 5;                   // gather: tile column j, rows r0, r0 + 8, ...

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;

  for (int s = s0; s < s1; ++s) {
    for (int c = 0; c < nchunks; ++c) {
      const int base = c * chunk;
      for (int t = t0; t < t1; ++t) {
        const int first = perm[t * TC_TILE];
        if (first < 0 || base + first >= TV) break;        // ascending run: the later tiles lie outside the plane too
        const int gp = perm[t * TC_TILE + j];
        const bool ok = gp >= 0 && base + gp < TV;
        const size_t pos = ok ? (size_t)(base + gp) : 0;
        float dr[8], xr[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int co = co0 + r0 + 8 * i, ci = ci0 + r0 + 8 * i;
          dr[i] = (ok && co < Co) ? dy[((size_t)s * Co + co) * TV + pos] : 0.f;
          xr[i] = !ok ? 0.f : (ci < Ci ? x[((size_t)s * Ci + ci) * TV + pos] : (ci == Ci ? 1.f : 0.f));
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          Ds[(r0 + 8 * i) * TC_WS + j] = dr[i];
          Xs[(r0 + 8 * i) * TC_WS + j] = xr[i];
        }
        __syncthreads();
#pragma unroll 4
        for (int kk = 0; kk < TC_TILE; kk += 2) {
          const float av = Ds[(32 * wm + l31) * TC_WS + kk + half];
          const float bv = Xs[(32 * wn + l31) * TC_WS + kk + half];
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
        }
      }
    }
  }
  // D[i = co][j = ci]
  const int ci = ci0 + 32 * wn + l31;
  if (ci > Ci) return;
  float* __restrict__ row = part + (size_t)blockIdx.z * pstride;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int co = co0 + 32 * wm + mfma_row32(r, half);
    if (co >= Co) continue;
    if (ci < Ci) row[((size_t)p * Co + co) * Ci + ci] = acc[r];
    else row[(size_t)P * Co * Ci + (size_t)p * Co + co] = acc[r];
  }
}

int tc_check(const void* a, const void* b, const void* c, const int* plan, int ntiles, int n, int Ci, int Co, int TV, int L,
             int chunk, int P) {
  if (!a || !b || !c || !plan || ntiles <= 0 || n <= 0 || Ci <= 0 || Co <= 0 || TV <= 0 || L <= 0 || P <= 0 || chunk <= 0 ||
      chunk % L != 0)
    return DSGCN_EINVAL;
  if (P > DSGCN_TYPED_MAX_TYPES || L > DSGCN_TYPED_MAX_PERIOD || chunk > 2 * DSGCN_TYPED_MAX_PERIOD ||
      ntiles > (chunk + P * (TC_TILE - 1)) / TC_TILE || (long)n * Ci * TV >= (1L << 31) || (long)n * Co * TV >= (1L << 31))
    return DSGCN_EUNSUPPORTED;
  return 0;
}

int tc_splits(int n, int Ci, int Co, int P) {
  const long blocks = (long)((Ci + 1 + 63) / 64) * ((Co + 63) / 64) * P;
  long S = (1024 + blocks - 1) / blocks;
  if (S > n) S = n;
  if (S > 64) S = 64;
  if (S < 1) S = 1;
  const int per = (int)((n + S - 1) / S);
  return (n + per - 1) / per;
}

template <int TRANS>
int tc_launch(const float* x, const float* w, const float* b, const int* plan, int ntiles, float* y, int n, int K, int M,
              int TV, int chunk, int P, void* stream) {
  const int nchunks = (TV + chunk - 1) / chunk;
  const long gy = (long)nchunks * ((n + TC_NS - 1) / TC_NS);
  if (gy > 65535) return DSGCN_EUNSUPPORTED;
  hipLaunchKernelGGL(k_typedconv<TRANS>, dim3((unsigned)ntiles, (unsigned)gy, (unsigned)((M + TC_ROWS - 1) / TC_ROWS)),
                     dim3(256), 0, (hipStream_t)stream, x, w, b, plan + TC_OFF, plan + TC_OFF + ntiles, y, n, K, M, TV,
                     chunk, nchunks, P);
  DSGCN_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" {

int dsgcn_typedconv_fwd(const float* x, const float* w, const float* b, const int* plan, int ntiles, float* y, int n,
                        int Ci, int Co, int TV, int L, int chunk, int P, void* stream) {
  const int rc = tc_check(x, w, y, plan, ntiles, n, Ci, Co, TV, L, chunk, P);
  if (rc) return rc;
  return tc_launch<0>(x, w, b, plan, ntiles, y, n, Ci, Co, TV, chunk, P, stream);
}

int dsgcn_typedconv_dgrad(const float* dy, const float* w, const int* plan, int ntiles, float* dx, int n, int Ci, int Co,
                          int TV, int L, int chunk, int P, void* stream) {
  const int rc = tc_check(dy, w, dx, plan, ntiles, n, Ci, Co, TV, L, chunk, P);
  if (rc) return rc;
  return tc_launch<1>(dy, w, nullptr, plan, ntiles, dx, n, Co, Ci, TV, chunk, P, stream);
}

int dsgcn_typedconv_wgrad_rows(int n, int Ci, int Co, int P) {
  if (n <= 0 || Ci <= 0 || Co <= 0 || P <= 0) return DSGCN_EINVAL;
  if (P > DSGCN_TYPED_MAX_TYPES) return DSGCN_EUNSUPPORTED;
  return tc_splits(n, Ci, Co, P);
}

int dsgcn_typedconv_wgrad(const float* x, const float* dy, const int* plan, int ntiles, float* part, int n, int Ci, int Co,
                          int TV, int L, int chunk, int P, void* stream) {
  const int rc = tc_check(x, dy, part, plan, ntiles, n, Ci, Co, TV, L, chunk, P);
  if (rc) return rc;
  const int S = tc_splits(n, Ci, Co, P);
  const int per = (n + S - 1) / S;
  const int ci_blocks = (Ci + 1 + 63) / 64, co_blocks = (Co + 63) / 64;
  const int nchunks = (TV + chunk - 1) / chunk;
  const size_t pstride = (size_t)P * Co * Ci + (size_t)P * Co;
  hipLaunchKernelGGL(k_typedconv_wgrad, dim3((unsigned)(ci_blocks * co_blocks), (unsigned)P, (unsigned)S), dim3(256), 0,
                     (hipStream_t)stream, x, dy, plan, plan + TC_OFF + ntiles, part, n, Ci, Co, TV, chunk, nchunks, P, per,
                     ci_blocks, ntiles, pstride);
  DSGCN_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
