// The library's small reductions: column sums of partial-row buffers (every kernel family writes one partial row per
// workgroup and leaves the sum to these: deterministic, fp64 accumulation, no float atomics) and train-mode BatchNorm's
// two micro-reductions — batch statistics -> deferred affine (finalize), a consumer's partial rows -> backward
// coefficients (coef).  Replaces nn.BatchNorm2d's statistics / backward reductions in the reference
// (pyskl/models/gcns/utils/gcn.py:2165-2169,2215, tcn.py:389-404).  The block bodies of the BatchNorm jobs live in
// bn_jobs.h: the kernels that HOST jobs as extra workgroups (K-B, the blocked weight gradient) run the same code.
#include "common.h"
#include "bn_jobs.h"

namespace {

// Column sums of a row-major (R, C) fp32 matrix -> out (C), accumulated in fp64 (partial-buffer reductions).
struct ColJob { const float* src; float* out; int R, C, inner, nblk; };

// 16-byte form: a thread owns 4 consecutive columns, a block 128 columns x 32 row slices, so every row visit of a wave is
// two 512-B segments instead of two 128-B ones (the big inputs are the weight-gradient partials: 10-30 MB each, ~0.8 GB
// per DS-STGCN step — these sums are bandwidth-bound, not launch-bound).  C % 4 == 0, rows 16-byte aligned, inner == 1.
__host__ __device__ inline bool colsum_wide(int C, int inner, const float* src) {
  return (C & 3) == 0 && inner == 1 && C >= 128 && ((size_t)src & 15) == 0;
}
__host__ __device__ inline int colsum_blocks(int C, int inner, const float* src) {
  return colsum_wide(C, inner, src) ? (C + 127) / 128 : (C + 31) / 32;
}

__device__ __forceinline__ void colsum_body4(const ColJob& j, int bid, double (*red)[32]) {
  const int cl = threadIdx.x & 31, slice = threadIdx.x >> 5;
  const int c = bid * 128 + 4 * cl;
  const int R = j.R, C = j.C;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  if (c < C) {
    for (int r0 = slice; r0 < R; r0 += 32 * 4) {
      f32x4 v[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int r = r0 + 32 * q;
        v[q] = r < R ? *reinterpret_cast<const f32x4*>(j.src + (size_t)r * C + c) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) { s0 += (double)v[q].x; s1 += (double)v[q].y; s2 += (double)v[q].z; s3 += (double)v[q].w; }
    }
  }
  // four passes through the [32][32] staging array, one per column of the quad
  double acc[4] = {s0, s1, s2, s3};
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    __syncthreads();
    red[slice][cl] = acc[e];
    __syncthreads();
    if (slice == 0 && c < C) {
      double t = 0.0;
#pragma unroll
      for (int i = 0; i < 32; ++i) t += red[i][cl];
      j.out[c + e] = (float)t;
    }
  }
}

__device__ __forceinline__ void colsum_body(const ColJob& j, int bid) {
  __shared__ double red[32][32];
  if (colsum_wide(j.C, j.inner, j.src)) { colsum_body4(j, bid, red); return; }
  const int cl = threadIdx.x & 31, slice = threadIdx.x >> 5;
  const int c = bid * 32 + cl;
  const int R = j.R, C = j.C;
  double s = 0.0;
  if (c < C) {
    for (int r0 = slice; r0 < R; r0 += 32 * 8) {
      float v[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int r = r0 + 32 * q;
        v[q] = r < R ? j.src[(size_t)r * C + c] : 0.f;
      }
#pragma unroll
      for (int q = 0; q < 8; ++q) s += (double)v[q];
    }
  }
  red[slice][cl] = s;
  __syncthreads();
  if (slice == 0 && c < C) {
#pragma unroll
    for (int i = 1; i < 32; ++i) s += red[i][cl];
    // inner > 1: columns are (C/inner, inner) pairs and leave transposed, out (inner, C/inner), so that each of the
    // `inner` reductions is a contiguous vector for its consumer
    j.out[j.inner > 1 ? (c % j.inner) * (C / j.inner) + c / j.inner : c] = (float)s;
  }
}

// up to two independent reductions in one launch (the weight-gradient and the input-affine partials of one conv)
__global__ __launch_bounds__(1024) void k_colsum(ColJob a, ColJob b) {
  if ((int)blockIdx.x < a.nblk) colsum_body(a, blockIdx.x);
  else colsum_body(b, blockIdx.x - a.nblk);
}

// any number of independent reductions in one launch: the partial rows of parameter gradients (weights, biases, A,
// alpha / beta, add_coeff) feed nothing but the optimizer, so their ~55 column sums per DS-STGCN step are queued during
// the backward and finished by ONE launch before the gradients are packed.  table: njobs x {src, out, (R, C) packed,
// first block} as 64-bit words (device memory), blocks of a job are contiguous in the grid.
__global__ __launch_bounds__(1024) void k_colsum_multi(const long* __restrict__ table, int njobs) {
  // binary search of the job that owns this block (first-block column is ascending)
  int lo = 0, hi = njobs - 1;
  const int b = blockIdx.x;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if ((int)table[4 * mid + 3] <= b) lo = mid; else hi = mid - 1;
  }
  ColJob j;
  j.src = reinterpret_cast<const float*>(table[4 * lo]);
  j.out = reinterpret_cast<float*>(table[4 * lo + 1]);
  j.R = (int)(table[4 * lo + 2] >> 32);
  j.C = (int)(table[4 * lo + 2] & 0xffffffffL);
  j.inner = 1;
  j.nblk = 0;
  colsum_body(j, b - (int)table[4 * lo + 3]);
}

// the same with the table in the kernel arguments (<= CM_MAXJOBS jobs per launch): no table upload in front of the launch,
// the job lookup runs on scalar loads
constexpr int CM_MAXJOBS = 112;
struct ColTable {
  long w[4 * CM_MAXJOBS];
  int njobs;
};

__global__ __launch_bounds__(1024) void k_colsum_multi_arg(ColTable t) {
  int lo = 0, hi = t.njobs - 1;
  const int b = blockIdx.x;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if ((int)t.w[4 * mid + 3] <= b) lo = mid; else hi = mid - 1;
  }
  ColJob j;
  j.src = reinterpret_cast<const float*>(t.w[4 * lo]);
  j.out = reinterpret_cast<float*>(t.w[4 * lo + 1]);
  j.R = (int)(t.w[4 * lo + 2] >> 32);
  j.C = (int)(t.w[4 * lo + 2] & 0xffffffffL);
  j.inner = 1;
  j.nblk = 0;
  colsum_body(j, b - (int)t.w[4 * lo + 3]);
}

// Batch statistics -> BN affine.  partial [nblk][C][2] (fp32 block sums) reduced in fp64: one 256-thread workgroup
// per 32 channels (8 row-slices x 32 channels, coalesced 256-B rows), then a cross-slice LDS reduction.
//   mean, var (biased) saved for backward; scale = gamma*rsqrt(var+eps); shift = beta - mean*scale.
// gamma/beta NULL -> identity affine parameters; channels >= c_affine get the identity affine (1, 0).
__global__ __launch_bounds__(1024) void k_bn_finalize(const float* __restrict__ partial, int nblk, int C, double count,
                                                     const float* __restrict__ gamma, const float* __restrict__ beta,
                                                     float eps, float* __restrict__ mean_out,
                                                     float* __restrict__ var_out, float* __restrict__ scale_out,
                                                     float* __restrict__ shift_out, int c_affine) {
  // 8 channels x 128 row slices per block: the kernel is a latency chain over the partial rows (up to ~1800 of them),
  // so the rows are spread over many threads and C/8 blocks rather than walked by 32 slices in C/32 blocks (bn_jobs.h)
  __shared__ double red[16][8][2];
  const BnFinJob J = {partial, gamma, beta, mean_out, var_out, scale_out, shift_out, count, eps, nblk, C, c_affine};
  bn_finalize_block(J, blockIdx.x, red);
}

// several finalize / coefficient jobs in one launch (bn_jobs.h): blocks = the jobs' blocks back to back
__global__ __launch_bounds__(1024) void k_bn_finalize_multi(BnFinTable t) {
  __shared__ double red[16][8][2];
  bnj_dispatch(t, blockIdx.x, [&](const BnFinJob& J, int b) { bn_finalize_block(J, b, red); });
}

__global__ __launch_bounds__(1024) void k_bn_coef_rows_multi(BnCoefTable t) {
  __shared__ double red[16][8][2];
  bnj_dispatch(t, blockIdx.x, [&](const BnCoefJob& J, int b) { bn_coef_rows_block(J, b, red); });
}

// BN backward coefficients of a conv whose batch statistics feed a deferred affine (scale, shift):
//   d gamma = r (g_scale - mean g_shift), d beta = g_shift, A0 = dmean/M - 2 dvar mean/M, B0 = 2 dvar/M
//   with dmean = -g_shift*gamma*r, dvar = -0.5 r^3 gamma (g_scale - mean g_shift).
__global__ __launch_bounds__(64) void k_bn_bwd_coef(const float* __restrict__ g_scale,
                                                    const float* __restrict__ g_shift,
                                                    const float* __restrict__ mean, const float* __restrict__ var,
                                                    const float* __restrict__ gamma, float eps, double count, int C,
                                                    int c_affine, float* __restrict__ dgamma,
                                                    float* __restrict__ dbeta, float* __restrict__ A0,
                                                    float* __restrict__ B0) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= C) return;
  if (c >= c_affine) { dgamma[c] = 0.f; dbeta[c] = 0.f; A0[c] = 0.f; B0[c] = 0.f; return; }
  const double gs = g_scale ? (double)g_scale[c] : 0.0, gh = g_shift ? (double)g_shift[c] : 0.0;
  const double mu = mean[c], r = 1.0 / sqrt((double)var[c] + (double)eps);
  const double g = gamma ? (double)gamma[c] : 1.0;
  const double t = gs - mu * gh;
  dgamma[c] = (float)(r * t);
  dbeta[c] = (float)gh;
  const double dmean = -gh * g * r;
  const double dvar = -0.5 * r * r * r * g * t;
  A0[c] = (float)((dmean - 2.0 * dvar * mu) / count);
  B0[c] = (float)(2.0 * dvar / count);
}

// The same coefficients straight from a consumer's partial rows: g_scale[c] = sum_r part[r][c][i_ds], g_shift[c] = sum_r
// part[r][c][i_dh] (fp64, rows in order), optionally ADDED to what another consumer of the same BatchNorm already wrote —
// the coefficients are linear in (g_scale, g_shift).  One launch instead of a column sum + k_bn_bwd_coef per consumer.
// Block = 8 channels x 128 row slices (as k_bn_finalize: the launch is a latency chain over up to ~1600 partial rows, so the
// rows are spread over many threads and C / 8 blocks: 6.6 -> 4.x us per launch, 55 launches per DS-STGCN step).
__global__ __launch_bounds__(1024) void k_bn_coef_rows(const float* __restrict__ part, int R, int C, int k, int ids, int idh,
                                                       const float* __restrict__ mean, const float* __restrict__ var,
                                                       const float* __restrict__ gamma, float eps, double count,
                                                       int c_affine, float* __restrict__ coef, int accumulate) {
  __shared__ double red[16][8][2];
  const BnCoefJob J = {part, mean, var, gamma, coef, count, eps, R, C, k, ids, idh, c_affine, accumulate};
  bn_coef_rows_block(J, blockIdx.x, red);
}

}  // namespace

int bnj_coef_launch(const BnCoefTable& t, hipStream_t st) {
  hipLaunchKernelGGL(k_bn_coef_rows_multi, dim3((unsigned)bnj_total_blocks(t)), dim3(BNJ_NT), 0, st, t);
  DSGCN_LAUNCH_CHECK();
  return 0;
}

extern "C" {

// out[c] = sum_r src[r, c]  (fp64 accumulation).
int dsgcn_colsum(const float* src, int R, int C, float* out, void* stream) {
  if (!src || !out || R <= 0 || C <= 0) return DSGCN_EINVAL;
  ColJob a{src, out, R, C, 1, colsum_blocks(C, 1, src)}, b{nullptr, nullptr, 0, 0, 1, 0};
  hipLaunchKernelGGL(k_colsum, dim3((unsigned)a.nblk), dim3(1024), 0, (hipStream_t)stream, a, b);
  DSGCN_LAUNCH_CHECK();
  return 0;
}

// Same, with the result transposed: src (R, C/inner, inner) -> out (inner, C/inner).
int dsgcn_colsum_t(const float* src, int R, int C, int inner, float* out, void* stream) {
  if (!src || !out || R <= 0 || C <= 0 || inner <= 0 || C % inner) return DSGCN_EINVAL;
  ColJob a{src, out, R, C, inner, (C + 31) / 32}, b{nullptr, nullptr, 0, 0, 1, 0};
  hipLaunchKernelGGL(k_colsum, dim3((unsigned)a.nblk), dim3(1024), 0, (hipStream_t)stream, a, b);
  DSGCN_LAUNCH_CHECK();
  return 0;
}

// Two reductions (as dsgcn_colsum_t each; inner = 1 for the plain form) in one launch.
int dsgcn_colsum2(const float* src_a, int Ra, int Ca, int inner_a, float* out_a, const float* src_b, int Rb, int Cb,
                  int inner_b, float* out_b, void* stream) {
  if (!src_a || !out_a || !src_b || !out_b || Ra <= 0 || Ca <= 0 || Rb <= 0 || Cb <= 0 || inner_a <= 0 ||
      inner_b <= 0 || Ca % inner_a || Cb % inner_b)
    return DSGCN_EINVAL;
  ColJob a{src_a, out_a, Ra, Ca, inner_a, colsum_blocks(Ca, inner_a, src_a)}, b{src_b, out_b, Rb, Cb, inner_b, colsum_blocks(Cb, inner_b, src_b)};
  hipLaunchKernelGGL(k_colsum, dim3((unsigned)(a.nblk + b.nblk)), dim3(1024), 0, (hipStream_t)stream, a, b);
  DSGCN_LAUNCH_CHECK();
  return 0;
}

// blocks a job of C columns takes in dsgcn_colsum_multi's grid (the caller lays the jobs' first blocks out with it)
int dsgcn_colsum_blocks(const float* src, int C) { return colsum_blocks(C, 1, src); }

// table (device, njobs x 4 int64): {src pointer, out pointer, (R << 32) | C, first block}; nblocks = sum of dsgcn_colsum_blocks.
int dsgcn_colsum_multi(const long* table, int njobs, int nblocks, void* stream) {
  if (!table || njobs <= 0 || nblocks <= 0) return DSGCN_EINVAL;
  hipLaunchKernelGGL(k_colsum_multi, dim3((unsigned)nblocks), dim3(1024), 0, (hipStream_t)stream, table, njobs);
  DSGCN_LAUNCH_CHECK();
  return 0;
}

// The same from a HOST table (njobs x 4 int64, layout as above): the jobs ride in the kernel arguments, CM_MAXJOBS per
// launch (first-block columns are rebased per launch).
int dsgcn_colsum_multi_host(const long* table, int njobs, void* stream) {
  if (!table || njobs <= 0) return DSGCN_EINVAL;
  for (int j0 = 0; j0 < njobs; j0 += CM_MAXJOBS) {
    ColTable t;
    t.njobs = njobs - j0 < CM_MAXJOBS ? njobs - j0 : CM_MAXJOBS;
    const long base = table[4 * j0 + 3];
    for (int j = 0; j < t.njobs; ++j) {
      for (int q = 0; q < 3; ++q) t.w[4 * j + q] = table[4 * (j0 + j) + q];
      t.w[4 * j + 3] = table[4 * (j0 + j) + 3] - base;
    }
    const int jl = j0 + t.njobs - 1;
    const float* lsrc = reinterpret_cast<const float*>(table[4 * jl]);
    const long end = table[4 * jl + 3] + colsum_blocks((int)(table[4 * jl + 2] & 0xffffffffL), 1, lsrc);
    hipLaunchKernelGGL(k_colsum_multi_arg, dim3((unsigned)(end - base)), dim3(1024), 0, (hipStream_t)stream, t);
    DSGCN_LAUNCH_CHECK();
  }
  return 0;
}

int dsgcn_bn_finalize(const float* partial, int nblk, int C, double count, const float* gamma, const float* beta,
                      float eps, float* mean_out, float* var_out, float* scale_out, float* shift_out, int c_affine,
                      void* stream) {
  if (!partial || !mean_out || !var_out || !scale_out || !shift_out || nblk <= 0 || C <= 0) return DSGCN_EINVAL;
  hipLaunchKernelGGL(k_bn_finalize, dim3((unsigned)((C + 7) / 8)), dim3(1024), 0, (hipStream_t)stream, partial, nblk,
                     C, count, gamma, beta, eps, mean_out, var_out, scale_out, shift_out, c_affine);
  DSGCN_LAUNCH_CHECK();
  return 0;
}

// njobs <= 4 finalize jobs (include/dsgcn.h: dsgcn_bn_fin_job, the arguments of dsgcn_bn_finalize as a struct) in ONE
// launch — BatchNorms whose producers are independent of one another and both done (gcn.py:2165-2169 `post` + `down`).
int dsgcn_bn_finalize_multi(const dsgcn_bn_fin_job* jobs, int njobs, void* stream) {
  if (!jobs || njobs <= 0 || njobs > BNJ_MAX) return DSGCN_EINVAL;
  BnFinTable t = {};
  t.n = njobs;
  for (int i = 0; i < njobs; ++i) {
    const dsgcn_bn_fin_job& q = jobs[i];
    t.j[i] = BnFinJob{q.partial, q.gamma, q.beta, q.mean, q.var, q.scale, q.shift, q.count, q.eps, q.nblk, q.C, q.c_affine};
  }
  if (!bnj_fin_ok(t)) return DSGCN_EINVAL;
  hipLaunchKernelGGL(k_bn_finalize_multi, dim3((unsigned)bnj_total_blocks(t)), dim3(BNJ_NT), 0, (hipStream_t)stream, t);
  DSGCN_LAUNCH_CHECK();
  return 0;
}

int dsgcn_bn_bwd_coef(const float* g_scale, const float* g_shift, const float* mean, const float* var,
                      const float* gamma, float eps, double count, int C, int c_affine, float* dgamma, float* dbeta,
                      float* A0, float* B0, void* stream) {
  if (!mean || !var || !dgamma || !dbeta || !A0 || !B0 || C <= 0) return DSGCN_EINVAL;
  hipLaunchKernelGGL(k_bn_bwd_coef, dim3((unsigned)((C + 63) / 64)), dim3(64), 0, (hipStream_t)stream, g_scale,
                     g_shift, mean, var, gamma, eps, count, C, c_affine, dgamma, dbeta, A0, B0);
  DSGCN_LAUNCH_CHECK();
  return 0;
}

// coef (4, C) = [d gamma | d beta | A0 | B0] from partial rows part (R, C, k): column i_ds holds a consumer's partial
// sums of d scale, column i_dh of d shift.  accumulate != 0: added to the coefficients already in coef (a second consumer
// of the same deferred BatchNorm).
int dsgcn_bn_coef_rows(const float* part, int R, int C, int k, int i_ds, int i_dh, const float* mean, const float* var,
                       const float* gamma, float eps, double count, int c_affine, float* coef, int accumulate,
                       void* stream) {
  if (!part || !mean || !var || !coef || R <= 0 || C <= 0 || k <= 0 || i_ds < 0 || i_ds >= k || i_dh < 0 || i_dh >= k)
    return DSGCN_EINVAL;
  hipLaunchKernelGGL(k_bn_coef_rows, dim3((unsigned)((C + 7) / 8)), dim3(1024), 0, (hipStream_t)stream, part, R, C, k, i_ds,
                     i_dh, mean, var, gamma, eps, count, c_affine, coef, accumulate);
  DSGCN_LAUNCH_CHECK();
  return 0;
}

// njobs <= 4 coefficient jobs (dsgcn_bn_coef_job = the arguments of dsgcn_bn_coef_rows) in one launch.
int dsgcn_bn_coef_rows_multi(const dsgcn_bn_coef_job* jobs, int njobs, void* stream) {
  if (!jobs || njobs <= 0 || njobs > BNJ_MAX) return DSGCN_EINVAL;
  BnCoefTable t = {};
  t.n = njobs;
  for (int i = 0; i < njobs; ++i) {
    const dsgcn_bn_coef_job& q = jobs[i];
    t.j[i] = BnCoefJob{q.part, q.mean, q.var, q.gamma, q.coef, q.count, q.eps, q.R, q.C, q.k, q.i_ds, q.i_dh, q.c_affine,
                       q.accumulate};
  }
  if (!bnj_coef_ok(t)) return DSGCN_EINVAL;
  return bnj_coef_launch(t, (hipStream_t)stream);
}

}  // extern "C"
