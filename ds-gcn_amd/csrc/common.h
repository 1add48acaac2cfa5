// Shared device helpers for the DS-GCN HIP kernels (gfx950 / CDNA4 only: wave64, MFMA f32).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// The C ABI: every source reaches this header, so each extern "C" definition is compiled against its prototype (a
// parameter list that drifts from the header is a compile error), and the error codes and job records have one copy.
#include "dsgcn.h"
#ifdef DSGCN_LAB
#include "dsgcn_lab.h"
#endif

#define DSGCN_WAVE 64

#define DSGCN_LAUNCH_CHECK()                      \
  do {                                            \
    hipError_t e__ = hipGetLastError();           \
    if (e__ != hipSuccess) return (int)e__;       \
  } while (0)

// Matmul precision level (include/dsgcn.h: dsgcn_set_matmul_precision): 0 = highest (six bf16 products per fp32 product),
// 1 = high (three).  One atomic in version.hip, read by the HOST launch code only — never by a kernel.
__attribute__((visibility("hidden"))) int dsgcn_precision_level();

typedef float f32x2v __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x2v __attribute__((ext_vector_type(2)));
typedef unsigned u32x4v __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// Sum / maximum over a 256-thread workgroup (four waves), the same bits in every thread.  red: >= 4 floats of LDS.
__device__ __forceinline__ float block_sum(float v, float* red, int tid) {
  v = wave_sum(v);
  __syncthreads();
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

__device__ __forceinline__ float block_max(float v, float* red, int tid) {
  v = wave_max(v);
  __syncthreads();
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// relu?(x*s+h)
__device__ __forceinline__ float affine_act(float x, float s, float h, int relu) {
  float v = fmaf(x, s, h);
  return relu ? fmaxf(v, 0.f) : v;
}

// Single-wave workgroups: LDS traffic of one wave is executed in issue order, so cross-lane exchange through
// LDS needs no s_barrier — only "all my DS ops are done" and a compiler fence.  Unlike __syncthreads() this does
// NOT emit s_waitcnt vmcnt(0), so global prefetch loads stay in flight across it.
__device__ __forceinline__ void wave_lds_sync() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}

// The workgroup's form of the same: "all my DS ops are done", then the raw s_barrier.  Again no s_waitcnt vmcnt(0): the
// global loads a wave has in flight stay in flight across the barrier.
__device__ __forceinline__ void block_lds_sync() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
}

// MFMA C/D row of accumulator register r for this lane (32x32 tile): (r&3) + 8*(r>>2) + 4*(lane>>5)
__device__ __forceinline__ int mfma_row32(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

// ---- raw buffer loads -----------------------------------------------------------------------------------------------
// A buffer resource over `bytes` bytes at p, stride 0 (raw: the offsets are bytes).  The last descriptor word (the literal below)
// selects DATA_FORMAT = 4 (one 32-bit element; bits 15-18 of the word) and leaves every other field zero: no swizzle, no
// thread-id addressing, and with stride 0 the raw range check (offset >= num_records).  A load past `bytes` returns 0 and
// a store there is dropped: the kernels use that instead of per-lane predication.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buf_rsrc(const void* p, size_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), (short)0, (int)bytes, 0x00020000);
}

// A vector offset that is out of range for every resource (num_records is an int) and stays so, without wrapping, under
// the 16-byte-aligned row offsets the kernels add to it.
constexpr int BUF_OOB = 0x7ffffff0;

// N consecutive floats at byte offset voff (per lane: VGPR) + soff (wave-uniform: SGPR operand); N = 1, 2, 4.
template <int N> struct buf_vec;
template <> struct buf_vec<1> { typedef float T; };
template <> struct buf_vec<2> { typedef f32x2v T; };
template <> struct buf_vec<4> { typedef f32x4 T; };

template <int N>
__device__ __forceinline__ typename buf_vec<N>::T buf_load(__amdgpu_buffer_rsrc_t r, int voff, int soff = 0) {
  if constexpr (N == 4) return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0));
  else if constexpr (N == 2) return __builtin_bit_cast(f32x2v, __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, 0));
  else return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0));
}

// Vector offset of a per-row access: base + rowoff (rowoff = row * plane bytes), or an out-of-range offset for an invalid
// row / position (unsigned sum: no wrap below 2^32).  The row depends on the lane's half, so it must NOT go into the scalar
// offset: hipcc then wraps every access in a readfirstlane loop that runs once per distinct value (two passes with half the
// lanes each; 35-195 such loops per kernel in the disassembly of the first version).
__device__ __forceinline__ int buf_rowoff(bool ok, int base, int rowoff) {
  return (int)((unsigned)(ok ? base : BUF_OOB) + (unsigned)rowoff);
}

// Sum of half of row l31 of a wave's [32][36] LDS tile (lane (half, l31); the caller adds the two halves).
template <typename ACC>
__device__ __forceinline__ ACC tile36_rowsum(const float* Tw, int half, int l31) {
  const f32x4* rowp = reinterpret_cast<const f32x4*>(Tw + l31 * 36 + half * 16);
  ACC s = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const f32x4 v = rowp[q];
    s += ((ACC)v.x + (ACC)v.y) + ((ACC)v.z + (ACC)v.w);
  }
  return s;
}

// t = e / V, v = e % V for 0 <= e < 2^22 with invV = 1.f / V (float reciprocal + one fix-up step: exact)
__device__ __forceinline__ void divmod_small(int e, int V, float invV, int& t, int& v) {
  t = (int)((float)e * invV);
  v = e - t * V;
  if (v < 0) { v += V; --t; }
  else if (v >= V) { v -= V; ++t; }
}

// One wave copies a 16-B aligned run of L4 float4 from global memory into LDS; the loads of a 512-float4 chunk are all
// issued before the first LDS write (whole (T,V) planes are <= a few KB: the wave keeps the entire plane in flight).
__device__ __forceinline__ void plane_to_lds(const float* __restrict__ src, float* __restrict__ dst, int L4, int lane) {
  const f32x4* __restrict__ s4 = reinterpret_cast<const f32x4*>(src);
  f32x4* __restrict__ d4 = reinterpret_cast<f32x4*>(dst);
  for (int base = 0; base < L4; base += 512) {
    f32x4 r[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int i = base + q * 64 + lane;
      if (i < L4) r[q] = s4[i];
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int i = base + q * 64 + lane;
      if (i < L4) d4[i] = r[q];
    }
  }
}

// ---- three-term bf16 form of the fp32 product (B3) -----------------------------------------------------------------
// An fp32 value is the exact sum of three bf16 terms (8 significand bits each, round-to-nearest residues: x0 = bf16(x),
// x1 = bf16(x - x0), x2 = x - x0 - x1; both subtractions are exact in fp32 and the last residue has at most 6 bits).
// a*b = sum_{i,j} a_i*b_j; the six terms with i + j <= 2 are kept (each exact in fp32, accumulated in the MFMA's fp32
// accumulator), the dropped ones are below 2^-24 |a||b| — the rounding class of the fp32 MFMA it replaces, at 2.7x its
// rate: six v_mfma_f32_32x32x16_bf16 (32 cycles each) per 16 channels against eight v_mfma_f32_32x32x2_f32 (64 cycles).
// Non-finite inputs give NaN where fp32 would keep an infinity (inf - inf in the residue).
//
// Two-term form (matmul precision 'high', opt-in): only x0 and x1 are formed (each cast is off by at most 2^-8 relative,
// so |x - x0 - x1| <= 2^-16 |x|) and the three products with i + j <= 1 are kept: a0*b0 + a0*b1 + a1*b0.  The dropped part
// of a*b is at most 3 * 2^-16 |a||b| (4.6e-5; about 5e-6 of sum |a||b| on random data: between TF32 and fp32) for half the
// MFMAs, two thirds of the split's VALU work and two thirds of the LDS traffic.  The kernels that offer it are second
// instantiations (term count 2) of the bodies of the three-term ones.
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ unsigned b3_pack(float a, float b) {
  return __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2v{a, b}, bf16x2));   // v_cvt_pk_bf16_f32: lo = a, hi = b
}

// packed bf16 pairs p[s] = (lo: term s of a, hi: term s of b)
__device__ __forceinline__ void b3_split(float a, float b, unsigned& p0, unsigned& p1, unsigned& p2) {
  p0 = b3_pack(a, b);
  a -= __builtin_bit_cast(float, p0 << 16);
  b -= __builtin_bit_cast(float, p0 & 0xffff0000u);
  p1 = b3_pack(a, b);
  a -= __builtin_bit_cast(float, p1 << 16);
  b -= __builtin_bit_cast(float, p1 & 0xffff0000u);
  p2 = b3_pack(a, b);
}

// the first two terms only (the two-term form above)
__device__ __forceinline__ void b2_split(float a, float b, unsigned& p0, unsigned& p1) {
  p0 = b3_pack(a, b);
  a -= __builtin_bit_cast(float, p0 << 16);
  b -= __builtin_bit_cast(float, p0 & 0xffff0000u);
  p1 = b3_pack(a, b);
}

// NT = 3: the three terms (p2 written); NT = 2: the first two (p2 untouched)
template <int NT>
__device__ __forceinline__ void bn_split(float a, float b, unsigned& p0, unsigned& p1, unsigned& p2) {
  if constexpr (NT == 3) b3_split(a, b, p0, p1, p2);
  else b2_split(a, b, p0, p1);
}

// the products of one 16-deep k-step on the terms' fragments: six (NT = 3: i + j <= 2) or three (NT = 2: i + j <= 1),
// smallest first
template <int NT>
__device__ __forceinline__ f32x16 bn_products(const bf16x8 (&a)[NT], const bf16x8 (&b)[NT], f32x16 c) {
  if constexpr (NT == 3) {
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[2], b[0], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[1], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[2], c, 0, 0, 0);
  }
  c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[0], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[1], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[0], c, 0, 0, 0);
  return c;
}
