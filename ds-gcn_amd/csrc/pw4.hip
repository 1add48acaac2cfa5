// K-C, wide-load form ("pw4"): the 1x1 channel mix with 16-byte-per-lane operand loads.
//
// Same math as pwconv.hip (which documents the reference lines this replaces: gcn.py:2165-2169,2209-2215,2363-2365,
// tcn.py:379-404,422,427): out[n,m,pos] = sum_k A[m,k] * B'[n,k,pos], B' = the "virtual" operand (deferred BatchNorm
// affine / ReLU / second stream applied while loading).  Forward: A = W (m = co, k = ci), B = the layer input.
// Data gradient: A = W^T (m = ci, k = co), B' = dz_eff = gz + A0[co] + B0[co]*z, epilogue = ReLU mask / affine of the
// forward's virtual input + the per-channel sums for d scale / d shift.
//
// Why this form (profiles/r02/kc_counters_before.csv): the first kernel read the B operand with 4-byte-per-lane loads
// (two 128-B segments per wave instruction, 64 different channel rows per wave) and reached 2.2 TB/s with the MFMA pipe
// 23 % busy — HBM saw 128-B visits scattered over rows 6.4 KB apart.  Here a lane owns NQ = 4 (or 2) CONSECUTIVE
// positions of one channel: one buffer_load_dwordx4 per k-step brings two 512-B row segments, and register q of the
// loaded vector is directly the B fragment of position sub-tile q (sub-tile q = positions {NQ*j + q}: the position
// order inside the wave's 32*NQ-position tile is a permutation the store undoes for free, because the four results
// of a lane are again 16 consecutive bytes).  Per k-step a wave issues 1 VMEM load, MT LDS reads and MT*NQ MFMAs
// (v_mfma_f32_32x32x2_f32), with PD k-steps of operand prefetch in flight and no barrier inside the K loop (the whole
// weight block of the workgroup's 32*MT output channels sits in LDS).  Sample base folded into the buffer resource:
// offsets stay 32-bit for any batch size and channels past K read as zero through the bounds check.
#include "pw4_block.h"

namespace {

// The hosts: what the shipped DS-STGCN step runs for the `pre` conv.  Forward: the plain-operand narrow conv (blocks 1-7)
// and its GEMM form (blocks 8-10); data gradient (dz_eff with the batch-statistics terms: MODE 2): the narrow form with two
// row tiles per wave (blocks 6-7) and both GEMM forms (blocks 8-10).  The guest runs the host's direction (EPI).  The
// one-pass backward of blocks 1-5: bwd64.hip.
template <int MT, int NQ, int MODE, int PD, int EPI, bool KSP>
constexpr bool p4_hosts = !KSP && NQ == 4 && PD == 8 && ((MT == 1 && MODE == 0 && EPI == 0) || (MT == 2 && MODE == 2 && EPI == 1));
template <int MODE, int EPI, int MT>
constexpr bool pwg3_hosts = (MODE == 0 && EPI == 0 && MT == 1) || (MODE == 2 && EPI == 1);

template <int MT, int NQ, int MODE, int PD, int EPI, bool KSP = false>
__global__ __launch_bounds__(P4_NT, (MT * NQ >= 6 ? 2 : (MT * NQ >= 4 ? 3 : 4))) void k_pw4(
    Pw4Args a_, P4GuestArg<p4_hosts<MT, NQ, MODE, PD, EPI, KSP>> guest) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  int bid = blockIdx.x;
  if constexpr (p4_hosts<MT, NQ, MODE, PD, EPI, KSP>) {
    if (bid < guest.nblk) {                        // (blocks past the guest's own grid return inside)
      p4_block<1, 2, 0, 16, EPI>(guest.a, bid, lds);
      return;
    }
    bid -= guest.nblk;
  }
  Pw4Args a = a_;
  if (a_.ngroup > 1) {                             // grouped launch: this workgroup's conv
    const Pw4Args::Grp& q = a_.g[blockIdx.y];
    a.b1 = q.b1; a.ps1 = q.ps1; a.ph1 = q.ph1; a.w = q.w; a.out = q.out;
    a.ex1 = q.ex1; a.es1 = q.es1; a.eh1 = q.eh1; a.ipart = q.ipart;
  }
  p4_block<MT, NQ, MODE, PD, EPI, KSP>(a, bid, lds);
}


// ---- K-C, GEMM form with three-term bf16 products ("pwg") ----------------------------------------------------------
// For convs wide on both sides (the fp32 MFMA form is bound by the matrix pipe: 85 TF of 157 at 256 -> 256) the product
// runs as six v_mfma_f32_32x32x16_bf16 per 16 channels on the exact three-way bf16 split of both operands (common.h).
// The split costs ~5 VALU operations per value, so it must not be repeated per output-row block the way k_pw4 re-reads
// its B operand: here a workgroup owns 128 output rows x 128 positions, its four waves hold 32 rows each of the SAME
// position tile, and both operand tiles of a 32-channel chunk are split once by the thread that loaded them and shared
// through LDS — rows of 32 bf16 (+16 B pad: conflict-free 16-byte fragment reads) per term, k contiguous.  The loader
// thread holds a 4 x 4 register block (4 channels x its lane's 4 positions; for W^T 4 k x 4 rows), so the k-contiguous
// image is written with 8-byte stores and no transposed reads are needed; position sub-tile q is again {4j + q}: the
// accumulators have k_pw4's layout and the epilogue is shared (p4_epilogue, OWNROWS).
constexpr int PG_KC = 32, PG_RB = PG_KC * 2 + 16, PG_T = 128, PG_TAM = 144;

template <int MODE, int EPI>
__global__ __launch_bounds__(P4_NT, 2) void k_pwg(Pw4Args a) {
  typedef f32x4 vq;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  char* Ab = reinterpret_cast<char*>(lds);                               // [3][128 rows][RB]
  // W^T arrives four consecutive ROWS per loader thread: written in row order the 8-byte stores of a wave would sit 320 B
  // apart (16-way bank conflicts: profiles/r02 counters); row 4a + rr is therefore kept at LDS row 36*rr + a (lanes 80 B
  // apart on the store side, and the 16-byte fragment reads of a wave's 32 rows — 4 row groups x 8 — stay conflict-free)
  constexpr int TA = EPI == 1 ? PG_TAM : PG_T;                           // A rows per term
  char* Bb = Ab + 3 * TA * PG_RB;                                        // [3][128 position slots][RB]
  f32x4* Ps = reinterpret_cast<f32x4*>(Bb + 3 * PG_T * PG_RB);           // [Kpad] (s1, h1, s2, h2)
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = lane >> 5, l31 = lane & 31;
  const int ngrp = a.WT;
  const int id = blockIdx.x, xcd = id & 7, slot = id >> 3;
  const int cz = slot % a.cc;
  const int grp = (slot / a.cc) * 8 + xcd;
  if (grp >= ngrp) return;
  const int mBase0 = cz * PG_T, mBase = mBase0 + 32 * wave;
  const int K = a.K, M = a.M, L = a.L, Kpad = a.Kpad;
  const int Lq = a.Lq;                             // (ragged planes: see k_pw4)
  const int g0 = grp * 128;
  const int n = g0 / Lq;
  int pos = g0 - n * Lq + l31 * 4;
  int ds = 0;
  while (pos >= Lq) { pos -= Lq; ++ds; }
  const bool pok = n + ds < a.n;
  int skip = 0;
  if (L - pos < 4) { skip = 4 - (L - pos); pos = L - 4; }
  const int L4 = L * 4;
  const int nrem = a.n - n < a.span ? a.n - n : a.span;
  const __amdgpu_buffer_rsrc_t r1 = buf_rsrc(a.b1 + (size_t)n * K * L, nrem * K * L4);
  const __amdgpu_buffer_rsrc_t r2 = buf_rsrc((MODE == 2 ? a.b2 : a.b1) + (size_t)n * K * L, MODE == 2 ? nrem * K * L4 : 0);
  // loader roles.  B: channels 4*cg .. 4*cg+3 of the chunk (cg = tid / 32) at the lane's own position quad.
  const int cg = tid >> 5;
  const int voffB = pok ? ds * K * L4 + pos * 4 : BUF_OOB;
  // A, k contiguous in memory (forward): rows (tid / 8) + 32*i, k = 4*(tid % 8) ..+3;  m contiguous (data gradient: W^T):
  // k = 4*(tid / 32) + e, rows 4*(tid % 32) ..+3
  constexpr bool mfast = EPI == 1;                 // data gradient: A = W^T, m contiguous in memory
  f32x4 aw[4];
  vq bwA[4], bwB[4], bw2A[MODE == 2 ? 4 : 1], bw2B[MODE == 2 ? 4 : 1];     // two chunks of B in flight (ping-pong sets)
  auto issueB = [&](int ch0, vq (&bw)[4], vq (&bw2)[MODE == 2 ? 4 : 1]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int c = ch0 + 4 * cg + e;                 // per half-wave: the channel goes into the vector offset
      const int vo = c < K ? voffB + c * L4 : BUF_OOB;
      bw[e] = buf_load<4>(r1, vo);
      if constexpr (MODE == 2) bw2[e] = buf_load<4>(r2, vo);
    }
  };
  // weights through a buffer resource too: rows / channels past the matrix are out-of-range offsets (zeros), no branches
  const __amdgpu_buffer_rsrc_t rw = buf_rsrc(a.w, M * K * 4);
  const int offA0 = mfast ? (4 * cg * a.w_ldk + mBase0 + 4 * l31) * 4 : ((mBase0 + (tid >> 3)) * a.w_ldm + 4 * (tid & 7)) * 4;
  const int stepE = mfast ? a.w_ldk * 4 : 32 * a.w_ldm * 4;             // between this thread's four loads
  const int stepC = mfast ? a.w_ldk * 4 : 4;                            // per channel of chunk advance
  const int kA = mfast ? 4 * cg : 4 * (tid & 7), mA = mfast ? mBase0 + 4 * l31 : mBase0 + (tid >> 3);
  auto issueA = [&](int ch0) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bool ok = (kA + ch0 + (mfast ? e : 0) < K) & (mA + (mfast ? 0 : 32 * e) < M);
      aw[e] = buf_load<4>(rw, ok ? offA0 + e * stepE + ch0 * stepC : BUF_OOB);
    }
  };
  const float lo = a.relu ? 0.f : -__builtin_inff();
  auto put = [&](char* base, int tstride, float v0, float v1, float v2, float v3) {   // four consecutive k of one row -> 8 B per term
    unsigned p0, p1, p2, q0, q1, q2;
    b3_split(v0, v1, p0, p1, p2);
    b3_split(v2, v3, q0, q1, q2);
    *reinterpret_cast<u32x2v*>(base) = u32x2v{p0, q0};
    *reinterpret_cast<u32x2v*>(base + tstride) = u32x2v{p1, q1};
    *reinterpret_cast<u32x2v*>(base + 2 * tstride) = u32x2v{p2, q2};
  };
  auto commit = [&](int ch0, vq (&bw)[4], vq (&bw2)[MODE == 2 ? 4 : 1]) {
    if (mfast) {
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) put(Ab + (36 * rr + l31) * PG_RB + cg * 8, TA * PG_RB, aw[0][rr], aw[1][rr], aw[2][rr], aw[3][rr]);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) put(Ab + ((tid >> 3) + 32 * e) * PG_RB + (tid & 7) * 8, TA * PG_RB, aw[e].x, aw[e].y, aw[e].z, aw[e].w);
    }
    f32x4 pr[4];
    if (MODE != 0) {
#pragma unroll
      for (int e = 0; e < 4; ++e) pr[e] = Ps[ch0 + 4 * cg + e];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float x = bw[e][q];
        if (MODE != 0) {
          x = fmaf(x, pr[e].x, pr[e].y);
          if constexpr (MODE == 2) x += fmaf(bw2[e][q], pr[e].z, pr[e].w);
          x = fmaxf(x, lo);
        }
        v[e] = x;
      }
      put(Bb + (32 * q + l31) * PG_RB + cg * 8, PG_T * PG_RB, v[0], v[1], v[2], v[3]);
    }
  };

  if (MODE != 0) {                                 // (before the operand loads: its own loads end in a vmcnt(0))
    for (int i = tid; i < Kpad; i += P4_NT) {
      f32x4 p = {0.f, 0.f, 0.f, 0.f};
      if (i < K) {
        p.x = a.ps1 ? a.ps1[i] : 1.f;
        p.y = a.ph1 ? a.ph1[i] : 0.f;
        p.z = a.ps2 ? a.ps2[i] : 1.f;
        p.w = a.ph2 ? a.ph2[i] : 0.f;
      }
      Ps[i] = p;
    }
  }
  __builtin_amdgcn_sched_barrier(0);
  issueA(0);
  issueB(0, bwA, bw2A);
  issueB(PG_KC, bwB, bw2B);
  __builtin_amdgcn_sched_barrier(0);
  f32x16 acc[1][4];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int row = mBase + mfma_row32(i, half);
    const float b0 = (EPI == 0 && a.bias && row < M) ? a.bias[row] : 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[0][q][i] = b0;
  }
  block_lds_sync();                    // Ps visible (raw barrier: the operand loads stay in flight)
  const char* Af = Ab + (mfast ? 36 * (l31 & 3) + 8 * wave + (l31 >> 2) : 32 * wave + l31) * PG_RB + 16 * half;
  const char* Bf = Bb + l31 * PG_RB + 16 * half;
  auto chunk = [&](int ch0, vq (&bw)[4], vq (&bw2)[MODE == 2 ? 4 : 1]) {
    commit(ch0, bw, bw2);
    block_lds_sync();
    __builtin_amdgcn_sched_barrier(0);
    issueA(ch0 + PG_KC);                           // (past K: zeros)
    issueB(ch0 + 2 * PG_KC, bw, bw2);              // this set is free again: two chunks ahead
    __builtin_amdgcn_sched_barrier(0);             // pinned here, in this order: the next commit's vmcnt leaves this set in flight
#pragma unroll
    for (int ks = 0; ks < PG_KC / 16; ++ks) {
      bf16x8 af[3];
#pragma unroll
      for (int t = 0; t < 3; ++t)
        af[t] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4v*>(Af + t * TA * PG_RB + 32 * ks));
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        bf16x8 bf[3];
#pragma unroll
        for (int t = 0; t < 3; ++t)
          bf[t] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4v*>(Bf + (t * PG_T + 32 * q) * PG_RB + 32 * ks));
        f32x16 c = acc[0][q];
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[2], bf[0], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[1], bf[1], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[0], bf[2], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[1], bf[0], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[0], bf[1], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[0], bf[0], c, 0, 0, 0);
        acc[0][q] = c;
      }
    }
    block_lds_sync();                  // raw barrier: the loads in flight stay in flight
  };
  // (pairs in the loop, an odd last chunk outside it: with the second call conditional inside the loop the compiler
  // must allow for a first-call -> first-call path, on which the set just refilled is the next one consumed: vmcnt(0))
  int ch0 = 0;
  for (; ch0 + PG_KC < Kpad; ch0 += 2 * PG_KC) {
    chunk(ch0, bwA, bw2A);
    chunk(ch0 + PG_KC, bwB, bw2B);
  }
  if (ch0 < Kpad) chunk(ch0, bwA, bw2A);
  __syncthreads();                                 // drains the read-ahead loads before LDS is reused
  const P4Tile tile = {wave, half, l31, tid, mBase, n, nrem, ds, pos, grp, true, pok, skip};
  if constexpr (EPI == 1) {
    if (a.ex2) p4_epilogue<1, 4, EPI, true, 4, 4, true>(a, acc, lds, tile);
    else p4_epilogue<1, 4, EPI, true, 4, 4, false>(a, acc, lds, tile);
  } else {
    p4_epilogue<1, 4, EPI, true>(a, acc, lds, tile);
  }
}


// ---- K-C, GEMM form with the weights split ahead of the launch -----------------------------------------------------------
// k_pwg spends as many VALU cycles on the three-way bf16 split as the matrix core spends on the six products (rocprofv3
// counters, profiles/r03: 9.8 M VALU instructions x 4 cycles against 39 M MFMA-busy cycles per 256 -> 256 launch, matrix
// pipe 27 % busy) and half of that split is the WEIGHT tile, the same for every workgroup and every chunk revisit: the
// weights are therefore split once per conv and step (k_wsplit below, the W and the W^T image).  Round 3's consumer of
// that image (k_pwg2: eight waves on one position tile, the weight chunk copied through LDS, two barriers per chunk) is
// gone; k_pwg3 below replaced it (same-box A/B of the step: 13.03 -> 12.55 ms, profiles/r04).
#ifdef DSGCN_LAB
// wall-clock stamps (10 ns) of one workgroup's thread 0 (include/dsgcn_lab.h: dsgcn_pwg2_phases), [63] = count
__device__ long long g_pwg_stamp[64];
__device__ int g_pwg_stamp_block = 0;            // which workgroup stamps (dsgcn_pwg2_phases_block)
#define PWG_STAMP_BLOCK g_pwg_stamp_block
#define PWG_STAMP() do { if (blockIdx.x == PWG_STAMP_BLOCK && threadIdx.x == 0 && nst < 62) g_pwg_stamp[nst++] = wall_clock64(); } while (0)
#else
#define PWG_STAMP() do {} while (0)
#endif

// ---- K-C, GEMM form, third generation ("pwg3"): two independent workgroups per CU, one barrier per chunk ------------
// What the lab stamps of round 3's k_pwg2 showed (profiles/r03/README.md): a workgroup's life is prologue -> 8 x (commit + barrier +
// products + barrier) -> epilogue with all eight waves of the CU in lockstep; the matrix pipe idles through every commit
// and through the HBM-bound epilogue (15 us of 45 in the data gradient), and 400 position tiles on 256 one-workgroup CUs
// make two rounds.  Here:
//   * a workgroup is FOUR waves that own 32*MT rows each (MT = 2: 256 rows) of the same 128-position tile: 8 accumulator
//     tiles per wave, two workgroups resident per CU (2 x 66 KB of LDS, <= 256 registers), so one workgroup's prologue /
//     epilogue / barrier waits run under the other's products — the tiles of a launch fit in one round;
//   * the weight terms never touch LDS: the image is written once per conv in FRAGMENT order (k_wsplit, frag = 1:
//     [term][row tile][k-step][lane][8 bf16], a wave's A fragment is one contiguous 1 KB) and every wave loads its own
//     rows' fragments straight into registers one k-step ahead (k_pwg2 tried this on the row-major image — 64 row
//     segments of 32 B per load — and lost);
//   * the activation chunk (32 channels x 128 positions, three bf16 terms) is double-buffered in LDS: chunk i+1 is split
//     and written while chunk i is multiplied (the split's VALU work sits in the MFMA shadow), ONE barrier per chunk.
// vmcnt is in order, so a wave's wait for its next A fragments also completes the older activation loads: the
// activation prefetch distance is one chunk by construction (a second register set would buy nothing).
constexpr int G3_BBUF = 3 * PG_T * PG_RB;          // one activation buffer: [3 terms][128 position slots][RB]

// The body is templated on the term count NT: 3 = the six products (k_pwg3), 2 = the three products of matmul precision
// 'high' (k_pwg3h: common.h, two-term form).  NT = 2 reads terms 0 and 1 of the SAME weight image and LDS layout (term 2's
// plane / rows are simply not touched): two split steps, two LDS rows and two A fragments per value instead of three.
template <int MODE, int EPI, int MT, int NT>
__device__ __forceinline__ void pwg3_body(const Pw4Args& a, const unsigned short* __restrict__ wfr, int RT, int bid, float* lds) {
  typedef f32x4 vq;
#ifdef DSGCN_LAB
  int nst = 0;
#endif
  PWG_STAMP();
  char* Bb = reinterpret_cast<char*>(lds);                               // [2][3][128 position slots][RB]
  f32x4* Ps = reinterpret_cast<f32x4*>(Bb + 2 * G3_BBUF);                // [Kpad] (s1, h1, s2, h2)
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = lane >> 5, l31 = lane & 31;
  const int ngrp = a.WT;
  const int id = bid, xcd = id & 7, slot = id >> 3;
  const int cz = slot % a.cc;
  const int grp = (slot / a.cc) * 8 + xcd;
  if (grp >= ngrp) return;
  const int mBase0 = cz * (128 * MT), mBase = mBase0 + 32 * MT * wave;
  const int K = a.K, M = a.M, L = a.L, Kpad = a.Kpad;
  const int Lq = a.Lq;                             // (ragged planes: see k_pw4)
  const int g0 = grp * 128;
  const int n = g0 / Lq;
  int pos = g0 - n * Lq + l31 * 4;
  int ds = 0;
  while (pos >= Lq) { pos -= Lq; ++ds; }
  const bool pok = n + ds < a.n;
  int skip = 0;
  if (L - pos < 4) { skip = 4 - (L - pos); pos = L - 4; }
  const int L4 = L * 4;
  const int nrem = a.n - n < a.span ? a.n - n : a.span;
  const __amdgpu_buffer_rsrc_t r1 = buf_rsrc(a.b1 + (size_t)n * K * L, nrem * K * L4);
  const __amdgpu_buffer_rsrc_t r2 = buf_rsrc((MODE == 2 ? a.b2 : a.b1) + (size_t)n * K * L, MODE == 2 ? nrem * K * L4 : 0);
  // B loader: channels 4*cg .. 4*cg+3 of the chunk (cg = tid / 32) at the lane's own position quad
  const int cg = tid >> 5;
  const int voffB = pok ? ds * K * L4 + pos * 4 : BUF_OOB;
  vq bw[4], bw2[MODE == 2 ? 4 : 1];
  auto issueB = [&](int ch0) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int c = ch0 + 4 * cg + e;
      const int vo = c < K ? voffB + c * L4 : BUF_OOB;
      bw[e] = buf_load<4>(r1, vo);
      if constexpr (MODE == 2) bw2[e] = buf_load<4>(r2, vo);
    }
  };
  // A fragments: (term t, row tile m of this wave, k-step ks) = 1 KB at ((t*RT + rt)*KS + ks) KB of the image
  const int KS = Kpad >> 4;
  const __amdgpu_buffer_rsrc_t rw = buf_rsrc(wfr, 3 * RT * KS * 1024);
  // (the fragment's KB index is wave-uniform: it rides in the scalar offset, one vector register addresses all of them)
  const int fragA0 = __builtin_amdgcn_readfirstlane(mBase >> 5);
  u32x4v af0[MT][NT], af1[MT][NT];                 // k-steps of even / odd index
  auto issueA = [&](int ks, u32x4v (&af)[MT][NT]) {
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int t = 0; t < NT; ++t)
        af[m][t] = __builtin_bit_cast(u32x4v, buf_load<4>(rw, lane * 16, ((t * RT + fragA0 + m) * KS + ks) * 1024));
  };
  const float lo = a.relu ? 0.f : -__builtin_inff();
  // the chunk in registers -> the operand values, in place (deferred-BatchNorm affine, second stream, ReLU): done as soon
  // as the loads land, so the affine table's rows and the second stream's registers are dead before the products start
  // (with them alive next to 128 accumulator + 48 fragment registers the two-stream kernels spilled INSIDE the loop, and a
  // scratch reload waits, in order, for every prefetch issued before it)
  auto combine = [&](int ch0) {
    if constexpr (MODE != 0) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const f32x4 pr = Ps[ch0 + 4 * cg + e];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          float x = fmaf(bw[e][q], pr.x, pr.y);
          if constexpr (MODE == 2) x += fmaf(bw2[e][q], pr.z, pr.w);
          bw[e][q] = fmaxf(x, lo);
        }
      }
    }
  };
  // position sub-tile q of the (combined) chunk -> its NT term rows of buffer `dst`
  auto commit_q = [&](char* dst, int q) {
    char* base = dst + (32 * q + l31) * PG_RB + cg * 8;
    unsigned p0, p1, p2, q0, q1, q2;
    bn_split<NT>(bw[0][q], bw[1][q], p0, p1, p2);
    bn_split<NT>(bw[2][q], bw[3][q], q0, q1, q2);
    *reinterpret_cast<u32x2v*>(base) = u32x2v{p0, q0};
    *reinterpret_cast<u32x2v*>(base + PG_T * PG_RB) = u32x2v{p1, q1};
    if constexpr (NT == 3) *reinterpret_cast<u32x2v*>(base + 2 * PG_T * PG_RB) = u32x2v{p2, q2};
  };

  // prologue: the first TWO activation chunks are requested before anything else (the second into a register set that is
  // dead once the loop starts), so the affine table, the bias and chunk 0's split all wait on one memory round trip
  vq bwN[4], bw2N[MODE == 2 ? 4 : 1];
  __builtin_amdgcn_sched_barrier(0);
  issueB(0);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int c = PG_KC + 4 * cg + e;
    const int vo = c < K ? voffB + c * L4 : BUF_OOB;
    bwN[e] = buf_load<4>(r1, vo);
    if constexpr (MODE == 2) bw2N[e] = buf_load<4>(r2, vo);
  }
  __builtin_amdgcn_sched_barrier(0);
  f32x16 acc[MT][4];
  const __amdgpu_buffer_rsrc_t rbias = buf_rsrc(a.bias, (EPI == 0 && a.bias) ? M * 4 : 0);
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row = mBase + 32 * m + mfma_row32(i, half);
      float b0 = 0.f;                              // (rows past M / no bias: the bounds check returns zero, no branches)
      if constexpr (EPI == 0) b0 = buf_load<1>(rbias, row * 4);
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[m][q][i] = b0;
    }
  if (MODE != 0) {
    for (int i = tid; i < Kpad; i += 256) {
      f32x4 p = {0.f, 0.f, 0.f, 0.f};
      if (i < K) {
        p.x = a.ps1 ? a.ps1[i] : 1.f;
        p.y = a.ph1 ? a.ph1[i] : 0.f;
        p.z = a.ps2 ? a.ps2[i] : 1.f;
        p.w = a.ph2 ? a.ph2[i] : 0.f;
      }
      Ps[i] = p;
    }
  }
  __builtin_amdgcn_sched_barrier(0);
  issueA(0, af0);
  __builtin_amdgcn_sched_barrier(0);
  block_lds_sync();                    // Ps visible (raw barrier: the operand loads stay in flight)
  PWG_STAMP();
  combine(0);
#pragma unroll
  for (int q = 0; q < 4; ++q) commit_q(Bb, q);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    bw[e] = bwN[e];
    if constexpr (MODE == 2) bw2[e] = bw2N[e];
  }
  block_lds_sync();
  PWG_STAMP();

  const int fragoff = l31 * PG_RB + 16 * half;
  // one k-step of products on buffer `cur` (ksl = 0 / 1: the chunk's first / second 16 channels); `fill(q)` runs after
  // the products of position sub-tile q (the next chunk's split: VALU + LDS stores in the MFMA shadow)
  auto products = [&](const char* cur, int ksl, u32x4v (&af)[MT][NT], auto&& fill) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      bf16x8 bf[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t)
        bf[t] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4v*>(cur + fragoff + (t * PG_T + 32 * q) * PG_RB + 32 * ksl));
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        bf16x8 am[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) am[t] = __builtin_bit_cast(bf16x8, af[m][t]);
        acc[m][q] = bn_products<NT>(am, bf, acc[m][q]);
      }
      fill(q);
    }
  };
  const int NC = Kpad / PG_KC;
  // ACT = false: a wave whose rows lie past M (M = 96: the fourth wave) only loads and splits
  auto mainloop = [&](auto act) {
    constexpr bool ACT = decltype(act)::value;
    char* cur = Bb;
    char* nxt = Bb + G3_BBUF;
    for (int i = 0; i < NC; ++i) {
      const int ch1 = (i + 1) * PG_KC;             // the chunk committed in this pass (past K: zeros, never multiplied)
      if constexpr (ACT) issueA(2 * i + 1, af1);
      __builtin_amdgcn_sched_barrier(0);
      combine(ch1 < Kpad ? ch1 : 0);
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (ACT) products(cur, 0, af0, [&](int q) { commit_q(nxt, q); });
      else {
#pragma unroll
        for (int q = 0; q < 4; ++q) commit_q(nxt, q);
      }
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (ACT) issueA(2 * i + 2, af0);
      issueB(ch1 + PG_KC);
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (ACT) products(cur, 1, af1, [&](int) {});
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      PWG_STAMP();
      __builtin_amdgcn_s_barrier();                // raw barrier: the loads in flight stay in flight
      PWG_STAMP();
      char* t = cur; cur = nxt; nxt = t;
    }
  };
  if (mBase < M) mainloop(std::true_type{});
  else mainloop(std::false_type{});
  __syncthreads();                                 // drains the read-ahead loads before LDS is reused
  PWG_STAMP();
  const P4Tile tile = {wave, half, l31, tid, mBase, n, nrem, ds, pos, grp, true, pok, skip};
  if constexpr (EPI == 1) {
    // operand prefetch depth of the epilogue: what the registers freed by the main loop hold next to the accumulators
    if (a.ex2) p4_epilogue<MT, 4, EPI, true, 4, MT == 2 ? 1 : 4, true>(a, acc, lds, tile);
    else p4_epilogue<MT, 4, EPI, true, 4, MT == 2 ? 3 : 4, false>(a, acc, lds, tile);
  } else {
    p4_epilogue<MT, 4, EPI, true, 4>(a, acc, lds, tile);
  }
  PWG_STAMP();
#ifdef DSGCN_LAB
  if (blockIdx.x == PWG_STAMP_BLOCK && threadIdx.x == 0) g_pwg_stamp[63] = nst;
#endif
}

template <int MODE, int EPI, int MT>
__global__ __launch_bounds__(256, 2) void k_pwg3(Pw4Args a, const unsigned short* __restrict__ wfr, int RT,
                                                 P4GuestArg<pwg3_hosts<MODE, EPI, MT>> guest) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  int bid = blockIdx.x;
  if constexpr (pwg3_hosts<MODE, EPI, MT>) {       // guest blocks (see P4Guest): the leading workgroups
    if (bid < guest.nblk) {
      p4_block<1, 2, 0, 16, EPI>(guest.a, bid, lds);
      return;
    }
    bid -= guest.nblk;
  }
  pwg3_body<MODE, EPI, MT, 3>(a, wfr, RT, bid, lds);
}

// matmul precision 'high': the same launch on two terms per operand (three products); the guest blocks run their narrow
// fp32 form unchanged
template <int MODE, int EPI, int MT>
__global__ __launch_bounds__(256, 2) void k_pwg3h(Pw4Args a, const unsigned short* __restrict__ wfr, int RT,
                                                  P4GuestArg<pwg3_hosts<MODE, EPI, MT>> guest) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  int bid = blockIdx.x;
  if constexpr (pwg3_hosts<MODE, EPI, MT>) {
    if (bid < guest.nblk) {
      p4_block<1, 2, 0, 16, EPI>(guest.a, bid, lds);
      return;
    }
    bid -= guest.nblk;
  }
  pwg3_body<MODE, EPI, MT, 2>(a, wfr, RT, bid, lds);
}

// The three bf16 terms of W (Co x Ci) as two images, k contiguous and zero-padded to whole tiles:
//   N (forward):        rows co < MpN = ceil256(Co), k = ci < KpN = ceil32(Ci)      [3][MpN][KpN] bf16
//   T (data gradient):  rows ci < MpT = ceil256(Ci), k = co < KpT = ceil32(Co)      [3][MpT][KpT] bf16, after N
// One thread per (row, 4 consecutive k).
// frag = 1 (k_pwg3): each plane in MFMA-fragment order instead, [row tile][k-step][lane = 32*(k%16 / 8) + row%32][k%8].
__global__ __launch_bounds__(256) void k_wsplit(const float* __restrict__ w, int Ci, int Co, unsigned short* __restrict__ out,
                                                int MpN, int KpN, int MpT, int KpT, int frag) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int t1 = MpN * (KpN >> 2), t2 = MpT * (KpT >> 2);
  float v[4];
  unsigned short* dst;
  int pstride;                                     // elements between the term planes
  if (i < t1) {
    const int r = i / (KpN >> 2), k = 4 * (i - r * (KpN >> 2));
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = (r < Co && k + e < Ci) ? w[(size_t)r * Ci + k + e] : 0.f;
    dst = out + (frag ? ((size_t)(r >> 5) * (KpN >> 4) + (k >> 4)) * 512 + (((k >> 3) & 1) * 32 + (r & 31)) * 8 + (k & 7)
                      : (size_t)r * KpN + k);
    pstride = MpN * KpN;
  } else if (i - t1 < t2) {
    const int j = i - t1;
    const int r = j / (KpT >> 2), k = 4 * (j - r * (KpT >> 2));
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = (r < Ci && k + e < Co) ? w[(size_t)(k + e) * Ci + r] : 0.f;
    dst = out + (size_t)3 * MpN * KpN +
          (frag ? ((size_t)(r >> 5) * (KpT >> 4) + (k >> 4)) * 512 + (((k >> 3) & 1) * 32 + (r & 31)) * 8 + (k & 7)
                : (size_t)r * KpT + k);
    pstride = MpT * KpT;
  } else {
    return;
  }
  unsigned p0, p1, p2, q0, q1, q2;
  b3_split(v[0], v[1], p0, p1, p2);
  b3_split(v[2], v[3], q0, q1, q2);
  *reinterpret_cast<u32x2v*>(dst) = u32x2v{p0, q0};
  *reinterpret_cast<u32x2v*>(dst + pstride) = u32x2v{p1, q1};
  *reinterpret_cast<u32x2v*>(dst + 2 * (size_t)pstride) = u32x2v{p2, q2};
}

// The same for up to WS_MAXJOBS convs in ONE launch (the 22 wide convs of a DS-STGCN step: 22 dependent 4 us launches at
// the head of their convs -> one at the head of the step).  The job table rides in the kernel arguments.
constexpr int WS_MAXJOBS = 32;
struct WsJobs {
  const float* w[WS_MAXJOBS];
  unsigned short* out[WS_MAXJOBS];
  int Ci[WS_MAXJOBS], Co[WS_MAXJOBS];
  int blk0[WS_MAXJOBS + 1];                         // first block of job j; blk0[njobs] = grid
  int njobs, frag;
};

__global__ __launch_bounds__(256) void k_wsplit_multi(WsJobs jb) {
  int j = 0;
  while (j + 1 < jb.njobs && (int)blockIdx.x >= jb.blk0[j + 1]) ++j;
  const int Ci = jb.Ci[j], Co = jb.Co[j];
  const float* __restrict__ w = jb.w[j];
  unsigned short* __restrict__ out = jb.out[j];
  const int MpN = (Co + 255) / 256 * 256, KpN = (Ci + 31) / 32 * 32, MpT = (Ci + 255) / 256 * 256, KpT = (Co + 31) / 32 * 32;
  const int i = ((int)blockIdx.x - jb.blk0[j]) * 256 + threadIdx.x;
  const int t1 = MpN * (KpN >> 2), t2 = MpT * (KpT >> 2);
  float v[4];
  unsigned short* dst;
  int pstride;
  if (i < t1) {
    const int r = i / (KpN >> 2), k = 4 * (i - r * (KpN >> 2));
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = (r < Co && k + e < Ci) ? w[(size_t)r * Ci + k + e] : 0.f;
    dst = out + (jb.frag ? ((size_t)(r >> 5) * (KpN >> 4) + (k >> 4)) * 512 + (((k >> 3) & 1) * 32 + (r & 31)) * 8 + (k & 7)
                         : (size_t)r * KpN + k);
    pstride = MpN * KpN;
  } else if (i - t1 < t2) {
    const int q = i - t1;
    const int r = q / (KpT >> 2), k = 4 * (q - r * (KpT >> 2));
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = (r < Ci && k + e < Co) ? w[(size_t)(k + e) * Ci + r] : 0.f;
    dst = out + (size_t)3 * MpN * KpN +
          (jb.frag ? ((size_t)(r >> 5) * (KpT >> 4) + (k >> 4)) * 512 + (((k >> 3) & 1) * 32 + (r & 31)) * 8 + (k & 7)
                   : (size_t)r * KpT + k);
    pstride = MpT * KpT;
  } else {
    return;
  }
  unsigned p0, p1, p2, q0, q1, q2;
  b3_split(v[0], v[1], p0, p1, p2);
  b3_split(v[2], v[3], q0, q1, q2);
  *reinterpret_cast<u32x2v*>(dst) = u32x2v{p0, q0};
  *reinterpret_cast<u32x2v*>(dst + pstride) = u32x2v{p1, q1};
  *reinterpret_cast<u32x2v*>(dst + 2 * (size_t)pstride) = u32x2v{p2, q2};
}

struct WsDims { int MpN, KpN, MpT, KpT; size_t bytes; };
WsDims ws_dims(int Ci, int Co) {
  WsDims d;
  d.MpN = (Co + 255) / 256 * 256; d.KpN = (Ci + 31) / 32 * 32;
  d.MpT = (Ci + 255) / 256 * 256; d.KpT = (Co + 31) / 32 * 32;
  d.bytes = ((size_t)3 * d.MpN * d.KpN + (size_t)3 * d.MpT * d.KpT) * 2;
  return d;
}

// K-split form of the tiny-plane launches (lab key 19).  OFF in the product: measured −0.02 ms/step (profiles/r06/
// small_launch_ab.txt) — and it changes the summation order of the projection convs, which moved the frozen whole-gradient
// ratios of the DS-STGCN configurations by 5-20 % (chaotic amplification, every per-kernel test unchanged): not worth a
// re-recording of the marks.
int g_p4_ksp = 0;
int g_p4_fill = 1;      // under-filled launches take one row tile per wave (lab key 20)
int g_p4_mt1 = 0;       // lab key 22: 128-row workgroups also for convs with more than 128 rows (bit 0 forward, bit 1 data gradient)
int g_p4_nq = 0, g_p4_mt = 0, g_p4_pd = 0, g_p4_gemm = 3, g_p4_gmin = 64, g_p4_gminl = 128, g_p4_ws = 2;   // ws: 2 = k_pwg3 on the fragment-order image; 1 = row-major image (lab A/B: no consumer left, k_pwg runs); g_p4_pd unused

struct P4Plan { int MT, NQ, PD, cc, span, WT, ngrp, Kpad, gemm, Lq, ksp; size_t lds; unsigned grid; };

bool p4_plan(int n, int K, int M, int L, P4Plan* p, int epi = 0) {
  const bool ragged = L % 2 != 0 && L >= 4;         // odd planes: runs of 4, the last one moved back to end at the plane's end
  if (L % 2 != 0 && !ragged) return false;
  int NQ = (L % 4 == 0 || ragged) ? 4 : 2;
  const int mtiles = (M + 31) / 32;
  int MT = mtiles >= 2 ? 2 : 1;
  // 33..48 and 65..96 output rows (the K*mid widths of the `pre` conv and of the `post` conv's data gradient): one row
  // tile per wave and one more workgroup per tile column — a 3-tile wave (NQ = 2) left the launch at 200 workgroups,
  // a 2-tile wave wastes a half-empty tile on every wave (tools/kc_bench.py 5=1: 256->96 forward 50 -> 39 us,
  // 96->256 data gradient 70 -> 62 us, 128->48 forward 29 -> 25 us, 48->128 data gradient 45 -> 36 us)
  if (mtiles == 3 || (mtiles == 2 && M <= 48)) MT = 1;
  // tiny planes (the dynamic-adjacency projections: 32 padded joints per sample): the launch is a latency chain of K/2
  // k-steps on few waves, so give every wave the smallest tile (1 x 2 MFMAs per k-step) and the grid the most waves
  const bool tiny = L <= 64 && (long)n * ((L + 127) / 128) < 1024 && !ragged;
  if (tiny) { NQ = 2; MT = 1; }
  // (round 6) a launch that would not even put one workgroup on every CU: one row tile per wave doubles the workgroups
  // (CTR-GCN's conv4 at 64 output channels: 157 position groups x 1 row block on 256 CUs)
  if (g_p4_fill && MT == 2 && ((((long)n * ((L + NQ - 1) / NQ * NQ) + 32 * NQ - 1) / (32 * NQ) + 3) / 4) * ((mtiles + 1) / 2) < 256) MT = 1;
  if ((g_p4_nq == 2 && !ragged) || (g_p4_nq == 4 && L % 4 == 0)) NQ = g_p4_nq;
  if (g_p4_mt) MT = g_p4_mt < mtiles ? g_p4_mt : mtiles;
  if (MT * NQ > 8 && !ragged) NQ = 2;
  if (MT * NQ > 8) MT = ragged ? 2 : 4;
  const int PD = NQ == 4 ? 8 : 16;
  // samples a wave's 32*NQ-position tile can touch; its buffer resources span that many planes (32-bit offsets)
  const int Lq = (L + NQ - 1) / NQ * NQ;
  const int span = (32 * NQ + Lq - 1) / Lq + 1;
  if ((long)K * L * 4 * span >= (1L << 31) - 64 || (long)M * L * 4 * span >= (1L << 31) - 64) return false;
  if ((long)n * L >= (1L << 31) - 256) return false;
  p->MT = MT; p->NQ = NQ; p->PD = PD; p->Lq = Lq;
  p->cc = (mtiles + MT - 1) / MT;
  p->span = span;
  p->WT = (int)(((long)n * Lq + 32 * NQ - 1) / (32 * NQ));
  p->ngrp = (p->WT + 3) / 4;
  p->Kpad = (K + 2 * PD - 1) / (2 * PD) * (2 * PD);
  size_t f = (size_t)((32 * MT * (p->Kpad + 1) + 2 + 3) & ~3) + (size_t)4 * (p->Kpad + 2);   // + the pipeline's read-ahead pad
  const size_t fe = (size_t)4 * 3 * 32 * 36 + (size_t)4 * MT * 32 * 4 + (size_t)MT * 32 * 4;    // epilogue image
  if (f < fe) f = fe;
  p->lds = f * sizeof(float);
  // the K-split form of the tiny-plane launches (k_pw4<.., KSP>): at least one prefetch round per wave; the launcher takes
  // it for plain operands without statistics / input-affine sums (the projections) and then needs room for three waves'
  // accumulators
  p->ksp = (g_p4_ksp && tiny && MT == 1 && NQ == 2 && p->Kpad / (2 * PD) >= 4) ? 1 : 0;
  if (p->ksp && p->lds < (size_t)3 * MT * NQ * 16 * 64 * sizeof(float)) p->lds = (size_t)3 * MT * NQ * 16 * 64 * sizeof(float);
  p->gemm = 0;
  if ((g_p4_gemm & (1 << epi)) && (L % 4 == 0 || ragged) && K % 4 == 0 && M % 4 == 0 && K >= g_p4_gmin && M > 64 &&
      L >= g_p4_gminl) {
    p->gemm = 1; p->MT = 1; p->NQ = 4;
    p->cc = (M + PG_T - 1) / PG_T;
    p->span = (128 + Lq - 1) / Lq + 1;             // (the tiny-plane rule above may have chosen 64-position tiles)
    p->WT = (int)(((long)n * Lq + 127) / 128);
    p->ngrp = p->WT;                               // one position tile per workgroup
    p->Kpad = (K + PG_KC - 1) / PG_KC * PG_KC;
    size_t b = (size_t)3 * ((epi ? PG_TAM : PG_T) + PG_T) * PG_RB + (size_t)p->Kpad * 16;
    const size_t be = ((size_t)4 * 3 * 32 * 36 + 4 * 32 * 4 + 4 * 32 * 4) * sizeof(float);   // epilogue image, per-wave rows
    p->lds = b < be ? be : b;
  }
  if (p->lds > 160 * 1024) return false;
  p->grid = (unsigned)((p->ngrp + 7) / 8 * 8 * p->cc);
  return true;
}

// The launch helpers return whether the instantiation they chose TOOK the guest `h` (a host kernel by its compile-time
// predicate): the entry points report "hosted" from that, so a guest no kernel carried is launched on its own.
template <int MT, int NQ, int MODE, int PD, int EPI>
bool p4_launch_one(const Pw4Args& a, const P4Plan& p, hipStream_t st, const P4Hosted* h) {
  constexpr bool HOST = p4_hosts<MT, NQ, MODE, PD, EPI, false>;
  const bool hosted = HOST && h;
  const dim3 grid(p.grid + (hosted ? (unsigned)h->g.nblk : 0u), a.ngroup > 1 ? (unsigned)a.ngroup : 1u), blk(P4_NT);
  const size_t lds = (hosted && h->lds > p.lds) ? h->lds : p.lds;
  hipLaunchKernelGGL((k_pw4<MT, NQ, MODE, PD, EPI>), grid, blk, lds, st, a, p4_guest_arg<HOST>(hosted ? h : nullptr));
  return hosted;
}

template <int MT, int NQ, int PD>
bool p4_launch_cfg(const Pw4Args& a, int mode, int epi, const P4Plan& p, hipStream_t st, const P4Hosted* h = nullptr) {
  if (epi == 0) {
    if (mode == 0) return p4_launch_one<MT, NQ, 0, PD, 0>(a, p, st, h);
    if (mode == 1) return p4_launch_one<MT, NQ, 1, PD, 0>(a, p, st, h);
    return p4_launch_one<MT, NQ, 2, PD, 0>(a, p, st, h);
  }
  if (mode == 0) return p4_launch_one<MT, NQ, 0, PD, 1>(a, p, st, h);
  return p4_launch_one<MT, NQ, 2, PD, 1>(a, p, st, h);
}

// the fragment-image form: MT = 2 (256 rows per workgroup) when the conv has more than 128 output rows
template <int MODE, int EPI, int MT>
bool pwg3_launch_one(const Pw4Args& a, const dim3 grid, size_t lds, hipStream_t st, const unsigned short* wfr, int RT,
                     const P4Hosted* h, bool high) {
  constexpr bool HOST = pwg3_hosts<MODE, EPI, MT>;
  const bool hosted = HOST && h;
  const dim3 g(grid.x + (hosted ? (unsigned)h->g.nblk : 0u));
  if (hosted && h->lds > lds) lds = h->lds;
  if (high) hipLaunchKernelGGL((k_pwg3h<MODE, EPI, MT>), g, dim3(256), lds, st, a, wfr, RT, p4_guest_arg<HOST>(hosted ? h : nullptr));
  else hipLaunchKernelGGL((k_pwg3<MODE, EPI, MT>), g, dim3(256), lds, st, a, wfr, RT, p4_guest_arg<HOST>(hosted ? h : nullptr));
  return hosted;
}

template <int MT>
bool pwg3_launch(Pw4Args a, int mode, int epi, const P4Plan& p, const unsigned short* wfr, int Mp, hipStream_t st,
                 const P4Hosted* h = nullptr, bool high = false) {
  constexpr int TA = 128 * MT;
  a.cc = (a.M + TA - 1) / TA;
  const size_t main_b = (size_t)2 * G3_BBUF + (size_t)p.Kpad * 16;
  const size_t epi_b = (size_t)4 * (3 * 32 * 36 + MT * 32 * 3 + MT * 32 * 4) * sizeof(float);
  const size_t lds = main_b > epi_b ? main_b : epi_b;
  static bool raised = false;
  if (!raised) {
    const void* fs[5] = {reinterpret_cast<const void*>(&k_pwg3<0, 0, MT>), reinterpret_cast<const void*>(&k_pwg3<1, 0, MT>),
                         reinterpret_cast<const void*>(&k_pwg3<2, 0, MT>), reinterpret_cast<const void*>(&k_pwg3<0, 1, MT>),
                         reinterpret_cast<const void*>(&k_pwg3<2, 1, MT>)};
    const void* hs[5] = {reinterpret_cast<const void*>(&k_pwg3h<0, 0, MT>), reinterpret_cast<const void*>(&k_pwg3h<1, 0, MT>),
                         reinterpret_cast<const void*>(&k_pwg3h<2, 0, MT>), reinterpret_cast<const void*>(&k_pwg3h<0, 1, MT>),
                         reinterpret_cast<const void*>(&k_pwg3h<2, 1, MT>)};
    for (const void* f : fs) (void)hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024);
    for (const void* f : hs) (void)hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024);
    raised = true;
  }
  const dim3 grid((unsigned)((p.ngrp + 7) / 8 * 8 * a.cc));
  const int RT = Mp / 32;
  if (epi == 0) {
    if (mode == 0) return pwg3_launch_one<0, 0, MT>(a, grid, lds, st, wfr, RT, h, high);
    if (mode == 1) return pwg3_launch_one<1, 0, MT>(a, grid, lds, st, wfr, RT, h, high);
    return pwg3_launch_one<2, 0, MT>(a, grid, lds, st, wfr, RT, h, high);
  }
  if (mode == 0) return pwg3_launch_one<0, 1, MT>(a, grid, lds, st, wfr, RT, h, high);
  return pwg3_launch_one<2, 1, MT>(a, grid, lds, st, wfr, RT, h, high);
}

template <int PD>
bool p4_launch_pd(const Pw4Args& a, int mode, int epi, const P4Plan& p, hipStream_t st, const unsigned short* wsp = nullptr,
                  int Mp = 0, const P4Hosted* h = nullptr, bool* took = nullptr, bool high = false) {
  const int key = p.MT * 10 + p.NQ;
  bool t = false;                                  // the launch carried the guest h
  if (took) *took = false;
  if (p.gemm && wsp && g_p4_ws == 2) {
    if (a.M > 128 && !(g_p4_mt1 & (1 << epi))) t = pwg3_launch<2>(a, mode, epi, p, wsp, Mp, st, h, high);
    else t = pwg3_launch<1>(a, mode, epi, p, wsp, Mp, st, h, high);
    if (took) *took = t;
    return true;
  }
  if (p.gemm) {
    static bool raised = false;                    // 64 KB+ of dynamic LDS
    if (!raised) {
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_pwg<0, 0>), hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024);
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_pwg<1, 0>), hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024);
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_pwg<2, 0>), hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024);
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_pwg<0, 1>), hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024);
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_pwg<2, 1>), hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024);
      raised = true;
    }
    const dim3 grid(p.grid), blk(P4_NT);
    if (epi == 0) {
      if (mode == 0) hipLaunchKernelGGL((k_pwg<0, 0>), grid, blk, p.lds, st, a);
      else if (mode == 1) hipLaunchKernelGGL((k_pwg<1, 0>), grid, blk, p.lds, st, a);
      else hipLaunchKernelGGL((k_pwg<2, 0>), grid, blk, p.lds, st, a);
    } else {
      if (mode == 0) hipLaunchKernelGGL((k_pwg<0, 1>), grid, blk, p.lds, st, a);
      else hipLaunchKernelGGL((k_pwg<2, 1>), grid, blk, p.lds, st, a);
    }
    return true;
  }
  // only the prefetch depth the plan chooses for each quad width is instantiated (4-position quads: 8 k-steps, 2-position
  // quads: 16): the other combinations were never launched and compiled to 140-VGPR-spill code objects
  if constexpr (PD == 8) {
    switch (key) {
      case 14: t = p4_launch_cfg<1, 4, PD>(a, mode, epi, p, st, h); if (took) *took = t; return true;
      case 24: t = p4_launch_cfg<2, 4, PD>(a, mode, epi, p, st, h); if (took) *took = t; return true;
    }
  } else {
    switch (key) {
      case 12: p4_launch_cfg<1, 2, PD>(a, mode, epi, p, st); return true;
      case 22: p4_launch_cfg<2, 2, PD>(a, mode, epi, p, st); return true;
      case 32: p4_launch_cfg<3, 2, PD>(a, mode, epi, p, st); return true;
      case 42: p4_launch_cfg<4, 2, PD>(a, mode, epi, p, st); return true;
    }
  }
  return false;
}

// A guest record (dsgcn_jobs.h) -> the arguments, grid and LDS of its body (the arguments dsgcn_p4_fwd / dsgcn_p4_dgrad
// give the stand-alone launch of the same conv); false unless it is the <1, 2, 0, 16, epi> shape of the dynamic-adjacency
// projections (plain operand, tiny planes, no K split).
bool p4_guest_plan(const dsgcn_guest_conv& g, int epi, P4Hosted* h) {
  if (!g.in || !g.w || !g.out || g.n <= 0 || g.Ci <= 0 || g.Co <= 0 || g.L <= 0) return false;
  const int K = epi ? g.Co : g.Ci, M = epi ? g.Ci : g.Co;
  P4Plan p;
  if (!p4_plan(g.n, K, M, g.L, &p, epi) || p.gemm || p.ksp || p.MT != 1 || p.NQ != 2 || p.PD != 16) return false;
  if (p.lds > 64 * 1024 || p.grid % 8 != 0) return false;
  Pw4Args a = {};
  a.b1 = g.in; a.w = g.w; a.out = g.out;
  if (epi == 0) { a.w_ldm = g.Ci; a.w_ldk = 1; a.bias = g.bias; }
  else { a.w_ldm = 1; a.w_ldk = g.Ci; }          // A = W^T; plain forward input: no mask, no affine sums
  a.n = g.n; a.K = K; a.M = M; a.L = g.L; a.span = p.span; a.WT = p.WT; a.cc = p.cc; a.Kpad = p.Kpad; a.Lq = p.Lq;
  h->g.a = a;
  h->g.nblk = (int)p.grid;
  h->lds = p.lds;
  return true;
}

// does the launch of plan `p` take guest blocks?  Forward (epi 0): plain operand on k_pw4<1, 4, 0, 8, 0> or, with the
// fragment-order weight image, on k_pwg3<0, 0, 1>; data gradient (epi 1): two-stream dz_eff on k_pw4<2, 4, 2, 8, 1> or
// k_pwg3<2, 1, .>
bool p4_hosts_guest(const P4Plan& p, int epi, int mode, int M, bool have_ws) {
  if (mode != (epi ? 2 : 0)) return false;
  if (p.gemm) return have_ws && g_p4_ws == 2 && (epi == 1 || !(M > 128 && !(g_p4_mt1 & 1)));
  return !p.ksp && p.MT == (epi ? 2 : 1) && p.NQ == 4 && p.PD == 8;
}

}  // namespace

int dsgcn_p4_guest_plan(const dsgcn_guest_conv* g, int epi, P4Hosted* h) {
  return (g && p4_guest_plan(*g, epi, h)) ? 1 : 0;
}

// Internal (not part of the C ABI; declared hidden in kc.h): called by pwconv.hip's dispatch when the shape qualifies
// (stride 1, even plane size).  Return 1 = launched, 0 = not eligible, <0 / >0 = error codes as everywhere.
int dsgcn_p4_tuning(int key, int value) {
  if (key == 0) g_p4_nq = value;
  else if (key == 1) g_p4_mt = value;
  else if (key == 2) g_p4_pd = value;
  else if (key == 3) g_p4_gemm = value;
  else if (key == 4) g_p4_gmin = value;
  else if (key == 5) g_p4_gminl = value;
  else if (key == 6) g_p4_ws = value;
  else if (key == 7) g_p4_ksp = value;
  else if (key == 8) g_p4_fill = value;
  else if (key == 9) g_p4_mt1 = value;
  else return DSGCN_EINVAL;
  return 0;
}

// bf16 products per fp32 product of the forward (epi 0: K = Ci, M = Co) / data gradient (epi 1: K = Co, M = Ci) launch of
// this shape under the current precision level, the weight image supplied wherever dsgcn_p4_ws_bytes asks for one:
// 6 / 3 = k_pwg3 / k_pwg3h (k_pwg without the fragment-order image: always 6), 0 = an fp32 MFMA form
int dsgcn_p4_terms(int n, int K, int M, int L, int epi) {
  P4Plan p;
  if (!p4_plan(n, K, M, L, &p, epi) || !p.gemm) return 0;
  return (g_p4_ws == 2 && dsgcn_precision_level() == 1) ? 3 : 6;
}

int dsgcn_p4_groups(int n, int K, int M, int L, int epi) {
  P4Plan p;
  return p4_plan(n, K, M, L, &p, epi) ? p.ngrp : 0;
}

int dsgcn_p4_fwd(const KcIn& in, const float* w, const float* bias, float* z, float* partial, int n, int Ci, int Co, int L,
                 hipStream_t st, const void* ws, const dsgcn_guest_conv* guest, int* hosted) {
  P4Plan p;
  if (hosted) *hosted = 0;
  if (!p4_plan(n, Ci, Co, L, &p)) return 0;
  const WsDims wd = ws_dims(Ci, Co);
  const unsigned short* wsp = static_cast<const unsigned short*>(ws);
  Pw4Args a = {};
  a.b1 = in.x1; a.b2 = in.x2; a.ps1 = in.s1; a.ph1 = in.h1; a.ps2 = in.s2; a.ph2 = in.h2; a.relu = in.relu;
  a.w = w; a.w_ldm = Ci; a.w_ldk = 1; a.bias = bias; a.out = z; a.partial = partial;
  a.n = n; a.K = Ci; a.M = Co; a.L = L; a.span = p.span; a.WT = p.WT; a.cc = p.cc; a.Kpad = p.Kpad; a.Lq = p.Lq;
  const int mode = in.x2 ? 2 : ((in.s1 || in.relu) ? 1 : 0);
  if (p.ksp && !p.gemm && mode == 0 && !partial) {
    hipLaunchKernelGGL((k_pw4<1, 2, 0, 16, 0, true>), dim3((unsigned)((p.WT + 7) / 8 * 8 * p.cc)), dim3(P4_NT), p.lds, st, a, P4NoGuest{});
    DSGCN_LAUNCH_CHECK();
    return 1;
  }
  // a guest conv rides in the leading workgroups when both sides qualify; otherwise the caller launches it on its own
  P4Hosted hg;
  const P4Hosted* h = nullptr;
  if (guest && p4_hosts_guest(p, 0, mode, Co, wsp != nullptr) && p4_guest_plan(*guest, 0, &hg)) h = &hg;
  bool took = false;
  const bool high = dsgcn_precision_level() == 1;  // (read here, on the host: a captured launch keeps its kernel)
  const bool ok = p.PD == 8 ? p4_launch_pd<8>(a, mode, 0, p, st, wsp, wd.MpN, h, &took, high)
                            : p4_launch_pd<16>(a, mode, 0, p, st, wsp, wd.MpN, h, &took, high);
  if (!ok) return 0;
  DSGCN_LAUNCH_CHECK();
  if (hosted && took) *hosted = 1;
  return 1;
}

// 1 = the forward of a plain-operand (Ci -> Co) conv over n planes of L positions hosts `guest` (have_ws: the caller passes
// the pre-split weight image the shape asks for)
int dsgcn_p4_fwd_hosts(int n, int Ci, int Co, int L, int have_ws, const dsgcn_guest_conv* guest) {
  P4Plan p;
  P4Hosted hg;
  if (!guest || !p4_plan(n, Ci, Co, L, &p)) return 0;
  if (p.ksp && !p.gemm) return 0;
  return (p4_hosts_guest(p, 0, 0, Co, have_ws != 0) && p4_guest_plan(*guest, 0, &hg)) ? 1 : 0;
}

// d: dz_eff = gz + A0 + B0*z (either part may be absent);  in: the forward's virtual input.
int dsgcn_p4_dgrad(const KcIn& in, const float* w, const KcDz& d, float* dx1, float* dx2, float* ipart, int n, int Ci, int Co,
                   int L, hipStream_t st, const void* ws, const dsgcn_guest_conv* guest, int* hosted) {
  P4Plan p;
  if (hosted) *hosted = 0;
  if (!d.gz) return 0;                             // (a conv whose output has no direct gradient: not on the fast path)
  if (!p4_plan(n, Co, Ci, L, &p, 1)) return 0;
  Pw4Args a = {};
  a.b1 = d.gz; a.b2 = d.A0 ? d.z : nullptr;
  a.ps1 = nullptr; a.ph1 = d.A0; a.ps2 = d.B0; a.ph2 = nullptr; a.relu = 0;
  a.w = w; a.w_ldm = 1; a.w_ldk = Ci; a.bias = nullptr; a.out = dx1; a.partial = nullptr;
  a.ex1 = in.x1; a.ex2 = in.x2; a.es1 = in.s1; a.eh1 = in.h1; a.es2 = in.s2; a.eh2 = in.h2; a.erelu = in.relu;
  a.out2 = dx2; a.ipart = ipart;
  a.n = n; a.K = Co; a.M = Ci; a.L = L; a.span = p.span; a.WT = p.WT; a.cc = p.cc; a.Kpad = p.Kpad; a.Lq = p.Lq;
  const int mode = d.A0 ? 2 : 0;
  if (p.ksp && !p.gemm && mode == 0 && !ipart) {
    hipLaunchKernelGGL((k_pw4<1, 2, 0, 16, 1, true>), dim3((unsigned)((p.WT + 7) / 8 * 8 * p.cc)), dim3(P4_NT), p.lds, st, a, P4NoGuest{});
    DSGCN_LAUNCH_CHECK();
    return 1;
  }
  const WsDims wd = ws_dims(Ci, Co);
  const unsigned short* wsp = ws ? static_cast<const unsigned short*>(ws) + (size_t)3 * wd.MpN * wd.KpN : nullptr;   // the T image
  P4Hosted hg;
  const P4Hosted* h = nullptr;
  if (guest && p4_hosts_guest(p, 1, mode, Ci, wsp != nullptr) && p4_guest_plan(*guest, 1, &hg)) h = &hg;
  bool took = false;
  const bool high = dsgcn_precision_level() == 1;
  const bool ok = p.PD == 8 ? p4_launch_pd<8>(a, mode, 1, p, st, wsp, wd.MpT, h, &took, high)
                            : p4_launch_pd<16>(a, mode, 1, p, st, wsp, wd.MpT, h, &took, high);
  if (!ok) return 0;
  DSGCN_LAUNCH_CHECK();
  if (hosted && took) *hosted = 1;
  return 1;
}

// 1 = the data gradient of a (Ci -> Co) conv with batch-statistics terms (A0 / B0) hosts `guest`
int dsgcn_p4_dgrad_hosts(int n, int Ci, int Co, int L, int have_ws, const dsgcn_guest_conv* guest) {
  P4Plan p;
  P4Hosted hg;
  if (!guest || !p4_plan(n, Co, Ci, L, &p, 1)) return 0;
  return (p4_hosts_guest(p, 1, 2, Ci, have_ws != 0) && p4_guest_plan(*guest, 1, &hg)) ? 1 : 0;
}

// Up to three convs of one shape in ONE launch (k_pw4 only: plain / affine operand, no second stream, no statistics).
// Return 1 = launched, 0 = not eligible (the caller launches them one by one).
int dsgcn_p4_group_ok(int n, int Ci, int Co, int L) {
  P4Plan pf, pb;
  return (p4_plan(n, Ci, Co, L, &pf, 0) && !pf.gemm && p4_plan(n, Co, Ci, L, &pb, 1) && !pb.gemm) ? 1 : 0;
}

int dsgcn_p4_fwd_group(const float* const* x1, const float* const* s1, const float* const* h1, int relu,
                       const float* const* w, float* const* z, int ng, int n, int Ci, int Co, int L, hipStream_t st) {
  P4Plan p;
  if (ng < 1 || ng > 3 || !p4_plan(n, Ci, Co, L, &p) || p.gemm) return 0;
  Pw4Args a = {};
  a.b1 = x1[0]; a.ps1 = s1[0]; a.ph1 = h1[0]; a.relu = relu;
  a.w = w[0]; a.w_ldm = Ci; a.w_ldk = 1; a.out = z[0];
  a.n = n; a.K = Ci; a.M = Co; a.L = L; a.span = p.span; a.WT = p.WT; a.cc = p.cc; a.Kpad = p.Kpad; a.Lq = p.Lq;
  a.ngroup = ng;
  for (int g = 0; g < ng; ++g) {
    if ((s1[g] == nullptr) != (s1[0] == nullptr)) return DSGCN_EINVAL;
    a.g[g] = Pw4Args::Grp{x1[g], s1[g], h1[g], w[g], z[g], nullptr, nullptr, nullptr, nullptr};
  }
  const int mode = (s1[0] || relu) ? 1 : 0;
  const bool ok = p.PD == 8 ? p4_launch_pd<8>(a, mode, 0, p, st) : p4_launch_pd<16>(a, mode, 0, p, st);
  if (!ok) return 0;
  DSGCN_LAUNCH_CHECK();
  return 1;
}

int dsgcn_p4_dgrad_group(const float* const* x1, const float* const* s1, const float* const* h1, int relu,
                         const float* const* w, const float* const* gz, float* const* dx1, float* const* ipart, int ng, int n,
                         int Ci, int Co, int L, hipStream_t st) {
  P4Plan p;
  if (ng < 1 || ng > 3 || !p4_plan(n, Co, Ci, L, &p, 1) || p.gemm) return 0;
  Pw4Args a = {};
  a.b1 = gz[0]; a.relu = 0;
  a.w = w[0]; a.w_ldm = 1; a.w_ldk = Ci; a.out = dx1[0];
  a.ex1 = x1[0]; a.es1 = s1[0]; a.eh1 = h1[0]; a.erelu = relu; a.ipart = ipart[0];
  a.n = n; a.K = Co; a.M = Ci; a.L = L; a.span = p.span; a.WT = p.WT; a.cc = p.cc; a.Kpad = p.Kpad; a.Lq = p.Lq;
  a.ngroup = ng;
  for (int g = 0; g < ng; ++g) {
    if ((s1[g] == nullptr) != (s1[0] == nullptr) || (ipart[g] == nullptr) != (ipart[0] == nullptr)) return DSGCN_EINVAL;
    a.g[g] = Pw4Args::Grp{gz[g], nullptr, nullptr, w[g], dx1[g], x1[g], s1[g], h1[g], ipart[g]};
  }
  const bool ok = p.PD == 8 ? p4_launch_pd<8>(a, 0, 1, p, st) : p4_launch_pd<16>(a, 0, 1, p, st);
  if (!ok) return 0;
  DSGCN_LAUNCH_CHECK();
  return 1;
}

// Bytes of the pre-split weight image a (Ci -> Co) conv over planes of L positions wants (0: neither its forward nor its
// data gradient takes the GEMM form), and the launch that fills it.
size_t dsgcn_p4_ws_bytes(int n, int Ci, int Co, int L) {
  P4Plan pf, pb;
  const bool f = p4_plan(n, Ci, Co, L, &pf, 0) && pf.gemm, b = p4_plan(n, Co, Ci, L, &pb, 1) && pb.gemm;
  if (!g_p4_ws || !(f || b)) return 0;
  return ws_dims(Ci, Co).bytes;
}

int dsgcn_p4_wsplit(const float* w, int Ci, int Co, void* out, hipStream_t st) {
  const WsDims d = ws_dims(Ci, Co);
  const long total = (long)d.MpN * (d.KpN >> 2) + (long)d.MpT * (d.KpT >> 2);
  hipLaunchKernelGGL(k_wsplit, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, w, Ci, Co,
                     static_cast<unsigned short*>(out), d.MpN, d.KpN, d.MpT, d.KpT, g_p4_ws == 2 ? 1 : 0);
  DSGCN_LAUNCH_CHECK();
  return 0;
}

int dsgcn_p4_wsplit_multi(const float* const* w, void* const* out, const int* Ci, const int* Co, int njobs, hipStream_t st) {
  for (int j0 = 0; j0 < njobs; j0 += WS_MAXJOBS) {
    WsJobs jb;
    jb.njobs = njobs - j0 < WS_MAXJOBS ? njobs - j0 : WS_MAXJOBS;
    jb.frag = g_p4_ws == 2 ? 1 : 0;
    int blk = 0;
    for (int j = 0; j < jb.njobs; ++j) {
      const WsDims d = ws_dims(Ci[j0 + j], Co[j0 + j]);
      const long total = (long)d.MpN * (d.KpN >> 2) + (long)d.MpT * (d.KpT >> 2);
      jb.w[j] = w[j0 + j]; jb.out[j] = static_cast<unsigned short*>(out[j0 + j]);
      jb.Ci[j] = Ci[j0 + j]; jb.Co[j] = Co[j0 + j];
      jb.blk0[j] = blk;
      blk += (int)((total + 255) / 256);
    }
    for (int j = jb.njobs; j <= WS_MAXJOBS; ++j) jb.blk0[j] = blk;
    hipLaunchKernelGGL(k_wsplit_multi, dim3((unsigned)blk), dim3(256), 0, st, jb);
    DSGCN_LAUNCH_CHECK();
  }
  return 0;
}

#ifdef DSGCN_LAB
extern "C" int dsgcn_pwg2_phases(long long* out) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_pwg_stamp), sizeof(long long) * 64);
}
extern "C" int dsgcn_pwg2_phases_block(int block) {
  return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_pwg_stamp_block), &block, sizeof(int));
}
#endif
