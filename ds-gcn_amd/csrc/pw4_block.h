// The body of K-C's wide-load kernel (k_pw4, csrc/pw4.hip) as a device function of (arguments, block id, LDS), shared by
// the kernels that run it: k_pw4 itself, and the launches that HOST a small conv in their leading workgroups (the guest
// blocks below: k_pw4 / k_pwg3 in pw4.hip, the one-pass narrow backward in bwd64.hip).
#pragma once
#include "kc.h"
#include <type_traits>

struct Pw4Args {
  const float* b1; const float* b2;                                        // B streams (n, K, L); b2 NULL unless MODE 2
  const float* ps1; const float* ph1; const float* ps2; const float* ph2;  // per-k affine (NULL = 1 / 0)
  int relu;
  const float* w; int w_ldm, w_ldk;                                        // A[m][k] = w[m*w_ldm + k*w_ldk]
  const float* bias;                                                       // per m, NULL ok
  float* out;                                                              // (n, M, L)
  float* partial;                                                          // EPI 0: [ngrp][M][2] or NULL
  const float* ex1; const float* ex2;                                      // EPI 1: forward operands at (n, M, L)
  const float* es1; const float* eh1; const float* es2; const float* eh2;
  int erelu;
  float* out2; float* ipart;                                               // EPI 1: d x2 or NULL; [ngrp][M][3] or NULL
  int n, K, M, L, span, WT, cc, Kpad;
  int Lq;                                                                  // positions per plane rounded up to a multiple of NQ (ragged planes)
  // (round 6) up to three convs of ONE shape in a launch (blockIdx.y = which): CTR-GCN refines its topology with three
  // conv4's per unit, each too small to fill the chip (k_pw4 only; the GEMM forms ignore it)
  int ngroup;
  struct Grp { const float* b1; const float* ps1; const float* ph1; const float* w; float* out;
               const float* ex1; const float* es1; const float* eh1; float* ipart; } g[3];
};

// A guest conv of a launch (see "guest blocks" below): its arguments and its grid (a multiple of 8; 0 = no guest).
struct P4Guest { Pw4Args a; int nblk; };
struct P4NoGuest {};
template <bool HOST> using P4GuestArg = std::conditional_t<HOST, P4Guest, P4NoGuest>;
// ... with the dynamic LDS its body needs (host side).  dsgcn_p4_guest_plan (kc.h, defined in pw4.hip): a guest record ->
// P4Hosted (epi 0: forward, in = x, out = z; 1: data gradient, in = gz, out = dx); 0 unless it is the <1, 2, 0, 16, epi>
// shape of the dynamic-adjacency projections (plain operand, tiny planes)
struct P4Hosted { P4Guest g; size_t lds; };

namespace {

constexpr int P4_NT = 256;
constexpr int P4_NT_STORE = 2;                   // cache-policy bits of the output stores: non-temporal (written once, read by a later launch)

template <int NQ>
__device__ __forceinline__ void p4_store(typename buf_vec<NQ>::T v, __amdgpu_buffer_rsrc_t r, int voff, int soff) {
  if constexpr (NQ == 4) {
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4v, v), r, voff, soff, P4_NT_STORE);
  } else {
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2v, v), r, voff, soff, P4_NT_STORE);
  }
}

// MODE 0: B' = b1;  1: relu?(b1*s1+h1);  2: relu?(b1*s1+h1 + b2*s2+h2).   EPI 0: forward (bias, statistics);  1: data gradient.
struct P4Tile { int wave, half, l31, tid, mBase, n, nrem, ds, pos, grp; bool wlive, pok; int skip; };

// Epilogue of a wave's (32*MT rows) x (32*NQ positions, lane-owned runs of NQ) accumulator tile, shared by k_pw4 and
// k_pwg.  OWNROWS = false: the workgroup's four waves hold the SAME rows at different positions (their per-row sums are
// added through LDS, one partial row per workgroup); true: the waves hold different rows of one position tile (each wave
// writes its rows of the workgroup's partial row itself).
// EPD > 0 (data gradient): the forward operands of the ReLU mask / affine sums are fetched EPD row groups (4 rows each)
// ahead of the group being finished, X2 saying at compile time whether a second stream exists — left to itself the loop
// is load -> wait -> compute -> store per group, eight dependent memory round trips per wave (the 15-27 us epilogue of the
// lab stamps, profiles/r03 / r04).  EPD = 0: the original form (the compiler's own schedule).
template <int MT, int NQ, int EPI, bool OWNROWS, int NWV = 4, int EPD = 0, bool X2 = true>
__device__ __forceinline__ void p4_epilogue(const Pw4Args& a, f32x16 (&acc)[MT][NQ], float* lds, const P4Tile& t) {
  typedef typename buf_vec<NQ>::T vq;
  const int wave = t.wave, half = t.half, l31 = t.l31, tid = t.tid, mBase = t.mBase, n = t.n, nrem = t.nrem, ds = t.ds,
            pos = t.pos, grp = t.grp;
  const bool wlive = t.wlive, pok = t.pok;
  const int M = a.M, L = a.L, L4 = L * 4;
  (void)L;
  const int skip = t.skip;                         // leading elements of the lane's run that the previous run also holds (0
                                                   // except for the last run of a ragged plane): stored, not summed
  // Epilogue.  Stores go through a per-sample buffer resource (invalid rows / positions get an out-of-range offset
  // and are dropped by the bounds check: no branches); per-channel sums through LDS transposes of the wave's tiles.
  constexpr int NTL = EPI == 0 ? 2 : 3;            // transposed tiles per wave
  float* Tw = lds + wave * (NTL * 32 * 36);
  const __amdgpu_buffer_rsrc_t ro = buf_rsrc(a.out + (size_t)n * M * L, wlive ? nrem * M * L4 : 0);
  const int ooff = pok ? ds * M * L4 + pos * 4 : BUF_OOB;
  if (EPI == 0) {
    double* Ss = reinterpret_cast<double*>(lds + NWV * NTL * 32 * 36);  // [waves][MT*32][2]
    const bool stats = a.partial != nullptr;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = mfma_row32(r, half);
        const int co = mBase + 32 * m + row;
        vq val;
        float s = 0.f, qq = 0.f;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
          val[q] = acc[m][q][r];
          if (q >= skip) {
            s += val[q];
            qq = fmaf(val[q], val[q], qq);
          }
        }
        p4_store<NQ>(val, ro, buf_rowoff(co < M, ooff, co * L4), 0);
        if (stats) {
          const bool ok = co < M && pok;
          Tw[row * 36 + l31] = ok ? s : 0.f;
          Tw[32 * 36 + row * 36 + l31] = ok ? qq : 0.f;
        }
      }
      if (stats) {
        wave_lds_sync();
        double sd = tile36_rowsum<double>(Tw, half, l31);
        double qd = tile36_rowsum<double>(Tw + 32 * 36, half, l31);
        wave_lds_sync();
        sd += __shfl_xor(sd, 32, 64);
        qd += __shfl_xor(qd, 32, 64);
        if (half == 0) {
          if constexpr (OWNROWS) {
            const int co = mBase + 32 * m + l31;
            if (co < M) {
              a.partial[((size_t)grp * M + co) * 2 + 0] = (float)sd;
              a.partial[((size_t)grp * M + co) * 2 + 1] = (float)qd;
            }
          } else {
            Ss[((wave * MT + m) * 32 + l31) * 2 + 0] = sd;
            Ss[((wave * MT + m) * 32 + l31) * 2 + 1] = qd;
          }
        }
      }
    }
    if (stats && !OWNROWS) {
      __syncthreads();
      if (tid < 32 * MT) {
        const int co = mBase + tid;
        if (co < M) {
          double s4 = 0.0, q4 = 0.0;
#pragma unroll
          for (int w = 0; w < 4; ++w) { s4 += Ss[((w * MT * 32) + tid) * 2]; q4 += Ss[((w * MT * 32) + tid) * 2 + 1]; }
          a.partial[((size_t)grp * M + co) * 2 + 0] = (float)s4;
          a.partial[((size_t)grp * M + co) * 2 + 1] = (float)q4;
        }
      }
    }
  } else {
    float* Ss = lds + NWV * NTL * 32 * 36;                               // [waves][MT*32][3]
    f32x4* Es = reinterpret_cast<f32x4*>(Ss + NWV * MT * 32 * 3);        // [MT*32] (s1, h1, s2, h2) of the block's rows
    const bool need_x = a.erelu || a.es1 != nullptr || a.ex2 != nullptr;
    const bool has2 = a.ex2 != nullptr;
    const bool sums = a.ipart != nullptr;
    if constexpr (OWNROWS) Es += wave * 32 * MT;       // every wave its own rows
    const int et = OWNROWS ? (tid & 63) : tid;
    if (et < 32 * MT) {
      const int ci = mBase + et;
      f32x4 p = {1.f, 0.f, 1.f, 0.f};
      if (ci < M) {
        if (a.es1) { p.x = a.es1[ci]; p.y = a.eh1[ci]; }
        if (a.es2) { p.z = a.es2[ci]; p.w = a.eh2[ci]; }
      }
      Es[et] = p;
    }
    __syncthreads();
    const __amdgpu_buffer_rsrc_t rx1 = buf_rsrc(a.ex1 + (size_t)n * M * L, (wlive && need_x) ? nrem * M * L4 : 0);
    const __amdgpu_buffer_rsrc_t rx2 = buf_rsrc((has2 ? a.ex2 : a.ex1) + (size_t)n * M * L, (wlive && has2) ? nrem * M * L4 : 0);
    const __amdgpu_buffer_rsrc_t ro2 = buf_rsrc((a.out2 ? a.out2 : a.out) + (size_t)n * M * L, (wlive && a.out2) ? nrem * M * L4 : 0);
    constexpr int G = MT * 4;                       // row groups of the wave's tile
    constexpr int PD = EPD > 0 ? (EPD < G ? EPD : G) : 1;
    vq xa[PD][4], xb[(X2 || EPD == 0) ? PD : 1][4];
    auto fetch = [&](int g, int slot) {
      const int m = g >> 2, rb = (g & 3) * 4;
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int ci = mBase + 32 * m + mfma_row32(rb + rr, half);
        xa[slot][rr] = buf_load<NQ>(rx1, buf_rowoff(ci < M, ooff, ci * L4), 0);      // zeros when the input is not needed
        if constexpr (X2 || EPD == 0) xb[slot][rr] = buf_load<NQ>(rx2, buf_rowoff(ci < M, ooff, ci * L4), 0);
      }
    };
    if constexpr (EPD > 0) {
#pragma unroll
      for (int g = 0; g < PD; ++g) fetch(g, g);
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const int m = g >> 2, rb = (g & 3) * 4;
      const int slot = EPD > 0 ? g % PD : 0;
      if constexpr (EPD == 0) fetch(g, 0);
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int r = rb + rr;
        const int row = mfma_row32(r, half);
        const int ci = mBase + 32 * m + row;
        const f32x4 e = Es[32 * m + row];
        float u0 = 0.f, u1 = 0.f, u2 = 0.f;
        vq d1, d2;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
          float pre = fmaf(xa[slot][rr][q], e.x, e.y);
          float xbq = 0.f;
          if constexpr (X2 || EPD == 0) {
            xbq = xb[slot][rr][q];
            if (has2) pre += fmaf(xbq, e.z, e.w);
          }
          const float dv = (!a.erelu || pre > 0.f) ? acc[m][q][r] : 0.f;
          d1[q] = dv * e.x;
          d2[q] = dv * e.z;
          if (q >= skip) {
            u0 = fmaf(dv, xa[slot][rr][q], u0);
            u1 += dv;
            u2 = fmaf(dv, xbq, u2);
          }
        }
        p4_store<NQ>(d1, ro, buf_rowoff(ci < M, ooff, ci * L4), 0);
        if constexpr (X2 || EPD == 0) p4_store<NQ>(d2, ro2, buf_rowoff(ci < M, ooff, ci * L4), 0);   // zero-sized resource when there is no dx2
        if (sums) {
          const bool ok = ci < M && pok;
          Tw[row * 36 + l31] = ok ? u0 : 0.f;
          Tw[32 * 36 + row * 36 + l31] = ok ? u1 : 0.f;
          Tw[2 * 32 * 36 + row * 36 + l31] = ok ? u2 : 0.f;
        }
      }
      if constexpr (EPD > 0) {
        __builtin_amdgcn_sched_barrier(0);
        if (g + PD < G) fetch(g + PD, slot);
        __builtin_amdgcn_sched_barrier(0);
      }
      if ((g & 3) == 3 && sums) {
        wave_lds_sync();
        float s0 = tile36_rowsum<float>(Tw, half, l31);
        float s1 = tile36_rowsum<float>(Tw + 32 * 36, half, l31);
        float s2 = tile36_rowsum<float>(Tw + 2 * 32 * 36, half, l31);
        wave_lds_sync();
        s0 += __shfl_xor(s0, 32, 64);
        s1 += __shfl_xor(s1, 32, 64);
        s2 += __shfl_xor(s2, 32, 64);
        if (half == 0) {
          if constexpr (OWNROWS) {
            const int ci = mBase + 32 * m + l31;
            if (ci < M) {
              float* o = a.ipart + ((size_t)grp * M + ci) * 3;
              o[0] = s0; o[1] = s1; o[2] = s2;
            }
          } else {
            float* q = Ss + ((wave * MT + m) * 32 + l31) * 3;
            q[0] = s0; q[1] = s1; q[2] = s2;
          }
        }
      }
    }
    if (sums && !OWNROWS) {
      __syncthreads();
      if (tid < 32 * MT) {
        const int ci = mBase + tid;
        if (ci < M) {
          float v0 = 0.f, v1 = 0.f, v2 = 0.f;
#pragma unroll
          for (int w = 0; w < 4; ++w) {
            const float* q = Ss + ((w * MT * 32) + tid) * 3;
            v0 += q[0]; v1 += q[1]; v2 += q[2];
          }
          float* o = a.ipart + ((size_t)grp * M + ci) * 3;
          o[0] = v0; o[1] = v1; o[2] = v2;
        }
      }
    }
  }
}

// KSP (round 6): the four waves of a workgroup share ONE position tile and split the K loop (whole prefetch rounds each);
// their accumulators meet in LDS and wave 0 runs the epilogue.  For the tiny-plane launches (the dynamic-adjacency
// projections: n x 32 positions, K = 128 .. 288): 64 wave tiles x 9 row blocks left the chip at 576 waves each walking
// K / 2 dependent k-steps (18-21 us for 0.6 GFLOP); split four ways the chain is a quarter as long on four times the waves.
//
// The body is a device function of (arguments, block id, LDS): k_pw4 runs it on its own grid, and a launch that HOSTS a
// small conv (the guest blocks below) runs the <1, 2, 0, 16, EPI> body in its leading workgroups — same k order, same
// accumulator start, same epilogue: a guest gives the bits of its stand-alone launch.
template <int MT, int NQ, int MODE, int PD, int EPI, bool KSP = false>
__device__ __forceinline__ void p4_block(const Pw4Args& a, const int bid, float* lds) {
  typedef typename buf_vec<NQ>::T vq;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = lane >> 5, l31 = lane & 31;
  // XCD-aware decode: the cc workgroups that read the same position tiles (one per 32*MT output channels) take
  // consecutive slots of one XCD (blockIdx % 8), so the re-reads are served by that XCD's L2
  const int ngrp = KSP ? a.WT : (a.WT + 3) >> 2;
  const int id = bid, xcd = id & 7, slot = id >> 3;
  const int cz = slot % a.cc;
  const int grp = (slot / a.cc) * 8 + xcd;
  if (grp >= ngrp) return;
  const int mBase = cz * 32 * MT;
  const int K = a.K, M = a.M, L = a.L;
  const int Kpad = a.Kpad, KP = Kpad + 1;
  float* Ws = lds;                                                       // [32*MT][KP], zero beyond (M, K)
  f32x4* Ps = reinterpret_cast<f32x4*>(lds + ((32 * MT * KP + 2 + 3) & ~3));  // [Kpad + 2] (s1, h1, s2, h2)

  // Position tiles run over the planes of all samples back to back (a tile may straddle samples: L % NQ == 0, so a lane's
  // NQ positions never do): no per-sample tail tile — at L = 400 (256 channels, 16 frames) per-sample tiling left
  // 22 % of the MFMA work on padding.  The wave's buffer resources start at its first sample n; a lane adds ds sample
  // strides in its vector offset.
  const int wt = KSP ? grp : grp * 4 + wave;
  const bool wlive = wt < a.WT;
  // Ragged planes (L % NQ != 0: K400's 25 x 17 and CTR-GCN's 25 x 25 planes): the tile walks Lq = L rounded up to NQ
  // positions per plane, and the plane's last run is moved back to END at the plane's end — it overlaps the run before it
  // by `skip` positions, which both lanes compute and store identically and only the earlier one adds to the per-channel
  // sums.  No load or store ever leaves the plane (a run reaching into the next row would need a per-element bounds
  // check: a 16-byte buffer load that straddles the end of its resource returns zeros from its second dword on, measured),
  // at the price of dword-aligned 16-byte accesses (legal and within 4 % of aligned ones on gfx950:
  // tools/probes/unaligned_b128.hip).
  const int Lq = a.Lq;
  const int g0 = (wlive ? wt : 0) * (32 * NQ);          // < 2^31 (p4_plan)
  const int n = g0 / Lq;
  int pos = g0 - n * Lq + l31 * NQ;
  int ds = 0;
  while (pos >= Lq) { pos -= Lq; ++ds; }
  const bool pok = wlive && n + ds < a.n;
  int skip = 0;
  if (L - pos < NQ) { skip = NQ - (L - pos); pos = L - NQ; }
  const int L4 = L * 4;
  const int nrem = a.n - n < a.span ? a.n - n : a.span;     // samples the wave can touch
  const int voff = pok ? ds * K * L4 + (half * L + pos) * 4 : BUF_OOB;
  const __amdgpu_buffer_rsrc_t r1 = buf_rsrc(a.b1 + (size_t)n * K * L, wlive ? nrem * K * L4 : 0);
  const __amdgpu_buffer_rsrc_t r2 = buf_rsrc((MODE == 2 ? a.b2 : a.b1) + (size_t)n * K * L, (wlive && MODE == 2) ? nrem * K * L4 : 0);

  f32x16 acc[MT][NQ];
  const float lo = a.relu ? 0.f : -__builtin_inff();
  // this wave's k-steps: all of them, or (KSP) its share of the Kpad / (2 PD) prefetch rounds
  const int KS = a.Kpad >> 1;                      // k-steps (2 channels each), a multiple of PD
  const int KSr = (K + 1) >> 1;                    // k-steps that hold real channels
  int ks0 = 0, ks1 = KS;
  if constexpr (KSP) {
    const int U = KS / PD;
    ks0 = (U * wave / 4) * PD;
    ks1 = (U * (wave + 1) / 4) * PD;
  }
  const int kse = ks1 < KSr ? ks1 : KSr;           // loads past it: out of range (zeros, no traffic)
  // ---- weights: global -> registers (all loads of a batch issued together), operand prefetch, then LDS ----
  constexpr int WB = 16;
  const bool mfast = a.w_ldm == 1;                 // A = W^T (data gradient): m is the contiguous index of w
  // element e of this thread: k fast: (r, k) = ((tid>>4) + 16*(e % (2*MT)), (tid&15) + 16*(e / (2*MT)))
  //                           m fast: (r, k) = ((tid&31) + 32*(e % MT),     (tid>>5) + 8*(e / MT))
  const int nel = mfast ? (Kpad >> 3) * MT : (Kpad >> 4) * 2 * MT;
  vq buf1[PD], buf2[MODE == 2 ? PD : 1];
  for (int e0 = 0; e0 < nel; e0 += WB) {
    float tmp[WB];
#pragma unroll
    for (int j = 0; j < WB; ++j) {
      const int e = e0 + j;
      int r, k;
      if (mfast) { r = (tid & 31) + 32 * (e % MT); k = (tid >> 5) + 8 * (e / MT); }
      else { r = (tid >> 4) + 16 * (e % (2 * MT)); k = (tid & 15) + 16 * (e / (2 * MT)); }
      const int m = mBase + r;
      tmp[j] = (e < nel && m < M && k < K) ? a.w[(size_t)m * a.w_ldm + (size_t)k * a.w_ldk] : 0.f;
    }
    if (e0 == 0) {
#pragma unroll
      for (int u = 0; u < PD; ++u) {
        const int s0 = ks0 + u < kse ? 2 * (ks0 + u) * L4 : BUF_OOB;   // (channels past K: out of range, zeros)
        buf1[u] = buf_load<NQ>(r1, voff, s0);
        if constexpr (MODE == 2) buf2[u] = buf_load<NQ>(r2, voff, s0);
      }
    }
#pragma unroll
    for (int j = 0; j < WB; ++j) {
      const int e = e0 + j;
      int r, k;
      if (mfast) { r = (tid & 31) + 32 * (e % MT); k = (tid >> 5) + 8 * (e / MT); }
      else { r = (tid >> 4) + 16 * (e % (2 * MT)); k = (tid & 15) + 16 * (e / (2 * MT)); }
      if (e < nel) Ws[r * KP + k] = tmp[j];
    }
  }
  // accumulators start at the bias of their output row (forward), so the epilogue has no per-row loads
  // (loaded here, with the affine table: after the barrier they were a memory round trip of their own)
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row = mBase + 32 * m + mfma_row32(i, half);
      const float b0 = (EPI == 0 && a.bias && row < M && (!KSP || wave == 0)) ? a.bias[row] : 0.f;
#pragma unroll
      for (int q = 0; q < NQ; ++q) acc[m][q][i] = b0;
    }

  if (MODE != 0) {
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
  block_lds_sync();                    // raw barrier: the operand prefetch stays in flight

  // Software pipeline, pinned with scheduling barriers.  Step ks: start the LDS reads of step ks+1 (A fragment, affine
  // row; double-buffered by step parity), apply the affine to the operand loaded PD steps ago, run the MT*NQ MFMAs, then
  // re-issue that operand buffer's load for step ks+PD (after the MFMAs: the buffer registers are dead by then, so the
  // load lands in place).  Left to itself the compiler sinks all PD loads to the end of the unrolled body and waits for
  // the first of them at the top of the next one — or, with the load ahead of the MFMAs, rotates the PD buffers through
  // v_mov chains behind a vmcnt(0) (profiles/r02: matrix pipe 61 % busy at 256 -> 256 channels).
  float avb[2][MT];
  f32x4 pb[2] = {{1.f, 0.f, 1.f, 0.f}, {1.f, 0.f, 1.f, 0.f}};
#pragma unroll
  for (int m = 0; m < MT; ++m) avb[0][m] = Ws[(32 * m + l31) * KP + 2 * ks0 + half];
  if (MODE != 0) pb[0] = Ps[2 * ks0 + half];
  for (int base = ks0; base < ks1; base += PD) {
#pragma unroll
    for (int u = 0; u < PD; ++u) {
      const int ks = base + u;
      const int cur = u & 1, nxt = cur ^ 1;                              // PD is even: the parity survives the back edge
      const int kn = 2 * (ks + 1) + half;                                // last step: reads the LDS pad, never used
#pragma unroll
      for (int m = 0; m < MT; ++m) avb[nxt][m] = Ws[(32 * m + l31) * KP + kn];
      if (MODE != 0) pb[nxt] = Ps[kn];
      vq b = buf1[u];
      if (MODE != 0) {
        const f32x4 p = pb[cur];
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
          float v = fmaf(b[q], p.x, p.y);
          if constexpr (MODE == 2) v += fmaf(buf2[u][q], p.z, p.w);
          b[q] = fmaxf(v, lo);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int q = 0; q < NQ; ++q) acc[m][q] = __builtin_amdgcn_mfma_f32_32x32x2f32(avb[cur][m], b[q], acc[m][q], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      // past K: the scalar offset jumps out of the buffer's range (zeros, no traffic: the bounds check covers it)
      const int sn = ks + PD < kse ? 2 * (ks + PD) * L4 : BUF_OOB;
      buf1[u] = buf_load<NQ>(r1, voff, sn);
      if constexpr (MODE == 2) buf2[u] = buf_load<NQ>(r2, voff, sn);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  __syncthreads();                                 // every wave is done with Ws / Ps: LDS is reused below

  if constexpr (KSP) {
    // the K shares meet: waves 1..3 park their accumulators ([wave][register][lane]: conflict-free), wave 0 adds them in
    // a fixed order (deterministic) and alone runs the epilogue — the others go through it as dead waves (no stores,
    // zero sums: what a partly empty last workgroup's waves do)
    float* Rs = lds;                               // [3][MT * NQ * 16][64]
    if (wave != 0) {
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int q = 0; q < NQ; ++q)
#pragma unroll
          for (int i = 0; i < 16; ++i) Rs[(((wave - 1) * MT * NQ + m * NQ + q) * 16 + i) * 64 + lane] = acc[m][q][i];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int w = 0; w < 3; ++w)
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
          for (int q = 0; q < NQ; ++q)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[m][q][i] += Rs[((w * MT * NQ + m * NQ + q) * 16 + i) * 64 + lane];
    }
    __syncthreads();
  }
  const bool elive = KSP ? (wlive && wave == 0) : wlive;
  const P4Tile tile = {wave, half, l31, tid, mBase, n, nrem, ds, pos, grp, elive, KSP ? (pok && wave == 0) : pok, skip};
  if constexpr (EPI == 1) {
    // (operand prefetch of the data-gradient epilogue: two row groups ahead — k_pw4's waves keep their PD operand slots
    // next to MT*NQ accumulator tiles, there is room for two)
    if (a.ex2) p4_epilogue<MT, NQ, EPI, false, 4, (MT * NQ >= 8 || (MT == 2 && NQ == 2) ? 1 : 2), true>(a, acc, lds, tile);
    else p4_epilogue<MT, NQ, EPI, false, 4, (MT * NQ >= 8 || (MT == 2 && NQ == 2) ? 1 : 2), false>(a, acc, lds, tile);
  } else {
    p4_epilogue<MT, NQ, EPI, false>(a, acc, lds, tile);
  }
}

// ---- guest blocks: a small conv in the leading workgroups of a launch that is there anyway --------------------------------
// The dynamic-adjacency projections (three mean-pooled 1x1 convs on a (n, Ci, 1, 32) "clip", k_pw4<1, 2, 0, 16, EPI>) are
// 48-144 workgroups bound by their own prologue / K chain / epilogue; nothing but launch order puts them behind the `pre`
// conv.  The bn_jobs.h pattern, extended from BatchNorm jobs to one conv body: the `pre` conv's launch takes the guest's
// arguments and runs p4_block<1, 2, 0, 16, EPI> in its first `nblk` workgroups (LEADING: they start at t = 0, not in the
// host's tail; nblk is a multiple of 8, so the host's XCD decode sees the block ids of its stand-alone launch).  nblk = 0:
// no guest — grid and decode are the stand-alone launch's.  Only the kernels the shipped DS-STGCN step runs for the `pre`
// conv take the argument block (P4GuestArg); every other instantiation gets an empty struct and carries no guest code.

// the guest argument of an instantiation: the hosted conv (or "none": nblk = 0) for a host kernel, the empty struct otherwise
template <bool HOST>
inline P4GuestArg<HOST> p4_guest_arg(const P4Hosted* h) {
  if constexpr (HOST) {
    if (h) return h->g;
    P4Guest none = {};
    return none;
  } else {
    return P4NoGuest{};
  }
}

}  // namespace
