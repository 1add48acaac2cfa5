// K-C's host layer, shared by its four translation units (pwconv.hip, pw4.hip, wgrad.hip, bwd64.hip): the operand
// structs the dispatch functions hand down, and the ONE declaration of every function that crosses a file boundary inside
// the family.  None of these is part of the C ABI (include/dsgcn.h): they are hidden, the library exports none of them.
// The structs exist on the host only — a kernel argument struct (PwArgs, PwBwdArgs, Pw4Args, Wg2Args, BfArgs) is filled
// from them field by field, so its layout is its own.
#pragma once
#include "common.h"
#include "bn_jobs.h"

// the conv's virtual input  v = relu?( x1*s1+h1 (+ x2*s2+h2 | + x2) );  s1/h1, x2, s2/h2 may be NULL
struct KcIn {
  const float* x1; const float* s1; const float* h1;
  const float* x2; const float* s2; const float* h2;
  int relu;
};

// the backward's output-side operand  dz_eff = gz + A0 + B0*z  (A0/B0: the batch-statistics terms; either part may be NULL)
struct KcDz {
  const float* z; const float* gz; const float* A0; const float* B0;
};

struct P4Hosted;                                   // pw4_block.h: a guest conv planned as leading workgroups of a launch

#pragma GCC visibility push(hidden)

// ---- pw4.hip: the wide-load / GEMM forms.  The launchers return 1 = launched, 0 = not eligible (the caller falls back),
//      anything else = an error code.  guest / hosted: a conv to carry in the launch, *hosted = 1 when it did.
int dsgcn_p4_tuning(int key, int value);
int dsgcn_p4_groups(int n, int K, int M, int L, int epi);
int dsgcn_p4_terms(int n, int K, int M, int L, int epi);
int dsgcn_p4_guest_plan(const dsgcn_guest_conv* g, int epi, P4Hosted* h);
int dsgcn_p4_fwd(const KcIn& in, const float* w, const float* bias, float* z, float* partial, int n, int Ci, int Co, int L,
                 hipStream_t st, const void* ws, const dsgcn_guest_conv* guest, int* hosted);
int dsgcn_p4_fwd_hosts(int n, int Ci, int Co, int L, int have_ws, const dsgcn_guest_conv* guest);
int dsgcn_p4_dgrad(const KcIn& in, const float* w, const KcDz& d, float* dx1, float* dx2, float* ipart, int n, int Ci, int Co,
                   int L, hipStream_t st, const void* ws, const dsgcn_guest_conv* guest, int* hosted);
int dsgcn_p4_dgrad_hosts(int n, int Ci, int Co, int L, int have_ws, const dsgcn_guest_conv* guest);
int dsgcn_p4_group_ok(int n, int Ci, int Co, int L);
int dsgcn_p4_fwd_group(const float* const* x1, const float* const* s1, const float* const* h1, int relu,
                       const float* const* w, float* const* z, int ng, int n, int Ci, int Co, int L, hipStream_t st);
int dsgcn_p4_dgrad_group(const float* const* x1, const float* const* s1, const float* const* h1, int relu,
                         const float* const* w, const float* const* gz, float* const* dx1, float* const* ipart, int ng, int n,
                         int Ci, int Co, int L, hipStream_t st);
size_t dsgcn_p4_ws_bytes(int n, int Ci, int Co, int L);
int dsgcn_p4_wsplit(const float* w, int Ci, int Co, void* out, hipStream_t st);
int dsgcn_p4_wsplit_multi(const float* const* w, void* const* out, const int* Ci, const int* Co, int njobs, hipStream_t st);

// ---- bwd64.hip: the one-pass narrow backward
int dsgcn_bwd64_tuning(int value);
int dsgcn_bwd64_splits(int n, int Ci, int Co, int L);
int dsgcn_bwd64_terms(int n, int Ci, int Co, int L);
int dsgcn_bwd64(const KcIn& in, const float* w, const KcDz& d, float* dx, float* dx2, float* dwp, float* dbp, int pstride,
                float* ipart, int n, int Ci, int Co, int L, hipStream_t st, const dsgcn_guest_conv* guest, int* hosted);
int dsgcn_bwd64_hosts(int n, int Ci, int Co, int L, const dsgcn_guest_conv* guest);

// ---- wgrad.hip: the blocked weight gradient.  jobs: BatchNorm coefficient jobs riding as extra workgroups.  ngroup > 1: up
//      to three convs of one shape in the launch, from the pointer tables (in / d / dwp / dbp then describe the first).
int dsgcn_wg2_tuning(int key, int value);
int dsgcn_wg2_splits(int n, int Ci, int Co, int L);
int dsgcn_wg2_terms(int n, int Ci, int Co, int L);
int dsgcn_wg2(const KcIn& in, const KcDz& d, float* dwp, float* dbp, int pstride, int n, int Ci, int Co, int L, hipStream_t st,
              const BnCoefTable* jobs, int ngroup = 0, const float* const* gx1 = nullptr, const float* const* gs1 = nullptr,
              const float* const* gh1 = nullptr, const float* const* ggz = nullptr, float* const* gdwp = nullptr,
              float* const* gdbp = nullptr);

#pragma GCC visibility pop
