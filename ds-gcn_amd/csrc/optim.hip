// Optimizer updates that know where one parameter tensor ends and the next begins: mmcv's build_optimizer with any
// paramwise_cfg (a rate and a weight decay per parameter tensor) and torch.optim.Adam / AdamW, over the two unpadded flat
// fp32 buffers, in ONE launch whatever the number of tensors or groups (two with the total-norm clip: k_grad_norm of
// clip.hip first).
//   table      ends[t]   ascending end offsets of the tensors in the flat buffer (ends[ntens - 1] == n)
//              group[t]  the tensor's group id, or DSGCN_OPTIM_SKIP: p and the optimizer state stay untouched bit for bit
//                        (a parameter that never receives a gradient: torch skips a .grad of None)
//              first[c]  the tensor that holds element c * 4096, the first one of workgroup c's chunk (one more entry for
//                        the end of the last chunk): a thread searches the few tensors of its own chunk only
//              lr[g], wd[g]  fp64 per group, as torch keeps them in Python floats; lr is rewritten by the host per iteration
//   k_optim    a workgroup takes 1024 consecutive float4; a float4 inside one tensor resolves its group once, one that
//              straddles a boundary walks the table per element.  SGD: sgd_update.h with the group's rate and decay.
//              Adam: torch's single-tensor order (amsgrad=False, maximize=False), every operation rounded on its own.
//   DEV forms  (the *_hyper entry points) SGD's momentum / Adam's beta1 is read from one fp64 device element instead of the
//              kernel arguments: a replayed launch follows a momentum schedule.  Same arithmetic, same bits at a same value.
// The Adam step count is one int per WORKGROUP (all equal): workgroup c reads step[c] and writes step[c] + 1, so no
// workgroup reads what another one of the same launch writes, and a replayed launch advances the count by itself.
// Fixed grid, fixed order, no atomics: the same bits on every run.
#include "common.h"
#include "grad_norm.h"
#include "sgd_update.h"

namespace {

constexpr int OP_NT = 256;
constexpr int OP_VPT = 4;                           // float4 per thread
constexpr int OP_CHUNK4 = OP_NT * OP_VPT;           // float4 per workgroup
constexpr int OP_CHUNK = 4 * OP_CHUNK4;             // elements per workgroup: 4096
constexpr int OP_MAXG = 256;                        // groups: one thread fills one row of the coefficient table

struct OpTable {
  const int* ends;
  const int* group;
  const int* first;
  const double* lr;
  const double* wd;
  int ntens, groups;
};

struct OpClip {
  const double* partial;
  float* grad_norm;
  int rows, inf;
  float max_norm;
};

struct OpHyper {
  int* step;                                        // Adam: one counter per workgroup
  double b1, b2;                                    // Adam
  float eps;                                        // Adam
  int decoupled;                                    // Adam: AdamW's p *= 1 - lr wd instead of g += wd p
  float mom;                                        // SGD
  int nesterov;                                     // SGD
  const double* dev;                                // DEV kernels: momentum (SGD) / beta1 (Adam) in device memory
};

// per-workgroup constants of the Adam update
struct OpAdamConst {
  float w1, w2, b2, bc2_sqrt, eps;
  int decoupled;
};

__device__ __forceinline__ double op_ipow(double x, int k) {       // x^k, k >= 0, by binary powering in fp64
  double r = 1.;
  while (k) {
    if (k & 1) r *= x;
    x *= x;
    k >>= 1;
  }
  return r;
}

// smallest t in [lo, hi] with ends[t] > e (ends[hi] > e by construction of first[])
__device__ __forceinline__ int op_find(const int* __restrict__ ends, int lo, int hi, int e) {
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (ends[mid] > e) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

// torch/optim/adam.py _single_tensor_adam on one element; c0 = lr / bc1, c1 = wd, c2 = 1 - lr wd
__device__ __forceinline__ float op_adam(float pv, float gv, float& mv, float& vv, float c0, float c1, float c2,
                                         const OpAdamConst& k) {
  if (k.decoupled) pv = __fmul_rn(pv, c2);
  else gv = fmaf(c1, pv, gv);
  mv = fmaf(k.w1, __fsub_rn(gv, mv), mv);                          // lerp(m, g, 1 - beta1)
  vv = fmaf(__fmul_rn(k.w2, gv), gv, __fmul_rn(k.b2, vv));         // v * beta2 + ((1 - beta2) g) g
  const float denom = __fadd_rn(__fdiv_rn(__fsqrt_rn(vv), k.bc2_sqrt), k.eps);
  return __fsub_rn(pv, __fdiv_rn(__fmul_rn(c0, mv), denom));
}

// s1: SGD's momentum buffer (may be NULL) / Adam's exp_avg;  s2: Adam's exp_avg_sq
// DEV: hy.dev[0] (fp64, one scalar load per wave) stands in for hy.mom (rounded to fp32 as the by-value argument is) resp.
// hy.b1 — a replayed launch follows a momentum schedule as it follows the rates.  SGD at a momentum of exactly 0 leaves the
// buffer alone, as the by-value form does when its caller drops the pointer and as torch does (`if momentum != 0`).
template <bool ADAM, bool CLIP, bool DEV>
__global__ __launch_bounds__(OP_NT) void k_optim(float* __restrict__ p, float* __restrict__ g, float* __restrict__ s1_arg,
                                                 float* __restrict__ s2, OpTable tab, OpClip clip, OpHyper hy, long n4,
                                                 long n) {
  __shared__ double red[CLIP ? OP_NT : 1];
  __shared__ float c0s[OP_MAXG], c1s[OP_MAXG], c2s[OP_MAXG];
  const int tid = threadIdx.x;
  if (DEV) {
    const double* __restrict__ dev = hy.dev;
    if (ADAM) hy.b1 = dev[0];
    else hy.mom = uniform_f32((float)dev[0]);
  }
  float* __restrict__ s1 = (DEV && !ADAM && hy.mom == 0.f) ? nullptr : s1_arg;
  float coef = 1.f;
  if (CLIP) {
    float total;
    coef = gn_clip_coef(clip.partial, clip.rows, clip.inf, clip.max_norm, red, tid, total);
    if (blockIdx.x == 0 && tid == 0) clip.grad_norm[0] = total;
  }
  OpAdamConst ak = {};
  int done = 0;
  if (ADAM) {
    done = hy.step[blockIdx.x];                                    // updates so far; this one is number done + 1
    ak.w1 = (float)(1. - hy.b1);
    ak.w2 = (float)(1. - hy.b2);
    ak.b2 = (float)hy.b2;
    ak.bc2_sqrt = (float)sqrt(1. - op_ipow(hy.b2, done + 1));
    ak.eps = hy.eps;
    ak.decoupled = hy.decoupled;
  }
  if (tid < tab.groups) {
    const double lr = tab.lr[tid], wd = tab.wd[tid];
    if (ADAM) {
      c0s[tid] = (float)(lr / (1. - op_ipow(hy.b1, done + 1)));
      c2s[tid] = (float)(1. - lr * wd);
    } else {
      c0s[tid] = (float)lr;
    }
    c1s[tid] = (float)wd;
  }
  __syncthreads();
  if (ADAM && tid == 0) hy.step[blockIdx.x] = done + 1;            // after every thread of the workgroup has read it
  const bool has_buf = s1 != nullptr;
  const int last = tab.ntens - 1;
  const int lo = min(max(tab.first[blockIdx.x], 0), last);
  const int hi = min(max(tab.first[blockIdx.x + 1], lo), last);

  // one element: gi = its tensor's group id
  auto one = [&](int gi, float& pv, float gv, float& av, float& bv) {
    if ((unsigned)gi >= (unsigned)tab.groups) return;              // DSGCN_OPTIM_SKIP
    if (ADAM) pv = op_adam(pv, gv, av, bv, c0s[gi], c1s[gi], c2s[gi], ak);
    else pv = sgd_update(pv, gv, av, has_buf, c0s[gi], hy.mom, c1s[gi], hy.nesterov);
  };
  // the float4 of elements e0 .. e0 + 3
  auto four = [&](int e0, f32x4& pv, f32x4& gv, f32x4& av, f32x4& bv) {
    int t = op_find(tab.ends, lo, hi, e0);
    int end = tab.ends[t], gi = tab.group[t];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (e0 + e >= end) {                                         // a boundary inside this float4
        while (t < hi && tab.ends[t] <= e0 + e) ++t;
        end = tab.ends[t];
        gi = tab.group[t];
      }
      float pe = pv[e], ae = av[e], be = bv[e];
      gv[e] = __fmul_rn(gv[e], coef);                              // rounded on its own; coef == 1: g itself
      one(gi, pe, gv[e], ae, be);
      pv[e] = pe;
      av[e] = ae;
      bv[e] = be;
    }
  };
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  const long i0 = (long)blockIdx.x * OP_CHUNK4 + tid;
  if (i0 + (OP_VPT - 1) * OP_NT < n4) {                            // all OP_VPT float4 of this thread exist: loads first
    f32x4 pv[OP_VPT], gv[OP_VPT], av[OP_VPT], bv[OP_VPT];
#pragma unroll
    for (int k = 0; k < OP_VPT; ++k) {
      const long i = i0 + k * OP_NT;
      pv[k] = reinterpret_cast<f32x4*>(p)[i];
      gv[k] = reinterpret_cast<f32x4*>(g)[i];
      av[k] = s1 ? reinterpret_cast<f32x4*>(s1)[i] : zero;
      bv[k] = ADAM ? reinterpret_cast<f32x4*>(s2)[i] : zero;
    }
#pragma unroll
    for (int k = 0; k < OP_VPT; ++k) {
      const long i = i0 + k * OP_NT;
      four((int)(4 * i), pv[k], gv[k], av[k], bv[k]);
      reinterpret_cast<f32x4*>(p)[i] = pv[k];
      if (CLIP) reinterpret_cast<f32x4*>(g)[i] = gv[k];
      if (s1) reinterpret_cast<f32x4*>(s1)[i] = av[k];
      if (ADAM) reinterpret_cast<f32x4*>(s2)[i] = bv[k];
    }
    return;
  }
  for (int k = 0; k < OP_VPT; ++k) {
    const long i = i0 + (long)k * OP_NT;
    if (i < n4) {
      f32x4 pv = reinterpret_cast<f32x4*>(p)[i];
      f32x4 gv = reinterpret_cast<f32x4*>(g)[i];
      f32x4 av = s1 ? reinterpret_cast<f32x4*>(s1)[i] : zero;
      f32x4 bv = ADAM ? reinterpret_cast<f32x4*>(s2)[i] : zero;
      four((int)(4 * i), pv, gv, av, bv);
      reinterpret_cast<f32x4*>(p)[i] = pv;
      if (CLIP) reinterpret_cast<f32x4*>(g)[i] = gv;
      if (s1) reinterpret_cast<f32x4*>(s1)[i] = av;
      if (ADAM) reinterpret_cast<f32x4*>(s2)[i] = bv;
    } else if (i == n4) {                                          // the tail (n % 4 elements)
      int t = op_find(tab.ends, lo, hi, (int)(4 * n4));
      for (long j = 4 * n4; j < n; ++j) {
        while (t < hi && tab.ends[t] <= (int)j) ++t;
        float pe = p[j], ae = s1 ? s1[j] : 0.f, be = ADAM ? s2[j] : 0.f;
        const float gc = __fmul_rn(g[j], coef);
        one(tab.group[t], pe, gc, ae, be);
        p[j] = pe;
        if (CLIP) g[j] = gc;
        if (s1) s1[j] = ae;
        if (ADAM) s2[j] = be;
      }
    }
  }
}

bool op_misaligned(const void* ptr, uintptr_t mask) { return ((uintptr_t)ptr & mask) != 0; }

// the checks every update entry point shares; 0 = launchable
int op_check(const float* p, const float* g, const OpTable& tab, long long n) {
  if (!p || !g || !tab.ends || !tab.group || !tab.first || !tab.lr || !tab.wd || n <= 0 || tab.ntens <= 0 || tab.groups <= 0)
    return DSGCN_EINVAL;
  if (op_misaligned(p, 15) || op_misaligned(g, 15) || op_misaligned(tab.ends, 3) || op_misaligned(tab.group, 3) ||
      op_misaligned(tab.first, 3) || op_misaligned(tab.lr, 7) || op_misaligned(tab.wd, 7))
    return DSGCN_EINVAL;
  if (tab.ntens > n) return DSGCN_EINVAL;                           // every tensor holds at least one element
  if (tab.groups > OP_MAXG || n > 0x7fffffffLL) return DSGCN_EUNSUPPORTED;
  return 0;
}

int op_check_clip(const OpClip& c) {
  if (!c.partial || !c.grad_norm || c.rows <= 0 || !(c.max_norm >= 0.f)) return DSGCN_EINVAL;
  if (op_misaligned(c.partial, 7) || op_misaligned(c.grad_norm, 3)) return DSGCN_EINVAL;
  return 0;
}

template <bool ADAM, bool DEV>
int op_launch(float* p, float* g, float* s1, float* s2, const OpTable& tab, const OpClip* clip, const OpHyper& hy,
              long long n, void* stream) {
  const long n4 = (long)(n / 4);
  const unsigned blocks = (unsigned)(n4 / OP_CHUNK4 + 1);           // the thread with float4 index n4 takes the tail
  if (clip)
    hipLaunchKernelGGL((k_optim<ADAM, true, DEV>), dim3(blocks), dim3(OP_NT), 0, (hipStream_t)stream, p, g, s1, s2, tab, *clip, hy,
                       n4, (long)n);
  else
    hipLaunchKernelGGL((k_optim<ADAM, false, DEV>), dim3(blocks), dim3(OP_NT), 0, (hipStream_t)stream, p, g, s1, s2, tab, OpClip{},
                       hy, n4, (long)n);
  DSGCN_LAUNCH_CHECK();
  return 0;
}

// hyper (DEV forms): buf is required whatever the value turns out to be — a schedule may pass through 0 and leave it again
int op_sgd(float* p, float* g, float* buf, const OpTable& tab, const OpClip* clip, float momentum, const double* hyper,
           int nesterov, long long n, void* stream) {
  int rc = op_check(p, g, tab, n);
  if (rc) return rc;
  if (hyper) {
    if (!buf || op_misaligned(buf, 15) || op_misaligned(hyper, 7)) return DSGCN_EINVAL;
    if (clip && (rc = op_check_clip(*clip))) return rc;
    OpHyper hy = {};
    hy.nesterov = nesterov;
    hy.dev = hyper;
    return op_launch<false, true>(p, g, buf, nullptr, tab, clip, hy, n, stream);
  }
  if (!(momentum >= 0.f) || (momentum != 0.f && !buf) || op_misaligned(buf, 15)) return DSGCN_EINVAL;
  if (clip && (rc = op_check_clip(*clip))) return rc;
  OpHyper hy = {};
  hy.mom = momentum;
  hy.nesterov = nesterov;
  return op_launch<false, false>(p, g, momentum != 0.f ? buf : nullptr, nullptr, tab, clip, hy, n, stream);
}

// hyper != NULL (DEV forms): beta1 is read from it on the device and the argument beta1 is not looked at
int op_adam(float* p, float* g, float* m, float* v, int* step, const OpTable& tab, const OpClip* clip, double beta1,
            const double* hyper, double beta2, float eps, int decoupled, long long n, void* stream) {
  int rc = op_check(p, g, tab, n);
  if (rc) return rc;
  if (!m || !v || !step || op_misaligned(m, 15) || op_misaligned(v, 15) || op_misaligned(step, 3)) return DSGCN_EINVAL;
  if (hyper ? op_misaligned(hyper, 7) : !(beta1 >= 0. && beta1 < 1.)) return DSGCN_EINVAL;
  if (!(beta2 >= 0. && beta2 < 1.) || !(eps >= 0.f)) return DSGCN_EINVAL;
  if (clip && (rc = op_check_clip(*clip))) return rc;
  OpHyper hy = {};
  hy.step = step;
  hy.b1 = beta1;
  hy.b2 = beta2;
  hy.eps = eps;
  hy.decoupled = decoupled ? 1 : 0;
  hy.dev = hyper;
  if (hyper) return op_launch<true, true>(p, g, m, v, tab, clip, hy, n, stream);
  return op_launch<true, false>(p, g, m, v, tab, clip, hy, n, stream);
}

}  // namespace

extern "C" {

int dsgcn_optim_chunks(long long n) {
  if (n <= 0) return DSGCN_EINVAL;
  if (n > 0x7fffffffLL) return DSGCN_EUNSUPPORTED;
  return (int)(n / OP_CHUNK + 1);
}

int dsgcn_optim_table(const int* ends, const int* group, int ntens, const double* wd, int groups, long long n, int* first) {
  if (!ends || !group || !wd || !first || ntens <= 0 || groups <= 0 || n <= 0) return DSGCN_EINVAL;
  if (groups > OP_MAXG || n > 0x7fffffffLL) return DSGCN_EUNSUPPORTED;
  int prev = 0;
  for (int t = 0; t < ntens; ++t) {
    if (ends[t] <= prev || group[t] < -1 || group[t] >= groups) return DSGCN_EINVAL;     // empty tensors have no row
    prev = ends[t];
  }
  if (prev != n) return DSGCN_EINVAL;
  for (int k = 0; k < groups; ++k)
    if (!(wd[k] >= 0.) || wd[k] > 3.4e38) return DSGCN_EINVAL;
  const int chunks = dsgcn_optim_chunks(n);
  int t = 0;
  for (int c = 0; c <= chunks; ++c) {
    long long e = (long long)c * OP_CHUNK;
    if (e > n - 1) e = n - 1;
    while (ends[t] <= e) ++t;
    first[c] = t;
  }
  return 0;
}

int dsgcn_sgd_group_step(float* p, float* g, float* buf, const int* ends, const int* group, const int* first, int ntens,
                         const double* lr, const double* wd, int groups, float momentum, int nesterov, long long n,
                         void* stream) {
  const OpTable tab = {ends, group, first, lr, wd, ntens, groups};
  return op_sgd(p, g, buf, tab, nullptr, momentum, nullptr, nesterov, n, stream);
}

int dsgcn_sgd_group_step_clip(float* p, float* g, float* buf, const int* ends, const int* group, const int* first, int ntens,
                              const double* lr, const double* wd, int groups, const double* partial, int rows,
                              int norm_type, float max_norm, float* grad_norm_out, float momentum, int nesterov,
                              long long n, void* stream) {
  if (norm_type != 0 && norm_type != 2) return DSGCN_EINVAL;
  const OpTable tab = {ends, group, first, lr, wd, ntens, groups};
  const OpClip clip = {partial, grad_norm_out, rows, norm_type == 0 ? 1 : 0, max_norm};
  return op_sgd(p, g, buf, tab, &clip, momentum, nullptr, nesterov, n, stream);
}

int dsgcn_adam_step(float* p, float* g, float* m, float* v, int* step, const int* ends, const int* group, const int* first,
                    int ntens, const double* lr, const double* wd, int groups, double beta1, double beta2, float eps,
                    int decoupled, long long n, void* stream) {
  const OpTable tab = {ends, group, first, lr, wd, ntens, groups};
  return op_adam(p, g, m, v, step, tab, nullptr, beta1, nullptr, beta2, eps, decoupled, n, stream);
}

int dsgcn_adam_step_clip(float* p, float* g, float* m, float* v, int* step, const int* ends, const int* group,
                         const int* first, int ntens, const double* lr, const double* wd, int groups, const double* partial,
                         int rows, int norm_type, float max_norm, float* grad_norm_out, double beta1, double beta2,
                         float eps, int decoupled, long long n, void* stream) {
  if (norm_type != 0 && norm_type != 2) return DSGCN_EINVAL;
  const OpTable tab = {ends, group, first, lr, wd, ntens, groups};
  const OpClip clip = {partial, grad_norm_out, rows, norm_type == 0 ? 1 : 0, max_norm};
  return op_adam(p, g, m, v, step, tab, &clip, beta1, nullptr, beta2, eps, decoupled, n, stream);
}

// ---- the same four with momentum / beta1 in device memory: hyper[0], fp64, NULL is DSGCN_EINVAL ------------------------
int dsgcn_sgd_group_step_hyper(float* p, float* g, float* buf, const int* ends, const int* group, const int* first, int ntens,
                               const double* lr, const double* wd, int groups, const double* hyper, int nesterov,
                               long long n, void* stream) {
  if (!hyper) return DSGCN_EINVAL;
  const OpTable tab = {ends, group, first, lr, wd, ntens, groups};
  return op_sgd(p, g, buf, tab, nullptr, 0.f, hyper, nesterov, n, stream);
}

int dsgcn_sgd_group_step_clip_hyper(float* p, float* g, float* buf, const int* ends, const int* group, const int* first,
                                    int ntens, const double* lr, const double* wd, int groups, const double* partial,
                                    int rows, int norm_type, float max_norm, float* grad_norm_out, const double* hyper,
                                    int nesterov, long long n, void* stream) {
  if (!hyper || (norm_type != 0 && norm_type != 2)) return DSGCN_EINVAL;
  const OpTable tab = {ends, group, first, lr, wd, ntens, groups};
  const OpClip clip = {partial, grad_norm_out, rows, norm_type == 0 ? 1 : 0, max_norm};
  return op_sgd(p, g, buf, tab, &clip, 0.f, hyper, nesterov, n, stream);
}

int dsgcn_adam_step_hyper(float* p, float* g, float* m, float* v, int* step, const int* ends, const int* group,
                          const int* first, int ntens, const double* lr, const double* wd, int groups, const double* hyper,
                          double beta2, float eps, int decoupled, long long n, void* stream) {
  if (!hyper) return DSGCN_EINVAL;
  const OpTable tab = {ends, group, first, lr, wd, ntens, groups};
  return op_adam(p, g, m, v, step, tab, nullptr, 0., hyper, beta2, eps, decoupled, n, stream);
}

int dsgcn_adam_step_clip_hyper(float* p, float* g, float* m, float* v, int* step, const int* ends, const int* group,
                               const int* first, int ntens, const double* lr, const double* wd, int groups,
                               const double* partial, int rows, int norm_type, float max_norm, float* grad_norm_out,
                               const double* hyper, double beta2, float eps, int decoupled, long long n, void* stream) {
  if (!hyper || (norm_type != 0 && norm_type != 2)) return DSGCN_EINVAL;
  const OpTable tab = {ends, group, first, lr, wd, ntens, groups};
  const OpClip clip = {partial, grad_norm_out, rows, norm_type == 0 ? 1 : 0, max_norm};
  return op_adam(p, g, m, v, step, tab, &clip, 0., hyper, beta2, eps, decoupled, n, stream);
}

}  // extern "C"
