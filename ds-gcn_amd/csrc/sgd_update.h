// The SGD update of one element, shared by k_sgd (head.hip) and k_sgd_clip (clip.hip) — torch.optim.SGD's order with
// dampening 0:  g' = g + wd p;  buf = mom buf + g';  step = nesterov ? g' + mom buf : buf;  p -= rate step.
// Every multiply-add is an explicit fmaf: both kernels round alike whatever the compiler would contract on its own, so
// the clipped step with coefficient 1 is bit-identical to the plain one.
#pragma once

__device__ __forceinline__ float sgd_update(float pv, float gv, float& bv, bool has_buf, float rate, float mom, float wd,
                                            int nesterov) {
  gv = fmaf(wd, pv, gv);
  float st = gv;
  if (has_buf) {
    bv = fmaf(bv, mom, gv);
    st = nesterov ? fmaf(mom, bv, gv) : bv;
  }
  return fmaf(-rate, st, pv);
}
