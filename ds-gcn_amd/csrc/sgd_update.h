// The SGD update of one element, shared by k_sgd (head.hip) and k_sgd_clip (clip.hip) — torch.optim.SGD's order with
// dampening 0:  g' = g + wd p;  buf = mom buf + g';  step = nesterov ? g' + mom buf : buf;  p -= rate step.
// Every multiply-add is an explicit fmaf: both kernels round alike whatever the compiler would contract on its own, so
// the clipped step with coefficient 1 is bit-identical to the plain one.
#pragma once

// A value every lane of the wave holds alike, moved to a scalar register: what depends on it (whether the momentum buffer
// is touched at all) then branches once per wave, as it does on a by-value kernel argument.
__device__ __forceinline__ float uniform_f32(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}

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
