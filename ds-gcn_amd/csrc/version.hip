#include "common.h"
#include <atomic>
extern "C" int dsgcn_version(void) { return 100; }

// Matmul precision: process-wide, read on the host when a launch is chosen (a captured graph keeps its kernels).
static std::atomic<int> g_matmul_precision{0};
__attribute__((visibility("hidden"))) int dsgcn_precision_level() { return g_matmul_precision.load(std::memory_order_relaxed); }
extern "C" int dsgcn_set_matmul_precision(int level) {
  if (level != 0 && level != 1) return DSGCN_EINVAL;
  g_matmul_precision.store(level, std::memory_order_relaxed);
  return 0;
}
extern "C" int dsgcn_get_matmul_precision(void) { return dsgcn_precision_level(); }
