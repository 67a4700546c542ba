// The kernels the mixed-pattern recover (full = false) and decode (full = true)
// launch (nxec::mixed_kernel) for every k they take, against the per-device
// preparation list (nxec::kernel_lds_list): non-null, listed, listed with at
// least the dynamic LDS the launch asks for and marked as carrying no static
// LDS; no two k share a kernel, and no decode kernel is the recover's kernel of
// the same k.  Linked against libnxec; taking a kernel's address needs no device.
#include <cstdio>
#include <map>

#include "nxec.h"
#include "nxec_internal.h"

int main() {
  int fail = 0;
  std::map<const void *, nxec::KernelLds> listed;
  for (const nxec::KernelLds &e : nxec::kernel_lds_list()) listed.emplace(e.fn, e);
  for (const bool full : {false, true}) {
    const char *what = full ? "decode" : "recover";
    for (int k = 1; k <= nxec::kMaxRaggedK; k++) {
      int lds = 0;
      const void *fn = nxec::mixed_kernel(k, full, &lds);
      if (!fn) {
        std::fprintf(stderr, "FAIL %s k=%d: no kernel\n", what, k);
        fail++;
        continue;
      }
      const auto it = listed.find(fn);
      if (it == listed.end()) {
        std::fprintf(stderr, "FAIL %s k=%d: not in the preparation list\n", what, k);
        fail++;
        continue;
      }
      if (lds <= 0 || lds > 160 * 1024 || it->second.bytes < lds) {
        std::fprintf(stderr, "FAIL %s k=%d: launch asks %d bytes, %d prepared\n", what, k, lds, it->second.bytes);
        fail++;
      }
      if (!it->second.no_static) {
        std::fprintf(stderr, "FAIL %s k=%d: listed without the no-static-LDS check\n", what, k);
        fail++;
      }
      int l2 = 0;
      if (full && nxec::mixed_kernel(k, false, &l2) == fn) {
        std::fprintf(stderr, "FAIL k=%d: the decode's kernel is the recover's\n", k);
        fail++;
      }
      for (int k2 = 1; k2 < k; k2++)
        if (nxec::mixed_kernel(k2, full, &l2) == fn) {
          std::fprintf(stderr, "FAIL %s k=%d and k=%d share a kernel\n", what, k2, k);
          fail++;
        }
    }
  }
  if (fail) return 1;
  std::printf("mixed_registry_test ok: %d kernels\n", 2 * nxec::kMaxRaggedK);
  return 0;
}
