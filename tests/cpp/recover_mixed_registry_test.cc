// The kernel the mixed-pattern recover launches (nxec::mixed_kernel) for every
// k it takes, against the per-device preparation list (nxec::kernel_lds_list):
// non-null, listed, listed with at least the dynamic LDS the launch asks for
// and marked as carrying no static LDS.  Linked against libnxec; taking a
// kernel's address needs no device.
#include <cstdio>
#include <map>

#include "nxec.h"
#include "nxec_internal.h"

int main() {
  int fail = 0;
  std::map<const void *, nxec::KernelLds> listed;
  for (const nxec::KernelLds &e : nxec::kernel_lds_list()) listed.emplace(e.fn, e);
  for (int k = 1; k <= nxec::kMaxRaggedK; k++) {
    int lds = 0;
    const void *fn = nxec::mixed_kernel(k, &lds);
    if (!fn) {
      std::fprintf(stderr, "FAIL k=%d: no kernel\n", k);
      fail++;
      continue;
    }
    const auto it = listed.find(fn);
    if (it == listed.end()) {
      std::fprintf(stderr, "FAIL k=%d: not in the preparation list\n", k);
      fail++;
      continue;
    }
    if (lds <= 0 || lds > 160 * 1024 || it->second.bytes < lds) {
      std::fprintf(stderr, "FAIL k=%d: launch asks %d bytes, %d prepared\n", k, lds, it->second.bytes);
      fail++;
    }
    if (!it->second.no_static) {
      std::fprintf(stderr, "FAIL k=%d: listed without the no-static-LDS check\n", k);
      fail++;
    }
    for (int k2 = 1; k2 < k; k2++) {
      int l2 = 0;
      if (nxec::mixed_kernel(k2, &l2) == fn) {
        std::fprintf(stderr, "FAIL k=%d and k=%d share a kernel\n", k2, k);
        fail++;
      }
    }
  }
  if (fail) return 1;
  std::printf("recover_mixed_registry_test ok: %d kernels\n", nxec::kMaxRaggedK);
  return 0;
}
