// The kernel the mixed-pattern decode launches (nxec::decode_mixed_kernel) for
// every k it takes, against the per-device preparation list
// (nxec::kernel_lds_list): non-null, listed, listed with at least the dynamic
// LDS the launch asks for and marked as carrying no static LDS; no two k share
// a kernel, and none is the recover's kernel of the same k.  Linked against
// libnxec; taking a kernel's address needs no device.
#include <cstdio>
#include <map>

#include "nxec.h"
#include "nxec_internal.h"

int main() {
  int fail = 0;
  std::map<const void *, nxec::KernelLds> listed;
  for (const nxec::KernelLds &e : nxec::kernel_lds_list()) listed.emplace(e.fn, e);
  for (int k = 1; k <= nxec::kMaxDecodeMixedK; k++) {
    int lds = 0;
    const void *fn = nxec::decode_mixed_kernel(k, &lds);
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
    int l2 = 0;
    if (k <= nxec::kMaxRaggedK && nxec::mixed_kernel(k, &l2) == fn) {
      std::fprintf(stderr, "FAIL k=%d: the recover's kernel\n", k);
      fail++;
    }
    for (int k2 = 1; k2 < k; k2++)
      if (nxec::decode_mixed_kernel(k2, &l2) == fn) {
        std::fprintf(stderr, "FAIL k=%d and k=%d share a kernel\n", k2, k);
        fail++;
      }
  }
  if (fail) return 1;
  std::printf("decode_mixed_registry_test ok: %d kernels\n", nxec::kMaxDecodeMixedK);
  return 0;
}
