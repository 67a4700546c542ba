// The kernels the delta update launches (nxec::update_vec_kernel for k <= 19,
// nxec::update_bytes_kernel for every k) against the per-device preparation
// list (nxec::kernel_lds_list): non-null, listed, and listed with at least the
// dynamic LDS the launch asks for; the vector kernels also marked as carrying
// no static LDS.  Linked against libnxec; taking a kernel's address needs no
// device.
#include <cstdio>
#include <map>
#include <set>

#include "nxec.h"
#include "nxec_internal.h"

int main() {
  int fail = 0;
  std::map<const void *, int> prepared;  // the most bytes any entry of the kernel lists
  std::set<const void *> no_static;
  for (const nxec::KernelLds &e : nxec::kernel_lds_list()) {
    int &b = prepared[e.fn];
    b = e.bytes > b ? e.bytes : b;
    if (e.no_static) no_static.insert(e.fn);
  }
  auto check = [&](const char *what, int k, const void *fn, int lds, bool want_no_static) {
    if (!fn) {
      std::fprintf(stderr, "FAIL %s k=%d: no kernel\n", what, k);
      fail++;
      return;
    }
    const auto it = prepared.find(fn);
    if (it == prepared.end()) {
      std::fprintf(stderr, "FAIL %s k=%d: not in the preparation list\n", what, k);
      fail++;
      return;
    }
    if (lds <= 0 || lds > 160 * 1024 || it->second < lds) {
      std::fprintf(stderr, "FAIL %s k=%d: launch asks %d bytes, %d prepared\n", what, k, lds, it->second);
      fail++;
    }
    if (want_no_static && !no_static.count(fn)) {
      std::fprintf(stderr, "FAIL %s k=%d: listed without the no-static-LDS check\n", what, k);
      fail++;
    }
  };
  std::set<const void *> vec;
  for (int k = 1; k <= nxec::kMaxRaggedK; k++) {
    int lds = 0;
    const void *fn = nxec::update_vec_kernel(k, &lds);
    check("k_update_vec", k, fn, lds, true);
    // the tables of all k columns at the replication of the encode, then the queue ring
    const int want = k * 1024 * (k <= 9 ? 16 : 8) + 16;
    if (lds != want) {
      std::fprintf(stderr, "FAIL k_update_vec k=%d: launch asks %d bytes, the tables and the ring take %d\n", k, lds, want);
      fail++;
    }
    vec.insert(fn);
  }
  for (int k = 1; k <= NXEC_MAX_K; k++) {
    int lds = 0;
    const void *fn = nxec::update_bytes_kernel(k, &lds);
    check("k_update_bytes", k, fn, lds, false);
    if (lds != k * 1024) {
      std::fprintf(stderr, "FAIL k_update_bytes k=%d: launch asks %d bytes\n", k, lds);
      fail++;
    }
  }
  if (fail) return 1;
  std::printf("update_registry_test ok: %zu vector kernels, k up to %d\n", vec.size(), NXEC_MAX_K);
  return 0;
}
