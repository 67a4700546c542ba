// Host side of the parity scrub's per-byte rule (include/nxec.h §4,
// nxec_rs_syndrome_locate): pure arithmetic, no device.  The rule itself is
// nxec_scrub_rule.h, the code the locate / heal kernel runs per byte.
#include <vector>

#include "nxec.h"
#include "nxec_internal.h"
#include "nxec_scrub_rule.h"

using namespace nxec;

extern "C" int nxec_rs_syndrome_locate(int n, int k, const unsigned char *syndrome, int32_t *chunk,
                                       unsigned char *error) {
  if (!valid_nk(n, k)) return set_error(NXEC_ERR_INVALID, "invalid (n,k)=(%d,%d)", n, k);
  if (!chunk || (n > k && !syndrome)) return set_error(NXEC_ERR_INVALID, "nxec_rs_syndrome_locate: null argument");
  static_assert(scrub::kClean == NXEC_SCRUB_CLEAN && scrub::kUnlocated == NXEC_SCRUB_UNLOCATED, "status codes");
  uint8_t e = 0;
  *chunk = scrub::locate(n, k, rs_parity_rows(n, k).data(), [&](int r) { return syndrome[r]; }, &e);
  if (error) *error = e;
  return NXEC_OK;
}
