// Host half of the mixed-pattern recover (include/nxec.h §4,
// nxec_rs_recover_stripes_mixed): per-stripe verdicts, the distinct erasure
// patterns with one nxec_rs_plan each, and the tables the kernel reads.  Pure
// arithmetic, no device: compiled alone under sanitizers by
// tests/cpp/recover_mixed_plan_test.cc.
#include <cstring>
#include <map>
#include <utility>
#include <vector>

#include "nxec.h"
#include "nxec_internal.h"

namespace nxec {

void mixed_plan(int n, int k, const uint8_t *alive, int64_t nstripes, int32_t *result, MixedPlan *plan) {
  using Key = std::pair<uint64_t, uint64_t>;  // n <= 128: one bit per erased chunk
  static_assert(NXEC_MAX_N <= 128, "the pattern key holds 128 chunks");
  // pattern index, or the verdict of a pattern that cannot be decoded
  std::map<Key, int32_t> seen;
  MixedPlan local;
  MixedPlan &p = plan ? *plan : local;
  p = MixedPlan{};
  p.pattern_of.assign(static_cast<size_t>(nstripes), -1);
  std::vector<int32_t> erased(n), inputs(n);
  Key last{0, 0};
  int32_t last_verdict = 0;  // of `last`: >= 0 pattern index, < 0 NXEC_RECOVER_*
  bool have_last = false;
  for (int64_t s = 0; s < nstripes; s++) {
    const uint8_t *a = alive + s * n;
    Key key{0, 0};
    int ne = 0;
    for (int c = 0; c < n; c++) {
      if (a[c]) continue;
      (c < 64 ? key.first : key.second) |= uint64_t(1) << (c & 63);
      erased[ne++] = c;
    }
    int32_t r = 0;
    if (ne > n - k) {
      r = NXEC_RECOVER_LOST;
    } else if (ne > 0) {
      int32_t verdict;
      if (have_last && key == last) {
        verdict = last_verdict;
      } else {
        auto it = seen.find(key);
        if (it == seen.end()) {
          MixedPlan::Pattern pat;
          pat.rows.resize(static_cast<size_t>(ne) * k);
          int ni = 0, mi = 0;
          const int rc = nxec_rs_plan(n, k, erased.data(), ne, 1, inputs.data(), &ni, &mi, pat.rows.data());
          if (rc == NXEC_OK) {
            pat.erased.assign(erased.begin(), erased.begin() + ne);
            pat.inputs.assign(inputs.begin(), inputs.begin() + k);
            verdict = static_cast<int32_t>(p.patterns.size());
            p.nsegments += (ne + kMaxRowsPerPass - 1) / kMaxRowsPerPass;
            p.patterns.push_back(std::move(pat));
          } else {
            verdict = NXEC_RECOVER_SINGULAR;
          }
          it = seen.emplace(key, verdict).first;
        }
        verdict = it->second;
        last = key;
        last_verdict = verdict;
        have_last = true;
      }
      if (verdict >= 0) {
        p.pattern_of[static_cast<size_t>(s)] = verdict;
        p.ncoded++;
        r = ne;
      } else {
        r = verdict;
      }
    }
    if (result) result[s] = r;
  }
}

void mixed_tables(const MixedPlan &plan, int k, int64_t chunk_stride, std::vector<MixedSeg> &segs,
                  std::vector<uint32_t> &order, std::vector<uint32_t> &seg_of) {
  segs.clear();
  order.clear();
  seg_of.clear();
  const size_t np = plan.patterns.size();
  std::vector<uint32_t> seg0(np), count(np, 0);  // first segment and number of stripes of each pattern
  for (size_t pi = 0; pi < np; pi++) {
    const MixedPlan::Pattern &pat = plan.patterns[pi];
    seg0[pi] = static_cast<uint32_t>(segs.size());
    const int ne = static_cast<int>(pat.erased.size());
    for (int r0 = 0; r0 < ne; r0 += kMaxRowsPerPass) {
      MixedSeg g;
      std::memset(&g, 0, sizeof(g));
      g.rows = static_cast<uint32_t>(ne - r0 < kMaxRowsPerPass ? ne - r0 : kMaxRowsPerPass);
      for (int j = 0; j < k; j++) g.src_off[j] = static_cast<uint32_t>(pat.inputs[j] * chunk_stride);
      for (uint32_t r = 0; r < g.rows; r++) {
        g.dst_off[r] = static_cast<uint32_t>(pat.erased[r0 + r] * chunk_stride);
        std::memcpy(g.coef + r * k, pat.rows.data() + static_cast<size_t>(r0 + r) * k, k);
      }
      segs.push_back(g);
    }
  }
  for (int32_t pi : plan.pattern_of)
    if (pi >= 0) count[pi]++;
  // items by segment, then ascending stripe: item_at[g] = the next free item of segment g
  std::vector<size_t> item_at(segs.size() + 1, 0);
  size_t total = 0;
  for (size_t pi = 0; pi < np; pi++) {
    const size_t nseg = (pi + 1 < np ? seg0[pi + 1] : segs.size()) - seg0[pi];
    for (size_t g = 0; g < nseg; g++) {
      item_at[seg0[pi] + g] = total;
      total += count[pi];
    }
  }
  order.resize(total);
  seg_of.resize(total);
  for (size_t s = 0; s < plan.pattern_of.size(); s++) {
    const int32_t pi = plan.pattern_of[s];
    if (pi < 0) continue;
    const size_t nseg = (static_cast<size_t>(pi) + 1 < np ? seg0[pi + 1] : segs.size()) - seg0[pi];
    for (size_t g = seg0[pi]; g < seg0[pi] + nseg; g++) {
      const size_t i = item_at[g]++;
      order[i] = static_cast<uint32_t>(s);
      seg_of[i] = static_cast<uint32_t>(g);
    }
  }
}

}  // namespace nxec

using namespace nxec;

extern "C" int nxec_rs_recover_mixed_plan(int n, int k, const unsigned char *alive, int64_t nstripes, int32_t *result,
                                          int64_t *npatterns, int64_t *nsegments, int64_t *ncoded) {
  if (!valid_nk(n, k)) return set_error(NXEC_ERR_INVALID, "invalid (n,k)=(%d,%d)", n, k);
  if (nstripes < 0) return set_error(NXEC_ERR_INVALID, "negative nstripes");
  if (!alive && nstripes > 0) return set_error(NXEC_ERR_INVALID, "mixed recover: null alive map");
  MixedPlan plan;
  mixed_plan(n, k, alive, nstripes, result, &plan);
  if (npatterns) *npatterns = static_cast<int64_t>(plan.patterns.size());
  if (nsegments) *nsegments = plan.nsegments;
  if (ncoded) *ncoded = plan.ncoded;
  return NXEC_OK;
}
