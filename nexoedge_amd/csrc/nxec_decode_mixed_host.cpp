// Host half of the mixed-pattern decode (include/nxec.h §4,
// nxec_rs_decode_stripes_mixed): per-stripe verdicts, the distinct decode plans
// with one nxec_rs_decode_matrix each, and the tables the kernel reads.  Pure
// arithmetic, no device: compiled alone under sanitizers by
// tests/cpp/decode_mixed_plan_test.cc.
#include <cstring>
#include <map>
#include <utility>
#include <vector>

#include "nxec.h"
#include "nxec_internal.h"

namespace nxec {

void decode_mixed_plan(int n, int k, const uint8_t *alive, int64_t nstripes, int32_t *result, DecodePlan *plan) {
  using Key = std::pair<uint64_t, uint64_t>;  // n <= 128: one bit per input chunk
  static_assert(NXEC_MAX_N <= 128, "the plan key holds 128 chunks");
  // plan index, or the verdict of an input set that does not invert
  std::map<Key, int32_t> seen;
  DecodePlan local;
  DecodePlan &p = plan ? *plan : local;
  p = DecodePlan{};
  p.plan_of.assign(static_cast<size_t>(nstripes), -1);
  std::vector<int32_t> inputs(k);
  Key last{0, 0};
  int32_t last_verdict = 0;  // of `last`: >= 0 plan index, < 0 NXEC_RECOVER_*
  bool have_last = false;
  for (int64_t s = 0; s < nstripes; s++) {
    const uint8_t *a = alive + s * n;
    Key key{0, 0};
    int ni = 0, ne = 0, nt = 0;  // inputs taken, erased chunks, erased data chunks
    for (int c = 0; c < n; c++) {
      if (!a[c]) {
        ne++;
        nt += c < k;
      } else if (ni < k) {  // rs.cc:252-265: the first k alive chunks
        (c < 64 ? key.first : key.second) |= uint64_t(1) << (c & 63);
        inputs[ni++] = c;
      }
    }
    int32_t r;
    if (ne > n - k) {
      r = NXEC_RECOVER_LOST;
    } else {
      int32_t verdict;
      if (have_last && key == last) {
        verdict = last_verdict;
      } else {
        auto it = seen.find(key);
        if (it == seen.end()) {
          DecodePlan::Plan pl;
          pl.inputs = inputs;
          for (int c = 0, j = 0; c < inputs[k - 1]; c++) {
            if (j < k && inputs[j] == c) {
              j++;
              continue;
            }
            pl.erased.push_back(c);
            if (c < k) pl.targets.push_back(c);
          }
          pl.rows.resize(pl.targets.size() * static_cast<size_t>(k));
          // no lost data chunk: the inputs are chunks 0..k-1 and nothing is inverted
          const int rc = pl.targets.empty() ? NXEC_OK
                                            : nxec_rs_decode_matrix(n, k, pl.inputs.data(), pl.targets.data(),
                                                                    static_cast<int>(pl.targets.size()), pl.rows.data());
          if (rc == NXEC_OK) {
            verdict = static_cast<int32_t>(p.plans.size());
            const int64_t nt_plan = static_cast<int64_t>(pl.targets.size());
            p.nsegments += nt_plan ? (nt_plan + kMaxRowsPerPass - 1) / kMaxRowsPerPass : 1;
            p.plans.push_back(std::move(pl));
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
        p.plan_of[static_cast<size_t>(s)] = verdict;
        p.ndecoded++;
        r = nt;
      } else {
        r = verdict;
      }
    }
    if (result) result[s] = r;
  }
}

void decode_mixed_tables(const DecodePlan &plan, int k, int64_t chunk_stride, int64_t out_chunk_stride,
                         std::vector<DecodeSeg> &segs, std::vector<uint32_t> &order, std::vector<uint32_t> &seg_of) {
  segs.clear();
  order.clear();
  seg_of.clear();
  const size_t np = plan.plans.size();
  std::vector<uint32_t> seg0(np), count(np, 0);  // first segment and number of stripes of each plan
  for (size_t pi = 0; pi < np; pi++) {
    const DecodePlan::Plan &pl = plan.plans[pi];
    seg0[pi] = static_cast<uint32_t>(segs.size());
    const int nt = static_cast<int>(pl.targets.size());
    for (int r0 = 0; r0 == 0 || r0 < nt; r0 += kMaxRowsPerPass) {
      DecodeSeg g;
      std::memset(&g, 0, sizeof(g));
      g.rows = static_cast<uint32_t>(nt - r0 < kMaxRowsPerPass ? nt - r0 : kMaxRowsPerPass);
      for (int j = 0; j < kMaxRaggedK; j++) g.copy_off[j] = kNoCopy;
      for (int j = 0; j < k; j++) {
        g.src_off[j] = static_cast<uint32_t>(pl.inputs[j] * chunk_stride);
        // surviving data chunks are unit rows of the inverse: copies of their input, made once
        if (r0 == 0 && pl.inputs[j] < k) g.copy_off[j] = static_cast<uint32_t>(pl.inputs[j] * out_chunk_stride);
      }
      for (uint32_t r = 0; r < g.rows; r++) {
        g.dst_off[r] = static_cast<uint32_t>(pl.targets[r0 + r] * out_chunk_stride);
        std::memcpy(g.coef + r * k, pl.rows.data() + static_cast<size_t>(r0 + r) * k, k);
      }
      segs.push_back(g);
    }
  }
  for (int32_t pi : plan.plan_of)
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
  for (size_t s = 0; s < plan.plan_of.size(); s++) {
    const int32_t pi = plan.plan_of[s];
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

extern "C" int nxec_rs_decode_mixed_plan(int n, int k, const unsigned char *alive, int64_t nstripes, int32_t *result,
                                         int64_t *nplans, int64_t *nsegments, int64_t *ndecoded) {
  if (!valid_nk(n, k)) return set_error(NXEC_ERR_INVALID, "invalid (n,k)=(%d,%d)", n, k);
  if (nstripes < 0) return set_error(NXEC_ERR_INVALID, "negative nstripes");
  if (!alive && nstripes > 0) return set_error(NXEC_ERR_INVALID, "mixed decode: null alive map");
  DecodePlan plan;
  decode_mixed_plan(n, k, alive, nstripes, result, &plan);
  if (nplans) *nplans = static_cast<int64_t>(plan.plans.size());
  if (nsegments) *nsegments = plan.nsegments;
  if (ndecoded) *ndecoded = plan.ndecoded;
  return NXEC_OK;
}
