// Host half of the mixed-pattern recover and decode (include/nxec.h §4,
// nxec_rs_recover_stripes_mixed / nxec_rs_decode_stripes_mixed): per-stripe
// verdicts, the distinct plans with one repair or inverse matrix each, and the
// tables the kernel reads.  Pure arithmetic, no device: compiled alone under
// sanitizers by tests/cpp/recover_mixed_plan_test.cc and decode_mixed_plan_test.cc.
#include <cstring>
#include <map>
#include <utility>
#include <vector>

#include "nxec.h"
#include "nxec_internal.h"

namespace nxec {

void mixed_plan(MixedMode mode, int n, int k, const uint8_t *alive, int64_t nstripes, int32_t *result, MixedPlan *plan) {
  const bool decode = mode == MixedMode::Decode;
  // n <= 128: one bit per chunk of the key set (Recover: the erased chunks; Decode: the first k alive ones)
  using Key = std::pair<uint64_t, uint64_t>;
  static_assert(NXEC_MAX_N <= 128, "the plan key holds 128 chunks");
  // plan index, or the verdict of a key that cannot be decoded
  std::map<Key, int32_t> seen;
  MixedPlan local;
  MixedPlan &p = plan ? *plan : local;
  p = MixedPlan{};
  p.plan_of.assign(static_cast<size_t>(nstripes), -1);
  std::vector<int32_t> erased(n), inputs(n);
  Key last{0, 0};
  int32_t last_verdict = 0;  // of `last`: >= 0 plan index, < 0 NXEC_RECOVER_*
  bool have_last = false;
  for (int64_t s = 0; s < nstripes; s++) {
    const uint8_t *a = alive + s * n;
    Key key{0, 0};
    int ni = 0, ne = 0, nt = 0;  // inputs taken, erased chunks, erased data chunks
    for (int c = 0; c < n; c++) {
      const bool in_key = decode ? a[c] && ni < k : !a[c];  // rs.cc:252-265: the first k alive chunks
      if (in_key) (c < 64 ? key.first : key.second) |= uint64_t(1) << (c & 63);
      if (!a[c]) {
        erased[ne++] = c;
        nt += c < k;
      } else if (ni < k) {
        inputs[ni++] = c;
      }
    }
    int32_t r = 0;
    if (ne > n - k) {
      r = NXEC_RECOVER_LOST;
    } else if (decode || ne > 0) {  // Recover: nothing erased, nothing planned
      int32_t verdict;
      if (have_last && key == last) {
        verdict = last_verdict;
      } else {
        auto it = seen.find(key);
        if (it == seen.end()) {
          MixedPlan::Plan pl;
          int rc = NXEC_OK;
          if (decode) {
            pl.inputs.assign(inputs.begin(), inputs.begin() + k);
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
            if (!pl.targets.empty())
              rc = nxec_rs_decode_matrix(n, k, pl.inputs.data(), pl.targets.data(), static_cast<int>(pl.targets.size()),
                                         pl.rows.data());
          } else {
            pl.rows.resize(static_cast<size_t>(ne) * k);
            int pi = 0, mi = 0;
            rc = nxec_rs_plan(n, k, erased.data(), ne, 1, inputs.data(), &pi, &mi, pl.rows.data());
            if (rc == NXEC_OK) {
              pl.erased.assign(erased.begin(), erased.begin() + ne);
              pl.targets = pl.erased;
              pl.inputs.assign(inputs.begin(), inputs.begin() + k);
            }
          }
          if (rc == NXEC_OK) {
            verdict = static_cast<int32_t>(p.plans.size());
            p.nsegments += row_passes(static_cast<int>(pl.targets.size()));  // no target: Decode's copy-only plan
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
        p.nstripes_planned++;
        r = decode ? nt : ne;
      } else {
        r = verdict;
      }
    }
    if (result) result[s] = r;
  }
}

void mixed_tables(const MixedPlan &plan, int k, int64_t chunk_stride, int64_t out_chunk_stride, bool copy,
                  std::vector<MixedSeg> &segs, std::vector<uint32_t> &order, std::vector<uint32_t> &seg_of) {
  segs.clear();
  order.clear();
  seg_of.clear();
  const size_t np = plan.plans.size();
  std::vector<uint32_t> seg0(np), count(np, 0);  // first segment and number of stripes of each plan
  for (size_t pi = 0; pi < np; pi++) {
    const MixedPlan::Plan &pl = plan.plans[pi];
    seg0[pi] = static_cast<uint32_t>(segs.size());
    const int nt = static_cast<int>(pl.targets.size());
    for (int p = 0; p < row_passes(nt); p++) {
      const int r0 = p * kMaxRowsPerPass;
      MixedSeg g;
      std::memset(&g, 0, sizeof(g));
      g.rows = static_cast<uint32_t>(pass_coef(nt, k, pl.rows.data(), p, g.coef));
      for (int j = 0; j < kMaxRaggedK; j++) g.copy_off[j] = kNoCopy;
      for (int j = 0; j < k; j++) {
        g.src_off[j] = static_cast<uint32_t>(pl.inputs[j] * chunk_stride);
        // surviving data chunks are unit rows of the inverse: copies of their input, made once
        if (copy && r0 == 0 && pl.inputs[j] < k) g.copy_off[j] = static_cast<uint32_t>(pl.inputs[j] * out_chunk_stride);
      }
      for (uint32_t r = 0; r < g.rows; r++) g.dst_off[r] = static_cast<uint32_t>(pl.targets[r0 + r] * out_chunk_stride);
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

static int plan_counters(MixedMode mode, const char *what, int n, int k, const unsigned char *alive, int64_t nstripes,
                         int32_t *result, int64_t *nplans, int64_t *nsegments, int64_t *nplanned) {
  if (!valid_nk(n, k)) return set_error(NXEC_ERR_INVALID, "invalid (n,k)=(%d,%d)", n, k);
  if (nstripes < 0) return set_error(NXEC_ERR_INVALID, "negative nstripes");
  if (!alive && nstripes > 0) return set_error(NXEC_ERR_INVALID, "mixed %s: null alive map", what);
  MixedPlan plan;
  mixed_plan(mode, n, k, alive, nstripes, result, &plan);
  if (nplans) *nplans = static_cast<int64_t>(plan.plans.size());
  if (nsegments) *nsegments = plan.nsegments;
  if (nplanned) *nplanned = plan.nstripes_planned;
  return NXEC_OK;
}

extern "C" int nxec_rs_recover_mixed_plan(int n, int k, const unsigned char *alive, int64_t nstripes, int32_t *result,
                                          int64_t *npatterns, int64_t *nsegments, int64_t *ncoded) {
  return plan_counters(MixedMode::Recover, "recover", n, k, alive, nstripes, result, npatterns, nsegments, ncoded);
}

extern "C" int nxec_rs_decode_mixed_plan(int n, int k, const unsigned char *alive, int64_t nstripes, int32_t *result,
                                         int64_t *nplans, int64_t *nsegments, int64_t *ndecoded) {
  return plan_counters(MixedMode::Decode, "decode", n, k, alive, nstripes, result, nplans, nsegments, ndecoded);
}
