// Stand-alone host program for the planner of the mixed-pattern recover
// (nxec_rs_recover_mixed_plan, nxec::mixed_plan, nxec::mixed_tables): no
// device, no libnxec.  Built with -fsanitize=address,undefined (make
// build/recover_mixed_plan_test) from the planner source and gf_host.cpp.
//
// Cases:
//  * every erasure set of 1..n-k chunks of five geometries, one stripe per
//    set: result is |E| exactly where nxec_rs_plan succeeds, SINGULAR where it
//    reports a singular matrix; the counts are pinned;
//  * every set of n-k+1 chunks is LOST, an all-alive stripe is 0;
//  * random maps of 10^4 stripes: verdicts and counters against a direct
//    per-stripe evaluation, and the device tables' invariants (items by
//    segment then ascending stripe, every coded stripe once per segment of its
//    pattern, offsets and coefficient rows those of nxec_rs_plan, unused rows zero);
//  * one RS(6,4) batch of five stripes: every field of the device tables
//    against values written out by hand, copy_off all kNoCopy.
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <set>
#include <vector>

#include "nxec.h"
#include "nxec_internal.h"

namespace nxec {
// the library's error sink lives with the device runtime; here a stub
int set_error(int code, const char *, ...) { return code; }
}  // namespace nxec

namespace {

int g_fail = 0;
#define EXPECT(cond, ...)                                       \
  do {                                                          \
    if (!(cond)) {                                              \
      std::fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
      std::fprintf(stderr, __VA_ARGS__);                        \
      std::fprintf(stderr, "\n");                               \
      g_fail++;                                                 \
    }                                                           \
  } while (0)

// every subset of `size` ids out of n, appended as alive rows (0 = erased)
void subsets(int n, int size, std::vector<std::vector<int32_t>> &out) {
  std::vector<int32_t> c(size);
  for (int i = 0; i < size; i++) c[i] = i;
  while (true) {
    out.push_back(c);
    int i = size - 1;
    while (i >= 0 && c[i] == n - size + i) i--;
    if (i < 0) break;
    c[i]++;
    for (int j = i + 1; j < size; j++) c[j] = c[j - 1] + 1;
  }
}

int direct(int n, int k, const std::vector<int32_t> &e, std::vector<int32_t> *inputs, std::vector<unsigned char> *rm) {
  if (e.empty()) return 0;
  if (static_cast<int>(e.size()) > n - k) return NXEC_RECOVER_LOST;
  std::vector<int32_t> in(n);
  std::vector<unsigned char> m(e.size() * k);
  int ni = 0, mi = 0;
  const int rc = nxec_rs_plan(n, k, e.data(), static_cast<int>(e.size()), 1, in.data(), &ni, &mi, m.data());
  if (rc == NXEC_ERR_SINGULAR) return NXEC_RECOVER_SINGULAR;
  EXPECT(rc == NXEC_OK, "(%d,%d) nxec_rs_plan rc %d", n, k, rc);
  if (inputs) inputs->assign(in.begin(), in.begin() + k);
  if (rm) *rm = m;
  return static_cast<int>(e.size());
}

void enumerate(int n, int k, int64_t want_patterns, int64_t want_singular) {
  std::vector<std::vector<int32_t>> sets;
  for (int size = 1; size <= n - k; size++) subsets(n, size, sets);
  const size_t ndec = sets.size();
  subsets(n, n - k + 1, sets);  // LOST
  sets.push_back({});           // all alive
  const int64_t ns = static_cast<int64_t>(sets.size());
  std::vector<unsigned char> alive(static_cast<size_t>(ns) * n, 1);
  for (int64_t s = 0; s < ns; s++)
    for (int32_t c : sets[s]) alive[s * n + c] = 0;
  std::vector<int32_t> res(ns, 12345);
  int64_t np = -1, nseg = -1, nc = -1;
  EXPECT(nxec_rs_recover_mixed_plan(n, k, alive.data(), ns, res.data(), &np, &nseg, &nc) == NXEC_OK, "(%d,%d) rc", n, k);
  int64_t singular = 0, segs = 0, coded = 0;
  for (size_t s = 0; s < sets.size(); s++) {
    const int want = direct(n, k, sets[s], nullptr, nullptr);
    EXPECT(res[s] == want, "(%d,%d) set %zu of %zu ids: result %d, want %d", n, k, s, sets[s].size(), res[s], want);
    if (s < ndec) {
      singular += want == NXEC_RECOVER_SINGULAR;
      if (want > 0) {
        coded++;
        segs += (want + 3) / 4;
      }
    } else if (!sets[s].empty()) {
      EXPECT(res[s] == NXEC_RECOVER_LOST, "(%d,%d) n-k+1 erased: %d", n, k, res[s]);
    }
  }
  EXPECT(res[ns - 1] == 0, "(%d,%d) all alive: %d", n, k, res[ns - 1]);
  EXPECT(static_cast<int64_t>(ndec) == want_patterns, "(%d,%d) %zu sets of 1..n-k ids, pinned %lld", n, k, ndec,
         static_cast<long long>(want_patterns));
  EXPECT(singular == want_singular, "(%d,%d) %lld singular sets, pinned %lld", n, k, static_cast<long long>(singular),
         static_cast<long long>(want_singular));
  EXPECT(np == coded && nc == coded && nseg == segs, "(%d,%d) counters %lld %lld %lld, want %lld %lld %lld", n, k,
         static_cast<long long>(np), static_cast<long long>(nseg), static_cast<long long>(nc),
         static_cast<long long>(coded), static_cast<long long>(segs), static_cast<long long>(coded));
  // the same batch twice: every pattern counts once
  std::vector<unsigned char> twice(alive);
  twice.insert(twice.end(), alive.begin(), alive.end());
  int64_t np2 = -1, nseg2 = -1, nc2 = -1;
  EXPECT(nxec_rs_recover_mixed_plan(n, k, twice.data(), 2 * ns, nullptr, &np2, &nseg2, &nc2) == NXEC_OK, "twice rc");
  EXPECT(np2 == np && nseg2 == nseg && nc2 == 2 * nc, "(%d,%d) duplicated patterns counted again", n, k);
}

void random_maps(int n, int k, uint32_t seed, int max_erased) {
  const int64_t ns = 10000;
  const int64_t cs = 4096 + 48;
  std::mt19937 rng(seed);
  std::vector<unsigned char> alive(static_cast<size_t>(ns) * n);
  for (int64_t s = 0; s < ns; s++) {
    const int ne = static_cast<int>(rng() % (max_erased + 1));
    for (int c = 0; c < n; c++) alive[s * n + c] = static_cast<unsigned char>(1 + rng() % 255);  // any non-zero is alive
    for (int i = 0; i < ne; i++) alive[s * n + rng() % n] = 0;
  }
  std::vector<int32_t> res(ns, 777);
  nxec::MixedPlan plan;
  nxec::mixed_plan(nxec::MixedMode::Recover, n, k, alive.data(), ns, res.data(), &plan);
  std::set<std::vector<int32_t>> distinct;
  int64_t coded = 0, segs = 0;
  for (int64_t s = 0; s < ns; s++) {
    std::vector<int32_t> e;
    for (int c = 0; c < n; c++)
      if (!alive[s * n + c]) e.push_back(c);
    const int want = direct(n, k, e, nullptr, nullptr);
    EXPECT(res[s] == want, "(%d,%d) random stripe %lld: %d, want %d", n, k, static_cast<long long>(s), res[s], want);
    EXPECT((plan.plan_of[s] >= 0) == (want > 0), "plan_of of stripe %lld", static_cast<long long>(s));
    if (want > 0) {
      coded++;
      if (distinct.insert(e).second) segs += (want + 3) / 4;
      EXPECT(plan.plans[plan.plan_of[s]].erased == e, "stripe %lld mapped to another pattern", static_cast<long long>(s));
    }
  }
  EXPECT(plan.nstripes_planned == coded && plan.nsegments == segs && plan.plans.size() == distinct.size(),
         "(%d,%d) random counters", n, k);
  if (k > nxec::kMaxRaggedK) return;
  std::vector<nxec::MixedSeg> sg;
  std::vector<uint32_t> order, seg_of;
  nxec::mixed_tables(plan, k, cs, cs, false, sg, order, seg_of);
  EXPECT(static_cast<int64_t>(sg.size()) == segs && order.size() == seg_of.size(), "(%d,%d) table sizes", n, k);
  std::map<uint32_t, int> times;  // stripe -> items
  std::map<uint32_t, std::set<int32_t>> rebuilt;
  for (size_t i = 0; i < order.size(); i++) {
    if (i) EXPECT(seg_of[i] > seg_of[i - 1] || (seg_of[i] == seg_of[i - 1] && order[i] > order[i - 1]),
                  "(%d,%d) item %zu out of order", n, k, i);
    if (seg_of[i] >= sg.size() || order[i] >= ns) {
      EXPECT(false, "(%d,%d) item %zu out of range", n, k, i);
      continue;
    }
    times[order[i]]++;
    const nxec::MixedSeg &g = sg[seg_of[i]];
    const nxec::MixedPlan::Plan &pat = plan.plans[plan.plan_of[order[i]]];
    std::vector<int32_t> in;
    std::vector<unsigned char> rm;
    direct(n, k, pat.erased, &in, &rm);
    EXPECT(g.rows >= 1 && g.rows <= 4, "rows %u", g.rows);
    for (int j = 0; j < k; j++) {
      EXPECT(g.src_off[j] == static_cast<uint32_t>(in[j] * cs), "src_off[%d]", j);
      EXPECT(alive[static_cast<size_t>(order[i]) * n + in[j]] != 0, "an erased chunk is a source");
    }
    for (uint32_t r = 0; r < 4; r++) {
      if (r >= g.rows) {
        for (int j = 0; j < k; j++) EXPECT(g.coef[r * k + j] == 0, "unused coefficient row %u not zero", r);
        continue;
      }
      const int32_t id = static_cast<int32_t>(g.dst_off[r] / cs);
      EXPECT(g.dst_off[r] % cs == 0 && !alive[static_cast<size_t>(order[i]) * n + id], "a live chunk is a destination");
      EXPECT(rebuilt[order[i]].insert(id).second, "chunk %d of stripe %u rebuilt twice", id, order[i]);
      const size_t pos = std::find(pat.erased.begin(), pat.erased.end(), id) - pat.erased.begin();
      EXPECT(pos < pat.erased.size() && std::memcmp(g.coef + r * k, rm.data() + pos * k, k) == 0, "row of chunk %d", id);
    }
  }
  for (int64_t s = 0; s < ns; s++) {
    const int want = res[s] > 0 ? (res[s] + 3) / 4 : 0;
    const auto it = times.find(static_cast<uint32_t>(s));
    EXPECT((it == times.end() ? 0 : it->second) == want, "stripe %lld: items", static_cast<long long>(s));
    if (res[s] > 0) EXPECT(static_cast<int>(rebuilt[static_cast<uint32_t>(s)].size()) == res[s], "stripe %lld: rows", static_cast<long long>(s));
  }
}

// The recover's device tables of one small batch against values written out by
// hand: RS(6,4), chunk stride 64, erased sets {}, {0}, {0}, {1,5}, {0,1,2}.
// Parity 4 is d0^d1^d2^d3 and parity 5 is d0 ^ 2 d1 ^ 4 d2 ^ 8 d3, so
//   chunk 0 from 1,2,3,4:  d0 = d1 ^ d2 ^ d3 ^ p4                        rows {1,1,1,1}
//   chunks 1,5 from 0,2,3,4: d1 = d0 ^ d2 ^ d3 ^ p4                      rows {1,1,1,1}
//                            p5 = d0 ^ 2 (d0^d2^d3^p4) ^ 4 d2 ^ 8 d3          {3,6,10,2}
// Recover records carry no copies: copy_off is kNoCopy throughout.
void hand_tables() {
  const int n = 6, k = 4;
  const int64_t cs = 64;
  unsigned char alive[5 * n];
  std::memset(alive, 1, sizeof alive);
  alive[1 * n + 0] = alive[2 * n + 0] = 0;
  alive[3 * n + 1] = alive[3 * n + 5] = 0;
  alive[4 * n + 0] = alive[4 * n + 1] = alive[4 * n + 2] = 0;
  int32_t res[5];
  nxec::MixedPlan plan;
  nxec::mixed_plan(nxec::MixedMode::Recover, n, k, alive, 5, res, &plan);
  const int32_t want_res[5] = {0, 1, 1, 2, NXEC_RECOVER_LOST};
  EXPECT(std::memcmp(res, want_res, sizeof res) == 0, "hand tables: verdicts");
  EXPECT(plan.plans.size() == 2 && plan.nsegments == 2 && plan.nstripes_planned == 3, "hand tables: 2 plans, 2 segments");
  std::vector<nxec::MixedSeg> sg;
  std::vector<uint32_t> order, seg_of;
  nxec::mixed_tables(plan, k, cs, cs, false, sg, order, seg_of);
  EXPECT(order == std::vector<uint32_t>({1, 2, 3}) && seg_of == std::vector<uint32_t>({0, 0, 1}), "hand tables: items");
  if (sg.size() != 2) {
    EXPECT(false, "hand tables: %zu segments", sg.size());
    return;
  }
  nxec::MixedSeg want[2];
  std::memset(want, 0, sizeof want);
  for (nxec::MixedSeg &g : want)
    for (uint32_t &c : g.copy_off) c = nxec::kNoCopy;
  want[0].rows = 1;
  want[0].dst_off[0] = 0;
  const uint32_t src0[4] = {64, 128, 192, 256}, src1[4] = {0, 128, 192, 256};
  const uint8_t coef0[4] = {1, 1, 1, 1}, coef1[8] = {1, 1, 1, 1, 3, 6, 10, 2};
  std::memcpy(want[0].src_off, src0, sizeof src0);
  std::memcpy(want[0].coef, coef0, sizeof coef0);
  want[1].rows = 2;
  want[1].dst_off[0] = 64;
  want[1].dst_off[1] = 320;
  std::memcpy(want[1].src_off, src1, sizeof src1);
  std::memcpy(want[1].coef, coef1, sizeof coef1);
  for (int g = 0; g < 2; g++) {
    EXPECT(sg[g].rows == want[g].rows, "hand tables: rows of segment %d: %u", g, sg[g].rows);
    EXPECT(std::memcmp(sg[g].dst_off, want[g].dst_off, sizeof want[g].dst_off) == 0, "hand tables: dst_off of segment %d", g);
    EXPECT(std::memcmp(sg[g].src_off, want[g].src_off, sizeof want[g].src_off) == 0, "hand tables: src_off of segment %d", g);
    EXPECT(std::memcmp(sg[g].coef, want[g].coef, sizeof want[g].coef) == 0, "hand tables: coef of segment %d", g);
    for (int j = 0; j < nxec::kMaxRaggedK; j++)
      EXPECT(sg[g].copy_off[j] == nxec::kNoCopy, "hand tables: copy_off[%d] of segment %d is set", j, g);
  }
}

}  // namespace

int main() {
  hand_tables();
  enumerate(6, 4, 21, 0);
  enumerate(14, 10, 1470, 0);
  enumerate(10, 4, 847, 0);
  enumerate(23, 19, 10902, 0);
  enumerate(12, 6, 2509, 10);
  {  // two of the ten singular sets of (12,6)
    const int sets[2][5] = {{0, 2, 5, 7, 8}, {0, 3, 5, 8, 9}};
    for (const auto &e : sets) {
      unsigned char alive[12];
      std::memset(alive, 1, sizeof alive);
      for (int c : e) alive[c] = 0;
      int32_t r = 0;
      EXPECT(nxec_rs_recover_mixed_plan(12, 6, alive, 1, &r, nullptr, nullptr, nullptr) == NXEC_OK &&
                 r == NXEC_RECOVER_SINGULAR, "(12,6) {%d,%d,%d,%d,%d}: %d", e[0], e[1], e[2], e[3], e[4], r);
    }
  }
  random_maps(14, 10, 1, 6);
  random_maps(10, 4, 2, 7);
  random_maps(6, 4, 3, 3);
  random_maps(24, 21, 4, 4);
  // argument validation
  unsigned char a[8] = {1, 1, 1, 1, 1, 1, 1, 1};
  int32_t r = 55;
  EXPECT(nxec_rs_recover_mixed_plan(0, 0, a, 1, &r, nullptr, nullptr, nullptr) == NXEC_ERR_INVALID, "n = 0 accepted");
  EXPECT(nxec_rs_recover_mixed_plan(4, 5, a, 1, &r, nullptr, nullptr, nullptr) == NXEC_ERR_INVALID, "k > n accepted");
  EXPECT(nxec_rs_recover_mixed_plan(6, 4, nullptr, 1, &r, nullptr, nullptr, nullptr) == NXEC_ERR_INVALID, "null alive accepted");
  EXPECT(nxec_rs_recover_mixed_plan(6, 4, a, -1, &r, nullptr, nullptr, nullptr) == NXEC_ERR_INVALID, "negative nstripes accepted");
  EXPECT(r == 55, "a refused call wrote the result");
  int64_t np = 9, nsg = 9, nc = 9;
  EXPECT(nxec_rs_recover_mixed_plan(6, 4, nullptr, 0, nullptr, &np, &nsg, &nc) == NXEC_OK && np == 0 && nsg == 0 && nc == 0,
         "empty batch");
  a[2] = 0;
  int32_t rr[2] = {55, 55};
  EXPECT(nxec_rs_recover_mixed_plan(4, 4, a, 2, rr, &np, &nsg, &nc) == NXEC_OK && rr[0] == NXEC_RECOVER_LOST &&
             rr[1] == 0 && nc == 0, "n == k: an erased chunk is lost");
  if (g_fail) {
    std::fprintf(stderr, "recover_mixed_plan_test: %d failures\n", g_fail);
    return 1;
  }
  std::printf("recover_mixed_plan_test ok\n");
  return 0;
}
