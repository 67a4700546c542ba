// Stand-alone host program for the planner of the mixed-pattern decode
// (nxec_rs_decode_mixed_plan, nxec::mixed_plan in Decode mode,
// nxec::mixed_tables with copies): no device, no libnxec.  Built with
// -fsanitize=address,undefined (make build/decode_mixed_plan_test) from the
// planner source and gf_host.cpp.
//
// Cases:
//  * every erasure set of 0..n-k chunks of five geometries, one stripe per
//    set: result is the number of erased data chunks exactly where
//    nxec_rs_plan(is_repair = 0) + nxec_rs_decode_matrix succeed, SINGULAR
//    where the matrix does not invert; plans are counted by input set;
//  * every set of n-k+1 chunks is LOST;
//  * random maps: verdicts and counters against a direct per-stripe
//    evaluation, and the device tables by brute force: every decoded stripe
//    has each of its k outputs produced exactly once (an inverse row or a
//    copy), rows and copies are those of nxec_rs_decode_stripes' own plan,
//    every offset lies inside its stripe, no erased chunk is a source, items
//    run by segment then ascending stripe, copies belong to a plan's first
//    segment only, unused rows and entries are zero / kNoCopy.
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

// every subset of `size` ids out of n
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

// What nxec_rs_decode_stripes plans for the erased list e: the verdict, the
// first k alive ids, the erased data ids and their inverse rows.
int direct(int n, int k, const std::vector<int32_t> &e, std::vector<int32_t> *inputs, std::vector<int32_t> *targets,
           std::vector<unsigned char> *rows) {
  if (static_cast<int>(e.size()) > n - k) return NXEC_RECOVER_LOST;
  std::vector<int32_t> in(n), t;
  int ni = 0, mi = 0;
  const int rc = nxec_rs_plan(n, k, e.data(), static_cast<int>(e.size()), 0, in.data(), &ni, &mi, nullptr);
  EXPECT(rc == NXEC_OK && ni >= k, "(%d,%d) nxec_rs_plan rc %d", n, k, rc);
  for (int32_t c : e)
    if (c < k) t.push_back(c);
  std::vector<unsigned char> m(std::max<size_t>(1, t.size() * k));
  if (!t.empty()) {
    const int rc2 = nxec_rs_decode_matrix(n, k, in.data(), t.data(), static_cast<int>(t.size()), m.data());
    if (rc2 == NXEC_ERR_SINGULAR) return NXEC_RECOVER_SINGULAR;
    EXPECT(rc2 == NXEC_OK, "(%d,%d) nxec_rs_decode_matrix rc %d", n, k, rc2);
  }
  if (inputs) inputs->assign(in.begin(), in.begin() + k);
  if (targets) *targets = t;
  if (rows) *rows = m;
  return static_cast<int>(t.size());
}

void enumerate(int n, int k, int64_t want_sets, int64_t want_singular) {
  std::vector<std::vector<int32_t>> sets;
  for (int size = 0; size <= n - k; size++) subsets(n, size, sets);
  const size_t ndec = sets.size();
  subsets(n, n - k + 1, sets);  // LOST
  const int64_t ns = static_cast<int64_t>(sets.size());
  std::vector<unsigned char> alive(static_cast<size_t>(ns) * n, 1);
  for (int64_t s = 0; s < ns; s++)
    for (int32_t c : sets[s]) alive[s * n + c] = 0;
  std::vector<int32_t> res(ns, 12345);
  int64_t np = -1, nseg = -1, nd = -1;
  EXPECT(nxec_rs_decode_mixed_plan(n, k, alive.data(), ns, res.data(), &np, &nseg, &nd) == NXEC_OK, "(%d,%d) rc", n, k);
  int64_t singular = 0, decoded = 0;
  std::map<std::vector<int32_t>, int> plans;  // input set -> |T|
  for (size_t s = 0; s < sets.size(); s++) {
    std::vector<int32_t> in;
    const int want = direct(n, k, sets[s], &in, nullptr, nullptr);
    EXPECT(res[s] == want, "(%d,%d) set %zu of %zu ids: result %d, want %d", n, k, s, sets[s].size(), res[s], want);
    if (s >= ndec) EXPECT(res[s] == NXEC_RECOVER_LOST, "(%d,%d) n-k+1 erased: %d", n, k, res[s]);
    singular += want == NXEC_RECOVER_SINGULAR;
    if (want >= 0) {
      decoded++;
      plans[in] = want;
    }
  }
  int64_t segs = 0;
  for (const auto &p : plans) segs += std::max(1, (p.second + 3) / 4);
  EXPECT(static_cast<int64_t>(ndec) == want_sets, "(%d,%d) %zu sets of 0..n-k ids, pinned %lld", n, k, ndec,
         static_cast<long long>(want_sets));
  EXPECT(singular == want_singular, "(%d,%d) %lld singular sets, pinned %lld", n, k, static_cast<long long>(singular),
         static_cast<long long>(want_singular));
  EXPECT(np == static_cast<int64_t>(plans.size()) && nd == decoded && nseg == segs,
         "(%d,%d) counters %lld %lld %lld, want %zu %lld %lld", n, k, static_cast<long long>(np),
         static_cast<long long>(nseg), static_cast<long long>(nd), plans.size(), static_cast<long long>(segs),
         static_cast<long long>(decoded));
  // the same batch twice: no new plan
  std::vector<unsigned char> twice(alive);
  twice.insert(twice.end(), alive.begin(), alive.end());
  int64_t np2 = -1, nseg2 = -1, nd2 = -1;
  EXPECT(nxec_rs_decode_mixed_plan(n, k, twice.data(), 2 * ns, nullptr, &np2, &nseg2, &nd2) == NXEC_OK, "twice rc");
  EXPECT(np2 == np && nseg2 == nseg && nd2 == 2 * nd, "(%d,%d) duplicated plans counted again", n, k);
}

// The device tables of `alive` against a brute-force walk of every item.
void check_tables(int n, int k, const std::vector<unsigned char> &alive, int64_t ns, int64_t cs, int64_t ocs, int64_t len) {
  std::vector<int32_t> res(ns, 777);
  nxec::MixedPlan plan;
  nxec::mixed_plan(nxec::MixedMode::Decode, n, k, alive.data(), ns, res.data(), &plan);
  std::set<std::vector<int32_t>> distinct;
  int64_t decoded = 0, segs = 0;
  for (int64_t s = 0; s < ns; s++) {
    std::vector<int32_t> e, in, t;
    for (int c = 0; c < n; c++)
      if (!alive[s * n + c]) e.push_back(c);
    const int want = direct(n, k, e, &in, &t, nullptr);
    EXPECT(res[s] == want, "(%d,%d) stripe %lld: %d, want %d", n, k, static_cast<long long>(s), res[s], want);
    EXPECT((plan.plan_of[s] >= 0) == (want >= 0), "plan_of of stripe %lld", static_cast<long long>(s));
    if (want < 0 || plan.plan_of[s] < 0) continue;
    decoded++;
    if (distinct.insert(in).second) segs += std::max(1, (want + 3) / 4);
    const nxec::MixedPlan::Plan &pl = plan.plans[plan.plan_of[s]];
    EXPECT(pl.inputs == in && pl.targets == t, "stripe %lld mapped to another plan", static_cast<long long>(s));
    // the by-runs list makes the same plan through nxec_rs_decode_stripes' own steps
    std::vector<int32_t> in2, t2;
    EXPECT(direct(n, k, pl.erased, &in2, &t2, nullptr) == want && in2 == in && t2 == t, "by-runs erased list of stripe %lld",
           static_cast<long long>(s));
    for (int32_t c : pl.erased) EXPECT(!alive[s * n + c], "stripe %lld: by-runs list erases a live chunk", static_cast<long long>(s));
  }
  EXPECT(plan.nstripes_planned == decoded && plan.nsegments == segs && plan.plans.size() == distinct.size(),
         "(%d,%d) counters", n, k);
  if (k > nxec::kMaxRaggedK) return;
  std::vector<nxec::MixedSeg> sg;
  std::vector<uint32_t> order, seg_of;
  nxec::mixed_tables(plan, k, cs, ocs, true, sg, order, seg_of);
  EXPECT(static_cast<int64_t>(sg.size()) == segs && order.size() == seg_of.size(), "(%d,%d) table sizes", n, k);
  std::map<uint32_t, int> times;                    // stripe -> items
  std::map<uint32_t, std::vector<int>> produced;    // stripe -> times each data chunk is written
  std::map<uint32_t, uint32_t> first_seg;           // stripe -> its first segment
  for (size_t i = 0; i < order.size(); i++) {
    if (i) EXPECT(seg_of[i] > seg_of[i - 1] || (seg_of[i] == seg_of[i - 1] && order[i] > order[i - 1]),
                  "(%d,%d) item %zu out of order", n, k, i);
    if (seg_of[i] >= sg.size() || order[i] >= ns) {
      EXPECT(false, "(%d,%d) item %zu out of range", n, k, i);
      continue;
    }
    const uint32_t s = order[i];
    times[s]++;
    const bool first = first_seg.emplace(s, seg_of[i]).second;
    std::vector<int> &made = produced[s];
    made.resize(k, 0);
    const nxec::MixedSeg &g = sg[seg_of[i]];
    std::vector<int32_t> e, in, t;
    std::vector<unsigned char> rm;
    for (int c = 0; c < n; c++)
      if (!alive[static_cast<size_t>(s) * n + c]) e.push_back(c);
    direct(n, k, e, &in, &t, &rm);
    EXPECT(g.rows <= 4 && (g.rows >= 1 || t.empty()), "rows %u of a plan with %zu targets", g.rows, t.size());
    for (int j = 0; j < nxec::kMaxRaggedK; j++) {
      if (j >= k) {
        EXPECT(g.src_off[j] == 0 && g.copy_off[j] == nxec::kNoCopy, "entry %d past k is set", j);
        continue;
      }
      EXPECT(g.src_off[j] == static_cast<uint32_t>(in[j] * cs), "src_off[%d]", j);
      EXPECT(static_cast<int64_t>(g.src_off[j]) + len <= n * cs, "src_off[%d] out of the stripe", j);
      EXPECT(alive[static_cast<size_t>(s) * n + in[j]] != 0, "an erased chunk is a source");
      if (g.copy_off[j] == nxec::kNoCopy) {
        EXPECT(!first || in[j] >= k, "stripe %u: data source %d is not copied in the first segment", s, in[j]);
        continue;
      }
      EXPECT(first, "stripe %u: a copy in a later segment", s);
      EXPECT(in[j] < k && g.copy_off[j] == static_cast<uint32_t>(in[j] * ocs), "copy_off[%d] of source %d", j, in[j]);
      EXPECT(static_cast<int64_t>(g.copy_off[j]) + len <= (k - 1) * ocs + len, "copy_off[%d] out of the output stripe", j);
      if (in[j] < k) made[in[j]]++;
    }
    for (uint32_t r = 0; r < 4; r++) {
      if (r >= g.rows) {
        EXPECT(g.dst_off[r] == 0, "unused destination %u set", r);
        for (int j = 0; j < k; j++) EXPECT(g.coef[r * k + j] == 0, "unused coefficient row %u not zero", r);
        continue;
      }
      const int32_t id = static_cast<int32_t>(g.dst_off[r] / ocs);
      EXPECT(g.dst_off[r] % ocs == 0 && id < k && !alive[static_cast<size_t>(s) * n + id], "a row goes to a live or parity chunk");
      if (id >= k) continue;
      made[id]++;
      const size_t pos = std::find(t.begin(), t.end(), id) - t.begin();
      EXPECT(pos < t.size() && std::memcmp(g.coef + r * k, rm.data() + pos * k, k) == 0, "row of chunk %d", id);
    }
  }
  for (int64_t s = 0; s < ns; s++) {
    const int want = res[s] >= 0 ? std::max(1, (res[s] + 3) / 4) : 0;
    const auto it = times.find(static_cast<uint32_t>(s));
    EXPECT((it == times.end() ? 0 : it->second) == want, "stripe %lld: items", static_cast<long long>(s));
    if (res[s] < 0) continue;
    const std::vector<int> &made = produced[static_cast<uint32_t>(s)];
    for (int j = 0; j < k; j++)
      EXPECT(static_cast<int>(made.size()) == k && made[j] == 1, "stripe %lld: data chunk %d produced %d times",
             static_cast<long long>(s), j, made.size() == static_cast<size_t>(k) ? made[j] : -1);
  }
}

void random_maps(int n, int k, uint32_t seed, int max_erased, int64_t ns) {
  std::mt19937 rng(seed);
  std::vector<unsigned char> alive(static_cast<size_t>(ns) * n);
  for (int64_t s = 0; s < ns; s++) {
    const int ne = static_cast<int>(rng() % (max_erased + 1));
    for (int c = 0; c < n; c++) alive[s * n + c] = static_cast<unsigned char>(1 + rng() % 255);  // any non-zero is alive
    for (int i = 0; i < ne; i++) alive[s * n + rng() % n] = 0;
  }
  check_tables(n, k, alive, ns, 4096 + 48, 4096 + 16, 4096);
}

// every erasure set of 0..n-k chunks and the LOST ones, as one small batch through the tables
void every_set_tables(int n, int k) {
  std::vector<std::vector<int32_t>> sets;
  for (int size = 0; size <= n - k + 1; size++) subsets(n, size, sets);
  const int64_t ns = static_cast<int64_t>(sets.size());
  std::vector<unsigned char> alive(static_cast<size_t>(ns) * n, 1);
  for (int64_t s = 0; s < ns; s++)
    for (int32_t c : sets[s]) alive[s * n + c] = 0;
  check_tables(n, k, alive, ns, 64, 80, 64);
}

}  // namespace

int main() {
  enumerate(6, 4, 22, 0);
  enumerate(14, 10, 1471, 0);
  enumerate(10, 4, 848, 0);
  enumerate(23, 19, 10903, 0);
  enumerate(12, 6, 2510, 10);
  {  // (12,6): a singular set, and a parity-only loss
    unsigned char alive[12];
    int32_t r = 55;
    std::memset(alive, 1, sizeof alive);
    for (int c : {0, 2, 5, 7, 8}) alive[c] = 0;
    EXPECT(nxec_rs_decode_mixed_plan(12, 6, alive, 1, &r, nullptr, nullptr, nullptr) == NXEC_OK && r == NXEC_RECOVER_SINGULAR,
           "(12,6) {0,2,5,7,8}: %d", r);
    std::memset(alive, 1, sizeof alive);
    for (int c = 6; c < 12; c++) alive[c] = 0;
    int64_t np = 0, nsg = 0, nd = 0;
    EXPECT(nxec_rs_decode_mixed_plan(12, 6, alive, 1, &r, &np, &nsg, &nd) == NXEC_OK && r == 0 && np == 1 && nsg == 1 && nd == 1,
           "(12,6) parity-only loss: %d", r);
  }
  every_set_tables(6, 4);
  every_set_tables(10, 4);
  every_set_tables(12, 6);  // five lost data chunks: two segments, copies once
  random_maps(14, 10, 1, 6, 4000);
  random_maps(10, 4, 2, 7, 4000);
  random_maps(6, 4, 3, 3, 1000);
  random_maps(23, 19, 5, 5, 2000);
  random_maps(24, 21, 4, 4, 1000);
  // argument validation
  unsigned char a[8] = {1, 1, 1, 1, 1, 1, 1, 1};
  int32_t r = 55;
  EXPECT(nxec_rs_decode_mixed_plan(0, 0, a, 1, &r, nullptr, nullptr, nullptr) == NXEC_ERR_INVALID, "n = 0 accepted");
  EXPECT(nxec_rs_decode_mixed_plan(4, 5, a, 1, &r, nullptr, nullptr, nullptr) == NXEC_ERR_INVALID, "k > n accepted");
  EXPECT(nxec_rs_decode_mixed_plan(6, 4, nullptr, 1, &r, nullptr, nullptr, nullptr) == NXEC_ERR_INVALID, "null alive accepted");
  EXPECT(nxec_rs_decode_mixed_plan(6, 4, a, -1, &r, nullptr, nullptr, nullptr) == NXEC_ERR_INVALID, "negative nstripes accepted");
  EXPECT(r == 55, "a refused call wrote the result");
  int64_t np = 9, nsg = 9, nd = 9;
  EXPECT(nxec_rs_decode_mixed_plan(6, 4, nullptr, 0, nullptr, &np, &nsg, &nd) == NXEC_OK && np == 0 && nsg == 0 && nd == 0,
         "empty batch");
  a[2] = 0;
  int32_t rr[2] = {55, 55};
  EXPECT(nxec_rs_decode_mixed_plan(4, 4, a, 2, rr, &np, &nsg, &nd) == NXEC_OK && rr[0] == NXEC_RECOVER_LOST && rr[1] == 0 &&
             np == 1 && nsg == 1 && nd == 1, "n == k: an erased chunk is lost, a clean stripe is k copies");
  if (g_fail) {
    std::fprintf(stderr, "decode_mixed_plan_test: %d failures\n", g_fail);
    return 1;
  }
  std::printf("decode_mixed_plan_test ok\n");
  return 0;
}
