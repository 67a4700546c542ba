// Host half of the delta update (include/nxec.h §4, nxec_rs_update_stripes):
// validation of the update list, the rounds, the split of every update into
// vector tiles and byte items, and the tables the kernels read.  Pure
// arithmetic, no device: compiled alone under sanitizers by
// tests/cpp/update_plan_test.cc.
#include <algorithm>
#include <numeric>
#include <vector>

#include "nxec.h"
#include "nxec_internal.h"

namespace nxec {

namespace {

// [a0, a1) and [b0, b1) share a byte
bool intersects(uintptr_t a0, uintptr_t a1, uintptr_t b0, uintptr_t b1) { return a0 < b1 && b0 < a1; }

}  // namespace

int update_plan(int n, int k, int64_t cs, int64_t ss, int64_t len, int64_t nstripes, uintptr_t stripes_addr,
                const nxec_update *updates, int64_t nupdates, UpdatePlan *plan) {
  if (!valid_nk(n, k)) return set_error(NXEC_ERR_INVALID, "invalid (n,k)=(%d,%d)", n, k);
  if (cs < 0 || ss < 0 || len < 0 || nstripes < 0 || nupdates < 0)
    return set_error(NXEC_ERR_INVALID, "update: negative stride, len, nstripes or nupdates");
  if (!updates && nupdates > 0) return set_error(NXEC_ERR_INVALID, "update: null update list");
  const uintptr_t batch_end = stripes_addr + static_cast<uintptr_t>(nstripes) * static_cast<uintptr_t>(ss);
  std::vector<int64_t> live;  // updates with length > 0
  for (int64_t i = 0; i < nupdates; i++) {
    const nxec_update &u = updates[i];
    if (u.stripe < 0 || u.stripe >= nstripes || u.chunk < 0 || u.chunk >= k)
      return set_error(NXEC_ERR_INVALID, "update %lld: stripe %lld or chunk %d out of range", static_cast<long long>(i),
                       static_cast<long long>(u.stripe), u.chunk);
    if (u.reserved != 0) return set_error(NXEC_ERR_INVALID, "update %lld: reserved != 0", static_cast<long long>(i));
    if (u.offset < 0 || u.length < 0 || u.offset > len || u.length > len - u.offset)
      return set_error(NXEC_ERR_INVALID, "update %lld: byte range outside the chunk", static_cast<long long>(i));
    if (u.length == 0) continue;
    if (!u.d_new) return set_error(NXEC_ERR_INVALID, "update %lld: null d_new", static_cast<long long>(i));
    const uintptr_t p = reinterpret_cast<uintptr_t>(u.d_new);
    if (intersects(p, p + static_cast<uintptr_t>(u.length), stripes_addr, batch_end))
      return set_error(NXEC_ERR_INVALID, "update %lld: d_new lies inside the batch", static_cast<long long>(i));
    live.push_back(i);
  }
  UpdatePlan local;
  UpdatePlan &p = plan ? *plan : local;
  p = UpdatePlan{};
  if (live.empty()) return NXEC_OK;
  // chunk byte offsets inside a stripe stay 32-bit (the kernels' scalar address math)
  if (!stripe_fits32(n, cs, len))
    return set_error(NXEC_ERR_INVALID, "update: chunk offset out of range (chunks of a stripe must lie within 4 GiB)");

  // by stripe, then by first column: the order the interval colouring wants
  std::sort(live.begin(), live.end(), [&](int64_t a, int64_t b) {
    const nxec_update &x = updates[a], &y = updates[b];
    if (x.stripe != y.stripe) return x.stripe < y.stripe;
    if (x.offset != y.offset) return x.offset < y.offset;
    return x.chunk < y.chunk;
  });
  // Greedy colouring of each stripe's column intervals in order of their first
  // column: an interval takes the lowest round whose intervals of this stripe
  // all ended at or before its first column.  The rounds used equal the most
  // intervals over one column, at most k (one per chunk).
  std::vector<int32_t> round_of(live.size());
  std::vector<int64_t> chunk_end(static_cast<size_t>(k)), round_end;
  int nrounds = 0;
  for (size_t i = 0; i < live.size();) {
    const int64_t stripe = updates[live[i]].stripe;
    std::fill(chunk_end.begin(), chunk_end.end(), 0);
    round_end.clear();
    for (; i < live.size() && updates[live[i]].stripe == stripe; i++) {
      const nxec_update &u = updates[live[i]];
      if (chunk_end[u.chunk] > u.offset)
        return set_error(NXEC_ERR_INVALID, "update %lld: intersects another update of stripe %lld chunk %d",
                         static_cast<long long>(live[i]), static_cast<long long>(stripe), u.chunk);
      chunk_end[u.chunk] = u.offset + u.length;
      size_t r = 0;
      while (r < round_end.size() && round_end[r] > u.offset) r++;
      if (r == round_end.size()) round_end.push_back(0);
      round_end[r] = u.offset + u.length;
      round_of[i] = static_cast<int32_t>(r);
    }
    nrounds = std::max(nrounds, static_cast<int>(round_end.size()));
  }

  const bool vec_layout = k <= kMaxRaggedK && stripes_addr % 16 == 0 && cs % 16 == 0 && ss % 16 == 0;
  // stable by round: inside a round the items stay in (stripe, column) order
  std::vector<size_t> order(live.size());
  std::iota(order.begin(), order.end(), size_t(0));
  std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return round_of[a] < round_of[b]; });
  std::vector<UpdateItem> bytes;  // the current round's byte items
  size_t at = 0;
  for (int r = 0; r < nrounds; r++) {
    UpdateRound rd{};
    rd.vec_item0 = p.items.size();
    rd.tile0 = p.tile_item.size();
    rd.prefix0 = p.byte_prefix.size();
    bytes.clear();
    for (; at < order.size() && round_of[order[at]] == r; at++) {
      const nxec_update &u = updates[live[order[at]]];
      rd.nupdates++;
      const int64_t end = u.offset + u.length;
      int64_t b0 = (u.offset + 15) / 16 * 16, b1 = end / 16 * 16;  // the body: whole 16-byte columns
      const bool vec = vec_layout && b0 < b1 && (reinterpret_cast<uintptr_t>(u.d_new) + (b0 - u.offset)) % 16 == 0;
      if (!vec) b0 = b1 = u.offset;  // no body: one byte item
      auto item = [&](int64_t c0, int64_t count) {
        return UpdateItem{u.d_new + (c0 - u.offset), u.stripe * ss, static_cast<uint32_t>(c0),
                          static_cast<uint32_t>(u.chunk), 0, static_cast<uint32_t>(count)};
      };
      if (vec) {
        UpdateItem it = item(b0, (b1 - b0) / 16);
        const int64_t tiles = (it.count + kUpdateTileVecs - 1) / kUpdateTileVecs;
        if (rd.ntiles + tiles >= (int64_t(1) << 32) || p.items.size() + bytes.size() >= (size_t(1) << 31))
          return set_error(NXEC_ERR_INVALID, "update: too many tiles for one launch (split the update list)");
        it.first = static_cast<uint32_t>(rd.ntiles);
        p.tile_item.insert(p.tile_item.end(), static_cast<size_t>(tiles), static_cast<uint32_t>(p.items.size()));
        p.items.push_back(it);
        rd.ntiles += tiles;
        rd.nvec_items++;
        if (u.offset < b0) bytes.push_back(item(u.offset, b0 - u.offset));
      }
      if (b1 < end) bytes.push_back(item(b1, end - b1));
    }
    rd.byte_item0 = p.items.size();
    rd.nbyte_items = static_cast<int64_t>(bytes.size());
    for (const UpdateItem &it : bytes) {
      p.byte_prefix.push_back(rd.nbytes);
      rd.nbytes += it.count;
    }
    p.byte_prefix.push_back(rd.nbytes);
    p.items.insert(p.items.end(), bytes.begin(), bytes.end());
    p.nvec_tiles += rd.ntiles;
    p.nbyte_items += rd.nbyte_items;
    p.rounds.push_back(rd);
  }
  return NXEC_OK;
}

}  // namespace nxec

extern "C" int nxec_rs_update_plan(int n, int k, int64_t chunk_stride, int64_t stripe_stride, int64_t len,
                                   int64_t nstripes, uintptr_t stripes_addr, const nxec_update *updates,
                                   int64_t nupdates, int64_t *nrounds, int64_t *nvec_tiles, int64_t *nbyte_items) {
  nxec::UpdatePlan plan;
  if (int rc = nxec::update_plan(n, k, chunk_stride, stripe_stride, len, nstripes, stripes_addr, updates, nupdates,
                                 &plan))
    return rc;
  if (nrounds) *nrounds = static_cast<int64_t>(plan.rounds.size());
  if (nvec_tiles) *nvec_tiles = plan.nvec_tiles;
  if (nbyte_items) *nbyte_items = plan.nbyte_items;
  return NXEC_OK;
}
