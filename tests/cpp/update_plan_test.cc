// Stand-alone host program for the planner of the delta update
// (nxec_rs_update_plan, nxec::update_plan): no device, no libnxec.  Built with
// -fsanitize=address,undefined (make build/update_plan_test) from the planner
// source and gf_host.cpp.
//
// Cases, over seeded update lists of six geometries, packed and padded
// layouts, aligned and unaligned batch addresses:
//  * the device tables on the host: every tile maps to a vector item and is
//    not empty, vector items are 16-byte aligned in column and d_new and only
//    exist where the layout allows them, the byte prefix is the running sum;
//  * over a byte map of the batch, the tiles and items of one round never
//    touch a byte twice (the invariant that makes the in-place kernel with
//    prefetch safe);
//  * all rounds together touch exactly the bytes the contract names: every
//    updated data byte once, from the d_new byte that belongs to it; every
//    parity byte of a column once per update that covers the column; nothing
//    else (no padding, no other chunk);
//  * the rounds used equal the most updates over one column of one stripe;
//  * the argument validation.
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
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

struct Geometry {
  int n, k;
  int64_t len, cs, ss, nstripes;
  uintptr_t addr;
};

const unsigned char *fake(uintptr_t p) { return reinterpret_cast<const unsigned char *>(p); }

// a seeded list without same-chunk intersections (rejection sampling)
std::vector<nxec_update> draw(const Geometry &g, int count, std::mt19937_64 &rng) {
  std::vector<nxec_update> out;
  const int64_t lens[] = {0, 1, 11, 16, 27, 100, 1024, 16384, 16384 + 20, g.len};
  for (int i = 0; i < count; i++) {
    for (int attempt = 0; attempt < 50; attempt++) {
      nxec_update u{};
      u.stripe = static_cast<int64_t>(rng() % g.nstripes);
      u.chunk = static_cast<int32_t>(rng() % g.k);
      u.length = std::min(lens[rng() % 10], g.len);
      u.offset = static_cast<int64_t>(rng() % (g.len - u.length + 1));
      if (rng() % 3 == 0) u.offset = u.offset / 16 * 16;
      if (rng() % 8 == 0) u.offset = g.len - u.length;
      // d_new: most updates agree with the alignment of their offset, some are off by 4
      const uintptr_t base = (uintptr_t(1) << 40) + (static_cast<uintptr_t>(out.size()) << 24);
      u.d_new = fake(base + static_cast<uintptr_t>(u.offset % 16) + (rng() % 5 == 0 ? 4 : 0));
      bool clash = false;
      for (const nxec_update &o : out)
        clash |= o.stripe == u.stripe && o.chunk == u.chunk && o.length > 0 && u.length > 0 &&
                 o.offset < u.offset + u.length && u.offset < o.offset + o.length;
      if (clash) continue;
      out.push_back(u);
      break;
    }
  }
  return out;
}

void check_list(const Geometry &g, const std::vector<nxec_update> &ups, const char *tag) {
  nxec::UpdatePlan plan;
  const int rc = nxec::update_plan(g.n, g.k, g.cs, g.ss, g.len, g.nstripes, g.addr, ups.data(),
                                   static_cast<int64_t>(ups.size()), &plan);
  EXPECT(rc == NXEC_OK, "%s: rc=%d", tag, rc);
  if (rc) return;
  const int m = g.n - g.k;
  const size_t total = static_cast<size_t>(g.nstripes * g.ss);
  // what the contract names: per batch byte, how often all rounds together may touch it, and for a data
  // byte the d_new address it is written from
  std::vector<int> want(total, 0), got(total, 0), depth(total, 0);
  std::vector<uintptr_t> src(total, 0), got_src(total, 0);
  int64_t live = 0;
  for (const nxec_update &u : ups) {
    live += u.length > 0;
    for (int64_t c = u.offset; c < u.offset + u.length; c++) {
      const size_t d = static_cast<size_t>(u.stripe * g.ss + u.chunk * g.cs + c);
      want[d]++;
      src[d] = reinterpret_cast<uintptr_t>(u.d_new) + static_cast<uintptr_t>(c - u.offset);
      for (int r = 0; r < m; r++) want[static_cast<size_t>(u.stripe * g.ss + (g.k + r) * g.cs + c)]++;
      depth[static_cast<size_t>(u.stripe * g.ss + c)]++;  // updates over column c of the stripe
    }
  }
  const int max_depth = *std::max_element(depth.begin(), depth.end());
  EXPECT(static_cast<int>(plan.rounds.size()) == max_depth, "%s: %zu rounds, depth %d", tag, plan.rounds.size(),
         max_depth);
  const bool vec_layout = g.k <= nxec::kMaxRaggedK && g.addr % 16 == 0 && g.cs % 16 == 0 && g.ss % 16 == 0;
  int64_t tiles = 0, byte_items = 0, nupdates = 0;
  std::vector<int> seen(total);
  for (const nxec::UpdateRound &rd : plan.rounds) {
    std::fill(seen.begin(), seen.end(), 0);
    // one work item's columns [c0, c0 + nbytes) of its data chunk and of every parity chunk
    auto touch = [&](const nxec::UpdateItem &it, int64_t c0, int64_t nbytes, uintptr_t from) {
      EXPECT(it.stripe_off % g.ss == 0 && it.stripe_off / g.ss < g.nstripes && static_cast<int>(it.chunk) < g.k &&
                 c0 + nbytes <= g.len,
             "%s: item out of range", tag);
      for (int64_t c = c0; c < c0 + nbytes; c++) {
        const size_t d = static_cast<size_t>(it.stripe_off + it.chunk * g.cs + c);
        seen[d]++;
        got[d]++;
        got_src[d] = from + static_cast<uintptr_t>(c - c0);
        for (int r = 0; r < m; r++) {
          const size_t p = static_cast<size_t>(it.stripe_off + (g.k + r) * g.cs + c);
          seen[p]++;
          got[p]++;
        }
      }
    };
    EXPECT(rd.nvec_items == 0 || vec_layout, "%s: vector items on a layout that has none", tag);
    int64_t next_tile = 0;
    for (int64_t i = 0; i < rd.nvec_items; i++) {
      const nxec::UpdateItem &it = plan.items[rd.vec_item0 + static_cast<size_t>(i)];
      EXPECT(it.col % 16 == 0 && reinterpret_cast<uintptr_t>(it.d_new) % 16 == 0 && it.count > 0,
             "%s: vector item misaligned or empty", tag);
      EXPECT(it.first == next_tile, "%s: tiles of the items do not follow each other", tag);
      const int64_t nt = (it.count + nxec::kUpdateTileVecs - 1) / nxec::kUpdateTileVecs;
      for (int64_t t = 0; t < nt; t++) {
        EXPECT(plan.tile_item[rd.tile0 + static_cast<size_t>(next_tile + t)] == rd.vec_item0 + static_cast<size_t>(i),
               "%s: tile map", tag);
        // the tile as the kernel walks it: vectors [t*1024, min(count, (t+1)*1024))
        const int64_t v0 = t * nxec::kUpdateTileVecs;
        const int64_t v1 = std::min<int64_t>(it.count, v0 + nxec::kUpdateTileVecs);
        EXPECT(v0 < v1, "%s: empty tile", tag);
        touch(it, it.col + v0 * 16, (v1 - v0) * 16, reinterpret_cast<uintptr_t>(it.d_new) + static_cast<uintptr_t>(v0 * 16));
      }
      next_tile += nt;
    }
    EXPECT(next_tile == rd.ntiles, "%s: tile count", tag);
    EXPECT(rd.byte_item0 == rd.vec_item0 + static_cast<size_t>(rd.nvec_items), "%s: byte items follow the vector items", tag);
    int64_t run = 0;
    for (int64_t i = 0; i < rd.nbyte_items; i++) {
      const nxec::UpdateItem &it = plan.items[rd.byte_item0 + static_cast<size_t>(i)];
      EXPECT(plan.byte_prefix[rd.prefix0 + static_cast<size_t>(i)] == run && it.count > 0, "%s: byte prefix", tag);
      EXPECT(!vec_layout || it.count < 16 || reinterpret_cast<uintptr_t>(it.d_new) % 16 != it.col % 16 ||
                 (it.col + 15) / 16 * 16 + 16 > it.col + it.count,
             "%s: a byte item holds a vector body", tag);
      touch(it, it.col, it.count, reinterpret_cast<uintptr_t>(it.d_new));
      run += it.count;
    }
    EXPECT(plan.byte_prefix[rd.prefix0 + static_cast<size_t>(rd.nbyte_items)] == run && rd.nbytes == run,
           "%s: byte total", tag);
    const int twice = *std::max_element(seen.begin(), seen.end());
    EXPECT(twice <= 1, "%s: a round touches a byte %d times", tag, twice);
    tiles += rd.ntiles;
    byte_items += rd.nbyte_items;
    nupdates += rd.nupdates;
  }
  EXPECT(got == want, "%s: the rounds do not touch exactly the contract's bytes", tag);
  EXPECT(got_src == src, "%s: a data byte is written from the wrong d_new byte", tag);
  EXPECT(tiles == plan.nvec_tiles && byte_items == plan.nbyte_items && nupdates == live, "%s: counters", tag);
  if (!vec_layout) EXPECT(plan.nvec_tiles == 0 && plan.nbyte_items == live, "%s: byte-only layout", tag);
  // the exported call reports the same counters
  int64_t nr = -1, nt = -1, nb = -1;
  EXPECT(nxec_rs_update_plan(g.n, g.k, g.cs, g.ss, g.len, g.nstripes, g.addr, ups.data(), static_cast<int64_t>(ups.size()),
                             &nr, &nt, &nb) == NXEC_OK &&
             nr == static_cast<int64_t>(plan.rounds.size()) && nt == plan.nvec_tiles && nb == plan.nbyte_items,
         "%s: nxec_rs_update_plan", tag);
}

void seeded_lists() {
  const int nk[][2] = {{6, 4}, {5, 4}, {14, 10}, {10, 4}, {23, 19}, {24, 21}, {4, 4}};
  const int64_t lens[] = {16, 100, 4096 + 5, 16384 + 16, 3 * 16384 + 48};
  std::mt19937_64 rng(20240607);
  int cases = 0;
  for (const auto &g0 : nk) {
    for (int64_t len : lens) {
      for (int layout = 0; layout < 4; layout++) {
        Geometry g{g0[0], g0[1], len, len, 0, 3, 0x10000};
        if (layout == 1) g.cs = len + 48;
        if (layout == 3) g.addr += 3;
        g.ss = g.n * g.cs + (layout == 2 ? g.cs : 0);
        char tag[96];
        std::snprintf(tag, sizeof tag, "(%d,%d) len %lld layout %d", g.n, g.k, static_cast<long long>(len), layout);
        check_list(g, draw(g, 1 + static_cast<int>(rng() % 30), rng), tag);
        cases++;
      }
    }
  }
  // all k chunks of one stripe over the whole length: k rounds of one update each
  Geometry g{6, 4, 16384 + 16, 16384 + 16, 6 * (16384 + 16), 2, 0x10000};
  std::vector<nxec_update> all;
  for (int j = 0; j < g.k; j++) all.push_back({1, j, 0, 0, g.len, fake((uintptr_t(1) << 40) + (uintptr_t(j) << 24))});
  check_list(g, all, "all chunks");
  nxec::UpdatePlan plan;
  EXPECT(nxec::update_plan(g.n, g.k, g.cs, g.ss, g.len, g.nstripes, g.addr, all.data(), 4, &plan) == NXEC_OK &&
             plan.rounds.size() == 4 && plan.nvec_tiles == 8 && plan.nbyte_items == 0,
         "all chunks: rounds");
  std::printf("seeded lists: %d\n", cases);
}

void validation() {
  const Geometry g{6, 4, 64, 64, 6 * 64, 2, 0x10000};
  const unsigned char *nw = fake(uintptr_t(1) << 40);
  auto call = [&](std::vector<nxec_update> ups, int n = 6, int k = 4, int64_t cs = 64, int64_t ss = 384, int64_t len = 64,
                  int64_t ns = 2) {
    return nxec::update_plan(n, k, cs, ss, len, ns, g.addr, ups.data(), static_cast<int64_t>(ups.size()), nullptr);
  };
  const nxec_update ok{0, 1, 0, 8, 16, nw};
  EXPECT(call({ok}) == NXEC_OK, "a valid update");
  EXPECT(call({}) == NXEC_OK, "an empty list");
  EXPECT(call({ok}, 4, 5) == NXEC_ERR_INVALID && call({ok}, 0, 0) == NXEC_ERR_INVALID, "(n,k)");
  EXPECT(call({ok}, 6, 4, -64) == NXEC_ERR_INVALID && call({ok}, 6, 4, 64, -1) == NXEC_ERR_INVALID &&
             call({ok}, 6, 4, 64, 384, -1) == NXEC_ERR_INVALID && call({ok}, 6, 4, 64, 384, 64, -1) == NXEC_ERR_INVALID,
         "negative sizes");
  EXPECT(nxec::update_plan(6, 4, 64, 384, 64, 2, g.addr, nullptr, 1, nullptr) == NXEC_ERR_INVALID, "null list");
  EXPECT(nxec::update_plan(6, 4, 64, 384, 64, 2, g.addr, &ok, -1, nullptr) == NXEC_ERR_INVALID, "negative count");
  auto with = [&](auto edit) {
    nxec_update u = ok;
    edit(u);
    return call({u});
  };
  EXPECT(with([](nxec_update &u) { u.stripe = 2; }) == NXEC_ERR_INVALID, "stripe past the batch");
  EXPECT(with([](nxec_update &u) { u.stripe = -1; }) == NXEC_ERR_INVALID, "negative stripe");
  EXPECT(with([](nxec_update &u) { u.chunk = 4; }) == NXEC_ERR_INVALID, "a parity chunk");
  EXPECT(with([](nxec_update &u) { u.chunk = -1; }) == NXEC_ERR_INVALID, "negative chunk");
  EXPECT(with([](nxec_update &u) { u.reserved = 1; }) == NXEC_ERR_INVALID, "reserved");
  EXPECT(with([](nxec_update &u) { u.offset = -1; }) == NXEC_ERR_INVALID, "negative offset");
  EXPECT(with([](nxec_update &u) { u.length = -1; }) == NXEC_ERR_INVALID, "negative length");
  EXPECT(with([](nxec_update &u) { u.offset = 49; }) == NXEC_ERR_INVALID, "range past the chunk");
  EXPECT(with([](nxec_update &u) { u.offset = 48; }) == NXEC_OK, "range up to the chunk's end");
  EXPECT(with([](nxec_update &u) { u.length = INT64_MAX; }) == NXEC_ERR_INVALID, "length overflow");
  EXPECT(with([](nxec_update &u) { u.d_new = nullptr; }) == NXEC_ERR_INVALID, "null d_new");
  EXPECT(with([](nxec_update &u) { u.d_new = nullptr; u.length = 0; }) == NXEC_OK, "null d_new of an empty update");
  EXPECT(with([&](nxec_update &u) { u.d_new = fake(g.addr + 2 * 384 - 1); }) == NXEC_ERR_INVALID, "d_new on the batch's last byte");
  EXPECT(with([&](nxec_update &u) { u.d_new = fake(g.addr - 16); }) == NXEC_OK, "d_new up to the batch");
  EXPECT(with([&](nxec_update &u) { u.d_new = fake(g.addr - 15); }) == NXEC_ERR_INVALID, "d_new into the batch");
  EXPECT(with([&](nxec_update &u) { u.d_new = fake(g.addr + 2 * 384); }) == NXEC_OK, "d_new right after the batch");
  // same chunk: one shared byte is an error, adjacent ranges are not; other chunks may share columns
  EXPECT(call({{0, 1, 0, 8, 16, nw}, {0, 1, 0, 23, 4, nw}}) == NXEC_ERR_INVALID, "one shared byte");
  EXPECT(call({{0, 1, 0, 23, 4, nw}, {0, 1, 0, 8, 16, nw}}) == NXEC_ERR_INVALID, "one shared byte, other order");
  EXPECT(call({{0, 1, 0, 8, 16, nw}, {0, 1, 0, 24, 4, nw}, {0, 1, 0, 0, 8, nw}}) == NXEC_OK, "adjacent ranges");
  EXPECT(call({{0, 1, 0, 8, 16, nw}, {0, 2, 0, 8, 16, nw}, {1, 1, 0, 8, 16, nw}}) == NXEC_OK, "other chunk, other stripe");
  EXPECT(call({{0, 1, 0, 8, 16, nw}, {0, 1, 0, 10, 0, nw}}) == NXEC_OK, "an empty update inside another");
  // chunks of a stripe beyond 4 GiB: refused only when there is work
  EXPECT(call({ok}, 6, 4, int64_t(1) << 30, int64_t(6) << 30) == NXEC_ERR_INVALID, "chunk offsets beyond 4 GiB");
  EXPECT(call({{0, 1, 0, 8, 0, nw}}, 6, 4, int64_t(1) << 30, int64_t(6) << 30) == NXEC_OK, "no work, any layout");
  int64_t nr = 7;
  EXPECT(nxec_rs_update_plan(6, 4, 64, 384, 64, 2, g.addr, &ok, 1, nullptr, nullptr, nullptr) == NXEC_OK, "counters optional");
  nxec_update bad = ok;
  bad.reserved = 3;
  EXPECT(nxec_rs_update_plan(6, 4, 64, 384, 64, 2, g.addr, &bad, 1, &nr, &nr, &nr) == NXEC_ERR_INVALID && nr == 7,
         "a refused call writes nothing");
}

}  // namespace

int main() {
  seeded_lists();
  validation();
  if (g_fail) {
    std::fprintf(stderr, "%d failures\n", g_fail);
    return 1;
  }
  std::printf("update_plan_test ok\n");
  return 0;
}
