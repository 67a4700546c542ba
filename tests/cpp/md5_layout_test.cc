// The host rules that keep the fused multiply + MD5 kernels' 32-bit offsets
// from wrapping (nxec_internal.h; no device and no libnxec: all are
// inline): chunk_off32, the contract "(idx * stride) + len <= 2^32 - 1" of every
// strided call, and stripe_fits32, the same rule for a whole stripe;
// mul_md5_layout_ok, the eligibility the three fused call sites share;
// mul_md5_group_cap, the stripes per workgroup that launch_mul_md5 may use at a
// given stripe stride.  With them the other inline host helpers of that header:
// row_passes / pass_rows / pass_coef, the split of a coefficient matrix into
// passes of at most 4 rows.
#include <cstdio>
#include <cstring>
#include <vector>

#include "nxec.h"
#include "nxec_internal.h"

static int fail = 0;
#define CHECK(c)                                                 \
  do {                                                           \
    if (!(c)) {                                                  \
      std::fprintf(stderr, "FAIL line %d: %s\n", __LINE__, #c); \
      fail++;                                                    \
    }                                                            \
  } while (0)

int main() {
  using namespace nxec;
  constexpr int64_t G4 = int64_t(1) << 32;
  uint32_t o = 7;

  // chunk_off32: the last byte a chunk may end at is 2^32 - 2
  CHECK(chunk_off32(0, 0, 0, &o) && o == 0);
  CHECK(chunk_off32(5, 858992638, 4105, &o) && o == 5u * 858992638u && int64_t(o) + 4105 == G4 - 1);
  CHECK(!chunk_off32(5, 858992638, 4106, &o));
  CHECK(chunk_off32(1, G4 - 2, 1, &o) && o == 0xFFFFFFFEu);
  CHECK(!chunk_off32(1, G4 - 1, 1, &o) && !chunk_off32(1, G4, 0, &o) && !chunk_off32(2, int64_t(1) << 62, 0, &o));
  CHECK(chunk_off32(0, G4, 16, &o) && o == 0);  // chunk 0 alone: the stride is never walked
  CHECK(!chunk_off32(-1, 16, 16, &o) && !chunk_off32(1, -16, 16, &o) && !chunk_off32(1, 16, -1, &o));
  CHECK(chunk_off32(0, 16, G4 - 1, &o) && !chunk_off32(0, 16, G4, &o));

  // stripe_fits32(n, stride, len) == chunk_off32(n - 1, stride, len, ..): the rule for a whole stripe
  CHECK(stripe_fits32(6, 858992638, 4105) && 5 * int64_t(858992638) + 4105 == G4 - 1);
  CHECK(!stripe_fits32(6, 858992638, 4106));  // one byte more
  CHECK(stripe_fits32(1, 16, G4 - 1) && !stripe_fits32(1, 16, G4) && !stripe_fits32(1, G4, G4));
  CHECK(stripe_fits32(1, G4, 16));  // one chunk: the stride is never walked
  CHECK(!stripe_fits32(6, -16, 16) && !stripe_fits32(6, 16, -1) && !stripe_fits32(0, 16, 16));
  // (n - 1) * stride wraps int64 here: the hand-written forms of the rule computed it first (UBSan aborts on that)
  CHECK(!stripe_fits32(255, int64_t(1) << 57, 4096) && !stripe_fits32(255, INT64_MAX, 1));
  for (const int64_t nn : {1, 2, 6, 24, 255})
    for (const int64_t st : {int64_t(0), int64_t(16), int64_t(858992638), G4 - 2, G4 - 1, G4, int64_t(1) << 57})
      for (const int64_t ln : {int64_t(0), int64_t(1), int64_t(4105), int64_t(4106), G4 - 1, G4})
        CHECK(stripe_fits32(nn, st, ln) == chunk_off32(nn - 1, st, ln, &o));

  // row_passes / pass_rows / pass_coef: a rows x k matrix in passes of at most 4 rows, at least one pass
  static_assert(kMaxRowsPerPass == 4, "the cases below count in fours");
  for (const int k : {1, 19, NXEC_MAX_K}) {
    for (const int rows : {0, 1, 4, 5, 8, 9}) {
      std::vector<uint8_t> m(static_cast<size_t>(rows) * k);
      for (size_t i = 0; i < m.size(); i++) m[i] = static_cast<uint8_t>(1 + i % 251);  // never zero
      const int passes = row_passes(rows);
      CHECK(passes == (rows == 0 ? 1 : (rows + 3) / 4));
      int total = 0;
      for (int p = 0; p < passes + 1; p++) {  // one pass past the end too: no rows, nothing read
        // exactly the block: ASan guards both ends, and the block starts as 0xEE
        std::vector<uint8_t> coef(static_cast<size_t>(kMaxRowsPerPass) * k, 0xEE);
        const int pr = pass_coef(rows, k, rows ? m.data() : nullptr, p, coef.data());
        CHECK(pr == pass_rows(rows, p) && pr == std::min(4, std::max(0, rows - 4 * p)));
        CHECK(p < passes ? (pr > 0 || rows == 0) : pr == 0);
        for (int r = 0; r < kMaxRowsPerPass; r++)
          for (int j = 0; j < k; j++)
            CHECK(coef[r * k + j] == (r < pr ? m[static_cast<size_t>(4 * p + r) * k + j] : 0));
        total += pr;
      }
      CHECK(total == rows);
      // inside a kernel-argument block of its full size, the bytes past 4 * k stay as they were
      uint8_t block[kMaxRowsPerPass * (NXEC_MAX_K + 1)];
      std::memset(block, 0xEE, sizeof block);
      pass_coef(rows, k, rows ? m.data() : nullptr, 0, block);
      for (size_t i = static_cast<size_t>(kMaxRowsPerPass) * k; i < sizeof block; i++) CHECK(block[i] == 0xEE);
    }
  }

  // mul_md5_layout_ok: RS(20,16) with data chunk 15 at 2^32 - 256 and 512-byte chunks is the layout the
  // fused encode used to take and wrap on; the same start with one 256-byte step less is not legal either
  // (it would end at 2^32), and the last legal 16-aligned start is 2^32 - 272 for one step
  const void *base = reinterpret_cast<const void *>(uintptr_t(1) << 40);
  uint32_t src[NXEC_MAX_K + 1] = {}, dst[kMaxRowsPerPass] = {}, cp[NXEC_MAX_K + 1];
  for (int j = 0; j < 16; j++) src[j] = static_cast<uint32_t>(j * int64_t(286331136)), cp[j] = kNoCopy;
  CHECK(int64_t(src[15]) == G4 - 256);
  CHECK(!mul_md5_layout_ok(16, 4, 512, base, 64, src, base, 64, dst));
  CHECK(!mul_md5_layout_ok(16, 4, 256, base, 64, src, base, 64, dst));
  src[15] = static_cast<uint32_t>(G4 - 272);
  CHECK(mul_md5_layout_ok(16, 4, 256, base, 64, src, base, 64, dst));
  CHECK(!mul_md5_layout_ok(16, 4, 512, base, 64, src, base, 64, dst));
  // the same for an output and for a copy offset; kNoCopy entries do not count
  src[15] = 0;
  CHECK(mul_md5_layout_ok(16, 4, 512, base, 64, src, base, 64, dst, cp));
  dst[3] = static_cast<uint32_t>(G4 - 528);
  CHECK(mul_md5_layout_ok(16, 4, 512, base, 64, src, base, 64, dst, cp));
  dst[3] = static_cast<uint32_t>(G4 - 512);
  CHECK(!mul_md5_layout_ok(16, 4, 512, base, 64, src, base, 64, dst, cp));
  CHECK(mul_md5_layout_ok(16, 3, 512, base, 64, src, base, 64, dst, cp));  // row 3 not in use
  dst[3] = 0;
  cp[7] = static_cast<uint32_t>(G4 - 528);
  CHECK(mul_md5_layout_ok(16, 4, 512, base, 64, src, base, 64, dst, cp));
  cp[7] = static_cast<uint32_t>(G4 - 512);
  CHECK(!mul_md5_layout_ok(16, 4, 512, base, 64, src, base, 64, dst, cp));
  CHECK(mul_md5_layout_ok(16, 4, 512, base, 64, src, base, 64, dst));  // no copy table
  cp[7] = kNoCopy;
  // what it checked before still holds: shape, step, alignment
  CHECK(!mul_md5_layout_ok(21, 4, 512, base, 64, src, base, 64, dst) && !mul_md5_layout_ok(16, 5, 512, base, 64, src, base, 64, dst));
  CHECK(!mul_md5_layout_ok(16, 4, 0, base, 64, src, base, 64, dst) && !mul_md5_layout_ok(16, 4, 520, base, 64, src, base, 64, dst));
  CHECK(!mul_md5_layout_ok(16, 4, 512, base, 72, src, base, 64, dst) && !mul_md5_layout_ok(16, 4, 512, base, 64, src, base, -64, dst));
  src[3] = 8;
  CHECK(!mul_md5_layout_ok(16, 4, 512, base, 64, src, base, 64, dst));
  src[3] = 3 * 286331136u;
  CHECK(mul_md5_layout_ok(16, 4, 512, base, 64, src, base, 64, dst));
  CHECK(!mul_md5_layout_ok(16, 4, 512, static_cast<const char *>(base) + 4, 64, src, base, 64, dst));

  // mul_md5_group_cap(S, src_ss, dst_ss, top_end): (S' - 1) * ss + top_end <= 2^32 - 1
  CHECK(mul_md5_group_cap(16, 14 << 20, 14 << 20, 14 << 20) == 16);  // an everyday batch keeps its S
  CHECK(mul_md5_group_cap(1, G4 + (1 << 20), G4 + (1 << 20), G4 - 32) == 1);
  CHECK(mul_md5_group_cap(2, G4 + (1 << 20), G4 + (1 << 20), 16384) == 1);  // stripes further apart than 4 GiB
  CHECK(mul_md5_group_cap(16, 1024, G4, 16384) == 1 && mul_md5_group_cap(16, G4, 1024, 16384) == 1);
  for (const int64_t S : {2, 3, 5, 16}) {
    const int64_t top_end = 65536;
    const int64_t at = (G4 - 1 - top_end) / (S - 1);  // the largest stride that still holds S stripes
    CHECK(mul_md5_group_cap(S, at, at, top_end) == S);
    CHECK(mul_md5_group_cap(S, at + 1, 16, top_end) == S - 1);
    CHECK(mul_md5_group_cap(S, 16, at + 1, top_end) == S - 1);
    CHECK((S - 1) * at + top_end <= G4 - 1 && (S - 1) * (at + 1) + top_end > G4 - 1);
    // just below and just above 2^32 / (S - 1) with nothing else in the stripe but one 256-byte step
    const int64_t q = G4 / (S - 1);
    CHECK(mul_md5_group_cap(S, q - 272, q - 272, 256) == S);
    CHECK(mul_md5_group_cap(S, q + 16, q + 16, 256) == S - 1);
    // every capped S' obeys the bound and S' + 1 would not
    for (const int64_t ss : {q / 3, q / 2, q - 256, q, q + 16, 2 * q, G4 - 16, G4 + 16}) {
      const int64_t c = mul_md5_group_cap(S, ss, ss / 2, top_end);
      CHECK(c >= 1 && c <= S && (c - 1) * ss + top_end <= G4 - 1);
      CHECK(c == S || c * ss + top_end > G4 - 1);
    }
  }
  CHECK(mul_md5_group_cap(16, 4096, 4096, G4) == 1);  // a top_end that launch_mul_md5 refuses anyway
  CHECK(mul_md5_group_cap(0, 4096, 4096, 4096) == 1 && mul_md5_group_cap(4, 0, 0, 4096) == 4);

  if (fail) return 1;
  std::printf("md5_layout_test ok\n");
  return 0;
}
