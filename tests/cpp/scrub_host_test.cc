// Stand-alone host program for the parity scrub's per-byte rule
// (nxec_rs_syndrome_locate, nxec_scrub_rule.h): no device, no libnxec.  Built
// with -fsanitize=address,undefined (make build/scrub_host_test) from the two
// pure-host sources, so the sanitizers see the rule and the matrix generator.
//
// Cases (the same as tests/test_scrub_host.py, over a grid of geometries):
//  * one error e in chunk c gives (c, e) for every c < n, e in {1, 0x53, 0xff};
//  * the zero syndrome is CLEAN;
//  * n-k >= 3, n <= 20: two chunks in error at one offset are UNLOCATED;
//  * n-k == 1: every non-zero syndrome is UNLOCATED.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "nxec.h"

namespace nxec {
// the library's error sink lives with the device runtime; here a stub
int set_error(int code, const char *, ...) { return code; }
}  // namespace nxec

namespace {

int g_fail = 0;
#define EXPECT(cond, ...)                       \
  do {                                          \
    if (!(cond)) {                              \
      std::fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
      std::fprintf(stderr, __VA_ARGS__);        \
      std::fprintf(stderr, "\n");               \
      g_fail++;                                 \
    }                                           \
  } while (0)

// column c of H = [C | I] times e
std::vector<unsigned char> syndrome_of(const std::vector<unsigned char> &enc, int n, int k, int c, unsigned char e) {
  std::vector<unsigned char> s(n - k, 0);
  for (int r = 0; r < n - k; r++) {
    if (c < k) s[r] = nxec_gf_mul(enc[static_cast<size_t>(k + r) * k + c], e);
    else if (c - k == r) s[r] = e;
  }
  return s;
}

void check_geometry(int n, int k) {
  const int m = n - k;
  std::vector<unsigned char> enc(static_cast<size_t>(n) * k);
  nxec_gf_gen_rs_matrix(enc.data(), n, k);
  int32_t chunk = 12345;
  unsigned char err = 77;
  std::vector<unsigned char> zero(m, 0);
  EXPECT(nxec_rs_syndrome_locate(n, k, zero.data(), &chunk, &err) == NXEC_OK, "(%d,%d) zero: rc", n, k);
  EXPECT(chunk == NXEC_SCRUB_CLEAN && err == 0, "(%d,%d) zero syndrome: chunk %d err %d", n, k, chunk, err);
  const unsigned char errs[3] = {1, 0x53, 0xff};
  for (int c = 0; c < n; c++) {
    for (unsigned char e : errs) {
      const std::vector<unsigned char> s = syndrome_of(enc, n, k, c, e);
      EXPECT(nxec_rs_syndrome_locate(n, k, s.data(), &chunk, &err) == NXEC_OK, "(%d,%d) c=%d: rc", n, k, c);
      if (m >= 2) EXPECT(chunk == c && err == e, "(%d,%d) c=%d e=%d: got chunk %d err %d", n, k, c, e, chunk, err);
      else EXPECT(chunk == NXEC_SCRUB_UNLOCATED, "(%d,%d) n-k=1 c=%d: got chunk %d", n, k, c, chunk);
      // error may be NULL
      EXPECT(nxec_rs_syndrome_locate(n, k, s.data(), &chunk, nullptr) == NXEC_OK, "(%d,%d) null error: rc", n, k);
    }
  }
  if (m >= 3 && n <= 20) {
    const unsigned char pairs[2][2] = {{1, 1}, {0x53, 0xca}};
    for (int a = 0; a < n; a++)
      for (int b = a + 1; b < n; b++)
        for (const auto &p : pairs) {
          std::vector<unsigned char> s = syndrome_of(enc, n, k, a, p[0]);
          const std::vector<unsigned char> t = syndrome_of(enc, n, k, b, p[1]);
          for (int r = 0; r < m; r++) s[r] ^= t[r];
          EXPECT(nxec_rs_syndrome_locate(n, k, s.data(), &chunk, &err) == NXEC_OK, "(%d,%d) pair: rc", n, k);
          EXPECT(chunk == NXEC_SCRUB_UNLOCATED, "(%d,%d) chunks %d,%d errors %d,%d: got chunk %d", n, k, a, b, p[0],
                 p[1], chunk);
        }
  }
}

}  // namespace

int main() {
  const int geoms[][2] = {{4, 2},   {5, 4},   {6, 4},   {9, 6},   {12, 6},  {12, 8},   {14, 10},
                          {16, 12}, {20, 16}, {24, 21}, {26, 22}, {40, 32}, {128, 127}, {128, 100}};
  for (const auto &g : geoms) check_geometry(g[0], g[1]);
  // argument validation
  int32_t chunk = 0;
  unsigned char s[4] = {0, 0, 0, 0};
  EXPECT(nxec_rs_syndrome_locate(0, 0, s, &chunk, nullptr) == NXEC_ERR_INVALID, "n = 0 accepted");
  EXPECT(nxec_rs_syndrome_locate(4, 5, s, &chunk, nullptr) == NXEC_ERR_INVALID, "k > n accepted");
  EXPECT(nxec_rs_syndrome_locate(NXEC_MAX_N + 1, 4, s, &chunk, nullptr) == NXEC_ERR_INVALID, "n > max accepted");
  EXPECT(nxec_rs_syndrome_locate(6, 4, nullptr, &chunk, nullptr) == NXEC_ERR_INVALID, "null syndrome accepted");
  EXPECT(nxec_rs_syndrome_locate(6, 4, s, nullptr, nullptr) == NXEC_ERR_INVALID, "null chunk accepted");
  EXPECT(nxec_rs_syndrome_locate(4, 4, nullptr, &chunk, nullptr) == NXEC_OK && chunk == NXEC_SCRUB_CLEAN,
         "n == k: no syndrome, clean");
  if (g_fail) {
    std::fprintf(stderr, "scrub_host_test: %d failures\n", g_fail);
    return 1;
  }
  std::printf("scrub_host_test ok\n");
  return 0;
}
