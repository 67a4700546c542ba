// The per-byte rule of the parity scrub, shared by the host entry point
// (nxec_rs_syndrome_locate) and the locate / heal kernel: which single chunk
// explains the n-k syndrome bytes of one byte column of a stripe?
//
// H = [C | I] is the parity-check matrix (C: the n-k parity rows of
// gf_gen_rs_matrix, all non-zero).  An error e in data chunk j gives the
// syndrome e * column j of C (every byte non-zero); an error in parity chunk
// r gives e * unit vector r.  Any two columns of H are independent for
// n-k >= 2, so at most one chunk matches.
#ifndef NXEC_SCRUB_RULE_H
#define NXEC_SCRUB_RULE_H

#include <cstdint>

#if defined(__HIPCC__)
#define NXEC_HD __host__ __device__
#else
#define NXEC_HD
#endif

namespace nxec {
namespace scrub {

constexpr int32_t kClean = -1;      // NXEC_SCRUB_CLEAN
constexpr int32_t kUnlocated = -2;  // NXEC_SCRUB_UNLOCATED

// GF(2^8) product over 0x11d (ISA-L gf_mul, ec_base.c:48-61), shift and add
NXEC_HD inline uint32_t mul(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (int i = 0; i < 8; i++) {
    p ^= (b & 1u) ? a : 0u;
    a = (a << 1) ^ ((a & 0x80u) ? 0x11du : 0u);
    b >>= 1;
  }
  return p;
}

// a^254 = 1/a (a != 0)
NXEC_HD inline uint32_t inv(uint32_t a) {
  uint32_t r = 1, sq = a;
  for (int i = 1; i < 8; i++) {  // exponent bits 1..7
    sq = mul(sq, sq);
    r = mul(r, sq);
  }
  return r;
}

// syn(r), r < n-k: the syndrome bytes; coef: (n-k) x k parity rows, row-major
// with row stride k.  Returns kClean, kUnlocated or the chunk id, with *err
// the value to XOR into that chunk's byte.
template <class Syn>
NXEC_HD inline int32_t locate(int n, int k, const uint8_t *coef, const Syn &syn, uint8_t *err) {
  const int m = n - k;
  int nz = 0, first = -1;
  for (int r = 0; r < m; r++) {
    if (syn(r) != 0) {
      if (first < 0) first = r;
      nz++;
    }
  }
  *err = 0;
  if (nz == 0) return kClean;
  if (m < 2) return kUnlocated;
  if (nz == 1) {  // one parity chunk alone
    *err = static_cast<uint8_t>(syn(first));
    return k + first;
  }
  if (nz != m) return kUnlocated;  // a data error reaches every row
  const uint32_t s0 = syn(0), s1 = syn(1);
  for (int j = 0; j < k; j++) {
    const uint32_t c0 = coef[j], c1 = coef[k + j];
    if (mul(c0, s1) != mul(c1, s0)) continue;  // s0 / c0 == s1 / c1
    const uint32_t e = c0 == 1 ? s0 : mul(s0, inv(c0));
    bool all = true;
    for (int r = 0; r < m && all; r++) all = mul(coef[r * k + j], e) == static_cast<uint32_t>(syn(r));
    if (all) {
      *err = static_cast<uint8_t>(e);
      return j;
    }
  }
  return kUnlocated;
}

}  // namespace scrub
}  // namespace nxec

#endif
