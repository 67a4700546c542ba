// gfx950 (CDNA4) kernels of the Nexoedge RS coding path.
//
// One primitive: dst_r[i] = XOR_j c(r,j) (x) src_j[i] over GF(2^8)/0x11d, for
// r < rows <= 4 and every byte i of every stripe in a batch.  This is the work
// of ISA-L's ec_encode_data (ec_base.c:302-317; SIMD gf_4vect_dot_prod_*.asm)
// as called by rs.cc:89 (encode), rs.cc:230 (decode/repair), rs.cc:106 (CAR
// XOR) and coding_util.hh:21,28 (agent partial encode) -- re-designed for
// MI355X rather than translated:
//
//  * Table lookup in LDS.  For every source j the workgroup builds a
//    256-entry table whose 32-bit entry x packs the products c(r,j)*x of all
//    (<= 4) output rows.  One ds_read_b32 per source byte yields every row's
//    product at once, so each data byte is read from HBM once and looked up
//    once, whatever the number of rows (the reference's SIMD kernel and the
//    "one wavefront per row" alternative both re-touch the data per row).
//  * Bank-conflict-free-ish replication.  Random data bytes make LDS bank
//    conflicts data dependent; table copy c = lane % R sits in the bank bits
//    (address = ((j*256 + x)*R + c)*4), so with R = 16 a half-wave's 32 lanes
//    collide at most pairwise (4 LDS cycles per wave lookup instead of ~8 at
//    R = 1).  R = 16 for k <= 10 (k*16 KiB of LDS), R = 8 for k <= 20.
//  * HBM side: each lane owns one 16-byte column vector of the stripe; a wave
//    issues k global_load_dwordx4 (1 KiB contiguous per source, all k in
//    flight) and `rows` global_store_dwordx4 after an in-register 4x4 byte
//    transpose (v_perm_b32) of the packed accumulators.
//  * Persistent grid (one or two 1024-thread workgroups per CU) walks the
//    flattened (stripe, column-tile) space, so the tables are built once per
//    workgroup, not per tile.
//  * No MFMA: this is byte-wise lookup/XOR work bounded by HBM bandwidth.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>

#include "nxec_device.h"
#include "nxec_internal.h"
#include "nxec_runtime.h"
#include "nxec_scrub_rule.h"

namespace nxec {

namespace {

constexpr int kBlock = 1024;       // threads per workgroup (16 waves)
constexpr int kMaxTemplK = 20;     // k with a fully unrolled kernel; larger k use the dynamic kernel
constexpr int kLdsBytes = 160 * 1024;
// next-tile prefetch doubles the source registers (4*K VGPRs); beyond these k
// the 128-VGPR budget of a 1024-thread workgroup would spill
constexpr int kPrefetchMaxK = 10;
constexpr int kPrefetchMaxKCopy = 8;  // k = 10 with copies fits (123 VGPRs) but measured 6-8% slower (full-output decode)
constexpr int kPermPrefetchMaxK = 4;
constexpr int kPermMaxK = 13;  // beyond this the single-row VALU kernel would spill (128-VGPR budget)

constexpr int kRingBytes = 16;  // work-queue broadcast ring, after the tables in dynamic LDS
constexpr bool queue_fits(int table_bytes) { return table_bytes + kRingBytes <= kLdsBytes; }

// Compile-time shape of each instantiation: next-tile prefetch (PF) and work
// queue (Q).  The kernel templates and the launch record (launch_log_append)
// both read these, so the record cannot drift from the code that runs.
constexpr int default_r(int k) { return k <= 9 ? 16 : 8; }
constexpr bool vec_prefetch(int k, bool copy, bool full) {
  return k <= ((copy || !full) ? kPrefetchMaxKCopy : kPrefetchMaxK);
}
// Dynamic LDS of each kernel family, computed here and nowhere else: the
// kernels' static_asserts, the per-device preparation (list_kernels) and the
// launches all call these.  r copies of k 256-entry tables, then the queue
// ring where it fits (the scrub and ragged kernels exist only where it does).
constexpr int table_bytes(int k, int r) { return k * 1024 * r; }
constexpr bool vec_queued(int k, int r) { return queue_fits(table_bytes(k, r)); }
constexpr int vec_lds(int k, int r) { return table_bytes(k, r) + (vec_queued(k, r) ? kRingBytes : 0); }
constexpr int scrub_vec_lds(int kd) { return vec_lds(kd, default_r(kd)); }
constexpr int ragged_lds(int k) { return vec_lds(k, default_r(k)); }
constexpr int perm_lds(int k) { return k * 32 + kRingBytes; }
constexpr int bytes_lds(int k) { return table_bytes(k, 1); }  // k_mul_vec_dyn, k_mul_bytes, k_scrub_bytes, k_mul_list
constexpr bool perm_prefetch(int k) { return k <= kPermPrefetchMaxK; }
constexpr bool ragged_prefetch(int k) { return k <= kPrefetchMaxKCopy; }
// nsrc = data chunks + parity rows of the pass (the tile loader's sources)
constexpr bool scrub_prefetch(int nsrc, bool full) { return nsrc <= (full ? kPrefetchMaxK : kPrefetchMaxKCopy); }

using dev::build_tables;
using dev::gf_mul_dev;
using dev::ld_stream;
using dev::lookup16;
using dev::rows_of;
using dev::st_stream;
using dev::u32x4;

template <int R>
__device__ __forceinline__ void build_tables(const MulArgs &a, int k, uint32_t *tab) {
  build_tables<R>(a.coef, a.k, a.rows, tab);
}

// Chunk addresses of stripe s.  GATHER is a template parameter so the
// per-source address math stays branch-free (uniform, SGPR-resident).
template <bool GATHER>
__device__ __forceinline__ uint8_t *dst_row(const MulArgs &a, uint32_t s, int r) {
  if (GATHER) return a.dst_ptrs[static_cast<size_t>(s) * a.dst_ptr_rows + a.dst_ptr_row0 + r];
  return a.dst + static_cast<int64_t>(s) * a.dst_stripe_stride + a.dst_off[r];
}

template <bool GATHER>
__device__ __forceinline__ const uint8_t *src_chunk(const MulArgs &a, uint32_t s, int j) {
  if (GATHER) return a.src_ptrs[static_cast<size_t>(s) * a.k + j];
  return a.src + static_cast<int64_t>(s) * a.src_stripe_stride + a.src_off[j];
}

// acc[p] holds the 4 row products of column byte p (p = 4q + b); write row r's
// 16 bytes = byte r of acc[0..15].  8 v_perm_b32 per 4 columns.
// Row r (< rows) goes to row(r), the address of this lane's 16 bytes of it.
// `rows` is read at each use and the callers' lambdas capture by value: the
// generated code is then that of the loop written out in each kernel (a row
// count read ahead of the loop, or by-reference captures, move k_mul_vec's and
// k_mul_ragged's register counts).
template <class RowF>
__device__ __forceinline__ void store_rows(const uint32_t acc[16], const int &rows, RowF row) {
  uint32_t o[4][4];
  rows_of(acc, o);
#pragma unroll
  for (int r = 0; r < kMaxRowsPerPass; r++)
    if (r < rows) st_stream(row(r), u32x4{o[r][0], o[r][1], o[r][2], o[r][3]});
}
template <bool GATHER>
__device__ __forceinline__ void store_rows(const MulArgs &a, uint32_t s, uint32_t v, const uint32_t acc[16]) {
  store_rows(acc, a.rows, [&a, s, v](int r) { return dst_row<GATHER>(a, s, r) + static_cast<size_t>(v) * 16; });
}

// acc = the packed row products of this lane's column, XORed over the first N
// sources of d; tlane = this lane's copy of source 0's table.
template <int N, int R, int K>
__device__ __forceinline__ void lookup_sources(const char *tlane, const u32x4 (&d)[K], uint32_t (&acc)[16]) {
  static_assert(N <= K, "N of the K loaded sources");
#pragma unroll
  for (int i = 0; i < 16; i++) acc[i] = 0;
#pragma unroll
  for (int j = 0; j < N; j++) lookup16<R>(tlane + j * table_bytes(1, R), d[j], acc);
}

// Column vector v (relative to the launch's vec_begin) of stripe s for tile t;
// tiles are kBlock consecutive vectors of one stripe.
struct TilePos {
  uint32_t s, v;
};
__device__ __forceinline__ TilePos tile_pos(uint32_t t, uint32_t tps) {
  const uint32_t s = t / tps;
  return {s, (t - s * tps) * kBlock + threadIdx.x};
}
// With stripe groups of sg > 1, tiles run column-major inside each group of
// sg consecutive stripes (the last group may be smaller).
__device__ __forceinline__ TilePos tile_pos(uint32_t t, uint32_t tps, uint32_t sg, uint32_t nstripes) {
  if (sg <= 1) return tile_pos(t, tps);
  const uint32_t per = sg * tps;
  const uint32_t g = t / per, w = t - g * per;
  const uint32_t gs = nstripes - g * sg < sg ? nstripes - g * sg : sg;
  const uint32_t c = w / gs;
  return {g * sg + (w - c * gs), c * kBlock + threadIdx.x};
}

// FULL: every tile is complete (vec_count % kBlock == 0), so no lane predicate
// and no exec-mask regions around the loads; the ragged remainder of a chunk
// gets its own predicated launch.
template <int K, bool GATHER, bool FULL>
__device__ __forceinline__ void load_tile(const MulArgs &a, TilePos p, uint32_t nvec, u32x4 (&d)[K]) {
  if (FULL || p.v < nvec) {
    const size_t off = (static_cast<size_t>(a.vec_begin) + p.v) * 16;
#pragma unroll
    for (int j = 0; j < K; j++) d[j] = ld_stream(src_chunk<GATHER>(a, p.s, j) + off);
  }
}

template <int K, bool COPY>
__device__ __forceinline__ void copy_through(const MulArgs &a, uint32_t s, uint32_t vg, const u32x4 (&d)[K]) {
  if (COPY) {
#pragma unroll
    for (int j = 0; j < K; j++) {
      const uint32_t c = a.copy_off[j];
      if (c != kNoCopy)
        st_stream(a.dst + static_cast<int64_t>(s) * a.dst_stripe_stride + c + static_cast<size_t>(vg) * 16, d[j]);
    }
  }
}

// --- algorithm 1: LDS product tables (any rows <= 4) ---
template <int K, int R, bool GATHER, bool COPY>
struct LdsBody {
  static constexpr int kLds = table_bytes(K, R);
  static __device__ __forceinline__ void setup(const MulArgs &a, uint32_t *tab) { build_tables<R>(a, K, tab); }
  const char *tlane;
  __device__ explicit LdsBody(const uint32_t *tab)
      : tlane(reinterpret_cast<const char *>(tab) + (threadIdx.x % R) * 4) {}
  __device__ __forceinline__ void operator()(const MulArgs &a, uint32_t s, uint32_t vg, const u32x4 (&d)[K]) const {
    uint32_t acc[16];
    lookup_sources<K, R>(tlane, d, acc);
    store_rows<GATHER>(a, s, vg, acc);
    copy_through<K, COPY>(a, s, vg, d);
  }
};

// --- parity scrub, detect stage (nxec_rs_scrub_stripes): LdsBody without stores ---
// The pass's ROWS parity chunks are sources KD .. KD+ROWS-1 of the tile loader
// (so tile_loop's vmcnt accounting sees every load of the step); only the KD
// data sources are looked up.  The recomputed rows are XORed with the loaded
// parity vectors and ORed into one per-lane register; a wave that saw a
// non-zero syndrome clears bit 0 of its stripe's status (CLEAN -> UNLOCATED)
// with one atomic.  A clean tile stores nothing.
__device__ __forceinline__ void scrub_flag(int32_t *status, uint32_t s) {
  __hip_atomic_fetch_and(status + s, ~1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <int KD, int ROWS, int R>
struct ScrubBody {
  static constexpr int K = KD + ROWS;
  static constexpr int kLds = table_bytes(KD, R);
  static __device__ __forceinline__ void setup(const MulArgs &a, uint32_t *tab) {
    build_tables<R>(a.coef, KD, ROWS, tab);
  }
  const char *tlane;
  int32_t *status;
  __device__ ScrubBody(const uint32_t *tab, int32_t *st)
      : tlane(reinterpret_cast<const char *>(tab) + (threadIdx.x % R) * 4), status(st) {}
  __device__ __forceinline__ void operator()(const MulArgs &, uint32_t s, uint32_t, const u32x4 (&d)[K]) const {
    uint32_t acc[16];
    lookup_sources<KD, R>(tlane, d, acc);
    uint32_t o[4][4];
    rows_of(acc, o);
    uint32_t bad = 0;
#pragma unroll
    for (int r = 0; r < ROWS; r++)
      bad |= (o[r][0] ^ d[KD + r].x) | (o[r][1] ^ d[KD + r].y) | (o[r][2] ^ d[KD + r].z) | (o[r][3] ^ d[KD + r].w);
    const uint64_t hit = __ballot(bad != 0);
    if (hit != 0) {  // wave-uniform, taken only on corruption
      if (static_cast<int>(__lane_id()) == __ffsll(static_cast<unsigned long long>(hit)) - 1) scrub_flag(status, s);
    }
  }
};

// --- algorithm 2: VALU nibble tables via v_perm_b32 (rows == 1) ---
// c*x = c*(x & 15) ^ c*(x & 0xf0).  v_perm_b32 picks 4 bytes at once from an
// 8-byte pool; a 16-entry nibble table is two pools, chosen per byte by the
// nibble's bit 3.  That bit becomes a 0x00/0xFF byte mask through v_perm's
// sign-replication selectors (8..11 copy bit 7 of pool bytes 1,3,5,7), and
// v_bfi_b32 merges the two halves.  No LDS traffic per byte (only 2 uniform
// ds_read_b128 per source per tile for the 32-byte table), so a single-row
// pass (repair, agent partial encode, CAR XOR) is not bound by LDS banks.
// Measured k=12 rows=1: 0.678 of 8 TB/s vs 0.608 for the LDS tables
// (tools/microbench/shape_ceiling.hip).
__device__ __forceinline__ uint32_t perm_mul(const uint32_t *t, uint32_t nl, uint32_t nh, uint32_t ml, uint32_t mh) {
  const uint32_t l0 = __builtin_amdgcn_perm(t[1], t[0], nl), l1 = __builtin_amdgcn_perm(t[3], t[2], nl);
  const uint32_t h0 = __builtin_amdgcn_perm(t[5], t[4], nh), h1 = __builtin_amdgcn_perm(t[7], t[6], nh);
  return ((ml & l1) | (~ml & l0)) ^ ((mh & h1) | (~mh & h0));
}

template <int K, bool GATHER, bool COPY>
struct PermBody {
  static constexpr int kLds = K * 32;
  // table of source j: bytes [32j .. 32j+15] = c*n, [32j+16 .. 32j+31] = c*(n<<4)
  static __device__ __forceinline__ void setup(const MulArgs &a, uint32_t *tab) {
    uint8_t *tb = reinterpret_cast<uint8_t *>(tab);
    for (int i = threadIdx.x; i < K * 16; i += blockDim.x) {
      const int j = i >> 4, n = i & 15;
      const uint32_t c = a.coef[j];
      tb[32 * j + n] = static_cast<uint8_t>(gf_mul_dev(c, n));
      tb[32 * j + 16 + n] = static_cast<uint8_t>(gf_mul_dev(c, n << 4));
    }
  }
  const uint32_t *tab;
  __device__ explicit PermBody(const uint32_t *t) : tab(t) {}
  __device__ __forceinline__ void operator()(const MulArgs &a, uint32_t s, uint32_t vg, const u32x4 (&d)[K]) const {
    // opaque zero: keeps the (uniform) table reads next to their use instead of
    // hoisting K*8 registers out of the tile loop
    uint32_t z;
    asm volatile("s_mov_b32 %0, 0" : "=s"(z));
    const uint32_t *tt = tab + z;
    uint32_t o[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < K; j++) {
      const uint32_t w[4] = {d[j].x, d[j].y, d[j].z, d[j].w};
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const uint32_t x = w[q], x4 = x << 4;
        const uint32_t nl = x & 0x07070707u, nh = (x >> 4) & 0x07070707u;
        const uint32_t ml = __builtin_amdgcn_perm(x4, x4 << 8, 0x0B090A08u);
        const uint32_t mh = __builtin_amdgcn_perm(x, x << 8, 0x0B090A08u);
        o[q] ^= perm_mul(tt + 8 * j, nl, nh, ml, mh);
      }
    }
    st_stream(dst_row<GATHER>(a, s, 0) + static_cast<size_t>(vg) * 16, u32x4{o[0], o[1], o[2], o[3]});
    copy_through<K, COPY>(a, s, vg, d);
  }
};

// Per-launch tile queues (one 128-byte slot per launch: [0] next tile, [1]
// workgroups finished).  The last workgroup to finish resets its slot, so a
// slot is clean for the next launch that draws it (host ring, kQueueSlots).
__device__ uint32_t g_tile_queue[kQueueSlots * 32];

// Work-queue grab: global_atomic_add with return, issued through inline asm
// so the compiler's wait-count bookkeeping never sees it.  Issued before a
// step's K loads, it is older than every op the compiler waits for, so the
// compiler's own waits stay correct (they can only wait longer), and the
// caller publishes g after an explicit vmcnt(K) -- instead of the vmcnt(0)
// (drain of every store) the compiler emits around a divergent atomic.
__device__ __forceinline__ uint32_t grab_async(uint32_t *q) {
  uint32_t g;
  asm volatile("global_atomic_add %0, %1, %2, off sc0" : "=&v"(g) : "v"(q), "v"(1u) : "memory");
  return g;
}
// ring[OFF/4] = g once at most N vector-memory ops are outstanding
template <int N, int OFF>
__device__ __forceinline__ void publish(uint32_t ring_base, uint32_t g) {
  static_assert(N >= 0 && N < 64, "vmcnt is 6 bits");
  asm volatile("s_waitcnt vmcnt(%2)\n\tds_write_b32 %0, %1 offset:%3" ::"v"(ring_base), "v"(g), "n"(N), "n"(OFF)
               : "memory");
}

// Persistent tile loop.
//
// Q (work queue, the default where 16 bytes of LDS are free): workgroups pull
// runs of T consecutive 16 KiB column tiles from a per-launch atomic counter
// (T = 1 for wide stripes; more for narrow ones so the counter is not
// hammered, tiles_per_grab()), the next run grabbed one run ahead and
// broadcast through a 4-entry LDS ring (one barrier per run).  In-flight tiles therefore always form one compact,
// ascending address window, and a workgroup slowed by a busy HBM channel
// simply takes fewer tiles: +12 % over static tile runs for the same bytes
// (tools/microbench/mem_pattern.hip, profiles/r01_mem_pattern.log).
//
// !Q (tables fill the whole 160 KiB), or queue_slot < 0 (NXEC_TILE_ORDER=static,
// for A/B only): workgroup b owns the contiguous tile run [b*ntiles/G, (b+1)*ntiles/G).
//
// PF: the next tile's loads go out before this tile's compute through two
// ping-pong register buffers (manual 2x unroll pinned by sched_barrier: no
// register copies, so the waitcnt pass keeps the prefetch in flight); a final
// prefetch past the end re-reads the current tile instead of branching, so
// every path has the same loads in flight.
//
// The geometry is the caller's: load(t, d) fetches tile t's K source vectors
// of this lane into d, run(t, d) computes and stores tile t.  ntiles tiles;
// slot >= 0 selects the queue (Q kernels), T = tiles per grab.
template <int K, bool PF, bool Q, bool QWAIT_K, class LoadF, class RunF>
__device__ __forceinline__ void tile_loop(const LoadF &load, const RunF &run, uint32_t ntiles, int32_t slot_arg,
                                          uint32_t T, uint32_t *ring) {
  if (Q && slot_arg >= 0) {
    uint32_t *q = g_tile_queue + static_cast<size_t>(slot_arg) * 32;
    if (threadIdx.x == 0) {
      ring[2] = atomicAdd(q, 1u);
      ring[3] = atomicAdd(q, 1u);
    }
    __syncthreads();
    // t: current tile; [t, rend) the rest of its run; nrun: first tile of the
    // run already grabbed for after it (all wave-uniform, SGPRs)
    auto run_start = [&](uint32_t r) -> uint32_t { return r * T; };
    uint32_t t = run_start(__builtin_amdgcn_readfirstlane(ring[2]));
    uint32_t nrun = run_start(__builtin_amdgcn_readfirstlane(ring[3]));
    uint32_t rend = t + T < ntiles ? t + T : ntiles;
    int slot = 0;
    // LDS byte address of ring[0], materialized once (a VGPR that no store
    // ever uses, so publishing never waits on the stores in flight)
    uint32_t ring_base = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(ring));
    asm volatile("" : "+v"(ring_base));
    // barrier that orders only the LDS ring (global loads stay in flight)
    auto ring_barrier = [] {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
    };
    // one tile: at the last tile of a run, grab the run after next (thread 0,
    // early, so the atomic's latency hides behind this tile's work) and
    // broadcast it at the end; nxt (PF) receives the next tile's sources
    // (the grab is issued before this step's loads: the ring write then only
    // waits for the atomic, not for the loads and stores behind it)
    auto step = [&](u32x4(&cur)[K], u32x4(&nxt)[K], bool pf) {
      const bool edge = t + 1 >= rend;
      const uint32_t tn = edge ? nrun : t + 1;
      uint32_t g = 0;
      if (edge && threadIdx.x == 0) g = grab_async(q);
      if (pf) {
        load(tn < ntiles ? tn : t, nxt);
        __builtin_amdgcn_sched_barrier(0);
      } else {
        load(t, cur);
        __builtin_amdgcn_sched_barrier(0);  // all K loads in flight before the lookups
      }
      run(t, cur);
      if (edge) {
        if (threadIdx.x == 0) {
          // >= K vector-memory ops (this step's loads) were issued after the
          // grab, so at most K outstanding means the grab has returned
          if (slot == 0) publish<QWAIT_K ? K : 0, 0>(ring_base, g);
          else publish<QWAIT_K ? K : 0, 4>(ring_base, g);
        }
        ring_barrier();
        const uint32_t nn = run_start(__builtin_amdgcn_readfirstlane(ring[slot]));
        slot ^= 1;
        rend = nrun + T < ntiles ? nrun + T : ntiles;
        nrun = nn;
      }
      t = tn;
      return t < ntiles;
    };
    if (t < ntiles) {
      if constexpr (PF) {
        u32x4 A[K], B[K];
        load(t, A);
        while (step(A, B, true) && step(B, A, true)) {
        }
      } else {
        bool more = true;
        while (more) {
          u32x4 d[K];
          more = step(d, d, false);
        }
      }
    }
    // every grab of this workgroup has returned (its values were consumed);
    // the last workgroup out resets the slot for the next launch
    if (threadIdx.x == 0) {
      __threadfence();
      if (atomicAdd(q + 1, 1u) == gridDim.x - 1) {
        atomicExch(q, 0u);
        atomicExch(q + 1, 0u);
      }
    }
    return;
  }
  // readfirstlane: the tile index is wave-uniform; keep its math on the SALU
  uint32_t t = __builtin_amdgcn_readfirstlane(
      static_cast<uint32_t>((static_cast<uint64_t>(blockIdx.x) * ntiles) / gridDim.x));
  const uint32_t tend = __builtin_amdgcn_readfirstlane(
      static_cast<uint32_t>((static_cast<uint64_t>(blockIdx.x + 1) * ntiles) / gridDim.x));
  if (t >= tend) return;
  if constexpr (PF) {
    u32x4 A[K], B[K];
    load(t, A);
    while (true) {
      const uint32_t tb = t + 1;
      load(tb < tend ? tb : t, B);
      __builtin_amdgcn_sched_barrier(0);
      run(t, A);
      if (tb >= tend) break;
      t = tb;
      const uint32_t ta = t + 1;
      load(ta < tend ? ta : t, A);
      __builtin_amdgcn_sched_barrier(0);
      run(t, B);
      if (ta >= tend) break;
      t = ta;
    }
  } else {
    for (; t < tend; t++) {
      u32x4 d[K];
      load(t, d);
      run(t, d);
    }
  }
}

// Fully unrolled vector kernels: all K source loads of a column vector in
// flight.  COPY: fused pass-through of sources (full-output decode); a
// separate instantiation so encode/recover kernels carry no copy registers.
// The queue ring lives in the dynamic LDS block after the tables (Q only
// where it fits: queue_fits()).
// Strided / gather geometry of a MulArgs launch: tile t = column tile
// t % tps of stripe t / tps.
template <int K, bool GATHER, bool FULL, bool PF, bool Q, class Body>
__device__ __forceinline__ void mul_tiles(const MulArgs &a, const Body &body, uint32_t *ring) {
  const uint32_t nvec = static_cast<uint32_t>(a.vec_count);
  const uint32_t tps = (nvec + kBlock - 1) / kBlock;
  const uint32_t ntiles = tps * static_cast<uint32_t>(a.nstripes);
  const uint32_t sg = a.stripe_group, ns = static_cast<uint32_t>(a.nstripes);
  auto load = [&](uint32_t t, u32x4(&d)[K]) { load_tile<K, GATHER, FULL>(a, tile_pos(t, tps, sg, ns), nvec, d); };
  auto run = [&](uint32_t t, const u32x4(&d)[K]) {
    const TilePos p = tile_pos(t, tps, sg, ns);
    if (FULL || p.v < nvec) body(a, p.s, static_cast<uint32_t>(a.vec_begin) + p.v, d);
  };
  tile_loop<K, PF, Q, FULL>(load, run, ntiles, a.queue_slot, a.tiles_per_grab, ring);
}

template <int K, int R, bool GATHER, bool COPY, bool FULL>
__global__ __launch_bounds__(kBlock) void k_mul_vec(const MulArgs a) {
  constexpr bool PF = vec_prefetch(K, COPY, FULL);
  constexpr bool Q = vec_queued(K, R);
  using Body = LdsBody<K, R, GATHER, COPY>;
  static_assert(Body::kLds + (Q ? kRingBytes : 0) == vec_lds(K, R), "tables, then the ring: what the launch asks for");
  extern __shared__ uint32_t tab[];
  Body::setup(a, tab);
  __syncthreads();
  mul_tiles<K, GATHER, FULL, PF, Q>(a, Body(tab), tab + Body::kLds / 4);
}

template <int K, bool GATHER, bool COPY, bool FULL>
__global__ __launch_bounds__(kBlock) void k_mul_perm(const MulArgs a) {
  constexpr bool PF = perm_prefetch(K);
  using Body = PermBody<K, GATHER, COPY>;
  static_assert(Body::kLds + kRingBytes == perm_lds(K), "tables, then the ring: what the launch asks for");
  extern __shared__ uint32_t tab[];
  Body::setup(a, tab);
  __syncthreads();
  mul_tiles<K, GATHER, FULL, PF, true>(a, Body(tab), tab + Body::kLds / 4);
}

// --- ragged stripes (the last stripes of many objects) ---
// Stripes of different chunk lengths in one launch, through the same
// work-queue tile loop and LDS tables as k_mul_vec: tile t belongs to stripe
// tile_stripe[t] (a device map built per call), column tile
// t - stripe_tile0[s].  Every stripe is 16-byte aligned with 16-byte chunk
// strides and len rounded up to 16 (the zero-padded tail arena of
// nxec_encode_objects), so every lane moves whole 16-byte vectors.
struct RaggedArgs {
  const ListStripe *__restrict__ stripes;
  const uint32_t *__restrict__ tile_stripe;
  const uint32_t *__restrict__ stripe_tile0;
  uint32_t ntiles;
  int32_t k, rows, row0, queue_slot;
  uint32_t tiles_per_grab;
  uint8_t coef[kMaxRowsPerPass * (NXEC_MAX_K + 1)];
};

template <int K, int R>
__global__ __launch_bounds__(kBlock) void k_mul_ragged(const RaggedArgs a) {
  constexpr bool PF = ragged_prefetch(K);
  constexpr int kLds = table_bytes(K, R);
  static_assert(R == default_r(K) && kLds + kRingBytes == ragged_lds(K), "ragged kernels are queue-driven");
  extern __shared__ uint32_t tab[];
  build_tables<R>(a.coef, K, a.rows, tab);
  __syncthreads();
  const char *tl = reinterpret_cast<const char *>(tab) + (threadIdx.x % R) * 4;
  auto where = [&](uint32_t t, ListStripe &st, uint32_t &v) {
    const uint32_t s = a.tile_stripe[t];
    st = a.stripes[s];
    v = (t - a.stripe_tile0[s]) * kBlock + threadIdx.x;
  };
  auto load = [&](uint32_t t, u32x4(&d)[K]) {
    ListStripe st;
    uint32_t v;
    where(t, st, v);
    if (v * int64_t(16) < st.len) {
#pragma unroll
      for (int j = 0; j < K; j++) d[j] = ld_stream(st.src + j * st.src_cs + static_cast<size_t>(v) * 16);
    }
  };
  auto run = [&](uint32_t t, const u32x4(&d)[K]) {
    ListStripe st;
    uint32_t v;
    where(t, st, v);
    if (v * int64_t(16) < st.len) {
      uint32_t acc[16];
      lookup_sources<K, R>(tl, d, acc);
      uint8_t *row0 = st.dst + a.row0 * st.dst_cs;
      const int rows = a.rows;
      store_rows(acc, rows, [=](int r) { return row0 + r * st.dst_cs + static_cast<size_t>(v) * 16; });
    }
  };
  // wave 0 (lane 0 = the tile's first vector) always issues its K loads
  tile_loop<K, PF, true, true>(load, run, a.ntiles, a.queue_slot, a.tiles_per_grab, tab + kLds / 4);
}

// --- mixed-pattern recover and decode (nxec_rs_recover_stripes_mixed, nxec_rs_decode_stripes_mixed) ---
// Every stripe names its own erased chunks.  Item i = stripe order[i] under
// segment seg_of[i] (one plan's <= 4 rows over its k sources); tile t = column
// tile t % tps of item t / tps.  Items run by segment, so a workgroup's tables
// stay valid for long stretches; where the segment of the tile it is about to
// run differs from the resident one it rebuilds them from the segment record.
// The tile index is workgroup-uniform (tile_loop), so the rebuild and its two
// barriers are too.  Item, stripe and segment stay in SGPRs (scalar loads of
// uniform addresses); only the vector index is per lane, and every address is
// a uniform 64-bit base plus one 32-bit lane offset.
//
// FULL = false (k_mul_mixed, the recover) works in place: sources and rebuilt
// chunks share one base and one stride (dst, dst_stripe_stride; the launch sets
// src and its stride equal to them and the kernel does not read them).
//
// FULL = true (k_decode_mixed, the decode) adds a full output: the sources come
// from a const batch (src, src_stripe_stride), all k data chunks of every
// item's stripe go to a separate output (dst, dst_stripe_stride).  A segment
// carries <= 4 inverse rows for the lost data chunks and, in the first segment
// of a plan, the output offsets of the sources that are surviving data chunks,
// which are stored from the registers that loaded them.  rows == 0 segments (no
// lost data chunk: the bulk of a healthy read) are pure copies: they skip the
// lookups and the row stores under a workgroup-uniform branch, build nothing
// and leave `resident` unchanged, so the tables of the last rows > 0 segment
// stay valid for its next tile, and a rows > 0 segment other than that one
// always rebuilds.  The output never intersects the source (refused by the
// host): tile_loop issues tile t+1's loads before tile t's stores.
struct MixedArgs {
  const uint8_t *src;
  uint8_t *dst;
  int64_t src_stripe_stride, dst_stripe_stride;
  const MixedSeg *__restrict__ segs;
  const uint32_t *__restrict__ order;
  const uint32_t *__restrict__ seg_of;
  uint32_t ntiles, tps, nvec;
  int32_t queue_slot;
  uint32_t tiles_per_grab;
};

constexpr int mixed_lds(int k) { return vec_lds(k, default_r(k)); }

// The launch's tables are written by the host before it starts and by no
// kernel: read through the constant address space, a load at a uniform index
// is a scalar load and its result stays in SGPRs (a global load would not be,
// next to the kernel's own stores).
template <class T>
__device__ __forceinline__ const __attribute__((address_space(4))) T *const_table(const T *p) {
  return (const __attribute__((address_space(4))) T *)(reinterpret_cast<uintptr_t>(p));
}

template <int K, int R, bool FULL>
__device__ __forceinline__ void mixed_body(const MixedArgs &a) {
  constexpr bool PF = ragged_prefetch(K);
  constexpr int kLds = table_bytes(K, R);
  static_assert(K <= kMaxRaggedK && R == default_r(K) && kLds + kRingBytes == mixed_lds(K),
                "mixed kernels are queue-driven");
  extern __shared__ uint32_t tab[];
  const char *tl = reinterpret_cast<const char *>(tab) + (threadIdx.x % R) * 4;
  uint32_t resident = ~0u;  // the (FULL: rows > 0) segment whose tables are in LDS (none yet)
  struct Where {
    uint32_t s, g, v;
  };
  auto where = [&](uint32_t t) -> Where {
    const uint32_t i = t / a.tps;
    // readfirstlane: where the compiler merges these with a copy made under a lane predicate they come back
    // as vector values; stripe and segment (and every address made from them) belong in SGPRs
    return {static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(const_table(a.order)[i])),
            static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(const_table(a.seg_of)[i])),
            (t - i * a.tps) * kBlock + threadIdx.x};
  };
  // a prefetched tile may belong to another segment than the resident one:
  // its source offsets come from its own record
  auto load = [&](uint32_t t, u32x4(&d)[K]) {
    const Where w = where(t);
    if (w.v < a.nvec) {
      const auto *sg = const_table(a.segs) + w.g;
      const uint8_t *sb;
      if constexpr (FULL) sb = a.src + static_cast<int64_t>(w.s) * a.src_stripe_stride;
      else sb = a.dst + static_cast<int64_t>(w.s) * a.dst_stripe_stride;
      // uniform 64-bit base + one 32-bit lane offset (chunks of a stripe lie within 4 GiB)
      const uint32_t vo = w.v * 16u;
#pragma unroll
      for (int j = 0; j < K; j++) d[j] = ld_stream(sb + sg->src_off[j] + vo);
    }
  };
  auto run = [&](uint32_t t, const u32x4(&d)[K]) {
    const Where w = where(t);
    // the tile's own record: row count, row offsets and copy offsets (never the resident segment's)
    const auto *sg = const_table(a.segs) + w.g;
    const int rows = static_cast<int>(sg->rows);
    const bool coded = !FULL || rows > 0;  // workgroup-uniform
    if (coded && w.g != resident) {        // workgroup-uniform
      // no wave may still be looking up the previous tile; LDS-only fences, so
      // the loads and stores in flight are not drained (tile_loop's ring_barrier)
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
      __builtin_amdgcn_s_barrier();
      build_tables<R>(a.segs[w.g].coef, K, rows, tab);  // rows >= the record's: zero products
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
      resident = w.g;
    }
    if (w.v < a.nvec) {
      uint8_t *db = a.dst + static_cast<int64_t>(w.s) * a.dst_stripe_stride;
      const uint32_t vo = w.v * 16u;
      if (coded) {
        uint32_t acc[16];
        lookup_sources<K, R>(tl, d, acc);
        const uint32_t o0 = sg->dst_off[0], o1 = sg->dst_off[1], o2 = sg->dst_off[2], o3 = sg->dst_off[3];
        store_rows(acc, rows, [=](int r) { return db + (r == 0 ? o0 : r == 1 ? o1 : r == 2 ? o2 : o3) + vo; });
      }
      if constexpr (FULL) {
#pragma unroll
        for (int j = 0; j < K; j++) {
          const uint32_t c = sg->copy_off[j];  // scalar; kNoCopy in every later segment of a plan
          if (c != kNoCopy) st_stream(db + c + vo, d[j]);
        }
      }
    }
  };
  // QWAIT_K: every tile has at least one vector, so wave 0 (lane 0 = the tile's first vector) always issues its
  // K loads after the grab; the row stores and the copies only add vector-memory operations after them
  tile_loop<K, PF, true, true>(load, run, a.ntiles, a.queue_slot, a.tiles_per_grab, tab + kLds / 4);
}

// The two entry points of the one body.  They keep the names of the two
// kernels they replace, and the decode's keeps an argument type of its own:
// the length of the kernels' symbol names decides where `.text` begins in the
// code object, and with every kernel of this file 0x300 bytes lower (one entry
// point `k_mixed<K, R, FULL>`, shorter names) every leg of
// tools/decode_mixed_rate.py, the untouched k_mul_vec copy form among them, ran
// 1.3-2.9 % slower ("One planner, one record, one kernel").
struct DecodeMixedArgs : MixedArgs {};

template <int K, int R>
__global__ __launch_bounds__(kBlock) void k_mul_mixed(const MixedArgs a) {
  mixed_body<K, R, false>(a);
}
template <int K, int R>
__global__ __launch_bounds__(kBlock) void k_decode_mixed(const DecodeMixedArgs a) {
  mixed_body<K, R, true>(a);
}

// --- delta update (nxec_rs_update_stripes) ---
// Byte ranges of data chunks are overwritten and the parity follows:
// p_r ^= c(r,j) (x) (new ^ old).  One pass covers <= 4 parity rows of one
// round (updates whose stripes and column ranges are pairwise disjoint, the
// host planner's invariant).  Every pass recomputes the delta from the old
// data, so only the last pass of a round stores the new data.
struct UpdateArgs {
  uint8_t *base;
  const UpdateItem *__restrict__ items;
  const uint32_t *__restrict__ tile_item;  // vector kernel: tile -> item
  const int64_t *__restrict__ byte_prefix;  // byte kernel: first byte index of each item, then the total
  int64_t nitems, nbytes;                   // byte kernel
  uint32_t ntiles;
  int32_t k, rows, last, queue_slot;
  uint32_t tiles_per_grab;
  uint32_t chunk_stride;
  uint32_t par_off[kMaxRowsPerPass];  // byte offset of the pass's parity chunks inside a stripe
  uint8_t coef[kMaxRowsPerPass * (NXEC_MAX_K + 1)];  // row-major rows x k
};

constexpr int update_lds(int k) { return vec_lds(k, default_r(k)); }
constexpr int kUpdateSrc = 2 + kMaxRowsPerPass;  // a lane's vectors per tile: old data, new data, the parity rows
static_assert(kUpdateTileVecs == kBlock, "the planner's tiles are one vector per thread");

// The encode tables of the pass's rows for all k columns (k_mul_vec's layout);
// the column an update multiplies by is a per-tile scalar, so k is not a
// template parameter: one instantiation per R, launched with update_lds(k).
// Item, stripe and column stay in SGPRs (const_table at a workgroup-uniform
// index); only the vector index is per lane.
//
// In place under prefetch: tile_loop issues tile t+1's loads before tile t's
// stores and re-reads the current tile once past the end.  The tiles of one
// launch are pairwise disjoint in every byte they read or write (one round),
// so no load can see a store of the same launch.
template <int R>
__global__ __launch_bounds__(kBlock) void k_update_vec(const UpdateArgs a) {
  constexpr int K = kUpdateSrc;
  extern __shared__ uint32_t tab[];
  build_tables<R>(a.coef, a.k, a.rows, tab);
  __syncthreads();
  const char *tl = reinterpret_cast<const char *>(tab) + (threadIdx.x % R) * 4;
  struct Where {
    const uint8_t *nw;  // the item's new bytes
    uint8_t *sb;        // its stripe
    uint32_t col, chunk, count, v;
  };
  auto where = [&](uint32_t t) -> Where {
    const uint32_t i = __builtin_amdgcn_readfirstlane(const_table(a.tile_item)[t]);
    const auto *it = const_table(a.items) + i;
    return {it->d_new,
            a.base + it->stripe_off,
            static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(it->col)),
            static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(it->chunk)),
            static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(it->count)),
            (t - static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(it->first))) * kBlock + threadIdx.x};
  };
  // d[0] = old data, d[1] = new data, d[2 + r] = parity row r of the pass
  auto load = [&](uint32_t t, u32x4(&d)[K]) {
    const Where w = where(t);
    if (w.v < w.count) {
      // uniform 64-bit base + one 32-bit lane offset (chunks of a stripe lie within 4 GiB)
      const uint32_t vo = w.col + w.v * 16u;
      d[0] = ld_stream(w.sb + w.chunk * a.chunk_stride + vo);
      d[1] = ld_stream(w.nw + w.v * 16u);
#pragma unroll
      for (int r = 0; r < kMaxRowsPerPass; r++)
        if (r < a.rows) d[2 + r] = ld_stream(w.sb + a.par_off[r] + vo);
    }
  };
  auto run = [&](uint32_t t, const u32x4(&d)[K]) {
    const Where w = where(t);
    if (w.v < w.count) {
      uint32_t acc[16];
#pragma unroll
      for (int i = 0; i < 16; i++) acc[i] = 0;
      lookup16<R>(tl + w.chunk * table_bytes(1, R), d[0] ^ d[1], acc);
      uint32_t o[4][4];
      rows_of(acc, o);
      const uint32_t vo = w.col + w.v * 16u;
#pragma unroll
      for (int r = 0; r < kMaxRowsPerPass; r++)
        if (r < a.rows)
          st_stream(w.sb + a.par_off[r] + vo, d[2 + r] ^ u32x4{o[r][0], o[r][1], o[r][2], o[r][3]});
      if (a.last) st_stream(w.sb + w.chunk * a.chunk_stride + vo, d[1]);
    }
  };
  // QWAIT_K = false: a pass of fewer than 4 rows issues fewer than K loads per
  // tile, so "at most K outstanding" would not prove that the grab returned;
  // the publishing thread waits for all of its vector-memory operations instead
  tile_loop<K, true, true, false>(load, run, a.ntiles, a.queue_slot, a.tiles_per_grab,
                                  tab + table_bytes(a.k, R) / 4);
}

// Byte items: one thread per byte, R = 1 tables, any k and alignment.  The
// items of one round touch pairwise disjoint bytes, so a byte store never
// meets a neighbour's.
__global__ __launch_bounds__(256) void k_update_bytes(const UpdateArgs a) {
  extern __shared__ uint32_t tab[];
  const int k = a.k;
  build_tables<1>(a.coef, k, a.rows, tab);
  __syncthreads();
  for (int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; i < a.nbytes;
       i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    int64_t lo = 0, hi = a.nitems - 1;  // last item with byte_prefix <= i
    while (lo < hi) {
      const int64_t mid = (lo + hi + 1) >> 1;
      if (a.byte_prefix[mid] <= i) lo = mid;
      else hi = mid - 1;
    }
    const UpdateItem it = a.items[lo];
    const int64_t b = i - a.byte_prefix[lo];
    uint8_t *stripe = a.base + it.stripe_off;
    const int64_t c = static_cast<int64_t>(it.col) + b;
    uint8_t *data = stripe + static_cast<int64_t>(it.chunk) * a.chunk_stride + c;
    const uint8_t nw = it.d_new[b];
    const uint32_t e = tab[it.chunk * 256 + (*data ^ nw)];
    for (int r = 0; r < a.rows; r++) stripe[a.par_off[r] + c] ^= static_cast<uint8_t>(e >> (8 * r));
    if (a.last) *data = nw;
  }
}

// Runtime-k vector kernel (k > kMaxTemplK), R = 1 tables, sources in groups of 4.
template <bool GATHER>
__global__ __launch_bounds__(kBlock) void k_mul_vec_dyn(const MulArgs a) {
  extern __shared__ uint32_t tab[];
  const int k = a.k;
  build_tables<1>(a, k, tab);
  __syncthreads();
  const uint32_t nvec = static_cast<uint32_t>(a.vec_count);
  const uint32_t tps = (nvec + kBlock - 1) / kBlock;
  const uint32_t ntiles = tps * static_cast<uint32_t>(a.nstripes);
  const char *tl = reinterpret_cast<const char *>(tab);
  const uint32_t t0 = static_cast<uint32_t>((static_cast<uint64_t>(blockIdx.x) * ntiles) / gridDim.x);
  const uint32_t t1 = static_cast<uint32_t>((static_cast<uint64_t>(blockIdx.x + 1) * ntiles) / gridDim.x);
  for (uint32_t t = t0; t < t1; t++) {
    const uint32_t s = t / tps;
    const uint32_t vl = (t - s * tps) * kBlock + threadIdx.x;
    if (vl >= nvec) continue;
    const uint32_t v = static_cast<uint32_t>(a.vec_begin) + vl;
    uint32_t acc[16];
#pragma unroll
    for (int i = 0; i < 16; i++) acc[i] = 0;
    for (int j0 = 0; j0 < k; j0 += 4) {
      u32x4 d[4];
#pragma unroll
      for (int jj = 0; jj < 4; jj++)
        if (j0 + jj < k) d[jj] = ld_stream(src_chunk<GATHER>(a, s, j0 + jj) + static_cast<size_t>(v) * 16);
#pragma unroll
      for (int jj = 0; jj < 4; jj++) {
        if (j0 + jj < k) {
          lookup16<1>(tl + (j0 + jj) * 1024, d[jj], acc);
          const uint32_t c = a.copy_off[j0 + jj];
          if (!GATHER && a.any_copy && c != kNoCopy)
            st_stream(a.dst + static_cast<int64_t>(s) * a.dst_stripe_stride + c + static_cast<size_t>(v) * 16, d[jj]);
        }
      }
    }
    store_rows<GATHER>(a, s, v, acc);
  }
}

// Byte-granular kernel: chunk tails past vec_count*16 and misaligned layouts.
template <bool GATHER>
__global__ __launch_bounds__(256) void k_mul_bytes(const MulArgs a) {
  extern __shared__ uint32_t tab[];
  const int k = a.k;
  build_tables<1>(a, k, tab);
  __syncthreads();
  const int64_t span = a.len - a.byte_begin;
  const int64_t total = span * a.nstripes;
  for (int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; i < total;
       i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const uint32_t s = static_cast<uint32_t>(i / span);
    const int64_t pos = a.byte_begin + (i - static_cast<int64_t>(s) * span);
    uint32_t acc = 0;
    for (int j = 0; j < k; j++) {
      const uint8_t x = src_chunk<GATHER>(a, s, j)[pos];
      acc ^= tab[j * 256 + x];
      const uint32_t c = a.copy_off[j];
      if (!GATHER && a.any_copy && c != kNoCopy) a.dst[static_cast<int64_t>(s) * a.dst_stripe_stride + c + pos] = x;
    }
    for (int r = 0; r < a.rows; r++) dst_row<GATHER>(a, s, r)[pos] = static_cast<uint8_t>(acc >> (8 * r));
  }
}

// --- parity scrub kernels (nxec_rs_scrub_stripes) ---
// Detect, vector form: K = KD + ROWS sources per lane through the work-queue
// tile loop (prefetch while 2 x 4K source registers fit the 128-VGPR budget).
template <int KD, int ROWS, bool FULL>
__global__ __launch_bounds__(kBlock) void k_scrub_vec(const ScrubArgs a) {
  constexpr int K = KD + ROWS;
  constexpr int R = default_r(KD);
  constexpr bool PF = scrub_prefetch(K, FULL);
  using Body = ScrubBody<KD, ROWS, R>;
  static_assert(K <= kScrubMaxSrc && Body::kLds + kRingBytes == scrub_vec_lds(KD), "scrub kernels are queue-driven");
  extern __shared__ uint32_t tab[];
  Body::setup(a.m, tab);
  __syncthreads();
  mul_tiles<K, false, FULL, PF, true>(a.m, Body(tab, a.status), tab + Body::kLds / 4);
}

// Detect, byte form: any k and alignment, chunk bytes [byte_begin, len).
__global__ __launch_bounds__(256) void k_scrub_bytes(const ScrubArgs a) {
  extern __shared__ uint32_t tab[];
  const MulArgs &m = a.m;
  const int k = m.k;
  build_tables<1>(m, k, tab);
  __syncthreads();
  const int64_t span = m.len - m.byte_begin;
  const int64_t total = span * m.nstripes;
  for (int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; i < total;
       i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const uint32_t s = static_cast<uint32_t>(i / span);
    const int64_t pos = m.byte_begin + (i - static_cast<int64_t>(s) * span);
    uint32_t acc = 0;
    for (int j = 0; j < k; j++) acc ^= tab[j * 256 + src_chunk<false>(m, s, j)[pos]];
    const uint8_t *stripe = m.src + static_cast<int64_t>(s) * m.src_stripe_stride;
    uint32_t par = 0;
    for (int r = 0; r < m.rows; r++) par |= static_cast<uint32_t>(stripe[a.par_off[r] + pos]) << (8 * r);
    if (acc != par) scrub_flag(a.status, s);
  }
}

// Locate / heal: the rare path, one workgroup per stripe, plain bytes.
// Dynamic LDS: the (n-k) x k coefficients, then 256 syndrome columns of n-k
// bytes (syndrome r of thread t at [r*256 + t]).
__global__ __launch_bounds__(256) void k_scrub_locate(const ScrubLocateArgs a) {
  extern __shared__ uint32_t scrub_lds[];
  __shared__ int s_lo, s_hi;
  const int64_t s = blockIdx.x;
  if (a.status[s] == scrub::kClean) return;  // uniform
  const int tid = threadIdx.x;
  if (tid == 0 && a.nbad) atomicAdd(a.nbad, 1ull);
  const int n = a.n, k = a.k, m = n - k;
  if (!(a.flags & NXEC_SCRUB_LOCATE) || m < 2) return;  // the detect stage left UNLOCATED
  uint8_t *coef = reinterpret_cast<uint8_t *>(scrub_lds);
  uint8_t *syn = coef + (m * k + 15) / 16 * 16 + tid;
  for (int i = tid; i < m * k; i += 256) coef[i] = a.coef[i];
  if (tid == 0) {
    s_lo = INT32_MAX;
    s_hi = INT32_MIN;
  }
  __syncthreads();
  uint8_t *base = a.base + s * a.stripe_stride;
  const int64_t cs = a.chunk_stride;
  // sweep 1: the chunk that explains each inconsistent byte column
  int32_t mine = scrub::kClean;
  for (int64_t i = tid; i < a.len; i += 256) {
    for (int r = 0; r < m; r++) syn[r * 256] = base[(k + r) * cs + i];
    for (int j = 0; j < k; j++) {
      const uint32_t x = base[j * cs + i];
      for (int r = 0; r < m; r++) syn[r * 256] ^= static_cast<uint8_t>(gf_mul_dev(coef[r * k + j], x));
    }
    uint8_t e;
    const int32_t c = scrub::locate(n, k, coef, [&](int r) { return syn[r * 256]; }, &e);
    if (c != scrub::kClean) mine = (mine == scrub::kClean || mine == c) ? c : scrub::kUnlocated;
  }
  if (mine != scrub::kClean) {
    atomicMin(&s_lo, mine);
    atomicMax(&s_hi, mine);
  }
  __syncthreads();
  const int32_t located = (s_lo == s_hi && s_lo >= 0) ? s_lo : scrub::kUnlocated;
  if (tid == 0) a.status[s] = located;
  if (!(a.flags & NXEC_SCRUB_REPAIR) || located < 0) return;
  // sweep 2: the whole stripe agreed on one chunk; heal it
  if (located >= k) {  // parity row r: p_r ^= sigma_r
    const uint8_t *row = coef + (located - k) * k;
    uint8_t *p = base + located * cs;
    for (int64_t i = tid; i < a.len; i += 256) {
      uint32_t v = 0;
      for (int j = 0; j < k; j++) v ^= gf_mul_dev(row[j], base[j * cs + i]);
      if (p[i] != static_cast<uint8_t>(v)) p[i] = static_cast<uint8_t>(v);
    }
  } else {  // data chunk c: e = sigma_0 / c(0, c)
    const uint32_t ic = scrub::inv(coef[located]);
    uint8_t *d = base + located * cs;
    for (int64_t i = tid; i < a.len; i += 256) {
      uint32_t s0 = base[k * cs + i];
      for (int j = 0; j < k; j++) s0 ^= gf_mul_dev(coef[j], base[j * cs + i]);
      if (s0) d[i] ^= static_cast<uint8_t>(gf_mul_dev(s0, ic));
    }
  }
}

// --- variable-length batches (many objects per call) ---
// One launch over stripes of different chunk lengths and layouts.  Work unit =
// one 16-byte column piece; workgroup b owns the contiguous unit run
// [b*T/G, (b+1)*T/G), finds its first stripe by binary search over the unit
// prefix once (thread 0, LDS broadcast), and every thread then advances its
// own stripe cursor monotonically.  R = 1 packed-row LDS tables; 16-byte
// vector loads where the piece is complete and aligned, bytes otherwise.
// Not the throughput path for big objects (their full stripes go through
// k_mul_vec in gather form); it covers the ragged last stripes.
struct ListArgs {
  const ListStripe *stripes;
  const int64_t *prefix;
  int64_t nstripes, total;
  int32_t k, rows, row0;
  uint8_t coef[kMaxRowsPerPass * (NXEC_MAX_K + 1)];
};

__global__ __launch_bounds__(256) void k_mul_list(const ListArgs a) {
  extern __shared__ uint32_t tab[];
  __shared__ int64_t s_first;
  const int k = a.k;
  for (int i = threadIdx.x; i < k * 256; i += blockDim.x) {
    const int j = i >> 8;
    uint32_t e = 0;
    for (int r = 0; r < a.rows; r++) e |= gf_mul_dev(a.coef[r * k + j], static_cast<uint32_t>(i & 255)) << (8 * r);
    tab[i] = e;
  }
  const int64_t u0 = static_cast<int64_t>(blockIdx.x) * a.total / gridDim.x;
  const int64_t u1 = static_cast<int64_t>(blockIdx.x + 1) * a.total / gridDim.x;
  if (threadIdx.x == 0) {
    int64_t lo = 0, hi = a.nstripes - 1;  // last s with prefix[s] <= u0
    while (lo < hi) {
      const int64_t mid = (lo + hi + 1) >> 1;
      if (a.prefix[mid] <= u0) lo = mid;
      else hi = mid - 1;
    }
    s_first = lo;
  }
  __syncthreads();
  int64_t s = s_first;
  const char *tl = reinterpret_cast<const char *>(tab);
  for (int64_t u = u0 + threadIdx.x; u < u1; u += blockDim.x) {
    while (a.prefix[s + 1] <= u) s++;
    const ListStripe st = a.stripes[s];
    const int64_t off = (u - a.prefix[s]) * 16;
    const int64_t nb = st.len - off < 16 ? st.len - off : 16;
    const bool vec = nb == 16 && ((reinterpret_cast<uintptr_t>(st.src) | reinterpret_cast<uintptr_t>(st.dst) |
                                   static_cast<uint64_t>(st.src_cs) | static_cast<uint64_t>(st.dst_cs) |
                                   static_cast<uint64_t>(off)) & 15) == 0;
    uint8_t *drow0 = st.dst + static_cast<int64_t>(a.row0) * st.dst_cs + off;
    if (vec) {
      uint32_t acc[16];
#pragma unroll
      for (int i = 0; i < 16; i++) acc[i] = 0;
      for (int j = 0; j < k; j++) lookup16<1>(tl + j * 1024, ld_stream(st.src + j * st.src_cs + off), acc);
      store_rows(acc, a.rows, [=](int r) { return drow0 + r * st.dst_cs; });
    } else {
      for (int b = 0; b < nb; b++) {
        uint32_t acc = 0;
        for (int j = 0; j < k; j++) acc ^= tab[j * 256 + st.src[j * st.src_cs + off + b]];
        for (int r = 0; r < a.rows; r++) drow0[r * st.dst_cs + b] = static_cast<uint8_t>(acc >> (8 * r));
      }
    }
  }
}

// Last stripe of an object into the aligned tail arena: chunk j of the
// stripe = object bytes [j*cl, (j+1)*cl) (zero past the object's remaining
// rem bytes, chunk_manager.cc:390-399), written at dst + j*cls with
// cls = cl rounded up to 16 and zeros in [cl, cls).  One thread per 16-byte
// output vector; the 16 source bytes are assembled from dword-aligned loads
// with v_alignbit (the source offset j*cl has any alignment), bytes where
// the 20-byte window would leave the object.  Item i owns blocks
// [bstart[i], bstart[i+1]) of kPadVecs*256 vectors (thread 0 finds the item).
__global__ __launch_bounds__(256) void k_pad_chunks(const PadChunks *__restrict__ items,
                                                    const uint32_t *__restrict__ bstart, int64_t nitems) {
  __shared__ int64_t s_item;
  if (threadIdx.x == 0) {
    int64_t lo = 0, hi = nitems - 1;  // last item with bstart <= blockIdx.x
    while (lo < hi) {
      const int64_t mid = (lo + hi + 1) >> 1;
      if (bstart[mid] <= blockIdx.x) lo = mid;
      else hi = mid - 1;
    }
    s_item = lo;
  }
  __syncthreads();
  const int64_t item = s_item;
  const PadChunks it = items[item];
  const int64_t vpc = it.cls / 16;  // vectors per chunk
  const int64_t u0 = static_cast<int64_t>(blockIdx.x - bstart[item]) * (256 * kPadVecs);
#pragma unroll
  for (int r = 0; r < kPadVecs; r++) {
    const int64_t u = u0 + r * 256 + threadIdx.x;  // output vector
    if (u >= vpc * it.k) break;
    const int64_t j = u / vpc, x = (u - j * vpc) * 16;  // chunk, byte offset in it
    const int64_t sidx = j * it.cl + x;                 // source byte of output byte x
    const int64_t nvalid = min(min(static_cast<int64_t>(16), it.cl - x), it.rem - sidx);  // may be <= 0
    uint32_t w[4] = {0, 0, 0, 0};
    if (nvalid > 0) {
      const uint8_t *sp = it.src + sidx;
      const uintptr_t base = reinterpret_cast<uintptr_t>(sp) & ~uintptr_t(3);
      if (nvalid == 16 && base + 20 <= reinterpret_cast<uintptr_t>(it.src + it.rem)) {
        const uint32_t *q = reinterpret_cast<const uint32_t *>(base);
        const uint32_t sb = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(sp) & 3) * 8;
        const uint32_t r0 = q[0], r1 = q[1], r2 = q[2], r3 = q[3], r4 = q[4];
        w[0] = __builtin_amdgcn_alignbit(r1, r0, sb);
        w[1] = __builtin_amdgcn_alignbit(r2, r1, sb);
        w[2] = __builtin_amdgcn_alignbit(r3, r2, sb);
        w[3] = __builtin_amdgcn_alignbit(r4, r3, sb);
      } else {
        for (int b = 0; b < nvalid; b++) w[b >> 2] |= static_cast<uint32_t>(sp[b]) << (8 * (b & 3));
      }
    }
    st_stream(it.dst + j * it.cls + x, u32x4{w[0], w[1], w[2], w[3]});
  }
}

// 16-byte vector copy; `dst` may be device-mapped pinned host memory, so a
// device -> host transfer runs as shader stores over PCIe on the compute
// queue instead of an SDMA copy (which would queue behind the H2D copies).
__global__ __launch_bounds__(256) void k_copy16(u32x4 *__restrict__ dst, const u32x4 *__restrict__ src, int64_t n) {
  for (int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; i < n;
       i += static_cast<int64_t>(gridDim.x) * blockDim.x)
    __builtin_nontemporal_store(__builtin_nontemporal_load(src + i), dst + i);
}

__global__ void k_fill(uint8_t *p, int64_t bytes, uint64_t seed) {
  const int64_t words = (bytes + 7) / 8;
  const bool aligned = (reinterpret_cast<uintptr_t>(p) & 7) == 0;
  for (int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; i < words;
       i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    uint64_t z = seed + static_cast<uint64_t>(i + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    if (aligned && (i + 1) * 8 <= bytes) {
      reinterpret_cast<uint64_t *>(p)[i] = z;
    } else {
      for (int b = 0; b < 8 && i * 8 + b < bytes; b++) p[i * 8 + b] = static_cast<uint8_t>(z >> (8 * b));
    }
  }
}

__global__ void k_checksum(const uint8_t *p, int64_t bytes, unsigned long long *out) {
  const int64_t words = (bytes + 7) / 8;
  const bool aligned = (reinterpret_cast<uintptr_t>(p) & 7) == 0;
  uint64_t acc = 0;
  for (int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; i < words;
       i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    uint64_t w = 0;
    if (aligned && (i + 1) * 8 <= bytes) {
      w = reinterpret_cast<const uint64_t *>(p)[i];
    } else {
      for (int b = 0; b < 8 && i * 8 + b < bytes; b++) w |= static_cast<uint64_t>(p[i * 8 + b]) << (8 * b);
    }
    acc += w * static_cast<uint64_t>(2 * i + 1);
  }
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if ((threadIdx.x & 63) == 0) atomicAdd(out, static_cast<unsigned long long>(acc));
}

using KernelFn = void (*)(MulArgs);

template <int R, bool G, bool CP, bool FULL, int... Ks>
constexpr std::array<KernelFn, sizeof...(Ks)> vec_table(std::integer_sequence<int, Ks...>) {
  return {{&k_mul_vec<Ks + 1, R, G, CP, FULL>...}};
}

// One table per (form, R, full-tiles): indexed by k-1.  Strided full-tile
// kernels exist for every R (tuning knob NXEC_LDS_R); every other form only
// at the default R (16 for k <= 10, else 8).
using KTable = std::array<KernelFn, kMaxTemplK>;
template <int R, bool G, bool CP, bool FULL>
KTable make_table() {
  KTable t{};
  if constexpr (R == 16) {
    auto a = vec_table<16, G, CP, FULL>(std::make_integer_sequence<int, 10>{});
    for (int i = 0; i < 10; i++) t[i] = a[i];
  } else {
    auto a = vec_table<R, G, CP, FULL>(std::make_integer_sequence<int, kMaxTemplK>{});
    for (int i = 0; i < kMaxTemplK; i++) t[i] = a[i];
  }
  return t;
}
// [gather][copy][full]
const KTable kDefR16[2][2][2] = {
    {{make_table<16, false, false, false>(), make_table<16, false, false, true>()},
     {make_table<16, false, true, false>(), make_table<16, false, true, true>()}},
    {{make_table<16, true, false, false>(), make_table<16, true, false, true>()}, {KTable{}, KTable{}}}};
const KTable kDefR8[2][2][2] = {
    {{make_table<8, false, false, false>(), make_table<8, false, false, true>()},
     {make_table<8, false, true, false>(), make_table<8, false, true, true>()}},
    {{make_table<8, true, false, false>(), make_table<8, true, false, true>()}, {KTable{}, KTable{}}}};
const KTable kTuneR1 = make_table<1, false, false, true>();

template <bool G, int... Ks>
constexpr std::array<KernelFn, sizeof...(Ks)> perm_table(std::integer_sequence<int, Ks...>) {
  return {{&k_mul_perm<Ks + 1, G, false, true>...}};
}
// single-row kernels (complete tiles, no pass-through), [gather][k-1]
const std::array<KernelFn, kPermMaxK> kPerm[2] = {perm_table<false>(std::make_integer_sequence<int, kPermMaxK>{}),
                                                  perm_table<true>(std::make_integer_sequence<int, kPermMaxK>{})};

// scrub detect kernels: every k <= kScrubMaxK with 1..4 parity rows per pass
// (k + rows <= kScrubMaxSrc), [rows-1][full][k-1]
using ScrubFn = void (*)(ScrubArgs);
using ScrubTable = std::array<ScrubFn, kScrubMaxK>;
template <int ROWS, bool FULL, int... Ks>
constexpr ScrubTable scrub_table(std::integer_sequence<int, Ks...>) {
  return {{&k_scrub_vec<Ks + 1, ROWS, FULL>...}};
}
template <int ROWS>
constexpr std::array<ScrubTable, 2> scrub_tables() {
  return {{scrub_table<ROWS, false>(std::make_integer_sequence<int, kScrubMaxK>{}),
           scrub_table<ROWS, true>(std::make_integer_sequence<int, kScrubMaxK>{})}};
}
const std::array<ScrubTable, 2> kScrub[kMaxRowsPerPass] = {scrub_tables<1>(), scrub_tables<2>(), scrub_tables<3>(),
                                                           scrub_tables<4>()};

using RaggedFn = void (*)(RaggedArgs);
template <int... Ks>
constexpr std::array<RaggedFn, sizeof...(Ks)> ragged_table(std::integer_sequence<int, Ks...>) {
  return {{&k_mul_ragged<Ks + 1, default_r(Ks + 1)>...}};
}
const std::array<RaggedFn, kMaxRaggedK> kRagged = ragged_table(std::make_integer_sequence<int, kMaxRaggedK>{});

template <int... Ks>
constexpr auto mixed_table(std::integer_sequence<int, Ks...>) {
  return std::array<void (*)(MixedArgs), sizeof...(Ks)>{{&k_mul_mixed<Ks + 1, default_r(Ks + 1)>...}};
}
template <int... Ks>
constexpr auto decode_mixed_table(std::integer_sequence<int, Ks...>) {
  return std::array<void (*)(DecodeMixedArgs), sizeof...(Ks)>{{&k_decode_mixed<Ks + 1, default_r(Ks + 1)>...}};
}
const auto kMixed = mixed_table(std::make_integer_sequence<int, kMaxRaggedK>{});
const auto kDecodeMixed = decode_mixed_table(std::make_integer_sequence<int, kMaxRaggedK>{});
const void *mixed_fn(int k, bool full) {
  return full ? reinterpret_cast<const void *>(kDecodeMixed[k - 1]) : reinterpret_cast<const void *>(kMixed[k - 1]);
}
// [full]: the launch-record families
constexpr const char *kMixedFamily[2] = {"k_mul_mixed", "k_decode_mixed"};

// two update kernels, each prepared at the largest k it serves: R = 16 while default_r(k) is 16, R = 8 up to kMaxRaggedK
using UpdateFn = void (*)(UpdateArgs);
constexpr int kUpdateMaxK16 = 9;
static_assert(default_r(kUpdateMaxK16) == 16 && default_r(kUpdateMaxK16 + 1) == 8, "the update kernels follow default_r");
static_assert(update_lds(kMaxRaggedK) <= kLdsBytes, "the widest update tables and the ring fit");
UpdateFn update_fn(int k) { return k <= kUpdateMaxK16 ? &k_update_vec<16> : &k_update_vec<8>; }

// LDS replication policy (the LDS-replication probe overrides it, nxec_tuning.h).
int choose_r(int k, bool tunable) {
  if (k > kMaxTemplK) return 1;
  const int want = tunable ? tuning().lds_r : 0;
  if (want == 1) return 1;
  if (want == 8) return 8;
  if (want == 16 && k <= 10) return 16;
  // the largest replication that leaves room for the tile-queue ring: the
  // queue's dynamic tile order is worth far more than R = 16's fewer LDS bank
  // conflicts (k = 10: 0.80 vs 0.64-0.73 of 8 TB/s, profiles/r01_mem_pattern.log)
  return default_r(k);
}

KernelFn vec_kernel(int k, int r, bool gather, bool copy, bool full) {
  if (k > kMaxTemplK) return gather ? &k_mul_vec_dyn<true> : &k_mul_vec_dyn<false>;
  if (r == 1 && !gather && !copy && full) return kTuneR1[k - 1];
  if (r == 16 && k <= 10) return kDefR16[gather][copy][full][k - 1];
  return kDefR8[gather][copy][full][k - 1];
}

// Appends every non-null entry of a dispatch table (indexed by k - 1) to the
// preparation list; bytes(k) is the family's size function.
template <class Table, class BytesF>
void list_table(std::vector<KernelLds> &out, const Table &table, const char *family, const BytesF &bytes) {
  int k = 0;
  for (auto fn : table) {
    k++;
    if (fn) out.push_back({reinterpret_cast<const void *>(fn), family, bytes(k), false});
  }
}

// This file's kernels with dynamic LDS, by walking the dispatch tables above.
void list_kernels(std::vector<KernelLds> &out) {
  for (int g = 0; g < 2; g++)
    for (int c = 0; c < 2; c++)
      for (int f = 0; f < 2; f++) {
        list_table(out, kDefR16[g][c][f], "k_mul_vec", [](int k) { return vec_lds(k, 16); });
        list_table(out, kDefR8[g][c][f], "k_mul_vec", [](int k) { return vec_lds(k, 8); });
      }
  list_table(out, kTuneR1, "k_mul_vec tune", [](int k) { return vec_lds(k, 1); });
  for (const auto &t : kPerm) list_table(out, t, "k_mul_perm", perm_lds);
  for (KernelFn fn : {&k_mul_vec_dyn<false>, &k_mul_vec_dyn<true>, &k_mul_bytes<false>, &k_mul_bytes<true>})
    out.push_back({reinterpret_cast<const void *>(fn), "dyn/bytes", bytes_lds(NXEC_MAX_K), false});
  for (const auto &rows : kScrub)
    for (const ScrubTable &t : rows) list_table(out, t, "k_scrub_vec", scrub_vec_lds);
  out.push_back({reinterpret_cast<const void *>(&k_scrub_bytes), "k_scrub_bytes", bytes_lds(NXEC_MAX_K), false});
  list_table(out, kRagged, "k_mul_ragged", ragged_lds);
  // the mixed kernels' tables start at dynamic LDS byte 0: no static LDS
  for (int full = 0; full < 2; full++)
    for (int k = 1; k <= kMaxRaggedK; k++)
      out.push_back({mixed_fn(k, full), kMixedFamily[full], mixed_lds(k), true});
  // like them, the update kernels index their tables from dynamic LDS byte 0
  out.push_back({reinterpret_cast<const void *>(update_fn(kUpdateMaxK16)), "k_update_vec", update_lds(kUpdateMaxK16), true});
  out.push_back({reinterpret_cast<const void *>(update_fn(kMaxRaggedK)), "k_update_vec", update_lds(kMaxRaggedK), true});
  out.push_back({reinterpret_cast<const void *>(&k_update_bytes), "k_update_bytes", bytes_lds(NXEC_MAX_K), false});
}

}  // namespace

// single-row passes use the VALU nibble-table kernel (a probe forces LDS tables, nxec_tuning.h)
bool use_perm(int k, int rows, bool full, bool copy, bool gather) {
  if (rows != 1 || k > kPermMaxK || !full || copy) return false;
  if (k == 11 && !gather) return false;  // this instantiation alone spills (hipcc 7.2 schedule); LDS tables instead
  return !tuning().lds_single_row;
}

LaunchInfo plan_launch(int k, int rows, int64_t vec_count, int64_t nstripes, int num_cus, bool full, bool copy,
                       bool gather) {
  const bool tunable = !gather && !copy && full;
  LaunchInfo li{};
  li.block = kBlock;
  int per_cu = 1;
  if (use_perm(k, rows, full, copy, gather)) {
    li.perm = true;
    li.lds_copies = 0;
    li.lds_bytes = perm_lds(k);
    li.variant = "vec_perm";
  } else {
    li.lds_copies = choose_r(k, tunable);
    const bool queued = k <= kMaxTemplK && vec_queued(k, li.lds_copies);
    li.lds_bytes = k <= kMaxTemplK ? vec_lds(k, li.lds_copies) : bytes_lds(k);
    per_cu = kLdsBytes / (li.lds_bytes > 0 ? li.lds_bytes : 1);
    if (per_cu > 2) per_cu = 2;  // 2 x 16 waves = the CU's 32-wave limit
    if (per_cu < 1) per_cu = 1;
    // queue-driven launches: one workgroup per CU keeps the in-flight window
    // tightest (two per CU measured 0.755 vs 0.798 of 8 TB/s, XOR probe)
    if (queued) per_cu = 1;
    li.variant = k > kMaxTemplK ? "vec_dyn" : "vec_lds";
  }
  const int64_t tps = (vec_count + kBlock - 1) / kBlock;
  int64_t ntiles = tps * nstripes;
  int64_t grid = static_cast<int64_t>(num_cus) * per_cu;
  if (grid > ntiles) grid = ntiles;
  li.grid = static_cast<int>(grid);
  return li;
}

void (*mul_kernel(const LaunchInfo &li, int k, bool gather, bool copy, bool full))(MulArgs) {
  return li.perm ? kPerm[gather][k - 1] : vec_kernel(k, li.lds_copies, gather, copy, full);
}
void (*scrub_kernel(int kd, int rows, bool full, int *lds_bytes))(ScrubArgs) {
  *lds_bytes = scrub_vec_lds(kd);
  return kScrub[rows - 1][full][kd - 1];
}
const void *ragged_kernel(int k, int *lds_bytes) {
  *lds_bytes = ragged_lds(k);
  return reinterpret_cast<const void *>(kRagged[k - 1]);
}

const void *mixed_kernel(int k, bool full, int *lds_bytes) {
  *lds_bytes = mixed_lds(k);
  return mixed_fn(k, full);
}

const void *update_vec_kernel(int k, int *lds_bytes) {
  *lds_bytes = update_lds(k);
  return reinterpret_cast<const void *>(update_fn(k));
}
const void *update_bytes_kernel(int k, int *lds_bytes) {
  *lds_bytes = bytes_lds(k);
  return reinterpret_cast<const void *>(&k_update_bytes);
}

const std::vector<KernelLds> &kernel_lds_list() {
  static const std::vector<KernelLds> list = [] {
    std::vector<KernelLds> l;
    list_kernels(l);
    list_encode_md5_kernels(l);
    list_files_md5_kernels(l);
    return l;
  }();
  return list;
}

int raise_lds(const void *fn, int bytes, const char *family, bool no_static) {
  hipFuncAttributes fa{};
  if (no_static && (hipFuncGetAttributes(&fa, fn) != hipSuccess || fa.sharedSizeBytes != 0))
    return set_error(NXEC_ERR_HIP, "%s: static LDS present (the tables must start at LDS byte 0)", family);
  const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e != hipSuccess) return set_error(NXEC_ERR_HIP, "hipFuncSetAttribute(%s): %s", family, hipGetErrorString(e));
  return NXEC_OK;
}

int prepare_kernels() {
  for (const KernelLds &e : kernel_lds_list())
    if (int rc = raise_lds(e.fn, e.bytes, e.family, e.no_static)) return rc;
  return NXEC_OK;
}

namespace {

// Work-queue run length: about 12 tiles' worth of chunk traffic per grab (a
// 16 KiB tile moves k + rows (+ copies) 16 KiB pieces), so wide stripes grab
// one tile at a time (the tightest in-flight window) and narrow ones (CAR XOR,
// small partial encodes) several, which keeps the single counter well under
// its atomic rate (~80 M/s) and the grab latency hidden.
uint32_t tiles_per_grab(int k, int rows, int copies) {
  const int units = k + rows + copies;
  return static_cast<uint32_t>(std::max(1, std::min(8, (12 + units - 1) / units)));
}

// Chunks of >= 2 MiB at a power-of-two-aligned chunk stride: walk groups of 8
// stripes column-major, so the in-flight window spans 8 stripes like it does
// at 1 MiB (4 MiB stride: 0.655 -> 0.711 of 8 TB/s,
// profiles/r01_chunk_stride_group.log).  A padded stride (the recommended
// layout, nxec_batch_layout) runs best stripe-major (4 MiB + 2 KiB: 0.758 at
// sg 1, profiles/r02_layout_sweep.log).
uint32_t stripe_group_for(int64_t vec_count, bool aliased) {
  return ((vec_count + kBlock - 1) / kBlock >= 128 && aliased) ? 8 : 1;
}

// host side of the tile-queue ring: each vector launch draws the next slot
// (4096 launches would have to be in flight at once for two to share one)
std::atomic<uint32_t> g_next_slot{0};

// A slot is cleaned by the last workgroup of the launch that used it.  A
// launch that never completes (enqueue failure, aborted stream) would leave a
// non-zero counter behind, and the launch that draws the same slot 4096
// launches later would start past tile 0 and silently skip tiles.  Every
// failed launch therefore zeroes its slot from the host before returning.
int reset_queue_slots(int first, int count, hipStream_t st) {
  void *base = nullptr;
  hipError_t e = hipGetSymbolAddress(&base, HIP_SYMBOL(g_tile_queue));
  if (e == hipSuccess) {
    if (count <= 0) {
      first = 0;
      count = kQueueSlots;
    }
    e = hipMemsetAsync(static_cast<uint8_t *>(base) + static_cast<size_t>(first) * 128, 0,
                       static_cast<size_t>(count) * 128, st);
  }
  return hip_check(e, "tile-queue reset");
}

int launch_failed(hipError_t e, const char *family, int slot, hipStream_t st) {
  const int rc = set_error(NXEC_ERR_HIP, "launch %s: %s", family, hipGetErrorString(e));
  if (slot >= 0) (void)reset_queue_slots(slot, 1, st);
  return rc;
}

// The launch of every kernel outside the tile queue, 256 threads a workgroup;
// `name` is the kernel's in the error text.  A launch record, where the kernel
// has one, is its caller's.
template <class... Params, class... Args>
int plain_launch(const char *name, void (*fn)(Params...), int64_t grid, size_t lds, void *stream, const Args &...args) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(fn, dim3(static_cast<unsigned>(grid)), dim3(256), lds, st, args...);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? NXEC_OK : launch_failed(e, name, -1, st);
}

// Grid of the byte kernels over `total` bytes or 16-byte units: 256 a workgroup, at most 8 workgroups per CU.
int64_t byte_grid(int64_t total, int num_cus) {
  return std::min<int64_t>((total + 255) / 256, static_cast<int64_t>(num_cus) * 8);
}

// What one launch of a tile-queue kernel (k_mul_vec, k_mul_perm, k_scrub_vec,
// k_mul_ragged; k_mul_vec_dyn shares k_mul_vec's path) used.  The launch and
// its record line both read this, so the record cannot drift from the launch.
// The constructor takes what every family has; a family sets its other fields by name.
struct QueueLaunch {
  const char *family, *kkey;  // kkey: "k", or "kd" for the scrub
  int k, rows, r, pf;
  uint32_t tpg;
  int64_t grid;
  int lds;
  int gather = -1, copy = -1, full = -1;  // -1: the family has no such form (the key is left out)
  int q = 1;
  uint32_t sg = 0;             // 0: no stripe groups (left out)
  int32_t slot = 0;            // drawn by queue_launch
  const char *tail = nullptr;  // family-specific keys after the slot
  QueueLaunch(const char *family, const char *kkey, int k, int rows, int r, int pf, uint32_t tpg, int64_t grid, int lds)
      : family(family), kkey(kkey), k(k), rows(rows), r(r), pf(pf), tpg(tpg), grid(grid), lds(lds) {}
};

void record_launch(const QueueLaunch &l) {
  char s[224];
  const size_t cap = sizeof s;
  int n = std::snprintf(s, cap, "family=%s %s=%d rows=%d r=%d", l.family, l.kkey, l.k, l.rows, l.r);
  if (l.gather >= 0) n += std::snprintf(s + n, cap - n, " gather=%d copy=%d", l.gather, l.copy);
  if (l.full >= 0) n += std::snprintf(s + n, cap - n, " full=%d", l.full);
  n += std::snprintf(s + n, cap - n, " pf=%d q=%d tpg=%u", l.pf, l.q, l.tpg);
  if (l.sg) n += std::snprintf(s + n, cap - n, " sg=%u", l.sg);
  n += std::snprintf(s + n, cap - n, " grid=%lld slot=%d", static_cast<long long>(l.grid), l.slot);
  if (l.tail) std::snprintf(s + n, cap - n, " %s", l.tail);
  launch_log_append("%s", s);
}

// The queue-driven launch: draws the launch's tile-queue slot (draw = false:
// none, the kernel walks static tile runs) into `slot`, a member of the kernel
// arguments `a`; records and launches; a failed launch zeroes its slot.
template <class Args>
int queue_launch(void (*fn)(Args), const Args &a, int32_t &slot, QueueLaunch &l, hipStream_t st, bool draw = true) {
  slot = l.slot = draw ? static_cast<int32_t>(g_next_slot.fetch_add(1, std::memory_order_relaxed) % kQueueSlots) : -1;
  if (launch_log_on()) record_launch(l);
  hipLaunchKernelGGL(fn, dim3(static_cast<unsigned>(l.grid)), dim3(kBlock), l.lds, st, a);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? NXEC_OK : launch_failed(e, l.family, slot, st);
}

// A chunk's vector range as up to two launches: launch(begin, count, full) for
// its complete tiles (no lane predicates), then for the ragged remainder.
template <class F>
int split_vectors(int64_t vec_count, int64_t nstripes, const F &launch) {
  const int64_t tps = (vec_count + kBlock - 1) / kBlock;
  if (tps * nstripes >= (int64_t(1) << 32) || vec_count >= (int64_t(1) << 32))
    return set_error(NXEC_ERR_INVALID, "batch too large for one launch (split nstripes)");
  const int64_t full = vec_count / kBlock * kBlock;
  int rc = full > 0 ? launch(int64_t(0), full, true) : NXEC_OK;
  if (rc == NXEC_OK && vec_count > full) rc = launch(full, vec_count - full, false);
  return rc;
}

}  // namespace

int launch_mul(const MulArgs &a, bool vec_ok, int num_cus, void *stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (a.nstripes <= 0 || a.len <= 0) return NXEC_OK;
  if (vec_ok && a.vec_count > 0) {
    const bool gather = a.src_ptrs != nullptr, copy = a.any_copy != 0;
    const bool dyn = a.k > kMaxTemplK;  // static tile runs: no queue, no stripe groups
    int copies = 0;
    for (int j = 0; copy && j < a.k; j++) copies += a.copy_off[j] != kNoCopy;
    const uint32_t tpg = tiles_per_grab(a.k, a.rows, copies);
    const bool aliased = gather || a.src_chunk_stride % (int64_t(1) << 20) == 0;
    const uint32_t sg = tuning().stripe_group > 0 ? static_cast<uint32_t>(tuning().stripe_group)
                                                  : stripe_group_for(a.vec_count, aliased);
    const int rc = split_vectors(a.vec_count, a.nstripes, [&](int64_t begin, int64_t count, bool full) {
      MulArgs b = a;
      b.tiles_per_grab = tpg;
      b.stripe_group = sg;
      b.vec_begin = a.vec_begin + begin;
      b.vec_count = count;
      const LaunchInfo li = plan_launch(b.k, b.rows, count, b.nstripes, num_cus, full, copy, gather);
      QueueLaunch l(li.perm ? "k_mul_perm" : dyn ? "k_mul_vec_dyn" : "k_mul_vec", "k", b.k, b.rows, li.lds_copies,
                    li.perm ? perm_prefetch(b.k) : !dyn && vec_prefetch(b.k, copy, full), dyn ? 0 : tpg, li.grid,
                    li.lds_bytes);
      l.gather = gather;
      l.copy = copy;
      l.full = full;
      l.q = li.perm || (!dyn && vec_queued(b.k, li.lds_copies));
      l.sg = dyn ? 1 : sg;
      return queue_launch(mul_kernel(li, b.k, gather, copy, full), b, b.queue_slot, l, st,
                          !dyn && !tuning().static_order);
    });
    if (rc) return rc;
  }
  if (a.byte_begin < a.len) {
    const int64_t blocks = byte_grid((a.len - a.byte_begin) * a.nstripes, num_cus);
    if (launch_log_on())
      launch_log_append("family=k_mul_bytes k=%d rows=%d r=1 gather=%d copy=%d full=0 pf=0 q=0 tpg=0 sg=1 grid=%lld "
                        "byte_begin=%lld",
                        a.k, a.rows, a.src_ptrs != nullptr, a.any_copy != 0, static_cast<long long>(blocks),
                        static_cast<long long>(a.byte_begin));
    return plain_launch("k_mul_bytes", a.src_ptrs ? &k_mul_bytes<true> : &k_mul_bytes<false>, blocks, bytes_lds(a.k), st, a);
  }
  return NXEC_OK;
}

bool scrub_vec_shape(int k, int rows) {
  return k >= 1 && k <= kScrubMaxK && rows >= 1 && rows <= kMaxRowsPerPass && k + rows <= kScrubMaxSrc;
}

int launch_scrub_detect(const ScrubArgs &a0, bool vec_ok, int num_cus, void *stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  ScrubArgs a = a0;
  MulArgs &m = a.m;
  if (m.nstripes <= 0 || m.len <= 0 || m.rows <= 0) return NXEC_OK;
  const bool vec = vec_ok && scrub_vec_shape(m.k, m.rows);
  m.vec_begin = 0;
  m.vec_count = vec ? m.len / 16 : 0;
  m.byte_begin = m.vec_count * 16;
  if (m.vec_count > 0) {
    for (int r = 0; r < m.rows; r++) m.src_off[m.k + r] = a.par_off[r];
    // The encode's run length and tile order (launch_mul), always queue-driven
    // and never with its two tuning knobs: tuning().static_order and
    // tuning().stripe_group are A/B probes of the encode kernels, and a scrub
    // that changed with them would only blur those measurements.
    m.tiles_per_grab = tiles_per_grab(m.k, m.rows, 0);
    m.stripe_group = stripe_group_for(m.vec_count, m.src_chunk_stride % (int64_t(1) << 20) == 0);
    const int rc = split_vectors(m.vec_count, m.nstripes, [&](int64_t begin, int64_t count, bool full) {
      ScrubArgs b = a;
      b.m.vec_begin = begin;
      b.m.vec_count = count;
      const int64_t ntiles = (count + kBlock - 1) / kBlock * m.nstripes;
      int lds = 0;
      const auto fn = scrub_kernel(m.k, m.rows, full, &lds);
      QueueLaunch l("k_scrub_vec", "kd", m.k, m.rows, default_r(m.k), scrub_prefetch(m.k + m.rows, full),
                    m.tiles_per_grab, std::min<int64_t>(num_cus, ntiles), lds);
      l.full = full;
      l.sg = m.stripe_group;
      return queue_launch(fn, b, b.m.queue_slot, l, st);
    });
    if (rc) return rc;
  }
  if (m.byte_begin < m.len) {
    const int64_t blocks = byte_grid((m.len - m.byte_begin) * m.nstripes, num_cus);
    if (launch_log_on())
      launch_log_append("family=k_scrub_bytes kd=%d rows=%d grid=%lld byte_begin=%lld", m.k, m.rows,
                        static_cast<long long>(blocks), static_cast<long long>(m.byte_begin));
    return plain_launch("k_scrub_bytes", k_scrub_bytes, blocks, bytes_lds(m.k), st, a);
  }
  return NXEC_OK;
}

int launch_scrub_locate(const ScrubLocateArgs &a, void *stream) {
  if (a.nstripes <= 0) return NXEC_OK;
  if (a.nstripes >= (int64_t(1) << 31)) return set_error(NXEC_ERR_INVALID, "scrub: too many stripes for one launch");
  const int m = a.n - a.k;
  const size_t lds = static_cast<size_t>((m * a.k + 15) / 16 * 16) + static_cast<size_t>(m) * 256;
  return plain_launch("k_scrub_locate", k_scrub_locate, a.nstripes, lds, stream, a);
}

int reset_work_queues(void *stream) {
  const int rc = reset_queue_slots(0, 0, static_cast<hipStream_t>(stream));
  return rc ? rc : hip_check(hipStreamSynchronize(static_cast<hipStream_t>(stream)), "tile-queue reset sync");
}

int debug_poison_next_queue_slot(uint32_t next_tile) {
  void *base = nullptr;
  hipError_t e = hipGetSymbolAddress(&base, HIP_SYMBOL(g_tile_queue));
  const uint32_t slot = g_next_slot.load() % kQueueSlots;
  if (e == hipSuccess)
    e = hipMemcpy(static_cast<uint8_t *>(base) + static_cast<size_t>(slot) * 128, &next_tile, sizeof(next_tile),
                  hipMemcpyHostToDevice);
  return hip_check(e, "tile-queue poison");
}

int launch_mul_list(int rows, int k, const uint8_t *coeffs, const ListStripe *d_stripes, const int64_t *d_prefix,
                    int64_t nstripes, int64_t total_units, int num_cus, void *stream) {
  if (nstripes <= 0 || total_units <= 0 || rows <= 0) return NXEC_OK;
  if (k < 1 || k > NXEC_MAX_K) return set_error(NXEC_ERR_INVALID, "k=%d out of range", k);
  const int64_t blocks = byte_grid(total_units, num_cus);
  for (int p = 0; p < row_passes(rows); p++) {
    ListArgs a;
    std::memset(&a, 0, sizeof(a));
    a.stripes = d_stripes;
    a.prefix = d_prefix;
    a.nstripes = nstripes;
    a.total = total_units;
    a.k = k;
    a.rows = pass_coef(rows, k, coeffs, p, a.coef);
    a.row0 = p * kMaxRowsPerPass;
    if (launch_log_on())
      launch_log_append("family=k_mul_list k=%d rows=%d grid=%lld", k, a.rows, static_cast<long long>(blocks));
    if (int rc = plain_launch("k_mul_list", k_mul_list, blocks, bytes_lds(k), stream, a)) return rc;
  }
  return NXEC_OK;
}

int launch_mul_ragged(int rows, int k, const uint8_t *coeffs, const ListStripe *d_stripes, const uint32_t *d_tile_stripe,
                      const uint32_t *d_stripe_tile0, int64_t ntiles, int num_cus, void *stream) {
  if (ntiles <= 0 || rows <= 0) return NXEC_OK;
  if (k < 1 || k > kMaxRaggedK) return set_error(NXEC_ERR_INVALID, "ragged launch: k=%d unsupported", k);
  if (ntiles >= (int64_t(1) << 32)) return set_error(NXEC_ERR_INVALID, "ragged launch: too many tiles");
  const int64_t grid = std::min<int64_t>(num_cus, ntiles);
  for (int p = 0; p < row_passes(rows); p++) {
    RaggedArgs a;
    std::memset(&a, 0, sizeof(a));
    a.stripes = d_stripes;
    a.tile_stripe = d_tile_stripe;
    a.stripe_tile0 = d_stripe_tile0;
    a.ntiles = static_cast<uint32_t>(ntiles);
    a.k = k;
    a.rows = pass_coef(rows, k, coeffs, p, a.coef);
    a.row0 = p * kMaxRowsPerPass;
    a.tiles_per_grab = tiles_per_grab(k, a.rows, 0);
    QueueLaunch l("k_mul_ragged", "k", k, a.rows, default_r(k), ragged_prefetch(k), a.tiles_per_grab, grid, ragged_lds(k));
    if (int rc = queue_launch(kRagged[k - 1], a, a.queue_slot, l, static_cast<hipStream_t>(stream))) return rc;
  }
  return NXEC_OK;
}

int launch_mixed(int k, bool full, const uint8_t *src, int64_t stripe_stride, uint8_t *dst, int64_t out_stripe_stride,
                 int64_t len, const MixedSeg *d_segs, const uint32_t *d_order, const uint32_t *d_seg_of, int64_t nitems,
                 int64_t nsegs, int64_t nstripes, int num_cus, void *stream) {
  if (nitems <= 0 || len <= 0) return NXEC_OK;
  const char *what = full ? "mixed decode launch" : "mixed launch";
  if (k < 1 || k > kMaxRaggedK) return set_error(NXEC_ERR_INVALID, "%s: k=%d unsupported", what, k);
  const int64_t nvec = len / 16, tps = (nvec + kBlock - 1) / kBlock;
  if (len % 16 || nvec >= (int64_t(1) << 32) || tps * nitems >= (int64_t(1) << 32))
    return set_error(NXEC_ERR_INVALID, "%s: too many tiles or a sub-16-byte tail", what);
  DecodeMixedArgs a{};
  a.src = src;
  a.dst = dst;
  a.src_stripe_stride = stripe_stride;
  a.dst_stripe_stride = out_stripe_stride;
  a.segs = d_segs;
  a.order = d_order;
  a.seg_of = d_seg_of;
  a.tps = static_cast<uint32_t>(tps);
  a.nvec = static_cast<uint32_t>(nvec);
  a.ntiles = static_cast<uint32_t>(tps * nitems);
  // full: a tile of a plan's first segment loads k pieces and stores k: its rows and its copies together
  a.tiles_per_grab = full ? tiles_per_grab(k, 0, k) : tiles_per_grab(k, kMaxRowsPerPass, 0);
  char tail[64];
  std::snprintf(tail, sizeof tail, "segs=%lld stripes=%lld", static_cast<long long>(nsegs),
                static_cast<long long>(nstripes));
  QueueLaunch l(kMixedFamily[full], "k", k, kMaxRowsPerPass, default_r(k), ragged_prefetch(k), a.tiles_per_grab,
                std::min<int64_t>(num_cus, a.ntiles), mixed_lds(k));
  l.tail = tail;
  if (full) return queue_launch(kDecodeMixed[k - 1], a, a.queue_slot, l, static_cast<hipStream_t>(stream));
  return queue_launch<MixedArgs>(kMixed[k - 1], a, a.queue_slot, l, static_cast<hipStream_t>(stream));
}

namespace {
void update_pass(UpdateArgs &a, int k, int rows, int row0, const uint8_t *coef, uint8_t *base, int64_t chunk_stride,
                 bool last) {
  a.base = base;
  a.k = k;
  a.rows = rows;
  a.last = last;
  a.chunk_stride = static_cast<uint32_t>(chunk_stride);
  pass_coef(rows, k, coef, 0, a.coef);  // the caller's rows are this pass's: coef starts at row0
  for (int r = 0; r < rows; r++) a.par_off[r] = static_cast<uint32_t>((k + row0 + r) * chunk_stride);
}
}  // namespace

int launch_update_vec(int k, int rows, int row0, const uint8_t *coef, uint8_t *base, int64_t chunk_stride,
                      const UpdateItem *d_items, const uint32_t *d_tile_item, int64_t ntiles, bool last,
                      int64_t nupdates, int round, int pass, int num_cus, void *stream) {
  if (ntiles <= 0) return NXEC_OK;
  if (k < 1 || k > kMaxRaggedK || rows < 0 || rows > kMaxRowsPerPass)
    return set_error(NXEC_ERR_INVALID, "update launch: k=%d rows=%d unsupported", k, rows);
  if (ntiles >= (int64_t(1) << 32)) return set_error(NXEC_ERR_INVALID, "update launch: too many tiles");
  UpdateArgs a{};
  update_pass(a, k, rows, row0, coef, base, chunk_stride, last);
  a.items = d_items;
  a.tile_item = d_tile_item;
  a.ntiles = static_cast<uint32_t>(ntiles);
  // a tile moves the old and new data, the new data back on the last pass, and every parity row both ways
  a.tiles_per_grab = tiles_per_grab(2 + (last ? 1 : 0), 2 * rows, 0);
  char tail[96];
  std::snprintf(tail, sizeof tail, "tiles=%lld updates=%lld round=%d pass=%d last=%d", static_cast<long long>(ntiles),
                static_cast<long long>(nupdates), round, pass, last ? 1 : 0);
  QueueLaunch l("k_update_vec", "k", k, rows, default_r(k), 1, a.tiles_per_grab, std::min<int64_t>(num_cus, ntiles),
                update_lds(k));
  l.tail = tail;
  return queue_launch(update_fn(k), a, a.queue_slot, l, static_cast<hipStream_t>(stream));
}

int launch_update_bytes(int k, int rows, int row0, const uint8_t *coef, uint8_t *base, int64_t chunk_stride,
                        const UpdateItem *d_items, const int64_t *d_byte_prefix, int64_t nitems, int64_t nbytes,
                        bool last, int round, int pass, int num_cus, void *stream) {
  if (nitems <= 0 || nbytes <= 0) return NXEC_OK;
  if (k < 1 || k > NXEC_MAX_K || rows < 0 || rows > kMaxRowsPerPass)
    return set_error(NXEC_ERR_INVALID, "update launch: k=%d rows=%d unsupported", k, rows);
  UpdateArgs a{};
  update_pass(a, k, rows, row0, coef, base, chunk_stride, last);
  a.items = d_items;
  a.byte_prefix = d_byte_prefix;
  a.nitems = nitems;
  a.nbytes = nbytes;
  a.queue_slot = -1;
  const int64_t blocks = byte_grid(nbytes, num_cus);
  if (launch_log_on())
    launch_log_append("family=k_update_bytes k=%d rows=%d r=1 grid=%lld items=%lld round=%d pass=%d last=%d", k, rows,
                      static_cast<long long>(blocks), static_cast<long long>(nitems), round, pass, last ? 1 : 0);
  return plain_launch("k_update_bytes", k_update_bytes, blocks, bytes_lds(k), stream, a);
}

int launch_pad_chunks(const PadChunks *d_items, const uint32_t *d_bstart, int64_t nitems, int64_t nblocks,
                      void *stream) {
  if (nitems <= 0 || nblocks <= 0) return NXEC_OK;
  if (nblocks >= (int64_t(1) << 31)) return set_error(NXEC_ERR_INVALID, "pad-chunks launch too large");
  return plain_launch("k_pad_chunks", k_pad_chunks, nblocks, 0, stream, d_items, d_bstart, nitems);
}

int launch_copy16(void *dst, const void *src, size_t bytes, int num_cus, void *stream) {
  if (bytes == 0) return NXEC_OK;
  if (bytes % 16 || (reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src)) & 15)
    return set_error(NXEC_ERR_INVALID, "copy16: unaligned");
  const int64_t n = static_cast<int64_t>(bytes / 16);
  const int64_t blocks = std::min<int64_t>((n + 255) / 256, static_cast<int64_t>(num_cus) * 4);
  return plain_launch("k_copy16", k_copy16, blocks, 0, stream, static_cast<u32x4 *>(dst),
                      static_cast<const u32x4 *>(src), n);
}

int launch_fill(void *d, size_t bytes, uint64_t seed, void *stream) {
  if (bytes == 0) return NXEC_OK;
  return plain_launch("k_fill", k_fill, 2048, 0, stream, static_cast<uint8_t *>(d), static_cast<int64_t>(bytes), seed);
}

int launch_checksum(const void *d, size_t bytes, uint64_t *d_out, void *stream) {
  return plain_launch("k_checksum", k_checksum, 1024, 0, stream, static_cast<const uint8_t *>(d),
                      static_cast<int64_t>(bytes), reinterpret_cast<unsigned long long *>(d_out));
}

}  // namespace nxec
