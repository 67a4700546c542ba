"""The digest matrix: the lengths and chunk layouts at which the plain MD5
kernel (k_md5, nexoedge_amd/csrc/nxec_md5.hip) is compared with hashlib, and
a model of the path each chunk takes through it.

Shared by tests/test_gpu_digest_paths.py (runs the matrix on the device) and
tests/test_digest_matrix_plan.py (proves on the CPU that the matrix reaches
every state of the kernel's streaming loops, for the ring shapes that stand in
the sources today).

k_md5 hashes one chunk per lane.  A chunk of `length` bytes has
nfull = length // 64 complete blocks and rem = length % 64 tail bytes:
  * a 16-byte aligned chunk streams all nfull blocks through
    md5_stream<D, G>: groups of G blocks through a ring of D group buffers,
    the last ngroups % D groups taken from the ring after the main loop, then
    the nfull % G leftover blocks one at a time;
  * any other chunk with nfull > 1 streams nblk = nfull - 1 blocks through
    md5_stream_u<Du, Gu> (dword loads, one extra dword per group, every word
    shifted by (address % 4) * 8 bits) and reads its last complete block byte
    by byte; with nfull <= 1 it reads everything byte by byte;
  * the tail and the padding are built in registers: one block when rem < 56,
    two otherwise.
The state of a streaming call is (ngroups % D, min(ngroups // D, 2), leftover):
which ring buffers hold the last groups, whether the main loop ran not at all,
once or more than once, and how many blocks follow the groups.

The constants below mirror nexoedge_amd/csrc (the CPU test reads the sources
and fails when one moves).
"""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nexoedge_amd", "csrc")

MD5_DEPTH, MD5_GROUP = 2, 8        # Tuning::md5_depth / md5_group: md5_stream<D, G> of the product build
MD5_U_DEPTH, MD5_U_GROUP = 2, 4    # md5_stream_u<2, 4>
MAX_MD5_REGIONS = 4                # kMaxMd5Regions
ENC_MD5_STEP = 256                 # kEncMd5Step
ENC_MD5_MAX_K = 20                 # kEncMd5MaxK
GATHER_MD5_MAX_K = 16              # kGatherMd5MaxK
MAX_ROWS = 4                       # kMaxRowsPerPass

SOURCE_CONSTANTS = {  # name in nxec_internal.h -> value here
    "kMaxMd5Regions": MAX_MD5_REGIONS,
    "kEncMd5Step": ENC_MD5_STEP,
    "kEncMd5MaxK": ENC_MD5_MAX_K,
    "kGatherMd5MaxK": GATHER_MD5_MAX_K,
    "kMaxRowsPerPass": MAX_ROWS,
}


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def source_constant(name):
    """The value of `constexpr int <name> = <int>;` in nxec_internal.h."""
    m = re.search(r"constexpr int %s = (\d+)\s*;" % re.escape(name), _source("nxec_internal.h"))
    assert m, f"{name} not found in nxec_internal.h"
    return int(m.group(1))


def source_ring_defaults():
    """(md5_depth, md5_group) as nxec_tuning.h initialises them."""
    m = re.search(r"int md5_depth = (\d+)\s*,\s*md5_group = (\d+)\s*;", _source("nxec_tuning.h"))
    assert m, "md5_depth / md5_group not found in nxec_tuning.h"
    return int(m.group(1)), int(m.group(2))


def source_misaligned_ring():
    """The template arguments of every md5_stream_u<D, G>( call in nxec_md5.hip."""
    calls = re.findall(r"md5_stream_u<\s*(\d+)\s*,\s*(\d+)\s*>\s*\(", _source("nxec_md5.hip"))
    assert calls, "no md5_stream_u<D, G>( call in nxec_md5.hip"
    return sorted({(int(d), int(g)) for d, g in calls})


def rup(x, m=16):
    return (x + m - 1) // m * m


# ------------------------------------------------------------ the matrix
# three periods of the aligned ring (D * G blocks) and one more block, so the last state of the third period
# still meets every tail length; six periods of the misaligned ring
LENGTHS = range(0, 64 * (3 * MD5_DEPTH * MD5_GROUP + 1))
NCHUNKS, NSTRIPES = 17, 4            # 68 lanes: two workgroups, the second with 4 live lanes
LANES = NCHUNKS * NSTRIPES
LAYOUTS = ("ragged", "aligned")
DIGEST_GUARD = 16
DIGEST_SLOT = LANES * 16 + DIGEST_GUARD  # one length's digests and the guard behind them
OK_SLOT = LANES + DIGEST_GUARD           # one length's ok map and the guard behind it


def strides(layout, length):
    """(chunk stride, stripe stride) of a layout at one length; the base is 16-byte aligned.
    ragged: the chunk stride is the smallest value >= length + 1 that is 1 mod 16 and the stripe stride is
    17 chunks + 5, so chunk c of stripe s sits at (6 * s + c) mod 16: every stripe shows all 16 alignments
    and aligned and misaligned lanes share a wave.  aligned: padded 16-byte strides, stripes packed."""
    if layout == "ragged":
        cs = length + 1 + (-length) % 16
        return cs, NCHUNKS * cs + 5
    assert layout == "aligned"
    cs = rup(length) + 16
    return cs, NCHUNKS * cs


def chunk_offset(layout, length, lane):
    cs, ss = strides(layout, length)
    s, c = divmod(lane, NCHUNKS)
    return s * ss + c * cs


def layout_bytes(layout, length):
    """Bytes from the base to the end of the last chunk."""
    return chunk_offset(layout, length, LANES - 1) + length


def buffer_bytes(layout):
    return rup(max(layout_bytes(layout, length) for length in LENGTHS)) + 64


def digest_offset(layout, length):
    """Where the digests of one length start in the shared digest buffer: an odd address in the ragged layout."""
    return (length - LENGTHS[0]) * DIGEST_SLOT + (3 if layout == "ragged" else 0)


def digest_bytes():
    return len(LENGTHS) * DIGEST_SLOT + 16


def altered(lane, length):
    """Verify test: this lane's expected digest has one bit flipped ..."""
    return (lane + length) % 3 == 0


def altered_byte(lane, length):
    """... in this byte."""
    return (lane + length) % 16


# ------------------------------------------------------------ path model
def ring_state(nblocks, depth, group):
    ngroups = nblocks // group
    return ngroups % depth, min(ngroups // depth, 2), nblocks - ngroups * group


def all_ring_states(depth, group):
    return {(a, b, c) for a in range(depth) for b in range(3) for c in range(group)}


def path(offset, length):
    """The path of a chunk at byte `offset` from a 16-byte aligned base: ("aligned", state),
    ("misaligned", state, shift) or ("bytes", nfull)."""
    nfull = length // 64
    if offset % 16 == 0:
        return ("aligned",) + ring_state(nfull, MD5_DEPTH, MD5_GROUP)
    if nfull > 1:
        return ("misaligned",) + ring_state(nfull - 1, MD5_U_DEPTH, MD5_U_GROUP) + (offset % 4 * 8,)
    return ("bytes", nfull)
