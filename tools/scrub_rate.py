"""Parity-scrub rate beside the encode (profiles/scrub_rs10_4.json).

RS(10,4), 1 MiB chunks, 4096 stripes in nxec_batch_layout's layout: the
detect-only scrub of the clean batch moves the same n*len*nstripes bytes as
the encode that made it (k reads + n-k writes there, n reads here).  Both are
timed with events in one process over interleaved rounds; one JSON line.

  python tools/scrub_rate.py                 encode / scrub pairs + the worst case of the rare path
  python tools/scrub_rate.py --scrub-only 3  just 3 detect-only scrubs (for a counters-only profiler run:
                                             rocprofv3 --pmc FETCH_SIZE, then WRITE_SIZE; tools/pmc_dispatch.py)
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nexoedge_amd import _lib, nxec  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=14)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--len", type=int, default=1 << 20)
    ap.add_argument("--stripes", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=4, help="calls per timed interval")
    ap.add_argument("--scrub-only", type=int, default=0, metavar="N")
    a = ap.parse_args()
    n, k, length, ns = a.n, a.k, a.len, a.stripes
    cs, ss = nxec.batch_layout(n, length)
    ctx = nxec.Context(0)
    buf = nxec.DeviceBuffer(ns * ss)
    aux = nxec.DeviceBuffer(ns * 4 + 16)
    cnt = (ns * 4 + 7) // 8 * 8
    buf.fill_random(2025)
    enc = lambda: ctx.rs_encode(n, k, buf.ptr, cs, ss, length, ns)  # noqa: E731
    scrub = lambda flags=0, nbad=None: ctx.rs_scrub_stripes(n, k, buf.ptr, cs, ss, length, ns, aux.ptr, flags,  # noqa: E731
                                                           nbad)
    enc()
    ctx.sync()
    if a.scrub_only:
        for _ in range(a.scrub_only):
            scrub()
        ctx.sync()
        st = aux.download()[: ns * 4].view(np.int32)
        print(json.dumps({"scrub_only": a.scrub_only, "all_clean": bool((st == nxec.SCRUB_CLEAN).all())}))
        return
    e0, e1 = nxec.Event(), nxec.Event()

    def timed(fn):
        fn()  # warm
        e0.record(ctx.stream)
        for _ in range(a.reps):
            fn()
        e1.record(ctx.stream)
        ctx.sync()
        return e0.elapsed_ms(e1) / a.reps

    enc_ms, scrub_ms = [], []
    for _ in range(a.rounds):
        enc_ms.append(timed(enc))
        scrub_ms.append(timed(scrub))
    st = aux.download()[: ns * 4].view(np.int32)
    assert (st == nxec.SCRUB_CLEAN).all(), "the encoded batch is not clean"
    # worst case of the rare path: one chunk of every stripe corrupt (chunk 3 zeroed), detect + locate
    buf.memset2d(0, 3 * cs, ss, length, ns)
    aux.upload(np.zeros(1, dtype=np.uint64), cnt)
    e0.record(ctx.stream)
    scrub(nxec.SCRUB_LOCATE, aux.ptr + cnt)
    e1.record(ctx.stream)
    ctx.sync()
    locate_ms = e0.elapsed_ms(e1)
    raw = aux.download()
    st = raw[: ns * 4].view(np.int32)
    nbad = int(raw[cnt: cnt + 8].view(np.uint64)[0])
    assert (st == 3).all() and nbad == ns, (st[:8], nbad)
    total = n * length * ns
    med = lambda v: float(np.median(v))  # noqa: E731
    print(json.dumps({
        "shape": {"n": n, "k": k, "len": length, "nstripes": ns, "chunk_stride": cs, "stripe_stride": ss},
        "bytes": total, "rounds": a.rounds, "reps": a.reps,
        "encode_ms": [round(x, 4) for x in enc_ms], "scrub_ms": [round(x, 4) for x in scrub_ms],
        "encode_ms_median": round(med(enc_ms), 4), "scrub_ms_median": round(med(scrub_ms), 4),
        "scrub_over_encode": round(med(scrub_ms) / med(enc_ms), 4),
        "encode_tbps": round(total / med(enc_ms) / 1e9, 4), "scrub_tbps": round(total / med(scrub_ms) / 1e9, 4),
        "detect_locate_all_corrupt_ms": round(locate_ms, 3),
        "library_sha256_16": hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest()[:16],
    }))
    buf.free()
    aux.free()
    ctx.close()


if __name__ == "__main__":
    main()
