#!/usr/bin/env python3
"""Delta update (nxec_rs_update_stripes) against what a caller had before it,
RS(10,4) (n = 14, k = 10) x 4096 stripes x 1 MiB chunks, one update per stripe
at a random data chunk and a random 16-byte-aligned offset, update lengths
4 KiB, 64 KiB and 1 MiB.

Legs, interleaved over --rounds rounds in one process, every shape warmed up:
  update    one nxec_rs_update_stripes over the list
  reencode  one device-to-device copy of the new bytes into place per update,
            then nxec_rs_encode_stripes over the batch
Both are event-timed on the context's stream (the copies' and the planner's
host time is inside where the device waits for it) and wall-clocked around a
synchronise.  The new bytes alternate between two buffers so that new ^ old is
never zero.  Algorithmic bytes of the update: (2 (n-k) + 3) x length per update
(old and new data and the parity read, data and parity written).

Before timing, each length checks at full size that the update leaves the batch
byte for byte as the re-encode does (checksums of the whole batch).

One JSON document on stdout, or in --out."""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from nexoedge_amd import _lib, nxec  # noqa: E402

n, k, cs = 14, 10, 1 << 20
LENGTHS = [4 << 10, 64 << 10, 1 << 20]
HBM = 8e12  # bytes/s


def median(xs):
    return float(np.median(xs))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--stripes", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", help="write the JSON document here instead of stdout")
    args = ap.parse_args()
    ns, ss = args.stripes, n * cs
    if nxec.device_count() == 0:
        raise SystemExit("no HIP device: nothing is measured without one")
    ctx = nxec.Context(0)
    st = ctx.stream
    buf = nxec.DeviceBuffer(ns * ss)
    buf.fill_random(5)
    ctx.rs_encode(n, k, buf.ptr, cs, ss, cs, ns, st)
    ctx.sync()
    rng = np.random.default_rng(23)
    lib, cp = _lib.lib, C.c_void_p(ctx.ptr)
    out = {"shape": {"n": n, "k": k, "len": cs, "stripes": ns, "rounds": args.rounds, "reps": args.reps}, "lengths": {}}
    for length in LENGTHS:
        chunk = rng.integers(0, k, ns)
        off = rng.integers(0, (cs - length) // 16 + 1, ns) * 16
        new = [nxec.DeviceBuffer(ns * length) for _ in range(2)]
        for i, b in enumerate(new):
            b.fill_random(100 + i)
        lists = [nxec._update_list([(s, int(chunk[s]), int(off[s]), length, b.ptr + s * length) for s in range(ns)])[0]
                 for b in new]
        dst = [buf.ptr + s * ss + int(chunk[s]) * cs + int(off[s]) for s in range(ns)]
        turn = [0]

        def update():
            _lib.check(lib.nxec_rs_update_stripes(cp, n, k, C.c_void_p(buf.ptr), cs, ss, cs, ns, lists[turn[0] & 1], ns, st),
                       "nxec_rs_update_stripes")
            turn[0] += 1

        def reencode():
            src = new[turn[0] & 1].ptr
            for s in range(ns):
                lib.nxec_memcpy_d2d(C.c_void_p(dst[s]), C.c_void_p(src + s * length), length, st)
            ctx.rs_encode(n, k, buf.ptr, cs, ss, cs, ns, st)
            turn[0] += 1

        # same result: the update, then the re-encode with the same new bytes, leave the same batch
        nxec.launch_log(True)
        nxec.launch_log_read()
        update()
        ctx.sync()
        recs = nxec.launch_log_read()
        nxec.launch_log(False)
        sum_update = buf.checksum(stream=st)
        turn[0] -= 1
        reencode()
        ctx.sync()
        if buf.checksum(stream=st) != sum_update:
            raise SystemExit(f"length {length}: the update and the re-encode disagree")
        legs = {"update": update, "reencode": reencode}
        for go in legs.values():  # warm-up; the update's table staging grows to its slots here
            for _ in range(4):
                go()
            ctx.sync()
        ms = {name: [] for name in legs}
        wall = {name: [] for name in legs}
        for _ in range(args.rounds):
            for name, go in legs.items():
                e0, e1 = nxec.Event(), nxec.Event()
                ctx.sync()
                t0 = time.perf_counter()
                e0.record(st)
                for _ in range(args.reps):
                    go()
                e1.record(st)
                ctx.sync()
                wall[name].append((time.perf_counter() - t0) * 1e3 / args.reps)
                ms[name].append(e0.elapsed_ms(e1) / args.reps)
        nbytes = (2 * (n - k) + 3) * length * ns
        um, rm = median(ms["update"]), median(ms["reencode"])
        out["lengths"][str(length)] = {
            "update_ms": [round(x, 4) for x in ms["update"]], "update_ms_median": round(um, 4),
            "update_wall_ms_median": round(median(wall["update"]), 4),
            "reencode_ms": [round(x, 4) for x in ms["reencode"]], "reencode_ms_median": round(rm, 4),
            "reencode_wall_ms_median": round(median(wall["reencode"]), 4),
            "algorithmic_bytes": nbytes, "update_gbps": round(nbytes / um / 1e6, 1),
            "frac8T": round(nbytes / (um * 1e-3) / HBM, 4), "reencode_over_update": round(rm / um, 2),
            "launches": [{key: r[key] for key in ("family", "rows", "grid", "pass", "last") if key in r} for r in recs],
        }
        for b in new:
            b.free()
    # the update length from which the full re-encode is the cheaper of the two: log-linear between the
    # measured lengths around the first one where it is
    cross, prev = None, None
    for length in LENGTHS:
        r = out["lengths"][str(length)]
        d = r["update_ms_median"] - r["reencode_ms_median"]
        if d >= 0:
            cross = length if prev is None else int(round(np.exp(np.log(prev[0]) + (np.log(length) - np.log(prev[0])) *
                                                                  (-prev[1]) / (d - prev[1]))))
            break
        prev = (length, d)
    out["reencode_cheaper_from_length"] = cross  # None: the update is the cheaper one at every measured length
    buf.free()
    ctx.close()
    doc = json.dumps(out, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(doc + "\n")
    else:
        print(doc)


if __name__ == "__main__":
    main()
