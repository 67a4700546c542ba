#!/usr/bin/env python3
"""Rate of the mixed-pattern decode (nxec_rs_decode_stripes_mixed) against the
single-pattern call on RS(10,4) = (n,k) (14,10), 1 MiB chunks, 4096 stripes,
packed; event-timed on the context stream, every leg warmed up, legs
interleaved over --rounds rounds of --reps calls in one process:
  A  nxec_rs_decode_stripes, chunk 0 erased in every stripe
  B  the mixed call, every stripe that pattern
  C  the mixed call, erased id s % 14
  D  a degraded read: nine stripes in ten clean, the rest one erased chunk rotating
  E  C without the call: one nxec_rs_decode_stripes per run of equal patterns
     (here every stripe), over the first 512 stripes
Bytes of a leg: 2 * k * len per decoded stripe.

Before any timing every leg's output is checked against the truth: the erased
chunks of the source are overwritten, the output is zeroed, the leg runs, and
the output's checksum must be that of the original data chunks; the source is
then healed with the mixed recover and its checksum compared too.

Yardsticks: B takes at most A's time plus the rounds' spread plus 3 %; D is no
slower than B.  One JSON document on stdout, or in --out."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from nexoedge_amd import nxec  # noqa: E402

n, k, cs = 14, 10, 1 << 20


def summary(ms, nbytes):
    gbps = [nbytes / m / 1e6 for m in ms]
    med = float(np.median(gbps))
    return {"ms": [round(m, 4) for m in ms], "ms_median": round(float(np.median(ms)), 4),
            "gbps": [round(g, 1) for g in gbps], "gbps_median": round(med, 1), "frac8T": round(med / 8e3, 4),
            "spread": round((max(gbps) - min(gbps)) / med, 4), "bytes": nbytes}


def run(args):
    stripes = args.stripes
    ctx = nxec.Context(0)
    st = ctx.stream
    src = nxec.DeviceBuffer(stripes * n * cs)
    out = nxec.DeviceBuffer(stripes * k * cs)
    src.fill_random(5)
    ctx.rs_encode(n, k, src.ptr, cs, n * cs, cs, stripes, st)
    ctx.sync()
    few = min(512, stripes)
    idx = np.arange(stripes)
    clean = np.ones((stripes, n), dtype=np.uint8)
    one = clean.copy()
    one[:, 0] = 0
    rot = clean.copy()
    rot[idx, idx % n] = 0
    deg = clean.copy()
    hit = idx[idx % 10 == 9]
    deg[hit, (hit // 10) % n] = 0

    def leg_e():
        for s in range(few):
            ctx.rs_decode(n, k, [s % n], src.ptr + s * n * cs, cs, n * cs, out.ptr + s * k * cs, cs, k * cs, cs, 1, st)

    def mixed(alive):
        return lambda: ctx.rs_decode_mixed(n, k, alive, src.ptr, cs, n * cs, out.ptr, cs, k * cs, cs, stripes, st)

    # leg: (call, its alive map, stripes it decodes)
    legs = {"A": (lambda: ctx.rs_decode(n, k, [0], src.ptr, cs, n * cs, out.ptr, cs, k * cs, cs, stripes, st), one, stripes),
            "B": (mixed(one), one, stripes), "C": (mixed(rot), rot, stripes), "D": (mixed(deg), deg, stripes),
            "E": (leg_e, rot, few)}

    # the truth: the data chunks themselves, packed (a decode with nothing erased is k copies per stripe)
    src_sum = src.checksum(stream=st)
    ctx.rs_decode(n, k, [], src.ptr, cs, n * cs, out.ptr, cs, k * cs, cs, stripes, st)
    truth = {stripes: out.checksum(stream=st), few: out.checksum(few * k * cs, stream=st)}
    nxec.launch_log(True)
    launches = {}
    for name, (go, alive, count) in legs.items():
        # check: garbage in the erased chunks, a zeroed output, then the leg
        for s, c in zip(*np.nonzero(alive[:count] == 0)):
            src.memset2d(0xEE, (int(s) * n + int(c)) * cs, cs, cs, 1, st)
        out.memset(0, stream=st)
        nxec.launch_log_read()
        go()
        ctx.sync()
        recs = nxec.launch_log_read()
        got = out.checksum(count * k * cs, stream=st)
        if got != truth[count]:
            raise SystemExit(f"leg {name}: the output's checksum {got:#x} is not the data chunks' {truth[count]:#x}")
        launches[name] = {"launches": len(recs), "families": sorted({r["family"] for r in recs})}
        if recs and recs[0]["family"] == "k_decode_mixed":
            launches[name].update(segs=recs[0]["segs"], stripes=recs[0]["stripes"], grid=recs[0]["grid"], tpg=recs[0]["tpg"])
        heal = clean.copy()
        heal[:count] = alive[:count]
        ctx.rs_recover_mixed(n, k, heal, src.ptr, cs, n * cs, cs, stripes, st)
        if src.checksum(stream=st) != src_sum:
            raise SystemExit(f"leg {name}: the source was not healed")
        for _ in range(4):  # warm-up; the mixed call's table staging grows to its slots here, not in a timed round
            go()
        ctx.sync()
    nxec.launch_log(False)
    ms = {name: [] for name in legs}
    for _ in range(args.rounds):
        for name, (go, _, _) in legs.items():
            e0, e1 = nxec.Event(), nxec.Event()
            e0.record(st)
            for _ in range(args.reps):
                go()
            e1.record(st)
            ctx.sync()
            ms[name].append(e0.elapsed_ms(e1) / args.reps)
    L = {name: dict(summary(ms[name], 2 * k * cs * legs[name][2]), **launches[name]) for name in legs}
    allowance = round(max(L["A"]["spread"], L["B"]["spread"]) + 0.03, 4)
    b_over_a = round(L["B"]["ms_median"] / L["A"]["ms_median"], 4)
    d_over_b = round(L["D"]["ms_median"] / L["B"]["ms_median"], 4)
    doc = {"shape": {"n": n, "k": k, "len": cs, "stripes": stripes, "rounds": args.rounds, "reps": args.reps,
                     "layout": "packed"},
           "legs": L,
           "yardsticks": {"B_time_over_A": b_over_a, "B_allowance": allowance, "B_within_allowance": b_over_a <= 1 + allowance,
                          "D_time_over_B": d_over_b, "D_no_slower_than_B": d_over_b <= 1.0,
                          "C_over_E": round(L["C"]["gbps_median"] / L["E"]["gbps_median"], 2)}}
    src.free()
    out.free()
    ctx.close()
    return doc


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--stripes", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", help="write the JSON document here instead of stdout")
    args = ap.parse_args()
    doc = json.dumps(run(args), indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(doc + "\n")
    else:
        print(doc)


if __name__ == "__main__":
    main()
