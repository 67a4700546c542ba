#!/usr/bin/env python3
"""Per-erasure-pattern timing of the RS(10,4) recover launch (4096 x 1 MiB),
event-timed on the context stream; encode for reference.

--mixed: the mixed-pattern recover (nxec_rs_recover_stripes_mixed) on the same
batch against the single-pattern call, legs interleaved over --rounds rounds in
one process, every shape warmed up first:
  A      nxec_rs_recover_stripes, chunk 0 erased in every stripe
  A_lds  the same with single-row passes on the LDS tables (NXEC_ALGO=lds), in a
         child process on a design-probe build of the library (--probe-lib)
  B      the mixed call, every stripe the same single pattern
  C      the mixed call, erased id s % 14
  D      the mixed call, seeded random 1-4 erasures per stripe
  E      what a caller does without it for C: one nxec_rs_recover_stripes per
         stripe, over the first 512 stripes
Bytes of a leg: sum over its coded stripes of (k + erased) * len.  One JSON
document on stdout, or in --out."""
import argparse
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from nexoedge_amd import nxec  # noqa: E402

n, k, cs, ns = 14, 10, 1 << 20, 4096


def patterns():
    ctx = nxec.Context(0)
    st = ctx.stream
    buf = nxec.DeviceBuffer(ns * n * cs)
    buf.fill_random(5)
    ctx.rs_encode(n, k, buf.ptr, cs, n * cs, cs, ns, st)
    ctx.sync()
    pats = {"encode": None, "data0-3": [0, 1, 2, 3], "parity10-13": [10, 11, 12, 13], "mixed1,4,11,13": [1, 4, 11, 13],
            "data6-9": [6, 7, 8, 9], "one0": [0], "two0,13": [0, 13],
            "0,2,4,6": [0, 2, 4, 6], "1,2,3,4": [1, 2, 3, 4], "0,1,12,13": [0, 1, 12, 13], "4,5,6,7": [4, 5, 6, 7],
            "1,4,11,13 again": [1, 4, 11, 13], "0,5,10,13": [0, 5, 10, 13], "2,3,11,12": [2, 3, 11, 12]}
    for name, f in pats.items():
        def go():
            if f is None:
                ctx.rs_encode(n, k, buf.ptr, cs, n * cs, cs, ns, st)
            else:
                ctx.rs_recover(n, k, f, buf.ptr, cs, n * cs, cs, ns, st)
        go()
        e0, e1 = nxec.Event(), nxec.Event()
        e0.record(st)
        for _ in range(5):
            go()
        e1.record(st)
        ctx.sync()
        ms = e0.elapsed_ms(e1) / 5
        e = k + (n - k if f is None else len(f))
        b = ns * e * cs
        print(f"{name:16s} {ms:7.3f} ms  {b / ms / 1e6:8.1f} GB/s  frac8T {b / ms / 1e6 / 8e3:.3f}", flush=True)
    buf.free()
    ctx.close()


def summary(ms, nbytes):
    gbps = [nbytes / m / 1e6 for m in ms]
    med = float(np.median(gbps))
    return {"ms": [round(m, 4) for m in ms], "gbps": [round(g, 1) for g in gbps], "gbps_median": round(med, 1),
            "frac8T": round(med / 8e3, 4), "spread": round((max(gbps) - min(gbps)) / med, 4), "bytes": nbytes}


def mixed(args):
    stripes = args.stripes
    ctx = nxec.Context(0)
    st = ctx.stream
    buf = nxec.DeviceBuffer(stripes * n * cs)
    buf.fill_random(5)
    ctx.rs_encode(n, k, buf.ptr, cs, n * cs, cs, stripes, st)
    ctx.sync()
    rng = np.random.default_rng(17)
    one = np.ones((stripes, n), dtype=np.uint8)
    one[:, 0] = 0
    rot = np.ones((stripes, n), dtype=np.uint8)
    rot[np.arange(stripes), np.arange(stripes) % n] = 0
    rnd = np.ones((stripes, n), dtype=np.uint8)
    for s in range(stripes):
        rnd[s, rng.choice(n, size=rng.integers(1, 5), replace=False)] = 0
    few = min(512, stripes)

    def leg_e():
        for s in range(few):
            ctx.rs_recover(n, k, [s % n], buf.ptr + s * n * cs, cs, n * cs, cs, 1, st)

    def coded_bytes(alive, count):
        return int(((alive[:count] == 0).sum(axis=1) + k).sum()) * cs

    legs = {"A": (lambda: ctx.rs_recover(n, k, [0], buf.ptr, cs, n * cs, cs, stripes, st), coded_bytes(one, stripes))}
    if not args.leg_a_only:
        legs["B"] = (lambda: ctx.rs_recover_mixed(n, k, one, buf.ptr, cs, n * cs, cs, stripes, st), coded_bytes(one, stripes))
        legs["C"] = (lambda: ctx.rs_recover_mixed(n, k, rot, buf.ptr, cs, n * cs, cs, stripes, st), coded_bytes(rot, stripes))
        legs["D"] = (lambda: ctx.rs_recover_mixed(n, k, rnd, buf.ptr, cs, n * cs, cs, stripes, st), coded_bytes(rnd, stripes))
        legs["E"] = (leg_e, coded_bytes(rot, few))
    nxec.launch_log(True)
    launches = {}
    for name, (go, _) in legs.items():  # warm-up, and which kernels each leg runs
        nxec.launch_log_read()
        go()
        ctx.sync()
        recs = nxec.launch_log_read()
        launches[name] = {"launches": len(recs), "families": sorted({r["family"] for r in recs})}
        for _ in range(4):  # the mixed call's table staging grows to its four slots here, not in a timed round
            go()
        ctx.sync()
        nxec.launch_log_read()
        if recs and recs[0]["family"] == "k_mul_mixed":
            launches[name].update(segs=recs[0]["segs"], stripes=recs[0]["stripes"], grid=recs[0]["grid"])
    nxec.launch_log(False)
    ms = {name: [] for name in legs}
    for _ in range(args.rounds):
        for name, (go, _) in legs.items():
            e0, e1 = nxec.Event(), nxec.Event()
            e0.record(st)
            for _ in range(args.reps):
                go()
            e1.record(st)
            ctx.sync()
            ms[name].append(e0.elapsed_ms(e1) / args.reps)
    out = {"shape": {"n": n, "k": k, "len": cs, "stripes": stripes, "rounds": args.rounds, "reps": args.reps},
           "legs": {name: dict(summary(ms[name], legs[name][1]), **launches[name]) for name in legs}}
    buf.free()
    ctx.close()
    if args.leg_a_only:
        return out
    if args.probe_lib:
        env = dict(os.environ, NXEC_LIB=os.path.abspath(args.probe_lib), NXEC_ALGO="lds")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--mixed", "--leg-a-only", "--stripes", str(stripes),
                            "--rounds", str(args.rounds), "--reps", str(args.reps)], capture_output=True, text=True, env=env)
        if r.returncode != 0:
            raise SystemExit(f"the probe-build child failed ({r.returncode}):\n{r.stdout}\n{r.stderr}")
        out["legs"]["A_lds"] = json.loads(r.stdout)["legs"]["A"]
    L = out["legs"]
    ref = "A_lds" if "A_lds" in L else "A"
    out["yardsticks"] = {
        "B_over_" + ref: round(L["B"]["gbps_median"] / L[ref]["gbps_median"], 4),
        "B_allowance": round(max(L["B"]["spread"], L[ref]["spread"]) + 0.03, 4),
        "C_over_B": round(L["C"]["gbps_median"] / L["B"]["gbps_median"], 4),
        "D_over_B": round(L["D"]["gbps_median"] / L["B"]["gbps_median"], 4),
        "C_over_E": round(L["C"]["gbps_median"] / L["E"]["gbps_median"], 2),
    }
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mixed", action="store_true", help="time the mixed-pattern recover against the single-pattern call")
    ap.add_argument("--stripes", type=int, default=ns)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--probe-lib", help="a `make PROBES=1` build of libnxec.so for leg A_lds")
    ap.add_argument("--leg-a-only", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", help="write the JSON document here instead of stdout")
    args = ap.parse_args()
    if not args.mixed:
        return patterns()
    doc = json.dumps(mixed(args), indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(doc + "\n")
    else:
        print(doc)


if __name__ == "__main__":
    main()
