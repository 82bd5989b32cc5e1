#!/usr/bin/env python3
"""Cost of both-strand overlaps (SA_OPT_STRANDS) at the bench shape.

Times sa_device_build and sa_device_align on configs[1] (100k x 500 bp synthetic
reads, k = 15, bench.py's generator) with every read reverse-complemented by a seeded
coin, in three legs:

    parent_forward   another build of the library (--parent-lib, e.g. the parent
                     commit's libsa_overlap.so), option never set
    forward          this tree's library, SA_STRANDS_FORWARD
    both             this tree's library, SA_STRANDS_BOTH

Each leg is a fresh process (the library path is fixed at import); the legs alternate
over --passes passes so that drift of the shared host shows up as spread inside a leg
rather than as a difference between legs.  A leg warms up, then takes --repeats timed
repeats of --steps calls each: host clock around calls that end in a device
synchronise, ms per call.  Prints and (with --out) writes one JSON document with every
repeat, min / median / max per leg, the both / parent-forward ratios and the option-off
leg against the parent's own run-to-run spread (median difference in percent, whether
the two min..max ranges overlap, whether the median lies at or below the parent's max).
--resummarise FILE recomputes those derived fields from the repeats a document holds.

    python tools/strand_cost.py --parent-lib /path/to/parent/libsa_overlap.so \\
        --out profiles/strands/cost.json
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def flipped_workload(n_reads, read_len, coverage, gc, seed):
    sys.path.insert(0, ROOT)
    import bench
    genome_len = int(n_reads * read_len / coverage)
    bases, offsets = bench.synth_workload(n_reads, read_len, genome_len, gc, seed=seed)
    comp = np.arange(256, dtype=np.uint8)
    for a, b in zip(b"ACGT", b"TGCA"):
        comp[a] = b
    rows = bases.reshape(n_reads, read_len)
    flip = np.random.default_rng(seed + 100).integers(0, 2, size=n_reads).astype(bool)
    rows[flip] = comp[rows[flip][:, ::-1]]
    return rows.reshape(-1), offsets, int(flip.sum())


def leg(args):
    """One leg in this process: JSON on stdout."""
    sys.path.insert(0, os.path.join(ROOT, "sequence-aligner_amd"))
    import saoverlap as sao
    bases, offsets, n_flipped = flipped_workload(args.reads, args.len, args.coverage, args.gc, 1)
    ov = sao.Overlapper(kmer_size=args.k, id_mode=sao.SA_IDS_WIDE)
    if args.leg == "both":
        ov.set_strands(sao.STRANDS_BOTH)
    elif args.leg == "forward":
        ov.set_strands(sao.STRANDS_FORWARD)
    ov.add_packed(bases.tobytes(), offsets)

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        ov.sync()
        out = []
        for _ in range(args.repeats):
            ov.sync()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                fn()
            ov.sync()
            out.append((time.perf_counter() - t0) * 1e3 / args.steps)
        return out

    ov.device_build()  # allocations, outside every timed window
    ov.sync()
    build = timed(ov.device_build)
    ov.device_align()
    ov.sync()
    align = timed(ov.device_align)
    st = ov.stats()
    res = {"leg": args.leg, "lib": os.path.realpath(sao.LIB_PATH), "build_ms": build, "align_ms": align,
           "reads_flipped": n_flipped,
           "stats": {k: int(st[k]) for k in ("kmers", "pairs", "dispatched", "aligned", "dp_cells")}}
    ov.close()
    print("STRAND_COST " + json.dumps(res))


def summary(v):
    return {"repeats": [round(x, 4) for x in v], "min": round(min(v), 4), "median": round(float(np.median(v)), 4),
            "max": round(max(v), 4)}


def derive(doc):
    """The ratios and the option-off comparison from the legs' repeats."""
    legs = doc["legs"]
    what = ("device_build_ms", "device_align_ms")
    base = "parent_forward" if "parent_forward" in legs else "forward"
    for k in [k for k in doc if k.startswith(("ratios_both_over_", "option_off_"))]:
        del doc[k]
    doc["ratios_both_over_" + base] = {w: round(legs["both"][w]["median"] / legs[base][w]["median"], 3) for w in what}
    if base == "parent_forward":
        p, f = legs["parent_forward"], legs["forward"]
        doc["option_off_vs_parent"] = {
            w: {"median_difference_pct": round(100.0 * (f[w]["median"] / p[w]["median"] - 1.0), 2),
                "parent_spread_pct": round(100.0 * (p[w]["max"] / p[w]["min"] - 1.0), 2),
                "min_max_ranges_overlap": bool(f[w]["min"] <= p[w]["max"] and p[w]["min"] <= f[w]["max"]),
                "median_at_or_below_parent_max": bool(f[w]["median"] <= p[w]["max"])} for w in what}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resummarise", default=None, metavar="FILE",
                    help="recompute the derived fields of an existing document in place")
    ap.add_argument("--parent-lib", default=None, help="libsa_overlap.so of the commit to compare against")
    ap.add_argument("--out", default=None)
    ap.add_argument("--reads", type=int, default=100_000)
    ap.add_argument("--len", type=int, default=500)
    ap.add_argument("--k", type=int, default=15)
    ap.add_argument("--gc", type=float, default=0.50)
    ap.add_argument("--coverage", type=float, default=20.0)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5, help="timed repeats per leg and pass (>= 5 over the passes)")
    ap.add_argument("--steps", type=int, default=10, help="calls per timed repeat")
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--leg", default=None, choices=("parent_forward", "forward", "both"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.leg:
        return leg(args)
    if args.resummarise:
        doc = json.load(open(args.resummarise))
        derive(doc)
        open(args.resummarise, "w").write(json.dumps(doc, indent=1) + "\n")
        return print(json.dumps(doc, indent=1))
    legs = (["parent_forward"] if args.parent_lib else []) + ["forward", "both"]
    acc = {name: {"build_ms": [], "align_ms": []} for name in legs}
    info = {}
    for _ in range(args.passes):
        for name in legs:
            env = dict(os.environ)
            env.pop("SA_OVERLAP_LIB", None)
            if name == "parent_forward":
                env["SA_OVERLAP_LIB"] = args.parent_lib
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", name] + [
                "--%s=%s" % (k, getattr(args, k)) for k in ("reads", "len", "k", "gc", "coverage", "warmup",
                                                              "repeats", "steps")]
            p = subprocess.run(cmd, env=env, capture_output=True, text=True)
            line = [x for x in p.stdout.splitlines() if x.startswith("STRAND_COST ")]
            if p.returncode or not line:
                sys.stderr.write(p.stdout + p.stderr)
                raise SystemExit("leg %s failed (%d)" % (name, p.returncode))
            r = json.loads(line[0][len("STRAND_COST "):])
            acc[name]["build_ms"] += r["build_ms"]
            acc[name]["align_ms"] += r["align_ms"]
            info[name] = {"stats": r["stats"], "lib": os.path.basename(os.path.dirname(r["lib"]))}
            flipped = r["reads_flipped"]
            sys.stderr.write("%s: build %s align %s\n" % (name, r["build_ms"], r["align_ms"]))
    doc = {"workload": "configs[1]: %d x %d bp synthetic reads, k=%d, %.0fx coverage, %d reads reverse-complemented "
                       "(seeded coin)" % (args.reads, args.len, args.k, args.coverage, flipped),
           "method": "host clock around %d calls ending in a device synchronise, ms per call; %d warm-up calls, "
                     "%d repeats per pass, %d alternating passes, one fresh process per leg and pass"
                     % (args.steps, args.warmup, args.repeats, args.passes),
           "legs": {name: {"device_build_ms": summary(acc[name]["build_ms"]),
                           "device_align_ms": summary(acc[name]["align_ms"]), **info[name]} for name in legs}}
    derive(doc)
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
