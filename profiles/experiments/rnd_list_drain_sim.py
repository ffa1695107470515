#!/usr/bin/env python3
"""Iterations of the wave-cooperative drain of the random-vector list (csrc/spira_device.h, drain_unit_sphere_list; docs/experiments.md §21).

A try is accepted with probability pi/6; whether try t of an entry is accepted is a pure function of (entry, t), drawn here once per list.
Three rules, 64 lanes:
  one    one lane per entry to the end: a lane keeps trying its entry, a finished lane claims the next unclaimed one (SPIRA_RND_TAIL=0)
  issue  the same until no unclaimed entry is left and p <= 32 are pending; then groups of g = the largest power of two with g*p <= 64 lanes
         per pending entry evaluate tries t0 .. t0+g-1 at once, re-formed every iteration
  built  what the kernel does: as `issue`, with g capped at 32 and groups re-formed only when g changes (re-forming with the same g gives no
         entry more tries, so the counts can differ only through the cap: a lone entry failing 32 tries in a row, 5e-11)
Every rule's result is checked against the serial definition (the lowest accepted try, or none up to MAXT).
usage: rnd_list_drain_sim.py [lists per length] [MAXT]"""
import math
import random
import sys

P = math.pi / 6
LENGTHS = (128, 100, 64, 32, 16, 8, 4, 1)


def serial(acc, maxt):
    return [next((t for t in range(1, maxt + 1) if a[t]), 0) for a in acc]


def drain(acc, maxt, rule):
    """acc[e][t]: try t of entry e accepted.  Returns (iterations, lane-tries evaluated, result per entry)."""
    n = len(acc)
    res = [None] * n
    lanes = [(e, 1) for e in range(min(n, 64))]          # (entry, next try) of the lanes that hold one
    nxt, iters, tries = 64, 0, 0
    while lanes and (rule == "one" or nxt < n or len(lanes) > 32):
        iters += 1
        tries += len(lanes)
        keep = []
        for e, t in lanes:
            if acc[e][t] or t == maxt:
                res[e] = t if acc[e][t] else 0
                if nxt < n:
                    keep.append((nxt, 1))
                    nxt += 1
            else:
                keep.append((e, t + 1))
        lanes = keep
    pend = lanes                                          # tail: (entry, t0)
    g = 0
    while pend:
        p = len(pend)
        g_new = 1 << int(math.log2(64 // p))
        if rule == "built":
            g_new = min(g_new, 32)
            if g_new != g:
                g, groups = g_new, list(pend)             # groups are formed again: the finished ones leave
        else:
            g, groups = g_new, list(pend)
        iters += 1
        out = []
        for grp in groups:
            if grp is None:
                out.append(None)
                continue
            e, t0 = grp
            span = [t for t in range(t0, t0 + g) if t <= maxt]
            tries += len(span)
            hit = next((t for t in span if acc[e][t]), 0)
            if hit or t0 + g > maxt:
                res[e] = hit
                out.append(None)
            else:
                out.append((e, t0 + g))
        groups = out
        pend = [x for x in groups if x is not None]
    return iters, tries, res


def main():
    lists = int(sys.argv[1]) if len(sys.argv) > 1 else 4000
    maxt = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    rng = random.Random(20261017)
    rows = {r: [] for r in ("one", "issue", "built")}
    util = {r: [] for r in rows}
    for n in LENGTHS:
        tot = {r: [0, 0] for r in rows}
        for _ in range(lists):
            acc = [[False] + [rng.random() < P for _ in range(maxt + 32)] for _ in range(n)]
            want = serial(acc, maxt)
            for r in rows:
                it, tr, res = drain(acc, maxt, r)
                assert res == want, (r, n)
                tot[r][0] += it
                tot[r][1] += tr
        for r in rows:
            rows[r].append(tot[r][0] / lists)
            util[r].append(tot[r][1] / (64.0 * tot[r][0]))
    print("| entries on the list | " + " | ".join(str(n) for n in LENGTHS) + " |")
    print("|---|" + "---:|" * len(LENGTHS))
    for r, label in (("one", "iterations, one lane per entry"), ("issue", "iterations, group tries re-formed every iteration"), ("built", "iterations, as built")):
        print("| %s | " % label + " | ".join("%.1f" % v for v in rows[r]) + " |")
    print("| lanes evaluating a try, one lane per entry | " + " | ".join("%.2f" % v for v in util["one"]) + " |")
    print("| lanes evaluating a try, as built | " + " | ".join("%.2f" % v for v in util["built"]) + " |")
    print("| ideal (n / (pi/6) / 64) | " + " | ".join("%.2f" % (n / P / 64) for n in LENGTHS) + " |")


if __name__ == "__main__":
    main()
