"""Multi-hit ray queries, traversal alone (docs/experiments.md, "Multi-hit ray queries"): the 81 920-triangle mesh of scenes.scene_s4(level=6), about 2 M rays
per set — the three ray sets of profiles/cast_bench.py — one precision per run, device tensors in and out, timed with events around one call.
Per set, Grays/s (rays of the list per second, median of the timed calls after the warm-up, the variants alternating call by call):
  cast              spira_scene_cast_device_* (prim and t), sessions and in place: the closest hit, the comparison point of K = 1
  K = 1, 4, 16      spira_scene_cast_hits_device_* (prim, t, count), sessions and in place
  count all         max_hits = 0 with SPIRA_HITS_COUNT_ALL (count only), sessions and in place
  K x cast          the alternative a caller had: K successive cast_device calls, t_min moved one ulp past the previous hit in between (torch.nextafter on
                    the device, inside the timed region: it is part of that route).  It drops tied hits, so it is an upper bound on the alternative's
                    usefulness, not an equal; the fraction of rays whose K hits agree with the multi-hit answer is printed beside it.
`cast` is listed twice ("cast" and "cast again"): the distance between its two medians is the run-to-run spread a comparison has to beat.
Asserted: sessions and in place give the same bytes; K = 1 gives cast's bytes.  Needs a GPU; no oracle.  Trips per ray are not reported: the entry has
no trip counter.

    python profiles/hits_bench.py --prec f32 [--out table.md] [--repeats 7] [--warmup 2] [--level 6]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "julia-spira_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def measure(a):
    import torch
    from spira_hip import _binding as B
    from spira_hip import query, scenes
    from cast_bench import ray_sets
    assert B.device_count() >= 1, "no HIP device: this is a GPU measurement"
    B.set_device(0)
    s = scenes.scene_s4(level=a.level)
    sets = ray_sets(s, scenes.scene_s5(level=0)["camera12"], 1 << 21, 1920, 1080)
    st = torch.cuda.current_stream()
    prec = a.prec
    npdt = np.float32 if prec == "f32" else np.float64
    tdt = torch.float32 if prec == "f32" else torch.float64
    inf = torch.tensor(float("inf"), dtype=tdt, device="cuda:0")

    def successive(h, d_rays, K):
        """K closest-hit calls with t_min advanced past the previous hit; a ray that missed keeps missing (t_min = t_max)."""
        r = d_rays.clone()
        prims, ts = [], []
        for _ in range(K):
            prim, t, _ = query.cast_rays(h, r, stream=st)
            prims.append(prim); ts.append(t)
            r[:, 3] = torch.where(prim >= 0, torch.nextafter(t, inf), r[:, 7])
        return torch.stack(prims, dim=1), torch.stack(ts, dim=1)

    rows = []
    with B.Scene(np.ascontiguousarray(s["spheres5"], dtype=npdt), np.ascontiguousarray(s["materials8"], dtype=npdt), np.ascontiguousarray(s["triangles10"], dtype=npdt), prec) as h:
        for name in a.sets.split(","):
            d_rays = torch.tensor(np.ascontiguousarray(sets[name], dtype=npdt), device="cuda:0")
            n = d_rays.shape[0]
            variants = [("cast", lambda ip: query.cast_rays(h, d_rays, inplace=ip, stream=st)[:2])]
            for K in (1, 4, 16):
                variants.append(("K = %d" % K, lambda ip, K=K: query.cast_all(h, d_rays, K, inplace=ip, stream=st)))
            variants.append(("count all", lambda ip: (query.count_hits(h, d_rays, inplace=ip, stream=st),)))
            variants.append(("cast again", variants[0][1]))
            ms = {(v[0], ip): [] for v in variants for ip in (False, True)}
            first = {}
            for i in range(a.warmup + a.repeats):
                for vname, fn in variants:
                    for ip in (False, True):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(st)
                        out = fn(ip)
                        e1.record(st)
                        e1.synchronize()
                        if i == 0:
                            first[(vname, ip)] = [o.cpu().numpy() for o in out]
                        if i >= a.warmup:
                            ms[(vname, ip)].append(e0.elapsed_time(e1))
                        del out
            for vname, _ in variants:
                assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(first[(vname, False)], first[(vname, True)])), (name, vname)
            assert np.array_equal(first[("K = 1", False)][0][:, 0], first[("cast", False)][0]) and np.array_equal(first[("K = 1", False)][1][:, 0].view(np.uint8), first[("cast", False)][1].view(np.uint8))
            succ = {}
            for K in (4, 16):
                t_ms = []
                for i in range(1 + max(2, a.repeats // 3)):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(st)
                    sp, stt = successive(h, d_rays, K)
                    e1.record(st)
                    e1.synchronize()
                    if i > 0:
                        t_ms.append(e0.elapsed_time(e1))
                agree = float((sp.cpu().numpy() == first[("K = %d" % K, False)][0]).all(axis=1).mean())
                succ[K] = (float(np.median(t_ms)), agree)
                del sp, stt
            cnt = first[("count all", False)][0]
            row = dict(prec=prec, set=name, rays=n, mean_candidates=float(cnt.mean()), max_candidates=int(cnt.max()), more_than_16=float((cnt > 16).mean()))
            for (vname, ip), v in ms.items():
                row["grays %s %s" % (vname, "in place" if ip else "sessions")] = n / (float(np.median(v)) * 1e6)
            for K, (m, agree) in succ.items():
                row["grays %d x cast" % K] = n / (m * 1e6)
                row["agree %d x cast" % K] = agree
            rows.append(row)
            print(json.dumps(row), flush=True)
            del d_rays
    return rows, B.build_id()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prec", default="f32", choices=["f32", "f64"])
    ap.add_argument("--sets", default="camera,incoherent,occlusion")
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--level", type=int, default=6)
    a = ap.parse_args()
    rows, build = measure(a)
    cols = ["cast", "cast again", "K = 1", "K = 4", "K = 16", "count all"]
    lines = ["build id " + build, "", "Grays/s, sessions / in place", "", "| precision | set | candidates mean / max | " + " | ".join(cols) + " | 4 x cast (agree) | 16 x cast (agree) |",
             "|---|---|---|" + "---|" * (len(cols) + 2)]
    for r in rows:
        cells = ["%.3f / %.3f" % (r["grays %s sessions" % c], r["grays %s in place" % c]) for c in cols]
        cells += ["%.3f (%.1f %%)" % (r["grays %d x cast" % K], 100 * r["agree %d x cast" % K]) for K in (4, 16)]
        lines.append("| %s | %s | %.2f / %d | " % (r["prec"], r["set"], r["mean_candidates"], r["max_candidates"]) + " | ".join(cells) + " |")
    table = "\n".join(lines)
    print(table)
    if a.out:
        with open(a.out, "w") as f:
            f.write(table + "\n")


if __name__ == "__main__":
    main()
