"""K-nearest point queries on a scene handle (docs/experiments.md, "K-nearest point queries"): the 81 920-triangle mesh of scenes.scene_s4(), both
precisions, 2^21 points per set, device tensors in and out (spira_scene_nearest_k_device_*, outputs allocated once), timed with events around one call.
Point sets: profiles/nearest_bench.py's — surface (within 1 % of the extent of the mesh), box (the mesh's box grown by 1.5), far (10 extents away).
Legs, each as the refilled sessions and as SPIRA_CAST_INPLACE:
  closest   spira_scene_closest_point_device_* of the same build on the same set: the yardstick of K = 1
  K = 1, 4, 16 with r_max = +Inf: prim, dist, point and count written
  count     SPIRA_NEAR_COUNT_ALL with max_near = 0 and r_max = 1 % of the extent: the count alone
The legs alternate inside one process, call by call; the figure is the median of the timed calls after the warm-up.  Per leg: Gqueries/s and the mean
out_trips of a point (taken on the first call).  "K = 1 / closest" is the ratio of the two Gqueries/s.  Nothing is asserted except that both organisations
of a leg give the same bytes and that K = 1 gives closest point's.  Needs a GPU; no oracle.

    python profiles/knearest_bench.py [--out table.md] [--repeats 9] [--warmup 2] [--level 6] [--log2n 21]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "julia-spira_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

LEGS = [("closest", None), ("K = 1", 1), ("K = 4", 4), ("K = 16", 16), ("count", 0)]
# where K = 16 spends its time: the same walk and list with fewer outputs (--attribute)
ATTRIBUTE = [("K = 16", 16), ("K = 16, no point", -16), ("K = 16, count alone", -1016), ("K = 4", 4), ("K = 4, count alone", -1004)]


def measure(a):
    import torch
    from spira_hip import _binding as B
    from spira_hip import scenes
    from nearest_bench import point_sets
    assert B.device_count() >= 1, "no HIP device: this is a GPU measurement"
    B.set_device(0)
    s = scenes.scene_s4(level=a.level)
    n = 1 << a.log2n
    sets = point_sets(s, n)
    v = np.asarray(s["triangles10"], dtype=np.float64)[:, :9].reshape(-1, 3)
    radius = 0.01 * float((v.max(axis=0) - v.min(axis=0)).max())
    st = torch.cuda.current_stream()
    rows = []
    legs = ATTRIBUTE if a.attribute else LEGS
    for prec in ("f32", "f64"):
        npdt, tdt = (np.float32, torch.float32) if prec == "f32" else (np.float64, torch.float64)
        sph, mats, tri = (np.ascontiguousarray(s[k], dtype=npdt) for k in ("spheres5", "materials8", "triangles10"))
        prim = torch.empty((n, 16), dtype=torch.int32, device="cuda:0")
        dist = torch.empty((n, 16), dtype=tdt, device="cuda:0")
        point = torch.empty((n, 16, 3), dtype=tdt, device="cuda:0")
        count = torch.empty(n, dtype=torch.int32, device="cuda:0")
        trips = torch.empty(n, dtype=torch.int32, device="cuda:0")
        with B.Scene(sph, mats, tri, prec) as h:
            for name, pts in sets.items():
                d_inf = torch.tensor(np.ascontiguousarray(pts, dtype=npdt), device="cuda:0")
                d_r = d_inf.clone()
                d_r[:, 3] = radius

                def call(K, inplace, want_trips):
                    tp = trips.data_ptr() if want_trips else 0
                    if K is None:
                        h.closest_point_device(d_inf.data_ptr(), n, prim.data_ptr(), dist.data_ptr(), point.data_ptr(), st.cuda_stream, inplace=inplace, d_trips_ptr=tp)
                    elif K < 0:      # --attribute: K = -K without the points, K = -(1000 + K) with the count alone
                        k, lists = (-K - 1000, False) if K <= -1000 else (-K, True)
                        h.nearest_k_device(d_inf.data_ptr(), n, k, prim.data_ptr() if lists else 0, dist.data_ptr() if lists else 0, 0, count.data_ptr(), st.cuda_stream,
                                           inplace=inplace, d_trips_ptr=tp)
                    elif K == 0:
                        h.nearest_k_device(d_r.data_ptr(), n, 0, 0, 0, 0, count.data_ptr(), st.cuda_stream, inplace=inplace, count_all=True, d_trips_ptr=tp)
                    else:
                        h.nearest_k_device(d_inf.data_ptr(), n, K, prim.data_ptr(), dist.data_ptr(), point.data_ptr(), count.data_ptr(), st.cuda_stream,
                                           inplace=inplace, d_trips_ptr=tp)

                def answer(K):
                    k = 1 if K is None else K
                    if k < 0:
                        return [count.cpu().numpy().copy()]
                    return [x.view(-1)[:n * k * w].cpu().numpy().copy() for x, w in ((prim, 1), (dist, 1), (point, 3))] if k else [count.cpu().numpy().copy()]
                ms = {(leg, ip): [] for leg, _ in legs for ip in (False, True)}
                mean_trips, first = {}, {}
                for i in range(a.warmup + a.repeats):
                    for leg, K in legs:
                        for ip in (False, True):
                            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            e0.record(st)
                            call(K, ip, i == 0)
                            e1.record(st)
                            e1.synchronize()
                            if i == 0:
                                got = answer(K)
                                if not ip:
                                    first[leg] = got
                                    mean_trips[leg] = float(trips.cpu().numpy().astype(np.float64).mean())
                                assert all(np.array_equal(x, y) for x, y in zip(first[leg], got)), (leg, "the two organisations differ")
                            if i >= a.warmup:
                                ms[(leg, ip)].append(e0.elapsed_time(e1))
                if a.attribute:
                    row = dict(prec=prec, set=name, points=n, trips={leg: mean_trips[leg] for leg, _ in legs},
                               sessions={leg: n / (float(np.median(ms[(leg, False)])) * 1e6) for leg, _ in legs},
                               in_place={leg: n / (float(np.median(ms[(leg, True)])) * 1e6) for leg, _ in legs})
                    rows.append(row)
                    print(json.dumps(row), flush=True)
                    continue
                assert all(np.array_equal(x, y) for x, y in zip(first["closest"], first["K = 1"])), "K = 1 is not closest point"
                gq = {k: n / (float(np.median(t)) * 1e6) for k, t in ms.items()}
                row = dict(prec=prec, set=name, points=n, within=float(first["count"][0].astype(np.float64).mean()),
                           trips={leg: mean_trips[leg] for leg, _ in legs}, sessions={leg: gq[(leg, False)] for leg, _ in legs},
                           in_place={leg: gq[(leg, True)] for leg, _ in legs},
                           spread={leg: [float(np.min(ms[(leg, False)])), float(np.max(ms[(leg, False)]))] for leg, _ in legs})
                rows.append(row)
                print(json.dumps(row), flush=True)
    return rows, B.build_id()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--log2n", type=int, default=21)
    ap.add_argument("--attribute", action="store_true", help="K = 16 and K = 4 with fewer outputs instead of the table: what the stores and the points cost")
    a = ap.parse_args()
    rows, build = measure(a)
    if a.attribute:
        names = [leg for leg, _ in ATTRIBUTE]
        lines = ["build id " + build, "", "Gqueries/s, sessions / in place", "", "| precision | set | " + " | ".join(names) + " |", "|---|---|" + "---|" * len(names)]
        for r in rows:
            lines.append("| %s | %s | " % (r["prec"], r["set"]) + " | ".join("%.3f / %.3f" % (r["sessions"][k], r["in_place"][k]) for k in names) + " |")
        print("\n".join(lines))
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
    names = [leg for leg, _ in LEGS]
    lines = ["build id " + build, "", "Gqueries/s, sessions / in place (mean trips per point)", "",
             "| precision | set | " + " | ".join(names) + " | K = 1 / closest | objects within 1 % |", "|---|---|" + "---|" * (len(names) + 2)]
    for r in rows:
        cells = ["%.3f / %.3f (%.1f)" % (r["sessions"][k], r["in_place"][k], r["trips"][k]) for k in names]
        ratio = "%.2f / %.2f" % (r["sessions"]["K = 1"] / r["sessions"]["closest"], r["in_place"]["K = 1"] / r["in_place"]["closest"])
        lines.append("| %s | %s | " % (r["prec"], r["set"]) + " | ".join(cells) + " | %s | %.2f |" % (ratio, r["within"]))
    table = "\n".join(lines)
    print(table)
    if a.out:
        with open(a.out, "w") as f:
            f.write(table + "\n")


if __name__ == "__main__":
    main()
