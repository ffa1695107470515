"""Triangle overlap queries on a scene handle (docs/experiments.md, "triangle overlap queries"): the 81 920-triangle mesh of scenes.scene_s4() as the
scene, both precisions, and copies of that mesh as about 2^21 query triangles, device tensors in and out (spira_scene_overlap_tri_device_* /
spira_scene_overlap_tri_any_device_*, outputs allocated once), timed with events around one call.
Query sets (each the mesh's own triangles10 rows, copy after copy until the list is full, every copy moved a little differently):
  displaced   the mesh shifted by 0.2 % .. 2 % of its extent along a random direction per copy
  twisted     the mesh twisted about the vertical axis through its middle, 0.5 .. 5 degrees per extent of height per copy
Legs, each as the refilled sessions and as SPIRA_CAST_INPLACE:
  count     max_list = 0, out_count alone
  any       spira_scene_overlap_tri_any_device_*
  list 4    max_list = 4, out_prim and out_count
  list 16   max_list = 16
  box       what a caller had until now: spira_scene_overlap_box_device_* (count) on the queries' enclosing axis-aligned boxes: its rate, its trips, and how
            many times more objects it reports than the triangles cut
  edges     ... and spira_scene_occluded_device_* on the three edge segments of every query (3 n rays; the rate is per QUERY): its rate, and the share
            of the cutting queries (any == 1) on which no edge hits anything — the scene edges that pierce the query's face
The legs alternate inside one process, call by call; the figure is the median of the timed calls after the warm-up.  Per leg: Gqueries/s and the mean
out_trips (taken on the first call).  Nothing is asserted except that both organisations of a leg give the same bytes and that any == (count > 0).
Needs a GPU; no oracle.

    python profiles/trioverlap_bench.py [--out table.md] [--repeats 5] [--warmup 1] [--level 6] [--log2n 21]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "julia-spira_amd"))

LEGS = ["count", "any", "list 4", "list 16", "box", "edges"]


def query_sets(s, n, seed=31):
    """name -> query triangles [n, 10] in Float64."""
    rng = np.random.default_rng(seed)
    tri = np.asarray(s["triangles10"], dtype=np.float64)
    v = tri[:, :9].reshape(-1, 3, 3)
    lo, hi = v.reshape(-1, 3).min(axis=0), v.reshape(-1, 3).max(axis=0)
    ext, mid = float((hi - lo).max()), (lo + hi) / 2
    copies = -(-n // len(tri))
    moved, twisted = [], []
    for c in range(copies):
        d = rng.normal(size=3)
        moved.append(v + d / np.linalg.norm(d) * ext * (0.002 + 0.018 * (c + 1) / copies))
        ang = np.radians(0.5 + 4.5 * (c + 1) / copies) * (v[..., 1] - mid[1]) / ext
        x, z = v[..., 0] - mid[0], v[..., 2] - mid[2]
        twisted.append(np.stack([mid[0] + np.cos(ang) * x - np.sin(ang) * z, v[..., 1], mid[2] + np.sin(ang) * x + np.cos(ang) * z], axis=-1))
    out = {}
    for name, parts in (("displaced", moved), ("twisted", twisted)):
        q = np.concatenate(parts)[:n].reshape(-1, 9)
        out[name] = np.concatenate([q, np.ones((len(q), 1))], axis=1)
    return out


def measure(a):
    import torch
    from spira_hip import _binding as B
    from spira_hip import scenes
    assert B.device_count() >= 1, "no HIP device: this is a GPU measurement"
    B.set_device(0)
    s = scenes.scene_s4(level=a.level)
    sets = query_sets(s, 1 << a.log2n)
    st = torch.cuda.current_stream()
    rows = []
    for prec in ("f32", "f64"):
        npdt = np.float32 if prec == "f32" else np.float64
        sph, mats, tri = (np.ascontiguousarray(s[k], dtype=npdt) for k in ("spheres5", "materials8", "triangles10"))
        with B.Scene(sph, mats, tri, prec) as h:
            for name, q in sets.items():
                n = len(q)
                d_q = torch.tensor(np.ascontiguousarray(q, dtype=npdt), device="cuda:0")
                vq = d_q[:, :9].reshape(n, 3, 3)
                blo, bhi = vq.min(dim=1).values, vq.max(dim=1).values
                ident = torch.zeros((n, 4), dtype=d_q.dtype, device="cuda:0")
                ident[:, 3] = 1
                d_boxes = torch.cat([(blo + bhi) / 2, (bhi - blo) / 2, ident], dim=1).contiguous()
                e = torch.roll(vq, -1, dims=1) - vq                                    # the three edges, [n, 3, 3]
                zero = torch.zeros((n, 3, 1), dtype=d_q.dtype, device="cuda:0")
                d_rays = torch.cat([vq, zero, e, torch.sqrt((e * e).sum(dim=2, keepdim=True))], dim=2).reshape(3 * n, 8).contiguous()
                prim = torch.empty((n, 16), dtype=torch.int32, device="cuda:0")
                count = torch.empty(n, dtype=torch.int32, device="cuda:0")
                hit = torch.empty(n, dtype=torch.uint8, device="cuda:0")
                hit3 = torch.empty(3 * n, dtype=torch.uint8, device="cuda:0")
                trips = torch.empty(n, dtype=torch.int32, device="cuda:0")

                def call(leg, inplace):
                    if leg == "any":
                        h.overlap_tri_any_device(d_q.data_ptr(), n, hit.data_ptr(), st.cuda_stream, inplace=inplace)
                    elif leg == "box":
                        h.overlap_box_device(d_boxes.data_ptr(), n, 0, 0, count.data_ptr(), st.cuda_stream, inplace=inplace, d_trips_ptr=trips.data_ptr())
                    elif leg == "edges":
                        h.occluded_device(d_rays.data_ptr(), 3 * n, hit3.data_ptr(), st.cuda_stream, inplace=inplace)
                    else:
                        k = {"count": 0, "list 4": 4, "list 16": 16}[leg]
                        h.overlap_tri_device(d_q.data_ptr(), n, k, prim.data_ptr() if k else 0, count.data_ptr(), st.cuda_stream, inplace=inplace, d_trips_ptr=trips.data_ptr())

                def answer(leg):
                    if leg == "any":
                        return [hit.cpu().numpy().copy()]
                    if leg == "edges":
                        return [hit3.cpu().numpy().reshape(n, 3).copy()]
                    k = {"count": 0, "list 4": 4, "list 16": 16, "box": 0}[leg]
                    return [count.cpu().numpy().copy()] + ([prim.cpu().numpy().reshape(-1)[:n * k].copy()] if k else [])
                ms = {(leg, ip): [] for leg in LEGS for ip in (False, True)}
                mean_trips, first = {}, {}
                for i in range(a.warmup + a.repeats):
                    for leg in LEGS:
                        for ip in (False, True):
                            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            e0.record(st)
                            call(leg, ip)
                            e1.record(st)
                            e1.synchronize()
                            if i == 0:
                                got = answer(leg)
                                if not ip:
                                    first[leg] = got
                                    if leg not in ("any", "edges"):
                                        mean_trips[leg] = float(trips.cpu().numpy().astype(np.float64).mean())
                                assert all(np.array_equal(x, y) for x, y in zip(first[leg], got)), (leg, "the two organisations differ")
                            if i >= a.warmup:
                                ms[(leg, ip)].append(e0.elapsed_time(e1))
                assert np.array_equal(first["any"][0] == 1, first["count"][0] > 0), "any is not count > 0"
                assert np.array_equal(first["list 4"][0], first["count"][0]) and np.array_equal(first["list 16"][0], first["count"][0])
                cut = first["count"][0] > 0
                objects = float(first["count"][0].astype(np.float64).sum())
                edge_hit = (first["edges"][0] == 1).any(axis=1)
                gq = {k: n / (float(np.median(v)) * 1e6) for k, v in ms.items()}
                row = dict(prec=prec, set=name, queries=n, cutting=float(cut.mean()), mean_count=objects / n, over_16=float((first["count"][0] > 16).mean()),
                           box_over=float(first["box"][0].astype(np.float64).sum()) / max(objects, 1.0),
                           edges_miss=float((cut & ~edge_hit).sum()) / max(float(cut.sum()), 1.0), trips=mean_trips,
                           sessions={leg: gq[(leg, False)] for leg in LEGS}, in_place={leg: gq[(leg, True)] for leg in LEGS})
                rows.append(row)
                print(json.dumps(row), flush=True)
                del d_q, d_boxes, d_rays, prim, count, hit, hit3, trips
                torch.cuda.empty_cache()
    return rows, B.build_id()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--log2n", type=int, default=21)
    a = ap.parse_args()
    rows, build = measure(a)
    lines = ["build id " + build, "", "Gqueries/s, sessions / in place (mean trips per query)", "",
             "| precision | set | queries | cutting | objects per query | " + " | ".join(LEGS) + " | box reports x | edges miss |", "|---|---|---|---|---|" + "---|" * (len(LEGS) + 2)]
    for r in rows:
        cells = ["%.4f / %.4f" % (r["sessions"][k], r["in_place"][k]) + (" (%.1f)" % r["trips"][k] if k in r["trips"] else "") for k in LEGS]
        lines.append("| %s | %s | %d | %.3f | %.2f | " % (r["prec"], r["set"], r["queries"], r["cutting"], r["mean_count"]) + " | ".join(cells)
                     + " | %.1f | %.3f |" % (r["box_over"], r["edges_miss"]))
    table = "\n".join(lines)
    print(table)
    if a.out:
        with open(a.out, "w") as f:
            f.write(table + "\n")


if __name__ == "__main__":
    main()
