"""Box overlap queries on a scene handle (docs/experiments.md, "box overlap queries"): the 81 920-triangle mesh of scenes.scene_s4(), both precisions,
2^21 boxes per set (the 10 % sets: 2^17 — each of those boxes touches thousands of triangles), device tensors in and out
(spira_scene_overlap_box_device_* / spira_scene_overlap_any_device_*, outputs allocated once), timed with events around one call.
Sets, each with the identity quaternion and with random rotations:
  surface 1 %   cubes of half extent 1 % of the mesh's extent, centred within that distance of the surface
  uniform 1 %   the same cubes, centres uniform in the mesh's box
  uniform 10 %  cubes of half extent 10 %, centres uniform in the mesh's box
Legs, each as the refilled sessions and as SPIRA_CAST_INPLACE:
  count     max_list = 0, out_count alone
  any       spira_scene_overlap_any_device_*
  list 4    max_list = 4, out_prim and out_count
  list 16   max_list = 16
  within    what a caller had until now: spira_scene_nearest_k_device_* with SPIRA_NEAR_COUNT_ALL and max_near = 0 on the same centres with
            r = the half diagonal |h| (count_within): its rate, its trips, and how many times more objects it reports than the boxes touch
The legs alternate inside one process, call by call; the figure is the median of the timed calls after the warm-up.  Per leg: Gqueries/s and the mean
out_trips (taken on the first call).  Nothing is asserted except that both organisations of a leg give the same bytes and that any == (count > 0).
Then one 256^3 query.voxelize of the mesh's box per precision (boxes made on the device, one any call), timed around the whole helper.
Needs a GPU; no oracle.

    python profiles/overlap_bench.py [--out table.md] [--repeats 5] [--warmup 1] [--level 6] [--log2n 21] [--voxels 256]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "julia-spira_amd"))

LEGS = ["count", "any", "list 4", "list 16", "within"]


def box_sets(s, n, seed=29):
    """name -> boxes [k, 10] in Float64."""
    rng = np.random.default_rng(seed)
    tri = np.asarray(s["triangles10"], dtype=np.float64)
    v = tri[:, :9].reshape(-1, 3)
    lo, hi = v.min(axis=0), v.max(axis=0)
    ext = float((hi - lo).max())

    def unit(k, d=3):
        x = rng.normal(size=(k, d))
        return x / np.linalg.norm(x, axis=1)[:, None]
    t = tri[rng.integers(0, len(tri), n)]
    a = rng.uniform(0.0, 1.0, (n, 1)); b = rng.uniform(0.0, 1.0, (n, 1)) * (1 - a)
    surface = t[:, 0:3] + a * (t[:, 3:6] - t[:, 0:3]) + b * (t[:, 6:9] - t[:, 0:3]) + 0.01 * ext * rng.random((n, 1)) * unit(n)
    uniform = lo + rng.random((n, 3)) * (hi - lo)
    ident = np.tile([0.0, 0.0, 0.0, 1.0], (n, 1))
    rot = unit(n, 4)
    out = {}
    for name, c, frac, k in (("surface 1 %", surface, 0.01, n), ("uniform 1 %", uniform, 0.01, n), ("uniform 10 %", uniform, 0.10, max(1, n >> 4))):
        for qn, q in (("identity", ident), ("rotated", rot)):
            out[name + ", " + qn] = np.concatenate([c[:k], np.full((k, 3), frac * ext), q[:k]], axis=1)
    return out, lo, hi


def measure(a):
    import torch
    from spira_hip import _binding as B
    from spira_hip import query, scenes
    assert B.device_count() >= 1, "no HIP device: this is a GPU measurement"
    B.set_device(0)
    s = scenes.scene_s4(level=a.level)
    sets, lo, hi = box_sets(s, 1 << a.log2n)
    st = torch.cuda.current_stream()
    rows, voxels = [], []
    for prec in ("f32", "f64"):
        npdt, tdt = (np.float32, torch.float32) if prec == "f32" else (np.float64, torch.float64)
        sph, mats, tri = (np.ascontiguousarray(s[k], dtype=npdt) for k in ("spheres5", "materials8", "triangles10"))
        with B.Scene(sph, mats, tri, prec) as h:
            for name, boxes in sets.items():
                n = len(boxes)
                d_boxes = torch.tensor(np.ascontiguousarray(boxes, dtype=npdt), device="cuda:0")
                half_diag = torch.sqrt((d_boxes[:, 3:6] * d_boxes[:, 3:6]).sum(dim=1, keepdim=True))
                d_pts = torch.cat([d_boxes[:, :3], half_diag], dim=1).contiguous()
                prim = torch.empty((n, 16), dtype=torch.int32, device="cuda:0")
                count = torch.empty(n, dtype=torch.int32, device="cuda:0")
                hit = torch.empty(n, dtype=torch.uint8, device="cuda:0")
                trips = torch.empty(n, dtype=torch.int32, device="cuda:0")

                def call(leg, inplace):
                    if leg == "any":
                        h.overlap_any_device(d_boxes.data_ptr(), n, hit.data_ptr(), st.cuda_stream, inplace=inplace)
                    elif leg == "within":
                        h.nearest_k_device(d_pts.data_ptr(), n, 0, 0, 0, 0, count.data_ptr(), st.cuda_stream, inplace=inplace, count_all=True, d_trips_ptr=trips.data_ptr())
                    else:
                        k = {"count": 0, "list 4": 4, "list 16": 16}[leg]
                        h.overlap_box_device(d_boxes.data_ptr(), n, k, prim.data_ptr() if k else 0, count.data_ptr(), st.cuda_stream, inplace=inplace, d_trips_ptr=trips.data_ptr())

                def answer(leg):
                    if leg == "any":
                        return [hit.cpu().numpy().copy()]
                    k = {"count": 0, "list 4": 4, "list 16": 16, "within": 0}[leg]
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
                                    if leg != "any":
                                        mean_trips[leg] = float(trips.cpu().numpy().astype(np.float64).mean())
                                assert all(np.array_equal(x, y) for x, y in zip(first[leg], got)), (leg, "the two organisations differ")
                            if i >= a.warmup:
                                ms[(leg, ip)].append(e0.elapsed_time(e1))
                assert np.array_equal(first["any"][0] == 1, first["count"][0] > 0), "any is not count > 0"
                assert np.array_equal(first["list 4"][0], first["count"][0]) and np.array_equal(first["list 16"][0], first["count"][0])
                touched = float(first["count"][0].astype(np.float64).sum())
                gq = {k: n / (float(np.median(v)) * 1e6) for k, v in ms.items()}
                row = dict(prec=prec, set=name, boxes=n, mean_count=touched / n, touching=float((first["count"][0] > 0).mean()),
                           within_over=float(first["within"][0].astype(np.float64).sum()) / max(touched, 1.0), trips=mean_trips,
                           sessions={leg: gq[(leg, False)] for leg in LEGS}, in_place={leg: gq[(leg, True)] for leg in LEGS})
                rows.append(row)
                print(json.dumps(row), flush=True)
                del d_boxes, d_pts, prim, count, hit, trips
            if a.voxels:
                dims = (a.voxels,) * 3
                for i in range(2):                                   # the first call warms the allocator
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(st)
                    grid = query.voxelize(h, lo, hi, dims)
                    e1.record(st)
                    e1.synchronize()
                    filled = float(grid.float().mean())
                    del grid
                voxels.append(dict(prec=prec, dims=a.voxels, ms=e0.elapsed_time(e1), filled=filled))
                print(json.dumps(voxels[-1]), flush=True)
                torch.cuda.empty_cache()
    return rows, voxels, B.build_id()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--log2n", type=int, default=21)
    ap.add_argument("--voxels", type=int, default=256)
    a = ap.parse_args()
    rows, voxels, build = measure(a)
    lines = ["build id " + build, "", "Gqueries/s, sessions / in place (mean trips per query)", "",
             "| precision | set | boxes | touching | mean count | " + " | ".join(LEGS) + " | within reports x |", "|---|---|---|---|---|" + "---|" * (len(LEGS) + 1)]
    for r in rows:
        cells = ["%.4f / %.4f" % (r["sessions"][k], r["in_place"][k]) + (" (%.1f)" % r["trips"][k] if k in r["trips"] else "") for k in LEGS]
        lines.append("| %s | %s | %d | %.2f | %.1f | " % (r["prec"], r["set"], r["boxes"], r["touching"], r["mean_count"]) + " | ".join(cells) + " | %.1f |" % r["within_over"])
    lines += [""] + ["voxelize %d^3, %s: %.1f ms, %.3f of the cells touch the surface" % (v["dims"], v["prec"], v["ms"], v["filled"]) for v in voxels]
    table = "\n".join(lines)
    print(table)
    if a.out:
        with open(a.out, "w") as f:
            f.write(table + "\n")


if __name__ == "__main__":
    main()
