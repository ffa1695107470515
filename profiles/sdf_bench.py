"""Signed distance queries on a scene handle (docs/experiments.md, "Signed distance queries"): the 81 920-triangle mesh of scenes.scene_s4(), both
precisions, 2^21 points per set, device tensors in and out (spira_scene_signed_distance_device_*), timed with events around one call.
Point sets, as profiles/nearest_bench.py's: within 1 % of the surface, uniform in the mesh's box grown by 1.5, and 10 extents away.
Table 1, per set and precision: Gqueries/s of the full query (nearest surface and sign) through the refilled sessions and through SPIRA_CAST_INPLACE, of
the sign-only query through both, the mean out_trips of a point and the share of points that needed ray 2 — beside what a caller had before the entry
existed, composed on the device: query.closest_points on the full handle, three query.count_hits calls (rays 0, 1 and 2 for every point: a caller cannot
pick the points that need ray 2 without a host round trip) on a handle created from the triangles alone, the ray tensors made with torch, the sphere
test and the vote combined with torch.  The variants alternate inside one process, call by call; the figure is the median of the timed calls after the
warm-up, with the least and the largest beside it in the JSON rows.
Table 2: query.distance_field on a 256^3 grid over the mesh's box against that same composition on the grid's cell centres.
Nothing is asserted except that every variant of one set gives the same bytes (the composition: the same sign and the same |distance|).  Needs a GPU.

    python profiles/sdf_bench.py [--out table.md] [--repeats 9] [--warmup 2] [--level 6] [--log2n 21] [--grid 256]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "julia-spira_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

VARIANTS = ["sessions", "in place", "sign only, sessions", "sign only, in place", "composed"]


def measure(a):
    import torch
    from spira_hip import _binding as B
    from spira_hip import query, scenes
    from nearest_bench import point_sets
    assert B.device_count() >= 1, "no HIP device: this is a GPU measurement"
    B.set_device(0)
    s = scenes.scene_s4(level=a.level)
    n = 1 << a.log2n
    sets = point_sets(s, n)
    st = torch.cuda.current_stream()
    v = np.asarray(s["triangles10"], dtype=np.float64)[:, :9].reshape(-1, 3)
    lo, hi = v.min(axis=0), v.max(axis=0)
    rows = []

    def composed(h, ht, d_pts, d_sph, dirs):
        """What a caller had: the magnitude from closest_points, the sign from three counted ray lists and the spheres, combined with torch."""
        prim, dist, _, _ = query.closest_points(h, d_pts, want_point=False, stream=st)
        m = d_pts.shape[0]
        rays = torch.empty((m, 8), dtype=d_pts.dtype, device=d_pts.device)
        rays[:, :3] = d_pts[:, :3]
        rays[:, 3] = 0
        rays[:, 7] = float("inf")
        odd = []
        for j in range(3):
            rays[:, 4:7] = dirs[j]
            odd.append((query.count_hits(ht, rays, stream=st) & 1) == 1)
        inside = (odd[0] & odd[1]) | (odd[2] & (odd[0] ^ odd[1]))
        w = d_pts[:, None, :3] - d_sph[None, :, :3]
        inside |= (torch.sqrt((w[..., 0] * w[..., 0] + w[..., 1] * w[..., 1]) + w[..., 2] * w[..., 2]) < d_sph[None, :, 3]).any(dim=1)
        inside &= prim != B.RAY_INVALID
        return torch.where(inside, -dist, dist), inside

    def run(name, h, ht, d_pts, d_sph, dirs, trips=False):
        if name == "composed":
            return composed(h, ht, d_pts, d_sph, dirs)
        if name.startswith("sign only"):
            inside = torch.empty(d_pts.shape[0], dtype=torch.uint8, device=d_pts.device)
            tr = torch.empty(d_pts.shape[0], dtype=torch.int32, device=d_pts.device) if trips else None
            h.signed_distance_device(d_pts.data_ptr(), d_pts.shape[0], 0, 0, 0, inside.data_ptr(), st.cuda_stream, inplace=name.endswith("in place"),
                                     d_trips_ptr=tr.data_ptr() if trips else 0)
            return None, inside, None, tr
        out = query.signed_distance(h, d_pts, inplace=(name == "in place"), want_point=False, want_crossings=trips, want_trips=trips, stream=st)
        return out[1], out[3], out[4], out[5]

    def timed(h, ht, d_pts, d_sph, dirs, variants):
        ms = {k: [] for k in variants}
        info = {}
        ref = None
        for i in range(a.warmup + a.repeats):
            for name in variants:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                out = run(name, h, ht, d_pts, d_sph, dirs, trips=(i == 0))
                e1.record(st)
                e1.synchronize()
                if i == 0:
                    inside = (out[1] == 1).cpu().numpy()
                    dist = None if out[0] is None else out[0].cpu().numpy()
                    if ref is None:
                        ref = (dist, inside)
                        cr = out[2].cpu().numpy().view(np.uint32)
                        info = dict(mean_trips=float(out[3].cpu().numpy().astype(np.float64).mean()), third=float((cr[:, 2] != B.SDF_SKIPPED).mean()),
                                    inside=float(inside.mean()))
                    elif name.startswith("sign only") and out[3] is not None:
                        info["mean_trips_" + name.replace(",", "").replace(" ", "_")] = float(out[3].cpu().numpy().astype(np.float64).mean())
                    assert np.array_equal(inside, ref[1]), name
                    assert dist is None or np.array_equal(dist.view(ref[0].dtype), ref[0]), name
                if i >= a.warmup:
                    ms[name].append(e0.elapsed_time(e1))
        return {k: (float(np.median(x)), float(np.min(x)), float(np.max(x))) for k, x in ms.items()}, info

    for prec in ("f32", "f64"):
        npdt = np.float32 if prec == "f32" else np.float64
        tdt = torch.float32 if prec == "f32" else torch.float64
        sph, mats, tri = (np.ascontiguousarray(s[k], dtype=npdt) for k in ("spheres5", "materials8", "triangles10"))
        d_sph = torch.tensor(sph, device="cuda:0")
        # (the library normalises the rays itself; the composition hands it the raw directions, as query.inside_mesh does)
        dirs = [torch.tensor(np.array(query.INSIDE_DIRECTIONS[j], dtype=npdt), device="cuda:0") for j in range(3)]
        with B.Scene(sph, mats, tri, prec) as h, B.Scene(None, mats, tri, prec) as ht:
            for name, pts in sets.items():
                d_pts = torch.tensor(np.ascontiguousarray(pts, dtype=npdt), device="cuda:0")
                res, info = timed(h, ht, d_pts, d_sph, dirs, VARIANTS)
                row = dict(table=1, prec=prec, set=name, points=n, **info, **{"gq_" + k: n / (x[0] * 1e6) for k, x in res.items()}, **{"ms_" + k: x for k, x in res.items()})
                rows.append(row)
                print(json.dumps(row), flush=True)
            g = a.grid
            cells = torch.tensor(query.voxel_boxes(lo, hi, (g, g, g), npdt)[:, :3], device="cuda:0")
            d_cells = torch.cat([cells, torch.full((cells.shape[0], 1), float("inf"), dtype=tdt, device="cuda:0")], dim=1).contiguous()
            ms = {"distance_field": [], "composed": []}
            for i in range(a.warmup + a.repeats):
                for name in ms:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(st)
                    out = query.distance_field(h, lo, hi, (g, g, g), stream=st).reshape(-1) if name == "distance_field" else composed(h, ht, d_cells, d_sph, dirs)[0]
                    e1.record(st)
                    e1.synchronize()
                    if i == 0:
                        if name == "distance_field":
                            field = out.cpu().numpy()
                        else:
                            assert np.array_equal(out.cpu().numpy().view(field.dtype), field), "the composition and distance_field disagree"
                    if i >= a.warmup:
                        ms[name].append(e0.elapsed_time(e1))
            row = dict(table=2, prec=prec, grid=g, cells=g ** 3, inside=float((field < 0).mean()), **{"ms_" + k: (float(np.median(x)), float(np.min(x)), float(np.max(x))) for k, x in ms.items()})
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
    ap.add_argument("--grid", type=int, default=256)
    a = ap.parse_args()
    rows, build = measure(a)
    lines = ["build id " + build, "", "| precision | set | inside | needed ray 2 | mean trips | " + " | ".join(VARIANTS) + " |", "|---|---|---|---|---|" + "---|" * len(VARIANTS)]
    for r in rows:
        if r["table"] == 1:
            lines.append("| %s | %s | %.0f %% | %.1f %% | %.1f | " % (r["prec"], r["set"], 100 * r["inside"], 100 * r["third"], r["mean_trips"]) + " | ".join("%.3f" % r["gq_" + k] for k in VARIANTS) + " |")
    lines += ["", "| precision | grid | inside | distance_field (ms) | composed (ms) |", "|---|---|---|---|---|"]
    for r in rows:
        if r["table"] == 2:
            lines.append("| %s | %d^3 | %.1f %% | %.1f | %.1f |" % (r["prec"], r["grid"], 100 * r["inside"], r["ms_distance_field"][0], r["ms_composed"][0]))
    table = "\n".join(lines)
    print(table)
    if a.out:
        with open(a.out, "w") as f:
            f.write(table + "\n")


if __name__ == "__main__":
    main()
