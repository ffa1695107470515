"""Sphere sweeps on a scene handle (docs/experiments.md, "sphere sweeps"): the 81 920-triangle mesh of scenes.scene_s4(), both precisions, 2^21 sweeps per
set, device tensors in and out (spira_scene_sweep_device_*, outputs allocated once), timed with events around one call.
Sets (origins 1.5 extents from the box centre unless said, t_min 0):
  toward 1 %    toward random surface points, r = 1 % of the extent, t_max +Inf
  toward 10 %   the same rays, r = 10 % of the extent
  overlap       origins within half a radius of the surface, r = 1 % of the extent, random directions: blocked at the start
  miss          rays leaving the scene upward from above the mesh, r = 1 % of the extent
Legs, each as the refilled sessions and as SPIRA_CAST_INPLACE:
  sweep     prim, t, point and normal written
  blocked   spira_scene_sweep_blocked_device_*
  cast      spira_scene_cast_device_* on the same rays (prim, t, normal): the walk's ceiling
  closest   spira_scene_closest_point_device_* on the origins with r_max = +Inf
The legs alternate inside one process, call by call; the figure is the median of the timed calls after the warm-up.  Per leg: Gqueries/s and the mean
out_trips (taken on the first call; cast has none).  Nothing is asserted except that both organisations of a leg give the same bytes.  Verifications per leaf
test are not reported: the kernels keep no such counter.  Needs a GPU; no oracle.

    python profiles/sweep_bench.py [--out table.md] [--repeats 9] [--warmup 2] [--level 6] [--log2n 21]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "julia-spira_amd"))

LEGS = ["sweep", "blocked", "cast", "closest"]


def sweep_sets(s, n, seed=23):
    """name -> (rays [n, 8], radii [n]) in Float64."""
    rng = np.random.default_rng(seed)
    tri = np.asarray(s["triangles10"], dtype=np.float64)
    v = tri[:, :9].reshape(-1, 3)
    lo, hi = v.min(axis=0), v.max(axis=0)
    c, ext = (lo + hi) / 2, float((hi - lo).max())

    def unit(k):
        x = rng.normal(size=(k, 3))
        return x / np.linalg.norm(x, axis=1)[:, None]

    def rays(o, d, t_max=np.inf):
        return np.concatenate([o, np.zeros((n, 1)), d, np.full((n, 1), t_max)], axis=1)
    t = tri[rng.integers(0, len(tri), n)]
    a = rng.uniform(0.0, 1.0, (n, 1)); b = rng.uniform(0.0, 1.0, (n, 1)) * (1 - a)
    surface = t[:, 0:3] + a * (t[:, 3:6] - t[:, 0:3]) + b * (t[:, 6:9] - t[:, 0:3])
    o = c + 1.5 * ext * unit(n)
    toward = rays(o, surface - o)
    r1, r10 = np.full(n, 0.01 * ext), np.full(n, 0.10 * ext)
    near = surface + 0.005 * ext * rng.random((n, 1)) * unit(n)
    up = unit(n)
    up[:, 1] = np.abs(up[:, 1]) + 0.2
    above = c + np.array([0.0, 1.0, 0.0]) * ext + 0.3 * ext * unit(n)
    return {"toward 1 %": (toward, r1), "toward 10 %": (toward, r10), "overlap": (rays(near, unit(n)), r1), "miss": (rays(above, up), r1)}


def measure(a):
    import torch
    from spira_hip import _binding as B
    from spira_hip import scenes
    assert B.device_count() >= 1, "no HIP device: this is a GPU measurement"
    B.set_device(0)
    s = scenes.scene_s4(level=a.level)
    n = 1 << a.log2n
    sets = sweep_sets(s, n)
    st = torch.cuda.current_stream()
    rows = []
    for prec in ("f32", "f64"):
        npdt, tdt = (np.float32, torch.float32) if prec == "f32" else (np.float64, torch.float64)
        sph, mats, tri = (np.ascontiguousarray(s[k], dtype=npdt) for k in ("spheres5", "materials8", "triangles10"))
        prim = torch.empty(n, dtype=torch.int32, device="cuda:0")
        t = torch.empty(n, dtype=tdt, device="cuda:0")
        point = torch.empty((n, 3), dtype=tdt, device="cuda:0")
        nrm = torch.empty((n, 3), dtype=tdt, device="cuda:0")
        hit = torch.empty(n, dtype=torch.uint8, device="cuda:0")
        trips = torch.empty(n, dtype=torch.int32, device="cuda:0")
        with B.Scene(sph, mats, tri, prec) as h:
            for name, (rays, radii) in sets.items():
                d_rays = torch.tensor(np.ascontiguousarray(rays, dtype=npdt), device="cuda:0")
                d_rad = torch.tensor(np.ascontiguousarray(radii, dtype=npdt), device="cuda:0")
                d_pts = torch.cat([d_rays[:, :3], torch.full((n, 1), float("inf"), dtype=tdt, device="cuda:0")], dim=1).contiguous()

                def call(leg, inplace, want_trips):
                    tp = trips.data_ptr() if want_trips else 0
                    if leg == "sweep":
                        h.sweep_device(d_rays.data_ptr(), d_rad.data_ptr(), n, prim.data_ptr(), t.data_ptr(), point.data_ptr(), nrm.data_ptr(), st.cuda_stream, inplace=inplace, d_trips_ptr=tp)
                    elif leg == "blocked":
                        h.sweep_blocked_device(d_rays.data_ptr(), d_rad.data_ptr(), n, hit.data_ptr(), st.cuda_stream, inplace=inplace)
                    elif leg == "cast":
                        h.cast_device(d_rays.data_ptr(), n, prim.data_ptr(), t.data_ptr(), nrm.data_ptr(), st.cuda_stream, inplace=inplace)
                    else:
                        h.closest_point_device(d_pts.data_ptr(), n, prim.data_ptr(), t.data_ptr(), point.data_ptr(), st.cuda_stream, inplace=inplace, d_trips_ptr=tp)

                def answer(leg):
                    outs = {"sweep": (prim, t, point, nrm), "blocked": (hit,), "cast": (prim, t, nrm), "closest": (prim, t, point)}[leg]
                    return [x.cpu().numpy().copy() for x in outs]
                ms = {(leg, ip): [] for leg in LEGS for ip in (False, True)}
                mean_trips, first, touched = {}, {}, 0.0
                for i in range(a.warmup + a.repeats):
                    for leg in LEGS:
                        for ip in (False, True):
                            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            e0.record(st)
                            call(leg, ip, i == 0 and leg in ("sweep", "closest"))
                            e1.record(st)
                            e1.synchronize()
                            if i == 0:
                                got = answer(leg)
                                if not ip:
                                    first[leg] = got
                                    if leg in ("sweep", "closest"):
                                        mean_trips[leg] = float(trips.cpu().numpy().astype(np.float64).mean())
                                    if leg == "sweep":
                                        touched = float((got[0] >= 0).mean())
                                assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(first[leg], got)), (leg, "the two organisations differ")
                            if i >= a.warmup:
                                ms[(leg, ip)].append(e0.elapsed_time(e1))
                assert np.array_equal(first["blocked"][0] == 1, first["sweep"][0] >= 0), "blocked is not prim >= 0"
                gq = {k: n / (float(np.median(v)) * 1e6) for k, v in ms.items()}
                row = dict(prec=prec, set=name, sweeps=n, touched=touched, trips=mean_trips, sessions={leg: gq[(leg, False)] for leg in LEGS},
                           in_place={leg: gq[(leg, True)] for leg in LEGS},
                           spread={leg: [float(np.min(ms[(leg, False)])), float(np.max(ms[(leg, False)]))] for leg in LEGS})
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
    a = ap.parse_args()
    rows, build = measure(a)
    lines = ["build id " + build, "", "Gqueries/s, sessions / in place (mean trips per query)", "",
             "| precision | set | touched | " + " | ".join(LEGS) + " | sweep / cast | sweep / closest |", "|---|---|---|" + "---|" * (len(LEGS) + 2)]
    for r in rows:
        cells = ["%.3f / %.3f" % (r["sessions"][k], r["in_place"][k]) + (" (%.1f)" % r["trips"][k] if k in r["trips"] else "") for k in LEGS]
        lines.append("| %s | %s | %.2f | " % (r["prec"], r["set"], r["touched"]) + " | ".join(cells) +
                     " | %.2f | %.2f |" % (r["sessions"]["sweep"] / r["sessions"]["cast"], r["sessions"]["sweep"] / r["sessions"]["closest"]))
    table = "\n".join(lines)
    print(table)
    if a.out:
        with open(a.out, "w") as f:
            f.write(table + "\n")


if __name__ == "__main__":
    main()
