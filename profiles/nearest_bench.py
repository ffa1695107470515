"""Closest-point queries on a scene handle (docs/experiments.md, "Closest-point queries"): the 81 920-triangle mesh of scenes.scene_s4(), both precisions,
2^21 points per set, device tensors in and out (spira_scene_closest_point_device_*), timed with events around one call.
Point sets:
  surface   points on random triangles displaced by up to 1 % of the mesh's extent in a random direction, r_max +Inf
  box       points uniform in the mesh's box grown by 1.5, r_max +Inf
  far       points 10 extents from the box centre in random directions, r_max +Inf
Table 1: Gqueries/s of the refilled sessions (refill threshold 8, 16, 32 free lanes through SPIRA_CAST_REFILL) against SPIRA_CAST_INPLACE per set and
precision, and the mean out_trips of a point.  The variants alternate inside one process, call by call; the figure is the median of the timed calls after
the warm-up; "16 again" is the same variant a second time: the distance between the two medians is the run-to-run spread the comparison has to beat.
--waves sweeps SPIRA_CAST_WAVES_PER_CU at threshold 16 instead.
Table 2: the box set through a fresh handle, through the handle refitted to the twist of profiles/refit_bench.py and through the handle rebuilt on the
twisted mesh, beside profiles/cast_bench.py's incoherent rays through the same tree.  Nothing is asserted except that all variants of one set give the same
bytes.  Needs a GPU; no oracle.

    python profiles/nearest_bench.py [--out table.md] [--repeats 15] [--warmup 3] [--level 6] [--waves]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "julia-spira_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

WAVES = 20      # SPIRA_CAST_WAVES_PER_CU of the library's default
VARIANTS = [("in place", True, 16, WAVES), ("8", False, 8, WAVES), ("16", False, 16, WAVES), ("32", False, 32, WAVES), ("16 again", False, 16, WAVES)]
WAVE_SWEEP = [("in place", True, 16, WAVES)] + [("%d waves" % w, False, 16, w) for w in (12, 16, 20, 24, 32, 48)]


def point_sets(s, n, seed=19):
    rng = np.random.default_rng(seed)
    tri = np.asarray(s["triangles10"], dtype=np.float64)
    v = tri[:, :9].reshape(-1, 3)
    lo, hi = v.min(axis=0), v.max(axis=0)
    c, ext = (lo + hi) / 2, float((hi - lo).max())

    def unit(k):
        x = rng.normal(size=(k, 3))
        return x / np.linalg.norm(x, axis=1)[:, None]
    t = tri[rng.integers(0, len(tri), n)]
    a = rng.uniform(0.0, 1.0, (n, 1)); b = rng.uniform(0.0, 1.0, (n, 1)) * (1 - a)
    surface = t[:, 0:3] + a * (t[:, 3:6] - t[:, 0:3]) + b * (t[:, 6:9] - t[:, 0:3]) + 0.01 * ext * rng.random((n, 1)) * unit(n)
    box = c + (rng.random((n, 3)) - 0.5) * (hi - lo) * 1.5
    far = c + 10.0 * ext * unit(n)
    inf = np.full((n, 1), np.inf)
    return {"surface": np.concatenate([surface, inf], axis=1), "box": np.concatenate([box, inf], axis=1), "far": np.concatenate([far, inf], axis=1)}


def measure(a):
    import torch
    from spira_hip import _binding as B
    from spira_hip import query, scenes
    from refit_bench import deformations
    from cast_bench import ray_sets
    assert B.device_count() >= 1, "no HIP device: this is a GPU measurement"
    B.set_device(0)
    s = scenes.scene_s4(level=a.level)
    n = 1 << a.log2n
    sets = point_sets(s, n)
    rays = ray_sets(s, scenes.scene_s5(level=0)["camera12"], n, 64, 64)["incoherent"]
    st = torch.cuda.current_stream()
    twist = deformations(np.asarray(s["triangles10"], dtype=np.float64))["twist"]
    rows = []

    def timed(h, d_in, variants, cast=False):
        """median ms per variant, alternating; the outputs of every variant must agree"""
        ms = {v[0]: [] for v in variants}
        ref, trips = None, None
        for i in range(a.warmup + a.repeats):
            for name, inplace, refill, waves in variants:
                os.environ["SPIRA_CAST_REFILL"], os.environ["SPIRA_CAST_WAVES_PER_CU"] = str(refill), str(waves)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                out = query.cast_rays(h, d_in, inplace=inplace, stream=st) if cast else query.closest_points(h, d_in, inplace=inplace, want_trips=(i == 0), stream=st)
                e1.record(st)
                e1.synchronize()
                if i == 0:
                    got = [out[0].cpu().numpy(), out[1].cpu().numpy()] + ([] if cast else [out[2].cpu().numpy()])
                    if ref is None:
                        ref = got
                        trips = None if cast else float(out[3].cpu().numpy().astype(np.float64).mean())
                    assert all(np.array_equal(x, y) for x, y in zip(ref, got)), name
                if i >= a.warmup:
                    ms[name].append(e0.elapsed_time(e1))
        os.environ.pop("SPIRA_CAST_REFILL", None)
        os.environ.pop("SPIRA_CAST_WAVES_PER_CU", None)
        return {k: (float(np.median(v)), float(np.min(v)), float(np.max(v))) for k, v in ms.items()}, ref, trips

    for prec in ("f32", "f64"):
        npdt = np.float32 if prec == "f32" else np.float64
        sph, mats = np.ascontiguousarray(s["spheres5"], dtype=npdt), np.ascontiguousarray(s["materials8"], dtype=npdt)
        base, moved = np.ascontiguousarray(s["triangles10"], dtype=npdt), np.ascontiguousarray(twist, dtype=npdt)
        d_sets = {k: torch.tensor(np.ascontiguousarray(v, dtype=npdt), device="cuda:0") for k, v in sets.items()}
        with B.Scene(sph, mats, base, prec) as h:
            for name, d_pts in d_sets.items():
                res, ref, trips = timed(h, d_pts, WAVE_SWEEP if a.waves else VARIANTS)
                row = dict(table=1, prec=prec, set=name, points=n, mean_trips=trips, on_mesh=float((ref[0] >= len(sph)).mean()),
                           **{"gq_" + k.replace(" ", "_"): n / (v[0] * 1e6) for k, v in res.items()}, **{"ms_" + k.replace(" ", "_"): v for k, v in res.items()})
                rows.append(row)
                print(json.dumps(row), flush=True)
        if a.waves:
            continue
        d_pts, d_rays, d_moved = d_sets["box"], torch.tensor(np.ascontiguousarray(rays, dtype=npdt), device="cuda:0"), torch.tensor(moved, device="cuda:0")
        two = [("in place", True, 16, WAVES), ("16", False, 16, WAVES)]
        with B.Scene(sph, mats, base, prec) as h:
            for tree, change in (("fresh, build pose", None), ("refitted to the twist", h.update_device), ("rebuilt on the twisted mesh", h.rebuild_device)):
                if change is not None:
                    change(d_moved, st)
                v, _, trips = timed(h, d_pts, two)
                c, _, _ = timed(h, d_rays, two, cast=True)
                row = dict(table=2, prec=prec, tree=tree, points=n, mean_trips=trips, gq_default=n / (v["16"][0] * 1e6), gq_in_place=n / (v["in place"][0] * 1e6),
                           grays_default=n / (c["16"][0] * 1e6), grays_in_place=n / (c["in place"][0] * 1e6))
                rows.append(row)
                print(json.dumps(row), flush=True)
    return rows, B.build_id()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--log2n", type=int, default=21)
    ap.add_argument("--waves", action="store_true", help="sweep SPIRA_CAST_WAVES_PER_CU instead of the refill threshold (table 1 only)")
    a = ap.parse_args()
    rows, build = measure(a)
    names = [v[0] for v in (WAVE_SWEEP if a.waves else VARIANTS)]
    lines = ["build id " + build, "", "| precision | set | on the mesh | mean trips | " + " | ".join(names) + " |", "|---|---|---|---|" + "---|" * len(names)]
    for r in rows:
        if r["table"] == 1:
            lines.append("| %s | %s | %.0f %% | %.1f | " % (r["prec"], r["set"], 100 * r["on_mesh"], r["mean_trips"]) + " | ".join("%.3f" % r["gq_" + k.replace(" ", "_")] for k in names) + " |")
    if not a.waves:
        lines += ["", "| precision | tree | mean trips | sessions (Gqueries/s) | in place (Gqueries/s) | cast, sessions (Grays/s) | cast, in place (Grays/s) |", "|---|---|---|---|---|---|---|"]
        for r in rows:
            if r["table"] == 2:
                lines.append("| %s | %s | %.1f | %.3f | %.3f | %.3f | %.3f |" % (r["prec"], r["tree"], r["mean_trips"], r["gq_default"], r["gq_in_place"], r["grays_default"], r["grays_in_place"]))
    table = "\n".join(lines)
    print(table)
    if a.out:
        with open(a.out, "w") as f:
            f.write(table + "\n")


if __name__ == "__main__":
    main()
