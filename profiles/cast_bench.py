"""Ray queries on a scene handle, traversal alone (docs/experiments.md, "Ray queries"): the 81 920-triangle mesh of scenes.scene_s4() / scene_s5(), both
precisions, about 2 M rays per set, device tensors in and out (spira_scene_cast_device_* / spira_scene_occluded_device_*), timed with events around one call.
Ray sets:
  camera      the 1920 x 1080 pixel-centre camera rays of S5 (coherent), closest hit
  incoherent  2^21 rays from c + 1.5 ext u (u random unit vectors) to targets uniform in the mesh box grown by 1.3, closest hit
  occlusion   2^21 short rays (t_max 0.25 ext) from points just above random triangles over the hemisphere of their normal, occluded
Table 1: Grays/s of the refilled sessions (refill threshold 8, 16, 32 free lanes through SPIRA_CAST_REFILL) against SPIRA_CAST_INPLACE per set and precision.
The variants alternate inside one process, call by call, and the figure is the median of the timed calls after the warm-up; the threshold-16 variant is
listed twice ("16" and "16 again"): the distance between its two medians is the run-to-run spread the comparison has to beat.
Table 2: the incoherent set through a fresh handle, through the handle refitted to the twist of profiles/refit_bench.py, through the handle rebuilt on the
twisted mesh (Morton order), and through a fresh handle (SAH build) on the twisted mesh.  Nothing is asserted except that all variants of one set give the
same bytes.  Needs a GPU; no oracle.

    python profiles/cast_bench.py [--out table.md] [--repeats 15] [--warmup 3] [--level 6]"""
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
# --waves: the refilled sessions at threshold 16 with other numbers of waves per CU (SPIRA_CAST_WAVES_PER_CU), beside in place
WAVE_SWEEP = [("in place", True, 16, WAVES)] + [("%d waves" % w, False, 16, w) for w in (12, 16, 20, 24, 32, 48)]


def ray_sets(s, s5_camera, n, width, height, seed=9):
    rng = np.random.default_rng(seed)
    tri = np.asarray(s["triangles10"], dtype=np.float64)
    v = tri[:, :9].reshape(-1, 3)
    lo, hi = v.min(axis=0), v.max(axis=0)
    c, ext = (lo + hi) / 2, float((hi - lo).max())
    cam = np.asarray(s5_camera, dtype=np.float64)
    u, w = np.meshgrid((np.arange(width) + 0.5) / width, (np.arange(height) + 0.5) / height)
    d = cam[3:6] + u.reshape(-1, 1) * cam[6:9] + w.reshape(-1, 1) * cam[9:12] - cam[0:3]
    m = len(d)
    camera = np.concatenate([np.tile(cam[0:3], (m, 1)), np.full((m, 1), 0.001), d, np.full((m, 1), np.inf)], axis=1)

    def unit(k):
        x = rng.normal(size=(k, 3))
        return x / np.linalg.norm(x, axis=1)[:, None]
    o = c + 1.5 * ext * unit(n)
    tgt = c + (rng.random((n, 3)) - 0.5) * (hi - lo) * 1.3
    incoherent = np.concatenate([o, np.full((n, 1), 0.001), 3.7 * (tgt - o), np.full((n, 1), np.inf)], axis=1)
    t = tri[rng.integers(0, len(tri), n)]
    nrm = np.cross(t[:, 3:6] - t[:, 0:3], t[:, 6:9] - t[:, 0:3])
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    p = (t[:, 0:3] + t[:, 3:6] + t[:, 6:9]) / 3 + 1e-3 * ext * nrm
    h = unit(n)
    h = np.where((h * nrm).sum(axis=1, keepdims=True) < 0, -h, h)
    occlusion = np.concatenate([p, np.zeros((n, 1)), h, np.full((n, 1), 0.25 * ext)], axis=1)
    return {"camera": camera, "incoherent": incoherent, "occlusion": occlusion}


def measure(a):
    import torch
    from spira_hip import _binding as B
    from spira_hip import query, scenes
    from refit_bench import deformations
    assert B.device_count() >= 1, "no HIP device: this is a GPU measurement"
    B.set_device(0)
    s = scenes.scene_s4(level=a.level)
    sets = ray_sets(s, scenes.scene_s5(level=0)["camera12"], 1 << 21, 1920, 1080)
    st = torch.cuda.current_stream()
    twist = deformations(np.asarray(s["triangles10"], dtype=np.float64))["twist"]
    rows = []

    def timed(h, d_rays, occlusion, variants):
        """median ms per variant, alternating; the outputs of every variant must agree"""
        ms = {v[0]: [] for v in variants}
        ref = None
        for i in range(a.warmup + a.repeats):
            for name, inplace, refill, waves in variants:
                os.environ["SPIRA_CAST_REFILL"], os.environ["SPIRA_CAST_WAVES_PER_CU"] = str(refill), str(waves)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                out = query.cast_rays(h, d_rays, occlusion=occlusion, inplace=inplace, stream=st)
                e1.record(st)
                e1.synchronize()
                if i == 0:
                    got = [out.cpu().numpy()] if occlusion else [out[0].cpu().numpy(), out[1].cpu().numpy()]
                    if ref is None:
                        ref = got
                    assert all(np.array_equal(x, y) for x, y in zip(ref, got)), name
                if i >= a.warmup:
                    ms[name].append(e0.elapsed_time(e1))
        os.environ.pop("SPIRA_CAST_REFILL", None)
        os.environ.pop("SPIRA_CAST_WAVES_PER_CU", None)
        return {k: (float(np.median(v)), float(np.min(v)), float(np.max(v))) for k, v in ms.items()}, ref

    for prec in ("f32", "f64"):
        npdt = np.float32 if prec == "f32" else np.float64
        sph, mats = np.ascontiguousarray(s["spheres5"], dtype=npdt), np.ascontiguousarray(s["materials8"], dtype=npdt)
        base, moved = np.ascontiguousarray(s["triangles10"], dtype=npdt), np.ascontiguousarray(twist, dtype=npdt)
        d_sets = {k: torch.tensor(np.ascontiguousarray(v, dtype=npdt), device="cuda:0") for k, v in sets.items()}
        with B.Scene(sph, mats, base, prec) as h:
            for name, d_rays in d_sets.items():
                res, ref = timed(h, d_rays, name == "occlusion", WAVE_SWEEP if a.waves else VARIANTS)
                n = d_rays.shape[0]
                hits = float((ref[0] == 1).mean()) if name == "occlusion" else float((ref[0] >= 0).mean())
                row = dict(table=1, prec=prec, set=name, rays=n, hit_fraction=hits,
                           **{"grays_" + k.replace(" ", "_"): n / (v[0] * 1e6) for k, v in res.items()}, **{"ms_" + k.replace(" ", "_"): v for k, v in res.items()})
                rows.append(row)
                print(json.dumps(row), flush=True)
        if a.waves:
            continue
        # ---- table 2: the same incoherent rays through four trees of the twisted mesh (and the build pose)
        d_rays, d_moved = d_sets["incoherent"], torch.tensor(moved, device="cuda:0")
        two = [("in place", True, 16, WAVES), ("16", False, 16, WAVES)]
        trees = {}
        with B.Scene(sph, mats, base, prec) as h:
            trees["fresh, build pose"], _ = timed(h, d_rays, False, two)
            h.update_device(d_moved, st)
            trees["refitted to the twist"], ref_r = timed(h, d_rays, False, two)
            h.rebuild_device(d_moved, st)
            trees["rebuilt on the twisted mesh"], ref_b = timed(h, d_rays, False, two)
        with B.Scene(sph, mats, moved, prec) as h:
            trees["fresh on the twisted mesh"], ref_f = timed(h, d_rays, False, two)
        same = all(np.array_equal(x, y) and np.array_equal(x, z) for x, y, z in zip(ref_f, ref_r, ref_b))
        for k, v in trees.items():
            row = dict(table=2, prec=prec, tree=k, rays=int(d_rays.shape[0]), same_answers=same,
                       grays_default=d_rays.shape[0] / (v["16"][0] * 1e6), grays_in_place=d_rays.shape[0] / (v["in place"][0] * 1e6), ms_default=v["16"], ms_in_place=v["in place"])
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows, B.build_id()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--waves", action="store_true", help="sweep SPIRA_CAST_WAVES_PER_CU instead of the refill threshold (table 1 only)")
    a = ap.parse_args()
    rows, build = measure(a)
    if a.waves:
        names = [v[0] for v in WAVE_SWEEP]
        lines = ["build id " + build, "", "| precision | set | " + " | ".join(names) + " |", "|---|---|" + "---|" * len(names)]
        for r in rows:
            lines.append("| %s | %s | " % (r["prec"], r["set"]) + " | ".join("%.3f" % r["grays_" + k.replace(" ", "_")] for k in names) + " |")
        print("\n".join(lines))
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
    lines = ["build id " + build, "", "| precision | set | hits | in place | refill 8 | refill 16 | refill 32 | refill 16 again |", "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        if r["table"] == 1:
            lines.append("| %s | %s | %.0f %% | %.3f | %.3f | %.3f | %.3f | %.3f |" % (r["prec"], r["set"], 100 * r["hit_fraction"], r["grays_in_place"], r["grays_8"], r["grays_16"],
                                                                                r["grays_32"], r["grays_16_again"]))
    lines += ["", "| precision | tree | sessions (Grays/s) | in place (Grays/s) | same answers |", "|---|---|---|---|---|"]
    for r in rows:
        if r["table"] == 2:
            lines.append("| %s | %s | %.3f | %.3f | %s |" % (r["prec"], r["tree"], r["grays_default"], r["grays_in_place"], "yes" if r["same_answers"] else "NO"))
    table = "\n".join(lines)
    print(table)
    if a.out:
        with open(a.out, "w") as f:
            f.write(table + "\n")


if __name__ == "__main__":
    main()
