"""Rebuild of a handle's tree on the device against scene creation (docs/experiments.md §24): the 81 920-triangle mesh of scenes.scene_s4(), both precisions.
(a) what a new tree costs: host wall time of Scene.rebuild (host arrays: returns when the scene is ready), host wall time and device time of
    Scene.rebuild_device (a device tensor, events on the caller's stream), beside Scene(...) creation of the same mesh in the same process — the only
    other way to a new tree, and unchanged code — and beside Scene.update_device (the refit, where the frame rule allows it);
(b) what the rebuilt (Morton order) tree costs a render: the frame of BASELINE configs[4] (S4, 1920 x 1080, spp 64, depth 12) and of the mesh stress scene
    S5 through a rebuilt handle, beside a fresh host-built (SAH) handle on the same mesh — in the build pose and after the twist of §23, where the
    refitted tree is the third column.
Every figure is the median of the timed calls after the warm-up (the minimum beside it); device times are events on the stream around one call, wall
times bracket the call and a synchronisation.  Both sides of every comparison are printed; nothing is asserted.  Needs a GPU; no oracle.

    python profiles/rebuild_bench.py [--out table.md] [--repeats 20] [--warmup 3] [--frames 5] [--level 6]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "julia-spira_amd"))


def poses(tri):
    """name -> triangles10: the build pose, the twist of refit_bench.py (inside the old frame) and a pose no update can reach (moved and grown)."""
    v = tri[:, :9].reshape(-1, 3)
    lo, hi = v.min(axis=0), v.max(axis=0)
    c, ext = (lo + hi) / 2.0, float((hi - lo).max())
    x, y, z = (v - c).T

    def put(xyz):
        t = tri.copy()
        t[:, :9] = (np.stack(xyz, axis=1) + c).reshape(-1, 9)
        return t
    ang = 3.0 * y / ext
    return {
        "build": tri.copy(),
        "twist": put([np.cos(ang) * x - np.sin(ang) * z, y, np.sin(ang) * x + np.cos(ang) * z]),
        "far": put([2.5 * x, 2.5 * y + 3.0 * ext, 2.5 * z]),
    }


def _stats(xs):
    return float(np.median(xs)), float(np.min(xs))


def measure(a):
    import torch
    from spira_hip import _binding as B
    from spira_hip import scenes
    assert B.device_count() >= 1, "no HIP device: this is a GPU measurement"
    B.set_device(0)
    s4, s5 = scenes.scene_s4(level=a.level), scenes.scene_s5(level=a.level)
    st = torch.cuda.current_stream()
    rows = []
    for prec in ("f32", "f64"):
        npdt = np.float32 if prec == "f32" else np.float64
        tdt = torch.float32 if prec == "f32" else torch.float64
        sph, mats = np.ascontiguousarray(s4["spheres5"], dtype=npdt), np.ascontiguousarray(s4["materials8"], dtype=npdt)
        pose = {k: np.ascontiguousarray(v, dtype=npdt) for k, v in poses(np.asarray(s4["triangles10"], dtype=np.float64)).items()}
        d_pose = {k: torch.tensor(v, device="cuda:0") for k, v in pose.items()}
        names = list(pose)

        # ---- (a) rebuild against create: the mesh alternates between the poses, so that no call finds the arrays it left
        def timed(fn, sync, which=names):
            wall, dev = [], []
            for i in range(a.warmup + a.repeats):
                k = which[i % len(which)]
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                e0.record(st)
                fn(k)
                e1.record(st)
                if sync:
                    e1.synchronize()
                t1 = time.perf_counter()
                e1.synchronize()
                if i >= a.warmup:
                    wall.append((t1 - t0) * 1e3)
                    dev.append(e0.elapsed_time(e1))
            return _stats(wall), _stats(dev)
        with B.Scene(sph, mats, pose["build"], prec) as h:
            (rw, rw_min), _ = timed(lambda k: h.rebuild(pose[k]), True)
            (dw, dw_min), (dd, dd_min) = timed(lambda k: h.rebuild_device(d_pose[k], st), True)
            (dr, dr_min), _ = timed(lambda k: h.rebuild_device(d_pose[k], st), False)      # wall time until the call RETURNS (the last of its work enqueued)
            h.rebuild_device(d_pose["build"], st)
            (uw, uw_min), _ = timed(lambda k: h.update_device(d_pose[k], st), True, ["build", "twist"])      # the refit, inside the frame
        cw = []
        for i in range(a.warmup + a.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hh = B.Scene(sph, mats, pose[names[i % len(names)]], prec)
            t1 = time.perf_counter()
            hh.destroy()
            if i >= a.warmup:
                cw.append((t1 - t0) * 1e3)
        row = dict(prec=prec, triangles=len(pose["build"]), rebuild_host_wall_ms=rw, rebuild_host_wall_ms_min=rw_min,
                   rebuild_device_wall_ms=dw, rebuild_device_wall_ms_min=dw_min, rebuild_device_device_ms=dd, rebuild_device_device_ms_min=dd_min,
                   rebuild_device_return_ms=dr, rebuild_device_return_ms_min=dr_min, update_device_wall_ms=uw, update_device_wall_ms_min=uw_min,
                   create_wall_ms=_stats(cw)[0], create_wall_ms_min=_stats(cw)[1])

        # ---- (b) frames through the rebuilt tree, a fresh host build and (after the twist) the refitted tree
        out = torch.empty((3, a.height, a.width), dtype=tdt, device="cuda:0")

        def frame_ms(h, cam, cfg):
            p = h.params(a.width, a.height, 64, 12, flags=B.POST_NONE, seed=scenes.seed_for(cfg))
            ms = []
            for i in range(1 + a.frames):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                h.render_device(cam, p, out.data_ptr(), 0, st.cuda_stream)
                e1.record(st)
                e1.synchronize()
                if i >= 1:
                    ms.append(e0.elapsed_time(e1))
            return _stats(ms)[0], out.cpu().numpy().copy()
        for scene_name, cam, cfg in (("s4", s4["camera12"], 5), ("s5", s5["camera12"], 6)):
            for k in ("build", "twist"):
                with B.Scene(sph, mats, pose[k], prec) as fresh:
                    f_ms, img_f = frame_ms(fresh, cam, cfg)
                with B.Scene(sph, mats, pose["far"], prec) as h:
                    h.rebuild_device(d_pose[k], st)
                    b_ms, img_b = frame_ms(h, cam, cfg)
                key = "%s_%s" % (scene_name, k)
                row["frame_fresh_%s_ms" % key], row["frame_rebuilt_%s_ms" % key] = f_ms, b_ms
                row["same_image_%s" % key] = bool(np.array_equal(img_b, img_f))
                if k == "twist":
                    with B.Scene(sph, mats, pose["build"], prec) as h:
                        h.update_device(d_pose[k], st)
                        r_ms, img_r = frame_ms(h, cam, cfg)
                    row["frame_refit_%s_ms" % key] = r_ms
                    row["same_image_%s" % key] = row["same_image_%s" % key] and bool(np.array_equal(img_r, img_f))
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    a = ap.parse_args()
    rows = measure(a)
    lines = ["| precision | create (ms, wall) | rebuild, host arrays (ms, wall) | rebuild_device until it returns (ms, wall) | ... until the scene is ready | ... its device time | update_device (refit) until ready |",
             "|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append("| %s | %.2f | %.2f | %.3f | %.3f | %.3f | %.3f |" % (r["prec"], r["create_wall_ms"], r["rebuild_host_wall_ms"], r["rebuild_device_return_ms"],
                                                                              r["rebuild_device_wall_ms"], r["rebuild_device_device_ms"], r["update_device_wall_ms"]))
    lines += ["", "| precision | scene | pose | fresh host build (ms) | rebuilt tree (ms) | rebuilt / fresh | refitted tree (ms) | same image |", "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        for sc in ("s4", "s5"):
            for k in ("build", "twist"):
                key = "%s_%s" % (sc, k)
                f, b = r["frame_fresh_%s_ms" % key], r["frame_rebuilt_%s_ms" % key]
                refit = r.get("frame_refit_%s_ms" % key)
                lines.append("| %s | %s | %s | %.3f | %.3f | %.3f | %s | %s |" % (r["prec"], sc, k, f, b, b / f, "%.3f" % refit if refit is not None else "", "yes" if r["same_image_%s" % key] else "NO"))
    table = "\n".join(lines)
    print(table)
    if a.out:
        with open(a.out, "w") as f:
            f.write(table + "\n")


if __name__ == "__main__":
    main()
