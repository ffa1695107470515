"""Scene update with a refitted tree against scene creation (docs/experiments.md, "Refit"): the 81 920-triangle mesh of scenes.scene_s4(), both precisions.
(a) what it costs to move the mesh: host wall time of Scene.update (host arrays: it runs on the library's own stream and returns when the scene is ready),
    host wall time and device time of Scene.update_device (a device tensor, events on the caller's stream), beside
    Scene(...) creation of the same moved mesh in the same process — the only way to move a mesh without an update;
(b) what the refitted tree costs a render: the frame of BASELINE configs[4] (1920 x 1080, spp 64, depth 12) through a handle refitted to a deformed mesh,
    beside a fresh handle built on that mesh — a rigid shift, a small sine displacement, and a twist of the whole mesh.
Every figure is the median of the timed calls after the warm-up (the minimum beside it); device times are events on the stream around one call, wall
times bracket the call and a synchronisation.  Both sides of every comparison are printed; nothing is asserted.  Needs a GPU; no oracle.

    python profiles/refit_bench.py [--out table.md] [--repeats 20] [--warmup 3] [--frames 5] [--level 6]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "julia-spira_amd"))


def deformations(tri):
    """name -> triangles10 of the moved mesh; all inside the frame of the tree built on `tri`."""
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
        "shift": put([x + 0.25 * ext, y + 0.1 * ext, z]),
        "sine": put([x + 0.03 * ext * np.sin(12.0 * y / ext), y, z + 0.03 * ext * np.sin(12.0 * x / ext)]),
        "twist": put([np.cos(ang) * x - np.sin(ang) * z, y, np.sin(ang) * x + np.cos(ang) * z]),
    }


def _stats(xs):
    return float(np.median(xs)), float(np.min(xs))


def measure(a):
    import torch
    from spira_hip import _binding as B
    from spira_hip import scenes
    assert B.device_count() >= 1, "no HIP device: this is a GPU measurement"
    B.set_device(0)
    s = scenes.scene_s4(level=a.level)
    st = torch.cuda.current_stream()
    rows = []
    for prec in ("f32", "f64"):
        npdt = np.float32 if prec == "f32" else np.float64
        tdt = torch.float32 if prec == "f32" else torch.float64
        sph, mats = np.ascontiguousarray(s["spheres5"], dtype=npdt), np.ascontiguousarray(s["materials8"], dtype=npdt)
        base = np.ascontiguousarray(s["triangles10"], dtype=npdt)
        moved = {k: np.ascontiguousarray(v, dtype=npdt) for k, v in deformations(np.asarray(s["triangles10"], dtype=np.float64)).items()}
        d_moved = {k: torch.tensor(v, device="cuda:0") for k, v in moved.items()}
        names = list(moved)

        # ---- (a) update against create: the mesh alternates between the deformations, so that no call finds the arrays it left
        def timed(fn, sync):
            wall, dev = [], []
            for i in range(a.warmup + a.repeats):
                k = names[i % len(names)]
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
        with B.Scene(sph, mats, base, prec) as h:
            (uw, uw_min), _ = timed(lambda k: h.update(triangles10=moved[k]), True)
            (dw, dw_min), (dd, dd_min) = timed(lambda k: h.update_device(d_moved[k], st), True)
            (dr, dr_min), _ = timed(lambda k: h.update_device(d_moved[k], st), False)      # wall time until the call RETURNS (one synchronisation inside, the refit enqueued)
        cw = []
        for i in range(a.warmup + a.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hh = B.Scene(sph, mats, moved[names[i % len(names)]], prec)
            t1 = time.perf_counter()
            hh.destroy()
            if i >= a.warmup:
                cw.append((t1 - t0) * 1e3)
        row = dict(prec=prec, triangles=len(base), update_host_wall_ms=uw, update_host_wall_ms_min=uw_min,
                   update_device_wall_ms=dw, update_device_wall_ms_min=dw_min, update_device_device_ms=dd, update_device_device_ms_min=dd_min,
                   update_device_return_ms=dr, update_device_return_ms_min=dr_min, create_wall_ms=_stats(cw)[0], create_wall_ms_min=_stats(cw)[1])

        # ---- (b) the frame of configs[4] through the refitted tree and through a fresh build of the same mesh
        out = torch.empty((3, a.height, a.width), dtype=tdt, device="cuda:0")

        def frame_ms(h):
            p = h.params(a.width, a.height, 64, 12, flags=B.POST_NONE, seed=scenes.seed_for(5))
            ms = []
            for i in range(1 + a.frames):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                h.render_device(s["camera12"], p, out.data_ptr(), 0, st.cuda_stream)
                e1.record(st)
                e1.synchronize()
                if i >= 1:
                    ms.append(e0.elapsed_time(e1))
            return _stats(ms)[0], out.cpu().numpy().copy()
        with B.Scene(sph, mats, base, prec) as h:
            row["render_build_pose_ms"], _ = frame_ms(h)
            for k in names:
                h.update_device(d_moved[k], st)
                row["render_refit_%s_ms" % k], img_r = frame_ms(h)
                with B.Scene(sph, mats, moved[k], prec) as fresh:
                    row["render_fresh_%s_ms" % k], img_f = frame_ms(fresh)
                row["same_image_%s" % k] = bool(np.array_equal(img_r, img_f))
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
    lines = ["| precision | create (ms, wall) | update, host arrays (ms, wall) | update_device until it returns (ms, wall) | ... until the scene is ready | ... its device time |",
             "|---|---|---|---|---|---|"]
    for r in rows:
        lines.append("| %s | %.2f | %.2f | %.3f | %.3f | %.3f |" % (r["prec"], r["create_wall_ms"], r["update_host_wall_ms"],
                                                                         r["update_device_return_ms"], r["update_device_wall_ms"], r["update_device_device_ms"]))
    lines += ["", "| precision | deformation | frame through the refitted tree (ms) | frame through a fresh build (ms) | same image |", "|---|---|---|---|---|"]
    for r in rows:
        lines.append("| %s | (build pose) | %.3f | | |" % (r["prec"], r["render_build_pose_ms"]))
        for k in ("shift", "sine", "twist"):
            lines.append("| %s | %s | %.3f | %.3f | %s |" % (r["prec"], k, r["render_refit_%s_ms" % k], r["render_fresh_%s_ms" % k], "yes" if r["same_image_%s" % k] else "NO"))
    table = "\n".join(lines)
    print(table)
    if a.out:
        with open(a.out, "w") as f:
            f.write(table + "\n")


if __name__ == "__main__":
    main()
