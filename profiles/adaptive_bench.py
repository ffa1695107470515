"""Adaptive sampling against the plain render at the cap (docs/experiments.md §19): S1 and the S4 mesh scene at 1080p, cap 64 spp, depth 8 / 12, both
precisions, a small grid of tolerances — frame time, share of the cap's samples actually taken, rounds, and the RMSE of the HDR frame against a 1 024-spp
render; the same two figures for spira_render_scene_device_* at spp 64 in the same process, alternating with the adaptive calls.  tolerance = 0 takes the
full sample count through the adaptive path: the price of the machinery.  Needs a GPU; no oracle, no reference checkout.

    python profiles/adaptive_bench.py [--out table.md] [--repeats 7] [--warmup 3] [--width 1920 --height 1080]

Times are host clocks around a call that ends in a stream synchronise (the adaptive entries synchronise once per round themselves), median of the
repeats after the warm-up calls; every (scene, precision) warms up both entries before anything is timed."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "julia-spira_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--cap", type=int, default=64)
    ap.add_argument("--min-spp", type=int, default=8)
    ap.add_argument("--batch-spp", type=int, default=8)
    ap.add_argument("--floor", type=float, default=0.01)
    ap.add_argument("--tolerances", default="0,0.02,0.05,0.1,0.2")
    ap.add_argument("--truth-spp", type=int, default=1024)
    ap.add_argument("--mesh-level", type=int, default=6)
    a = ap.parse_args()
    import torch
    from spira_hip import _binding as B
    from spira_hip import scenes
    assert B.device_count() >= 1, "no HIP device: this is a GPU measurement"
    B.set_device(0)
    W, H = a.width, a.height
    tols = [float(t) for t in a.tolerances.split(",")]
    st = torch.cuda.current_stream()
    rows = []
    for name, s, depth in (("S1", scenes.scene_s1(), 8), ("S4", scenes.scene_s4(level=a.mesh_level), 12)):
        for prec in ("f32", "f64"):
            tdt = torch.float32 if prec == "f32" else torch.float64
            with B.Scene(s["spheres5"], s["materials8"], s.get("triangles10"), prec) as scene:
                d_hdr = torch.empty((3, H, W), dtype=tdt, device="cuda:0")
                d_spp = torch.empty((H, W), dtype=torch.int32, device="cuda:0")
                p = lambda spp: scene.params(W, H, spp, depth, flags=B.POST_NONE, seed=5)

                def plain(spp=a.cap):
                    t0 = time.perf_counter()
                    scene.render_device(s["camera12"], p(spp), d_hdr.data_ptr(), 0, st.cuda_stream)
                    st.synchronize()
                    return (time.perf_counter() - t0) * 1e3

                def adaptive(tol):
                    t0 = time.perf_counter()
                    scene.render_adaptive_device(s["camera12"], p(a.cap), B.make_adaptive(a.min_spp, a.batch_spp, tol, a.floor), d_hdr.data_ptr(), 0, d_spp.data_ptr(), 0, st.cuda_stream)
                    st.synchronize()
                    return (time.perf_counter() - t0) * 1e3
                plain(a.truth_spp)
                truth = d_hdr.double().clone()
                rmse = lambda: float(torch.sqrt(torch.mean((d_hdr.double() - truth) ** 2)))
                for _ in range(a.warmup):
                    plain()
                    adaptive(tols[-1])
                base_ms = []
                for tol in tols:
                    ms = []
                    for _ in range(a.repeats):          # alternating: other people's work shares the host
                        base_ms.append(plain())
                        ms.append(adaptive(tol))
                    c = B.counters()
                    share = float(d_spp.sum().item()) / (a.cap * W * H)
                    assert c["samples"] == int(d_spp.sum().item())
                    rows.append(dict(scene=name, prec=prec, tolerance=tol, ms=float(np.median(ms)), ms_min=float(np.min(ms)), share=share, rounds=int(c["passes"]),
                                     launches=int(c["launches"]), kernel_ms=float(c["kernel_ms"]), rmse=rmse()))
                plain()
                base = dict(scene=name, prec=prec, tolerance=None, ms=float(np.median(base_ms)), ms_min=float(np.min(base_ms)), share=1.0, rounds=1, launches=int(B.counters()["launches"]),
                            kernel_ms=float(B.counters()["kernel_ms"]), rmse=rmse())
                rows.append(base)
                for r in rows[-len(tols) - 1:]:
                    r["time_ratio"] = r["ms"] / base["ms"]
                    print(json.dumps(r), flush=True)
    lines = ["| scene | precision | tolerance | frame ms | x plain | samples taken | passes + rounds | launches | RMSE vs %d spp |" % a.truth_spp, "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append("| %s | %s | %s | %.2f | %.2f | %.3f | %d | %d | %.5f |" % (r["scene"], r["prec"], "plain spp %d" % a.cap if r["tolerance"] is None else "%g" % r["tolerance"],
                                                                          r["ms"], r["time_ratio"], r["share"], r["rounds"], r["launches"], r["rmse"]))
    table = "\n".join(lines)
    print(table)
    if a.out:
        with open(a.out, "w") as f:
            f.write(table + "\n")


if __name__ == "__main__":
    main()
