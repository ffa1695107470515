"""Hemisphere gather at surface points against the routes the ray-list entries offer for the same samples (docs/experiments.md section 30).  The scene is
the 81 920-triangle mesh of scenes.scene_s4(); the points are bake.triangle_points of it (one per triangle), optionally tiled (--tile: the list repeated,
every copy under its own keys — a lightmap of tile x 81 920 texels); spp 64, depth 8, Float32 and Float64, device tensors throughout, events on one stream.

Radiance   gather       ONE spira_scene_gather_device_* call of spp 64
           list         64 x (spira_gather_rays_device_* + spira_scene_radiance_device_* at one sample per ray) — the route without the gather
           list traced  the same with the 64 lists generated beforehand: tracing alone
           one list     ONE spira_scene_radiance_device_* call of spp 64 on the sample-0 list (the same ray for every sample of a point: not a gather, but
                        k_radiance's many-samples-per-call case on rays of this kind — the case docs/experiments.md section 29 found at MEGA's rate on camera rays)
           MEGA         SPIRA_KERNEL_MEGA rendering 1920 x 1080 at spp 64, depth 8 on the same scene in the same rotation: the rate to compare with
           MEGA close   the same with the camera of scenes.scene_s5() (same objects, the mesh covering 70 % of the frame instead of 0.7 %): nearly every
                        camera path walks the tree, as every gathered path does
Visibility gather       ONE spira_scene_gather_visible_device_* call of spp 64 (t_max = a quarter of the mesh's extent), sessions and in place
           list         64 x spira_scene_occluded_device_* on the 64 generated [p t_min v t_max] lists (generated beforehand: tracing alone)
Equal bytes are checked first: the gather's sums against the list route's, the counts against the number of zeros the occlusion lists give.  The
variants alternate inside one process, call by call; the figure is the median of the timed calls with min and max beside it; "gather again" is the
gather a second time in the same rotation: the distance between its two medians is the spread a comparison has to beat.  Nothing else is asserted.
Needs a GPU; no oracle.

    python profiles/gather_bench.py [--out table.md] [--repeats 15] [--warmup 3] [--level 6] [--tile 1,16]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "julia-spira_amd"))

SPP, DEPTH, SEED = 64, 8, 5
W, H = 1920, 1080


def _timed(torch, st, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    fn()
    e1.record(st)
    e1.synchronize()
    return e0.elapsed_time(e1)


def _stat(v):
    return (float(np.median(v)), float(np.min(v)), float(np.max(v)))


def _rotate(torch, st, variants, warmup, repeats):
    ms = {k: [] for k, _ in variants}
    for i in range(warmup + repeats):
        for name, fn in variants:
            t = _timed(torch, st, fn)
            if i >= warmup:
                ms[name].append(t)
    return {k: _stat(v) for k, v in ms.items()}


def measure(a):
    import torch
    from spira_hip import _binding as B
    from spira_hip import bake, scenes
    assert B.device_count() >= 1, "no HIP device: this is a GPU measurement"
    B.set_device(0)
    st = torch.cuda.current_stream()
    sp = st.cuda_stream
    s = scenes.scene_s4(level=a.level)
    base = bake.triangle_points(s["triangles10"])
    v = np.asarray(s["triangles10"], dtype=np.float64)[:, :9].reshape(-1, 3)
    t_max = 0.25 * float((v.max(axis=0) - v.min(axis=0)).max())
    rows = []
    for prec in ("f32", "f64"):
        tdt = torch.float32 if prec == "f32" else torch.float64
        npdt = np.float32 if prec == "f32" else np.float64
        with B.Scene(s["spheres5"], s["materials8"], s["triangles10"], prec=prec) as h:
            d_hdr = torch.empty((3, H, W), dtype=tdt, device="cuda:0")
            p_mega = h.params(W, H, SPP, DEPTH, flags=B.POST_NONE | B.KERNEL_MEGA, seed=SEED)
            mega = lambda: h.render_device(s["camera12"], p_mega, d_hdr.data_ptr(), 0, sp)
            cam_close = scenes.scene_s5(level=0)["camera12"]
            mega_close = lambda: h.render_device(cam_close, p_mega, d_hdr.data_ptr(), 0, sp)
            for tile in a.tile:
                pts = np.ascontiguousarray(np.tile(base, (tile, 1)), dtype=npdt)
                n = len(pts)
                d_pts = torch.tensor(pts, device="cuda:0")
                d_sums = torch.zeros((n, 3), dtype=tdt, device="cuda:0")
                d_rays = torch.empty((n, 6), dtype=tdt, device="cuda:0")
                lists = torch.empty((SPP, n, 6), dtype=tdt, device="cuda:0")
                for smp in range(SPP):
                    B.gather_rays_device(d_pts.data_ptr(), n, lists[smp].data_ptr(), smp, SEED, 0, sp, prec)

                def gather():
                    d_sums.zero_()
                    h.gather_device(d_pts.data_ptr(), n, SPP, DEPTH, d_sums.data_ptr(), seed=SEED, stream_ptr=sp)

                def route_list():
                    d_sums.zero_()
                    for smp in range(SPP):
                        B.gather_rays_device(d_pts.data_ptr(), n, d_rays.data_ptr(), smp, SEED, 0, sp, prec)
                        h.radiance_device(d_rays.data_ptr(), n, 1, DEPTH, d_sums.data_ptr(), seed=SEED, sample0=smp, stream_ptr=sp)

                def route_traced():
                    d_sums.zero_()
                    for smp in range(SPP):
                        h.radiance_device(lists[smp].data_ptr(), n, 1, DEPTH, d_sums.data_ptr(), seed=SEED, sample0=smp, stream_ptr=sp)

                def one_list():
                    d_sums.zero_()
                    h.radiance_device(lists[0].data_ptr(), n, SPP, DEPTH, d_sums.data_ptr(), seed=SEED, stream_ptr=sp)
                gather(); st.synchronize(); ref = d_sums.cpu().numpy()
                route_list(); st.synchronize(); same_list = bool(np.array_equal(d_sums.cpu().numpy(), ref))
                route_traced(); st.synchronize(); same_traced = bool(np.array_equal(d_sums.cpu().numpy(), ref))
                assert same_list and same_traced, (prec, tile, same_list, same_traced)
                res = _rotate(torch, st, [("gather", gather), ("list", route_list), ("list traced", route_traced), ("one list", one_list), ("MEGA", mega), ("MEGA close", mega_close),
                                          ("gather again", gather)], a.warmup, a.repeats)
                gs = lambda k, items=n * SPP: items / (res[k][0] * 1e6)
                row = dict(run="radiance", prec=prec, tile=tile, points=n, same_bytes=True, plan=B.gather_plan(n, SPP, 256),
                           gsamples_gather=gs("gather"), gsamples_gather_again=gs("gather again"), gsamples_list=gs("list"), gsamples_list_traced=gs("list traced"),
                           gsamples_one_list=gs("one list"), gsamples_mega=gs("MEGA", W * H * SPP), gsamples_mega_close=gs("MEGA close", W * H * SPP), gather_over_list=res["list"][0] / res["gather"][0],
                           gather_rate_over_mega=gs("gather") / gs("MEGA", W * H * SPP), gather_rate_over_mega_close=gs("gather") / gs("MEGA close", W * H * SPP), list_rate_over_mega=gs("list") / gs("MEGA", W * H * SPP),
                           mean_sum=float(ref.mean()), **{"ms_" + k.replace(" ", "_"): v for k, v in res.items()})
                rows.append(row)
                print(json.dumps(row), flush=True)
                del lists
                # ---- visibility
                d_counts = torch.zeros((n,), dtype=torch.int32, device="cuda:0")
                d_hit = torch.empty((n,), dtype=torch.uint8, device="cuda:0")
                lists8 = torch.empty((SPP, n, 8), dtype=tdt, device="cuda:0")
                for smp in range(SPP):
                    B.gather_rays_device(d_pts.data_ptr(), n, d_rays.data_ptr(), smp, SEED, 0, sp, prec)
                    lists8[smp, :, 0:3] = d_rays[:, 0:3]; lists8[smp, :, 3] = 1e-3; lists8[smp, :, 4:7] = d_rays[:, 3:6]; lists8[smp, :, 7] = t_max
                tot = torch.zeros((n,), dtype=torch.int32, device="cuda:0")

                def vis(inplace):
                    def run():
                        d_counts.zero_()
                        h.gather_visible_device(d_pts.data_ptr(), n, SPP, d_counts.data_ptr(), t_min=1e-3, t_max=t_max, seed=SEED, stream_ptr=sp, inplace=inplace)
                    return run

                def occ_lists(count=False):
                    def run():
                        for smp in range(SPP):
                            h.occluded_device(lists8[smp].data_ptr(), n, d_hit.data_ptr(), sp)
                            if count:
                                tot.add_((d_hit == 0).to(torch.int32))
                    return run
                occ_lists(True)(); st.synchronize(); want = tot.cpu().numpy()
                same = {}
                for name, ip in (("sessions", False), ("in place", True)):
                    vis(ip)(); st.synchronize(); same[name] = bool(np.array_equal(d_counts.cpu().numpy(), want))
                assert all(same.values()), (prec, tile, same)
                res = _rotate(torch, st, [("gather", vis(False)), ("gather in place", vis(True)), ("list", occ_lists()), ("gather again", vis(False))], a.warmup, a.repeats)
                gr = lambda k: n * SPP / (res[k][0] * 1e6)
                row = dict(run="visible", prec=prec, tile=tile, points=n, same_bytes=True, t_max=t_max, visible_fraction=float(want.mean() / SPP),
                           grays_gather=gr("gather"), grays_gather_again=gr("gather again"), grays_gather_in_place=gr("gather in place"), grays_list=gr("list"),
                           gather_over_list=res["list"][0] / res["gather"][0], **{"ms_" + k.replace(" ", "_"): v for k, v in res.items()})
                rows.append(row)
                print(json.dumps(row), flush=True)
                del lists8
    return rows, B.build_id()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--tile", default="1,16", help="comma-separated multiples of the 81 920-point list")
    a = ap.parse_args()
    a.tile = [int(x) for x in a.tile.split(",")]
    rows, build = measure(a)
    f3 = lambda v: "%.3f (%.3f .. %.3f)" % tuple(v)
    lines = ["build id " + build, "", "Radiance: ms per call of points x spp 64, depth 8, median (min .. max); Gsamples/s of the median; MEGA renders 1920 x 1080 spp 64",
             "| precision | points | gather | gather again | list (generate + trace) | list traced | one list, spp 64 | MEGA frame | MEGA close frame | gather Gs/s | list Gs/s | one list Gs/s | MEGA Gs/s | MEGA close Gs/s | gather / list | gather rate / MEGA | / MEGA close | list rate / MEGA |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        if r["run"] == "radiance":
            lines.append("| %s | %d | %s | %s | %s | %s | %s | %s | %s | %.2f | %.2f | %.2f | %.2f | %.2f | %.2f | %.2f | %.2f | %.2f |" % (
                r["prec"], r["points"], f3(r["ms_gather"]), f3(r["ms_gather_again"]), f3(r["ms_list"]), f3(r["ms_list_traced"]), f3(r["ms_one_list"]), f3(r["ms_MEGA"]),
                f3(r["ms_MEGA_close"]), r["gsamples_gather"], r["gsamples_list"], r["gsamples_one_list"], r["gsamples_mega"], r["gsamples_mega_close"], r["gather_over_list"],
                r["gather_rate_over_mega"], r["gather_rate_over_mega_close"], r["list_rate_over_mega"]))
    lines += ["", "Visibility: ms per call of points x spp 64, median (min .. max); Grays/s of the median",
              "| precision | points | visible | gather (sessions) | gather again | gather in place | 64 x occluded on lists | gather Gr/s | in place Gr/s | lists Gr/s | gather / lists |",
              "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        if r["run"] == "visible":
            lines.append("| %s | %d | %.0f %% | %s | %s | %s | %s | %.2f | %.2f | %.2f | %.2f |" % (
                r["prec"], r["points"], 100 * r["visible_fraction"], f3(r["ms_gather"]), f3(r["ms_gather_again"]), f3(r["ms_gather_in_place"]), f3(r["ms_list"]),
                r["grays_gather"], r["grays_gather_in_place"], r["grays_list"], r["gather_over_list"]))
    table = "\n".join(lines)
    print(table)
    if a.out:
        with open(a.out, "w") as f:
            f.write(table + "\n")


if __name__ == "__main__":
    main()
