"""Light probes (spira_scene_probe_sh_*) against the routes a caller had for the same samples (docs/experiments.md section 46).  The scene is the
81 920-triangle mesh of scenes.scene_s4(); the probes are one per triangle, the centroid pushed 1 % of the mesh's extent along the triangle's normal,
and that list tiled (--tile: the list repeated, every copy under its own keys); spp 64, depth 8, Float32 and Float64, device tensors throughout, events on
one stream.

    probe        ONE spira_scene_probe_sh_device_* call of spp 64: k_probe + k_probe_sum
    gather       ONE spira_scene_gather_device_* call of spp 64 on the same points with their normals: the hemisphere walk, 3 sums per point instead of 27
                 (k_gather and k_gather_sum are byte for byte the parent commit's: this is the parent's figure, taken in the same rotation)
    list         64 x (spira_probe_rays_device_* + spira_scene_radiance_device_* at one sample per ray into a zeroed [n, 3] + the projection in torch:
                 the unit direction, the nine basis values, sums += Y L) — the route without the entry
    gather down  the same gather with every normal reversed: the hemisphere that faces the mesh.  A probe's sphere is both hemispheres; the two gathers
                 (cosine-weighted, not uniform: an indication, not a decomposition) show which half the probe's time goes to
    direct       ONE probe call of spp 64 with SPIRA_GATHER_MAX_ITEMS = n: 64 passes of one sample per point, k_probe alone, the owning lanes doing the
                 27 read-modify-writes — no workspace and no k_probe_sum; the other organisation of the same bytes (a pass holds n items only, so
                 small lists leave most of the device idle: not the entry's default for a reason)
Equal bytes are checked first: the probe's sums against the list route's (the torch projection is written in the entry's order of operations) and
against the 64 direct passes.  The variants alternate inside one process, call by call; the figure is the median of the timed calls with min and max
beside it; "probe again" is the probe a second time in the same rotation: the distance between its two medians is the spread a comparison has to beat.
The split between k_probe and k_probe_sum inside one call comes from a kernel trace of this script (--once runs one probe call per precision and tile and
nothing else, for `rocprofv3 --kernel-trace --stats -- python profiles/probe_bench.py --once`): two launches of one entry cannot be bracketed by events
from outside it.  Nothing else is asserted.  Needs a GPU; no oracle.

    python profiles/probe_bench.py [--out table.md] [--repeats 15] [--warmup 3] [--level 6] [--tile 1,16] [--once]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "julia-spira_amd"))

SPP, DEPTH, SEED = 64, 8, 5


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


def _project(torch, bake, d_rays, d_L, d_sums, tdt):
    """sums[k][j][c] += Y_j(d) L[c] in the entry's order of operations: d = v / sqrt((vx vx + vy vy) + vz vz), sh9_basis, one product, one addition."""
    v = d_rays[:, 3:6]
    s = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
    d = v / torch.sqrt(s)[:, None]
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    c0, c1, c2, c3, c4 = (torch.tensor(c, dtype=tdt, device=d.device) for c in bake.SH9_C)
    one, three = torch.tensor(1.0, dtype=tdt, device=d.device), torch.tensor(3.0, dtype=tdt, device=d.device)
    Y = torch.stack([c0.expand_as(x), c1 * y, c1 * z, c1 * x, c2 * (x * y), c2 * (y * z), c3 * (three * (z * z) - one), c2 * (x * z), c4 * (x * x - y * y)], dim=1)
    d_sums.add_(Y[:, :, None] * d_L[:, None, :])


def measure(a):
    import torch
    from spira_hip import _binding as B
    from spira_hip import bake, scenes
    assert B.device_count() >= 1, "no HIP device: this is a GPU measurement"
    B.set_device(0)
    st = torch.cuda.current_stream()
    sp = st.cuda_stream
    s = scenes.scene_s4(level=a.level)
    base6 = bake.triangle_points(s["triangles10"])
    v = np.asarray(s["triangles10"], dtype=np.float64)[:, :9].reshape(-1, 3)
    extent = float((v.max(axis=0) - v.min(axis=0)).max())
    base6[:, 0:3] += 0.01 * extent * base6[:, 3:6]
    rows = []
    for prec in ("f32", "f64"):
        tdt = torch.float32 if prec == "f32" else torch.float64
        npdt = np.float32 if prec == "f32" else np.float64
        with B.Scene(s["spheres5"], s["materials8"], s["triangles10"], prec=prec) as h:
            for tile in a.tile:
                pts6 = np.ascontiguousarray(np.tile(base6, (tile, 1)), dtype=npdt)
                n = len(pts6)
                d_pts6 = torch.tensor(pts6, device="cuda:0")
                d_pts3 = d_pts6[:, 0:3].contiguous()
                d_sh = torch.zeros((n, 9, 3), dtype=tdt, device="cuda:0")
                d_sums = torch.zeros((n, 3), dtype=tdt, device="cuda:0")
                d_L = torch.zeros((n, 3), dtype=tdt, device="cuda:0")
                d_rays = torch.empty((n, 6), dtype=tdt, device="cuda:0")

                def probe():
                    d_sh.zero_()
                    h.probe_sh_device(d_pts3.data_ptr(), n, SPP, DEPTH, d_sh.data_ptr(), seed=SEED, stream_ptr=sp)
                if a.once:
                    probe(); st.synchronize()
                    continue

                def probe_direct():
                    os.environ["SPIRA_GATHER_MAX_ITEMS"] = str(n)
                    try:
                        probe()
                    finally:
                        del os.environ["SPIRA_GATHER_MAX_ITEMS"]

                def gather():
                    d_sums.zero_()
                    h.gather_device(d_pts6.data_ptr(), n, SPP, DEPTH, d_sums.data_ptr(), seed=SEED, stream_ptr=sp)

                d_down6 = d_pts6.clone()
                d_down6[:, 3:6] *= -1

                def gather_down():
                    d_sums.zero_()
                    h.gather_device(d_down6.data_ptr(), n, SPP, DEPTH, d_sums.data_ptr(), seed=SEED, stream_ptr=sp)

                def route_list():
                    d_sh.zero_()
                    for smp in range(SPP):
                        B.probe_rays_device(d_pts3.data_ptr(), n, d_rays.data_ptr(), smp, SEED, 0, sp, prec)
                        d_L.zero_()
                        h.radiance_device(d_rays.data_ptr(), n, 1, DEPTH, d_L.data_ptr(), seed=SEED, sample0=smp, stream_ptr=sp)
                        _project(torch, bake, d_rays, d_L, d_sh, tdt)
                probe(); st.synchronize(); ref = d_sh.cpu().numpy()
                route_list(); st.synchronize(); same_list = bool(np.array_equal(d_sh.cpu().numpy(), ref))
                probe_direct(); st.synchronize(); same_direct = bool(np.array_equal(d_sh.cpu().numpy(), ref))
                res = _rotate(torch, st, [("probe", probe), ("gather", gather), ("gather down", gather_down), ("list", route_list), ("direct", probe_direct), ("probe again", probe)], a.warmup, a.repeats)
                gs = lambda k: n * SPP / (res[k][0] * 1e6)
                row = dict(prec=prec, tile=tile, points=n, same_bytes_list=same_list, same_bytes_direct=same_direct, plan=B.gather_plan(n, SPP, 256),
                           gsamples_probe=gs("probe"), gsamples_probe_again=gs("probe again"), gsamples_gather=gs("gather"), gsamples_list=gs("list"),
                           gsamples_gather_down=gs("gather down"), gsamples_direct=gs("direct"), probe_over_list=res["list"][0] / res["probe"][0], probe_rate_over_gather=gs("probe") / gs("gather"),
                           mean_y0_sum=float(ref[:, 0].mean()), **{"ms_" + k.replace(" ", "_"): v for k, v in res.items()})
                rows.append(row)
                print(json.dumps(row), flush=True)
    return rows, B.build_id()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--tile", default="1,16", help="comma-separated multiples of the 81 920-point list")
    ap.add_argument("--once", action="store_true", help="one probe call per precision and tile, nothing timed: the run a kernel trace is taken of")
    a = ap.parse_args()
    a.tile = [int(x) for x in a.tile.split(",")]
    rows, build = measure(a)
    if a.once:
        return
    f3 = lambda v: "%.3f (%.3f .. %.3f)" % tuple(v)
    lines = ["build id " + build, "", "ms per call of points x spp 64, depth 8, median (min .. max); Gsamples/s of the median",
             "| precision | points | probe | probe again | gather (hemisphere, 3 sums) | gather, normals reversed | list (generate + trace + project) | 64 direct passes | bytes = list / direct | probe Gs/s | gather Gs/s | gather down Gs/s | list Gs/s | probe / list | probe rate / gather |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append("| %s | %d | %s | %s | %s | %s | %s | %s | %s / %s | %.2f | %.2f | %.2f | %.2f | %.2f | %.2f |" % (
            r["prec"], r["points"], f3(r["ms_probe"]), f3(r["ms_probe_again"]), f3(r["ms_gather"]), f3(r["ms_gather_down"]), f3(r["ms_list"]), f3(r["ms_direct"]),
            r["same_bytes_list"], r["same_bytes_direct"], r["gsamples_probe"], r["gsamples_gather"], r["gsamples_gather_down"], r["gsamples_list"], r["probe_over_list"],
            r["probe_rate_over_gather"]))
    table = "\n".join(lines)
    print(table)
    if a.out:
        with open(a.out, "w") as f:
            f.write(table + "\n")


if __name__ == "__main__":
    main()
