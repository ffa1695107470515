"""Radiance along ray lists against the renderer (docs/experiments.md section 29).  Workloads: S1 (spp 64, depth 8) and BASELINE configs[4] (the 81 920-
triangle mesh of scenes.scene_s4(), spp 64, depth 12) at 1920 x 1080, Float32 and Float64, device tensors throughout, timed with events on one stream.

Run 1  the pinhole ray list traced as 64 calls of spp = 1 (spira_scene_radiance_device_*; the 64 lists generated beforehand, so tracing alone is timed)
       against SPIRA_KERNEL_MEGA and the default organisation rendering the same frame (spira_render_scene_device_*).  Equal bytes are checked first:
       sums / 64 against the renders' out_hdr.  The three alternate inside one process, frame by frame; the figure is the median of the timed frames, with
       min and max beside it; "list again" is the list variant measured a second time in the same rotation: the distance between its two medians is the
       spread a comparison has to beat.  --parent-lib PATH: the two renders also timed in a child process that loads the library at PATH (the parent
       commit's build) — the render kernels are the same source in both, this shows it.
Run 2  the generator alone: milliseconds per 1080p sample, per model.
Run 3  a thin-lens frame (lens radius 0.05) end to end through cameras.render: 64 x (generate + trace), the sums to the host, the division there.
Run 4  where run 1's time goes: the same 64 x 2 M paths as 64 calls of spp = 1 at 64 (the default), 16 and 8 waves per CU (SPIRA_RADIANCE_WAVES_PER_CU: 2, 8
       and 16 paths per lane and launch), and as ONE call of spp = 64 on the sample-0 list (the same rays for every sample — not a camera frame, but the
       same number of paths of the same kind in two launches of 32 samples, through the workspace and k_radiance_sum).
Nothing is asserted except the equal bytes of run 1.  Needs a GPU; no oracle.

    python profiles/radiance_bench.py [--out table.md] [--repeats 7] [--warmup 2] [--parent-lib PATH] [--only s1|c5]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "julia-spira_amd"))

W, H, SPP = 1920, 1080, 64
WORK = {"s1": ("scene_s1", 8, 3), "c5": ("scene_s4", 12, 5)}      # builder, depth, config index of the seed


def _timed(torch, st, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    fn()
    e1.record(st)
    e1.synchronize()
    return e0.elapsed_time(e1)


def _stat(v):
    return (float(np.median(v)), float(np.min(v)), float(np.max(v)))


def measure(a):
    import torch
    from spira_hip import _binding as B
    from spira_hip import cameras, scenes
    if a.renders_only:      # (the child's library is the parent commit's: it predates the entries this script measures, and the child calls none of them)
        B.EXPORTS = [e for e in B.EXPORTS if "radiance" not in e and "camera_rays" not in e]
    assert B.device_count() >= 1, "no HIP device: this is a GPU measurement"
    B.set_device(0)
    st = torch.cuda.current_stream()
    sp = st.cuda_stream
    rows = []
    n = W * H
    for work in ([a.only] if a.only else list(WORK)):
        builder, depth, cfg = WORK[work]
        s = getattr(scenes, builder)()
        seed = scenes.seed_for(cfg)
        for prec in ("f32", "f64"):
            tdt = torch.float32 if prec == "f32" else torch.float64
            npdt = np.float32 if prec == "f32" else np.float64
            cam = s["camera12"]
            with B.Scene(s["spheres5"], s["materials8"], s["triangles10"], prec=prec) as h:
                d_hdr = torch.empty((3, H, W), dtype=tdt, device="cuda:0")
                p_def = h.params(W, H, SPP, depth, flags=B.POST_NONE, seed=seed)
                p_mega = h.params(W, H, SPP, depth, flags=B.POST_NONE | B.KERNEL_MEGA, seed=seed)
                render = lambda p: h.render_device(cam, p, d_hdr.data_ptr(), 0, sp)
                if a.renders_only:
                    ms = {"mega": [], "default": []}
                    for i in range(a.warmup + a.repeats):
                        for name, p in (("mega", p_mega), ("default", p_def)):
                            t = _timed(torch, st, lambda: render(p))
                            if i >= a.warmup:
                                ms[name].append(t)
                    row = dict(run="1-parent", work=work, prec=prec, build=B.build_id(), **{"ms_" + k: _stat(v) for k, v in ms.items()})
                    rows.append(row)
                    print(json.dumps(row), flush=True)
                    continue
                # ---- run 1
                lists = torch.empty((SPP, n, 6), dtype=tdt, device="cuda:0")
                for smp in range(SPP):
                    B.camera_rays_device(cam, B.CAM_PINHOLE, W, H, lists[smp].data_ptr(), sample=smp, seed=seed, stream_ptr=sp, prec=prec)
                d_sums = torch.zeros((n, 3), dtype=tdt, device="cuda:0")

                def trace_lists():
                    d_sums.zero_()
                    for smp in range(SPP):
                        h.radiance_device(lists[smp].data_ptr(), n, 1, depth, d_sums.data_ptr(), seed=seed, sample0=smp, stream_ptr=sp)
                trace_lists()
                st.synchronize()
                frame = (d_sums.cpu().numpy() / npdt(SPP)).reshape(H, W, 3)[::-1]
                frame = np.ascontiguousarray(np.moveaxis(frame, -1, 0))
                same = {}
                for name, p in (("mega", p_mega), ("default", p_def)):
                    render(p)
                    st.synchronize()
                    same[name] = bool(np.array_equal(d_hdr.cpu().numpy(), frame))
                assert all(same.values()), (work, prec, same)
                variants = [("list", trace_lists), ("mega", lambda: render(p_mega)), ("default", lambda: render(p_def)), ("list again", trace_lists)]
                ms = {k: [] for k, _ in variants}
                for i in range(a.warmup + a.repeats):
                    for name, fn in variants:
                        t = _timed(torch, st, fn)
                        if i >= a.warmup:
                            ms[name].append(t)
                res = {k: _stat(v) for k, v in ms.items()}
                gs = lambda k: n * SPP / (res[k][0] * 1e6)
                row = dict(run=1, work=work, prec=prec, same_bytes=same, gsamples_list=gs("list"), gsamples_list_again=gs("list again"), gsamples_mega=gs("mega"),
                           gsamples_default=gs("default"), list_over_mega=res["mega"][0] / res["list"][0], list_over_default=res["default"][0] / res["list"][0],
                           **{"ms_" + k.replace(" ", "_"): v for k, v in res.items()})
                rows.append(row)
                print(json.dumps(row), flush=True)
                # ---- run 4
                def with_waves(wpc, fn):
                    def run():
                        os.environ["SPIRA_RADIANCE_WAVES_PER_CU"] = str(wpc)
                        fn()
                        os.environ.pop("SPIRA_RADIANCE_WAVES_PER_CU", None)
                    return run

                def one_call():
                    d_sums.zero_()
                    h.radiance_device(lists[0].data_ptr(), n, SPP, depth, d_sums.data_ptr(), seed=seed, stream_ptr=sp)
                variants = [("64 x spp 1, 64 waves/CU", trace_lists), ("64 x spp 1, 16 waves/CU", with_waves(16, trace_lists)), ("64 x spp 1, 8 waves/CU", with_waves(8, trace_lists)),
                            ("1 x spp 64, 64 waves/CU", one_call), ("1 x spp 64, 16 waves/CU", with_waves(16, one_call)), ("MEGA", lambda: render(p_mega))]
                ms = {k: [] for k, _ in variants}
                for i in range(1 + max(3, a.repeats // 2)):
                    for name, fn in variants:
                        t = _timed(torch, st, fn)
                        if i >= 1:
                            ms[name].append(t)
                row = dict(run=4, work=work, prec=prec, plan_one_call=B.radiance_plan(n, SPP, 256), **{"ms_" + k: _stat(v) for k, v in ms.items()})
                rows.append(row)
                print(json.dumps(row), flush=True)
                del lists
                # ---- run 2
                if work == "s1":
                    rays = torch.empty((n, 6), dtype=tdt, device="cuda:0")
                    for model, radius in (("CAM_PINHOLE", 0.0), ("CAM_THIN_LENS", 0.05), ("CAM_ORTHO", 0.0)):
                        v = []
                        for i in range(a.warmup + 3 * a.repeats):
                            t = _timed(torch, st, lambda: B.camera_rays_device(cam, getattr(B, model), W, H, rays.data_ptr(), sample=i, seed=seed, lens_radius=radius,
                                                                               stream_ptr=sp, prec=prec))
                            if i >= a.warmup:
                                v.append(t)
                        row = dict(run=2, prec=prec, model=model, ms_per_sample=_stat(v), gbytes_per_s=n * 6 * (4 if prec == "f32" else 8) / (np.median(v) * 1e6))
                        rows.append(row)
                        print(json.dumps(row), flush=True)
                # ---- run 3
                v = []
                for i in range(1 + 3):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    hdr = cameras.render(h, cameras.ThinLens(cam, 0.05), W, H, SPP, depth, seed=seed)
                    v.append((time.perf_counter() - t0) * 1e3)
                row = dict(run=3, work=work, prec=prec, ms_end_to_end=_stat(v[1:]), finite=bool(np.isfinite(hdr).all()), mean=float(hdr.mean()), pinhole_mean=float(frame.mean()))
                rows.append(row)
                print(json.dumps(row), flush=True)
    return rows, B.build_id()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default=None, choices=sorted(WORK))
    ap.add_argument("--parent-lib", default=None, help="libspira_hip.so of the parent commit: its MEGA and default renders are timed in a child process")
    ap.add_argument("--renders-only", action="store_true", help="(the child's mode) time the two renders, nothing else")
    a = ap.parse_args()
    rows, build = measure(a)
    if a.renders_only:
        return
    parent = []
    if a.parent_lib:
        cmd = [sys.executable, os.path.abspath(__file__), "--renders-only", "--repeats", str(a.repeats), "--warmup", str(a.warmup)] + (["--only", a.only] if a.only else [])
        out = subprocess.run(cmd, env=dict(os.environ, SPIRA_HIP_LIB=os.path.abspath(a.parent_lib)), capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
        parent = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    f3 = lambda v: "%.2f (%.2f .. %.2f)" % tuple(v)
    lines = ["build id " + build, "", "Run 1: ms per 1080p spp 64 frame, median (min .. max); Gsamples/s of the median",
             "| workload | precision | list | list again | MEGA | default | list Gs/s | MEGA Gs/s | default Gs/s | list / MEGA | list / default | same bytes |", "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        if r["run"] == 1:
            lines.append("| %s | %s | %s | %s | %s | %s | %.2f | %.2f | %.2f | %.2f | %.2f | %s |" % (
                r["work"], r["prec"], f3(r["ms_list"]), f3(r["ms_list_again"]), f3(r["ms_mega"]), f3(r["ms_default"]), r["gsamples_list"], r["gsamples_mega"], r["gsamples_default"],
                r["list_over_mega"], r["list_over_default"], "yes" if all(r["same_bytes"].values()) else "NO"))
    if parent:
        lines += ["", "The same renders by the parent commit's library (build id %s), a child process" % parent[0]["build"], "| workload | precision | MEGA | default |", "|---|---|---|---|"]
        lines += ["| %s | %s | %s | %s |" % (r["work"], r["prec"], f3(r["ms_mega"]), f3(r["ms_default"])) for r in parent]
    lines += ["", "Run 2: the generator, ms per 1080p sample", "| precision | model | ms | GB/s written |", "|---|---|---|---|"]
    lines += ["| %s | %s | %.4f (%.4f .. %.4f) | %.0f |" % ((r["prec"], r["model"]) + tuple(r["ms_per_sample"]) + (r["gbytes_per_s"],)) for r in rows if r["run"] == 2]
    lines += ["", "Run 3: a thin-lens frame end to end (cameras.render, 64 x (generate + trace), sums to the host), ms", "| workload | precision | ms | mean radiance (pinhole) |", "|---|---|---|---|"]
    lines += ["| %s | %s | %s | %.4f (%.4f) |" % (r["work"], r["prec"], f3(r["ms_end_to_end"]), r["mean"], r["pinhole_mean"]) for r in rows if r["run"] == 3]
    r4 = [r for r in rows if r["run"] == 4]
    if r4:
        names = [k[3:] for k in r4[0] if k.startswith("ms_")]
        lines += ["", "Run 4: the same 64 x 2 M paths, ms per frame", "| workload | precision | " + " | ".join(names) + " |", "|---|---|" + "---|" * len(names)]
        lines += ["| %s | %s | " % (r["work"], r["prec"]) + " | ".join(f3(r["ms_" + k]) for k in names) + " |" for r in r4]
    table = "\n".join(lines)
    print(table)
    if a.out:
        with open(a.out, "w") as f:
            f.write(table + "\n")


if __name__ == "__main__":
    main()
