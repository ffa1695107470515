"""Feature buffers and the denoiser at 1080p (docs/experiments.md §20): S1, both precisions, iterations = 5 — the feature pass at spp 8 and the
denoise call, each timed with events on the stream around one call, median of the timed calls after the warm-up; beside them the plain spp-64 frame
the two are meant to cost less than.  --split adds the per-kernel times from `rocprofv3 --kernel-trace --stats` of a child run of this script;
--renders DIR writes a 640 x 360 before / after pair.  Needs a GPU; no oracle, no reference checkout.

    python profiles/denoise_bench.py [--out table.md] [--repeats 25] [--warmup 5] [--split] [--renders docs/renders]"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "julia-spira_amd"))


def _timed(torch, st, fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        fn()
        e1.record(st)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(np.min(ms))


def measure(a):
    import torch
    from spira_hip import _binding as B
    from spira_hip import denoise as dnz
    from spira_hip import scenes
    assert B.device_count() >= 1, "no HIP device: this is a GPU measurement"
    assert a.repeats >= 20
    B.set_device(0)
    W, H = a.width, a.height
    s = scenes.scene_s1()
    st = torch.cuda.current_stream()
    rows = []
    for prec in ("f32", "f64"):
        tdt = torch.float32 if prec == "f32" else torch.float64
        with B.Scene(s["spheres5"], s["materials8"], None, prec) as scene:
            p = scene.params(W, H, 8, 8, flags=B.POST_NONE, seed=5)
            r = dnz.render_denoised(scene, s["camera12"], p, B.make_adaptive(4, 4, 0.0, 0.0), feature_spp=8)      # the inputs: a noisy spp-8 frame and its guides
            out = torch.empty((3, H, W), dtype=tdt, device="cuda:0")
            frame = torch.empty((3, H, W), dtype=tdt, device="cuda:0")
            dn = B.make_denoise(W, H, a.iterations, B.POST_NONE, 4.0, 0.1)
            feat = lambda: scene.render_features_device(s["camera12"], p, r["albedo"].data_ptr(), r["normal"].data_ptr(), r["depth"].data_ptr(), st.cuda_stream)
            den = lambda: B.denoise_device(r["noisy"].data_ptr(), dn, out.data_ptr(), 0, st.cuda_stream, r["variance"].data_ptr(), r["albedo"].data_ptr(),
                                           r["normal"].data_ptr(), r["depth"].data_ptr(), prec=prec)
            p64 = scene.params(W, H, 64, 8, flags=B.POST_NONE, seed=5)
            plain = lambda: scene.render_device(s["camera12"], p64, frame.data_ptr(), 0, st.cuda_stream)
            row = dict(prec=prec, width=W, height=H, iterations=a.iterations)
            for key, fn in (("features_spp8", feat), ("denoise", den), ("plain_spp64", plain)):
                row[key + "_ms"], row[key + "_ms_min"] = _timed(torch, st, fn, a.warmup, a.repeats)
            row["features_plus_denoise_ms"] = row["features_spp8_ms"] + row["denoise_ms"]
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def kernel_split(a):
    """Per-kernel device time of the new kernels from rocprofv3 --kernel-trace --stats over a child run (the program goes after `--`)."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "denoise", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--inner", "--repeats", str(a.repeats), "--warmup", str(a.warmup),
               "--width", str(a.width), "--height", str(a.height), "--iterations", str(a.iterations)]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=900)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        assert files, "rocprofv3 wrote no kernel_stats.csv"
        out = []
        for row in csv.DictReader(open(files[0])):
            name = row.get("Name", "")
            if "k_features" in name or "k_denoise" in name:
                calls, total_ns = int(row["Calls"]), float(row["TotalDurationNs"])
                out.append(dict(kernel=name.split("(")[0], calls=calls, avg_us=total_ns / calls / 1e3, total_ms=total_ns / 1e6))
        assert out, "no k_features / k_denoise rows in " + files[0]
        return out


def renders(a):
    from spira_hip import _binding as B
    from spira_hip import denoise as dnz
    from spira_hip import scenes
    from spira_hip.png import save_png
    s = scenes.scene_s1()
    W, H = 640, 360
    with B.Scene(s["spheres5"], s["materials8"], None, "f32") as scene:
        p = scene.params(W, H, 8, 8, flags=B.POST_ACES_GAMMA, seed=5)
        r = dnz.render_denoised(scene, s["camera12"], p, B.make_adaptive(4, 4, 0.0, 0.0), feature_spp=8, want_img=True)
        import torch
        torch.cuda.synchronize()
        before = B.tonemap(r["noisy"].cpu().numpy(), B.POST_ACES_GAMMA).reshape(3, H, W)
        save_png(os.path.join(a.renders, "s1_spp8_noisy.png"), before.transpose(1, 2, 0))
        save_png(os.path.join(a.renders, "s1_spp8_denoised.png"), r["img"].cpu().numpy().transpose(1, 2, 0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--split", action="store_true")
    ap.add_argument("--renders", default=None)
    ap.add_argument("--inner", action="store_true", help="(the child run under rocprofv3)")
    a = ap.parse_args()
    if a.inner:
        measure(a)
        return
    split = kernel_split(a) if a.split else []      # (first: the profiler's child is the only process on the device while it runs)
    rows = measure(a)
    lines = ["| precision | features spp 8 (ms) | denoise, %d iterations (ms) | features + denoise (ms) | plain spp-64 frame (ms) |" % a.iterations, "|---|---|---|---|---|"]
    for r in rows:
        lines.append("| %s | %.3f | %.3f | %.3f | %.3f |" % (r["prec"], r["features_spp8_ms"], r["denoise_ms"], r["features_plus_denoise_ms"], r["plain_spp64_ms"]))
    if split:
        lines += ["", "| kernel | calls | average (us) | total (ms) |", "|---|---|---|---|"]
        lines += ["| `%s` | %d | %.1f | %.2f |" % (k["kernel"], k["calls"], k["avg_us"], k["total_ms"]) for k in split]
    table = "\n".join(lines)
    print(table)
    if a.out:
        with open(a.out, "w") as f:
            f.write(table + "\n")
    if a.renders:
        renders(a)


if __name__ == "__main__":
    main()
