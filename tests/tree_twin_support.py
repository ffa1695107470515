"""Shared by tests/test_tree_twin_cpu.py and tests/test_gpu_tree_bytes.py (no test lives here): the host twins of a handle's tree as a program
(tests/native/tree_twin_dump.cpp) — build it, write a job for it, run it, read what it wrote — and the meshes both tests use.

A chain is a list of (kind, triangles10) steps, kind one of "create" / "update" / "rebuild"; the program answers per step with a status and, for a step
it took, the four blobs of spira_debug_scene_tree: summary, nodes, frame packets + triangle records, screening records."""
import collections
import os
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "tree_twin_dump.cpp")
KINDS = {"create": 0, "update": 1, "rebuild": 2}
BLOBS = ("summary", "nodes", "records", "screen")
NODE_DWORDS = 20
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"]
SAN_ENV = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")

Step = collections.namedtuple("Step", "kind status blobs")          # blobs: None for a refused step, else a dict of uint8 arrays by BLOBS name
Summary = collections.namedtuple("Summary", "prec n n_slots depth centre scale level_first")


def npdt(prec):
    return np.float32 if prec == "f32" else np.float64


def build_dump(directory, sanitize=False):
    """g++ -std=c++17 -O2 -ffp-contract=off (the flags the comparison rests on: nothing fused, as in the library); returns the program's path."""
    exe = os.path.join(str(directory), "tree_twin_dump_san" if sanitize else "tree_twin_dump")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-pthread", SRC, "-o", exe] + (SANITIZE if sanitize else []), check=True)
    return exe


def write_job(path, prec, n_materials, screen, chain):
    arrays = [np.ascontiguousarray(tri, dtype=npdt(prec)) for _, tri in chain]      # the conversion the binding makes: round to nearest, once
    n = len(arrays[0])
    assert all(a.shape == (n, 10) for a in arrays)
    with open(path, "wb") as f:
        f.write(b"SPTWJOB1" + struct.pack("<5I", 4 if prec == "f32" else 8, n, n_materials, 1 if screen else 0, len(chain)))
        for (kind, _), a in zip(chain, arrays):
            f.write(struct.pack("<2I", KINDS[kind], 0))
            f.write(a.tobytes())


def read_out(path):
    data = open(path, "rb").read()
    steps, at = [], 0
    while at < len(data):
        kind, status, n_blobs, _ = struct.unpack_from("<IiII", data, at)
        at += 16
        blobs = None
        if n_blobs:
            assert n_blobs == len(BLOBS)
            blobs = {}
            for name in BLOBS:
                (size,) = struct.unpack_from("<Q", data, at)
                blobs[name] = np.frombuffer(data, dtype=np.uint8, count=size, offset=at + 8).copy()
                at += 8 + size
        steps.append(Step({v: k for k, v in KINDS.items()}[kind], status, blobs))
    assert at == len(data)
    return steps


def run_dump(exe, directory, name, prec, n_materials, screen, chain, env=None):
    """The twin's answer to `chain`: (steps, the finished process, the output file's path)."""
    job, out = os.path.join(str(directory), name + ".job"), os.path.join(str(directory), name + ".out")
    write_job(job, prec, n_materials, screen, chain)
    r = subprocess.run([exe, job, out], capture_output=True, text=True, env=dict(os.environ, **(env or {})), timeout=600)
    assert r.returncode == 0, "tree_twin_dump: exit %d\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-6000:])
    steps = read_out(out)
    assert [s.kind for s in steps] == [k for k, _ in chain]
    return steps, r, out


def summary(blob):
    prec, n, n_slots, depth = struct.unpack_from("<4I", blob.tobytes(), 0)
    fr = struct.unpack_from("<4d", blob.tobytes(), 16)
    assert len(blob) == 48 + 4 * (depth + 1)
    lf = list(struct.unpack_from("<%dI" % (depth + 1), blob.tobytes(), 48))
    return Summary(prec, n, n_slots, depth, fr[:3], fr[3], lf)


def level_widths(s):
    return [b - a for a, b in zip(s.level_first[:-1], s.level_first[1:])]


# ---- meshes
def icosphere3():
    """The 1 280-triangle icosphere of the native harnesses: unit sphere moved off the origin, materials 1 .. 3."""
    from spira_hip import scenes
    v, f = scenes.icosphere(3)
    tri = scenes.mesh_triangles10(v + [0.3, 0.0, -2.0], f, 1)
    tri[:, 9] = 1.0 + np.arange(len(tri)) % 3
    return tri


def soup(n, seed, centre=(0.0, 0.0, -1.0), extent=1.0):
    """n small triangles scattered through a box of `extent` about `centre` (in view of scene_s4's camera), materials 1 .. 3."""
    rng = np.random.default_rng(seed)
    c = (rng.random((n, 1, 3)) - 0.5) * extent * np.array([1.0, 0.8, 0.6]) + np.array(centre)
    v = c + (rng.random((n, 3, 3)) - 0.5) * 0.08 * extent
    return np.concatenate([v.reshape(n, 9), (1.0 + np.arange(n) % 3)[:, None]], axis=1)


def scaled(tri, factor, shift=(0.0, 0.0, 0.0)):
    """The mesh scaled about the middle of its bounds and moved by `shift`."""
    t = np.array(tri, dtype=np.float64)
    v = t[:, :9].reshape(-1, 3)
    c = (v.min(axis=0) + v.max(axis=0)) / 2.0
    t[:, :9] = ((v - c) * factor + c + np.array(shift)).reshape(-1, 9)
    return t
