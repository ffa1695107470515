"""GPU: the trees the device refits (spira_scene_update_*: k_refit_check, k_refit_tris, k_refit_level) and builds (spira_scene_rebuild_*: k_lbvh_check, _keys,
_sort_tile, _sort_wide, _radix, _boxes, _make, _scan, _write, _commit, then the refit passes) against the host twin, BYTE FOR BYTE.  spira_refit.h and
spira_lbvh.h state it: "host and device agree bit for bit, and nothing here depends on the order in which lanes run".  A render cannot check that sentence —
the tree only prunes, so boxes that are too large, a degenerate but valid topology or a level table out of step with the nodes all render the right image.
Here every case applies a chain of steps to a handle through the real entry points, reads the handle's tree back after every step
(spira_debug_scene_tree: summary, node array, frame packets + triangle records, screening records) and demands numpy.array_equal with what the twin
program (tests/native/tree_twin_dump.cpp: the same header functions run serially, std::stable_sort for the device's pair sort) wrote for the same chain.
No tolerance and no masked byte anywhere.  What a case is there to reach (a sort-tile edge, a level of more than 1024 nodes, a node array that has to
grow, a run of equal keys across sorted position 1024) is asserted from the twin's output, so a case that stops reaching its branch fails."""
import bisect
import ctypes as C

import numpy as np
import pytest

from spira_hip import scenes

import test_gpu_rebuild as RB          # deform() and the awkward meshes
import tree_twin_support as TW

pytestmark = pytest.mark.gpu

SORT_TILE = 1024          # kLbvhSortTile
SCAN_BLOCK = 1024         # kLbvhScanBlock: k_lbvh_scan takes a level in chunks of this many nodes
_cache = {}


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    """The twin program, compiled once per module; twin(name, prec, chain, screen) -> the steps it wrote (cached per name)."""
    d = tmp_path_factory.mktemp("tree_bytes")
    exe = TW.build_dump(d)
    done = {}

    def run(name, prec, chain, screen=False):
        key = (name, prec, screen)
        if key not in done:
            done[key] = TW.run_dump(exe, d, "%s_%s_%d" % (name, prec, screen), prec, 3, screen, chain)[0]
        return done[key]
    return run


def _scene():
    if "s4" not in _cache:
        _cache["s4"] = scenes.scene_s4(level=3)
    return _cache["s4"]


def _tensor(tri, prec):
    import torch
    return torch.tensor(np.ascontiguousarray(tri, dtype=TW.npdt(prec)), device="cuda:0").contiguous()


# ---- the read-back
def _fn(gpu):
    fn = gpu.lib().spira_debug_scene_tree
    fn.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    fn.restype = C.c_int
    return fn


def _read(gpu, h):
    """The four blobs of handle h, as uint8 arrays by name."""
    out = {}
    for what, name in enumerate(TW.BLOBS):
        need = C.c_uint64(0xDEAD)
        rc = _fn(gpu)(h._h, what, None, 0, C.byref(need))
        if name == "screen" and need.value == 0:
            assert rc == 0
            out[name] = np.zeros(0, dtype=np.uint8)
            continue
        assert rc == -1 and 0 < need.value < (1 << 32), (name, rc, need.value)          # (nothing is copied into no buffer: the size comes back)
        buf = np.empty(need.value, dtype=np.uint8)
        need2 = C.c_uint64(0)
        rc = _fn(gpu)(h._h, what, buf.ctypes.data_as(C.c_void_p), buf.size, C.byref(need2))
        assert rc == 0 and need2.value == need.value, (name, rc, gpu.lib().spira_last_error())
        out[name] = buf
    return out


# ---- the comparison
def _hex(words):
    return " ".join("%08x" % int(x) for x in words)


def _leaf_slot(nodes, rec):
    """The slot (in the twin's node array) whose leaves include triangle position rec, or None."""
    b = nodes.copy().view(np.uint8).reshape(-1, 80)
    present = ~((b[:, 32:40] == 255) & (b[:, 56:64] == 0))
    imask = (nodes[:, 3] >> 24)[:, None] >> np.arange(8) & 1
    n_leaf = (present & (imask == 0)).sum(axis=1)
    hit = np.nonzero((n_leaf > 0) & (nodes[:, 5] <= rec) & (rec < nodes[:, 5] + n_leaf))[0]
    return int(hit[0]) if len(hit) else None


def _difference(name, got, want, want_blobs):
    """None when the blobs are equal, else the message: the blob, the first differing slot or record, its level and both values in hex."""
    if got.dtype == want.dtype and np.array_equal(got, want):
        return None
    if len(got) != len(want):
        return "%s: the device holds %d bytes, the twin %d" % (name, len(got), len(want))
    sm = TW.summary(want_blobs["summary"])
    level = lambda slot: bisect.bisect_right(sm.level_first, slot) - 1
    if name == "summary":
        g, w = got.view(np.uint32), want.view(np.uint32)
        i = int(np.nonzero(g != w)[0][0])
        return "summary: dword %d (0-3 precision n slots depth, 4-11 centre and scale, 12.. level_first): device %s, twin %s" % (i, _hex(g), _hex(w))
    if name == "nodes":
        g, w = got.view(np.uint32).reshape(-1, TW.NODE_DWORDS), want.view(np.uint32).reshape(-1, TW.NODE_DWORDS)
        rows = np.nonzero((g != w).any(axis=1))[0]
        s = int(rows[0])
        return "nodes: %d of %d slots differ; the first is slot %d (level %d of %d), words %s: device %s, twin %s" % (
            len(rows), len(g), s, level(s), sm.depth, [int(k) for k in np.nonzero(g[s] != w[s])[0]], _hex(g[s]), _hex(w[s]))
    words = 4 if name == "screen" else sm.prec
    g, w = got.view(np.uint32).reshape(-1, words), want.view(np.uint32).reshape(-1, words)
    rows = np.nonzero((g != w).any(axis=1))[0]
    p = int(rows[0])
    if name == "records" and p < 3:
        return "records: frame packet %d (0 / 1 the root box, 2 centre and scale; level 0): device %s, twin %s" % (p, _hex(g[p]), _hex(w[p]))
    q = p - 3 if name == "records" else p
    slot = _leaf_slot(want_blobs["nodes"].view(np.uint32).reshape(-1, TW.NODE_DWORDS), q // 3)
    where = "no leaf of the twin's tree" if slot is None else "a leaf of slot %d, level %d of %d" % (slot, level(slot), sm.depth)
    return "%s: %d of %d packets differ; the first is packet %d of record %d (%s): device %s, twin %s" % (name, len(rows), len(g), q % 3, q // 3, where, _hex(g[p]), _hex(w[p]))


def _assert_same(got, want, what):
    for name in TW.BLOBS:
        msg = _difference(name, got[name], want[name], want)
        assert msg is None, "%s: %s" % (what, msg)


def _code(status):
    """The return code of the entry point for the twin's status of a refused step (spira_refit.h: 1 non-finite, 2 material, 4 frame; -4)."""
    return -1 if status > 0 and status & 3 else -4


def _apply(gpu, h, form, tri, prec, keep):
    """One step through the real entry point; the return code (0, or the refusal's)."""
    try:
        if form == "update":
            h.update(triangles10=tri)
        elif form == "rebuild":
            h.rebuild(tri)
        else:
            import torch
            keep.append(_tensor(tri, prec))          # (alive until the handle is read back: the device forms only enqueue)
            torch.cuda.synchronize()
            if "stream" not in _cache:
                _cache["stream"] = torch.cuda.Stream()
            getattr(h, form)(keep[-1], _cache["stream"])          # a stream of its own, never synchronised here: the read-back has to come after it by itself
    except gpu.SpiraError as e:
        return int(str(e).split("error ")[1].split(":")[0])
    return 0


def _chain(gpu, twin, name, prec, first, steps):
    """Create a handle on `first`, apply steps = [(form, triangles10)] (form: update / update_device / rebuild / rebuild_device), read back after every one
    and compare with the twin.  Returns (the twin's steps, the device's blobs per step)."""
    s = _scene()
    chain = [("create", first)] + [(form.replace("_device", ""), tri) for form, tri in steps]
    want = twin(name, prec, chain)                   # on the CPU, before the device is involved
    assert want[0].status == 0
    keep, got = [], []
    with gpu.Scene(s["spheres5"], s["materials8"], first, prec) as h:
        got.append(_read(gpu, h))
        if len(got[0]["screen"]):                    # (a library built with SPIRA_BVH_SCREEN keeps Float32 screening records for Float64 scenes)
            want = twin(name, prec, chain, screen=True)
        _assert_same(got[0], want[0].blobs, "%s %s after create" % (name, prec))
        last = want[0].blobs
        for i, (form, tri) in enumerate(steps, 1):
            rc = _apply(gpu, h, form, tri, prec, keep)
            got.append(_read(gpu, h))
            if want[i].status == 0:
                assert rc == 0, (name, i, form, rc)
                last = want[i].blobs
            else:
                assert rc == _code(want[i].status), (name, i, form, rc, want[i].status)
            _assert_same(got[i], last, "%s %s after step %d (%s)" % (name, prec, i, form))
    return want, got


def _nodes(blobs):
    return blobs["nodes"].view(np.uint32).reshape(-1, TW.NODE_DWORDS)


def _real_nodes_per_level(blobs):
    """Per level, the slots that are nodes (not holes): what one launch of k_lbvh_make / _scan / _write sees."""
    sm = TW.summary(blobs["summary"])
    b = blobs["nodes"].reshape(-1, 80)
    hole = np.all((b[:, 32:40] == 255) & (b[:, 56:64] == 0), axis=1)
    return [int((~hole[a:e]).sum()) for a, e in zip(sm.level_first[:-1], sm.level_first[1:])]


# ---- the cases
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_create(gpu, twin, prec):
    """Upload and layout of bvh_build's own tree: the baseline that makes every later mismatch attributable."""
    A = _scene()["triangles10"]
    want, _ = _chain(gpu, twin, "create", prec, A, [])
    sm = TW.summary(want[0].blobs["summary"])
    print("create", prec, "slots", sm.n_slots, "levels", TW.level_widths(sm))
    assert sm.n == 1280 and sm.depth >= 3


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_refit_a_b_a(gpu, twin, prec):
    """Device refit equals host refit both ways; the third read-back EQUALS the twin's A -> B -> A, so boxes that only ever grow fail here."""
    A = _scene()["triangles10"]
    B = RB.deform(A)
    want, got = _chain(gpu, twin, "refit_aba", prec, A, [("update", B), ("update_device", A), ("update_device", B), ("update", A)])
    assert [w.status for w in want] == [0] * 5
    assert not np.array_equal(want[1].blobs["nodes"], want[2].blobs["nodes"]) and np.array_equal(want[1].blobs["nodes"], want[3].blobs["nodes"])
    assert np.array_equal(got[2]["nodes"], got[4]["nodes"]) and np.array_equal(got[2]["records"], got[4]["records"])      # both forms, either history
    # grow-only boxes would be caught: B's root box holds points A's does not, on some axis
    packet = 16 if prec == "f32" else 32
    root = lambda b: b["records"][:2 * packet].view(TW.npdt(prec)).reshape(2, 4)[:, :3]
    ra, rb = root(want[2].blobs), root(want[1].blobs)
    assert np.any(rb[0] < ra[0]) or np.any(rb[1] > ra[1])


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_refit_after_rebuild(gpu, twin, prec):
    """The refit ranges of an update come from the REBUILT level table (the mesh of test_the_frame_rule_is_gone: an update alone is refused)."""
    A = _scene()["triangles10"]
    c, ext = RB._bounds(A)
    moved = TW.scaled(A, 2.5, [0.0, 3.0 * ext, 0.0])
    want, _ = _chain(gpu, twin, "refit_after_rebuild", prec, A, [("update", moved), ("rebuild", moved), ("update", RB.deform(moved)), ("update_device", moved)])
    assert [w.status for w in want] == [0, 4, 0, 0, 0]
    a, b = TW.summary(want[0].blobs["summary"]), TW.summary(want[2].blobs["summary"])
    assert a.level_first != b.level_first and a.scale != b.scale          # another level table, another frame


def _sort_passes(n):
    """lbvh_sort_schedule for n triangles: (n_pad, the number of `wide` passes of each stage beyond the tile)."""
    n_pad = SORT_TILE
    while n_pad < n:
        n_pad *= 2
    wide, k = [], 2 * SORT_TILE
    while k <= n_pad:
        wide.append(len([j for j in (k >> e for e in range(1, 32)) if j >= SORT_TILE]))
        k *= 2
    return n_pad, wide


SIZES = {33: (1024, []), 1024: (1024, []), 1025: (2048, [1]), 2049: (4096, [1, 2]), 5120: (8192, [1, 2, 3])}


def _sizes_case(n):
    target = TW.soup(n, 100 + n)
    return TW.scaled(target, 0.6), target


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("n", sorted(SIZES))
def test_rebuild_sizes(gpu, twin, prec, n):
    """One sort tile (33, 1024), the first `wide` pass (1025), two `wide` passes in one stage (2049), three (5120); the host form and the device form of a
    rebuild give identical bytes."""
    assert _sort_passes(n) == SIZES[n]
    first, target = _sizes_case(n)
    want, got = _chain(gpu, twin, "sizes%d" % n, prec, first, [("rebuild", target), ("rebuild", first), ("rebuild_device", target)])
    assert [w.status for w in want] == [0] * 4
    for name in TW.BLOBS:
        assert np.array_equal(got[1][name], got[3][name]), name
    assert not np.array_equal(got[1]["nodes"], got[2]["nodes"])
    sm = TW.summary(want[1].blobs["summary"])
    print("sizes", n, prec, "n_pad", SIZES[n][0], "slots", sm.n_slots, "nodes per level", _real_nodes_per_level(want[1].blobs))


def _morton_keys(tri, centre, scale):
    """lbvh_key of spira_lbvh.h in numpy (double arithmetic, nothing fused): the 63-bit keys of the triangles, in their order."""
    t = np.asarray(tri, dtype=np.float64)
    c = np.array(centre, dtype=np.float64)
    m = (((t[:, 0:3] - c) * scale + (t[:, 3:6] - c) * scale) + (t[:, 6:9] - c) * scale) / 3.0
    x = (m + 0.5) * 2097152.0
    x = np.where(x >= 0.0, x, 0.0)
    q = np.minimum(x, 2097151.0).astype(np.uint64)
    keys = np.zeros(len(t), dtype=np.uint64)
    for b in range(21):
        for axis, sh in ((0, 2), (1, 1), (2, 0)):
            keys |= ((q[:, axis] >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b + sh)
    return keys


def _equal_run_case(prec):
    """1500 triangles, 700 .. 1299 copies of one: the copied triangle is chosen so that the run of its key lies across sorted position 1024."""
    key = ("equal_run", prec)
    if key not in _cache:
        base = TW.soup(1500, 7)
        keep = np.r_[0:700, 1300:1500]
        tT = np.ascontiguousarray(base, dtype=TW.npdt(prec))
        v = tT[:, :9].reshape(-1, 3).astype(np.float64)
        lo, hi = v.min(axis=0), v.max(axis=0)
        k = _morton_keys(tT[keep], (lo + hi) / 2.0, 1.0 / (hi - lo).max())          # (any frame close to the real one will do to pick the triangle)
        pick = keep[np.argsort(k, kind="stable")[724]]                              # about 724 of the 900 others sort before it: the run starts near 724
        tri = base.copy()
        tri[700:1300] = base[pick]
        _cache[key] = (TW.scaled(tri, 0.6), tri, int(pick))
    return _cache[key]


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_equal_keys_across_a_tile(gpu, twin, prec):
    """A run of 601 equal keys straddling sorted position 1024 (the edge of the first sort tile), next to distinct keys: the index tie-break of the pair
    sort across tiles, and the 64 + clz(i ^ j) branch of lbvh_delta beside the ordinary one."""
    first, target, pick = _equal_run_case(prec)
    want, _ = _chain(gpu, twin, "equal_run", prec, first, [("rebuild", target), ("rebuild_device", first), ("rebuild_device", target)])
    assert [w.status for w in want] == [0] * 4
    sm = TW.summary(want[1].blobs["summary"])
    keys = _morton_keys(np.ascontiguousarray(target, dtype=TW.npdt(prec)), sm.centre, sm.scale)          # in the twin's frame
    order = np.argsort(keys, kind="stable")
    sk = keys[order]
    run = np.nonzero(sk == keys[700])[0]
    print("equal keys", prec, "run at sorted positions", run[0], "..", run[-1])
    assert len(run) >= 601 and np.array_equal(run, np.arange(run[0], run[-1] + 1)) and run[0] < SORT_TILE - 1 and run[-1] > SORT_TILE
    assert sk[run[0] - 1] != sk[run[0]] and sk[run[-1] + 1] != sk[run[-1]] and len(np.unique(sk)) > 800          # distinct keys on either side
    # the tree order holds every index once
    packet = 16 if prec == "f32" else 32
    w = want[1].blobs["records"][3 * packet:].reshape(-1, 3 * packet)[:, packet - packet // 4:packet]
    idx = w.copy().view(np.uint32 if prec == "f32" else np.uint64).ravel()
    assert np.array_equal(np.sort(idx), np.arange(1500))


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("name", ["copies200", "flat512"])
def test_all_keys_equal_and_flat(gpu, twin, name, prec):
    """200 copies of one triangle (every key equal, every area tie in lbvh_make_node) and a flat grid (a frame axis without extent)."""
    F, T = RB._awkward(name)
    want, _ = _chain(gpu, twin, name, prec, F["triangles10"], [("rebuild", T["triangles10"]), ("rebuild_device", F["triangles10"]), ("update_device", F["triangles10"])])
    assert [w.status for w in want] == [0] * 4
    sm = TW.summary(want[1].blobs["summary"])
    print(name, prec, "slots", sm.n_slots, "levels", TW.level_widths(sm))


def test_wide_level(gpu, twin):
    """scene_s4(level=5), 20 480 triangles, Float32: the twin's rebuilt tree has a level of more than 1024 nodes (asserted below, before the device is
    involved: 2 522 and 3 238 nodes in its two widest levels), so the one workgroup of k_lbvh_scan loops over more than one chunk and carries its running sums across."""
    if "s4_5" not in _cache:
        _cache["s4_5"] = scenes.scene_s4(level=5)["triangles10"]
    A = _cache["s4_5"]
    B = RB.deform(A)
    assert len(A) == 20480
    chain = [("create", A), ("rebuild", B), ("update", A), ("rebuild", A)]
    want = twin("wide", "f32", chain)
    per_level = _real_nodes_per_level(want[1].blobs)
    print("wide level: nodes per level", per_level, "slots", TW.summary(want[1].blobs["summary"]).n_slots)
    assert max(per_level) > SCAN_BLOCK and max(_real_nodes_per_level(want[3].blobs)) > SCAN_BLOCK
    _chain(gpu, twin, "wide", "f32", A, [("rebuild_device", B), ("update_device", A), ("rebuild", A)])


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_slots_grow(gpu, twin, prec):
    """A handle created on a flat grid (bvh_build: few slots) and rebuilt to a soup of the same size that needs more: the node array is reallocated.  Then
    back: the smaller tree sits in the larger allocation."""
    _, flat = RB._awkward("flat512")
    flat = flat["triangles10"]
    c, ext = RB._bounds(flat)
    big = TW.soup(512, 3, centre=c, extent=ext)
    want, _ = _chain(gpu, twin, "slots_grow", prec, flat, [("rebuild", big), ("rebuild_device", flat), ("rebuild", big)])
    assert [w.status for w in want] == [0] * 4
    s0, s1, s2 = (TW.summary(w.blobs["summary"]).n_slots for w in want[:3])
    print("slots grow", prec, s0, "->", s1, "->", s2)
    assert len(want[0].blobs["nodes"]) == s0 * 80
    assert s1 * 80 + 128 > s0 * 80 + 128          # scene_rebuild_impl: nodes_b + 128 > the capacity scene_upload left (the first tree's bytes + 128)
    assert s2 < s1


def test_twice(gpu, twin):
    """The n = 5120 chain on two separate handles in one process: identical bytes from both — the context's scratch, reused across calls, leaves no trace."""
    first, target = _sizes_case(5120)
    steps = [("rebuild", target), ("rebuild", first), ("rebuild_device", target)]
    _, one = _chain(gpu, twin, "sizes5120", "f32", first, steps)
    _, two = _chain(gpu, twin, "sizes5120", "f32", first, steps)
    for a, b in zip(one, two):
        for name in TW.BLOBS:
            assert np.array_equal(a[name], b[name]), name


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_refusals_leave_every_byte(gpu, twin, prec):
    """A NaN array to rebuild and update, an out-of-frame array to update, both forms: every blob after the refusal equals the blob before it."""
    A = np.array(_scene()["triangles10"])
    B = RB.deform(A)
    c, ext = RB._bounds(A)
    nan, oof = A.copy(), A.copy()
    nan[5, 2] = np.nan
    oof[700, 3:6] = c + [0.0, 3.0 * ext, 0.0]
    steps = [("update", B), ("rebuild", nan), ("rebuild_device", nan), ("update", nan), ("update_device", nan), ("update", oof), ("update_device", oof), ("rebuild", B),
             ("update_device", nan), ("update", A)]
    want, got = _chain(gpu, twin, "refusals", prec, A, steps)
    assert [w.status for w in want] == [0, 0, 1, 1, 1, 1, 4, 4, 0, 1, 0]
    for i in (2, 3, 4, 5, 6, 7):
        for name in TW.BLOBS:
            assert np.array_equal(got[i][name], got[1][name]), (i, name)


def test_the_read_back_itself(gpu, twin):
    """The documented return codes; need_bytes is filled; neither the caller's buffer (when it is too small) nor the handle is touched."""
    s = _scene()
    A = s["triangles10"]
    fn = _fn(gpu)
    need = C.c_uint64(77)
    assert fn(None, 1, None, 0, C.byref(need)) == -1 and need.value == 0 and b"NULL or was destroyed" in gpu.lib().spira_last_error()
    with gpu.Scene(s["spheres5"], s["materials8"], A[:12], "f32") as h:
        assert fn(h._h, 1, None, 0, C.byref(need)) == -1 and b"no tree" in gpu.lib().spira_last_error()
    with gpu.Scene(s["spheres5"], s["materials8"], A, "f32", n_devices=1) as h:
        assert fn(h._h, 1, None, 0, C.byref(need)) == -5
    with gpu.Scene(s["spheres5"], s["materials8"], A, "f32") as h:
        before = _read(gpu, h)
        assert fn(h._h, 4, None, 0, C.byref(need)) == -1
        assert fn(h._h, 1, None, 0, None) == -1
        for what, name in enumerate(TW.BLOBS[:3]):
            size = len(before[name])
            buf = np.full(size, 0xA5, dtype=np.uint8)
            need = C.c_uint64(0)
            assert fn(h._h, what, buf.ctypes.data_as(C.c_void_p), size - 1, C.byref(need)) == -1 and need.value == size and np.all(buf == 0xA5), name
            assert fn(h._h, what, buf.ctypes.data_as(C.c_void_p), size, C.byref(need)) == 0 and need.value == size and np.array_equal(buf, before[name]), name
        sm = TW.summary(before["summary"])
        assert len(before["nodes"]) == sm.n_slots * 80 and len(before["records"]) == (3 + 3 * 1280) * 16
        after = _read(gpu, h)
        for name in TW.BLOBS:
            assert np.array_equal(before[name], after[name]), name
        _assert_same(after, twin("create", "f32", [("create", A)], screen=len(after["screen"]) > 0)[0].blobs, "read-back after refusals")


def test_a_handle_that_was_read_back_renders_as_before(gpu):
    """One render at 64 x 36, spp 1: reading a handle's tree back does not alter the handle."""
    s = _scene()
    B = RB.deform(s["triangles10"])
    p = gpu.make_params(64, 36, 1, 5, len(s["spheres5"]), len(s["materials8"]), 1280, seed=11)
    with gpu.Scene(s["spheres5"], s["materials8"], B, "f32") as h:
        want, _ = h.render(s["camera12"], p)
        seg = gpu.counters()["segments"]
    with gpu.Scene(s["spheres5"], s["materials8"], s["triangles10"], "f32") as h:
        _read(gpu, h)
        h.rebuild(B)
        _read(gpu, h)
        got, _ = h.render(s["camera12"], p)
        assert np.array_equal(got, want) and gpu.counters()["segments"] == seg
