"""Lockstep host emulation of drain_unit_sphere_list (csrc/spira_device.h; docs/experiments.md §21): 64 lanes, the kernel's statements one by one with the real
hash, against the serial loop — lists of the native test's lengths, MAXT 64, 1, 2, 3, 5, 7; every slot must be written exactly once.  Also: the integer
accept test against the Float64 one on 2e6 random draws.  (No substitute for tests/native/rnd_list.hip: it checks the rule, not the compiled code.)"""
import numpy as np, sys
M32 = 0xFFFFFFFF
def mix32(x):
    x = np.asarray(x, dtype=np.uint64) & M32
    x ^= x >> 16; x = (x * 0x7feb352d) & M32
    x ^= x >> 15; x = (x * 0x846ca68b) & M32
    x ^= x >> 16
    return x
def words(hA, hB, t):
    hBr = ((hB << 16) | (hB >> 16)) & M32
    a = mix32(((hA + t * 0x9E3779B9) & M32) ^ hBr)
    b = mix32((a + hB) & M32)
    return a, b
def ms(a, b):
    return (a >> 11).astype(np.int64), (b >> 11).astype(np.int64), (((a & 0x7FF) << 10) | (b & 0x3FF)).astype(np.int64)
def acc_int(a, b):
    m0, m1, m2 = ms(a, b)
    k0, k1, k2 = m0 - (1 << 20), m1 - (1 << 20), m2 - (1 << 20)
    return (k0 * k0 + k1 * k1 + k2 * k2) < (1 << 40)
def acc_f64(a, b):
    m0, m1, m2 = ms(a, b)
    s = 1.0 / 1048576.0
    c0, c1, c2 = m0 * s - 1.0, m1 * s - 1.0, m2 * s - 1.0
    return (c0 * c0 + c1 * c1 + c2 * c2) < 1.0
def serial(hA, hB, maxt):
    for t in range(1, maxt + 1):
        a, b = words(np.uint64(hA), np.uint64(hB), t)
        if acc_int(a, b): return (int(a), int(b))
    return (0x80000400, 0x80000000)
def popc(x): return bin(x).count("1")
def drain(keys, maxt):
    n = len(keys)
    slot = [dict(k=keys[i] if i < n else None, res=None, tab=None) for i in range(128)]
    lane = list(range(64))
    e = list(range(64)); t = [1] * 64; nxt = 64
    have = [x < n for x in e]
    k = [slot[x]["k"] if have[i] else (0, 0) for i, x in enumerate(e)]
    def draw(i, tt):
        a, b = words(np.uint64(k[i][0]), np.uint64(k[i][1]), tt)
        return bool(acc_int(a, b)), (int(a), int(b))
    iters = 0
    pm = [i for i in lane if have[i]]
    while pm and (nxt < n or len(pm) > 32):
        iters += 1
        done = [False] * 64
        for i in lane:
            if have[i]:
                d, r = draw(i, t[i])
                if not d and t[i] == maxt: r = (0x80000400, 0x80000000); d = True
                if d:
                    assert slot[e[i]]["res"] is None; slot[e[i]]["res"] = r
                t[i] += 1
                done[i] = d
        m = [i for i in lane if done[i]]
        for i in m:
            e[i] = nxt + sum(1 for x in m if x < i); t[i] = 1
            have[i] = e[i] < n
            if have[i]: k[i] = slot[e[i]]["k"]
        nxt += len(m)
        pm = [i for i in lane if have[i]]
    p = len(pm); lg = None
    lead = list(have)
    while p:
        iters += 1
        cl = 32 - (32 - (p - 1).bit_length()) if p > 1 else 0       # 32 - clz(p-1)
        lg_new = min(5, 6 - cl)
        if lg_new != lg:
            lg = lg_new
            for i in lane:
                if lead[i]: slot[sum(1 for x in pm if x < i)]["tab"] = e[i] | (t[i] << 16)
            for i in lane:
                grp = i >> lg
                have[i] = grp < p
                if have[i]:
                    w = slot[grp]["tab"]; e[i] = w & 0xFFFF; t[i] = w >> 16; k[i] = slot[e[i]]["k"]
        g = 1 << lg
        assert g * p <= 64
        acc = [False] * 64; r = [None] * 64
        for i in lane:
            j = i & (g - 1)
            if have[i] and t[i] + j <= maxt: acc[i], r[i] = draw(i, t[i] + j)
        mbits = sum(1 << i for i in lane if acc[i])
        newhave = list(have)
        for i in lane:
            j = i & (g - 1)
            half = (mbits & M32) if i < 32 else (mbits >> 32)
            field = (half >> ((i & 31) - j)) & (M32 >> (32 - g))
            if acc[i] and (field & ((1 << j) - 1)) == 0:
                assert slot[e[i]]["res"] is None; slot[e[i]]["res"] = r[i]
            over = field == 0 and t[i] + g > maxt
            if have[i] and over and j == 0:
                assert slot[e[i]]["res"] is None; slot[e[i]]["res"] = (0x80000400, 0x80000000)
            newhave[i] = have[i] and field == 0 and not over
            t[i] += g
            lead[i] = newhave[i] and j == 0
        have = newhave
        pm = [i for i in lane if lead[i]]
        p = len(pm)
    return [s["res"] for s in slot[:n]], iters
rng = np.random.default_rng(1)
# int test == float64 test on many draws, including boundary-ish
a = rng.integers(0, 1 << 32, 2_000_000, dtype=np.uint64); b = rng.integers(0, 1 << 32, 2_000_000, dtype=np.uint64)
assert np.array_equal(acc_int(a, b), acc_f64(a, b)); print("int == f64 accept on 2e6 draws, accept rate %.4f" % acc_int(a, b).mean())
# sentinel converts to zero
m0, m1, m2 = ms(np.uint64(0x80000400), np.uint64(0x80000000)); assert m0 == m1 == m2 == 1 << 20
bad = 0
for maxt in (64, 1, 2, 3, 5, 7):
    ex = ok = 0
    for n in (0, 1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128):
        for rep in range(6):
            keys = [(int(x), int(y)) for x, y in rng.integers(0, 1 << 32, (n, 2), dtype=np.uint64)]
            got, it = drain(keys, maxt)
            want = [serial(x, y, maxt) for x, y in keys]
            if got != want: bad += 1; print("MISMATCH", maxt, n)
            ex += sum(1 for w in want if w == (0x80000400, 0x80000000)); ok += sum(1 for w in want if w != (0x80000400, 0x80000000))
    print("MAXT", maxt, "exhausted", ex, "accepted", ok)
print("bad", bad)
