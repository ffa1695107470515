"""Adaptive sampling's stopping rule and schedule, restated in numpy (include/spira_hip.h, "adaptive sampling"; csrc/spira_adaptive.h,
csrc/spira_plan.h).  Every operation is done in the render precision in the written order, so `converged` gives the bits of
spira_adaptive_converged_* and of the kernels (tests/test_adaptive_cpu.py compares them on random inputs)."""
import numpy as np


def _dt(prec):
    if prec == "f32":
        return np.float32
    if prec == "f64":
        return np.float64
    raise ValueError("prec must be 'f32' or 'f64'")


def luma(r, g, b, prec="f64"):
    """(0.2126 r + 0.7152 g) + 0.0722 b in the precision of `prec`."""
    T = _dt(prec)
    r, g, b = (np.asarray(x, dtype=T) for x in (r, g, b))
    with np.errstate(all="ignore"):
        return (T(0.2126) * r + T(0.7152) * g) + T(0.0722) * b


def converged(sum3, q, n, tol, floor, prec="f64"):
    """The rule after n samples.  sum3: [3, ...] RGB sums in sample order, q: [...] sum of the samples' squared luminances, n: scalar or [...]
    sample counts.  Returns a bool array: V = max(n q - Y Y, 0) <= ((tol (Y + n floor)) (tol (Y + n floor))) (n - 1), NaN or tol == 0: False."""
    T = _dt(prec)
    sum3 = np.asarray(sum3, dtype=T)
    q = np.asarray(q, dtype=T)
    n = np.asarray(n, dtype=np.uint32)
    tol, floor = T(tol), T(floor)
    with np.errstate(all="ignore"):
        nn = n.astype(T)
        Y = luma(sum3[0], sum3[1], sum3[2], prec)
        d = nn * q - Y * Y
        V = np.where(d > T(0), d, T(0)).astype(T)
        a = tol * (Y + nn * floor)
        rhs = (a * a) * (n - np.uint32(1)).astype(T)
        ok = ~np.isnan(d) & (V <= rhs)
    return ok if tol > T(0) else np.zeros_like(ok)


def levels(min_spp, batch_spp, spp):
    """The sample counts a pixel can end with: min, min + batch, ..., spp."""
    if min_spp < 2 or batch_spp < 1 or min_spp > spp:
        raise ValueError("need min_spp >= 2, batch_spp >= 1, min_spp <= spp")
    out = list(range(min_spp, spp, batch_spp))
    return out + [spp]


def counts_from_samples(radiance, min_spp, batch_spp, tol, floor, prec="f64"):
    """The schedule applied to per-sample radiance [spp, 3, ...] (sample-major): returns (n, sum3, q) per pixel — the count each pixel ends with
    and its sums and Q at that count.  A reference for tests (the oracle's samples go through this)."""
    T = _dt(prec)
    radiance = np.asarray(radiance, dtype=T)
    spp = radiance.shape[0]
    shape = radiance.shape[2:]
    s = np.zeros((3,) + shape, dtype=T)
    q = np.zeros(shape, dtype=T)
    n = np.zeros(shape, dtype=np.uint32)
    active = np.ones(shape, dtype=bool)
    out_s, out_q = s.copy(), q.copy()
    done = 0
    for lv in levels(min_spp, batch_spp, spp):
        with np.errstate(all="ignore"):
            for k in range(done, lv):
                s = s + radiance[k]
                y = luma(radiance[k, 0], radiance[k, 1], radiance[k, 2], prec)
                q = q + y * y
        done = lv
        stop = active & (converged(s, q, lv, tol, floor, prec) | (lv == spp))
        n[active] = lv
        out_s[:, active] = s[:, active]
        out_q[active] = q[active]
        active &= ~stop
    return n, out_s, out_q
