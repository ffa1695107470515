// spira_sky.h — which spheres can the camera rays of one pixel reach, and can they reach any?  Two functions, host and device, Float64 (pixel-owning passes are): k_path asks it
// once per owned pixel ahead of its loop (spira_device.h, "sky pass"), spira_sky_pixel_f64 / spira_pixel_reach_f64 export them, tests/native/sky_cull.cpp and reach_mask.cpp hold them against the
// scan's own discriminant.  No HIP header, no library call: a host compiler reads it as it stands.
//
// The rays of pixel (i, j) (reference indices, 1-based) have the directions D = llc + hor u + ver v - origin with u in [(i-1)/(W-1), i/(W-1)),
// v alike (examples/julia-raytracer.jl:398-399, :303).  With Dc the direction of the footprint's centre and
//     rho = (|hor| / (W-1) + |ver| / (H-1)) / 2
// every such D is Dc + e with |e| <= rho, so it lies within the angle delta = asin(rho / |Dc|) of Dc.  A sphere with centre C (from the camera's
// origin) and radius r has disc < 0 (:118-120) exactly when the LINE of sight passes it by: the angle between line and C, folded into [0, pi/2],
// exceeds alpha = asin(r / |C|).  With theta that folded angle for Dc (sin theta = |C x Dc| / (|C| |Dc|), cos theta = |C . Dc| / (|C| |Dc|)) every ray
// of the pixel misses the sphere if theta - delta > alpha, which is sin(theta - delta) > r / |C|, which multiplied through by |C| |Dc|^2 is
//     |C x Dc| sqrt(|Dc|^2 - rho^2) - |C . Dc| rho  >  (r (1 + 2^-20) + |C| 2^-20) |Dc|^2.
// (The cruder |C x Dc| - |C| rho > r (|Dc| + rho) gives up a relative rho / |Dc| of r: nothing is left of S1's sky above the radius-100 ground at
// 97 x 55, where rho / |Dc| = 0.013 and 1 - r / |C| = 0.015.)
// The two 2^-20 are what the rounding is given.  The scan evaluates disc = b b - 4 a cc from a normalised d (|d| = 1 within a few ulp; the
// speculative quotients of SpecDiv stay within a few ulp too, or the wave is rendered again): the terms are of size 4 |C|^2 and carry a few dozen
// 2^-53 of that between them, the direction a relative 2^-52.  The bound keeps the line of sight at least r + |C| 2^-20 from the centre, so the true
// disc is below -4 |C|^2 2^-40 — 2^7 times the error at the least, whatever r / |C| is.  (Of rho the same factor: u and v are rounded quotients.)
// The slack costs an angle of 2^-20 rad, a 400th of a 1080p pixel.
//
// The answer errs towards "may hit" only: every comparison is written so that a NaN fails it, and a radius that is not positive, a camera inside or
// on a sphere (|C| <= r: the left side is at most |C| |Dc|^2 <= r |Dc|^2), a direction that may vanish (|Dc| <= rho), W or H
// below 2 (rho is Inf or NaN) and lengths outside 1e-100 .. 1e100 (products that could overflow or lose their bits) all answer "may hit".
#pragma once
#include <stdint.h>
#include "spira_fastdiv.h"      // SPIRA_HD

namespace spira {

// cam: origin, lower-left corner, horizontal, vertical (3 values each, the kernel's LDS order); spheres5: {x, y, z, radius, material} per sphere.
// Bit s of the result is clear only if no ray of pixel (i, j) can have disc >= 0 for sphere s: the inequality above, sphere by sphere, with the same
// slack and the same guards.  Where a guard of the pixel fails (the early "may hit" exits) every bit is set; where a guard of a sphere fails, its bit.
// Spheres with index >= 32 have no bit: a caller that wants a mask treats them as reachable (k_path scans all of them then).  `beyond` (optional)
// receives whether one of THEM may be hit, so that sky_pixel still answers for sphere sets of any size as it always has.
SPIRA_HD inline uint32_t pixel_reach(const double *cam, uint32_t W, uint32_t H, uint32_t i, uint32_t j, const double *spheres5, uint32_t n_spheres, bool *beyond = nullptr) {
    const double kSlack = 1.0 / 1048576.0, kHuge = 1.0e100, kTiny = 1.0e-100;
    const double w1 = (double)W - 1.0, h1 = (double)H - 1.0;
    const double uc = ((double)i - 0.5) / w1, vc = ((double)j - 0.5) / h1;
    const double hn = __builtin_sqrt((cam[6] * cam[6] + cam[7] * cam[7]) + cam[8] * cam[8]);
    const double vn = __builtin_sqrt((cam[9] * cam[9] + cam[10] * cam[10]) + cam[11] * cam[11]);
    const double rho = (0.5 * (hn / w1 + vn / h1)) * (1.0 + kSlack);
    const double dx = ((cam[3] + cam[6] * uc) + cam[9] * vc) - cam[0];
    const double dy = ((cam[4] + cam[7] * uc) + cam[10] * vc) - cam[1];
    const double dz = ((cam[5] + cam[8] * uc) + cam[11] * vc) - cam[2];
    const double dd = (dx * dx + dy * dy) + dz * dz, dn = __builtin_sqrt(dd);
    if (!(rho >= 0.0 && dn > rho && dn > kTiny && dn < kHuge)) { if (beyond) *beyond = n_spheres > 32u; return 0xFFFFFFFFu; }
    const double q = __builtin_sqrt(dd - rho * rho);                 // |Dc| cos delta
    uint32_t reach = 0;
    bool far = false;
    for (uint32_t s = 0; s < n_spheres; ++s) {
        const double *sp = spheres5 + 5 * (uint64_t)s;
        const double r = sp[3];
        const double cx = sp[0] - cam[0], cy = sp[1] - cam[1], cz = sp[2] - cam[2];
        const double cn = __builtin_sqrt((cx * cx + cy * cy) + cz * cz);
        const double xx = cy * dz - cz * dy, xy = cz * dx - cx * dz, xz = cx * dy - cy * dx;
        const double xn = __builtin_sqrt((xx * xx + xy * xy) + xz * xz);
        const double cd = __builtin_fabs((cx * dx + cy * dy) + cz * dz);
        const bool missed = (r > 0.0 && r < kHuge && cn > kTiny && cn < kHuge) && (xn * q - cd * rho > (r * (1.0 + kSlack) + cn * kSlack) * dd);
        if (!missed) { if (s < 32u) reach |= 1u << s; else far = true; }
    }
    if (beyond) *beyond = far;
    return reach;
}

// true: no ray of pixel (i, j) has disc >= 0 for any sphere — the pixel sees the sky alone.  For up to 32 spheres this is pixel_reach() == 0; beyond
// that the mask has run out of bits (the overflow case) and the spheres without one are asked for through `beyond`.
SPIRA_HD inline bool sky_pixel(const double *cam, uint32_t W, uint32_t H, uint32_t i, uint32_t j, const double *spheres5, uint32_t n_spheres) {
    bool beyond = false;
    return pixel_reach(cam, W, H, i, j, spheres5, n_spheres, &beyond) == 0 && !beyond;
}

}  // namespace spira
