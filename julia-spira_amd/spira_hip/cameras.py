"""Cameras as ray lists: generators for spira_scene_radiance_* (Scene.radiance / Scene.radiance_device).

Any camera is a list of rays plus a pixel key per ray; the integrator, its RNG and its sample order are the renderer's own.  Three models have a
device generator in the library (spira_camera_rays_*: pinhole, thin lens, orthographic); `Equirect` is a host-only numpy generator that shows the
same route for a camera the library knows nothing about.  The numpy functions below restate the library's arithmetic bit for bit (the same
operations in the same order and precision: tests compare them with the library by array_equal) — the counter RNG included, so that this module
never needs the oracle.

Rays are ordered by reference pixel: ray k = (j - 1 - row0) * width + (i - 1), row j - 1 = 0 the BOTTOM of the image; the key of ray k is its global
pixel, so a chunk of rows is traced with key0 = row0 * width.
"""
import numpy as np

from . import _binding as B

K_MAX_TRIES = 64      # kMaxTries of csrc/spira_device.h
LENS_BOUNCE = 255     # the bounce index of the lens point's RNG key: no path reaches it (max_depth <= 255)


def _npdt(prec):
    return B._dt(prec)[0]


# ---------------------------------------------------------------- the counter RNG (csrc/spira_device.h: mix32, rng_key, rng3)
def mix32(x):
    x = np.asarray(x, dtype=np.uint32).copy()
    with np.errstate(over="ignore"):
        x ^= x >> np.uint32(16); x *= np.uint32(0x7FEB352D)
        x ^= x >> np.uint32(15); x *= np.uint32(0x846CA68B)
        x ^= x >> np.uint32(16)
    return x


def seed_halves(seed):
    lo, hi = np.uint32(seed & 0xFFFFFFFF), np.uint32((seed >> 32) & 0xFFFFFFFF)
    with np.errstate(over="ignore"):
        sA = mix32(mix32(np.uint32(lo + np.uint32(0x9E3779B9))) ^ hi)
        sB = mix32(mix32(np.uint32(hi + np.uint32(0x85EBCA6B))) ^ lo)
    return np.uint32(sA), np.uint32(sB)


def rng_key(seed, pixel, sample, bounce):
    """(hA, hB, hBr) uint32 arrays for pixel (array or scalar), sample and bounce."""
    sA, sB = seed_halves(seed)
    pixel = np.asarray(pixel, dtype=np.uint32)
    sb = np.uint32(((int(sample) << 8) | int(bounce)) & 0xFFFFFFFF)
    with np.errstate(over="ignore"):
        hA = mix32(mix32(sA + pixel) ^ sb)
        hB = mix32(mix32(sB ^ pixel) + sb)
    return hA, hB, (hB << np.uint32(16)) | (hB >> np.uint32(16))


def _rng3_key(key, t, prec, scale):
    hA, hB, hBr = key
    npdt = _npdt(prec)
    with np.errstate(over="ignore"):
        a = mix32((hA + np.uint32((int(t) * 0x9E3779B9) & 0xFFFFFFFF)) ^ hBr)
        b = mix32(a + hB)
    s = npdt(scale)
    u0 = (a >> np.uint32(11)).astype(npdt) * s
    u1 = (b >> np.uint32(11)).astype(npdt) * s
    u2 = (((a & np.uint32(0x7FF)) << np.uint32(10)) | (b & np.uint32(0x3FF))).astype(npdt) * s
    return u0, u1, u2


def rng3(seed, pixel, sample, bounce, t, prec="f64", scale=1.0 / 2097152.0):
    """Try t of the key (pixel, sample, bounce): three uniforms in [0, 1), shape pixel.shape + (3,).  scale 2^-20 gives 2 u (the rejection loops)."""
    u = _rng3_key(rng_key(seed, pixel, sample, bounce), t, prec, scale)
    return np.stack(u, axis=-1)


# ---------------------------------------------------------------- ray preparation (csrc/spira_radiance.h: radiance_ray_prepare)
def ray_prepare(rays6, prec="f32"):
    """(valid bool [n], unit directions [n, 3]; rows of invalid rays are 0) — the library's classification and normalisation of a ray list."""
    npdt = _npdt(prec)
    r = np.ascontiguousarray(rays6, dtype=npdt).reshape(-1, 6)
    with np.errstate(all="ignore"):
        finite = np.all((r - r) == 0, axis=1)
        dx, dy, dz = r[:, 3], r[:, 4], r[:, 5]
        s = (dx * dx + dy * dy) + dz * dz
        valid = finite & ((s - s) == 0) & ~(s < np.finfo(npdt).tiny)
        length = np.sqrt(s)
        d = r[:, 3:6] / length[:, None]
    d[~valid] = 0
    return valid, d


# ---------------------------------------------------------------- the generator models (csrc/spira_radiance.h: camera_ray_generate)
def _pixel_grid(width, height, row0, rows):
    rows = rows or height
    jy, ix = np.meshgrid(np.arange(row0, row0 + rows, dtype=np.uint32), np.arange(width, dtype=np.uint32), indexing="ij")
    return ix.reshape(-1), jy.reshape(-1)


def generate_rays(camera12, model, width, height, sample=0, seed=0, row0=0, rows=0, lens_radius=0.0, prec="f32"):
    """The numpy restatement of spira_camera_rays_*: [rows * width, 6] = [o, d], d not normalised."""
    npdt = _npdt(prec)
    cam = np.ascontiguousarray(camera12, dtype=npdt)
    origin, llc, hor, ver = cam[0:3], cam[3:6], cam[6:9], cam[9:12]
    if not rows:
        row0 = 0
    ix, jy = _pixel_grid(width, height, row0, rows)
    pixel = jy * np.uint32(width) + ix
    xu, xv, _ = _rng3_key(rng_key(seed, pixel, sample, 0), 0, prec, 1.0 / 2097152.0)
    u = (ix.astype(npdt) + xu) / npdt(width - 1)
    v = (jy.astype(npdt) + xv) / npdt(height - 1)
    P = (llc[None, :] + hor[None, :] * u[:, None]) + ver[None, :] * v[:, None]
    q = P - origin[None, :]
    n = len(pixel)
    out = np.empty((n, 6), dtype=npdt)
    R = npdt(lens_radius)
    if model == B.CAM_ORTHO:
        out[:, 0:3] = P
        out[:, 3:6] = (((llc + hor / npdt(2)) + ver / npdt(2)) - origin)[None, :]
    elif model == B.CAM_THIN_LENS and R != 0:
        lu = np.sqrt((hor[0] * hor[0] + hor[1] * hor[1]) + hor[2] * hor[2])
        lv = np.sqrt((ver[0] * ver[0] + ver[1] * ver[1]) + ver[2] * ver[2])
        eu, ev = hor / lu, ver / lv
        key = rng_key(seed, pixel, sample, LENS_BOUNCE)
        px, py = np.zeros(n, dtype=npdt), np.zeros(n, dtype=npdt)
        todo = np.ones(n, dtype=bool)
        for t in range(1, K_MAX_TRIES + 1):
            if not todo.any():
                break
            u0, u1, _ = _rng3_key(key, t, prec, 1.0 / 1048576.0)
            ax, ay = u0 - npdt(1), u1 - npdt(1)
            ok = todo & (ax * ax + ay * ay < npdt(1))
            px[ok], py[ok] = ax[ok], ay[ok]
            todo &= ~ok
        rx, ry = R * px, R * py
        off = eu[None, :] * rx[:, None] + ev[None, :] * ry[:, None]
        out[:, 0:3] = origin[None, :] + off
        out[:, 3:6] = q - off
    elif model in (B.CAM_PINHOLE, B.CAM_THIN_LENS):
        out[:, 0:3] = origin[None, :]
        out[:, 3:6] = q
    else:
        raise ValueError("unknown camera model %r" % (model,))
    return out


class _LibraryCamera:
    """A model the library generates on the device (spira_camera_rays_device_*) and on the host (spira_camera_rays_*)."""
    model = B.CAM_PINHOLE
    lens_radius = 0.0

    def __init__(self, camera12):
        self.camera12 = np.ascontiguousarray(camera12, dtype=np.float64)
        assert self.camera12.shape == (12,)

    def rays(self, width, height, sample=0, seed=0, prec="f32", row0=0, rows=0):
        return B.camera_rays(self.camera12, self.model, width, height, sample, seed, row0, rows, self.lens_radius, prec)

    def rays_numpy(self, width, height, sample=0, seed=0, prec="f32", row0=0, rows=0):
        return generate_rays(self.camera12, self.model, width, height, sample, seed, row0, rows, self.lens_radius, prec)

    def rays_device(self, d_rays_ptr, width, height, sample=0, seed=0, prec="f32", row0=0, rows=0, stream_ptr=0):
        B.camera_rays_device(self.camera12, self.model, width, height, d_rays_ptr, sample, seed, row0, rows, self.lens_radius, stream_ptr, prec)


class Pinhole(_LibraryCamera):
    """The renderer's own camera: its ray list reproduces Scene.render bit for bit."""
    model = B.CAM_PINHOLE


class ThinLens(_LibraryCamera):
    """A thin lens of radius lens_radius (= aperture / 2) focused on the plane camera12 was built for (focus_dist)."""
    model = B.CAM_THIN_LENS

    def __init__(self, camera12, lens_radius):
        super().__init__(camera12)
        self.lens_radius = float(lens_radius)


class Ortho(_LibraryCamera):
    """Parallel rays along the camera axis, from the points of the pinhole camera's focus plane."""
    model = B.CAM_ORTHO


class Equirect:
    """A full panorama (longitude x latitude) around `position`: host-only, numpy — any camera is a ray list.  Pixel (ix, jy) with the renderer's jitter
    looks along longitude 2 pi (u - 1/2) from `forward` (towards `right` = forward x up) and latitude pi (v - 1/2) above the horizon."""

    def __init__(self, position, forward=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0)):
        self.position = np.asarray(position, dtype=np.float64)
        f = np.asarray(forward, dtype=np.float64)
        f = f / np.sqrt(f @ f)
        r = np.cross(f, np.asarray(up, dtype=np.float64))
        r = r / np.sqrt(r @ r)
        self.forward, self.right, self.up = f, r, np.cross(r, f)

    def rays(self, width, height, sample=0, seed=0, prec="f32", row0=0, rows=0):
        npdt = _npdt(prec)
        if not rows:
            row0 = 0
        ix, jy = _pixel_grid(width, height, row0, rows)
        pixel = jy * np.uint32(width) + ix
        xu, xv, _ = _rng3_key(rng_key(seed, pixel, sample, 0), 0, "f64", 1.0 / 2097152.0)
        lon = 2.0 * np.pi * ((ix + xu) / width - 0.5)
        lat = np.pi * ((jy + xv) / height - 0.5)
        d = (np.cos(lat) * np.cos(lon))[:, None] * self.forward + (np.cos(lat) * np.sin(lon))[:, None] * self.right + np.sin(lat)[:, None] * self.up
        out = np.empty((len(pixel), 6), dtype=npdt)
        out[:, 0:3] = self.position.astype(npdt)
        out[:, 3:6] = d.astype(npdt)
        return out


def _torch_device():
    try:
        import torch
    except Exception:
        return None
    return torch if torch.cuda.is_available() else None


def render(scene, model, width, height, spp, max_depth, seed=0, flags=0):
    """A frame through the ray-list route: for every sample, the model's rays, then one radiance call of spp = 1 at sample0 = s into one running sum.
    With torch and a device the rays and the sums stay on the device (nothing crosses to the host inside the loop; a model without a device generator
    uploads its host rays); without torch the host forms are used.  Returns hdr [3, height, width] (sum / spp in the scene's precision, row 0 = top)."""
    prec = scene.prec
    npdt = _npdt(prec)
    n = width * height
    torch = _torch_device()
    if torch is None:
        sums = np.zeros((n, 3), dtype=npdt)
        for s in range(spp):
            scene.radiance(model.rays(width, height, s, seed, prec), 1, max_depth, seed=seed, sample0=s, flags=flags, sums=sums)
    else:
        tdt = torch.float32 if prec == "f32" else torch.float64
        rays = torch.empty((n, 6), dtype=tdt, device="cuda")
        d_sums = torch.zeros((n, 3), dtype=tdt, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        for s in range(spp):
            if hasattr(model, "rays_device"):
                model.rays_device(rays.data_ptr(), width, height, s, seed, prec, stream_ptr=stream)
            else:
                rays.copy_(torch.from_numpy(model.rays(width, height, s, seed, prec)), non_blocking=False)
            scene.radiance_device(rays.data_ptr(), n, 1, max_depth, d_sums.data_ptr(), seed=seed, sample0=s, flags=flags, stream_ptr=stream)
        sums = d_sums.cpu().numpy()
    hdr = (sums / npdt(spp)).reshape(height, width, 3)[::-1]      # reference rows run from the bottom; row 0 of the frame is the top
    return np.ascontiguousarray(np.moveaxis(hdr, -1, 0))
