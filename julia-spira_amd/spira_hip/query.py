"""Ray queries on a scene handle: the numpy restatement of the library's ray preparation (include/spira_hip.h, "ray queries") and the torch form of
spira_scene_cast_device_* / spira_scene_occluded_device_*.

A ray is eight values [ox oy oz t_min dx dy dz t_max].  The library normalises the direction in the call's precision T, nothing fused:
s = (dx dx + dy dy) + dz dz, d = (dx, dy, dz) / sqrt(s); t, t_min and t_max are distances along that unit direction."""
import numpy as np

from . import _binding as B

ORIGIN_BOUND = 64      # the origin rule of scenes with a tree: |(o_k - centre_k) * scale| <= 64


def normalize_rays(rays8, dtype, frame=None):
    """The preparation of spira_query.h (cast_ray_prepare), bit for bit: returns (rays, valid) — `rays` a copy of rays8 in `dtype` whose direction columns
    are the unit directions the kernels walk with (left as given where the ray is invalid), `valid` the library's verdict per ray.
    frame: None for a scene without a tree, else (centre[3], scale) of the tree's normalised frame — the origin rule is then applied."""
    T = np.dtype(dtype).type
    r = np.array(rays8, dtype=T, copy=True).reshape(-1, 8)
    with np.errstate(all="ignore"):
        valid = ~np.isnan(r).any(axis=1)
        valid &= np.isfinite(r[:, [0, 1, 2, 4, 5, 6]]).all(axis=1)
        s = (r[:, 4] * r[:, 4] + r[:, 5] * r[:, 5]) + r[:, 6] * r[:, 6]
        valid &= np.isfinite(s) & ~(s < np.finfo(T).tiny)
        valid &= ~(r[:, 3] < T(0)) & ~(r[:, 7] < r[:, 3])
        if frame is not None:
            c, scale = np.asarray(frame[0], dtype=T), T(frame[1])
            x = (r[:, :3] - c[None, :]) * scale
            valid &= ((x >= T(-ORIGIN_BOUND)) & (x <= T(ORIGIN_BOUND))).all(axis=1)
        d = r[:, 4:7] / np.sqrt(s)[:, None]
    r[:, 4:7] = np.where(valid[:, None], d, r[:, 4:7])
    return r, valid


def cast_rays(scene, rays, want_normal=False, occlusion=False, inplace=False, stream=None):
    """spira_scene_cast_device_* (occlusion: spira_scene_occluded_device_*) for a torch tensor of rays [n, 8] on the scene's device, in the scene's
    precision.  Enqueues on `stream` (a torch.cuda.Stream; None: the current one) and returns device tensors without synchronising:
    (prim int32 [n], t [n], normal [n, 3] or None), or hit uint8 [n] for occlusion.  `rays` must stay alive until the work has run."""
    import torch
    want = torch.float32 if scene.prec == "f32" else torch.float64
    if rays.dtype != want or not rays.is_cuda or rays.dim() != 2 or rays.shape[1] != 8 or not rays.is_contiguous():
        raise ValueError("cast_rays: a contiguous device tensor of n x 8 %s values is needed" % scene.prec)
    n = rays.shape[0]
    st = stream if stream is not None else torch.cuda.current_stream(rays.device)
    with torch.cuda.stream(st):
        if occlusion:
            hit = torch.empty(n, dtype=torch.uint8, device=rays.device)
            scene.occluded_device(rays.data_ptr(), n, hit.data_ptr(), st.cuda_stream, inplace=inplace)
            return hit
        prim = torch.empty(n, dtype=torch.int32, device=rays.device)
        t = torch.empty(n, dtype=want, device=rays.device)
        nrm = torch.empty((n, 3), dtype=want, device=rays.device) if want_normal else None
        scene.cast_device(rays.data_ptr(), n, prim.data_ptr(), t.data_ptr(), nrm.data_ptr() if want_normal else 0, st.cuda_stream, inplace=inplace)
    return prim, t, nrm
