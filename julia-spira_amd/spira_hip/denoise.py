"""The a-trous denoiser of spira_denoise_* restated in numpy (include/spira_hip.h, "denoiser"; csrc/spira_denoise.h), the variance estimate an
adaptive render's outputs give it, and the chain adaptive render -> feature buffers -> denoise on device buffers.  Every operation of `denoise`
is done in the call's precision in the written order, so it gives the bits of the kernels (tests/test_gpu_denoise.py compares them)."""
import numpy as np

from .adaptive import _dt, luma

K5 = (0.0625, 0.25, 0.375, 0.25, 0.0625)
B3 = (0.25, 0.5, 0.25)


def _max0(x, T):
    return np.where(x > T(0), x, T(0)).astype(T)


def denoise(color, variance=None, albedo=None, normal=None, depth=None, iterations=5, sigma_l=4.0, sigma_z=0.1, prec="f64", return_variance=False):
    """color [3, H, W]; variance / depth [H, W], albedo / normal [3, H, W] or None.  Returns out_hdr [3, H, W] (and the filtered variance of the
    demodulated colour when asked; None without a variance plane)."""
    T = _dt(prec)
    if not 1 <= iterations <= 6:
        raise ValueError("iterations must be 1 .. 6")
    if not (sigma_l > 0 and sigma_z > 0):
        raise ValueError("sigma_l and sigma_z must be > 0")
    color = np.asarray(color, dtype=T)
    _, H, W = color.shape
    sl, sz = T(sigma_l), T(sigma_z)
    with np.errstate(all="ignore"):
        # prepare
        if albedo is not None:
            a = np.asarray(albedo, dtype=T) + T(0.001)
            c = color / a
            ya = luma(a[0], a[1], a[2], prec)
        else:
            a = None
            c = color.copy()
        v = None
        if variance is not None:
            v = np.asarray(variance, dtype=T)
            v = v / (ya * ya) if albedo is not None else v.copy()
        n = np.asarray(normal, dtype=T) if normal is not None else None
        z = np.asarray(depth, dtype=T) if depth is not None else None
        for it in range(iterations):
            s = 1 << it
            y = luma(c[0], c[1], c[2], prec)
            if v is not None:
                vp = np.pad(v, 1, mode="edge")
                g = np.zeros((H, W), dtype=T)
                for j in range(3):
                    for i in range(3):
                        g = g + (T(B3[j]) * T(B3[i])) * vp[j:j + H, i:i + W]
                den = (sl * sl) * g + T(1e-12)
            sw = np.zeros((H, W), dtype=T)
            sc = np.zeros((3, H, W), dtype=T)
            sv = np.zeros((H, W), dtype=T)
            for dy in range(-2, 3):
                oy = dy * s
                py0, py1 = max(0, -oy), min(H, H - oy)          # rows p whose tap row p + oy lies inside the image
                if py0 >= py1:
                    continue
                for dx in range(-2, 3):
                    ox = dx * s
                    px0, px1 = max(0, -ox), min(W, W - ox)
                    if px0 >= px1:
                        continue
                    P = (slice(py0, py1), slice(px0, px1))
                    Q = (slice(py0 + oy, py1 + oy), slice(px0 + ox, px1 + ox))
                    w = np.full((py1 - py0, px1 - px0), T(K5[dy + 2]) * T(K5[dx + 2]), dtype=T)
                    centre = dy == 0 and dx == 0                 # the centre tap takes no factor: w = 9/64, so sw >= 9/64 whatever the guides hold
                    if n is not None and not centre:
                        e = _max0((n[0][P] * n[0][Q] + n[1][P] * n[1][Q]) + n[2][P] * n[2][Q], T)
                        for _ in range(6):
                            e = e * e
                    if centre:
                        pass
                    elif z is not None:
                        zp, zq = z[P], z[Q]
                        hp, hq = zp > T(0), zq > T(0)
                        both = hp & hq
                        w = np.where(hp != hq, T(0), w).astype(T)
                        if n is not None:
                            w = np.where(both, w * e, w).astype(T)
                        zm = np.where(zp > zq, zp, zq).astype(T)
                        t = _max0(T(1) - np.abs(zp - zq) / (sz * zm), T)
                        w = np.where(both, w * (t * t), w).astype(T)
                    elif n is not None:
                        w = w * e
                    if v is not None and not centre:
                        dl = y[P] - y[Q]
                        t = _max0(T(1) - (dl * dl) / den[P], T)
                        w = w * (t * t)
                    sw[P] = sw[P] + w
                    for ch in range(3):
                        sc[ch][P] = sc[ch][P] + w * c[ch][Q]
                    if v is not None:
                        sv[P] = sv[P] + (w * w) * v[Q]
            c = sc / sw
            if v is not None:
                v = sv / (sw * sw)
        out = c * a if a is not None else c * T(1)
    return (out, v) if return_variance else out


def variance_of_mean(hdr, q, spp, prec="f64"):
    """The variance of a pixel's MEAN luminance from the outputs of an adaptive render (out_hdr [3, ...], out_q [...], out_spp [...]), in the
    precision of `prec`, in this order: Y = n * luma(hdr), max(n q - Y Y, 0) / ((n n) (n - 1)).  numpy arrays or torch tensors."""
    if type(hdr).__module__.startswith("torch"):
        import torch
        T = torch.float32 if prec == "f32" else torch.float64
        n = spp.to(T)
        lum = (hdr[0].to(T) * 0.2126 + hdr[1].to(T) * 0.7152) + hdr[2].to(T) * 0.0722
        Y = n * lum
        d = n * q.to(T) - Y * Y
        return torch.where(d > 0, d, torch.zeros_like(d)) / ((n * n) * (n - 1))
    T = _dt(prec)
    with np.errstate(all="ignore"):
        n = np.asarray(spp).astype(T)
        Y = n * luma(hdr[0], hdr[1], hdr[2], prec)
        d = n * np.asarray(q, dtype=T) - Y * Y
        return (_max0(d, T) / ((n * n) * (n - T(1)))).astype(T)


def render_denoised(scene_or_arrays, camera12, params, adaptive, feature_spp=8, prec=None, stream=None, iterations=5, sigma_l=4.0, sigma_z=0.1,
                    post=None, want_img=False):
    """Adaptive render -> first-hit features -> denoise, all on device buffers (torch tensors on the current device), on `stream` (a
    torch.cuda.Stream; None: the current one).  scene_or_arrays: a _binding.Scene, or (spheres5, materials8, triangles10) with `prec`.
    params: a whole frame (rows == 0); params.spp is the adaptive cap.  Returns a dict of tensors: hdr (denoised), img (or None), noisy, spp, q,
    variance, albedo, normal, depth.  Nothing here waits for the device beyond the one synchronisation per adaptive round."""
    import copy
    import torch
    from . import _binding as B
    if params.rows:
        raise ValueError("the denoiser takes whole frames: params.rows must be 0")
    own = not isinstance(scene_or_arrays, B.Scene)
    scene = B.Scene(*scene_or_arrays, prec=prec or "f32") if own else scene_or_arrays
    try:
        p = scene.prec
        T = torch.float32 if p == "f32" else torch.float64
        H, W = params.height, params.width
        st = stream if stream is not None else torch.cuda.current_stream()
        sp = st.cuda_stream
        with torch.cuda.stream(st):
            dev = torch.device("cuda", torch.cuda.current_device())
            noisy = torch.empty((3, H, W), dtype=T, device=dev)
            spp = torch.empty((H, W), dtype=torch.int32, device=dev)          # (uint32 on the library's side; counts stay below 2^24)
            q = torch.empty((H, W), dtype=T, device=dev)
            albedo = torch.empty((3, H, W), dtype=T, device=dev)
            normal = torch.empty((3, H, W), dtype=T, device=dev)
            depth = torch.empty((H, W), dtype=T, device=dev)
            hdr = torch.empty((3, H, W), dtype=T, device=dev)
            img = torch.empty((3, H, W), dtype=T, device=dev) if want_img else None
            scene.render_adaptive_device(camera12, params, adaptive, noisy.data_ptr(), 0, spp.data_ptr(), q.data_ptr(), sp)
            fp = copy.copy(params)
            fp.spp = feature_spp
            scene.render_features_device(camera12, fp, albedo.data_ptr(), normal.data_ptr(), depth.data_ptr(), sp)
            variance = variance_of_mean(noisy, q, spp, p).contiguous()
            dn = B.make_denoise(W, H, iterations, params.flags & 0xF00 if post is None else post, sigma_l, sigma_z)
            B.denoise_device(noisy.data_ptr(), dn, hdr.data_ptr(), img.data_ptr() if want_img else 0, sp, d_variance_ptr=variance.data_ptr(),
                             d_albedo_ptr=albedo.data_ptr(), d_normal_ptr=normal.data_ptr(), d_depth_ptr=depth.data_ptr(), prec=p)
        return {"hdr": hdr, "img": img, "noisy": noisy, "spp": spp, "q": q, "variance": variance, "albedo": albedo, "normal": normal, "depth": depth}
    finally:
        if own:
            torch.cuda.current_stream().synchronize() if stream is None else stream.synchronize()
            scene.destroy()
