"""numpy restatement of the guided denoiser, written from DESIGN.md section 9.1 (the specification), not from the kernel.

denoise_f32(exp, ...): every operation is one float32 numpy operation in the order the specification fixes, `exp` is passed in
(the oracle's: lambda x: orc.math_eval(1, x)[0]), so the device's output can be compared with it bit for bit.
denoise_f64(...): the same filter in float64 with numpy's exp, the yardstick for rounding-error bounds."""
import numpy as np

H5 = (1.0 / 16, 1.0 / 4, 3.0 / 8, 1.0 / 4, 1.0 / 16)          # indexed by i + 2; every product h_i * h_j is exact in float32
DEFAULTS = dict(iterations=5, sigma_color=0.3, sigma_normal=0.1, sigma_albedo=0.05, eps_a=0.5)   # include/liverrt.h LRT_DENOISE_*


def _shift(a, dx, dy):
    """b[y, x] = a[y + dy, x + dx] where that lies inside the image, and the mask of those (y, x)."""
    h, w = a.shape[:2]
    b = np.zeros_like(a); inside = np.zeros((h, w), bool)
    x0, x1 = max(0, -dx), min(w, w - dx)
    y0, y1 = max(0, -dy), min(h, h - dy)
    if x0 < x1 and y0 < y1:
        b[y0:y1, x0:x1] = a[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
        inside[y0:y1, x0:x1] = True
    return b, inside


def _denoise(T, exp, noisy, albedo, normals, denoise_alpha, iterations, sigma_color, sigma_normal, sigma_albedo, eps_a):
    noisy = np.asarray(noisy, T)
    h, w, C = noisy.shape
    assert C in (3, 4) and 1 <= iterations <= 8
    sc, sn, sa, eps = T(sigma_color), T(sigma_normal), T(sigma_albedo), T(eps_a)
    sc2 = sc * sc
    i_n, i_a = T(1) / (sn * sn), T(1) / (sa * sa)
    alpha_filtered = bool(denoise_alpha) and C == 4
    with np.errstate(all="ignore"):
        rgb = noisy[..., :3]
        if albedo is not None:
            a = np.asarray(albedo, T)
            d = np.where(a > eps, a, eps).astype(T)
            c = rgb / d
        else:
            a, d, c = None, None, rgb.copy()
        n = None if normals is None else np.asarray(normals, T)
        ok = np.isfinite(c).all(axis=2)
        if a is not None: ok &= np.isfinite(a).all(axis=2)
        if n is not None: ok &= np.isfinite(n).all(axis=2)
        if alpha_filtered: ok &= np.isfinite(noisy[..., 3])
        if alpha_filtered:
            c = np.concatenate([c, noisy[..., 3:4]], axis=2)
        nch = c.shape[2]

        def dist2(u, uq):
            v = uq - u
            return (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]

        for k in range(iterations):
            s = 1 << k
            ic = T(4 ** k) / sc2
            sum_w = np.zeros((h, w), T); sum_c = np.zeros((h, w, nch), T)
            for j in range(-2, 3):
                for i in range(-2, 3):
                    cq, inside = _shift(c, s * i, s * j)
                    okq, _ = _shift(ok, s * i, s * j)
                    take = inside & okq & ok
                    e = dist2(c, cq) * ic
                    if n is not None:
                        e = e + dist2(n, _shift(n, s * i, s * j)[0]) * i_n
                    if a is not None:
                        e = e + dist2(a, _shift(a, s * i, s * j)[0]) * i_a
                    e = np.where(take, e, T(0)).astype(T)                  # skipped taps: keep exp's argument defined
                    wt = T(H5[i + 2] * H5[j + 2]) * exp(-e)
                    sum_w = np.where(take, sum_w + wt, sum_w)
                    sum_c = np.where(take[..., None], sum_c + wt[..., None] * np.where(take[..., None], cq, T(0)), sum_c)
            nxt = sum_c / sum_w[..., None]
            c = np.where(ok[..., None], nxt, c).astype(T)
        out = noisy.copy()
        res = c[..., :3] * d if d is not None else c[..., :3]
        out[..., :3] = np.where(ok[..., None], res, noisy[..., :3])
        if alpha_filtered:
            out[..., 3] = np.where(ok, c[..., 3], noisy[..., 3])
    return out.astype(T)


def _params(kw):
    p = dict(DEFAULTS); p.update({k: v for k, v in kw.items() if v is not None})
    return p


def denoise_f32(exp, noisy, albedo=None, normals=None, denoise_alpha=False, **params):
    f = lambda x: np.asarray(exp(np.ascontiguousarray(x, np.float32)), np.float32).reshape(np.shape(x))
    return _denoise(np.float32, f, noisy, albedo, normals, denoise_alpha, **_params(params))


def denoise_f64(noisy, albedo=None, normals=None, denoise_alpha=False, **params):
    """The float64 filter on the float32 parameters and inputs (converted exactly)."""
    p = _params(params)
    for k in ("sigma_color", "sigma_normal", "sigma_albedo", "eps_a"):
        p[k] = float(np.float32(p[k]))
    return _denoise(np.float64, np.exp, noisy, albedo, normals, denoise_alpha, **p)
