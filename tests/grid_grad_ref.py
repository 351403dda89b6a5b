"""Float64 references for the per-voxel gradients of a heterogeneous medium's sigma_t grid (test_grid_grad.py,
test_grid_grad_gpu.py).  numpy only, independent of the renderer's code.

sigma_t(p) = scale * sum_v w_v(p) grid[v] with the trilinear weights of src/volumes/grid.cpp (texel centres at (i + .5) / res,
clamped corner indices).  Arrays are indexed (z, y, x) like the array write_volume_grid takes; points are in the volume's unit cube.
"""
import numpy as np


def corners(p, shape):
    """The eight corner voxels of the lookup at local points p (..., 3): (flat indices (..., 8), weights (..., 8)).  Clamping can make
    two corners the same voxel; both weights belong to it."""
    p = np.asarray(p, np.float64)
    rz, ry, rx = shape
    res = np.array([rx, ry, rz], np.float64)
    f = p * res - 0.5
    fl = np.floor(f)
    w1 = f - fl
    w0 = 1.0 - w1
    i0 = np.clip(fl.astype(np.int64), 0, np.array([rx, ry, rz]) - 1)
    i1 = np.clip(fl.astype(np.int64) + 1, 0, np.array([rx, ry, rz]) - 1)
    idx, wgt = [], []
    for cz in (0, 1):
        for cy in (0, 1):
            for cx in (0, 1):
                x = (i1 if cx else i0)[..., 0]; y = (i1 if cy else i0)[..., 1]; z = (i1 if cz else i0)[..., 2]
                idx.append((z * ry + y) * rx + x)
                wgt.append((w1 if cx else w0)[..., 0] * (w1 if cy else w0)[..., 1] * (w1 if cz else w0)[..., 2])
    return np.stack(idx, -1), np.stack(wgt, -1)


def weights(p, shape):
    """Dense w_v(p) for points p (n, 3): (n, rz * ry * rx)."""
    p = np.asarray(p, np.float64).reshape(-1, 3)
    idx, wgt = corners(p, shape)
    out = np.zeros((p.shape[0], int(np.prod(shape))))
    np.add.at(out, (np.arange(p.shape[0])[:, None], idx), wgt)
    return out


def trilinear(grid, p):
    """Direct evaluation, written apart from corners(): clamp-to-edge texel fetches, lerp along x, then y, then z."""
    g = np.asarray(grid, np.float64)
    p = np.asarray(p, np.float64)
    rz, ry, rx = g.shape

    def axis(v, n):
        f = v * n - 0.5
        i = np.floor(f).astype(np.int64)
        return np.clip(i, 0, n - 1), np.clip(i + 1, 0, n - 1), f - np.floor(f)
    x0, x1, tx = axis(p[..., 0], rx); y0, y1, ty = axis(p[..., 1], ry); z0, z1, tz = axis(p[..., 2], rz)

    def lerp(a, b, t):
        return a + (b - a) * t
    c0 = lerp(lerp(g[z0, y0, x0], g[z0, y0, x1], tx), lerp(g[z0, y1, x0], g[z0, y1, x1], tx), ty)
    c1 = lerp(lerp(g[z1, y0, x0], g[z1, y0, x1], tx), lerp(g[z1, y1, x0], g[z1, y1, x1], tx), ty)
    return lerp(c0, c1, tz)


def line_weights(o, d, t0, t1, to_local, shape, n=512):
    """W_v = integral over [t0, t1] of w_v(to_local(o + t d)) dt for rays (m, 3), by midpoint quadrature with n steps: (m, n_voxels).
    to_local: 3 x 4 affine world -> unit cube.  Rays with t1 <= t0 give 0."""
    o = np.broadcast_to(np.asarray(o, np.float64), np.asarray(d).shape).reshape(-1, 3)
    d = np.asarray(d, np.float64).reshape(-1, 3)
    t0 = np.asarray(t0, np.float64).reshape(-1); t1 = np.asarray(t1, np.float64).reshape(-1)
    A = np.asarray(to_local, np.float64).reshape(3, 4)
    length = np.maximum(t1 - t0, 0.0)
    out = np.zeros((d.shape[0], int(np.prod(shape))))
    rows = np.arange(d.shape[0])[:, None]
    for k in range(n):
        t = t0 + (k + 0.5) / n * length
        p = o + d * t[:, None]
        idx, wgt = corners(p @ A[:, :3].T + A[:, 3], shape)
        np.add.at(out, (rows, idx), wgt * (length / n)[:, None])
    return out


def cube_to_local():
    """to_local of the tests' volumes: to_world = translate(-1) * scale(2), the unit cube onto [-1, 1]^3."""
    return np.array([[0.5, 0, 0, 0.5], [0, 0.5, 0, 0.5], [0, 0, 0.5, 0.5]], np.float64)
