"""numpy restatement of the moment integrator's per-sample arithmetic, written from DESIGN.md section 10.1 (not from the kernel):

    zero L when the nested integrator is `path` and the sample is invalid (path.cpp:342-345)
    X = fmaf(m02, B, fmaf(m01, G, m00 * R))      and likewise Y, Z with rows 1, 2 of srgb_to_xyz
    m2_X = X * X                                  one rounding

all in IEEE binary32, the matrix entries being the float32 roundings of the decimals of include/mitsuba/core/spectrum.h:396-402.
TEST INFRASTRUCTURE ONLY."""
import numpy as np

SRGB_TO_XYZ = np.array([[0.412453, 0.357580, 0.180423],
                        [0.212671, 0.715160, 0.072169],
                        [0.019334, 0.119193, 0.950227]], dtype=np.float32)


def fma32(a, b, c):
    """fmaf(a, b, c) for float32 arrays, correctly rounded.  The product of two float32 values is exact in float64; the sum with c
    is formed in float64 ROUNDED TO ODD (TwoSum gives the rounding error; an inexact even result is moved to its odd neighbour on
    the error's side), and a round-to-odd value with 53 >= 24 + 2 bits rounds to float32 as the exact sum would."""
    a, b, c = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (a, b, c))
    with np.errstate(invalid="ignore", over="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)
        ok = np.isfinite(s) & np.isfinite(e) & (e != 0)
        bits = np.ascontiguousarray(s).view(np.int64)
        away = (e > 0) == (s > 0)                      # the exact sum lies further from zero than s
        odd = np.where(ok & ((bits & 1) == 0), bits + np.where(away, 1, -1), bits).view(np.float64)
        return odd.astype(np.float32)


def moment_values(L, valid=None, zero_invalid=False):
    """L: (n, 3) float32 radiance; valid: (n,) nonzero where the sample is valid.  Returns (n, 6) float32: X, Y, Z, m2X, m2Y, m2Z."""
    L = np.ascontiguousarray(L, dtype=np.float32).reshape(-1, 3).copy()
    if zero_invalid:
        L[np.asarray(valid).reshape(-1) == 0] = 0
    out = np.empty((L.shape[0], 6), dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for r in range(3):
            m = SRGB_TO_XYZ[r]
            x = fma32(m[2], L[:, 2], fma32(m[1], L[:, 1], (m[0] * L[:, 0]).astype(np.float32)))
            out[:, r] = x
            out[:, 3 + r] = (x * x).astype(np.float32)
    return out


def moment_lanes(lanes, integrator_is_path):
    """The oracle's render_samples lanes (n, 4: R, G, B, valid) -> (n, 6)."""
    lanes = np.asarray(lanes, dtype=np.float32)
    return moment_values(lanes[:, :3], lanes[:, 3], zero_invalid=bool(integrator_is_path))


def film_record(lanes, integrator_is_path, has_alpha):
    """Per lane, what ImageBlock::put multiplies by the filter weight: R, G, B, [A], 1, X, Y, Z, m2X, m2Y, m2Z (float32, (n, 10|11))."""
    lanes = np.asarray(lanes, dtype=np.float32)
    L = lanes[:, :3].copy()
    if integrator_is_path:
        L[lanes[:, 3] == 0] = 0
    cols = [L] + ([lanes[:, 3:4]] if has_alpha else []) + [np.ones((len(lanes), 1), np.float32), moment_values(L)]
    return np.concatenate(cols, axis=1).astype(np.float32)
