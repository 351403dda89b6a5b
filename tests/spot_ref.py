"""A numpy restatement of the spot and directional emitters' sample_direction (the renderer this project follows: src/emitters/spot.cpp
:90-117, 129-150, 176-210 and src/emitters/directional.cpp:65-108, 148-176), of the checkerboard a spot may project
(src/textures/checkerboard.cpp:70-88) and of the constant emitter beside them in a two-emitter scene (src/emitters/constant.cpp,
Scene::sample_emitter_direction's uniform selection with its re-used sample, src/render/scene.cpp:333-383).  The precision T is a
parameter, in the manner of phase_ref.py: float64 is the reference the device is held to, float32 the run whose distance from it sets
the tolerances (spot_cases.py).  What the host derives once per emitter (radians, cosines, 1 / (cutoff - beam), tan(cutoff), the inverse
of to_world, a directional light's direction, the bounding sphere) is float32, and both precisions read the same numbers."""
import numpy as np

EPS = 2.0 ** -23
F = np.float32
RAY_EPS = F(5.9604644775390625e-8) * F(1500.0)


def _f32_inverse3(m):
    """the linear part's inverse, computed in double and rounded (csrc/scene_prep.cpp inverse3)"""
    return np.linalg.inv(np.asarray(m, np.float64)[:3, :3]).astype(F)


class Checkerboard:
    def __init__(self, color0=(0.4, 0.4, 0.4), color1=(0.2, 0.2, 0.2), scale=1.0):
        self.color0, self.color1 = np.asarray(color0, F), np.asarray(color1, F)
        self.to_uv = np.array([[scale, 0, 0], [0, scale, 0]], F)             # rows 0 and 1 of the 3 x 3 affine uv transform

    def eval(self, uv, T):
        """(value (n x 3), margin (n): the distance in uv to the nearest tile edge)"""
        m = self.to_uv.astype(T); uv = np.asarray(uv, T)
        u = m[0, 0] * uv[:, 0] + m[0, 1] * uv[:, 1] + m[0, 2]
        v = m[1, 0] * uv[:, 0] + m[1, 1] * uv[:, 1] + m[1, 2]
        fu, fv = u - np.floor(u), v - np.floor(v)
        same = (fu > T(0.5)) == (fv > T(0.5))
        val = np.where(same[:, None], self.color0.astype(T)[None], self.color1.astype(T)[None])
        edge = lambda f: np.minimum(np.minimum(f, 1 - f), np.abs(f - 0.5))
        scale = max(float(np.abs(m[:, :2]).sum(1).max()), 1e-30)
        return val, np.minimum(edge(fu), edge(fv)).astype(np.float64) / scale


class Spot:
    kind = "spot"

    def __init__(self, label, intensity=(1, 1, 1), cutoff_angle=20.0, beam_width=None, to_world=None, texture=None):
        self.label = label
        self.intensity = np.asarray(intensity, F) * np.ones(3, F)
        self.cutoff_deg = F(cutoff_angle)
        self.beam_deg = F(beam_width) if beam_width is not None else self.cutoff_deg * F(3.0) / F(4.0)
        self.to_world = np.eye(4, dtype=F) if to_world is None else np.asarray(to_world, F)
        self.texture = texture
        deg = F(np.pi) / F(180.0)                                            # dr::deg_to_rad: value * (Pi / 180), float32
        self.cutoff, self.beam = self.cutoff_deg * deg, self.beam_deg * deg
        with np.errstate(divide="ignore"):
            self.inv_transition = F(1.0) / (self.cutoff - self.beam)          # +inf when the two are equal: the ring is empty
        self.cos_cutoff, self.cos_beam = np.cos(self.cutoff).astype(F), np.cos(self.beam).astype(F)
        self.uv_factor = np.tan(self.cutoff).astype(F)
        self.pos = self.to_world[:3, 3].copy()
        self.to_local = _f32_inverse3(self.to_world)

    def falloff_curve(self, d, T):
        """spot.cpp:142-150 on an unnormalised local direction"""
        d = np.asarray(d, T)
        cos = d[:, 2] / np.sqrt((d * d).sum(1))
        with np.errstate(invalid="ignore", over="ignore"):
            ring = (T(self.cutoff) - np.arccos(np.clip(cos, -1, 1))) * T(self.inv_transition)
        beam = np.where(cos >= T(self.cos_beam), T(1.0), ring)
        return np.where(cos > T(self.cos_cutoff), beam, T(0.0)), cos

    def direction_to_uv(self, d, T):
        """spot.cpp:129-134"""
        d = np.asarray(d, T)
        with np.errstate(invalid="ignore", divide="ignore"):
            den = d[:, 2] * T(self.uv_factor)
            return np.stack([T(0.5) + T(0.5) * d[:, 0] / den, T(0.5) + T(0.5) * d[:, 1] / den], 1)

    def sample_direction(self, ref, T=np.float64):
        ref = np.asarray(ref, T); n = len(ref)
        p = np.broadcast_to(self.pos.astype(T), (n, 3)).copy()
        d = p - ref
        dist = np.sqrt((d * d).sum(1))
        inv = T(1.0) / dist
        d = d * inv[:, None]
        local = (-d) @ self.to_local.astype(T).T
        falloff, cos = self.falloff_curve(local, T)
        lit = falloff > 0
        val = np.broadcast_to(self.intensity.astype(T), (n, 3)).copy()
        margin = np.full(n, np.inf)
        if self.texture is not None:
            uv = np.where(lit[:, None], self.direction_to_uv(local, T), T(0.25))
            tex, m = self.texture.eval(uv, T)
            val = val * tex; margin = np.where(lit, m, np.inf)
        w = np.where(lit[:, None], val, T(0.0)) * (falloff * inv * inv)[:, None]
        return {"p": p, "n": np.zeros((n, 3), T), "d": d, "dist": dist, "pdf": np.ones(n, T), "weight": w,
                "falloff": falloff, "cos": cos, "margin": margin}


def look_at_direction(direction):
    """directional.cpp:75-78 in float32: normalize, coordinate_system (include/mitsuba/core/vector.h:118-138), look_at(0, direction, up)"""
    n = np.asarray(direction, F); n = n * (F(1.0) / np.sqrt((n * n).sum(dtype=F)))
    sign = np.copysign(F(1.0), n[2]); a = -(F(1.0) / (sign + n[2])); b = n[0] * n[1] * a
    up = np.array([sign * (n[0] * n[0] * a) + F(1.0), sign * b, -sign * n[0]], F)
    dirv = n * (F(1.0) / np.sqrt((n * n).sum(dtype=F)))
    left = np.cross(up, dirv).astype(F); left = left * (F(1.0) / np.sqrt((left * left).sum(dtype=F)))
    nup = np.cross(dirv, left).astype(F)
    m = np.eye(4, dtype=F); m[:3, 0], m[:3, 1], m[:3, 2] = left, nup, dirv
    return m


def bounding_sphere(lo, hi):
    """Scene::bbox().bounding_sphere() with the emitters' margin (bbox.h:343-346; directional.cpp:98-108), float32"""
    lo, hi = np.asarray(lo, F), np.asarray(hi, F)
    c = (hi + lo) * F(0.5); dd = c - hi
    r = np.sqrt((dd * dd).sum(dtype=F)).astype(F)
    return c, max(RAY_EPS, r * (F(1.0) + RAY_EPS))


class Directional:
    kind = "directional"

    def __init__(self, label, irradiance=(1, 1, 1), to_world=None, direction=None, bsphere=((0, 0, 0), 1.0)):
        assert to_world is None or direction is None
        self.label = label
        self.irradiance = np.asarray(irradiance, F) * np.ones(3, F)
        self.direction = None if direction is None else np.asarray(direction, np.float64)
        self.to_world = look_at_direction(direction) if direction is not None else (np.eye(4, dtype=F) if to_world is None else np.asarray(to_world, F))
        self.d = self.to_world[:3, 2].copy()                                  # to_world * (0, 0, 1)
        self.center, self.radius = np.asarray(bsphere[0], F), F(bsphere[1])

    def sample_direction(self, ref, T=np.float64):
        ref = np.asarray(ref, T); n = len(ref)
        d = np.broadcast_to(self.d.astype(T), (n, 3)).copy()
        rel = ref - self.center.astype(T)
        radius = np.maximum(T(self.radius), np.sqrt((rel * rel).sum(1)))
        dist = T(2.0) * radius
        return {"p": ref - d * dist[:, None], "n": d, "d": -d, "dist": dist, "pdf": np.ones(n, T),
                "weight": np.broadcast_to(self.irradiance.astype(T), (n, 3)).copy(), "margin": np.full(n, np.inf)}


class ConstantSky:
    """src/emitters/constant.cpp sample_direction: a uniform direction, the sample at twice the bounding sphere's radius"""
    kind = "constant"

    def __init__(self, radiance=(1, 1, 1), bsphere=((0, 0, 0), 1.0)):
        self.radiance = np.asarray(radiance, F) * np.ones(3, F)
        self.center, self.radius = np.asarray(bsphere[0], F), F(bsphere[1])

    def sample_direction(self, ref, smp, T=np.float64):
        ref = np.asarray(ref, T); smp = np.asarray(smp, T); n = len(ref)
        z = T(1.0) - T(2.0) * smp[:, 1]
        r = np.sqrt(np.maximum(T(1.0) - z * z, T(0.0)))
        phi = T(2.0) * T(np.pi) * smp[:, 0]
        d = np.stack([r * np.cos(phi), r * np.sin(phi), z], 1)
        rel = ref - self.center.astype(T)
        dist = T(2.0) * np.maximum(T(self.radius), np.sqrt((rel * rel).sum(1)))
        pdf = np.full(n, T(1.0) / (T(4.0) * T(np.pi)), T)
        return {"p": ref + d * dist[:, None], "n": -d, "d": d, "dist": dist, "pdf": pdf,
                "weight": np.broadcast_to(self.radiance.astype(T), (n, 3)) / pdf[:, None], "margin": np.full(n, np.inf)}


def sample_emitter_direction(emitters, ref, smp, T=np.float64):
    """Scene::sample_emitter_direction without the visibility test (scene.cpp:333-383): emitter min(floor(sx n), n - 1), sx re-scaled,
    pdf / n, weight * n.  `emitters` in the scene's order; returns the records' union plus `index`."""
    ref = np.asarray(ref, T); smp = np.asarray(smp, T).copy(); n = len(ref); ne = len(emitters)
    index = np.zeros(n, np.int64)
    if ne > 1:
        scaled = smp[:, 0] * T(ne)
        index = np.minimum(scaled.astype(np.int64), ne - 1)
        smp[:, 0] = scaled - index.astype(T)
    out = {k: np.zeros((n, 3), T) for k in ("p", "n", "d", "weight")}
    out.update(dist=np.zeros(n, T), pdf=np.zeros(n, T), margin=np.full(n, np.inf), index=index)
    for k, e in enumerate(emitters):
        sel = index == k
        if not sel.any():
            continue
        s = e.sample_direction(ref[sel], smp[sel], T) if e.kind == "constant" else e.sample_direction(ref[sel], T)
        for key in ("p", "n", "d", "weight", "dist", "pdf", "margin"):
            out[key][sel] = s[key]
    if ne > 1:
        out["pdf"] = out["pdf"] * (T(1.0) / T(ne)); out["weight"] = out["weight"] * T(ne)
    return out
