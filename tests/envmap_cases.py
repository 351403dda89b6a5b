"""The maps, scenes, sample sets and checks that tests/test_envmap.py (oracle, CPU) and tests/test_envmap_gpu.py (device) share.
A "probe" is a dict of arrays d, pdf, weight, hit_pdf, hit_le for a set of samples: the device's Scene.emitter_probe returns one,
`orc_probe` assembles one from the oracle's envmap hooks.  Every check takes a probe and the float64 reference (envmap_ref.py)."""
import os

import numpy as np

import envmap_ref as er

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASSET = os.path.join(ROOT, "scenes", "assets", "cavidade_latitude.exr")

LIVER_TO_WORLD = ('<transform name="to_world"><translate x="-3" y="3" z="4"/><scale value="1.0"/>'
                  '<rotate x="0.57735" y="0.57735" z="0.57735" angle="180"/></transform>')

#: name -> (width, height); the shared asset last
MAPS = ["const_2x3", "one_texel_10x100", "const_100x100", "rand_5x3", "rand_7x5", "rand_17x9", "rand_33x31", "zeros_16x9",
        "rotated_17x9", "cavidade"]
N_ROUND_TRIP = 1 << 16
N_CHI2 = 1 << 18
CHI2_GRID = (64, 32)            # bins in u, in v
POLE_SIN = 1e-3                 # samples with sin(theta) below this only have to be finite and non-negative ...
POLE_SHARE = 0.01               # ... and may be at most this share of a map's samples
LRT_EMITTER_ENVMAP = 1          # include/liverrt.h


def _random_map(w, h, seed):
    return (10.0 ** np.random.default_rng(seed).uniform(-1.5, 1.5, (h, w, 3))).astype(np.float32)        # three decades


def texels(name):
    if name == "const_2x3": return np.ones((3, 2, 3), np.float32)
    if name == "const_100x100": return np.ones((100, 100, 3), np.float32)
    if name == "one_texel_10x100":
        t = np.zeros((100, 10, 3), np.float32); t[40, 5] = 1; return t
    if name == "zeros_16x9":
        t = _random_map(16, 9, 16); t[3:6, 5:9] = 0; t[:, 0] = 0; return t       # an interior block and the column at the u seam
    w, h = (int(x) for x in name.split("_")[1].split("x"))
    return _random_map(w, h, w * 100 + h)


def emitter_xml(mi, tmp_path, name):
    if name == "cavidade":
        return f'<emitter type="envmap"><string name="filename" value="{ASSET}"/></emitter>'
    path = os.path.join(str(tmp_path), name + ".exr")
    mi.write_exr(path, texels(name))
    extra = '<float name="scale" value="2.5"/>' + LIVER_TO_WORLD if name == "rotated_17x9" else ""
    return f'<emitter type="envmap"><string name="filename" value="{path}"/>{extra}</emitter>'


def scene_xml(emitter, shapes="", integrator="path", res=8, spp=1, media=""):
    return f"""<scene version="3.0.0"><integrator type="{integrator}"><integer name="max_depth" value="8"/></integrator>{media}
      <sensor type="perspective"><transform name="to_world"><lookat origin="0, 0, 5" target="0, 0, 0" up="0, 1, 0"/></transform>
        <sampler type="independent"><integer name="sample_count" value="{spp}"/></sampler>
        <film type="hdrfilm"><integer name="width" value="{res}"/><integer name="height" value="{res}"/><rfilter type="box"/></film></sensor>
      {shapes}{emitter}</scene>"""


def reference_of(sc):
    """the float64 reference of the scene's envmap, from the texels as the loader read them back"""
    for k in range(sc.desc.n_emitters):
        e = sc.desc.emitters[k]
        if e.type == LRT_EMITTER_ENVMAP:
            t = np.ctypeslib.as_array(e.data, shape=(e.height, e.width, 3)).copy()
            m = np.array(list(e.to_world), np.float64).reshape(4, 4)[:3, :3]
            return er.EnvmapRef(t, e.scale, m)
    raise ValueError("no envmap emitter")


def load(mi, tmp_path, name):
    sc = mi.load_string(scene_xml(emitter_xml(mi, tmp_path, name)))
    return sc, reference_of(sc)


def load_two_emitters(mi, tmp_path):
    """the 17x9 map beside a small, distant rectangle light (the area emitter comes first: the envmap is emitter 1 of 2)"""
    rect = ('<shape type="rectangle"><transform name="to_world"><scale value="0.01"/><translate y="50"/></transform>'
            '<emitter type="area"><rgb name="radiance" value="1"/></emitter></shape>')
    sc = mi.load_string(scene_xml(emitter_xml(mi, tmp_path, "rand_17x9"), rect))
    assert sc.desc.n_emitters == 2 and sc.desc.emitters[1].type == LRT_EMITTER_ENVMAP
    return sc, reference_of(sc)


def load_cube(mi, tmp_path, name):
    """check g: a dielectric-bounded homogeneous cube under the map, volpath, 32 x 32 pixels at 16 spp"""
    media = ('<medium type="homogeneous" id="fog"><rgb name="sigma_t" value="2.0, 1.5, 1.0"/><rgb name="albedo" value="0.9, 0.8, 0.7"/>'
             '<phase type="hg"><float name="g" value="0.3"/></phase></medium>')
    cube = '<shape type="cube"><bsdf type="dielectric"/><ref name="interior" id="fog"/></shape>'
    return mi.load_string(scene_xml(emitter_xml(mi, tmp_path, name), cube, "volpath", 32, 16, media))


# --------------------------------------------------------------------------------------------------------------- samples
def round_trip_samples():
    """2^16 uniform samples and a 64 x 64 grid that holds the exact values 0, 1, 2^-24 and 1 - 2^-24"""
    s = np.random.default_rng(20240).random((N_ROUND_TRIP, 2), dtype=np.float32)
    g = np.linspace(0, 1, 64).astype(np.float32); g[1] = 2.0 ** -24; g[-2] = 1 - 2.0 ** -24
    return np.concatenate([s, np.stack(np.meshgrid(g, g), -1).reshape(-1, 2)]).astype(np.float32)


def chi2_samples():
    return np.random.default_rng(77).random((N_CHI2, 2), dtype=np.float32)


def chosen_directions(ref):
    """Check e: the six axes; both poles, directions within 1e-6 of them (their float32 y is exactly +-1) and a ladder of unit
    directions whose float32 y is 1, 2, 4, ... 1024 floats off +-1 (sin theta from 3.5e-4, the smallest a float32 unit vector off
    the pole has, to 1.1e-2); the u = 0/1 seam and one float either side of it; all of these in the map's frame and carried
    through its rotation; and 4096 random directions.  Returns float32 world directions."""
    rng = np.random.default_rng(5)
    axes = np.concatenate([np.eye(3), -np.eye(3)])
    az = rng.uniform(0, 2 * np.pi, 16)
    near = lambda s: np.stack([1e-6 * np.cos(az), np.full(16, s), 1e-6 * np.sin(az)], 1)
    y = 1 - 2.0 ** np.arange(-24, -13)                          # exact in float32
    y, za = np.repeat(np.concatenate([y, -y]), 8), rng.uniform(0, 2 * np.pi, 8 * 22)
    ladder = np.stack([np.sqrt(1 - y * y) * np.cos(za), y, np.sqrt(1 - y * y) * np.sin(za)], 1)
    poles = np.concatenate([[[0, 1, 0], [0, -1, 0]], near(1.0), near(-1.0), ladder])
    # u = 0 where atan2(x, -z) / 2 pi = 0.5 / w; atan2's own cut is at x = 0, z > 0 (its value jumps from pi to -pi)
    th = np.pi * np.linspace(0.05, 0.95, 19)
    seam = []
    for phi in (2 * np.pi * 0.5 / ref.w, np.pi):
        for k in (-1, 0, 1):
            p = np.float32(phi) if k == 0 else np.nextafter(np.float32(phi), np.float32(phi + k))
            seam.append(np.stack([np.sin(p) * np.sin(th), np.cos(th), -np.cos(p) * np.sin(th)], 1))
    cut = np.stack([np.float32(k) * np.float32(1e-45) * np.ones_like(th) for k in (-1, 0, 1)])       # x = -denormal, 0, +denormal at z > 0
    seam += [np.stack([c, np.cos(th), np.sin(th)], 1) for c in cut]
    seam = np.concatenate(seam)
    rnd = rng.normal(size=(4096, 3)); rnd /= np.linalg.norm(rnd, axis=1, keepdims=True)
    local = np.concatenate([poles, seam])
    return np.concatenate([axes, local, local @ ref.to_world.T, rnd]).astype(np.float32)


# ------------------------------------------------------------------------------------------------- the oracle as a probe
def orc_dirs(o, d):
    """orc.envmap_pdf and orc.envmap_eval at n directions: (pdf, rgb)"""
    return o.envmap_pdf_eval_n(d)


def orc_sample(o, smp):
    d, pdf, w = o.envmap_sample_n(smp)
    return {"d": d, "pdf": pdf, "weight": w}


def orc_probe(o, smp, hits=True):
    pr = orc_sample(o, smp)
    if hits:
        pr["hit_pdf"], pr["hit_le"] = orc_dirs(o, pr["d"])
        dead = pr["pdf"] == 0                                  # (the device's probe sends no ray for a sample of pdf 0)
        pr["hit_pdf"][dead] = 0; pr["hit_le"][dead] = 0
    return pr


# ------------------------------------------------------------------------------------------------------------ the checks
def check_round_trip(ref, pr, smp, label, sx_scale=1.0, sx_offset=0.0):
    """a: the inverse warp at the returned direction gives the input sample back.  (sx_scale, sx_offset): the re-stretching of sx
    when the scene holds more than one emitter.  Returns (largest error / bound, largest error)."""
    live = pr["pdf"] > 0
    sx = np.clip(smp[live, 0].astype(np.float64) * sx_scale - sx_offset, 0, 1); sy = smp[live, 1].astype(np.float64)
    ratio, err, p, located = ref.round_trip(pr["d"][live], sx, sy)
    assert live.mean() > 0.99 and located.mean() >= 1 - POLE_SHARE, (label, live.mean(), located.mean())
    assert (ref.dir_to_uv(pr["d"][live][~located])[2] < POLE_SIN).all()
    ratio, err, p, s = ratio[located], err[located], p[located], smp[live][located]
    k = int(np.argmax(ratio))
    print(f"[envmap a] {label}: n={len(err)} max error/bound {ratio[k]:.3f} (error there {err[k]:.3e}, patch probability {p[k]:.3e}), "
          f"median error {np.median(err):.3e}, level term of the bound {ref.level_error():.3e}")
    assert (ratio <= 1).all(), (label, s[k], err[k], ratio[k])
    return float(ratio[k]), float(err[k])


def check_pdf_and_weight(ref, pr, label, pmf=1.0):
    """b and d: the pdf is the float64 density at the returned direction and equals hit_pdf; weight * pdf and hit_le are the
    float64 radiance there; samples of pdf 0 carry weight 0.  Returns the largest error / tolerance of (pdf, hit_pdf, weight, hit_le)."""
    d, pdf, w = pr["d"], pr["pdf"].astype(np.float64), pr["weight"].astype(np.float64)
    assert np.isfinite(pdf).all() and (pdf >= 0).all() and np.isfinite(w).all() and (w >= 0).all()
    dead = pdf == 0
    assert (w[dead] == 0).all()
    d = np.where(dead[:, None], np.float32([1, 0, 0]), d)          # (a sample of pdf 0 has no direction to speak of)
    u, v, st = ref.dir_to_uv(d)
    pole = st < POLE_SIN
    assert pole.mean() <= POLE_SHARE, (label, pole.mean())
    ok = ~pole & ~dead
    want = ref.pdf(d) * pmf
    tol = ref.pdf_tolerance(want, st) * pmf
    rad = ref.radiance(d)
    rtol = ref.radiance_tolerance(rad, st)
    out = []
    for name, got in (("pdf", pdf), ("hit_pdf", pr["hit_pdf"].astype(np.float64))):
        r = np.abs(got - want)[ok] / tol[ok]
        out.append(float(r.max()))
        print(f"[envmap b] {label}: {name} max error/tolerance {r.max():.3f}, max relative error {(np.abs(got - want)[ok] / want[ok]).max():.3e}")
    # the reference's own assertion: the sampled pdf equals pdf_direction to rtol 1e-3
    assert (np.abs(pr["hit_pdf"].astype(np.float64) - pdf) <= 1e-3 * pdf + tol - ref.RTOL * want * pmf)[ok].all()
    # weight * pdf: one more rounding each for the division and the product, and the weight carries 1 / pmf
    for name, got in (("weight*pdf", w * pdf[:, None]), ("hit_le", pr["hit_le"].astype(np.float64))):
        r = (np.abs(got - rad) / (rtol + 2 * er.F32_EPS * np.abs(rad) + 1e-300))[ok]
        out.append(float(r.max()))
        print(f"[envmap d] {label}: {name} max error/tolerance {r.max():.3f}")
    assert max(out) <= 1.0, (label, out)
    return out


def uv_counts(ref, d):
    u, v, _ = ref.dir_to_uv(d, wrap_v=False)
    nu, nv = CHI2_GRID
    iu = np.minimum((u * nu).astype(np.int64), nu - 1); iv = np.minimum((v * nv).astype(np.int64), nv - 1)
    return np.bincount(iv * nu + iu, minlength=nu * nv).reshape(nv, nu)


def check_chi2(ref, d, label):
    """c: 2^18 directions binned on 64 x 32 in (u, v) against the exact box integrals, significance 0.01 with the Sidak
    correction over the maps"""
    nu, nv = CHI2_GRID
    expected = ref.box_masses(np.linspace(0, 1, nu + 1), np.linspace(0, 1, nv + 1)) * len(d)
    assert abs(expected.sum() - len(d)) < 1e-6 * len(d)
    stat, dof, p = er.chi_square(uv_counts(ref, d), expected)
    alpha = er.sidak(0.01, len(MAPS))
    print(f"[envmap c] {label}: chi2 {stat:.1f} on {dof} dof, p-value {p:.4f} (threshold {alpha:.5f})")
    assert dof >= 8, (label, dof)
    assert p > alpha, (label, stat, dof, p)
    return p


def check_directions(ref, d, pdf, rgb, label, pmf=1.0):
    """e: pdf_emitter_direction and the emitter's eval at given directions against float64, under the tolerances of b and d.

    A map without a transform reads the direction as given, so every direction is held to the value, the poles included
    (envmap_ref.py, "At the poles"): where the float32 y is +-1 the pdf is exactly 0 whatever x and z are, and the radiance is
    row 0 at the direction's azimuth; the (u, v) uncertainty is that of atan2 and acos alone, which keeps the tolerance
    meaningful down to the first float off a pole.
    Under a rotation the map-frame direction is the kernel's own float32 product, 2^-24 per component off the float64 one: with
    sin theta < POLE_SIN that is as much as the polar angle itself, so there only the sign of the pdf and the range of the
    radiance (the two rows next to either pole) are required, and the full tolerance further out."""
    pdf = pdf.astype(np.float64); rgb = rgb.astype(np.float64); d = np.asarray(d, np.float32)
    assert np.isfinite(pdf).all() and np.isfinite(rgb).all()
    assert (pdf >= 0).all(), (label, d[np.argmin(pdf)], pdf.min())
    u, v, st = ref.dir_to_uv(d)
    exact = ref.reads_direction_as_given
    want = ref.pdf(d) * pmf
    tol = ref.pdf_tolerance(want, st, rounded=not exact) * pmf
    rad = ref.radiance(d)
    rtol = ref.radiance_tolerance(rad, st, rounded=not exact) + 1e-300
    r_pdf, r_rad = np.abs(pdf - want) / (tol + 1e-300), (np.abs(rgb - rad) / rtol).max(1)
    near = st < POLE_SIN
    if exact:
        pole = ref.at_pole(d)
        assert pole.sum() >= 34 and (st[pole] < 2e-6).all() and (st[~pole] > 3.4e-4).all()    # (the least sin theta of a float32 unit vector off the pole)
        assert (pdf[pole] == 0).all() and (want[pole] == 0).all(), (label, d[pole][np.argmax(pdf[pole])], pdf[pole].max())
        held = np.ones(len(d), bool)
        ptol, prtol = ref.pole_tolerances(want / pmf, rad, u, v, st)      # next to a pole: the slopes of the spot, not of the map
        tol = np.where(near, ptol * pmf, tol); rtol = np.where(near[:, None], prtol + 1e-300, rtol)
        r_pdf, r_rad = np.abs(pdf - want) / (tol + 1e-300), (np.abs(rgb - rad) / rtol).max(1)
        r_pdf[pole] = 0
        first = near & ~pole                                       # the first floats off a pole
        print(f"[envmap e] {label}: {pole.sum()} directions with y = +-1: pdf 0, radiance max error/tolerance {r_rad[pole].max():.3f}; {first.sum()} within "
              f"sin theta {POLE_SIN} off them: max error/tolerance pdf {r_pdf[first].max():.3f} radiance {r_rad[first].max():.3f}, "
              f"pdf tolerance / pdf at most {(tol / np.maximum(want, 1e-300))[first & (want > 0)].max(initial=0):.3g}")
    else:
        held = ~near
        rows = ref.rgb[[0, 1, ref.h - 2, ref.h - 1]] * ref.scale
        assert (rgb[near] >= rows.min((0, 1)) * (1 - ref.RTOL)).all() and (rgb[near] <= rows.max((0, 1)) * (1 + ref.RTOL)).all()
    print(f"[envmap e] {label}: {len(d)} directions, {held.sum()} held to the value: max error/tolerance pdf {r_pdf[held].max():.3f} "
          f"radiance {r_rad[held].max():.3f}; smallest sin theta among them off a pole {st[held & (st > 2e-6)].min():.2e}")
    assert (r_pdf[held] <= 1).all() and (r_rad[held] <= 1).all(), (label, d[np.argmax(r_pdf * held)], (r_pdf * held).max(), d[np.argmax(r_rad * held)], (r_rad * held).max())
    lo, hi = ref.rgb.min() * ref.scale, ref.rgb.max() * ref.scale
    assert (rgb >= lo * (1 - ref.RTOL)).all() and (rgb <= hi * (1 + ref.RTOL)).all()
    return float(r_pdf[held].max()), float(r_rad[held].max())
