"""Scene generators shared by the tests and by bench.py's f4 configurations (`--config het`, `--config mis`): the fog box of the
reference's own fog render (MitsubaRunner.py:8-40 recipe), and a grid-volume medium in a box."""
import numpy as np


def fog_xml(md="12", rf="gaussian", sensor_medium="", exterior="", env=""):
    return f"""<scene version="3.0.0">
  <integrator type="volpath"><integer name="max_depth" value="{md}"/></integrator>
  <medium type="homogeneous" id="fog"><rgb name="sigma_t" value="1.5, 0.7, 2.0"/><rgb name="albedo" value="0.9, 0.95, 0.6"/>
    <phase type="hg"><float name="g" value="0.5"/></phase></medium>
  <medium type="homogeneous" id="haze"><float name="sigma_t" value="0.05"/><float name="albedo" value="0.8"/>
    <boolean name="has_spectral_extinction" value="false"/></medium>
  <sensor type="perspective"><float name="fov" value="40"/>
    <transform name="to_world"><lookat origin="3, 2.5, 4" target="0, 0, 0" up="0, 1, 0"/></transform>
    <sampler type="independent"><integer name="sample_count" value="32"/></sampler>
    <film type="hdrfilm"><integer name="width" value="64"/><integer name="height" value="48"/><rfilter type="{rf}"/></film>
    {sensor_medium}
  </sensor>
  <shape type="cube"><bsdf type="null"/><ref name="interior" id="fog"/>{exterior}</shape>
  <shape type="rectangle"><transform name="to_world"><scale value="6"/><rotate x="1" angle="-90"/><translate y="-1.001"/></transform>
    <bsdf type="diffuse"><texture name="reflectance" type="checkerboard"><transform name="to_uv"><scale x="8" y="8"/></transform></texture></bsdf>{exterior}</shape>
  <shape type="rectangle"><transform name="to_world"><scale value="0.7"/><rotate x="1" angle="90"/><translate y="3.5"/></transform>
    <emitter type="area"><rgb name="radiance" value="20, 18, 15"/></emitter>{exterior}</shape>
  {env}
</scene>"""


def het_xml(vol, sampler="independent", spectral="true", boundary="null", extra_medium="", inside_ref="smoke", md=12):
    return f"""<scene version="3.0.0">
  <integrator type="volpath"><integer name="max_depth" value="{md}"/></integrator>
  <medium type="heterogeneous" id="smoke">
    <volume name="sigma_t" type="gridvolume"><string name="filename" value="{vol}"/>
      <transform name="to_world"><scale value="2"/><translate x="-1" y="-1" z="-1"/></transform></volume>
    <rgb name="albedo" value="0.9, 0.8, 0.6"/><float name="scale" value="3"/><boolean name="has_spectral_extinction" value="{spectral}"/>
    <phase type="hg"><float name="g" value="0.3"/></phase>
  </medium>
  {extra_medium}
  <sensor type="perspective"><float name="fov" value="40"/>
    <transform name="to_world"><lookat origin="3, 2.5, 4" target="0, 0, 0" up="0, 1, 0"/></transform>
    <sampler type="{sampler}"><integer name="sample_count" value="16"/></sampler>
    <film type="hdrfilm"><integer name="width" value="64"/><integer name="height" value="48"/><rfilter type="box"/></film>
  </sensor>
  <shape type="cube"><bsdf type="{boundary}"/><ref name="interior" id="{inside_ref}"/></shape>
  <shape type="rectangle"><transform name="to_world"><scale value="6"/><rotate x="1" angle="-90"/><translate y="-1.001"/></transform>
    <bsdf type="diffuse"><texture name="reflectance" type="checkerboard"><transform name="to_uv"><scale x="8" y="8"/></transform></texture></bsdf></shape>
  <shape type="rectangle"><transform name="to_world"><scale value="0.7"/><rotate x="1" angle="90"/><translate y="3.5"/></transform>
    <emitter type="area"><rgb name="radiance" value="20, 18, 15"/></emitter></shape>
  <emitter type="constant"><rgb name="radiance" value="0.3, 0.4, 0.6"/></emitter>
</scene>"""


TWO_MEDIA_FOG = '<medium type="homogeneous" id="fog"><rgb name="sigma_t" value="0.9, 0.3, 1.6"/><rgb name="albedo" value="0.8, 0.8, 0.9"/><boolean name="has_spectral_extinction" value="false"/></medium>'


def two_media_xml(vol, hom=TWO_MEDIA_FOG, **kw):
    """het_xml plus a second box filled with a homogeneous medium next to the grid volume"""
    return het_xml(vol, extra_medium=hom, **kw).replace('<shape type="rectangle"><transform name="to_world"><scale value="6"/>',
        '<shape type="cube"><transform name="to_world"><scale value="0.5"/><translate x="2" y="-0.4"/></transform><bsdf type="null"/><ref name="interior" id="fog"/></shape>'
        '<shape type="rectangle"><transform name="to_world"><scale value="6"/>')


def smoke_grid(seed=3, shape=(12, 10, 8)):
    """the density grid of the heterogeneous-medium tests"""
    return (0.05 + np.random.default_rng(seed).random(shape) ** 3).astype(np.float32)


def resized(xml, width, height, spp):
    """the same scene at another film size / sample count (the generators above hard-code small ones)"""
    import re
    xml = re.sub(r'<integer name="width" value="\d+"/>', f'<integer name="width" value="{width}"/>', xml)
    xml = re.sub(r'<integer name="height" value="\d+"/>', f'<integer name="height" value="{height}"/>', xml)
    return re.sub(r'<integer name="sample_count" value="\d+"/>', f'<integer name="sample_count" value="{spp}"/>', xml)


def sphere_fuzz_xml(seed, assets):
    """An opt-in family for the random-scene tests (its own generator state: the other families draw what they drew before it existed):
    0 - 3 sphere shapes with a random BSDF and, often, an interior medium, 0 - 2 cubes, a floor, and optionally a point light beside or
    instead of an area light and an environment; path / volpath / volpathmis on homogeneous media, biovolpath / biovolpath06 on tissue
    media.  Spheres may overlap each other and the cubes, sit on the floor or hold the camera's view ray; `flip_normals` is drawn too.
    Returns (xml, integrator)."""
    r = np.random.default_rng(30_000 + seed)
    pick = lambda *a: a[int(r.integers(len(a)))]
    f3 = lambda lo, hi: ", ".join(f"{x:.4g}" for x in r.uniform(lo, hi, 3))
    integrator = pick("path", "volpath", "volpath", "volpathmis", "volpathmis", "biovolpath", "biovolpath06")
    bio = integrator.startswith("bio")
    n_media = 0 if integrator == "path" else int(r.integers(1, 3))
    media = []
    for m in range(n_media):
        phase = pick('<phase type="isotropic"/>', f'<phase type="hg"><float name="g" value="{r.uniform(-0.8, 0.8):.3f}"/></phase>')
        common = (f'<rgb name="sigma_t" value="{f3(0.2, 2.0)}"/><boolean name="has_spectral_extinction" value="{pick("true", "false")}"/>'
                  f'<boolean name="sample_emitters" value="{pick("true", "true", "false")}"/><float name="scale" value="{r.uniform(0.5, 2):.3f}"/>{phase}')
        if bio:
            kind = pick("liver", "parenchyma", "glissonCapsule")
            lim = np.sort(r.uniform(0.03, 0.7, 4))
            coeffs = "".join(f'<float name="sigma_{k}{l}_{c}" value="{r.uniform(0.05, 3.0):.4f}"/>' for k in ("collagen", "elastin") for l in range(1, 5) for c in "RGB")
            limits = "".join(f'<float name="layer{i + 1}Limit" value="{lim[i]:.4f}"/>' for i in range(4))
            par = (f'<rgb name="sigma_blood" value="{f3(0.01, 1.2)}"/><rgb name="sigma_bile" value="{f3(0.0, 0.4)}"/><rgb name="sigma_lipid_water" value="{f3(0.0, 0.3)}"/>'
                   f'<float name="sigma_hepatocity" value="{r.uniform(0.5, 300):.3f}"/>')
            body = {"liver": coeffs + limits + par, "parenchyma": par, "glissonCapsule": coeffs + limits}[kind]
            media.append(f'<medium type="{kind}" id="m{m}">{body}{common}</medium>')
        else:
            media.append(f'<medium type="homogeneous" id="m{m}"><rgb name="albedo" value="{f3(0.3, 1.0)}"/>{common}</medium>')

    def bsdf(allow_null):
        k = pick(*(["diffuse", "diffuse_tex", "dielectric", "dielectric"] + (["null"] if allow_null else [])))
        if k == "diffuse": return f'<bsdf type="diffuse"><rgb name="reflectance" value="{f3(0.1, 0.9)}"/></bsdf>'
        if k == "diffuse_tex": return ('<bsdf type="diffuse"><texture name="reflectance" type="checkerboard"><transform name="to_uv">'
                                        f'<scale x="{r.uniform(2, 9):.2f}" y="{r.uniform(2, 9):.2f}"/></transform></texture></bsdf>')
        if k == "dielectric": return f'<bsdf type="dielectric"><float name="int_ior" value="{r.uniform(1.1, 1.7):.3f}"/><float name="ext_ior" value="1"/></bsdf>'
        return '<bsdf type="null"/>'

    def interior():
        return f'<ref name="interior" id="m{int(r.integers(n_media))}"/>' if n_media and r.random() < 0.8 else ""
    shapes = []
    for k in range(int(r.integers(0, 4))):
        inside = interior()
        flip = '<boolean name="flip_normals" value="true"/>' if r.random() < 0.2 else ""
        radius = r.uniform(0.3, 1.1)
        y = radius - 1.2 if r.random() < 0.3 else r.uniform(-0.4, 1.0)             # tangent to the floor (the equal-t tie), or anywhere
        shapes.append(f'<shape type="sphere"><point name="center" x="{r.uniform(-1.6, 1.6):.3f}" y="{y:.4f}" z="{r.uniform(-1.6, 1.6):.3f}"/>'
                      f'<float name="radius" value="{radius:.4f}"/>{flip}{bsdf(bool(inside))}{inside}</shape>')
    for k in range(int(r.integers(0, 3))):
        inside = interior()
        tr = (f'<transform name="to_world"><scale value="{r.uniform(0.4, 1.1):.3f}"/><rotate x="{r.random():.3f}" y="{r.random():.3f}" z="{r.random() + 0.1:.3f}" angle="{r.uniform(0, 90):.1f}"/>'
              f'<translate x="{r.uniform(-1.6, 1.6):.3f}" y="{r.uniform(-0.4, 1.0):.3f}" z="{r.uniform(-1.6, 1.6):.3f}"/></transform>')
        shapes.append(f'<shape type="cube">{tr}{bsdf(bool(inside))}{inside}</shape>')
    if r.random() < 0.85:
        shapes.append(f'<shape type="rectangle"><transform name="to_world"><scale value="6"/><rotate x="1" angle="-90"/><translate y="-1.2"/></transform>{bsdf(False)}</shape>')
    emitters = []
    if r.random() < 0.5:
        emitters.append(f'<emitter type="point"><point name="position" x="{r.uniform(-2.5, 2.5):.3f}" y="{r.uniform(1.5, 4):.3f}" z="{r.uniform(-2.5, 2.5):.3f}"/>'
                        f'<rgb name="intensity" value="{f3(3, 20)}"/></emitter>')
    if r.random() < 0.4:
        emitters.append(f'<shape type="rectangle"><transform name="to_world"><scale value="{r.uniform(0.3, 1.2):.3f}"/><rotate x="1" angle="90"/>'
                        f'<translate x="{r.uniform(-1, 1):.3f}" y="{r.uniform(2.5, 4):.3f}" z="{r.uniform(-1, 1):.3f}"/></transform>'
                        f'<emitter type="area"><rgb name="radiance" value="{f3(5, 25)}"/></emitter></shape>')
    env = pick("none", "constant", "envmap") if emitters else pick("constant", "envmap")
    if env == "constant": emitters.append(f'<emitter type="constant"><rgb name="radiance" value="{f3(0.2, 1.2)}"/></emitter>')
    if env == "envmap": emitters.append(f'<emitter type="envmap"><string name="filename" value="{assets}/cavidade_latitude.exr"/><float name="scale" value="{r.uniform(0.5, 3):.3f}"/>'
                                        f'<transform name="to_world"><rotate y="1" angle="{r.uniform(0, 360):.1f}"/></transform></emitter>')
    r.shuffle(emitters)                                                              # (the selection pmf's order: the point light first, last or between)
    sampler = pick("independent", "independent", "ldsampler")
    spp = pick(8, 8, 5, 3, 1) if sampler != "ldsampler" else 4
    fw, fh = (32, 24) if r.random() < 0.6 else (int(r.integers(17, 40)), int(r.integers(9, 30)))
    max_depth = pick(3, 6, 12, 30) if sampler == "ldsampler" else pick(-1, 3, 6, 12)
    smis_xml = f'<boolean name="use_spectral_mis" value="{pick("true", "false")}"/>' if integrator == "volpathmis" else ""
    xml = f"""<scene version="3.0.0">
  <integrator type="{integrator}"><integer name="max_depth" value="{max_depth}"/><integer name="rr_depth" value="{pick(1, 3, 5)}"/>
    <boolean name="hide_emitters" value="{pick("false", "false", "true")}"/>{smis_xml}</integrator>
  {''.join(media)}
  <sensor type="perspective"><float name="fov" value="{r.uniform(30, 60):.2f}"/>
    <transform name="to_world"><lookat origin="{r.uniform(2.5, 4):.3f}, {r.uniform(1, 3):.3f}, {r.uniform(2.5, 4.5):.3f}" target="0, 0, 0" up="0, 1, 0"/></transform>
    <sampler type="{sampler}"><integer name="sample_count" value="{spp}"/><integer name="seed" value="{int(r.integers(0, 5))}"/></sampler>
    <film type="hdrfilm"><integer name="width" value="{fw}"/><integer name="height" value="{fh}"/><string name="pixel_format" value="{pick("rgb", "rgba")}"/><rfilter type="{pick("box", "gaussian", "tent")}"/></film>
  </sensor>
  {''.join(shapes)}
  {''.join(emitters)}
</scene>"""
    return xml, integrator
