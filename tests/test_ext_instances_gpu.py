"""The `EXT` kernel instances (scenes with sphere shapes, point emitters or mesh area emitters: DESIGN.md §2, §14) against the CPU oracle by a
differential scene that asks nothing of the oracle's own sphere code: the hidden sphere.

Every scene is built twice from one description.  (a) holds a small closed diffuse cube, the "vault", outside every medium boundary and
away from the camera.  (b) is (a) plus one diffuse sphere wholly inside the vault, appended as the last shape, so no shape, face or emitter
index moves.  The vault is opaque and closed, so no path reaches the sphere; the sphere lies inside the vault, so the scene's bounds (and
the bounding sphere the constant and envmap emitters read) are those of (a); the emitter list is that of (a).  Scene (b) selects the EXT
instances of `k_render` and `k_trace[_lds]` with their wide path records, and must give the ORACLE'S lanes of scene (a) bit for bit, with
the oracle's loop-trip and shadow-ray counts, and the oracle's film up to the order of the float atomics.

What a wrong EXT instance would break here: the triangle / emitter / medium branches the EXT instances share with the plain ones (an RNG
draw out of order, a wrong record field in the wide layout, a miscompiled spill), the `maxt` tightening of the EXT tracer (rays towards
the vault meet the sphere's `t` first and must still return the wall in front of it), the any-hit order (a shadow ray through the vault
is stopped by the sphere test before the BVH is walked: occluded either way), and the distance field with a sphere folded into it."""
import os

import numpy as np
import pytest

from conftest import LIVER_XML
from scene_gen import fog_xml, het_xml, two_media_xml, smoke_grid, resized
from test_bio_gpu import bio_xml
from test_parity_gpu import assert_lanes_equal, bits, film_close

pytestmark = pytest.mark.gpu

W, H, SPP = 32, 24, 4                    # (4 = 4^1: the ld sampler keeps it)


def vault_xml(c, half):
    return (f'<shape type="cube"><transform name="to_world"><scale value="{half}"/><translate x="{c[0]}" y="{c[1]}" z="{c[2]}"/></transform>'
            '<bsdf type="diffuse"/></shape>')


def sphere_xml(c, r):
    return f'<shape type="sphere"><point name="center" x="{c[0]}" y="{c[1]}" z="{c[2]}"/><float name="radius" value="{r}"/><bsdf type="diffuse"/></shape>'


def with_shapes(xml, *shapes):
    """the scene with these shapes appended after every shape it has"""
    assert xml.count("</scene>") == 1
    return xml.replace("</scene>", "".join(shapes) + "</scene>")


# The fog-box layout of scene_gen / bio_xml: cube [-1, 1]^3, floor at y = -1.001, area light at y = 3.5, camera at (3, 2.5, 4).  The vault
# floats between the cube and the light: in the camera's view, and in the way of the shadow rays from the cube's top to the light.
BOX_CAM, BOX_VAULT = (3.0, 2.5, 4.0), ((0.0, 1.35, 0.0), 0.25, 0.15)
# Cornell box: the vault floats above the large box, inside the room.
CORNELL_CAM, CORNELL_VAULT = (0.0, 0.0, 3.9), ((0.1, 0.45, 0.5), 0.15, 0.1)
# Liver-SingleMesh: 30 units down the camera's axis, 6 to the side, in front of the liver.
LIVER_CAM, LIVER_VAULT = (7.481132, 5.343665, 6.507640), ((-7.1, -5.1, -12.7), 2.0, 1.0)

CASES = ["path-cornell", "volpath-fog", "volpath-liver", "volpath-het", "volpathmis-spectral", "volpathmis-plain", "biovolpath", "biovolpath06"]


def case_scene(mi, case, sampler, tmp_path):
    """(xml, base_dir, defines, camera origin, (vault centre, vault half width, sphere radius)) of a case: scene (a) without its vault"""
    base, defines = ".", {}
    if case == "path-cornell":
        d = mi.cornell_box(); d['sensor']['film'].update({'width': W, 'height': H})
        d['sensor']['sampler'] = {'type': sampler, 'sample_count': SPP}
        return mi.dict_to_xml(d), base, defines, CORNELL_CAM, CORNELL_VAULT
    if case == "volpath-liver":
        xml = open(LIVER_XML).read()
        return (xml.replace('<sampler type="independent">', f'<sampler type="{sampler}">'), os.path.dirname(LIVER_XML),
                dict(integrator="volpath", spp=SPP, res_width=W, res_height=H), LIVER_CAM, LIVER_VAULT)
    if case == "volpath-fog":
        xml = fog_xml()
    elif case in ("biovolpath", "biovolpath06"):
        xml = bio_xml("liver", case, "null")
    else:
        vol = os.path.join(str(tmp_path), "smoke.vol"); mi.write_volume_grid(vol, smoke_grid())
        if case == "volpath-het":
            xml = het_xml(vol)
        else:
            smis = "true" if case == "volpathmis-spectral" else "false"
            xml = two_media_xml(vol).replace('<integrator type="volpath">', f'<integrator type="volpathmis"><boolean name="use_spectral_mis" value="{smis}"/>')
    assert xml.count('<sampler type="independent">') == 1
    xml = resized(xml, W, H, SPP).replace('<sampler type="independent">', f'<sampler type="{sampler}">')
    return xml, base, defines, BOX_CAM, BOX_VAULT


def check_runs_ext(a, b):
    """`D->ext` seen from outside: prbvolpath has no EXT instances and refuses the scene that selects them"""
    a.render(integrator="prbvolpath", spp=1)
    with pytest.raises(RuntimeError, match="unsupported: prbvolpath"):
        b.render(integrator="prbvolpath", spp=1)


@pytest.mark.parametrize("setting", ["independent-lds", "ld-lds", "independent-global"])
@pytest.mark.parametrize("case", CASES)
def test_hidden_sphere_lanes_equal_the_oracles(mi, orc, monkeypatch, tmp_path, case, setting):
    sampler = "ldsampler" if setting.startswith("ld") else "independent"
    if setting.endswith("global"):
        monkeypatch.setenv("LRT_NO_LDS_BVH", "1")
    xml, base, defines, cam, (c, half, r) = case_scene(mi, case, sampler, tmp_path)
    xml_a = with_shapes(xml, vault_xml(c, half))
    xml_b = with_shapes(xml_a, sphere_xml(c, r))
    a = mi.load_string(xml_a, base, **defines)
    b = mi.load_string(xml_b, base, **defines)
    assert a.film_shape()[:2] == (H, W) and a.spp == SPP and a.desc.sampler_type == (1 if sampler == "ldsampler" else 0)
    assert b.desc.n_faces == a.desc.n_faces and b.desc.n_shapes == a.desc.n_shapes + 1 and b.desc.n_emitters == a.desc.n_emitters
    check_runs_ext(a, b)
    o = orc.OrcScene(a)
    n = W * H * SPP
    # a ray from the camera to the vault's centre: the EXT tracer meets the sphere first and must still return the vault's wall (one of the
    # last 12 faces) in front of it, with the oracle's t, u, v bit for bit; the any-hit query is occluded
    org = np.float32([cam]); d = np.float32([c]) - org; dist = np.linalg.norm(d); d /= dist
    tmax = np.float32([np.finfo(np.float32).max])
    gt, ct = b.trace(org, d, tmax), o.trace(org, d, tmax, brute_force=True)
    assert a.desc.n_faces - 12 <= gt[3][0] < a.desc.n_faces and gt[0][0] < dist - r
    for x, y in zip(gt, ct):
        assert (bits(x) == bits(y)).all() if x.dtype == np.float32 else (x == y).all()
    assert b.trace(org, d, tmax, any_hit=True)[0][0] == 0
    # the plain instance on (a) first, so that a failure below names the EXT instance and not the scene
    assert_lanes_equal(a, o, 0, n, seed=3)
    g = assert_lanes_equal(b, o, 0, n, seed=3)
    assert np.isfinite(g).all() and (g[:, :3] > 0).any()
    raw = b.render(return_raw=True, seed=3)[1]
    st = b.stats()
    oraw = o.render(return_raw=True, seed=3)[1]
    assert st["n_iter"] == o.last_stats["n_iter"] and st["n_shadow"] == o.last_stats["n_shadow_needed"]
    assert film_close(raw, oraw).all()


def test_a_reachable_sphere_changes_the_lanes(mi, orc):
    """The same comparison with the sphere OUTSIDE the vault, in view of the camera, must fail: the test above can see a difference."""
    xml, base, defines, cam, (c, half, r) = case_scene(mi, "volpath-fog", "independent", None)
    xml_a = with_shapes(xml, vault_xml(c, half))
    a = mi.load_string(xml_a, base, **defines)
    b = mi.load_string(with_shapes(xml_a, sphere_xml((c[0] + 0.6, c[1], c[2] + 0.6), r)), base, **defines)
    check_runs_ext(a, b)
    n = W * H * SPP
    g = b.render_samples(0, n, seed=3); ref = orc.OrcScene(a).render_samples(0, n, seed=3)
    differ = (bits(g) != bits(ref)).any(axis=1)
    assert differ.sum() > 10
