"""The per-face cone table (scene_prep.cpp: build_cone_table) lets the 64-byte-record volpath kernels prove free the
segments that start on a surface, which the distance field never can.  A proof only elides a ray query that finds nothing, so the table
may be visible in speed and in `n_proven` alone: every lane bit-identical with and without it (LRT_NO_CONE_PROOF, read when the scene is
uploaded) and to the CPU oracle, the same trips, shadow queries and records.

Liver-SingleMesh at 128 x 72 x 16 spp, both samplers; the same with the 80-byte kernels (which do not read the table: `n_proven` equal
too), with every scatter through the emitter sampling, and with a medium so thin that the free flights outrun the table's lengths.
The worst case for a wrong row is a fold: a box whose floor is folded up by 45 degrees into the medium, where a row one bin too generous sends
a path through the folded wall; its lanes are held to the oracle."""
import re

import numpy as np
import pytest

from test_closed_kernel_lean_gpu import thin
from test_closed_records_gpu import ld, liver
from test_parity_gpu import assert_lanes_equal, bits

pytestmark = pytest.mark.gpu

COUNTS = ("n_iter", "n_shadow", "n_records")


def lanes_with_and_without(mi, monkeypatch, xml_edit, seed=3, **kw):
    """(lanes, stats, scene) with the table, then without it"""
    out = []
    for table in (True, False):
        if table:
            monkeypatch.delenv("LRT_NO_CONE_PROOF", raising=False)
        else:
            monkeypatch.setenv("LRT_NO_CONE_PROOF", "1")
        sc = liver(mi, xml_edit, **kw)
        n = int(np.prod(sc.film_shape()[:2])) * sc.spp
        out.append((sc.render_samples(0, n, seed=seed), sc.stats(), sc))
    monkeypatch.delenv("LRT_NO_CONE_PROOF", raising=False)
    return out


def assert_table_invisible(mi, orc, monkeypatch, xml_edit=None, closed=True, seed=3):
    (a, sa, sc), (b, sb, _) = lanes_with_and_without(mi, monkeypatch, xml_edit, seed)
    print("table", {k: sa[k] for k in COUNTS + ("n_proven", "record_bytes")}, "none", {k: sb[k] for k in COUNTS + ("n_proven", "record_bytes")})
    assert sa["record_bytes"] == sb["record_bytes"] == (64 if closed else 80) and sa["n_closed_guard"] == 0 and sb["n_closed_guard"] == 0
    same = (bits(a) == bits(b)).all(axis=1)
    assert same.all(), f"{(~same).sum()} of {len(a)} lanes differ with the table; first: lane {int(np.argmin(same))} table={a[np.argmin(same)]} none={b[np.argmin(same)]}"
    for k in COUNTS:
        assert sa[k] == sb[k], (k, sa, sb)
    o = orc.OrcScene(sc)
    c = o.render_samples(0, len(a), seed=seed)
    same = (bits(a) == bits(c)).all(axis=1)
    assert same.all(), f"{(~same).sum()} of {len(a)} lanes differ from the oracle; first: lane {int(np.argmin(same))} gpu={a[np.argmin(same)]} cpu={c[np.argmin(same)]}"
    assert sa["n_iter"] == o.last_stats["n_iter"] and sa["n_shadow"] == o.last_stats["n_shadow_needed"]
    return sa, sb


@pytest.mark.parametrize("sampler", ["independent", "ld"])
def test_liver_lanes_identical_and_more_records_proven(mi, orc, monkeypatch, sampler):
    sa, sb = assert_table_invisible(mi, orc, monkeypatch, ld if sampler == "ld" else None)
    assert sa["n_proven"] > sb["n_proven"] > 0, (sa, sb)


def test_wide_kernels_do_not_read_the_table(mi, orc, monkeypatch):
    monkeypatch.setenv("LRT_NO_CLOSED_RECORDS", "1")
    sa, sb = assert_table_invisible(mi, orc, monkeypatch, closed=False)
    assert sa["n_proven"] == sb["n_proven"], (sa, sb)


def test_every_scatter_through_the_emitter_sampling(mi, orc, monkeypatch):
    monkeypatch.setenv("LRT_NO_NEE_REJECT", "1")
    sa, sb = assert_table_invisible(mi, orc, monkeypatch)
    assert sa["n_proven"] > sb["n_proven"], (sa, sb)


def test_thin_medium_outruns_the_table(mi, orc, monkeypatch):
    """scale 0.015: a mean free path of 67 units in a liver 38 across, so nearly every free flight is longer than its row: what is proven
    here beyond the balls alone comes from the cone as the start of the balls' cover, and from the few flights short enough for their row"""
    sa, sb = assert_table_invisible(mi, orc, monkeypatch, thin)
    assert sa["n_proven"] > sb["n_proven"], (sa, sb)


# ---- the fold
def folded_box_obj(path, deg=45.0):
    """A closed prism: the profile (x, z) = (0, 0) (2, 0) (2 + 2 cos a, 2 sin a) (2 + 2 cos a, 3) (0, 3) swept over y in [0, 4].  Every side is cut
    into quads about one unit wide (the floor and the folded wall 2 x 4 each, as tests/host/cone_proof_main.cpp folds them), so that the faces in
    the middle of a side touch no other side and keep rows; the two ends are fans about their centroids.  Returns the centroid and the face count."""
    a = np.radians(deg); cx, sz = 2 + 2 * np.cos(a), 2 * np.sin(a)
    prof = [(0, 0), (1, 0), (2, 0), (2 + np.cos(a), np.sin(a)), (cx, sz), (cx, 0.5 * (sz + 3)), (cx, 3), (2 * cx / 3, 3), (cx / 3, 3), (0, 3), (0, 1.5)]
    ys = (0.0, 1.0, 2.0, 3.0, 4.0)
    verts = [(x, y, z) for y in ys for (x, z) in prof]
    idx = lambda j, i: j * len(prof) + i % len(prof)
    faces = []
    for j in range(len(ys) - 1):
        for i in range(len(prof)):
            q = (idx(j, i), idx(j, i + 1), idx(j + 1, i + 1), idx(j + 1, i))
            faces += [(q[0], q[3], q[2]), (q[0], q[2], q[1])]                               # wound like the fans: every normal points out of the prism
    mx, mz = np.mean(prof, axis=0)
    for j, y in ((0, ys[0]), (len(ys) - 1, ys[-1])):
        verts.append((mx, y, mz)); c = len(verts) - 1
        for i in range(len(prof)):
            faces.append((c, idx(j, i), idx(j, i + 1)) if j == 0 else (c, idx(j, i + 1), idx(j, i)))
    v = np.array(verts, np.float64); f = np.array(faces)
    # outward normals, the medium on the inside: every face sees the centroid behind it (the prism is convex)
    nrm = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    assert (np.einsum("ij,ij->i", nrm, v.mean(axis=0) - v[f[:, 0]]) < 0).all()
    with open(path, "w") as out:
        for p in v:
            out.write("v %.9g %.9g %.9g\n" % tuple(p))
        for t in f:
            out.write("f %d %d %d\n" % tuple(t + 1))
    return v.mean(axis=0), len(f)


def test_folded_box_lanes_match_the_oracle(mi, orc, monkeypatch, tmp_path):
    obj = str(tmp_path / "fold.obj")
    centre, n_faces = folded_box_obj(obj)
    centre = centre + np.array([-5.0, 5.0, -5.0])                                            # the scene file's to_world

    def edit(xml):
        out = xml.replace('value="liver2.obj"', 'value="%s"' % obj)
        eye = centre + np.array([6.0, -7.0, 5.0])
        out, n = re.subn(r"<lookat [^>]*/>", '<lookat up="0, 0, 1" target="%g, %g, %g" origin="%g, %g, %g"/>' % (*centre, *eye), out, flags=re.S)
        assert n == 1 and out != xml
        return out

    (a, sa, sc), (b, sb, _) = lanes_with_and_without(mi, monkeypatch, edit, res_width=64, res_height=64)
    assert sc.desc.n_faces == n_faces == 110 and sa["record_bytes"] == 64 and sb["record_bytes"] == 64 and sa["n_closed_guard"] == 0
    print("table", sa, "none", sb)
    assert sa["n_proven"] > sb["n_proven"], (sa, sb)                                          # the table is in use on this mesh
    assert (bits(a) == bits(b)).all()
    for k in COUNTS:
        assert sa[k] == sb[k], (k, sa, sb)
    assert_lanes_equal(sc, orc.OrcScene(sc), 0, 64 * 64 * 16, seed=3)
