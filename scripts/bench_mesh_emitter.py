"""Throughput of area emitters on triangle meshes on one GPU: mi.cornell_box() (path, max_depth 8, 256 x 256, 64 spp) with its light
as the `rectangle` and as the same quad written as a 2-triangle `obj` (same world vertices and faces), and the Cornell box lit by an
emissive sphere-like mesh of several thousand triangles (an icosphere in place of the light) through path and volpath.  Best of
`reps` renders per scene (lrt_render_stats.total_ms) as Msamples/s, one JSON line.  python scripts/bench_mesh_emitter.py [reps]"""
import os, sys, json, tempfile
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import liverrenderer_amd as mi
import mesh_emitter_ref as mr
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
tmp = tempfile.mkdtemp(prefix="bench_mesh_emitter_")


def icosphere(level, center, radius):
    """An icosahedron subdivided `level` times, projected to the sphere: 20 * 4^level outward-facing triangles"""
    t = (1 + 5 ** 0.5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    v = [np.array(p, float) / np.linalg.norm(p) for p in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(level):
        mid = {}
        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                p = v[a] + v[b]; v.append(p / np.linalg.norm(p)); mid[k] = len(v) - 1
            return mid[k]
        f = [g for (a, b, c) in f for g in ((a, m(a, b), m(c, a)), (b, m(b, c), m(a, b)), (c, m(c, a), m(b, c)), (m(a, b), m(b, c), m(c, a)))]
    return np.array(v) * radius + np.asarray(center), np.array(f)


def best(sc, **kw):
    sc.render(**kw)                               # warm-up: device image, workspace
    ms = []
    for _ in range(reps):
        sc.render(**kw)
        ms.append(sc.stats()["total_ms"])
    n = sc.stats()["n_samples"]
    return {"samples": int(n), "lds_resident": int(sc.stats()["lds_resident"]), "ms_best": round(min(ms), 3), "Msamples_per_s": round(n / min(ms) / 1e3, 2)}


out = {}
d = mi.cornell_box()
rect = mi.load_dict(d)
out["cornell_rectangle"] = best(rect)
pos, nrm, faces, shapes, emitters = mr.scene_arrays(rect)
s = shapes[emitters[0].shape]
fq = faces[s.first_face:s.first_face + s.n_faces]
used = np.unique(fq); remap = {int(x): i for i, x in enumerate(used)}
quad = mr.write_obj(os.path.join(tmp, "light.obj"), pos[used], [[remap[int(x)] for x in t] for t in fq])
d2 = mi.cornell_box(); d2["light"] = dict(d2["light"], type="obj", filename=quad); del d2["light"]["to_world"]
out["cornell_obj_2_triangles"] = best(mi.load_dict(d2))
v, f = icosphere(4, (0.0, 0.75, 0.0), 0.15)
ball = mr.write_obj(os.path.join(tmp, "ball.obj"), v, f)
d3 = mi.cornell_box(); d3["light"] = {"type": "obj", "filename": ball, "emitter": {"type": "area", "radiance": {"type": "rgb", "value": [6.0, 5.0, 3.0]}}}
mesh = mi.load_dict(d3)
out[f"cornell_mesh_light_{len(f)}_triangles_path"] = best(mesh)
out[f"cornell_mesh_light_{len(f)}_triangles_volpath"] = best(mesh, integrator="volpath")
print(json.dumps({"bench": "area emitters on meshes (mi.cornell_box at its defaults)", "scenes": out}))
