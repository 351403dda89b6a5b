"""What a rough capsule costs on one GPU: Liver-SingleMesh through volpath at 256 x 192, 64 spp, as the scene stands (its capsule is a
bumpmap over a smooth `dielectric`: the 64-byte closed-records kernel) and with that dielectric replaced by a `roughdielectric` of
alpha 0.1, ggx and beckmann (a smooth lobe at the boundary: the wide EXT instances).  Best of `reps` renders per
scene (lrt_render_stats.total_ms) as Msamples/s, one JSON line.  python scripts/bench_rough.py [reps]"""
import os, sys, json, re
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import liverrenderer_amd as mi
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
BASE = os.path.join(ROOT, "scenes", "Liver-SingleMesh", "mitsuba3")
DEFINES = dict(integrator="volpath", spp=64, res_width=256, res_height=192)


def best(sc):
    sc.render()                                   # warm-up: device image, workspace
    ms = []
    for _ in range(reps):
        sc.render()
        ms.append(sc.stats()["total_ms"])
    st = sc.stats()
    return {"samples": int(st["n_samples"]), "lds_resident": int(st["lds_resident"]), "record_bytes": int(st.get("record_bytes", 0)), "ms_best": round(min(ms), 3),
            "Msamples_per_s": round(st["n_samples"] / min(ms) / 1e3, 2)}


xml = open(os.path.join(BASE, "scene.xml")).read()
smooth = r'(<bsdf type="bumpmap" id="GlissonCapsuleBSDF">.*?)<bsdf type="dielectric">(.*?)</bsdf>'
out = {"as_it_stands": best(mi.load_string(xml, BASE, **DEFINES))}
for distribution in ("ggx", "beckmann"):
    rough, n = re.subn(smooth, r'\1<bsdf type="roughdielectric"><float name="alpha" value="0.1"/><string name="distribution" value="%s"/>\2</bsdf>' % distribution, xml, flags=re.S)
    assert n == 1
    out["capsule_roughdielectric_" + distribution] = best(mi.load_string(rough, BASE, **DEFINES))
print(json.dumps({"bench": "Liver-SingleMesh volpath 256 x 192 x 64 spp, smooth against rough capsule", "scenes": out}))
