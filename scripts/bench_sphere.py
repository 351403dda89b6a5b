"""Throughput of the fork's three sphere scenes (tests/golden/scenes/SphereLiver*/scene.xml at its own defaults: volpath, ldsampler, 4 spp,
1280x720, max_depth 65) on one GPU, the parenchyma spectra given as RGB values (tests/sphere_ref.py rgb_variant: the file itself does not
load; volpath does not read those values).  Best of `reps` renders per scene (lrt_render_stats.total_ms) as
Msamples/s, one JSON line.  python scripts/bench_sphere.py [reps]"""
import os, sys, json
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import liverrenderer_amd as mi
import sphere_ref as sr
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
out = {}
for name in sr.SPHERE_SCENES:
    d = os.path.join(sr.GOLDEN_SCENES, name)
    sc = mi.load_string(sr.rgb_variant(os.path.join(d, "scene.xml")), d)
    sc.render()                                   # warm-up: device image, workspace
    ms = []
    for _ in range(reps):
        sc.render()
        ms.append(sc.stats()["total_ms"])
    n = sc.stats()["n_samples"]
    out[name] = {"samples": int(n), "lds_resident": int(sc.stats()["lds_resident"]), "ms_best": round(min(ms), 3),
                 "Msamples_per_s": round(n / min(ms) / 1e3, 2)}
print(json.dumps({"bench": "sphere scenes at their scene.xml defaults", "scenes": out}))
