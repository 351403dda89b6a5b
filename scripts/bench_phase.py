"""What a tabulated or blended phase function costs on one GPU: Liver-SingleMesh through volpath at 256 x 192, 64 spp (the c3hg
workload of bench.py at a small size) with the liver medium's phase function set to hg g = 0.7 (the plain instance: the 64-byte
closed-records kernel, unchanged by this feature), to the same lobe tabulated at n = 257 and n = 1801, and to
blendphase(0.3, rayleigh, hg 0.7) (the wide EXT instances).  Best of `reps` renders per scene
(lrt_render_stats.total_ms) as Msamples/s, one JSON line.  python scripts/bench_phase.py [reps]"""
import os, sys, json
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import liverrenderer_amd as mi
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
BASE = os.path.join(ROOT, "scenes", "Liver-SingleMesh", "mitsuba3")
DEFINES = dict(integrator="volpath", spp=64, res_width=256, res_height=192)
G = 0.7


def best(sc):
    sc.render()                                   # warm-up: device image, workspace
    ms = []
    for _ in range(reps):
        sc.render()
        ms.append(sc.stats()["total_ms"])
    st = sc.stats()
    return {"samples": int(st["n_samples"]), "lds_resident": int(st["lds_resident"]), "record_bytes": int(st.get("record_bytes", 0)), "ms_best": round(min(ms), 3),
            "Msamples_per_s": round(st["n_samples"] / min(ms) / 1e3, 2)}


def hg_table(n):                                  # physics convention: node value hg(g, -cos)
    c = np.linspace(-1.0, 1.0, n)
    t = 1 + G * G - 2 * G * c
    return ", ".join(repr(float(v)) for v in ((1 - G * G) / (4 * np.pi) / (t * np.sqrt(t))).astype(np.float32))


xml = open(os.path.join(BASE, "scene.xml")).read()
assert xml.count('<phase type="isotropic"/>') == 1
hg = f'<phase type="hg"><float name="g" value="{G}"/></phase>'
cases = {"hg": hg,
         "tabphase_257": f'<phase type="tabphase"><string name="values" value="{hg_table(257)}"/></phase>',
         "tabphase_1801": f'<phase type="tabphase"><string name="values" value="{hg_table(1801)}"/></phase>',
         "blend_0.3_rayleigh_hg": f'<phase type="blendphase"><float name="weight" value="0.3"/><phase type="rayleigh"/>{hg}</phase>'}
out = {k: best(mi.load_string(xml.replace('<phase type="isotropic"/>', v), BASE, **DEFINES)) for k, v in cases.items()}
print(json.dumps({"bench": "Liver-SingleMesh volpath 256 x 192 x 64 spp, phase function of the liver medium", "scenes": out}))
