"""What the light source costs on one GPU: Liver-SingleMesh through volpath at 256 x 192, 64 spp (the c3hg workload of bench.py at a
small size) under the file's envmap (the plain instance, unchanged by this feature), under a point light at the camera, a spot at the
same place looking where the camera looks (an endoscope's light), the same spot projecting a checkerboard, and a directional light along
the view direction (the wide EXT instances).  Best of `reps` renders per scene (lrt_render_stats.total_ms) as
Msamples/s, one JSON line.  python scripts/bench_spot.py [reps] [case ...]   (cases: envmap point spot spot_checker directional; all when
none is named.  LRT_LIBRARY=<another libliverrt.so> runs a case through that build, e.g. `point` through the parent commit's.)"""
import os, re, sys, json
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import liverrenderer_amd as mi
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
BASE = os.path.join(ROOT, "scenes", "Liver-SingleMesh", "mitsuba3")
DEFINES = dict(integrator="volpath", spp=64, res_width=256, res_height=192)
ORIGIN, TARGET, UP = "7.481132, 5.343665, 6.507640", "6.826270, 5.011984, 5.896974", "-0.317370, 0.895343, -0.312469"      # the file's camera
VIEW = ", ".join(repr(float(t) - float(o)) for o, t in zip(ORIGIN.split(","), TARGET.split(",")))


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
ENV = re.compile(r'<emitter type="envmap">.*?</emitter>', re.S)
assert len(ENV.findall(xml)) == 1
pose = f'<transform name="to_world"><lookat origin="{ORIGIN}" target="{TARGET}" up="{UP}"/></transform>'
spot = '<emitter type="spot"><rgb name="intensity" value="40"/><float name="cutoff_angle" value="30"/><float name="beam_width" value="20"/>' + pose
cases = {"envmap": None,
         "point": f'<emitter type="point"><rgb name="intensity" value="40"/><point name="position" value="{ORIGIN}"/></emitter>',
         "spot": spot + '</emitter>',
         "spot_checker": spot + '<texture type="checkerboard" name="texture"><transform name="to_uv"><scale x="8" y="8"/></transform></texture></emitter>',
         "directional": f'<emitter type="directional"><rgb name="irradiance" value="3"/><vector name="direction" value="{VIEW}"/></emitter>'}
names = sys.argv[2:] or list(cases)
out = {k: best(mi.load_string(xml if cases[k] is None else ENV.sub(cases[k], xml), BASE, **DEFINES)) for k in names}
print(json.dumps({"bench": "Liver-SingleMesh volpath 256 x 192 x 64 spp, light source", "library": os.path.basename(os.path.dirname(os.path.abspath(mi._lib.LIB_PATH))),
                  "scenes": out}))
