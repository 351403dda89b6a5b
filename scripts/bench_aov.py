"""Cost of the aov integrator's first-hit pass (kernels_aov.h, k_aov) alone on C3's scene and size: Liver-SingleMesh, 1920x1080,
512 spp, aovs="albedo:albedo,nn:sh_normal,dd:depth", no nested integrator (their images are ordinary renders, bench.py measures
those).  Prints the AOV kernel time of the best of `reps` renders (HIP events: lrt_render_stats.kernel_ms) and Mrays/s, one JSON line.
rfilter: the scene's box filter (default), or gaussian / tent for the wide-filter branch of k_aov (film.h, film_walk); spp: default 512.
python scripts/bench_aov.py [reps] [rfilter] [spp]"""
import os, sys, re, json
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import liverrenderer_amd as mi
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
rfilter = sys.argv[2] if len(sys.argv) > 2 else "box"
xml_path = os.path.join(ROOT, "scenes", "Liver-SingleMesh", "mitsuba3", "scene.xml")
xml, n = re.subn(r'<integrator type="\$integrator">.*?</integrator>',
                 '<integrator type="aov"><string name="aovs" value="albedo:albedo,nn:sh_normal,dd:depth"/></integrator>', open(xml_path).read(), flags=re.S)
assert n == 1 and xml.count('<rfilter type="box"/>') == 1
xml = xml.replace('<rfilter type="box"/>', f'<rfilter type="{rfilter}"/>')
W, H, SPP = 1920, 1080, int(sys.argv[3]) if len(sys.argv) > 3 else 512
sc = mi.load_string(xml, os.path.dirname(xml_path), spp=SPP, res_width=W, res_height=H)
sc.render(spp=8)                                  # warm-up: device image, workspace
ms = []
for _ in range(reps):
    img = sc.render()
    ms.append(sc.stats()["kernel_ms"])
best = min(ms)
rays = W * H * SPP
print(json.dumps({"scene": "C3 Liver-SingleMesh aov pass (albedo, sh_normal, depth)", "rfilter": rfilter, "width": W, "height": H, "spp": SPP,
                  "lds_resident": int(sc.stats()["lds_resident"]), "aov_pass_ms_best": round(best, 3),
                  "aov_pass_ms_all": [round(x, 3) for x in ms], "Mrays_per_s": round(rays / best / 1e3, 1)}))
