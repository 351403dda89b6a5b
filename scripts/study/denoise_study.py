"""Parameter study behind the guided denoiser's defaults.  Needs a GPU.

Inputs: mi.cornell_box() (path) and Liver-SingleMesh (volpath) under the aov integrator (albedo, sh_normal) at 8 and 64 spp;
metric: RMSE of the denoised image against a 1024-spp render (the definition bench.py uses for rmse_vs_oracle), as a ratio to the
noisy image's RMSE; score of a parameter set: the mean of the four ratios.  The defaults are the best-scoring set among those
that make none of the four inputs worse (every ratio below 1).  Prints the table and both sets as JSON."""
import itertools
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import liverrenderer_amd as mi

LIVER_XML = os.path.join(ROOT, "scenes", "Liver-SingleMesh", "mitsuba3", "scene.xml")
W, H = 256, 144
GRID = dict(sigma_color=(0.3, 1.0, 3.0, 10.0, 30.0), sigma_normal=(0.1, 0.25, 0.5), sigma_albedo=(0.05, 0.1, 0.3), eps_a=(1e-3, 0.05, 0.5))


def scenes():
    d = mi.cornell_box()
    d["integrator"] = {"type": "aov", "aovs": "albedo:albedo,nn:sh_normal", "image": d["integrator"]}
    d["sensor"]["film"]["width"], d["sensor"]["film"]["height"] = W, H
    yield "cornell", mi.load_dict(d)
    xml = open(LIVER_XML).read()
    xml, n = re.subn(r'<integrator type="\$integrator">(.*?)</integrator>',
                     r'<integrator type="aov"><string name="aovs" value="albedo:albedo,nn:sh_normal"/><integrator type="$integrator" name="image">\1</integrator></integrator>', xml, flags=re.S)
    assert n == 1
    yield "liver", mi.load_string(xml, os.path.dirname(LIVER_XML), integrator="volpath", res_width=W, res_height=H)


def rmse(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


def main():
    cases = []
    for name, sc in scenes():
        names = sc.aov_channel_names()
        ref = mi.Bitmap(mi.render(sc, spp=1024, seed=2), channel_names=names).select("image")[..., :3]
        for spp in (8, 64):
            b = mi.Bitmap(mi.render(sc, spp=spp, seed=1), channel_names=names)
            cases.append((f"{name}@{spp}", b.select("image"), b.select("albedo"), b.select("nn"), ref))
    rows = []
    for combo in itertools.product(*GRID.values()):
        prm = dict(zip(GRID.keys(), combo))
        dn = mi.Denoiser((W, H), albedo=True, normals=True, **prm)
        ratios = [rmse(dn(n, a, nr)[..., :3], ref) / rmse(n[..., :3], ref) for _, n, a, nr, ref in cases]
        rows.append((float(np.mean(ratios)), prm, ratios))
    rows.sort(key=lambda r: r[0])
    print("noisy RMSE:", {c[0]: round(rmse(c[1][..., :3], c[4]), 5) for c in cases})
    print("score  " + "  ".join(GRID.keys()) + "   " + "  ".join(c[0] for c in cases))
    for score, prm, ratios in rows[:12] + rows[-3:]:
        print(f"{score:.4f}  " + "  ".join(f"{v:g}" for v in prm.values()) + "   " + "  ".join(f"{r:.3f}" for r in ratios))
    safe = next((r for r in rows if max(r[2]) < 1.0), None)
    print(json.dumps({"study": "denoise_defaults", "size": [W, H], "chosen": None if safe is None else {"params": safe[1], "score": safe[0], "ratios": safe[2]}, "best": rows[0][1], "best_score": rows[0][0], "best_ratios": dict(zip([c[0] for c in cases], rows[0][2])),
                      "n_sets": len(rows)}))


if __name__ == "__main__":
    main()
