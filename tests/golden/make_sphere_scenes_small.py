"""Generates tests/golden/reference_{sphereliverpoint,sphereliverconstenv}_{main,temp}_down8.npy from the reference's own float renders
that sit beside the fork's sphere scenes (/root/reference/scenes/SphereLiver{Point,ConstEnv}/mitsuba3/{sphereliverpoint,
sphereliverconstenv}.exr -> "main", scene_temp.exr -> "temp"; 960x540 half-float PIZ): linear RGB, cropped to the first 536 rows
(540 is not a multiple of 8), box-averaged over 8x8 blocks (67x120x3 float16).  Data only.

Which file and spp produced each render is not recorded, and neither scene file loads in the reference as it stands
(tests/test_sphere_scenes.py).  The renders are 960x540, the size scene_temp.xml asks for (scene.xml asks for 1280x720)."""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import liverrenderer_amd as mi
for name, main in (("SphereLiverPoint", "sphereliverpoint.exr"), ("SphereLiverConstEnv", "sphereliverconstenv.exr")):
    for tag, fn in (("main", main), ("temp", "scene_temp.exr")):
        q = mi.read_image(f"/root/reference/scenes/{name}/mitsuba3/{fn}")[..., :3].astype(np.float64)
        assert q.shape == (540, 960, 3), q.shape
        small = q[:536].reshape(67, 8, 120, 8, 3).mean((1, 3))
        out = os.path.join(ROOT, "tests", "golden", f"reference_{name.lower()}_{tag}_down8.npy")
        np.save(out, small.astype(np.float16))
        print(out, small.shape, small.mean((0, 1)))
