"""Density reconstruction from one image, the inverse counterpart of `bench.py --config het`: render a target from
scene_gen.smoke_grid() in scene_gen.het_xml, start from a uniform grid and run plain gradient descent on the mean squared image
difference with the per-voxel gradients of Scene.render_backward(grid=True).  A fresh seed per step (the primal image and its adjoint
use different seeds, so the gradient of the loss is unbiased); the grid is clamped to stay positive.  A demonstration, not a test.
python scripts/fit_density.py [steps] [spp] [learning rate]"""
import os, sys, tempfile
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import liverrenderer_amd as mi
import scene_gen
steps = int(sys.argv[1]) if len(sys.argv) > 1 else 40
spp = int(sys.argv[2]) if len(sys.argv) > 2 else 64
lr = float(sys.argv[3]) if len(sys.argv) > 3 else 80.0
W, H = 64, 48

truth = scene_gen.smoke_grid()
vol = os.path.join(tempfile.mkdtemp(prefix="fit_density_"), "smoke.vol"); mi.write_volume_grid(vol, truth)
sc = mi.load_string(scene_gen.resized(scene_gen.het_xml(vol, md=8), W, H, spp))
key = "smoke.sigma_t.data"
target = sc.render(integrator="prbvolpath", spp=1024, seed=10 ** 6).astype(np.float64)
noise = float(np.mean((sc.render(integrator="prbvolpath", spp=1024, seed=10 ** 6 + 1) - target) ** 2))
grid = np.full(truth.shape, float(truth.mean()), np.float32)
print(f"grid {truth.shape} (z, y, x), image {W} x {H}, {spp} spp per step, learning rate {lr}; loss of two renders of the truth at 1024 spp: {noise:.3e}")
for step in range(steps + 1):
    sc.param_set(key, grid)
    img = sc.render(integrator="prbvolpath", seed=2 * step).astype(np.float64)
    diff = img - target
    if step % 5 == 0 or step == steps:
        check = sc.render(integrator="prbvolpath", spp=1024, seed=10 ** 6 + 2).astype(np.float64)
        print(f"step {step:3d}  loss at {spp} spp {np.mean(diff ** 2):.4e}  loss at 1024 spp {np.mean((check - target) ** 2):.4e}  "
              f"grid rms error {np.sqrt(np.mean((grid - truth) ** 2)):.4f}", flush=True)
    if step == steps: break
    g = sc.render_backward((2.0 * diff / diff.size).astype(np.float32), medium=0, grid=True, seed=2 * step + 1)["sigma_t_data"]
    grid = np.clip(grid - lr * g, 1e-3, None).astype(np.float32)
