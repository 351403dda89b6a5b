"""Cost of the per-voxel sigma_t gradient on one GPU: scene_gen.het_xml at 256 x 192 x 64 spp with the 12 x 10 x 8 smoke grid and with a
64^3 grid of the same recipe.  Best of `reps` calls (lrt_render_stats.total_ms: primal + adjoint pass) of lrt_render_backward and of
lrt_render_backward_grid on this build; with --parent-root DIR also lrt_render_backward of a built checkout of the parent commit (its own
package and library: nothing on that path changed, so the two agree within run-to-run noise).  With --count-lib PATH (a build made with
`make -C liverrenderer_amd/csrc count`, whose grid_scatter adds 1.0 per add instead of the value) the number of scatter adds and the
most loaded voxel are exact; without it the adds are bounded from n_iter / n_shadow: at most 8 per loop trip and 8 per replayed march
query.  One JSON line.   python scripts/bench_grid_grad.py [reps] [--parent-root DIR] [--count-lib PATH]
Every library runs in a child process of its own (LRT_LIBRARY is read when the package loads the library)."""
import json, os, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, SPP = 256, 192, 64
GRIDS = {"smoke_12x10x8": (12, 10, 8), "smoke_64x64x64": (64, 64, 64)}
# MI355X float atomic add rates (bytes of f32 adds per second): well-shaped, 64 lanes in 64 rows, everything in one row (1 / 14 of that)
RATES_TBS = {"well_shaped": 1.3, "64_lanes_64_rows": 0.08, "one_row": 0.08 / 14}


def worker(mode, reps):
    sys.path[:0] = [os.environ.get("BENCH_GRID_PACKAGE_ROOT", ROOT), os.path.join(ROOT, "tests")]
    import numpy as np
    import liverrenderer_amd as mi
    import scene_gen
    tmp = tempfile.mkdtemp(prefix="bench_grid_grad_")
    has_grid = hasattr(mi._lib.lib(), "lrt_render_backward_grid")
    out = {}
    for name, shape in GRIDS.items():
        vol = os.path.join(tmp, name + ".vol"); mi.write_volume_grid(vol, scene_gen.smoke_grid(shape=shape))
        sc = mi.load_string(scene_gen.resized(scene_gen.het_xml(vol), W, H, SPP))
        h, w, c = sc.film_shape()
        grad = np.full((h, w, c), 1.0 / (h * w * c), np.float32)
        r = {}
        if mode == "count":
            d = sc.render_backward(grad, medium=0, grid=True)["sigma_t_data"].astype(np.float64)
            r = {"adds": int(d.sum()), "adds_max_voxel": int(d.max()), "adds_median_voxel": float(np.median(d)), "voxels_touched": int((d > 0).sum())}
        else:
            for key, kw in (("backward", {}),) + ((("backward_grid", {"grid": True}),) if has_grid and mode == "this" else ()):
                sc.render_backward(grad, medium=0, **kw)                          # warm-up: device image, workspace
                ms = []
                for _ in range(reps):
                    sc.render_backward(grad, medium=0, **kw); ms.append(sc.stats()["total_ms"])
                st = sc.stats()
                r[key] = {"ms_best": round(min(ms), 3), "ms_all": [round(x, 3) for x in ms], "kernel_ms": round(st["kernel_ms"], 3),
                          "n_iter": int(st["n_iter"]), "n_shadow": int(st["n_shadow"]), "samples": int(st["n_samples"])}
        out[name] = r
    print("RESULT " + json.dumps(out), flush=True)


def child(mode, reps, lib=None, root=None):
    env = dict(os.environ)
    if lib: env["LRT_LIBRARY"] = os.path.abspath(lib)
    if root: env["BENCH_GRID_PACKAGE_ROOT"] = os.path.abspath(root)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", mode, str(reps)], env=env, capture_output=True, text=True)
    line = next((l for l in p.stdout.splitlines() if l.startswith("RESULT ")), None)
    if p.returncode != 0 or line is None:
        raise SystemExit(f"worker {mode} failed ({p.returncode}):\n{p.stdout}\n{p.stderr}")
    return json.loads(line[7:])


if __name__ == "__main__":
    a = sys.argv[1:]
    if a and a[0] == "--worker":
        worker(a[1], int(a[2])); sys.exit(0)
    opt = {}
    for k in ("--parent-root", "--count-lib"):
        if k in a:
            i = a.index(k); opt[k] = a[i + 1]; del a[i:i + 2]
    reps = int(a[0]) if a else 5
    this = child("this", reps)
    parent = child("parent", reps, root=opt["--parent-root"]) if "--parent-root" in opt else None
    count = child("count", 1, opt["--count-lib"]) if "--count-lib" in opt else None
    res = {}
    for name in GRIDS:
        b, g = this[name]["backward"], this[name]["backward_grid"]
        r = {"voxels": GRIDS[name][0] * GRIDS[name][1] * GRIDS[name][2], "backward": b, "backward_grid": g, "grid_over_backward": round(g["ms_best"] / b["ms_best"], 3)}
        if parent: r["parent_backward"] = parent[name]["backward"]; r["backward_over_parent"] = round(b["ms_best"] / parent[name]["backward"]["ms_best"], 3)
        if count: r.update(count[name]); adds, exact = count[name]["adds"], True
        else: adds, exact = 8 * (b["n_iter"] // 2 + (g["n_shadow"] - b["n_shadow"])), False      # n_iter counts the primal and the adjoint pass
        r["adds"], r["adds_exact"] = adds, exact
        r["add_GB_per_s_over_whole_call"] = round(adds * 4 / (g["ms_best"] * 1e-3) / 1e9, 3)
        extra = max(g["ms_best"] - b["ms_best"], 1e-6)
        r["add_GB_per_s_over_added_time"] = round(adds * 4 / (extra * 1e-3) / 1e9, 3)
        res[name] = r
    print(json.dumps({"bench": f"per-voxel sigma_t gradient (het_xml, {W} x {H} x {SPP} spp, best of {reps})", "guide_rates_TB_per_s": RATES_TBS, "grids": res}))
