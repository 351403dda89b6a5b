#!/usr/bin/env python3
"""Benchmark of the hip_ad_rgb hot path on BASELINE.json's metric: Msamples/s at fixed spp.

A "step" is one complete render of the workload (ray generation -> persistent sample loop -> film -> develop, plus the RCCL
film all-reduce when N > 1).  Default workload (`--config c3`): BASELINE config C3 = scenes/Liver-SingleMesh, plain
`volpath`, 1920x1080, 512 spp, max_depth 12.  Other single-GPU workloads of BASELINE.json, each with its own roofline:

  --config c3hg         C3 with the medium's phase function set to Henyey-Greenstein, g = 0.7 (BASELINE.json config 3 names "HG phase")
  --config c3bio        the same scene file with its OWN defaults' integrator and medium (`biovolpath` + `liver`), the
                        transport every published timing of the reference is quoted on
  --config c2           mi.cornell_box() at 1080x1080, `path`, 256 spp (Gaussian filter)
  --config c5           PRB adjoint d(mean image)/d(sigma_t, albedo, g) on the Parenchyma scene, 1920x1080, 256 spp
                        (a step = primal + adjoint pass; medium read as homogeneous)
  --config parenchyma   scenes/Parenchyma/mitsuba3/scene_temp.xml with its own defaults (`biovolpath06`, ld sampler, tent)
  --config multimesh    scenes/Liver-MultiMesh/mitsuba3/scene_temp.xml with its own defaults (`biovolpath`, both meshes, both tissue
                        media, envmap, 256 spp): the scene of BASELINE.md's published 44.6 s / 11.89 Msamples/s; `vs_baseline` is set
  --config c4           scenes/Liver-MultiMesh/mitsuba3/scene.xml as committed (BASELINE config C4's geometry), 1024 spp
  --config het          SURVEY.md 8f row 4: `volpath` through a grid-volume medium (delta tracking, null collisions) in a box, 1080x1080, 64 spp
  --config mis          the same scene plus a homogeneous medium under `volpathmis` (spectral MIS), 1080x1080, 64 spp

For N > 1 the SAME image is sharded by 32x32 pixel tiles over the ranks (strong scaling) and the per-rank raw films are
summed with one all-reduce before develop.  Prints ONE JSON line on rank 0 (contract: see the task statement).

A plain run sets up, warms up, times the steps, writes `--dump-outputs` if asked and prints the line: `value`, `ms_per_step` and the
`roofline` of the timed launches.  `--full` adds what takes runs of its own (single GPU, forward integrators): `host_visible` (the same
renders into host memory), `hg_phase` (C3 only: the c3hg workload timed beside it), `cpu_baseline` (the oracle's scalar renderer built
for the host CPU) and `rmse_vs_oracle`.  `--main-only` and `--no-cpu-baseline` drop legs of a `--full` run.

`--dump-outputs DIR` writes what the last timed step computed (image + raw film, or the PRB gradients) as DIR/<name>.npy once the
clock has stopped.  Step k renders with seed k, so the same arguments give the same inputs on every run: two builds can be compared
output for output (to float-atomic order in the film, see rmse_vs_oracle).
"""
import argparse
import json
import glob, os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np

HBM_PEAK_GBS = 8000.0          # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
SCENES = os.path.join(ROOT, "scenes")

# bytes of one path record across the SoA streams (csrc/device_types.h); PRB carries one more float4 stream (delta_L)
RECORD_BYTES = {"path": 88, "volpath": 88, "biovolpath": 96, "biovolpath06": 96, "prbvolpath": 104, "volpathmis": 168, "volpath_het": 104}
KERNEL_ID = {"path": 0, "volpath": 1, "biovolpath": 3, "biovolpath06": 4, "volpathmis": 5, "volpathmis_plain": 102, "volpath_het": 101}
CONFIGS = {
    "c3": dict(scene=os.path.join(SCENES, "Liver-SingleMesh", "mitsuba3", "scene.xml"), integrator="volpath", spp=512, width=1920, height=1080,
               label="C3 Liver-SingleMesh {integrator} {w}x{h} {spp} spp max_depth 12 (homogeneous medium, isotropic phase, envmap)"),
    # BASELINE.json config 3 names "homogeneous medium + HG phase": the same workload with the medium's phase function set to HG, g = 0.7,
    # through the reference's own parameter interface (mi.traverse; BASELINE.md C3 "HG g=0.7 as a second run")
    "c3hg": dict(scene=os.path.join(SCENES, "Liver-SingleMesh", "mitsuba3", "scene.xml"), integrator="volpath", spp=512, width=1920, height=1080,
                 params={"LiverMedium.phase_function.g": 0.7},
                 label="C3 Liver-SingleMesh {integrator} {w}x{h} {spp} spp max_depth 12 (homogeneous medium, HG phase g = 0.7, envmap)"),
    "c3bio": dict(scene=os.path.join(SCENES, "Liver-SingleMesh", "mitsuba3", "scene.xml"), integrator=None, spp=512, width=1920, height=1080,
                  label="C3-bio Liver-SingleMesh {integrator} (file defaults: liver medium) {w}x{h} {spp} spp max_depth 12"),
    "c2": dict(scene="cornell_box", integrator="path", spp=256, width=1080, height=1080,
               label="C2 cornell_box {integrator} {w}x{h} {spp} spp max_depth 8 (Gaussian filter)"),
    "c5": dict(scene=os.path.join(SCENES, "Parenchyma", "mitsuba3", "scene_temp.xml"), integrator="prbvolpath", spp=256, width=1920, height=1080,
               label="C5 Parenchyma {integrator} backward (primal + adjoint) {w}x{h} {spp} spp, ld sampler, tent filter"),
    "c4": dict(scene=os.path.join(SCENES, "Liver-MultiMesh", "mitsuba3", "scene.xml"), integrator=None, spp=1024, width=1920, height=1080,
               label="C4 Liver-MultiMesh {integrator} as committed (black diffuse liver1.obj under a constant emitter; ld sampler, box filter) {w}x{h} {spp} spp"),
    # the scene behind BASELINE.md's "Liver-MultiMesh, 256 spp, latest run: 44.638 s = 11.89 Msamples/s" (time.txt next to the file)
    "multimesh": dict(scene=os.path.join(SCENES, "Liver-MultiMesh", "mitsuba3", "scene_temp.xml"), integrator=None, spp=256, width=1920, height=1080,
                      published_msamples=11.89,
                      label="Liver-MultiMesh scene_temp.xml {integrator} (file defaults: capsule shell + parenchyma mesh, glissonCapsule + parenchyma media, envmap, ld sampler, tent) {w}x{h} {spp} spp max_depth 12"),
    "parenchyma": dict(scene=os.path.join(SCENES, "Parenchyma", "mitsuba3", "scene_temp.xml"), integrator=None, spp=256, width=1920, height=1080,
                       label="Parenchyma {integrator} (file defaults: parenchyma medium, ld sampler, tent) {w}x{h} {spp} spp max_depth 12"),
    # SURVEY.md 8f row 4 (parity unpinned by the reference beyond analytic answers): the scenes of tests/test_round2_gpu.py at bench size
    "het": dict(scene="generated:het", integrator=None, spp=64, width=1080, height=1080,
                label="f4 heterogeneous (grid-volume) medium in a null-boundary box, {integrator} with delta tracking, area light + constant environment {w}x{h} {spp} spp max_depth 12"),
    "mis": dict(scene="generated:mis", integrator=None, spp=64, width=1080, height=1080,
                label="f4 {integrator} (spectral MIS) through a grid-volume medium and a homogeneous medium {w}x{h} {spp} spp max_depth 12"),
}


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=3)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--config", default="c3", choices=sorted(CONFIGS))
    p.add_argument("--spp", type=int, default=0, help="override the config's samples per pixel")
    p.add_argument("--width", type=int, default=0)
    p.add_argument("--height", type=int, default=0)
    p.add_argument("--scene", default=None, help="override the config's scene file")
    p.add_argument("--integrator", default=None, help="override the config's integrator")
    p.add_argument("--full", action="store_true", help="after the headline figure, also run the host_visible / hg_phase / cpu_baseline (+ rmse_vs_oracle) legs")
    p.add_argument("--no-cpu-baseline", action="store_true", help="with --full: no cpu_baseline / rmse_vs_oracle leg")
    p.add_argument("--main-only", action="store_true", help="only the timed steps of the named configuration, even with --full: no host_visible / hg_phase / cpu_baseline legs (profiling: every dispatch of the render kernel then belongs to the workload)")
    p.add_argument("--backend", default="nccl", help="process-group backend; gloo allows a multi-rank rehearsal on a single GPU")
    p.add_argument("--cpu-spp", type=int, default=0, help="with --full: spp of the bounded CPU-baseline sample (0: calibrate to ~15 s)")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="after the timed steps, write what the last timed step computed as DIR/<name>.npy (float32, at most 64 MB in all)")
    a = p.parse_args()
    if a.steps < 1:
        p.error("--steps must be at least 1")
    a.extra_legs = a.full and not a.main_only
    return a


DUMP_BYTES = 64 * 1000 * 1000
DUMP_SEED = 20240229


def dump_outputs(path, outputs, h, w):
    """Writes `outputs` ({name: array}) as path/<name>.npy in float32 (float64 stays float64).  Arrays shaped (h, w, ...) are
    per-pixel; when everything together exceeds DUMP_BYTES, each of them is cut to the same fixed, seeded sample of pixels
    (flat indices y * w + x, ascending, in path/pixel_index.npy as float64), so that runs with the same arguments write the same
    elements."""
    os.makedirs(path, exist_ok=True)
    arrs = {}
    for name, v in outputs.items():
        a = np.asarray(v)
        arrs[name] = np.array(a, dtype=np.float64 if a.dtype == np.float64 else np.float32, order="C")
    pixel = [k for k, a in arrs.items() if a.shape[:2] == (h, w)]
    total = sum(a.nbytes for a in arrs.values())
    if total > DUMP_BYTES and pixel:
        per_pixel = sum(arrs[k].nbytes for k in pixel) // (h * w) + 8          # + the float64 index
        rest = total - sum(arrs[k].nbytes for k in pixel) + 128 * (len(arrs) + 1)      # + the .npy headers
        n = max(1, min(h * w, (DUMP_BYTES - rest) // per_pixel))
        idx = np.sort(np.random.default_rng(DUMP_SEED).choice(h * w, size=n, replace=False))
        for k in pixel:
            arrs[k] = np.ascontiguousarray(arrs[k].reshape((h * w,) + arrs[k].shape[2:])[idx])
        arrs["pixel_index"] = idx.astype(np.float64)
    for name, a in arrs.items():
        np.save(os.path.join(path, name + ".npy"), a)
    return {k: a.shape for k, a in arrs.items()}


def kernel_source_id():
    """sha1 over the kernel sources the loaded library was built from (csrc/*.h, *.hip, *.cpp + include/liverrt.h).  profiles/*traffic.json
    records it; `roofline.traffic` is taken from a traffic file only when the ids agree, else it is null."""
    import hashlib
    h = hashlib.sha1()
    src = os.path.join(ROOT, "liverrenderer_amd", "csrc")
    for f in sorted(os.listdir(src)):
        if f.endswith((".h", ".hip", ".cpp")): h.update(f.encode()); h.update(open(os.path.join(src, f), "rb").read())
    h.update(open(os.path.join(ROOT, "include", "liverrt.h"), "rb").read())
    return h.hexdigest()[:16]


def usable_cores():
    """Host cores this process may actually use: the affinity mask, capped by the cgroup CPU quota (the GPU boxes expose
    all cores of the host but grant a share of them)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            txt = open(path).read().split()
            if path.endswith("cpu.max"):
                if txt[0] != "max": n = min(n, max(1, int(float(txt[0]) / float(txt[1]) + 0.5)))
            else:
                q = int(txt[0]); per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
                if q > 0: n = min(n, max(1, int(q / per + 0.5)))
            break
        except Exception:
            continue
    return max(1, n)


_TMP = []


def load(mi, cfg, spp, w, h, integrator):
    if cfg["scene"].startswith("generated:"):
        import tempfile
        import scene_gen
        tmp = tempfile.mkdtemp(prefix="lrt_bench_"); _TMP.append(tmp)
        vol = os.path.join(tmp, "smoke.vol"); mi.write_volume_grid(vol, scene_gen.smoke_grid())
        xml = scene_gen.het_xml(vol) if cfg["scene"] == "generated:het" else scene_gen.two_media_xml(vol).replace(
            '<integrator type="volpath">', '<integrator type="volpathmis"><boolean name="use_spectral_mis" value="true"/>')
        if integrator: xml = xml.replace('<integrator type="volpath">', f'<integrator type="{integrator}">')
        return mi.load_string(scene_gen.resized(xml, w, h, spp))
    if cfg["scene"] == "cornell_box":
        d = mi.cornell_box()
        d["sensor"]["film"]["width"], d["sensor"]["film"]["height"] = w, h
        d["sensor"]["sampler"]["sample_count"] = spp
        if integrator: d["integrator"]["type"] = integrator
        return mi.load_dict(d)
    kw = dict(spp=spp, res_width=w, res_height=h)
    if integrator: kw["integrator"] = integrator
    scene = mi.load_file(cfg["scene"], **kw)
    if cfg.get("params"):
        p = mi.traverse(scene)
        for k, v in cfg["params"].items(): p[k] = v
        p.update()
    return scene


def main():
    a = parse()
    cfg = dict(CONFIGS[a.config])
    if a.scene: cfg["scene"] = a.scene
    spp, w, h = a.spp or cfg["spp"], a.width or cfg["width"], a.height or cfg["height"]
    integrator_override = a.integrator or cfg["integrator"]
    import torch
    import liverrenderer_amd as mi
    from liverrenderer_amd import _lib
    from liverrenderer_amd.distributed import render_distributed, reduce_gradients

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != a.gpus:
        if world == 1 and a.gpus > 1:
            raise SystemExit("launch with: python -m torch.distributed.run --nnodes=1 --nproc-per-node N bench.py --gpus N ...")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (the hip_ad_rgb back-end has no CPU fallback)")
    local_rank %= max(torch.cuda.device_count(), 1)            # several ranks share a GPU only in a gloo rehearsal
    torch.cuda.set_device(local_rank)
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if a.backend == "nccl": dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        else: dist.init_process_group(a.backend)

    scene = load(mi, cfg, spp, w, h, integrator_override)
    integrator = {v: k for k, v in _lib.INTEGRATOR.items()}[scene.desc.integrator.type]
    spp = scene.spp                                             # the ld sampler rounds up to 4, 16, 64, 256, ...
    h, w, _ = scene.film_shape()
    C = scene.raw_channels()
    n_samples = w * h * spp
    backward = integrator == "prbvolpath"
    grad = (np.ones((h, w, C - 1), np.float32) / (h * w * (C - 1))) if backward else None      # loss = mean(image)

    def step(seed):
        """One timed step; returns what its caller receives: the developed image and the raw film (forward), the
        parameter gradients (PRB)."""
        if backward:                                            # common.py:625-783: primal pass + adjoint replay
            g = scene.render_backward(grad, spp=spp, seed=seed, tile_rank=rank, tile_count=world, device=local_rank)
            g = reduce_gradients(g) if world > 1 else g
            return {"grad_" + k: v for k, v in g.items()}
        if world > 1:
            img, raw = render_distributed(scene, spp=spp, seed=seed)
            return {"image": img, "film": raw}
        dev = torch.device("cuda", local_rank)
        film = torch.zeros((h, w, C), dtype=torch.float32, device=dev)
        image = torch.empty((h, w, C - 1), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        scene.render_to_device(film.data_ptr(), image.data_ptr(), spp=spp, seed=seed, device=local_rank)
        return {"image": image, "film": film}

    def fence():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
            torch.cuda.synchronize()

    for i in range(a.warmup):
        step(1000 + i)
    fence()
    t0 = time.perf_counter()
    kern_ms = iters = shadows = launches = records = 0.0
    for i in range(a.steps):
        last = step(i)
        st = scene.stats()
        kern_ms += st["kernel_ms"]; iters += st["n_iter"]; shadows += st["n_shadow"]; launches += st["n_launches"]; records += st["n_records"]
        if i + 1 < a.steps:
            last = None                                         # only the last step's outputs outlive their step (--dump-outputs)
    fence()
    dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    value = n_samples * a.steps / dt / 1e6
    dumped = None
    if a.dump_outputs and rank == 0:
        host = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in last.items()}
        dumped = dump_outputs(a.dump_outputs, host, h, w)
    last = None

    # ---- roofline of the dominant kernel (k_render / k_render_prb: persistent, ONE launch per pass), this rank's launches.
    # Algorithmic bytes: every queued path record is written once and read once (RECORD_BYTES each way; fresh camera paths
    # run their first trip in registers and trips the look-ahead retires early move no record), plus what the launch
    # leaves for the film: 4*C bytes per pixel (box filter: in-kernel splat) or 16 B per lane (wide filters and PRB: per-lane
    # radiance for the splat pass / the adjoint replay, which reads it back).  Duration: HIP events around the launches on the
    # library's stream (kernel_ms).  BASELINE.md "Roofline accounting" states the same model.
    n_rank = st["n_samples"]
    has_het = any(scene.desc.media[i].type == _lib.MEDIUM["heterogeneous"] for i in range(scene.desc.n_media))
    kkey = integrator
    if integrator == "volpath" and has_het: kkey = "volpath_het"                       # 104-B records: the kept surface hit rides along
    if integrator == "volpathmis" and not scene.desc.use_spectral_mis: kkey = "volpathmis_plain"
    rec_b = RECORD_BYTES["volpathmis" if integrator == "volpathmis" else kkey]
    lds = bool(st.get("lds_resident", 1))                      # False: the mesh did not fit the LDS image, BVH in global memory, 256-thread workgroups
    # compact records (kernels.h, store_state): a scene without area emitters does not queue the last scatter position: 8 bytes less per record
    compact = (lds and not backward and kkey in ("path", "volpath", "biovolpath", "biovolpath06") and not os.environ.get("LRT_WIDE_RECORDS")
               and not any(scene.desc.emitters[i].type == _lib.EMITTER["area"] for i in range(scene.desc.n_emitters)))
    if compact: rec_b -= 8
    box = scene.desc.film.rfilter == 0
    if backward: out_bytes = 2.0 * 16.0 * n_rank * a.steps
    elif box: out_bytes = 4.0 * C * w * h * a.steps / max(world, 1)
    else: out_bytes = 16.0 * n_rank * a.steps
    alg_bytes = 2.0 * rec_b * records + out_bytes
    achieved = alg_bytes / (kern_ms * 1e-3) / 1e9 if kern_ms > 0 else 0.0
    workload = cfg["label"].format(integrator=integrator, w=w, h=h, spp=spp)
    # HBM traffic per launch from the PMC passes of the same workload (scripts/profile_bench.sh -> profiles/*traffic.json)
    # (a counter pass cannot run inside this process: rocprofv3 wraps the program; the file must come from THIS build of the kernels)
    traffic = None; traffic_file = None; ksid = kernel_source_id()
    for tf in sorted(glob.glob(os.path.join(ROOT, "profiles", "*traffic*.json"))):
        try:
            tj = json.load(open(tf))
            if tj.get("workload") == workload and world == 1 and tj.get("kernel_source_id") == ksid:
                traffic = tj["traffic_bytes_per_launch"]; traffic_file = os.path.basename(tf)
        except Exception:
            pass
    ld = scene.desc.sampler_type == 1
    geom = ("768, true" if kkey in ("volpath_het", "volpathmis", "volpathmis_plain") else "1024, true") if lds else "256, false"
    kname = ("lrt::k_render_prb<*, %s, %s>" % (geom, str(ld).lower())) if backward else ("lrt::k_render<%d, %s, %s%s>" % (KERNEL_ID[kkey], geom, str(ld).lower(), ", true" if compact else ""))
    roofline = {"bound": "hbm", "achieved": round(achieved, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": round(achieved / HBM_PEAK_GBS, 5), "traffic": traffic, "traffic_source": traffic_file, "kernel_source_id": ksid, "kernel": kname,
                "launches_per_step": launches / a.steps, "avg_launch_ms": kern_ms / max(launches, 1),
                "alg_bytes_per_launch": alg_bytes / max(launches, 1), "record_bytes": rec_b,
                "iterations_per_sample": iters / (n_rank * a.steps), "records_per_sample": records / (n_rank * a.steps),
                "shadow_queries_per_sample": shadows / (n_rank * a.steps)}

    data = ("mi.cornell_box() dictionary" if cfg["scene"] == "cornell_box" else "synthetic: generated scene (tests/scene_gen.py), random density grid" if cfg["scene"].startswith("generated:")
            else "reference scene files (scene xml, liver2.obj, tissue_n.png, cavidade_latitude.exr)")
    out = {"metric": "Msamples/s", "value": round(value, 3), "unit": "Msamples/s", "n_gpus": world, "steps": a.steps,
           "warmup": a.warmup, "ms_per_step": round(dt / a.steps * 1e3, 3), "higher_is_better": True, "scaling": "strong",
           "vs_baseline": None, "dtype": "f32", "data": data,
           "config": {"workload": workload, "width": w, "height": h, "spp": spp, "samples_per_step": n_samples,
                      "timed_region": "lrt_render / lrt_render_backward entry to the developed image (gradients) in device memory; scene resident in HBM",
                      "parallelism": "1 GPU" if world == 1 else f"32x32 pixel tiles over {world} GPUs + RCCL film all-reduce"},
           "roofline": roofline}
    if dumped is not None:
        out["dumped_outputs"] = {"dir": a.dump_outputs, "seed_of_step": a.steps - 1, "arrays": {k: list(s) for k, s in dumped.items()}}
    if cfg.get("published_msamples") and world == 1 and not (a.spp or a.width or a.height or a.scene or a.integrator):
        # BASELINE.md holds a published figure for exactly this scene, resolution and sample count (the reference's own time.txt;
        # hardware unstated there): the ratio is reported for this config only
        out["vs_baseline"] = round(value / cfg["published_msamples"], 2)
        out["config"]["published"] = {"value": cfg["published_msamples"], "unit": "Msamples/s", "source": "scenes/Liver-MultiMesh/mitsuba3/time.txt (BASELINE.md), GPU unstated"}

    if rank == 0 and world == 1 and not backward and a.extra_legs:
        # SURVEY.md 8d's form of the metric: lrt_render entry to the developed image AND raw film in host memory (PCIe included).
        # Reported beside `value`, never as it: the bench contract takes `value` with everything resident in HBM.
        scene.render(spp=spp, seed=77, return_raw=True)
        t1 = time.perf_counter()
        for i in range(max(1, a.steps)): scene.render(spp=spp, seed=i, return_raw=True)
        hdt = (time.perf_counter() - t1) / max(1, a.steps)
        out["host_visible"] = {"value": round(n_samples / hdt / 1e6, 3), "unit": "Msamples/s", "ms_per_step": round(hdt * 1e3, 3),
                               "note": "lrt_render with host output buffers: developed image + raw film copied over PCIe inside the call (SURVEY.md 8d t_render); reported beside `value`, never as it"}

    if rank == 0 and world == 1 and a.config == "c3" and not (a.scene or a.integrator) and a.extra_legs:
        # BASELINE.json config 3 is worded "homogeneous medium + HG phase"; the scene file says isotropic.  A --full
        # line carries both: `value` on the file as committed, `hg_phase` on the same workload with the phase function set to
        # HG, g = 0.7, through the parameter interface (mi.traverse) - same size, same timed region, same number of steps.
        hg = load(mi, CONFIGS["c3hg"], spp, w, h, integrator_override)
        dev = torch.device("cuda", local_rank)
        film = torch.zeros((h, w, C), dtype=torch.float32, device=dev); image = torch.empty((h, w, C - 1), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        hg.render_to_device(film.data_ptr(), image.data_ptr(), spp=spp, seed=999, device=local_rank)
        torch.cuda.synchronize(); t1 = time.perf_counter(); hk = hi = hr = 0.0
        for i in range(a.steps):
            hg.render_to_device(film.data_ptr(), image.data_ptr(), spp=spp, seed=i, device=local_rank)
            hs = hg.stats(); hk += hs["kernel_ms"]; hi += hs["n_iter"]; hr += hs["n_records"]
        torch.cuda.synchronize(); hdt = (time.perf_counter() - t1) / a.steps
        hb = 2.0 * rec_b * hr + 4.0 * C * w * h * a.steps                 # (same scene, same record layout as the main leg)
        out["hg_phase"] = {"value": round(n_samples / hdt / 1e6, 3), "unit": "Msamples/s", "ms_per_step": round(hdt * 1e3, 3), "g": 0.7,
                           "workload": CONFIGS["c3hg"]["label"].format(integrator=integrator, w=w, h=h, spp=spp),
                           "roofline_frac": round(hb / (hk * 1e-3) / 1e9 / HBM_PEAK_GBS, 5) if hk > 0 else None,
                           "iterations_per_sample": hi / (n_samples * a.steps), "records_per_sample": hr / (n_samples * a.steps)}

    if rank == 0 and world == 1 and not a.no_cpu_baseline and not backward and a.extra_legs:
        # ---- CPU baseline (reported, not a target): the oracle's scalar_rgb restatement - SamplingIntegrator::render's scalar branch,
        # 32x32 blocks in Morton order, one std::thread per granted core (oracle/orc_render.cpp orc_render_scalar; SURVEY.md 8d,
        # BASELINE.md section 3.5) - on a bounded sample of the same workload: same scene and resolution at a reduced spp.
        # Built here with -O3 -march=native for the box's own host CPU when g++ is present (the shipped liborc.so is -O2 -mfma so that
        # it runs on any x86-64-v3 host); both builds keep -ffp-contract=off and give the same numbers (tests/test_oracle_pins.py).
        import subprocess, tempfile
        import orc
        cores = usable_cores()
        flags = "g++ -O2 -mfma -ffp-contract=off (shipped oracle/liborc.so)"
        try:
            tmp = tempfile.mkdtemp(prefix="lrt_orc_"); _TMP.append(tmp)
            native = os.path.join(tmp, "liborc_native.so")
            src = [os.path.join(ROOT, "oracle", f) for f in ("orc_scene.cpp", "orc_render.cpp", "orc_api.cpp", "orc_vae.cpp")]
            subprocess.run(["g++", "-O3", "-march=native", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-pthread", "-shared", "-o", native] + src,
                           check=True, capture_output=True, timeout=300)
            orc.use_library(native); flags = "g++ -O3 -march=native -ffp-contract=off -fno-fast-math, built on this host"
        except Exception:
            pass
        if a.cpu_spp <= 0:                       # calibrate on 1 spp so that the sample takes ~15 s of wall time
            cs = load(mi, cfg, 1, w, h, integrator_override)
            c_spp1 = cs.spp
            t1 = time.perf_counter(); orc.OrcScene(cs).render(threads=cores, seed=0, scalar=True); c1 = (time.perf_counter() - t1) / c_spp1
            a.cpu_spp = int(min(spp, max(1, round(15.0 / max(c1, 1e-3)))))
        cs = load(mi, cfg, a.cpu_spp, w, h, integrator_override)
        cpu_spp = cs.spp
        o = orc.OrcScene(cs)
        t1 = time.perf_counter()
        o.render(threads=cores, seed=0, scalar=True)
        ct = time.perf_counter() - t1
        out["cpu_baseline"] = {"value": round(w * h * cpu_spp / ct / 1e6, 4), "unit": "Msamples/s", "cores": cores, "kind": "port",
                               "sample": f"same scene and resolution at {cpu_spp} spp ({w * h * cpu_spp} samples, {ct:.1f} s)",
                               "build": f"oracle (scalar C++ restatement of the reference's scalar_rgb render loop, orc_render_scalar): {flags}; one std::thread per granted core"}
        # ---- RMSE against the llvm_ad_rgb restatement (lane semantics, same seeding as the GPU): same seed, a sample of <= 4 spp
        r_spp = max(1, min(cpu_spp, 4))
        rs = load(mi, cfg, r_spp, w, h, integrator_override); r_spp = rs.spp
        cimg = orc.OrcScene(rs).render(threads=cores, seed=0)
        gimg = rs.render(seed=0)
        rmse = float(np.sqrt(np.mean((gimg.astype(np.float64) - cimg.astype(np.float64)) ** 2)))
        out["rmse_vs_oracle"] = {"value": rmse, "spp": r_spp, "tolerance": 1e-4,
                                 "note": "against the oracle's llvm_ad_rgb lane semantics at the same seed: per-lane radiance is bit-identical, the film differs by float-atomic order only"}
    if rank == 0:
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    import shutil
    for t in _TMP: shutil.rmtree(t, ignore_errors=True)


if __name__ == "__main__":
    main()
