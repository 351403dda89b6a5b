"""bench.py as the driver runs it: one JSON line on stdout with the keys of the bench contract (task statement, section 4), at a reduced
sample count so that the test takes seconds; the N = 2 launch line of the contract with the gloo backend on the one GPU of the box."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

ENV = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")


def last_json(out):
    lines = [l for l in out.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out[-2000:]
    return json.loads(lines[0])


EXTRA_LEGS = ("host_visible", "hg_phase", "cpu_baseline", "rmse_vs_oracle")


def test_bench_line_plain_n1():
    """a plain run is the headline figure alone: the contract keys and the roofline of the timed launches, none of the legs of --full"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--spp", "16"],
                       capture_output=True, text=True, cwd=ROOT, env=ENV, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    j = last_json(r.stdout)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config", "roofline"):
        assert k in j, k
    assert j["metric"] == "Msamples/s" and j["unit"] == "Msamples/s" and j["n_gpus"] == 1 and j["steps"] == 2 and j["warmup"] == 1
    assert j["higher_is_better"] is True and j["dtype"] == "f32" and j["config"]["spp"] == 16
    assert abs(j["value"] - j["config"]["samples_per_step"] / (j["ms_per_step"] * 1e-3) / 1e6) < 1e-2 * j["value"]
    assert j["roofline"]["kernel"].startswith("lrt::k_render<1, 1024, true") and j["roofline"]["avg_launch_ms"] > 0
    assert not any(k in j for k in EXTRA_LEGS), [k for k in EXTRA_LEGS if k in j]


def test_bench_line_n1():
    """--full: the headline figure and, beside it, the legs that take runs of their own"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--spp", "16", "--cpu-spp", "1", "--full"],
                       capture_output=True, text=True, cwd=ROOT, env=ENV, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    j = last_json(r.stdout)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in j, k
    assert j["metric"] == "Msamples/s" and j["unit"] == "Msamples/s" and j["n_gpus"] == 1 and j["steps"] == 2 and j["warmup"] == 1
    assert j["higher_is_better"] is True and j["dtype"] == "f32" and j["vs_baseline"] is None and "workload" in j["config"]
    assert abs(j["value"] - j["config"]["samples_per_step"] / (j["ms_per_step"] * 1e-3) / 1e6) < 1e-2 * j["value"]
    ro = j["roofline"]
    assert ro["bound"] == "hbm" and ro["unit"] == "GB/s" and ro["peak"] == 8000.0 and abs(ro["frac"] - ro["achieved"] / ro["peak"]) < 1e-4
    assert ro["kernel"].startswith("lrt::k_render<1, 1024, true") and ro["avg_launch_ms"] > 0 and ro["avg_launch_ms"] <= j["ms_per_step"] * 1.001
    assert ro["traffic"] is None or ro["traffic_source"]            # traffic only from a profile of THIS build of the kernels (kernel_source_id)
    cb = j["cpu_baseline"]
    assert cb["kind"] == "port" and cb["cores"] >= 1 and cb["value"] > 0 and "spp" in cb["sample"] and "orc_render_scalar" in cb["build"]
    assert j["rmse_vs_oracle"]["value"] <= j["rmse_vs_oracle"]["tolerance"]
    hg = j["hg_phase"]                                            # BASELINE.json config 3 as worded (HG phase) rides in the --full line
    assert hg["g"] == 0.7 and hg["value"] > 0 and "HG phase" in hg["workload"]
    assert j["host_visible"]["value"] > 0 and j["host_visible"]["value"] <= j["value"] * 1.05


@pytest.mark.parametrize("config,samples", [("c3", 1920 * 1080 * 8), ("c2", 1080 * 1080 * 8), ("c5", 1920 * 1080 * 16)])
def test_bench_line_two_ranks_gloo(config, samples):
    """the driver's N = 2 launch line (gloo instead of RCCL: both ranks share the box's one GPU): film all-reduce + develop for the
    forward configurations, gradient all-reduce for the PRB one (c5: ld sampler, 8 -> 16 spp; tent filter: weight film over tiles + halo)"""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(29700 + (os.getpid() + len(config) * 7 + samples) % 200),
           os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--spp", "8", "--backend", "gloo", "--config", config]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, env=ENV, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    j = last_json(r.stdout)
    assert j["n_gpus"] == 2 and j["scaling"] == "strong" and "cpu_baseline" not in j and "hg_phase" not in j
    assert j["config"]["samples_per_step"] == samples and j["value"] > 0
    assert "2 GPUs" in j["config"]["parallelism"]


@pytest.mark.parametrize("config", ["het", "mis"])
def test_bench_f4_configs(config):
    """SURVEY.md 8f row 4 has bench configurations of its own: a short run of each prints a line whose roofline names
    the heterogeneous-media / volpathmis kernel and prices its wider record."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--config", config, "--steps", "1", "--warmup", "1", "--spp", "4", "--width", "256", "--height", "256", "--no-cpu-baseline"],
                       capture_output=True, text=True, cwd=ROOT, env=ENV, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    j = last_json(r.stdout); ro = j["roofline"]
    assert ro["kernel"].startswith("lrt::k_render<101," if config == "het" else "lrt::k_render<5,") and ro["record_bytes"] == (104 if config == "het" else 168)
    assert j["value"] > 0 and ro["records_per_sample"] > 0 and j["data"].startswith("synthetic")


@pytest.mark.parametrize("config,extra,names", [("c3", ["--spp", "16"], {"image", "film", "pixel_index"}),
                                                ("c5", ["--spp", "4", "--width", "256", "--height", "256"], {"grad_sigma_t", "grad_albedo", "grad_g"})])
def test_bench_dump_outputs(tmp_path, config, extra, names):
    """--dump-outputs DIR: the last timed step's outputs as DIR/<name>.npy in float32 / float64, at most 64 MB in all; --steps sets the
    number of timed steps"""
    d = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--config", config, "--steps", "3", "--warmup", "1", "--main-only", "--dump-outputs", str(d)] + extra,
                       capture_output=True, text=True, cwd=ROOT, env=ENV, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    j = last_json(r.stdout)
    assert j["steps"] == 3 and j["ms_per_step"] > 0 and j["dumped_outputs"]["seed_of_step"] == 2
    got = {f[:-4]: np.load(d / f) for f in os.listdir(d)}
    assert set(got) == names == set(j["dumped_outputs"]["arrays"])
    assert sum(os.path.getsize(d / f) for f in os.listdir(d)) <= 64 * 1000 * 1000
    assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in got.values())
    if config == "c3":                                          # RGBA image + 5-channel film at 1920x1080: 75 MB, so a fixed pixel sample
        h, w = j["config"]["height"], j["config"]["width"]; idx = got["pixel_index"]
        assert h * w // 2 < len(idx) < h * w and np.all(np.diff(idx) > 0)
        assert got["image"].shape == (len(idx), 4) and got["film"].shape == (len(idx), 5)
        assert (got["film"][:, 4] > 0).all() and (got["image"][:, 3] == 1).all() and 0 < got["image"][:, :3].mean() < 10
    else:
        assert got["grad_sigma_t"].shape == (3,) and got["grad_albedo"].shape == (3,) and np.abs(got["grad_sigma_t"]).sum() > 0
