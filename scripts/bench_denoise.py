"""Time the guided denoiser at 1920 x 1080 with both guides on device buffers, against a plain torch
restatement of the same filter on the same GPU (padded shifts, one torch.exp per tap, float32), the two alternating in one run.

  python scripts/bench_denoise.py                         timing: device events around windows of back-to-back calls, best of 5, spread
  rocprofv3 --kernel-trace --stats -d DIR -- python scripts/bench_denoise.py --trace-target
  python scripts/bench_denoise.py --trace-dir DIR          per-pass kernel times from that trace, bytes per pass, share of HBM rate
Prints one JSON line last."""
import argparse
import csv
import glob
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_ACHIEVABLE = 6.3e12          # bytes / s


def make_inputs(h, w, seed=0):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    region = ((x // 97 + y // 61) % 4).astype(np.float32)
    albedo = (0.2 + 0.2 * region[..., None] + 0.02 * rng.random((h, w, 3))).astype(np.float32)
    normals = np.stack([np.sin(0.01 * x + region), np.cos(0.013 * y), np.ones_like(x)], axis=2)
    normals = (normals / np.linalg.norm(normals, axis=2, keepdims=True)).astype(np.float32)
    light = 1.0 + 0.5 * np.sin(0.004 * (x + 2 * y))
    noisy = (albedo * light[..., None] * (1 + 0.4 * rng.standard_normal((h, w, 3)))).astype(np.float32)
    return noisy, albedo, normals


def torch_denoise(torch, noisy, albedo, normals, p):
    """The filter of DESIGN.md section 9.1 in plain torch ops (not held to the bits: torch.exp and torch's own sum order)."""
    H, W = noisy.shape[:2]
    hk = (1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16)
    eps = p["eps_a"]
    d = torch.where(albedo > eps, albedo, torch.full_like(albedo, eps))
    c = noisy[..., :3] / d
    ok = torch.isfinite(c).all(2) & torch.isfinite(albedo).all(2) & torch.isfinite(normals).all(2)
    i_n, i_a = 1.0 / p["sigma_normal"] ** 2, 1.0 / p["sigma_albedo"] ** 2

    def padded(t, r):
        out = torch.zeros((H + 2 * r, W + 2 * r) + tuple(t.shape[2:]), dtype=t.dtype, device=t.device)
        out[r:r + H, r:r + W] = t
        return out
    for k in range(p["iterations"]):
        s = 1 << k; r = 2 * s
        ic = 4.0 ** k / p["sigma_color"] ** 2
        cp, npad, apad, okp = padded(torch.where(ok[..., None], c, torch.zeros_like(c)), r), padded(normals, r), padded(albedo, r), padded(ok, r)
        sw = torch.zeros((H, W), dtype=c.dtype, device=c.device); sc = torch.zeros_like(c)
        for j in range(-2, 3):
            for i in range(-2, 3):
                ys, xs = slice(r + s * j, r + s * j + H), slice(r + s * i, r + s * i + W)
                cq = cp[ys, xs]
                e = ((cq - c) ** 2).sum(2) * ic + ((npad[ys, xs] - normals) ** 2).sum(2) * i_n + ((apad[ys, xs] - albedo) ** 2).sum(2) * i_a
                wt = (hk[i + 2] * hk[j + 2]) * torch.exp(-e) * okp[ys, xs]
                sw = sw + wt; sc = sc + wt[..., None] * cq
        c = torch.where(ok[..., None], sc / sw[..., None], c)
    return torch.where(ok[..., None], c * d, noisy[..., :3])


def per_pass_from_trace(trace_dir, iterations):
    """Mean duration of each pass (by its position between a pack and an unpack kernel), of the prologue and of the epilogue."""
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {trace_dir}")
    rows = []
    for f in files:
        for r in csv.DictReader(open(f)):
            if "k_denoise" in r["Kernel_Name"]:
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    passes = [[] for _ in range(iterations)]; pack, unpack = [], []; k = 0
    for _, dur, name in rows:
        if "k_denoise_pack" in name: pack.append(dur); k = 0
        elif "k_denoise_unpack" in name: unpack.append(dur)
        else: passes[k % iterations].append(dur); k += 1
    skip = lambda v: v[len(v) // 4:]                          # the first quarter of the calls is warm-up
    return {"pack_us": float(np.mean(skip(pack))) / 1e3, "unpack_us": float(np.mean(skip(unpack))) / 1e3,
            "pass_us": [float(np.mean(skip(v))) / 1e3 for v in passes], "calls": len(pack)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920); ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--windows", type=int, default=5); ap.add_argument("--window-seconds", type=float, default=0.5)
    ap.add_argument("--trace-target", action="store_true", help="run 40 calls and exit (the program to put behind rocprofv3 --kernel-trace --stats)")
    ap.add_argument("--trace-dir", help="summarise the kernel trace under this directory instead of timing")
    a = ap.parse_args()
    W, H = a.width, a.height
    npx = W * H
    bytes_pass = npx * (16 + 16 + 16 + 16)                   # colour, normal and albedo records in, colour record out
    if a.trace_dir:
        t = per_pass_from_trace(a.trace_dir, 5)
        t.update({"bytes_per_pass": bytes_pass, "pass_GBps": [bytes_pass / (us * 1e-6) / 1e9 for us in t["pass_us"]],
                  "pass_share_of_hbm_rate": [bytes_pass / (us * 1e-6) / HBM_ACHIEVABLE for us in t["pass_us"]]})
        print(json.dumps({"bench": "denoise_trace", "size": [W, H], **t})); return
    import torch
    import liverrenderer_amd as mi
    if not torch.cuda.is_available():
        raise SystemExit("bench_denoise.py needs a GPU: there is no CPU path to time")
    noisy, albedo, normals = (torch.from_numpy(x).cuda() for x in make_inputs(H, W))
    dn = mi.Denoiser((W, H), albedo=True, normals=True)
    if a.trace_target:
        for _ in range(40): dn(noisy, albedo, normals)
        torch.cuda.synchronize(); return
    hip = lambda: dn(noisy, albedo, normals)
    ref = lambda: torch_denoise(torch, noisy, albedo, normals, dn.params)
    out_h, out_t = hip(), ref()                               # warm-up of both, and a sanity check that they are the same filter
    torch.cuda.synchronize()
    diff = float((out_h - out_t).abs().max())

    def window(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls): fn()
        e1.record(); e1.synchronize()
        return e0.elapsed_time(e1) / calls                    # ms per call
    for fn in (hip, ref): window(fn, 3)
    calls_h = max(3, int(a.window_seconds * 1e3 / window(hip, 10)))
    calls_t = max(3, int(a.window_seconds * 1e3 / window(ref, 3)))
    th, tt = [], []
    for _ in range(a.windows):                                # alternating
        th.append(window(hip, calls_h)); tt.append(window(ref, calls_t))
    res = {"bench": "denoise", "size": [W, H], "params": dn.params, "calls_per_window": {"hip": calls_h, "torch": calls_t},
           "hip_ms_per_call": {"best": min(th), "median": float(np.median(th)), "worst": max(th)},
           "torch_ms_per_call": {"best": min(tt), "median": float(np.median(tt)), "worst": max(tt)},
           "speedup_best": min(tt) / min(th), "max_abs_diff_hip_vs_torch": diff, "bytes_per_pass": bytes_pass,
           "hbm_floor_ms_per_call": (5 * bytes_pass + npx * (36 + 48) + npx * (44 + 12)) / HBM_ACHIEVABLE * 1e3}
    print(json.dumps(res))
    if not min(th) < min(tt):
        raise SystemExit("the HIP path is not faster than the torch restatement")


if __name__ == "__main__":
    main()
