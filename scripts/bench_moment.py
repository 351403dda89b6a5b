"""Cost of the moment integrator on C3 (Liver-SingleMesh, volpath, 1920x1080, 512 spp, box filter): the same scene rendered as a
plain lrt_render and under <integrator type="moment">, both into device buffers, in one process, in alternating windows.  Times are
host-clock intervals around calls that end in a stream synchronise.  Prints best and median per leg, the ratio, and the bytes the
lane-buffer route moves (16 B written + 16 B read per lane, plus the film atomics), one JSON line.
python scripts/bench_moment.py [reps]

For k_moment_splat's own time run it once under the profiler, in a run of its own:
rocprofv3 --kernel-trace --stats -d <out dir> -- python scripts/bench_moment.py 1"""
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import liverrenderer_amd as mi  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
W, H, SPP = 1920, 1080, 512
xml_path = os.path.join(ROOT, "scenes", "Liver-SingleMesh", "mitsuba3", "scene.xml")
text = open(xml_path).read()
wrapped, n = re.subn(r'<integrator type="\$integrator">(.*?)</integrator>',
                     r'<integrator type="moment"><integrator type="$integrator" name="img">\1</integrator></integrator>', text, flags=re.S)
assert n == 1
kw = dict(integrator="volpath", spp=SPP, res_width=W, res_height=H)
plain = mi.load_file(xml_path, **kw)
moment = mi.load_string(wrapped, os.path.dirname(xml_path), **kw)
assert plain.desc.film.rfilter == 0 and moment.is_moment()
md = moment.moment_desc()
dev = torch.device("cuda:0")
film_p = torch.empty((H, W, plain.raw_channels()), dtype=torch.float32, device=dev)
film_m = torch.empty((H, W, md.n_raw_channels), dtype=torch.float32, device=dev)
img_m = torch.empty((H, W, md.n_channels), dtype=torch.float32, device=dev)
torch.cuda.synchronize()


def run_plain(spp=0):
    t = time.perf_counter(); plain.render_to_device(film_p.data_ptr(), spp=spp); return (time.perf_counter() - t) * 1e3


def run_moment(spp=0):
    t = time.perf_counter(); moment.render_moment_to_device(film_m.data_ptr(), img_m.data_ptr(), spp=spp); return (time.perf_counter() - t) * 1e3


run_plain(8); run_moment(8); run_plain(); run_moment()          # warm-up: device images, workspaces (the 4 GiB lane buffer), both code paths
tp, tm, kp, km = [], [], [], []
for _ in range(reps):
    tp.append(run_plain()); kp.append(plain.stats()["kernel_ms"])
    tm.append(run_moment()); km.append(moment.stats()["kernel_ms"])
# the colour part of the moment film is the plain film
fm, fp = film_m[..., :plain.raw_channels()], film_p
rel = float(((fm - fp).abs() / fp.abs().clamp(min=1.0)).max())
lanes = W * H * SPP
extra_bytes = lanes * 32 + W * H * md.n_raw_channels * 4 * (SPP // 64)       # lane buffer round trip + one film record per wave and pixel
print(json.dumps({"scene": "C3 Liver-SingleMesh volpath, box filter", "width": W, "height": H, "spp": SPP, "reps": reps,
                  "plain_ms_best": round(min(tp), 2), "plain_ms_median": round(statistics.median(tp), 2),
                  "moment_ms_best": round(min(tm), 2), "moment_ms_median": round(statistics.median(tm), 2),
                  "ratio_best": round(min(tm) / min(tp), 4), "ratio_median": round(statistics.median(tm) / statistics.median(tp), 4),
                  "render_kernel_ms_plain_best": round(min(kp), 2), "render_kernel_ms_moment_best": round(min(km), 2),
                  "lane_buffer_and_film_bytes": extra_bytes, "colour_film_max_rel_diff": rel,
                  "record_bytes": int(moment.stats()["record_bytes"])}))
