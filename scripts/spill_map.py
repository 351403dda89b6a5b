"""Spill map of one k_render instance: registers, spills and scratch bytes from the code-object metadata, and the static
scratch_load / scratch_store count per loop depth (LLVM's `Loop Header: Depth=N` block comments).

    python scripts/spill_map.py                    # the C3 instance: k_render<1,1024,true,false,true,false> (volpath, compact records)
    python scripts/spill_map.py --wide             # k_render<1,1024,true,false,false,false> (C3 with wide records)
    python scripts/spill_map.py --s file.s         # an existing listing instead of compiling
    python scripts/spill_map.py -- -DLRT_DEV_INTEGRATOR=LRT_INTEGRATOR_BIOVOLPATH    # extra hipcc flags after --

The kernel is compiled device-only with the Makefile's flags and -DLRT_DEV_VOLPATH_ONLY (the `make dev` build: one render kernel)."""
import argparse, os, re, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "liverrenderer_amd", "csrc", "device.hip")
FLAGS = ["-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-slp-vectorize", "-fvisibility=hidden", "-Wno-unused-function", "-Wno-unused-result"]


def compile_listing(extra, out):
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", *FLAGS, "-DLRT_DEV_VOLPATH_ONLY", *extra, "--cuda-device-only", "-S", SRC, "-o", out]
    subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)


def demangle(n):
    """k_render<...> from the mangled name (its template arguments are integers and booleans only)."""
    m = re.search(r"8k_renderI((?:L[ib]\d+E)+)E", n)
    if not m: return n
    args = re.findall(r"L([ib])(\d+)E", m.group(1))
    return "k_render<" + ", ".join(v if k == "i" else ("true" if v == "1" else "false") for k, v in args) + ">"


def kernel_body(lines, sym):
    start = next(i for i, l in enumerate(lines) if l.startswith(sym + ":"))
    end = next(i for i in range(start + 1, len(lines)) if lines[i].startswith(".Lfunc_end"))
    return lines[start:end]


def metadata(text, sym):
    """The kernel's entry in the amdhsa.kernels metadata block (YAML): the scalar fields that describe its resources."""
    meta = text[text.find(".amdgpu_metadata"):]
    blk = next((e for e in re.split(r"\n  - ", meta) if re.search(r"^\s*\.name:\s+" + re.escape(sym) + r"\s*$", e, re.M)), "")
    out = {}
    for k in ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size"):
        mm = re.search(r"\." + k + r":\s+(\d+)", blk)
        out[k] = int(mm.group(1)) if mm else None
    return out


def scratch_by_depth(body):
    """Static scratch accesses per loop depth.  A block's depth is the one its `Loop Header: Depth=N` or `in Loop: Header=... Depth=N`
    comment names; blocks without such a comment are at depth 0."""
    depth = 0; loads = {}; stores = {}
    for l in body:
        if l.startswith(".LBB") or l.startswith("; %bb"):
            m = re.search(r"Depth=(\d+)", l)
            depth = int(m.group(1)) if m else 0
            continue
        t = l.strip()
        if t.startswith("scratch_load"): loads[depth] = loads.get(depth, 0) + 1
        elif t.startswith("scratch_store"): stores[depth] = stores.get(depth, 0) + 1
    return loads, stores


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--s", help="read this hipcc -S listing instead of compiling")
    ap.add_argument("--wide", action="store_true", help="the wide-record instance (fifth template argument false)")
    ap.add_argument("--kernel", help="substring of the demangled name to select (overrides --wide)")
    ap.add_argument("extra", nargs="*", help="extra hipcc flags (after --)")
    a = ap.parse_args()
    path = a.s
    if not path:
        path = os.path.join(tempfile.mkdtemp(prefix="spill_map_"), "dev.s")
        compile_listing(a.extra, path)
    text = open(path).read()
    lines = text.splitlines()
    syms = [l.split(":")[0] for l in lines if re.match(r"_Z\S*k_render\S*:( |$)", l)]
    want = a.kernel or ("k_render<1, 1024, true, false, false, false>" if a.wide else "k_render<1, 1024, true, false, true, false>")
    picked = [s for s in syms if want in demangle(s)]
    if not picked:
        sys.exit("no k_render instance matches %r among: %s" % (want, ", ".join(demangle(s) for s in syms)))
    for sym in picked:
        body = kernel_body(lines, sym)
        md = metadata(text, sym)
        n_ins = sum(1 for l in body if l.startswith("\t") and not l.strip().startswith((".", ";")))
        print(demangle(sym))
        print("  VGPR %s  AGPR %s  SGPR %s  VGPR spills %s  SGPR spills %s  scratch %s B/lane  LDS %s B  instructions %d" % (
            md["vgpr_count"], md["agpr_count"], md["sgpr_count"], md["vgpr_spill_count"], md["sgpr_spill_count"], md["private_segment_fixed_size"],
            md["group_segment_fixed_size"], n_ins))
        loads, stores = scratch_by_depth(body)
        depths = sorted(set(loads) | set(stores))
        print("  scratch_load / scratch_store per loop depth: " + (", ".join("depth %d: %d / %d" % (d, loads.get(d, 0), stores.get(d, 0)) for d in depths) or "none"))
        print("  at depth >= 2 (inside the tile loop): %d" % sum(loads.get(d, 0) + stores.get(d, 0) for d in depths if d >= 2))


if __name__ == "__main__":
    main()
