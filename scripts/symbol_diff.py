"""Per-symbol comparison of the gfx950 code objects of two builds of libliverrt.so: which functions are instruction-identical, addresses aside
(DESIGN.md sections 6d - 6g: "N of M functions are instruction-identical to the parent's").  Usage: python scripts/symbol_diff.py PARENT.so BUILD.so
Each library's .hip_fatbin section is unbundled for gfx950 and disassembled with llvm-objdump -d --no-show-raw-insn; per function the listing is
compared without its address comments and with branch targets (<symbol+offset>) blanked.  For a function that differs: its instruction count, the
vector instructions, s_nop, float atomics and DPP instructions on both sides."""
import collections, re, subprocess, sys, tempfile

LLVM = "/opt/rocm/llvm/bin"


def functions(lib):
    d = tempfile.mkdtemp(); fat, co = d + "/fat.bin", d + "/gfx950.co"
    subprocess.run([LLVM + "/llvm-objcopy", "--dump-section", ".hip_fatbin=" + fat, lib, d + "/stripped.so"], check=True, capture_output=True)
    subprocess.run([LLVM + "/clang-offload-bundler", "--unbundle", "--type=o", "--input=" + fat, "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co], check=True, capture_output=True)
    out = subprocess.run([LLVM + "/llvm-objdump", "-d", "--no-show-raw-insn", co], check=True, capture_output=True, text=True).stdout
    f = collections.OrderedDict(); cur = None
    for line in out.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.*)>:$", line)
        if m:
            cur = m.group(1); f[cur] = []; continue
        if cur is None or not line.strip():
            continue
        f[cur].append(re.sub(r"<[^>]*>", "<>", line.split("//")[0].rstrip()))
    return f


def count(listing, pattern):
    return sum(1 for x in listing if re.search(pattern, x))


if __name__ == "__main__":
    a, b = functions(sys.argv[1]), functions(sys.argv[2])
    diff = [k for k in a if k in b and a[k] != b[k]]
    print("functions: parent %d, build %d, identical %d, different %d, only in the parent %d, only in the build %d" % (
        len(a), len(b), sum(1 for k in a if k in b and a[k] == b[k]), len(diff), sum(1 for k in a if k not in b), sum(1 for k in b if k not in a)))
    for k in diff:
        print(k, "| instructions %d -> %d" % (len(a[k]), len(b[k])), *("| %s %d -> %d" % (name, count(a[k], p), count(b[k], p)) for name, p in
              (("v_*", r"^\s*v_"), ("s_nop", "s_nop"), ("global_atomic_add_f32", "global_atomic_add_f32"), ("dpp", "dpp"))))
