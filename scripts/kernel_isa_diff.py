"""Compare the gfx950 machine code of two builds, kernel by kernel.

    python scripts/kernel_isa_diff.py OLD NEW [--map REGEX=REPL ...]

OLD and NEW are source trees (ext.hip is compiled device-only to assembly,
no GPU needed) or ready-made .s files. Kernels are paired by mangled name
after the --map rewrites (for renamed templates, e.g.
'(attn_bwd_dkv_kernelILi\\d+ELi\\d+E)Li0ELi2E=\\1'). Prints the kernels on one
side only and the paired ones whose bodies differ; exits 1 if any differ."""
import argparse, os, re, subprocess, sys, sysconfig, tempfile


def assembly(path):
    if os.path.isfile(path):
        return open(path).read()
    from torch.utils.cpp_extension import include_paths
    incs = include_paths() + [sysconfig.get_paths()["include"]]
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "ext.s")
        subprocess.run(["hipcc", "--offload-arch=gfx950", "--cuda-device-only", "-S", "-O3",
                        "-std=c++17", *("-I" + i for i in incs), "-o", out,
                        os.path.join(path, "midgpt_amd/ops/csrc/ext.hip")], check=True)
        return open(out).read()


def normalise(text):
    out = []
    for line in text.split("\n"):
        line = line.split(";")[0].rstrip()
        if re.match(r"\s*\.(section|text)\b", line):  # placement, not code
            continue
        line = re.sub(r"\.L([A-Za-z_]+?)\d+(_|\b)", r".L\1\2", line)  # per-function label numbers
        out.append(re.sub(r"\b_Z\w+", "SYM", line))
    return [l for l in out if l]


def kernels(text, maps):
    """{mapped name: normalised body + .amdhsa_kernel block} of every kernel."""
    found = {}
    for m in re.finditer(r"^[ \t]*\.amdhsa_kernel (\S+)\n.*?\.end_amdhsa_kernel", text, re.M | re.S):
        name, desc = m.group(1), m.group(0)
        body = re.search(rf"^{name}:.*?^\.Lfunc_end\d+:", text, re.M | re.S).group(0)
        for rx, repl in maps:
            name = re.sub(rx, repl, name)
        found[name] = normalise(body.replace(desc, "")) + normalise(desc)
    return found


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--map", action="append", default=[], metavar="REGEX=REPL")
    args = ap.parse_args()
    maps = [m.split("=", 1) for m in args.map]
    old, new = (kernels(assembly(p), maps) for p in (args.old, args.new))
    paired = old.keys() & new.keys()
    differ = sorted(n for n in paired if old[n] != new[n])
    for title, names in (("only in old", sorted(old.keys() - paired)),
                         ("only in new", sorted(new.keys() - paired)), ("bodies differ", differ)):
        print(f"{title}: {len(names)}", *names, sep="\n  ")
    print(f"kernels: old {len(old)}, new {len(new)}, paired {len(paired)}, identical "
          f"{len(paired) - len(differ)}, lines compared {sum(len(new[n]) for n in paired)}")
    sys.exit(1 if differ else 0)


if __name__ == "__main__":
    main()
