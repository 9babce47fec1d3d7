#!/usr/bin/env python3
"""Compare the gfx950 code of every kernel in two source trees: each .hip that a tree's Makefile
builds into libtfrg.so is compiled to assembly (the Makefile's own command for it plus
--offload-device-only -S), and per kernel symbol the instruction text is compared after dropping `;`
comments and renumbering local labels. Prints SAME or DIFF per kernel, ONLY-A / ONLY-B for a symbol
one tree lacks, and the compiler's kernel-resource-usage figures per kernel of both trees; exit status
1 unless every kernel is SAME. The comparison is textual: it does not look at which instructions appear.

usage: kernel_isa_diff.py TREE_A TREE_B [--keep DIR]   (trees: repository roots; --keep: the .s files)"""
import argparse
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

CSRC = Path("tfrecords-reader_amd") / "csrc"
LABEL = re.compile(r"\.L[A-Za-z_$]+[0-9]+(?:_[0-9]+)?")


def product_units(tree: Path) -> list[tuple[list[str], Path]]:
    """(compile command without -c / -o, source) of every .hip the Makefile compiles into libtfrg.so."""
    p = subprocess.run(["make", "-n", "-B", "-C", str(tree / CSRC), "../tfr_reader/libtfrg.so"], capture_output=True,
                       text=True, check=True)
    units = []
    for ln in p.stdout.splitlines():
        m = re.match(r"^(\S*hipcc) (.*) -c (\S+\.hip) -o \S+$", ln.strip())
        if m and "--offload-arch" in m.group(2):
            units.append(([m.group(1), *m.group(2).split()], tree / CSRC / m.group(3)))
    return units


def compile_tree(tree: Path, out: Path) -> tuple[dict[str, list[str]], list[str]]:
    """{kernel symbol: normalised lines}, resource-usage remarks."""
    out.mkdir(parents=True, exist_ok=True)

    def one(unit):
        cmd, src = unit
        s, r = out / (src.stem + ".s"), out / (src.stem + ".remarks")
        newest = max(f.stat().st_mtime for f in src.parent.iterdir() if f.is_file())
        if s.exists() and r.exists() and s.stat().st_mtime > newest:  # (--keep: a tree compiled before)
            return s.read_text(), r.read_text().splitlines()
        p = subprocess.run([*cmd, "--offload-device-only", "-S", "-Rpass-analysis=kernel-resource-usage",
                            src.name, "-o", str(s)], cwd=src.parent, capture_output=True, text=True)
        if p.returncode:
            sys.exit(f"{src}: {p.stderr}")
        r.write_text("\n".join(ln for ln in p.stderr.splitlines() if "remark:" in ln))
        return s.read_text(), r.read_text().splitlines()

    kernels, remarks = {}, []
    with ThreadPoolExecutor(8) as ex:
        for asm, rem in ex.map(one, product_units(tree)):
            remarks += [re.sub(r"^\S*?([^/\s]+\.(?:hip|h)):", r"\1:", ln) for ln in rem]
            kernels.update(split_kernels(asm))
    return kernels, remarks


def split_kernels(asm: str) -> dict[str, list[str]]:
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M))
    res, cur, ids = {}, None, {}
    for ln in asm.splitlines():
        ln = ln.split(";", 1)[0].strip()
        if not ln:
            continue
        if cur is None:
            if ln.endswith(":") and ln[:-1] in names:
                cur, ids = ln[:-1], {}
                res[cur] = []
            continue
        if ln.startswith(".Lfunc_end"):
            cur = None
            continue
        res[cur].append(LABEL.sub(lambda m: ids.setdefault(m.group(0), f".L{len(ids)}"), ln))
    return res


def resources(remarks: list[str]) -> dict[str, str]:
    """{kernel symbol: the kernel-resource-usage remark's figures on one line}."""
    res, cur = {}, None
    for ln in remarks:
        m = re.search(r"remark:\s+(.*?):\s+(\S+) \[-Rpass-analysis", ln)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = m.group(2)
            res[cur] = ""
        elif cur:
            res[cur] += f" {m.group(1).split(' [')[0]}={m.group(2)}"
    return res


def demangle(names: list[str]) -> dict[str, str]:
    try:
        p = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
        return dict(zip(names, p.stdout.splitlines()))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def short(name: str) -> str:
    """A demangled kernel name without its parameter list (the template arguments stay)."""
    depth = 0
    for i in range(len(name) - 1, -1, -1):
        depth += (name[i] == ")") - (name[i] == "(")
        if depth == 0 and name[i] == "(":
            return name[:i].replace("void ", "")
    return name


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("tree_a", type=Path)
    ap.add_argument("tree_b", type=Path)
    ap.add_argument("--keep", type=Path)
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as td:
        keep = a.keep or Path(td)
        ka, ra = compile_tree(a.tree_a.resolve(), keep / "a")
        kb, rb = compile_tree(a.tree_b.resolve(), keep / "b")
    names = sorted(set(ka) | set(kb))
    pretty = demangle(names)
    bad = 0
    for n in names:
        v = "ONLY-A" if n not in kb else "ONLY-B" if n not in ka else "SAME" if ka[n] == kb[n] else "DIFF"
        bad += v != "SAME"
        print(f"{v:6s} {len(ka.get(n, kb.get(n))):6d} lines  {short(pretty[n])}")
    print(f"\n{len(names)} kernels, {bad} not SAME")
    res_a, res_b = resources(ra), resources(rb)
    print("\n== kernel-resource-usage, tree A")
    for n in names:
        print(f"{short(pretty[n])}:{res_a.get(n, ' -')}")
    print("\n== kernel-resource-usage, tree B: the kernels whose figures differ from tree A's")
    for n in names:
        if res_b.get(n) != res_a.get(n):
            print(f"{short(pretty[n])}:{res_b.get(n, ' -')}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
