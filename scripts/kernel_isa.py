#!/usr/bin/env python
"""Per-kernel device code of one source tree, or the difference between two (an A/B is two trees).

    python scripts/kernel_isa.py TREE            # one line per kernel: TU, body hash, registers, LDS, scratch, spills
    python scripts/kernel_isa.py TREE_A TREE_B   # kernels only in one tree, kernels whose body or resources differ

Every translation unit in a tree's build.py SOURCES is compiled to gfx950 assembly with that tree's FLAGS.  A kernel is keyed by
its base name and template arguments (namespace and parameter types dropped).  Its body hash covers the instructions between its
label and its end label, with comments dropped, local label numbers and the kernel's own mangled name normalised.  The scan
for the scalar-store family of instructions covers the whole assembly of every TU.  Exit status 1 when two trees differ."""
import hashlib
import os
import re
import runpy
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

PKG = "spotify_recsys_challenge_2018_amd"
FIGURES = ("vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size",
           "vgpr_spill_count", "sgpr_spill_count")
# any scalar-unit instruction that writes memory: a scalar mnemonic with store / atomic in it, or a scalar cache write-back
SCALAR_WRITES = re.compile(r"^\s*s_\w*(?:store|atomic|dcache_(?:wb|discard))", re.M)


def kernel_key(demangled):
    s = demangled.replace("(anonymous namespace)::", "")
    s = s[5:] if s.startswith("void ") else s
    depth = 0
    for i, ch in enumerate(s):
        depth += (ch == "<") - (ch == ">")
        if ch == "(" and depth == 0:
            return s[:i]
    return s


def tree_kernels(tree):
    b = runpy.run_path(os.path.join(tree, PKG, "build.py"))
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        def cc(src):
            asm = os.path.join(tmp, src + ".s")
            subprocess.check_call([b["HIPCC"]] + b["FLAGS"] + ["--cuda-device-only", "-S", os.path.join(b["CSRC"], src), "-o", asm])
            return src, open(asm).read()
        with ThreadPoolExecutor(max_workers=8) as ex:
            texts = list(ex.map(cc, b["SOURCES"]))
    for src, text in texts:
        if SCALAR_WRITES.search(text):
            raise SystemExit("%s/%s: a scalar store / scalar atomic / scalar cache write-back instruction" % (tree, src))
        meta = text[text.index("amdhsa.kernels:"):text.index("amdhsa.target:")] if "amdhsa.kernels:" in text else ""
        for block in re.split(r"\n  - ", meta)[1:]:
            sym = re.search(r"\.name:\s+(\S+)", block).group(1)
            fig = {f: int(m.group(1)) if (m := re.search(r"\.%s:\s+(\d+)" % f, block)) else 0 for f in FIGURES}
            body = text[text.index("\n%s:" % sym):]
            body = body[:re.search(r"\n\.Lfunc_end\d+:", body).start()]
            body = re.sub(r"\s*;.*", "", body).replace(sym, "<self>").replace(sym[2:], "<self>")
            body = re.sub(r"\.LBB\d+_", ".LBB_", body)
            fig["body"] = hashlib.sha256(body.encode()).hexdigest()[:12]
            fig["tu"] = src
            key = kernel_key(subprocess.check_output(["c++filt", sym], text=True).strip())
            assert key not in out, key
            out[key] = fig
    return out


def show(key, f):
    return "%-62s %-18s %s  v%d a%d s%d  scratch %d  lds %d  spills %d/%d" % (
        key, f["tu"], f["body"], f["vgpr_count"], f["agpr_count"], f["sgpr_count"], f["private_segment_fixed_size"],
        f["group_segment_fixed_size"], f["vgpr_spill_count"], f["sgpr_spill_count"])


def main(argv):
    if len(argv) == 1:
        ks = tree_kernels(argv[0])
        for k in sorted(ks):
            print(show(k, ks[k]))
        print("%d kernels" % len(ks))
        return 0
    a, b = tree_kernels(argv[0]), tree_kernels(argv[1])
    for tu in sorted({f["tu"] for f in list(a.values()) + list(b.values())}):
        print("%-20s %3d -> %3d kernels" % (tu, sum(f["tu"] == tu for f in a.values()), sum(f["tu"] == tu for f in b.values())))
    only = sorted(set(a) ^ set(b))
    for k in only:
        print("only in %s: %s" % (argv[0] if k in a else argv[1], k))
    moved = sorted(k for k in set(a) & set(b) if a[k]["tu"] != b[k]["tu"])
    differ = sorted(k for k in set(a) & set(b) if {**a[k], "tu": ""} != {**b[k], "tu": ""})
    for k in differ:
        print("differs:\n  %s\n  %s" % (show(k, a[k]), show(k, b[k])))
    print("%d / %d kernels, %d in both, %d moved to another TU, %d differ in body or resources" % (
        len(a), len(b), len(set(a) & set(b)), len(moved), len(differ)))
    return 1 if only or differ else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]) if len(sys.argv) in (2, 3) else __doc__)
