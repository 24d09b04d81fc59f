"""Device assembly of every kernel of csrc/*.hip at a parent revision against the working tree, kernel by kernel; no GPU.

Both sides are compiled with _build.py's flags (FILE_FLAGS included) plus ``--cuda-device-only -S``; the parent's csrc/ comes
out of ``git show`` into a temporary directory.  Comments, ``.ident`` and ``.file`` lines are dropped and the numbering of
local labels (the function's position in its file) is neutralised; what is compared per kernel symbol is its code and its
kernel descriptor, as text.  A kernel whose name changed on purpose is matched with ``--alias PARENT_TEXT=NEW_TEXT``
(substrings of the mangled name; repeatable).  How code is moved between files with this: move it, run the tool, and keep
the move only where every kernel that includes it reads "identical" (or its difference is accounted for in the report).

    python tools/isa_diff.py --parent HEAD [--alias OLD=NEW] [--only conv.hip,bn.hip] [--out profiles/helper_share_isa.txt]

The exit status is 1 when a kernel differs or exists on one side only.
"""
import argparse
import concurrent.futures
import importlib.util
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "cova-web-object-detection_amd"
spec = importlib.util.spec_from_file_location("_cova_build", os.path.join(ROOT, PKG, "_build.py"))
B = importlib.util.module_from_spec(spec)
spec.loader.exec_module(B)

ap = argparse.ArgumentParser()
ap.add_argument("--parent", required=True, help="git revision to compare the working tree with")
ap.add_argument("--alias", action="append", default=[], help="PARENT_TEXT=NEW_TEXT: a rename to apply to the parent's assembly")
ap.add_argument("--only", help="comma-separated file names (default: every csrc/*.hip)")
ap.add_argument("--out", help="also write the report to this file")
args = ap.parse_args()
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FIGURES = (("vgpr", ".amdhsa_next_free_vgpr"), ("sgpr", ".amdhsa_next_free_sgpr"),
           ("scratch", ".amdhsa_private_segment_fixed_size"), ("lds", ".amdhsa_group_segment_fixed_size"))


def assembly(src):
    """the device assembly of one file, or None when the file does not exist on that side"""
    if not os.path.exists(src):
        return None
    cmd = [HIPCC] + B.flags(src) + ["-w", "--cuda-device-only", "-S", src, "-o", "-"]
    return subprocess.run(cmd, check=True, stdout=subprocess.PIPE, text=True).stdout


def kernels(text):
    """kernel symbol -> (code and descriptor as normalised text, instruction count, descriptor figures)"""
    lines = []
    for ln in text.splitlines():
        ln = ln.split(";")[0].rstrip()
        if ln.strip() and not re.match(r"\s*\.(ident|file)\b", ln):
            lines.append(re.sub(r"\.L(BB|func_(?:begin|end)|tmp|JTI)\d+", r".L\1", ln))
    res = {}
    for i, ln in enumerate(lines):
        m = re.match(r"\s*\.amdhsa_kernel (\S+)", ln)
        if not m:
            continue
        sym = m.group(1)
        desc = lines[i:lines.index("\t.end_amdhsa_kernel", i) + 1]
        b0 = lines.index(sym + ":")
        code = lines[b0:next(j for j in range(b0, len(lines)) if lines[j].startswith("\t.size\t" + sym + ","))]
        n_ins = sum(1 for c in code if c.startswith("\t") and not c.startswith("\t."))
        fig = {k: next(d.split()[-1] for d in desc if d.split()[0] == key) for k, key in FIGURES}
        res[sym] = ("\n".join(code + desc), n_ins, fig)
    return res


def show(k):
    return "%d instructions, " % k[1] + ", ".join("%s %s" % (n, k[2][n]) for n, _ in FIGURES)


def main():
    names = args.only.split(",") if args.only else [os.path.basename(s) for s in B.SOURCES]
    rel = PKG + "/csrc/"
    out = ["Device assembly (gfx950, _build.py's flags, --cuda-device-only -S) of every kernel of csrc/*.hip: revision %s against"
           % subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", args.parent], text=True).strip(),
           "the tree that holds this file (tools/isa_diff.py).  Compared per kernel symbol: its code and its kernel descriptor."]
    with tempfile.TemporaryDirectory() as tmp:
        for path in subprocess.check_output(["git", "-C", ROOT, "ls-tree", "--name-only", args.parent, rel, "include/"],
                                            text=True).split():
            os.makedirs(os.path.dirname(os.path.join(tmp, path)), exist_ok=True)
            with open(os.path.join(tmp, path), "wb") as fh:
                fh.write(subprocess.check_output(["git", "-C", ROOT, "show", "%s:%s" % (args.parent, path)]))
        srcs = [os.path.join(d, "csrc", n) for n in names for d in (os.path.join(tmp, PKG), os.path.join(ROOT, PKG))]
        with concurrent.futures.ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as pool:
            asm = list(pool.map(assembly, srcs))
    syms = [s for a in asm if a for s in kernels(a)]
    plain = {}
    if shutil.which("c++filt"):                                          # readable names; the mangled ones serve without it
        plain = dict(zip(syms, subprocess.run(["c++filt"], input="\n".join(syms), stdout=subprocess.PIPE, text=True,
                                              check=True).stdout.splitlines()))
    bad = total = 0
    for n, (old, new) in zip(names, zip(asm[0::2], asm[1::2])):
        for a in args.alias:
            old = old and old.replace(*a.split("=", 1))
        ko, kn = kernels(old or ""), kernels(new or "")
        same = sum(1 for s in kn if s in ko and ko[s][0] == kn[s][0])
        total += len(kn)
        out += ["", "%s: %d kernels, %d identical" % (n, len(kn), same)]
        for s in sorted(set(ko) | set(kn), key=lambda s: plain.get(s, s)):
            name = plain.get(s, s).replace("(anonymous namespace)::", "").split("(")[0]
            if s in ko and s in kn and ko[s][0] == kn[s][0]:
                out.append("  identical  " + name)
                continue
            bad += 1
            out.append("  %-9s  %s" % ("DIFFERENT" if s in ko and s in kn else "PARENT ONLY" if s in ko else "NEW ONLY", name))
            out += ["      %-6s %s" % (w, show(k[s])) for w, k in (("parent", ko), ("new", kn)) if s in k]
    out += ["", "%d kernels in the tree; %d differ or exist on one side only" % (total, bad)]
    print("\n".join(out))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(out) + "\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
