#!/usr/bin/env python
"""Static resource report of the PRODUCT library's kernels (no GPU needed): every csrc/*.hip is compiled for gfx950 with
-save-temps and the code-object metadata of each kernel is tabulated — VGPRs / AGPRs / SGPRs, spills, scratch, static LDS — together
with its count of MFMA, LDS-DMA (`buffer_load ... lds`) and `ds_read_b128` instructions and a hash of its whole body (label to
`.Lfunc_end`, mangled symbols and local label numbers replaced by placeholders: equal hashes = the same instructions).  Usage:
    python tools/isa_report.py [--tools] > profiles/rNN_isa_resources.txt
    python tools/isa_report.py --compare before.txt after.txt     # same kernels per source file, whatever their names?"""
import argparse
import collections
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pantomatrix_amd", "csrc")
sys.path.insert(0, CSRC)
import build  # noqa: E402


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    return [re.sub(r"\(anonymous namespace\)::|emage_dev::", "", n).replace("void ", "") for n in out]


def body_hash(body):
    body = re.sub(r"\s*;.*", "", body)          # comments (basic-block names, which carry the names of inlined functions)
    body = re.sub(r"\.LBB\d+_\d+", ".LBB", re.sub(r"_Z\w+", "_Z", body))
    return hashlib.sha256(body.encode()).hexdigest()[:16]


def compare(before, after):
    """Two reports hold the same device code when each source file has the same multiset of (registers, spills, scratch, LDS, hash)."""
    def load(path):
        per_file = collections.defaultdict(collections.Counter)
        for line in open(path):
            f = line.split()
            if len(f) >= 13 and f[0].endswith(".hip"):
                per_file[f[0]][(*f[1:8], f[11])] += 1
        return per_file
    a, b = load(before), load(after)
    bad = 0
    for src in sorted(set(a) | set(b)):
        if a[src] != b[src]:
            bad += 1
            print(f"{src}: {sum(a[src].values())} -> {sum(b[src].values())} kernels; only before {sorted((a[src] - b[src]).elements())}; only after {sorted((b[src] - a[src]).elements())}")
    n = sum(sum(c.values()) for c in b.values())
    print(f"{n} kernels, {'identical' if not bad else f'{bad} source files differ'}")
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tools", action="store_true", help="the -DEMAGE_TOOLS build (every swept tile configuration)")
    ap.add_argument("--compare", nargs=2, metavar=("BEFORE", "AFTER"), help="compare two reports instead of compiling")
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    extra = ["-DEMAGE_TOOLS"] if args.tools else []
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        for src in build.SOURCES:
            subprocess.run([build._hipcc(), *build.FLAGS, *extra, "-save-temps", "-c", os.path.join(CSRC, src), "-o", os.path.join(tmp, src + ".o")],
                           cwd=tmp, check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
            asm = [f for f in os.listdir(tmp) if f.startswith(src.replace(".hip", "") + "-hip-amdgcn") and f.endswith(".s")]
            if not asm:
                continue
            text = open(os.path.join(tmp, asm[0])).read()
            # instruction counts and hash per kernel body: its label to its .Lfunc_end marker (an early exit has an s_endpgm of its own)
            counts = {}
            for m in re.finditer(r"^(_Z\w+):.*?\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M):
                body = m.group(2)
                counts[m.group(1)] = (len(re.findall(r"\bv_mfma_", body)), len(re.findall(r"buffer_load_dword\w* .* lds", body)), len(re.findall(r"\bds_read_b128\b", body)),
                                      body_hash(body))
            for m in re.finditer(r"- \.agpr_count:\s+(\d+).*?\.group_segment_fixed_size:\s+(\d+).*?\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+).*?\.sgpr_count:\s+(\d+).*?"
                                 r"\.sgpr_spill_count:\s+(\d+).*?\.vgpr_count:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+)", text, re.S):
                agpr, lds, name, scratch, sgpr, sspill, vgpr, vspill = m.groups()
                c = counts.get(name, (0, 0, 0, "-"))
                rows.append((src, name, int(vgpr), int(agpr), int(sgpr), int(vspill), int(sspill), int(scratch), int(lds), *c))
    names = demangle([r[1] for r in rows])
    print(f"# {'tools' if args.tools else 'product'} library, hipcc {' '.join(build.FLAGS + extra)}; {len(rows)} kernels; vgpr = arch VGPRs + AGPRs as allocated")
    print(f"{'file':14s} {'vgpr':>4s} {'agpr':>4s} {'sgpr':>4s} {'vsp':>3s} {'ssp':>3s} {'scr':>4s} {'lds(B)':>6s} {'mfma':>5s} {'dma':>4s} {'dsr128':>6s} {'body hash':16s}  kernel")
    for r, n in sorted(zip(rows, names), key=lambda t: (t[0][0], t[1])):
        print(f"{r[0]:14s} {r[2]:4d} {r[3]:4d} {r[4]:4d} {r[5]:3d} {r[6]:3d} {r[7]:4d} {r[8]:6d} {r[9]:5d} {r[10]:4d} {r[11]:6d} {r[12]:16s}  {n[:150]}")
    print(f"# kernels with spills or scratch: {sum(1 for r in rows if r[5] or r[6] or r[7])}")


if __name__ == "__main__":
    main()
