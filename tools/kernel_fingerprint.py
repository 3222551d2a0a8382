#!/usr/bin/env python3
"""Fingerprint of every kernel's device code, to show that a change left it alone (no GPU needed).

    python tools/kernel_fingerprint.py path/to/csrc > tree.txt       # one line per kernel symbol
    python tools/kernel_fingerprint.py parent.txt tree.txt           # what differs between two listings

Every csrc/*.hip is cross-compiled to device assembly with the Makefile's flags (tools/isa_waits.py: product_flags, device_asm).
A kernel's text runs from its label to the end of its .amdhsa_kernel descriptor; the __hip_cuid_ lines are dropped and the
per-function number of the basic-block labels (.LBBn_, "Header=BBn_", .Lfunc_endn: n counts the functions in front of the kernel
in its module) is normalised, then sha256.  A listing line is
    sha256/16  VGPRs AGPRs SGPRs  scratch bytes  LDS bytes  lines hashed  file  symbol
and two listings are compared per symbol on everything but the file, so a kernel may move between files."""
import glob, hashlib, os, re, sys
from concurrent.futures import ThreadPoolExecutor

from isa_waits import device_asm

META = ("vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")


def fingerprints(csrc, name):
    """[(symbol, listing line without the symbol)] of the kernels of csrc/name."""
    text = device_asm(name, csrc=csrc)
    meta = {}                                   # symbol -> the resource fields of its amdgpu_metadata entry
    for entry in re.split(r"\n  - (?=\.)", "\n".join(text)):
        m = re.search(r"^\s*\.name:\s*(\S+)$", entry, re.M)
        if m and ".vgpr_count:" in entry:
            meta[m.group(1)] = [re.search(r"\.%s:\s*(\d+)" % k, entry).group(1) for k in META]
    out = []
    for sym in meta:
        start = next(i for i, l in enumerate(text) if l.startswith(sym + ":"))
        body = text[start:text.index("\t.end_amdhsa_kernel", text.index("\t.amdhsa_kernel " + sym)) + 1]
        body = [re.sub(r"((?:\.L|\b)BB|\.Lfunc_(?:begin|end))\d+", r"\1", l) for l in body if "__hip_cuid_" not in l]
        body = [re.sub(r"\s+", " ", l) if l.startswith(".LBB") else l for l in body]       # (a label's comment is padded to a column)
        sha = hashlib.sha256("\n".join(body).encode()).hexdigest()[:16]
        out.append((sym, "%s %5s %5s %5s %7s %6s %6d  %-16s" % ((sha,) + tuple(meta[sym]) + (len(body), name))))
    return out


def listing(csrc):
    files = sorted(os.path.basename(f) for f in glob.glob(os.path.join(csrc, "*.hip")))
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        for res in ex.map(lambda f: fingerprints(csrc, f), files):
            for sym, line in sorted(res):
                print(line, sym)


def read(path):
    """{symbol: [fingerprint without the file]}, {file: kernels}"""
    syms, files = {}, {}
    for l in open(path).read().splitlines():
        f = l.split()
        syms.setdefault(f[8], []).append(" ".join(f[:7]))
        files[f[7]] = files.get(f[7], 0) + 1
    return syms, files


def compare(a, b):
    (sa, fa), (sb, fb) = read(a), read(b)
    print("kernels per file %12s %6s" % ("first", "second"))
    for f in sorted(set(fa) | set(fb)):
        print("  %-24s %6s %6s" % (f, fa.get(f, "-"), fb.get(f, "-")))
    print("  %-24s %6d %6d" % ("total", sum(fa.values()), sum(fb.values())))
    for s in sorted(set(sa) - set(sb)):
        print("only in the first: ", s)
    for s in sorted(set(sb) - set(sa)):
        print("only in the second:", s)
    both = sorted(set(sa) & set(sb))
    differ = [s for s in both if sorted(sa[s]) != sorted(sb[s])]
    for s in differ:
        print("differs: %s\n    %s\n    %s" % (s, " | ".join(sa[s]), " | ".join(sb[s])))
    print("kernels whose instruction stream or resource line differs: %d of %d in both listings" % (len(differ), len(both)))
    return 1 if differ else 0


if __name__ == "__main__":
    if len(sys.argv) == 2 and os.path.isdir(sys.argv[1]):
        listing(os.path.abspath(sys.argv[1]))
    elif len(sys.argv) == 3:
        sys.exit(compare(sys.argv[1], sys.argv[2]))
    else:
        sys.exit(__doc__)
