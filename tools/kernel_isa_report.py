#!/usr/bin/env python3
"""Static figures of every kernel of one .hip source, from the gfx950 assembly the library's own flags give (a .s file is
taken as it is): instructions, VGPRs / SGPRs (next_free_*), scratch and LDS bytes, the counts of global_load* / global_store* /
s_waitcnt vmcnt, the wavefronts per SIMD the VGPR count allows (min(8, 512 / roundup8(vgpr))), and a digest of the
instruction stream with its basic-block labels renumbered -- two builds of a kernel with the same digest are the same code.
With --against OLD the figures of OLD (a .hip or .s of another tree) stand beside them, one line per kernel that differs.
Usage: kernel_isa_report.py FILE [--against OLD] [--only SUBSTRING]"""
import argparse
import hashlib
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from openjph_amd.build import FLAGS, HIPCC  # noqa: E402

KEYS = ["instr", "vgpr", "sgpr", "scratch", "lds", "gload", "gstore", "vmcnt", "waves"]
FIELDS = {"next_free_vgpr": "vgpr", "next_free_sgpr": "sgpr", "private_segment_fixed_size": "scratch", "group_segment_fixed_size": "lds"}


def assembly(path):
    if path.endswith(".s"):
        return open(path).read()
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        subprocess.check_call([HIPCC, "-x", "hip"] + FLAGS + ["--cuda-device-only", "-S", path, "-o", out], stderr=subprocess.DEVNULL)
        return open(out).read()


def demangled(names):
    for tool in ("/opt/rocm/llvm/bin/llvm-cxxfilt", "c++filt"):
        try:
            out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
            return [re.sub(r"\(.*$", "", re.sub(r"^void ", "", o.replace("(anonymous namespace)::", ""))) for o in out]
        except (OSError, subprocess.CalledProcessError):
            continue
    return list(names)


def kernels(text):
    """{mangled name: figures} of every .amdhsa_kernel of the assembly"""
    lines = text.splitlines()
    body = {}                                            # function label -> its instruction lines
    name = None
    for l in lines:
        m = re.match(r"^([A-Za-z_][\w$.]*):", l)
        if m and not m.group(1).startswith(".L"):
            name = m.group(1); body[name] = []
            continue
        t = l.split(";")[0].strip()
        if t.startswith(".Lfunc_end"):
            name = None
        if name is None or not t or t.startswith("."):
            if name is not None and re.match(r"^\.LBB\d+_\d+:", t):
                body[name].append(t)
            continue
        body[name].append(t)
    res = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, re.S):
        k = {v: 0 for v in KEYS}
        for f, key in FIELDS.items():
            k[key] = int(re.search(r"\.amdhsa_%s (\d+)" % f, m.group(2)).group(1))
        labels, stream = {}, []
        for t in body.get(m.group(1), []):
            t = re.sub(r"\.LBB\d+_\d+", lambda x: labels.setdefault(x.group(0), "L%d" % len(labels)), t)
            stream.append(t)
            if t.endswith(":"):
                continue
            k["instr"] += 1
            k["gload"] += t.startswith("global_load"); k["gstore"] += t.startswith("global_store")
            k["vmcnt"] += t.startswith("s_waitcnt") and "vmcnt" in t
        k["waves"] = min(8, 512 // ((k["vgpr"] + 7) // 8 * 8)) if k["vgpr"] else 8
        k["digest"] = hashlib.sha256("\n".join(stream).encode()).hexdigest()[:12]
        res[m.group(1)] = k
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("file")
    ap.add_argument("--against")
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    new = kernels(assembly(a.file))
    names = sorted(n for n in new if a.only in n)
    shown = dict(zip(names, demangled(names)))
    head = "".join("%8s" % k for k in KEYS) + "  %-12s  kernel" % "digest"
    if not a.against:
        print(head)
        for n in names:
            print("".join("%8d" % new[n][k] for k in KEYS) + "  %-12s  %s" % (new[n]["digest"], shown[n]))
        return
    old = kernels(assembly(a.against))
    same = [n for n in names if n in old and old[n]["digest"] == new[n]["digest"]]
    print("%d kernels, %d with the instruction stream of %s; the others (old line, new line):" % (len(names), len(same), a.against))
    print(head)
    for n in names:
        if n in same:
            continue
        if n in old:
            print("".join("%8d" % old[n][k] for k in KEYS) + "  %-12s  %s" % (old[n]["digest"], shown[n]))
        print("".join("%8d" % new[n][k] for k in KEYS) + "  %-12s  %s%s" % (new[n]["digest"], shown[n], "" if n in old else "   (new)"))
    for n in sorted(set(old) - set(new)):
        if a.only in n:
            print("gone: %s" % n)


if __name__ == "__main__":
    main()
