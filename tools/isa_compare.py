#!/usr/bin/env python3
"""Are the slicing kernels a build launches with its newest option off the kernels of another build (the parent commit's)?

Two gfx950 assembly listings of csrc/am_kernels.hip, made with the Makefile's flags plus `--cuda-device-only -S`:
    python tools/isa_compare.py parent.s this.s
Every kernel whose name contains "slice" is compared as its instruction stream AND its kernel descriptor (.amdhsa_* block:
registers, LDS, scratch, kernarg size), comments stripped, basic-block labels renumbered per function and the kernel's own
mangled name replaced by a placeholder.  A kernel `name<..., 0>` of the second listing is matched with `name<...>` of the
first: the last template argument, = 0, is the only difference in the name (FIX when the repair was added, GATE when the
address gate was: `am_k_extract_slice_iq<32, 1, 0>` is matched with `am_k_extract_slice_iq<32, 1>`).  Exit status 1 if any pair differs.

    python tools/isa_compare.py --same-names parent.s this.s
is for a commit that adds a VALUE of an existing template argument instead (GATE = 2 for am_set_address_repair): every kernel
whose name contains "slice" or "gate" and which the first listing has under the same name is compared with that one; the others
are listed as new.

    python tools/isa_compare.py --pattern 'am_k_fe3|am_k_refine_seg' parent.s this.s
chooses the kernels by a regular expression on the mangled name instead of "slice" (either mode; listings of other files than
am_kernels.hip are made the same way).  The template arguments in front of the new last one may be numbers or true / false
(`am_k_refine_seg<true, 0>` is matched with `am_k_refine_seg<true>`, `am_k_fe3<0>` with `am_k_fe3`)."""
import re
import subprocess
import sys


def kernels(path):
    txt = open(path).read()
    out = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", txt, re.S | re.M):
        name, body = m.group(1), m.group(2)
        lines = [re.sub(r"\s*;.*$", "", ln) for ln in body.split("\n")]
        lines = [re.sub(r"\.LBB\d+_", ".LBB_", ln).replace(name, "<self>") for ln in lines if ln.strip()]
        # (where the code goes: a template's own comdat section, a plain function's .text)
        lines = [ln for ln in lines if ln.strip() != ".text" and not ln.strip().startswith(".section")]
        info = {}
        for key in ("num_vgpr", "numbered_sgpr", "private_seg_size"):
            mm = re.search(r"\.set " + re.escape(name) + r"\." + key + r", (\S+)", txt)
            info[key] = mm.group(1) if mm else "?"
        mm = re.search(r"\.amdhsa_kernel " + re.escape(name) + r"\n(.*?)\.end_amdhsa_kernel", txt, re.S)
        if mm:
            info["lds"] = re.search(r"\.amdhsa_group_segment_fixed_size (\S+)", mm.group(1)).group(1)
        at = txt.find(".size\t" + name)
        mm = re.search(r"; Occupancy: (\d+)", txt[at:at + 3000]) if at >= 0 else None
        info["waves_per_simd"] = mm.group(1) if mm else "?"
        out[name] = (lines, info)
    return out


def demangle(names):
    res = subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True).stdout.split("\n")
    return {n: d.split("(")[0].replace("void ", "") for n, d in zip(names, res)}


def same_names(a, b, wanted):
    na, nb = demangle([k for k in a]), demangle([k for k in b if wanted(k)])
    first = {d: k for k, d in na.items()}
    worst = 0
    for k, d in sorted(nb.items(), key=lambda kv: kv[1]):
        lines, info = b[k]
        text = "%-36s %5d lines  %s" % (d, len(lines), " ".join("%s=%s" % kv for kv in info.items()))
        if d in first:
            same = a[first[d]][0] == lines and a[first[d]][1] == info
            text += "   == the first listing's: %s" % ("IDENTICAL" if same else "DIFFERENT")
            worst |= not same
        else:
            text += "   new"
        print(text)
    sys.exit(int(worst))


def main():
    args = sys.argv[1:]
    pattern = None
    if "--pattern" in args:
        at = args.index("--pattern")
        pattern = re.compile(args[at + 1])
        del args[at:at + 2]
    if args[0] == "--same-names":
        same_names(kernels(args[1]), kernels(args[2]), (lambda k: pattern.search(k)) if pattern else (lambda k: "slice" in k or "gate" in k))
    wanted = (lambda k: pattern.search(k)) if pattern else (lambda k: "slice" in k)
    a, b = kernels(args[0]), kernels(args[1])
    na, nb = demangle([k for k in a if wanted(k)]), demangle([k for k in b if wanted(k)])
    first = {d: k for k, d in na.items()}
    worst = 0
    for k, d in sorted(nb.items(), key=lambda kv: kv[1]):
        lines, info = b[k]
        text = "%-36s %5d lines  %s" % (d, len(lines), " ".join("%s=%s" % kv for kv in info.items()))
        m = re.match(r"(\w+)<((?:\w+, )*)0>$", d)
        if m:
            old = m.group(1) + ("<%s>" % m.group(2)[:-2] if m.group(2) else "")
            same = old in first and a[first[old]][0] == lines and a[first[old]][1] == info
            text += "   == %s of the first listing: %s" % (old, "IDENTICAL" if same else "DIFFERENT")
            worst |= not same
        print(text)
    sys.exit(int(worst))


if __name__ == "__main__":
    main()
