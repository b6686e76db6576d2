#!/usr/bin/env python3
"""Compare the gfx950 machine code of the kernels of two builds, symbol by symbol.

    python tools/isa_diff.py [--same 'OLD_KEY=NEW_KEY' ...] OLD_TREE NEW_TREE [OBJECT ...] [> profiles/attn_template_isa_diff.txt]

OBJECT names files of lstc_vad_amd/csrc without their suffix (gemm_f32, rowops, ...); the default is the attention files.
Each tree must have been built with `make` (the per-file objects lstc_vad_amd/csrc/OBJECT.o are read: one offload bundle
each).  Every kernel of OLD is looked up in NEW by its demangled name (key(): the two spellings of a masked instantiation count
as one, and so do an instantiation and its spelling with further template arguments `false` behind it) and its disassembly
compared as text after the addresses are stripped (instruction words and operands stay).  --same names a kernel of OLD and the
kernel of NEW that took its place under another name (both as the keys this tool prints); it is compared with that one, and a
name that matches nothing leaves its kernels MISSING / NEW.  A kernel that DIFFERS is listed with the registers, scratch bytes
and code bytes of both builds.  Exit status 1 if an OLD kernel is missing or differs, or if NEW has a kernel that OLD has not."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
FILES = ("attention", "attention_long", "attention_pk")
STATS = {}      # (tree, symbol) -> registers, scratch and code size, from the code object's metadata


def kernels(tree, name, tmp):
    d = os.path.join(tmp, f"{len(os.listdir(tmp))}_{name}")
    os.makedirs(d)
    obj = os.path.join(d, name + ".o")
    with open(os.path.join(tree, "lstc_vad_amd", "csrc", name + ".o"), "rb") as f, open(obj, "wb") as g:
        g.write(f.read())
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", obj], check=True, capture_output=True, cwd=d)   # writes <obj>.0.<target>
    co = [os.path.join(d, f) for f in os.listdir(d) if f.endswith("gfx950")][0]
    syms = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-t", co], check=True, capture_output=True, text=True).stdout
    funcs = {ln.split()[-1] for ln in syms.splitlines() if " F .text" in ln}
    dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co], check=True, capture_output=True,
                         text=True).stdout
    out, cur = {}, None
    for ln in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", ln)
        if m:
            cur = m.group(1) if m.group(1) in funcs else cur
            if m.group(1) in funcs:
                out[cur] = []
            continue
        if cur is not None and ln.strip() and ln.strip() != "...":      # "...": objdump's mark for alignment padding after a function
            out[cur].append(re.sub(r"\s*//.*$", "", ln).strip())      # drop the address comment
    size = {ln.split()[-1]: int(ln.split()[-3], 16) for ln in syms.splitlines() if " F .text" in ln}
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    for entry in re.split(r"^  - ", notes, flags=re.M)[1:]:      # one block of amdhsa.kernels per kernel
        f = dict(re.findall(r"^\s+\.(name|vgpr_count|sgpr_count|private_segment_fixed_size):\s+(\S+)$", entry, flags=re.M))
        f["name"] = f.get("name", "").strip("'")      # quoted where the mangling holds a `$`
        if f["name"] in out:
            STATS[(tree, f["name"])] = (f"{f['vgpr_count']} VGPRs, {f['sgpr_count']} SGPRs, {f['private_segment_fixed_size']} B scratch, "
                                        f"{size[f['name']]} B code")
    return out


def demangle(syms):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(syms), capture_output=True, text=True).stdout.split("\n")
    except OSError:
        out = []
    return dict(zip(syms, out)) if len(out) >= len(syms) else {s: s for s in syms}


def key(dem):
    """One name per kernel whichever way its tree spells the masked instantiation: the demangled name without the parameter list,
    with `X_masked_kernel<A>` (a twin of its own) and `X_kernel<A, true>` (a template argument MASKED, which the
    `conditional<true, MaskParams, NoMask>` in the parameter list gives away) both as `X_kernel<A> [masked]`.  Trailing template
    arguments `false` are dropped first (`X_kernel<A, false, false>` is `X_kernel<A>`): a parameter added behind the others with that
    default leaves the old instantiations their names, and one that is `true` names a kernel of its own.  Every other kernel keeps its name.
    This leans on how the mangling spells MaskArg<MASKED> (csrc/attention_common.h): as
    `std::conditional<B, MaskParams, NoMask>::type`, so both instantiations name NoMask.  Another definition of MaskArg or
    another demangler would leave the template form unrecognised: its kernels then come out MISSING / NEW, never as a false pass."""
    depth, cut = 0, len(dem)
    for i in range(len(dem) - 1, -1, -1):      # the parameter list is the last parenthesised group
        depth += (dem[i] == ")") - (dem[i] == "(")
        if depth == 0:
            cut = i
            break
    name, params = dem[:cut], dem[cut:]
    # a template parameter added behind the others with the default `false` (VAR of the attention and CLS kernels): the tree
    # without it spells the same instantiation without the trailing `, false`; a `true` stays and names a kernel of its own
    while name.endswith(", false>"):
        name = name[:-len(", false>")] + ">"
    masked = False
    which = re.search(r"conditional<(true|false), [^<>]*MaskParams", params)
    if which and which.group(1) == "true":
        m = re.match(r"^(.*), true>$", name)
        if m:
            name, masked = m.group(1) + ">", True
    elif "_masked_kernel<" in name:
        name, masked = name.replace("_masked_kernel<", "_kernel<"), True
    return name + (" [masked]" if masked else "")


def keyed(kern, tree):
    dem = demangle(sorted(kern))
    out = {}
    for sym, body in kern.items():
        k = key(dem[sym])
        assert k not in out, f"two kernels named {k}"
        out[k] = (body, STATS.get((tree, sym), "?"))
    return out


def main():
    argv, same = sys.argv[1:], {}
    while argv and argv[0] == "--same":
        o, n = argv[1].split("=", 1)
        same[o.strip()] = n.strip()
        argv = argv[2:]
    old, new = argv[0], argv[1]
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        for name in argv[2:] or FILES:
            a, b = keyed(kernels(old, name, tmp), old), keyed(kernels(new, name, tmp), new)
            print(f"== csrc/{name}.hip: {len(a)} kernels before, {len(b)} after")
            taken = set()
            for k in sorted(a):
                kb = same[k] if k not in b and same.get(k) in b else k      # the kernel that took this one's place
                as_new = f"  as {kb}" if kb != k else ""
                taken.add(kb)
                if kb not in b:
                    print(f"MISSING   {k}"); bad += 1
                elif a[k][0] != b[kb][0]:
                    print(f"DIFFERS   {k}{as_new}  ({len(a[k][0])} -> {len(b[kb][0])} instructions)\n"
                          f"            before: {a[k][1]}\n            after:  {b[kb][1]}"); bad += 1
                else:
                    print(f"identical {k}{as_new}  ({len(a[k][0])} instructions)")
            for k in sorted(set(b) - taken):
                print(f"NEW       {k}  ({len(b[k][0])} instructions)"); bad += 1
    print(f"== {bad} kernel(s) missing, changed or without a counterpart in the old tree")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
