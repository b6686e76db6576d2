#!/usr/bin/env python3
"""Compare the gfx950 machine code of the attention kernels of two builds, symbol by symbol.

    python tools/attn_isa_diff.py OLD_TREE NEW_TREE [> profiles/attn_mask_isa_diff.txt]

Each tree must have been built with `make` (the per-file objects lstc_vad_amd/csrc/attention*.o are read: one offload bundle
each).  Every kernel symbol of OLD is looked up in NEW and its disassembly compared as text after the addresses are stripped
(instruction words and operands stay).  Kernels only NEW has are listed, not compared.  Exit status 1 if an OLD kernel is missing
or differs."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
FILES = ("attention", "attention_long", "attention_pk")


def kernels(tree, name, tmp):
    d = os.path.join(tmp, f"{abs(hash(tree))}_{name}")
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
    return out


def demangle(s):
    try:
        return subprocess.run(["c++filt", s], capture_output=True, text=True).stdout.strip() or s
    except OSError:
        return s


def main():
    old, new = sys.argv[1], sys.argv[2]
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        for name in FILES:
            a, b = kernels(old, name, tmp), kernels(new, name, tmp)
            print(f"== csrc/{name}.hip: {len(a)} kernels before, {len(b)} after")
            for k in sorted(a):
                if k not in b:
                    print(f"MISSING   {demangle(k)}"); bad += 1
                elif a[k] != b[k]:
                    print(f"DIFFERS   {demangle(k)}  ({len(a[k])} -> {len(b[k])} instructions)"); bad += 1
                else:
                    print(f"identical {demangle(k)}  ({len(a[k])} instructions)")
            for k in sorted(set(b) - set(a)):
                print(f"new       {demangle(k)}  ({len(b[k])} instructions)")
    print(f"== {bad} pre-existing attention kernel(s) missing or changed")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
