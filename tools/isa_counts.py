#!/usr/bin/env python3
"""What the compiler made of the tensor-product walks (no GPU needed):
    python tools/isa_counts.py [--csrc DIR] [--out FILE] [--kernel REGEX ...]
Compiles e3k_tp.hip, e3k_tp_scalar.hip and e3k_tp_masked.hip of DIR (default: this tree's csrc) to gfx950 assembly with the
Makefile's CXXFLAGS plus `--cuda-device-only -S`, and prints per kernel
  - from the kernel's metadata: .sgpr_count, .vgpr_count, .sgpr_spill_count, .vgpr_spill_count, scratch bytes per lane;
  - over the whole kernel and over its largest loop: the counts of global_load, buffer_load, s_load, v_readfirstlane, v_readlane,
    v_writelane, s_nop, `s_waitcnt vmcnt` and of vector (v_*) instructions.
"Largest loop" = among the loops the compiler marks (label to the last branch back to it) the one with the most v_* instructions:
in these kernels that is the edge loop of the highest input degree the kernel carries (l1 = 2 for the l_max 2 instantiations)."""
import argparse, collections, os, re, shlex, shutil, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRCS = ["e3k_tp.hip", "e3k_tp_scalar.hip", "e3k_tp_masked.hip"]
KERNELS = [r"tp_bwd_x_kernel<2, 2, false, true, 5>", r"tp_bwd_x_kernel<2, 2, false, true, 4>", r"tp_bwd_x_kernel<0, 3, false, true, 5>",
           r"tp_bwd_xw_masked_kernel", r"tp_bwd_xw_scalar_kernel", r"tp_fwd_kernel<2, 2, false, true, 4>"]
COUNTS = [("global_load", r"global_load"), ("buffer_load", r"buffer_load"), ("s_load", r"s_load"), ("v_readfirstlane", r"v_readfirstlane"),
          ("v_readlane", r"v_readlane"), ("v_writelane", r"v_writelane"), ("s_nop", r"s_nop"), ("waitcnt_vmcnt", r"s_waitcnt .*vmcnt"),
          ("vector", r"v_")]


def makefile_var(csrc, name):
    for line in open(os.path.join(csrc, "Makefile")):
        m = re.match(rf"{name}\s*\??=\s*(.*)", line)
        if m:
            return m.group(1).strip()
    raise SystemExit(f"no {name} in the Makefile")


def count(lines):
    c = collections.OrderedDict((k, 0) for k, _ in COUNTS)
    for l in lines:
        for k, pat in COUNTS:
            if re.match(pat, l):
                c[k] += 1
    return c


def largest_loop(body):
    """body: (label or None, instruction) pairs.  Returns the instructions of the loop with the most v_* instructions."""
    pos = {lab: i for i, (lab, hdr) in enumerate(body) if lab and hdr}      # the labels the compiler marks as loop headers
    last = {}
    for i, (lab, ins) in enumerate(body):
        m = re.match(r"s_c?branch\w*\s+(\S+)", "" if lab else ins)
        if m and m.group(1) in pos and pos[m.group(1)] <= i:
            last[m.group(1)] = i
    best, best_n = [], -1
    for a, b in ((pos[lab], i) for lab, i in last.items()):
        ins = [x for lab, x in body[a:b + 1] if lab is None]
        n = sum(1 for x in ins if x.startswith("v_"))
        if n > best_n:
            best, best_n = ins, n
    return best


def kernels_of(asm):
    """name -> (body, metadata dict) for every kernel of one assembly file"""
    text = open(asm).read()
    meta = {}
    for blk in re.split(r"\n  - \.agpr_count", text)[1:]:
        m = re.search(r"\.name:\s+(\S+)", blk)
        if not m:
            continue
        d = {k: int(v) for k, v in re.findall(r"\.(sgpr_count|vgpr_count|sgpr_spill_count|vgpr_spill_count|private_segment_fixed_size):\s+(\d+)", blk)}
        meta[m.group(1)] = d
    out = {}
    lines = text.splitlines()
    i = 0
    while i < len(lines):
        m = re.match(r"(\w+):\s*(;.*)?$", lines[i])
        if m and m.group(1) in meta:
            body, lab = [], None
            i += 1
            while i < len(lines):
                s = lines[i].split(";")[0].strip()
                lm = re.match(r"(\.LBB\w+):", s)
                if lm:
                    body.append((lm.group(1), "Loop Header" in lines[i]))
                elif s and not s.startswith("."):
                    body.append((None, s))
                    if s.startswith("s_endpgm") and re.match(r"\s*\.section|\s*\.p2align|\.Lfunc_end", lines[i + 1] if i + 1 < len(lines) else ".section"):
                        break
                elif s.startswith(".Lfunc_end"):
                    break
                i += 1
            out[m.group(1)] = (body, meta[m.group(1)])
        i += 1
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--csrc", default=os.path.join(ROOT, "equivariant-nn-zoo_amd", "csrc"))
    ap.add_argument("--out")
    ap.add_argument("--kernel", action="append", help="regex on the demangled name (default: the walks of the l_max 2 step)")
    ap.add_argument("--asm", help="keep the assembly files in this directory, and reuse those already there")
    ap.add_argument("--flags", default="", help="extra compiler flags")
    a = ap.parse_args()
    hipcc = os.environ.get("HIPCC", makefile_var(a.csrc, "HIPCC"))
    flags = shlex.split(makefile_var(a.csrc, "CXXFLAGS").replace("$(ARCH)", "gfx950")) + shlex.split(a.flags)
    filt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not filt:
        raise SystemExit("needs llvm-cxxfilt or c++filt on PATH")
    found = {}
    with tempfile.TemporaryDirectory() as tmp:
        tmp = a.asm or tmp
        os.makedirs(tmp, exist_ok=True)
        for src in SRCS:
            asm = os.path.join(tmp, src + ".s")
            if not (a.asm and os.path.exists(asm)):
                subprocess.run([hipcc] + flags + ["--cuda-device-only", "-S", os.path.join(a.csrc, src), "-o", asm], check=True)
            ks = kernels_of(asm)
            names = list(ks)
            dem = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
            for n, d in zip(names, dem):
                found[d] = ks[n]
    out = open(a.out, "w") if a.out else sys.stdout
    print(f"# {os.path.basename(hipcc)} {' '.join(flags)} --cuda-device-only -S; whole kernel / largest loop (the edge loop of the kernel's", file=out)
    print("# highest input degree).  Compile-time facts, not timings.", file=out)
    for pat in a.kernel or [re.escape(k) for k in KERNELS]:
        hits = [d for d in found if re.search(pat, d)]
        if not hits:
            print(f"## {pat}: no such kernel", file=out)
        for d in hits:
            body, meta = found[d]
            name = re.sub(r"\(.*", "", d.replace("void ", "").replace("e3k::", ""))
            print(f"## {name}", file=out)
            print("   " + "  ".join(f".{k} {meta.get(k, 0)}" for k in ("sgpr_count", "vgpr_count", "sgpr_spill_count", "vgpr_spill_count"))
                  + f"  scratch {meta.get('private_segment_fixed_size', 0)}", file=out)
            whole, loop = count([x for lab, x in body if lab is None]), count(largest_loop(body))
            for k in whole:
                print(f"   {k:16s} kernel {whole[k]:5d}   loop {loop[k]:5d}", file=out)


if __name__ == "__main__":
    main()
