#!/usr/bin/env python3
"""Static instruction accounting of one gfx950 kernel (no GPU).

  isa_count.py SYMBOL FILE [--split MNEMONIC ...] [--mnemonics] [--front]

FILE is the assembly of `hipcc -S --cuda-device-only` or a built library
(libairscmp.so: its gfx950 code objects are disassembled with llvm-objdump).
Prints, for the kernel SYMBOL:
  * the code-object metadata (VGPRs, SGPRs, spills, LDS, scratch);
  * the instruction counts by class between consecutive barriers, in text
    order (region 0 is the code before the first s_barrier);
  * the same per basic block (a block starts at a label).
The class of an instruction is its mnemonic's prefix and nothing else:
  valu    v_*
  salu    s_*      (scalar ALU, scalar loads, branches, waits, barriers)
  lds     ds_*
  vmem    global_* buffer_* flat_*
  other   anything else
--split MNEMONIC makes every instruction of that name a region boundary
beside the barriers (the Rice kernel's packer starts at its one s_setprio);
--mnemonics adds a histogram of every mnemonic per region.
--front prints instead the instructions between the kernel's entry and its
first vector-memory load (global_load_* / buffer_load_* / flat_load_*), in text
order with their operands, and their counts: the chain a wave walks before its
first request to memory leaves the CU.

The counts are static: a block inside a loop or behind a branch counts once.
They say where the instructions are, not how often they issue; the dynamic
figures are the profiler's (profiles/*pmc_summary*.json)."""
import argparse
import collections
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = ("valu", "salu", "lds", "vmem", "other")
META_KEYS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count",
             ".group_segment_fixed_size", ".private_segment_fixed_size", ".wavefront_size", ".max_flat_workgroup_size")


def classify(mnemonic):
    if mnemonic.startswith("v_"):
        return "valu"
    if mnemonic.startswith("s_"):
        return "salu"
    if mnemonic.startswith("ds_"):
        return "lds"
    if mnemonic.startswith(("global_", "buffer_", "flat_")):
        return "vmem"
    return "other"


def asm_kernel(text, sym):
    """(label or None, mnemonic, instruction text) in text order, from compiler assembly."""
    lines = text.splitlines()
    try:
        start = next(i for i, ln in enumerate(lines) if ln.startswith(sym + ":"))
    except StopIteration:
        sys.exit(f"{sym}: no such symbol in the assembly")
    out = []
    for ln in lines[start + 1:]:
        s = ln.split(";")[0].split("//")[0].strip()
        if not s:
            continue
        if s.startswith(".Lfunc_end") or s.startswith(".section") or s.startswith(".amdhsa_kernel"):
            break
        m = re.match(r"^([.\w$]+):$", s)
        if m:
            out.append((m.group(1), None, None))
        elif not s.startswith("."):
            out.append((None, s.split()[0], " ".join(s.split())))
    return out


def asm_meta(text, sym):
    m = re.search(r"^amdhsa\.kernels:\n(.*?)^amdhsa\.", text, re.S | re.M)
    if not m:
        return {}
    for item in re.split(r"^  - ", m.group(1), flags=re.M):
        if re.search(r"^\s*\.name:\s+" + re.escape(sym) + r"\s*$", item, re.M):
            meta = {}
            for k in META_KEYS:
                v = re.search(r"^\s*" + re.escape(k) + r":\s+(\S+)", item, re.M)
                if v:
                    meta[k] = int(v.group(1), 0)
            return meta
    return {}


def lib_kernel(path, sym):
    """The same from a built library: its gfx950 code objects, disassembled."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import kernel_meta
    objdump = shutil.which("llvm-objdump") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin",
                                                           "llvm-objdump")
    meta = kernel_meta.kernels(path).get(sym)
    if meta is None:
        sys.exit(f"{sym}: no such kernel in {path}")
    with open(path, "rb") as f:
        blob = f.read()
    for co in kernel_meta._code_objects(blob):
        with tempfile.NamedTemporaryFile(suffix=".co") as tmp:
            tmp.write(co)
            tmp.flush()
            dis = subprocess.run([objdump, "-d", "--symbolize-operands", "--no-show-raw-insn", tmp.name],
                                 check=True, capture_output=True, text=True).stdout
        lines = dis.splitlines()
        start = [i for i, ln in enumerate(lines) if re.match(r"^[0-9a-f]+ <" + re.escape(sym) + r">:$", ln)]
        if not start:
            continue
        out = []
        for ln in lines[start[0] + 1:]:
            s = ln.split("//")[0].strip()
            if not s:
                continue
            m = re.match(r"^(?:[0-9a-f]+ )?<(L\d+)>:$", s)  # a branch target of --symbolize-operands
            if m:
                out.append((m.group(1), None, None))
            elif re.match(r"^[0-9a-f]+ <[^>]+>:$", s):  # the next symbol
                break
            else:
                out.append((None, s.split()[0], " ".join(s.split())))
        return out, {k: meta[k] for k in META_KEYS if k in meta}
    sys.exit(f"{sym}: metadata present, code not found in {path}")


def table(rows, head):
    w = max([len(head)] + [len(r[0]) for r in rows])
    print(f"{head:<{w}} " + " ".join(f"{c:>6}" for c in CLASSES) + f" {'total':>6}")
    for name, cnt in rows:
        print(f"{name:<{w}} " + " ".join(f"{cnt[c]:>6}" for c in CLASSES) + f" {sum(cnt.values()):>6}")


def is_vmem_load(mn):
    return mn.startswith(("global_load", "buffer_load", "flat_load"))


def front(stream):
    """The text between the entry and the first vector-memory load."""
    cnt = collections.Counter()
    print("\nentry .. first vector-memory load (text order)")
    for label, mn, text in stream:
        if label is not None:
            print(f"{label}:")
            continue
        print(f"  {text}")
        if is_vmem_load(mn):
            break
        cnt[mn] += 1
    else:
        print("  (no vector-memory load)")
    print(f"\ninstructions before it: {sum(cnt.values())}")
    for key, name in (("s_load", "scalar loads"), ("s_waitcnt", "s_waitcnt"), ("v_rcp_iflag_f32", "v_rcp_iflag_f32"),
                      ("s_mul_hi_u32", "s_mul_hi_u32")):
        print(f"  {name:<16} {sum(n for m, n in cnt.items() if m.startswith(key))}")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("symbol")
    ap.add_argument("file")
    ap.add_argument("--split", action="append", default=[], metavar="MNEMONIC",
                    help="a further region boundary beside s_barrier")
    ap.add_argument("--mnemonics", action="store_true", help="histogram of every mnemonic per region")
    ap.add_argument("--front", action="store_true",
                    help="list the instructions from the entry to the first vector-memory load")
    a = ap.parse_args()
    with open(a.file, "rb") as f:
        is_elf = f.read(4) == b"\x7fELF"
    if is_elf:
        stream, meta = lib_kernel(a.file, a.symbol)
    else:
        with open(a.file) as f:
            text = f.read()
        stream, meta = asm_kernel(text, a.symbol), asm_meta(text, a.symbol)

    print(f"kernel {a.symbol}")
    print(f"source {'library' if is_elf else 'assembly'} {os.path.basename(a.file)}")
    for k in META_KEYS:
        if k in meta:
            print(f"  {k[1:]:<28} {meta[k]}")

    if a.front:
        front(stream)
        return

    regions = [collections.Counter()]
    marks = ["entry"]  # what opens each region
    nbar = 0
    hist = [collections.Counter()]
    blocks = [("(entry)", 0, collections.Counter())]
    for label, mn, _ in stream:
        if label is not None:
            blocks.append((label, len(regions) - 1, collections.Counter()))
            continue
        regions[-1][classify(mn)] += 1
        hist[-1][mn] += 1
        blocks[-1][2][classify(mn)] += 1
        if mn == "s_barrier" or mn in a.split:  # the boundary instruction closes its region
            regions.append(collections.Counter())
            hist.append(collections.Counter())
            if mn == "s_barrier":
                marks.append(f"B{nbar}")
                nbar += 1
            else:
                marks.append(mn)
    total = collections.Counter()
    for r in regions:
        total.update(r)

    print("\nbetween barriers (text order; Bn = the n-th s_barrier of the kernel's text, counted from 0)")
    names = []
    for i in range(len(regions)):
        hi = "end" if i == len(regions) - 1 else marks[i + 1]
        names.append(f"{i:>2} {marks[i]}..{hi}")
    table(list(zip(names, regions)) + [("   whole kernel", total)], "region")

    print("\nper basic block (region = the barrier region its label lies in)")
    table([(f"{reg:>2} {lab}", cnt) for lab, reg, cnt in blocks if sum(cnt.values())], "region block")

    if a.mnemonics:
        for name, h in zip(names, hist):
            print(f"\nmnemonics of region {name.strip()}")
            for mn, n in sorted(h.items(), key=lambda kv: (-kv[1], kv[0])):
                print(f"  {n:>5} {mn}")


if __name__ == "__main__":
    main()
