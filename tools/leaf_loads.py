#!/usr/bin/env python3
"""How the regen kernels fetch a leaf's pair record (pt_trace.h pairTestT), read from the assembly
hipcc generates for pt_regen.hip with _build.py's HIP_FLAGS (device only, no GPU needed).

    python tools/leaf_loads.py                       a table per regenKernel instantiation
    python tools/leaf_loads.py --json OUT.json       the same as JSON (profiles/<round>/leaf_loads.json)
    python tools/leaf_loads.py --src DIR [...]       another tree's csrc/ and include/ (DIR = its root)

Per kernel: its global loads by width, and for every leaf loop the loads from the record's base
register (width in bytes and offset, in program order, with the basic block each sits in) and the
loop's other global loads. A leaf loop is an innermost loop of the kernel that loads from global
memory and divides (the triangle test's IEEE division, v_div_scale_f32: node loops multiply by the
ray's reciprocal direction); the record's base is the address register most of the loop's loads
use. The record is PAIR_F4 = 7 float4: fetched whole and in one round trip it is seven 16-byte
loads at offsets 0, 16, ..., 96 in the loop's first block, and nothing else from that base.
"""
import json
import re
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from opengl_ray_tracing_amd import _build  # noqa: E402

WIDTH = {"ubyte": 1, "sbyte": 1, "ushort": 2, "sshort": 2, "short_d16": 2, "short_d16_hi": 2, "dword": 4,
         "dwordx2": 8, "dwordx3": 12, "dwordx4": 16}
RECORD_OFFSETS = [0, 16, 32, 48, 64, 80, 96]  # PAIR_F4 float4
LOAD = re.compile(r"^\s*global_load_(\w+)\s+(\S+),\s*(v\[\d+:\d+\]|v\d+),\s*(off|s\[\d+:\d+\])(?:\s+offset:(-?\d+))?")
BLOCK = re.compile(r"^(?:\.LBB(\d+_\d+):|; %bb\.(\d+):)")
IN_LOOP = re.compile(r"in Loop: Header=BB(\d+_\d+) Depth=(\d+)")
HEADER = re.compile(r"Loop Header: Depth=(\d+)")


def assembly(root=ROOT, extra=()):
    """pt_regen.hip of the tree at `root` as gfx950 assembly text."""
    root = Path(root)
    csrc, inc = root / "opengl_ray_tracing_amd" / "csrc", root / "include"
    with tempfile.TemporaryDirectory() as tmp:
        out = Path(tmp) / "pt_regen.s"
        cmd = [_build.HIPCC, *_build.HIP_FLAGS, f"-I{inc}", f"-I{csrc}", *extra, "--cuda-device-only", "-S",
               str(csrc / "pt_regen.hip"), "-o", str(out)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode:
            raise RuntimeError("hipcc failed: " + " ".join(cmd) + "\n" + r.stderr[-3000:])
        return out.read_text()


def functions(asm):
    """{mangled name: its lines} of every function of the assembly."""
    out, name, cur = {}, None, []
    for line in asm.splitlines():
        m = re.match(r"^\s*\.type\s+(\S+),@function", line)
        if m:
            name, cur = m.group(1), []
            continue
        if name is not None:
            if line.startswith(".Lfunc_end"):
                out[name] = cur
                name = None
            else:
                cur.append(line)
    return out


def blocks_of(lines):
    """The function's basic blocks in program order: {label, loop (header label of the innermost loop
    the block is in, None outside every loop), inner (it heads an innermost loop), lines}."""
    blocks = [{"label": "entry", "loop": None, "inner": False, "lines": []}]
    for i, line in enumerate(lines):
        m = BLOCK.match(line)
        if m:
            fn_label = m.group(1)
            label = fn_label if fn_label else "%bb." + m.group(2)
            # the loop annotation is on the label's line and the comment lines that follow it
            note = line
            j = i + 1
            while j < len(lines) and lines[j].lstrip().startswith(";") and not BLOCK.match(lines[j]):
                note += lines[j]
                j += 1
            loop, inner = None, False
            if HEADER.search(note):
                loop, inner = label, "Inner Loop Header" in note
            else:
                il = IN_LOOP.search(note)
                if il:
                    loop = il.group(1)
            blocks.append({"label": label, "loop": loop, "inner": inner, "lines": []})
        blocks[-1]["lines"].append(line)
    return blocks


def loads_of(lines):
    out = []
    for line in lines:
        m = LOAD.match(line)
        if m:
            kind, _, vaddr, saddr, off = m.groups()
            out.append({"bytes": WIDTH.get(kind, 0), "kind": kind, "base": vaddr if saddr == "off" else f"{saddr}+{vaddr}",
                        "offset": int(off or 0)})
    return out


def kernel_report(lines):
    by_width = {}
    for ld in loads_of(lines):
        by_width[ld["kind"]] = by_width.get(ld["kind"], 0) + 1
    blocks = blocks_of(lines)
    inner = [b["label"] for b in blocks if b["inner"]]
    loops = []
    for head in inner:
        body = [b for b in blocks if b["loop"] == head]
        text = [ln for b in body for ln in b["lines"]]
        lds = [dict(ld, block=b["label"]) for b in body for ld in loads_of(b["lines"])]
        if not lds or not any("v_div_scale_f32" in ln for ln in text):
            continue
        count = {}
        for ld in lds:
            count[ld["base"]] = count.get(ld["base"], 0) + 1
        base = max(count, key=lambda k: count[k])
        rec = [{"bytes": ld["bytes"], "offset": ld["offset"], "block": ld["block"]} for ld in lds if ld["base"] == base]
        loops.append({"header": head, "base": base, "record_loads": rec,
                      "record_load_blocks": len({ld["block"] for ld in rec}),
                      "other_loads": [{"bytes": ld["bytes"], "offset": ld["offset"], "base": ld["base"]}
                                      for ld in lds if ld["base"] != base],
                      "one_trip": one_trip(rec, head)})
    return {"global_loads": dict(sorted(by_width.items())), "global_loads_total": sum(by_width.values()),
            "leaf_loops": loops}


def one_trip(rec, head):
    """The record as seven 16-byte loads at 0, 16, ..., 96, all in the loop's first block, and no other
    load from its base in the loop."""
    return (sorted(ld["offset"] for ld in rec) == RECORD_OFFSETS and all(ld["bytes"] == 16 for ld in rec)
            and all(ld["block"] == head for ld in rec))


def leaf_loads(root=ROOT, extra=(), prefix="pt::regenKernel<"):
    """{demangled kernel name: kernel_report} of every regenKernel instantiation of the tree at root."""
    fns = functions(assembly(root, extra))
    names = subprocess.run(["c++filt"], input="\n".join(fns), capture_output=True, text=True).stdout.split("\n")
    out = {}
    for nice, mangled in zip(names, fns):
        short = nice.replace("void ", "", 1).split("(")[0]
        if short.startswith(prefix):
            out[short] = kernel_report(fns[mangled])
    return out


def main():
    args = sys.argv[1:]
    root, out = ROOT, None
    if "--src" in args:
        i = args.index("--src")
        root = Path(args[i + 1])
        del args[i:i + 2]
    if "--json" in args:
        i = args.index("--json")
        out = args[i + 1]
        del args[i:i + 2]
    rep = leaf_loads(root, args)
    if out:
        Path(out).write_text(json.dumps(rep, indent=1, sort_keys=True) + "\n")
        print(len(rep), "kernels ->", out)
        return
    for name, k in rep.items():
        print(f"{name}: {k['global_loads_total']} global loads {k['global_loads']}")
        for lp in k["leaf_loops"]:
            widths = {}
            for ld in lp["record_loads"]:
                widths[ld["bytes"]] = widths.get(ld["bytes"], 0) + 1
            print(f"   leaf loop {lp['header']}: {len(lp['record_loads'])} loads from {lp['base']} in "
                  f"{lp['record_load_blocks']} block(s), by bytes {dict(sorted(widths.items()))}, offsets "
                  f"{sorted(ld['offset'] for ld in lp['record_loads'])}, other loads {len(lp['other_loads'])}, "
                  f"one trip: {lp['one_trip']}")


if __name__ == "__main__":
    main()
