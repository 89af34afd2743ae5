#!/usr/bin/env python3
"""Register use of every kernel of one HIP source as hipcc reports it (VGPRs, spills, scratch,
occupancy in waves per SIMD), compiled exactly as _build.py compiles it.

    python tools/kernel_regs.py pt_regen.hip [extra hipcc flags, e.g. -DPT_X=1] [--filter regenKernel]
    python tools/kernel_regs.py --json OUT.json      every .hip of _build.SOURCES (namespace pt), with LDS and code length
    python tools/kernel_regs.py --diff A.json B.json  kernel sets and every figure compared (exit 1 if unequal)
"""
import json
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from opengl_ray_tracing_amd import _build  # noqa: E402

FIELDS = {"VGPRs": "vgpr", "AGPRs": "agpr", "TotalSGPRs": "sgpr", "ScratchSize [bytes/lane]": "scratch",
          "Occupancy [waves/SIMD]": "waves", "VGPRs Spill": "vgpr_spill", "SGPRs Spill": "sgpr_spill",
          "LDS Size [bytes/block]": "lds"}
# what a refactor must leave as it is (SGPRs follow the parameter block's layout)
PINNED = ("vgpr", "agpr", "scratch", "waves", "vgpr_spill", "sgpr_spill", "lds")


def kernels_of(src, extra=()):
    """{demangled kernel name: {vgpr, ..., code_len, file}} of one source."""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [_build.HIPCC, *_build.HIP_FLAGS, f"-I{_build.INCLUDE}", f"-I{_build.CSRC}", *extra, "-c", str(src),
               "-o", f"{tmp}/k.o", "-Rpass-analysis=kernel-resource-usage", "--save-temps"]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=tmp)
        if r.returncode:
            sys.exit(r.stderr[-3000:])
        asm = "".join(p.read_text() for p in Path(tmp).glob("*gfx950*.s"))
    rows, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:.*?\s(Function Name|" + "|".join(map(re.escape, FIELDS)) + r"): (\S+)", line)
        if not m:
            continue
        k, v = m.groups()
        if k == "Function Name":
            cur = rows.setdefault(v, {"file": Path(src).name})
        elif cur is not None:
            cur[FIELDS[k]] = int(v)
    for m in re.finditer(r"^\s*\.size\s+(\S+),.*\n(?:.*\n){0,40}?; codeLenInByte = (\d+)", asm, re.M):
        if m.group(1) in rows:
            rows[m.group(1)]["code_len"] = int(m.group(2))
    names = subprocess.run(["c++filt"], input="\n".join(rows), capture_output=True, text=True).stdout.split("\n")
    return {n: rows[k] for n, k in zip(names, rows)}


def diff(a, b):
    a, b = json.loads(Path(a).read_text()), json.loads(Path(b).read_text())
    bad = 0
    for n in sorted(set(a) ^ set(b)):
        print("only in", "A" if n in a else "B", n)
        bad += 1
    same_len = 0
    for n in sorted(set(a) & set(b)):
        d = {f: (a[n].get(f), b[n].get(f)) for f in PINNED if a[n].get(f) != b[n].get(f)}
        if d:
            print("DIFFERS", n, d)
            bad += 1
        if a[n].get("code_len") == b[n].get("code_len"):
            same_len += 1
        else:
            print(f"code_len {a[n].get('code_len')} -> {b[n].get('code_len')}  {a[n]['file']} -> {b[n]['file']}  {n[:100]}")
    print(f"{len(set(a) & set(b))} kernels in both, {same_len} of equal code length, {bad} differences")
    return 1 if bad else 0


def main():
    args = sys.argv[1:]
    if args and args[0] == "--diff":
        sys.exit(diff(args[1], args[2]))
    if args and args[0] == "--json":
        srcs = [src for kind, src, _ in _build.SOURCES.values() if kind == "hip"]
        with ThreadPoolExecutor(max_workers=4) as ex:
            out = {}
            for rows in ex.map(kernels_of, srcs):  # the project's own functions (not hipcub's instantiations)
                out.update({n: r for n, r in rows.items() if "pt::" in n.split("(")[0]})
        Path(args[1]).write_text(json.dumps(out, indent=1, sort_keys=True) + "\n")
        print(len(out), "kernels ->", args[1])
        return
    flt = None
    if "--filter" in args:
        i = args.index("--filter")
        flt = args[i + 1]
        del args[i:i + 2]
    for name, c in kernels_of(_build.CSRC / args[0], args[1:]).items():
        if flt and flt not in name:
            continue
        print(f"{c.get('vgpr', '?'):>4} vgpr  spill {c.get('vgpr_spill', '?'):>4}/{c.get('sgpr_spill', '?'):>4}  "
              f"scratch {c.get('scratch', '?'):>4}  lds {c.get('lds', '?'):>6}  waves {c.get('waves', '?')}  "
              f"code {c.get('code_len', '?'):>6}  {name[:110]}")


if __name__ == "__main__":
    main()
