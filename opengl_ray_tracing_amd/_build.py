"""In-tree native build: libpt.so (HIP kernels + C-ABI runtime + host scene
prep) for gfx950, and the test-only oracle (oracle/liboracle.so). The host runtime
is one g++ unit per subject (csrc/pt_runtime.h lists them; pt_scene_prep.cpp is the
host-only scene preparation, which tests/native/scene_prep_check.cpp links too).

The built shared objects stay in the source tree (git-ignored) so they travel
to the GPU box with the repository snapshot.
"""
from __future__ import annotations

import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

PKG = Path(__file__).resolve().parent
ROOT = PKG.parent
CSRC = PKG / "csrc"
INCLUDE = ROOT / "include"
BUILD = PKG / "_objs"
LIB = PKG / "libpt.so"
ORACLE_DIR = ROOT / "oracle"
ORACLE_LIB = ORACLE_DIR / "liboracle.so"

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
HIPCC = os.path.join(ROCM, "bin", "hipcc")
ARCH = "gfx950"

HIP_FLAGS = [
    f"--offload-arch={ARCH}", "-O3", "-fPIC", "-std=c++17",
    # exact single-rounding float semantics, matching the CPU checker
    "-ffp-contract=off",
    # no SLP packing of the scalar shading/triangle code into v_pk_* pairs: the
    # lane shuffles it needs raised the MIS megakernel to 239 VGPRs (129 -> 167
    # Lambert / 187 MIS without it) and cost 4-6 % per frame on c2/c3/c4
    # (tools/tune.py); visitNode's explicit float2 slab pairs stay packed
    "-fno-slp-vectorize",
    "-Wall", "-Wno-unused-function",
]
CXX_FLAGS = ["-O2", "-fPIC", "-pthread", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall",
             "-D__HIP_PLATFORM_AMD__", f"-I{ROCM}/include"]

# what every device file sees: pt_device.h and pt_trace.h include pt_kernels.h and pt_fmath.h
_DEV = [CSRC / "pt_device.h", CSRC / "pt_kernels.h", INCLUDE / "pt_fmath.h"]
_FRAME = [*_DEV, CSRC / "pt_frame.h", CSRC / "pt_trace.h"]  # pt_frame.h's device half includes pt_trace.h
_HOST = [CSRC / "pt_runtime.h", CSRC / "pt_frame.h", CSRC / "pt_kernels.h", INCLUDE / "pt_abi.h", CSRC / "pt_rccl.h",
         CSRC / "pt_envupdate.h"]
_UPDATE = [CSRC / "pt_update.h"]  # what the in-place updates share (pt_scene_upload.cpp, pt_env.cpp)
_PREP = [CSRC / "pt_scene_prep.h", CSRC / "pt_kernels.h"]  # the host-only scene preparation (no context, no HIP call)

SOURCES = {
    "pt_kernels.o": ("hip", CSRC / "pt_kernels.hip", [*_FRAME, CSRC / "pt_paths.h", INCLUDE / "pt_scene.h"]),
    "pt_radiance.o": ("hip", CSRC / "pt_radiance.hip", [*_FRAME, CSRC / "pt_paths.h"]),
    "pt_regen.o": ("hip", CSRC / "pt_regen.hip", _FRAME),
    "pt_primary.o": ("hip", CSRC / "pt_primary.hip", _FRAME),
    "pt_guides.o": ("hip", CSRC / "pt_guides.hip", _FRAME),
    "pt_query.o": ("hip", CSRC / "pt_query.hip", _FRAME),
    "pt_display.o": ("hip", CSRC / "pt_display.hip", _FRAME),
    "pt_basic.o": ("hip", CSRC / "pt_basic.hip", [*_DEV, INCLUDE / "pt_scene.h"]),
    "pt_diag.o": ("hip", CSRC / "pt_diag.hip", _DEV),
    "pt_envcache.o": ("hip", CSRC / "pt_envcache.hip", _DEV),
    "pt_envupdate.o": ("hip", CSRC / "pt_envupdate.hip", [*_DEV, CSRC / "pt_envupdate.h", INCLUDE / "pt_rgbe.h"]),
    "pt_build.o": ("hip", CSRC / "pt_build.hip", [CSRC / "pt_kernels.h"]),
    "pt_refit.o": ("hip", CSRC / "pt_refit.hip", [CSRC / "pt_kernels.h"]),
    "pt_materials.o": ("hip", CSRC / "pt_materials.hip", [CSRC / "pt_kernels.h"]),
    "pt_denoise.o": ("hip", CSRC / "pt_denoise.hip", [CSRC / "pt_atrous.h", *_DEV]),
    "pt_temporal.o": ("hip", CSRC / "pt_temporal.hip", _DEV),
    "pt_variance.o": ("hip", CSRC / "pt_variance.hip", [CSRC / "pt_atrous.h", *_DEV]),
    "pt_adaptive.o": ("hip", CSRC / "pt_adaptive.hip", _FRAME),
    # (last of the device objects: the order bench.py's c2 line was measured with)
    "pt_radiance_mean.o": ("hip", CSRC / "pt_radiance_mean.hip", [*_FRAME, CSRC / "pt_paths.h"]),
    # the host runtime by subject (pt_runtime.h lists the files); the host-only scene preparation keeps
    # -ffp-contract=off like the rest: its unit normal and plane offset round as the reference's do
    "pt_context.o": ("cxx", CSRC / "pt_context.cpp", [*_HOST, CSRC / "pt_plan.h", INCLUDE / "pt_fmath.h"]),
    "pt_scene_prep.o": ("cxx", CSRC / "pt_scene_prep.cpp", [*_PREP, CSRC / "pt_accel.h"]),
    "pt_scene_upload.o": ("cxx", CSRC / "pt_scene_upload.cpp", [*_HOST, *_PREP, *_UPDATE, CSRC / "pt_plan.h"]),
    "pt_env.o": ("cxx", CSRC / "pt_env.cpp", [*_HOST, *_UPDATE, INCLUDE / "pt_scene.h"]),
    "pt_runtime.o": ("cxx", CSRC / "pt_runtime.cpp", [*_HOST, CSRC / "pt_plan.h"]),  # the frame path
    "pt_queries.o": ("cxx", CSRC / "pt_queries.cpp", _HOST),
    "pt_accum.o": ("cxx", CSRC / "pt_accum.cpp", [*_HOST, CSRC / "pt_plan.h"]),
    "pt_group.o": ("cxx", CSRC / "pt_group.cpp", _HOST),
    "pt_post.o": ("cxx", CSRC / "pt_post.cpp", [*_HOST, CSRC / "pt_plan.h"]),
    "pt_rccl.o": ("cxx", CSRC / "pt_rccl.cpp", [CSRC / "pt_rccl.h"]),
    "scene.o": ("cxx", CSRC / "scene.cpp", [INCLUDE / "pt_scene.h", CSRC / "pt_accel.h", CSRC / "pt_introsort.h"]),
}


def _stale(target: Path, deps) -> bool:
    if not target.exists():
        return True
    t = target.stat().st_mtime
    return any(Path(d).stat().st_mtime > t for d in deps)


def _run(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("build failed: " + " ".join(map(str, cmd)) + "\n" + r.stdout + r.stderr)
    return r


def build_native(force: bool = False, verbose: bool = False) -> Path:
    BUILD.mkdir(exist_ok=True)
    jobs = []
    objs = []
    for obj, (kind, src, deps) in SOURCES.items():
        out = BUILD / obj
        objs.append(out)
        if force or _stale(out, [src, *deps]):
            inc = [f"-I{INCLUDE}", f"-I{CSRC}"]
            if kind == "hip":
                cmd = [HIPCC, *HIP_FLAGS, *inc, "-c", str(src), "-o", str(out)]
            else:
                cmd = ["g++", *CXX_FLAGS, *inc, "-c", str(src), "-o", str(out)]
            jobs.append(cmd)
    if jobs:
        with ThreadPoolExecutor(max_workers=min(4, len(jobs))) as ex:
            for r in ex.map(_run, jobs):
                if verbose and (r.stdout or r.stderr):
                    sys.stderr.write(r.stdout + r.stderr)
    if force or jobs or _stale(LIB, objs):
        _run([HIPCC, f"--offload-arch={ARCH}", "-shared", "-pthread", "-o", str(LIB), *map(str, objs), "-ldl"])
    return LIB


VARIANTS = PKG / "_variants"


def variant_lib(name: str) -> Path:
    return VARIANTS / f"libpt_{name}.so"


def build_variant(name: str, defines: dict, hip_flags=()) -> Path:
    """A tuning build of libpt.so with extra -D defines (e.g. PT_MIN_WAVES, PT_LDS_STACK)
    and extra hipcc flags, kept in-tree under _variants/ so tools/tune.py can A/B it on
    the GPU box."""
    out_dir = VARIANTS / name
    out_dir.mkdir(parents=True, exist_ok=True)
    dflags = [f"-D{k}={v}" for k, v in defines.items()]
    inc = [f"-I{INCLUDE}", f"-I{CSRC}"]
    objs, cmds = [], []
    for obj, (kind, src, deps) in SOURCES.items():
        out = out_dir / obj
        objs.append(out)
        if kind == "hip":
            cmds.append([HIPCC, *HIP_FLAGS, *hip_flags, *dflags, *inc, "-c", str(src), "-o", str(out)])
        else:
            cmds.append(["g++", *CXX_FLAGS, *dflags, *inc, "-c", str(src), "-o", str(out)])
    with ThreadPoolExecutor(max_workers=4) as ex:
        list(ex.map(_run, cmds))
    lib = variant_lib(name)
    _run([HIPCC, f"--offload-arch={ARCH}", "-shared", "-pthread", "-o", str(lib), *map(str, objs), "-ldl"])
    return lib


ABI_CALLER_SRC = ROOT / "tests" / "native" / "abi_caller.cpp"
ABI_CALLER = ROOT / "tests" / "native" / "abi_caller"


def build_abi_caller(force: bool = False) -> Path:
    """Test infrastructure: the compiled reference-side caller of the C ABI (tests/native/abi_caller.cpp,
    INTEGRATION.md's DisneyBRDF display() loop), g++ against include/*.h and -lpt only."""
    deps = [ABI_CALLER_SRC, INCLUDE / "pt_abi.h", INCLUDE / "pt_scene.h", LIB]
    if force or _stale(ABI_CALLER, deps):
        _run(["g++", "-std=c++17", "-O2", "-Wall", str(ABI_CALLER_SRC), f"-I{INCLUDE}", f"-L{PKG}", "-lpt",
              "-Wl,-rpath,$ORIGIN/../../opengl_ray_tracing_amd", "-o", str(ABI_CALLER)])
    return ABI_CALLER


PLAN_TABLE_SRC = ROOT / "tests" / "native" / "plan_table.cpp"
PLAN_TABLE = ROOT / "tests" / "native" / "plan_table"


def build_plan_table(force: bool = False) -> Path:
    """Test infrastructure: the frame path's launch policy (csrc/pt_plan.h) on contexts filled by hand
    (tests/native/plan_table.cpp), host-only: the HIP headers for the types, no HIP library."""
    deps = [PLAN_TABLE_SRC, CSRC / "pt_plan.h", *_HOST]
    if force or _stale(PLAN_TABLE, deps):
        _run(["g++", "-std=c++17", "-O1", "-Wall", "-Wno-unused-function", "-D__HIP_PLATFORM_AMD__", f"-I{ROCM}/include",
              f"-I{INCLUDE}", f"-I{CSRC}", str(PLAN_TABLE_SRC), "-o", str(PLAN_TABLE)])
    return PLAN_TABLE


ENV_FORMS_TABLE_SRC = ROOT / "tests" / "native" / "env_forms_table.cpp"
ENV_FORMS_TABLE = ROOT / "tests" / "native" / "env_forms_table"


def build_env_forms_table(force: bool = False) -> Path:
    """Test infrastructure: the view of the environment's store the kernels get (csrc/pt_envupdate.h envForms)
    for stores filled by hand (tests/native/env_forms_table.cpp), host-only like plan_table."""
    deps = [ENV_FORMS_TABLE_SRC, CSRC / "pt_envupdate.h", CSRC / "pt_kernels.h"]
    if force or _stale(ENV_FORMS_TABLE, deps):
        _run(["g++", "-std=c++17", "-O1", "-Wall", "-Wno-unused-function", "-D__HIP_PLATFORM_AMD__", f"-I{ROCM}/include",
              f"-I{INCLUDE}", f"-I{CSRC}", str(ENV_FORMS_TABLE_SRC), "-o", str(ENV_FORMS_TABLE)])
    return ENV_FORMS_TABLE


SHARE_TABLE_SRC = ROOT / "tests" / "native" / "share_table.cpp"
SHARE_TABLE = ROOT / "tests" / "native" / "share_table"


def build_share_table(force: bool = False) -> Path:
    """Test infrastructure: the screen-tile share's arithmetic (csrc/pt_frame.h, the host half the kernels
    share) printed as tables (tests/native/share_table.cpp), host-only like plan_table."""
    deps = [SHARE_TABLE_SRC, CSRC / "pt_frame.h", CSRC / "pt_kernels.h"]
    if force or _stale(SHARE_TABLE, deps):
        _run(["g++", "-std=c++17", "-O1", "-Wall", "-Wno-unused-function", "-D__HIP_PLATFORM_AMD__", f"-I{ROCM}/include",
              f"-I{INCLUDE}", f"-I{CSRC}", str(SHARE_TABLE_SRC), "-o", str(SHARE_TABLE)])
    return SHARE_TABLE


SCENE_PREP_CHECK_SRC = ROOT / "tests" / "native" / "scene_prep_check.cpp"
SCENE_PREP_CHECK = ROOT / "tests" / "native" / "scene_prep_check"


def build_scene_prep_check(force: bool = False) -> Path:
    """Test infrastructure: the host-only scene preparation (csrc/pt_scene_prep.cpp, with scene.cpp's host
    builder) dumped for a scene read from a file (tests/native/scene_prep_check.cpp), host-only like
    plan_table, compiled with the library's own CXX_FLAGS (the unit normal and plane offset round by them)."""
    srcs = [SCENE_PREP_CHECK_SRC, CSRC / "pt_scene_prep.cpp", CSRC / "scene.cpp"]
    deps = [*srcs, *_PREP, CSRC / "pt_accel.h", CSRC / "pt_introsort.h", INCLUDE / "pt_scene.h"]
    if force or _stale(SCENE_PREP_CHECK, deps):
        _run(["g++", *CXX_FLAGS, "-Wno-unused-function", f"-I{INCLUDE}", f"-I{CSRC}", *map(str, srcs),
              "-o", str(SCENE_PREP_CHECK)])
    return SCENE_PREP_CHECK


MATERIAL_TABLE_CHECK_SRC = ROOT / "tests" / "native" / "material_table_check.cpp"
MATERIAL_TABLE_CHECK = ROOT / "tests" / "native" / "material_table_check"


def build_material_table_check(force: bool = False, sanitize: bool = False) -> Path:
    """Test infrastructure: the material-table function of the host-only scene preparation
    (csrc/pt_scene_prep.cpp materialTable) on records read from a file (tests/native/material_table_check.cpp),
    host-only like scene_prep_check. sanitize: a second program, built with -fsanitize=address,undefined,
    whose self check runs without arguments."""
    srcs = [MATERIAL_TABLE_CHECK_SRC, CSRC / "pt_scene_prep.cpp", CSRC / "scene.cpp"]
    deps = [*srcs, *_PREP, CSRC / "pt_accel.h", CSRC / "pt_introsort.h", INCLUDE / "pt_scene.h"]
    out = MATERIAL_TABLE_CHECK.with_name("material_table_check_san") if sanitize else MATERIAL_TABLE_CHECK
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O1"] if sanitize else []
    if force or _stale(out, deps):
        _run(["g++", *CXX_FLAGS, *san, "-Wno-unused-function", f"-I{INCLUDE}", f"-I{CSRC}", *map(str, srcs), "-o", str(out)])
    return out


ENV_QUANTISE_CHECK_SRC = ROOT / "tests" / "native" / "env_quantise_check.cpp"
ENV_QUANTISE_CHECK = ROOT / "tests" / "native" / "env_quantise_check"


def build_env_quantise_check(force: bool = False, sanitize: bool = False) -> Path:
    """Test infrastructure: the RGBE quantiser of pt_update_env (include/pt_rgbe.h, the function the kernel
    calls) on texels read from a file (tests/native/env_quantise_check.cpp), host-only, compiled with the
    library's own CXX_FLAGS. sanitize: a second program built with -fsanitize=address,undefined."""
    deps = [ENV_QUANTISE_CHECK_SRC, INCLUDE / "pt_rgbe.h"]
    out = ENV_QUANTISE_CHECK.with_name("env_quantise_check_san") if sanitize else ENV_QUANTISE_CHECK
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O1"] if sanitize else []
    if force or _stale(out, deps):
        _run(["g++", *CXX_FLAGS, *san, f"-I{INCLUDE}", str(ENV_QUANTISE_CHECK_SRC), "-o", str(out)])
    return out


def build_oracle(force: bool = False) -> Path:
    """Test infrastructure only (see oracle/pt_oracle.h)."""
    src = [ORACLE_DIR / "pt_oracle.c", ORACLE_DIR / "pt_oracle.h", ORACLE_DIR / "Makefile", INCLUDE / "pt_fmath.h"]
    if force or _stale(ORACLE_LIB, src):
        _run(["make", "-s", "-C", str(ORACLE_DIR), "-B" if force else "all"])
    return ORACLE_LIB


if __name__ == "__main__":
    build_native(force="--force" in sys.argv, verbose=True)
    build_oracle(force="--force" in sys.argv)
    build_abi_caller(force="--force" in sys.argv)
    build_plan_table(force="--force" in sys.argv)
    build_share_table(force="--force" in sys.argv)
    build_env_forms_table(force="--force" in sys.argv)
    build_scene_prep_check(force="--force" in sys.argv)
    build_material_table_check(force="--force" in sys.argv)
    build_env_quantise_check(force="--force" in sys.argv)
    print(LIB)
    print(ORACLE_LIB)
