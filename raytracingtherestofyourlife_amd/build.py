"""Build librtp.so (HIP kernels + C ABI) in-tree for gfx950 with hipcc.

The shared object lands next to this file so it travels to the GPU box with
the repository snapshot.  Flags that the parity contract depends on:
  -ffp-contract=off      no a*b+c -> fma contraction (the reference's x86-64
                         g++ build has no FMA);
  no -ffast-math, HIP's default correctly-rounded f32 div/sqrt, denormals kept.
"""
from __future__ import annotations

import hashlib
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "librtp.so")
# the host units that make no HIP call and include no HIP header: they also build
# as plain C++ without a HIP include path or library (build_scene_build_check)
DEVICE_FREE_SOURCES = ["rtp_base_host.cpp", "rtp_scene_host.cpp", "rtp_mesh_host.cpp", "scene_cornell.cpp"]
SOURCES = ["rtp_kernels.hip", "rtp_direct.hip", "rtp_bvh_gpu.hip", "rtp_mesh_gpu.hip", "rtp_denoise.hip", "rtp_adaptive.hip", "rtp_host.cpp", "rtp_ff_host.cpp", "rtp_debug_host.cpp", "rtp_direct_host.cpp", "rtp_adaptive_host.cpp",
           *DEVICE_FREE_SOURCES]
HEADERS = ["rtp_trace.hpp", "rtp_pool.hpp", "rtp_diag.hpp", "rtp_launch.hpp", "rtp_launch_decl.hpp", "rtp_device.hpp", "rtp_layout.hpp", "rtp_context.hpp", "rtp_host_base.hpp", "rtp_host_util.hpp", "rtp_scene.hpp", "rtp_ff.hpp", "rtp_adaptive.hpp", "rtp_bvh_host.hpp", "rtp_mesh.hpp", "rtp_mesh_gpu.hpp", "rtp_mesh_cell.hpp", "rtp_lbvh.hpp", "glibc_powf.hpp", os.path.join("..", "..", "include", "rtp.h"),
           os.path.join("..", "..", "include", "rtp_adaptive.h"), os.path.join("..", "..", "include", "rtp_mesh.h")]
ARCH = os.environ.get("RTP_OFFLOAD_ARCH", "gfx950")


def hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found: librtp.so cannot be built")


def flags() -> list[str]:
    # -fno-slp-vectorize: the SLP vectorizer paired scalar float products
    # (dot products, cross products) into v_pk_mul_f32 / v_pk_add_f32, each
    # followed by an s_nop before its result is read (gfx950's packed-FP32
    # hazard); scalar they need none.  C2 101.5-102.9 -> 96.2-97.2 ms (-5.5%),
    # C3 -3.2% (profiles/r04n_ab_noslp.txt).  The explicit packed pairs of the
    # quad tests (ext_vector_type) stay packed.  Results are the same bits:
    # a packed half rounds like the scalar instruction.
    return ["-O3", f"--offload-arch={ARCH}", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
            "-fno-fast-math", "-fno-slp-vectorize", "-Wall", "-Wno-unused-function", "-Wno-unused-variable"]


def stale() -> bool:
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    deps = [os.path.join(CSRC, f) for f in SOURCES + HEADERS] + [os.path.abspath(__file__)]
    return any(os.path.getmtime(d) > t for d in deps if os.path.exists(d))


def build(force: bool = False, verbose: bool = False) -> str:
    if not force and not stale():
        return LIB
    cmd = [hipcc(), *flags(), "-o", LIB + ".tmp", *[os.path.join(CSRC, s) for s in SOURCES]]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError(f"hipcc failed ({res.returncode}):\n{res.stdout}\n{res.stderr}")
    os.replace(LIB + ".tmp", LIB)
    return LIB


ROOT = os.path.dirname(HERE)
# C++ host programs over the C ABI (include/rtp/rendering.hpp), linked with g++
CPP_PROGRAMS = {
    os.path.join(ROOT, "examples", "rtp_path"): os.path.join(ROOT, "examples", "path_main.cpp"),
    os.path.join(ROOT, "tests", "cpp", "shim_check"): os.path.join(ROOT, "tests", "cpp", "shim_check.cpp"),
    os.path.join(ROOT, "tests", "cpp", "mesh_mapper"): os.path.join(ROOT, "tests", "cpp", "mesh_mapper.cpp"),
}


def build_cpp(force: bool = False) -> list[str]:
    """g++ the C++ host programs against librtp.so (rpath to the package dir)."""
    lib = build()
    built = []
    hdrs = [os.path.join(ROOT, "include", "rtp.h"), os.path.join(ROOT, "include", "rtp_adaptive.h"),
            os.path.join(ROOT, "include", "rtp_mesh.h"), os.path.join(ROOT, "include", "rtp", "rendering.hpp"), lib]
    for exe, src in CPP_PROGRAMS.items():
        rel = os.path.relpath(HERE, os.path.dirname(exe))
        if force or not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in hdrs + [src]):
            cmd = [os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), src,
                   "-L", HERE, "-lrtp", f"-Wl,-rpath,$ORIGIN/{rel}", "-o", exe]
            res = subprocess.run(cmd, capture_output=True, text=True)
            if res.returncode != 0:
                raise RuntimeError(f"g++ failed for {src}:\n{res.stderr}")
        built.append(exe)
    return built


# The per-cell maths of the mesh builders (csrc/rtp_mesh_cell.hpp) as host C++
# with its own main: no HIP, no librtp.so (tests/test_mesh_cell.py).
MESH_CELL_CHECK = os.path.join(ROOT, "tests", "cpp", "mesh_cell_check")


def build_mesh_cell_check(force: bool = False) -> str:
    src = MESH_CELL_CHECK + ".cpp"
    deps = [src, os.path.join(CSRC, "rtp_mesh_cell.hpp"), os.path.join(CSRC, "rtp_layout.hpp")]
    if force or not os.path.exists(MESH_CELL_CHECK) or any(os.path.getmtime(d) > os.path.getmtime(MESH_CELL_CHECK)
                                                            for d in deps):
        cmd = [hipcc(), "-x", "c++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-I", CSRC,
               src, "-o", MESH_CELL_CHECK]
        res = subprocess.run(cmd, capture_output=True, text=True)
        if res.returncode != 0:
            raise RuntimeError(f"hipcc -x c++ failed for {src}:\n{res.stderr}")
    return MESH_CELL_CHECK


# The inline scene build (csrc/rtp_scene_host.cpp) with the other device-free
# units as plain C++ under a main of its own (tests/test_scene_build.py): no
# HIP include path on the compile, no HIP library on the link, every symbol
# resolved -- a HIP dependency in any of these units fails this build.
SCENE_BUILD_CHECK = os.path.join(ROOT, "tests", "cpp", "scene_build_check")


def rocm_clangxx() -> str:
    """The clang++ beside hipcc: the same compiler without the HIP driver, so
    no HIP include path or library comes in unasked."""
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(hipcc())))
    for cand in (os.path.join(rocm, "llvm", "bin", "clang++"), os.path.join(rocm, "lib", "llvm", "bin", "clang++")):
        if os.path.exists(cand):
            return cand
    raise RuntimeError(f"ROCm clang++ not found under {rocm}")


def build_scene_build_check(force: bool = False) -> str:
    src = SCENE_BUILD_CHECK + ".cpp"
    units = [os.path.join(CSRC, s) for s in DEVICE_FREE_SOURCES]
    hdrs = [os.path.join(CSRC, h) for h in HEADERS]
    cmd = [rocm_clangxx(), "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-I", CSRC,
           "-I", os.path.join(ROOT, "include"), src, *units]
    key = _content_key(cmd, [src, *units, *hdrs])
    if force or not _cached(SCENE_BUILD_CHECK, key):
        res = subprocess.run([*cmd, "-o", SCENE_BUILD_CHECK], capture_output=True, text=True)
        if res.returncode != 0:
            raise RuntimeError(f"clang++ failed for {src}:\n{res.stderr[-4000:]}")
        _made(SCENE_BUILD_CHECK, key)
    return SCENE_BUILD_CHECK


# The reference's own main.cc and CornellBox.cpp, compiled UNCHANGED against
# librtp.so through the VTK-m-named headers of include/vtkm_compat
# (rtp/vtkm_compat.hpp).  The recipe is oracle/ref_build.py; its objects and
# binaries land in oracle/_ref/ (ignored by git): nothing of the reference is
# copied, the binaries are built where the reference tree exists and are used
# as built where it does not (oracle/_ref/ goes with the built tree).
REFERENCE_DIR = os.environ.get("RTP_REFERENCE_DIR", "/root/reference")
REFERENCE_MAIN = os.path.join(REFERENCE_DIR, "main.cc")
MAIN_UNCHANGED = os.path.join(ROOT, "oracle", "_ref", "main_cc")
SCENE_CHECK = os.path.join(ROOT, "oracle", "_ref", "scene_unchanged_check")


def _ref_recipe():
    import importlib.util

    spec = importlib.util.spec_from_file_location("rtp_oracle_ref_build", os.path.join(ROOT, "oracle", "ref_build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def build_main_unchanged(force: bool = False):
    """Build oracle/_ref/main_cc from the reference's main.cc + CornellBox.cpp,
    and oracle/_ref/scene_unchanged_check (the reference's CornellBox against
    rtp_cornell_box), by oracle/ref_build.py; None when the reference is
    absent (a machine that received the built tree)."""
    recipe = _ref_recipe()
    assert (recipe.MAIN_UNCHANGED, recipe.SCENE_CHECK) == (MAIN_UNCHANGED, SCENE_CHECK)
    if not all(os.path.exists(os.path.join(REFERENCE_DIR, f)) for f in recipe.REFERENCE_SOURCES):
        return None
    return recipe.build_ref(REFERENCE_DIR, build(), force=force)


ASAN_DIR = os.path.join(ROOT, "tests", "cpp", "asan")
# programs linked against the host-sanitized library sources (not librtp.so)
ASAN_PROGRAMS = {
    os.path.join(ASAN_DIR, "asan_scene"): os.path.join(ROOT, "tests", "cpp", "asan_scene.cpp"),
    os.path.join(ASAN_DIR, "shim_check"): os.path.join(ROOT, "tests", "cpp", "shim_check.cpp"),
    os.path.join(ASAN_DIR, "asan_adaptive"): os.path.join(ROOT, "tests", "cpp", "asan_adaptive.cpp"),
    os.path.join(ASAN_DIR, "asan_mesh"): os.path.join(ROOT, "tests", "cpp", "asan_mesh.cpp"),
    os.path.join(ASAN_DIR, "asan_mesh_tri"): os.path.join(ROOT, "tests", "cpp", "asan_mesh_tri.cpp"),
    os.path.join(ASAN_DIR, "mesh_cell_check"): os.path.join(ROOT, "tests", "cpp", "mesh_cell_check.cpp"),
    os.path.join(ASAN_DIR, "scene_build_check"): os.path.join(ROOT, "tests", "cpp", "scene_build_check.cpp"),
}
# AddressSanitizer + UBSan on host code only (GPU sanitizers are not available
# on the pool): each -fsanitize= directly after -Xarch_host.  The sanitizer
# runtime links statically into the executables (clang's default).
ASAN_HOST = ["-Xarch_host", "-fsanitize=address", "-Xarch_host", "-fsanitize=undefined",
             "-Xarch_host", "-fno-omit-frame-pointer", "-Xarch_host", "-fno-sanitize-recover=undefined"]


def _content_key(cmd: list[str], files: list[str], more: list[str] = ()) -> str:
    """What a cached build product was made from: the command, the bytes of
    the files it read and the keys of the products it linked."""
    # (paths by their last component: the same tree elsewhere makes the same key)
    h = hashlib.sha256("\0".join([*[os.path.basename(c) if os.path.isabs(c) else c for c in cmd], *more]).encode())
    for f in files:
        h.update(b"\0" + os.path.basename(f).encode() + b"\0")
        if os.path.exists(f):
            with open(f, "rb") as fh:
                h.update(fh.read())
    return h.hexdigest()


def _file_digest(path: str) -> str:
    with open(path, "rb") as fh:
        return hashlib.sha256(fh.read()).hexdigest()


def _cached(target: str, key: str) -> bool:
    """Whether `target` is the very file that was made from `key` (_made wrote
    both digests beside it).  A product without a key file, made from other
    sources, or overwritten since by another build, is not reused whatever its
    time stamp says: an object left by another revision of a source
    (rtp_host.cpp before its split defines what other units define now) would
    otherwise link into the programs of this one."""
    try:
        with open(target + ".key") as fh:
            return fh.read().split() == [key, _file_digest(target)]
    except OSError:
        return False


def _made(target: str, key: str) -> None:
    with open(target + ".key", "w") as fh:
        fh.write(f"{key} {_file_digest(target)}\n")


def build_asan(force: bool = False) -> list[str]:
    """Host-sanitized builds of the library's sources linked into the test
    drivers of tests/cpp (one object per source, cached by the content of the
    source and the headers, not by time stamps)."""
    os.makedirs(ASAN_DIR, exist_ok=True)
    base = [hipcc(), "-O1", "-g", f"--offload-arch={ARCH}", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
            "-fno-slp-vectorize", *ASAN_HOST]
    hdrs = [os.path.join(CSRC, f) for f in HEADERS]
    objs, obj_keys = [], []
    for s in SOURCES:
        src = os.path.join(CSRC, s)
        obj = os.path.join(ASAN_DIR, s + ".o")
        cmd = [*base, "-fPIC", "-c", src]
        key = _content_key(cmd, [src, *hdrs])
        if force or not _cached(obj, key):
            res = subprocess.run([*cmd, "-o", obj + ".tmp"], capture_output=True, text=True)
            if res.returncode != 0:
                raise RuntimeError(f"hipcc (asan) failed for {s}:\n{res.stderr}")
            os.replace(obj + ".tmp", obj)
            _made(obj, key)
        objs.append(obj)
        obj_keys.append(key)
    inc = os.path.join(ROOT, "include")
    built = []
    for exe, src in ASAN_PROGRAMS.items():
        if not os.path.exists(src):
            continue  # a tests/ tree without this driver: the others still build; its test finds no program
        # the driver is host C++ (g++-style, like build_cpp), the link
        # pulls in the HIP runtime and the static sanitizer runtimes
        cmd = [*base, "-x", "c++", "-I", inc, "-I", CSRC, "-c", src]
        key = _content_key(cmd, [src, os.path.join(inc, "rtp.h"), os.path.join(inc, "rtp_adaptive.h"),
                                 os.path.join(inc, "rtp", "rendering.hpp"), *hdrs], obj_keys)
        if force or not _cached(exe, key):
            res = subprocess.run([*cmd, "-o", exe + ".o"], capture_output=True, text=True)
            if res.returncode == 0:
                res = subprocess.run([hipcc(), "-fsanitize=address,undefined", exe + ".o", *objs, "-o", exe],
                                     capture_output=True, text=True)
            if res.returncode != 0:
                raise RuntimeError(f"hipcc (asan) build failed for {src}:\n{res.stderr[-4000:]}")
            _made(exe, key)
        built.append(exe)
    return built


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
    print("\n".join(build_cpp(force="--force" in sys.argv)))
    print(build_mesh_cell_check(force="--force" in sys.argv))
    print(build_scene_build_check(force="--force" in sys.argv))
    print(build_main_unchanged(force="--force" in sys.argv))
