"""The C ABI library (librtp.so) loads and exports every symbol include/rtp.h
declares; host-side helpers behave like the reference (CPU only)."""
from __future__ import annotations

import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(ROOT, "include", "rtp.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(rtp_[a-z_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    import raytracingtherestofyourlife_amd as rtp

    L = rtp.load()
    names = _declared()
    assert len(names) >= 12
    missing = [n for n in names if not hasattr(L, n)]
    assert not missing, missing
    out = subprocess.run(["nm", "-D", "--defined-only", rtp.LIB_PATH], capture_output=True, text=True).stdout
    for n in names:
        assert re.search(rf"\bT {n}$", out, flags=re.M), n
    assert set(names) == set(rtp._lib.EXPORTED_SYMBOLS) == set(rtp._lib.SIGNATURES["include/rtp.h"])


@pytest.mark.parametrize("group", [*_abi.PUBLIC_HEADERS, "hooks"])
def test_signature_table_matches_the_header(group):
    """Every row of a group of _lib.SIGNATURES against its prototype: argument
    count, each argument's class (exact scalar; pointer kind and pointee; a
    struct pointer typed, never void*), return class.  A public header's group
    is the header: the same names in the same order.  The hooks' group holds
    what Python calls of csrc/rtp_launch_decl.hpp and csrc/rtp_mesh.hpp, in
    their order; launchers that take device structs have no row."""
    from raytracingtherestofyourlife_amd import _lib

    rows = _lib.SIGNATURES[group]
    if group in _abi.PUBLIC_HEADERS:
        protos = _abi.prototypes(group)
        assert set(protos) == set(rows) and len(protos) == _abi.PUBLIC_HEADERS[group]
        assert list(protos) == list(rows), "the table is in the header's order"
    else:
        assert group == _lib.HOOKS and list(_lib.SIGNATURES) == [*_abi.PUBLIC_HEADERS, _lib.HOOKS]
        protos = _abi.prototypes(*[os.path.relpath(os.path.join(_abi.CSRC, h), ROOT) for h in _lib.HOOK_HEADERS])
        assert rows and not set(rows) - set(protos), "every hook row has a prototype"
        assert [n for n in protos if n in rows] == list(rows), "the rows are in the headers' order"
    bad = _abi.disagreements(protos, rows, plain_c=group == _lib.HOOKS)
    assert not bad, "\n".join(bad)
    # no name in two groups
    assert all(name not in g for key, g in _lib.SIGNATURES.items() if key != group for name in rows)
    # and load() applied the rows
    L = _lib.load()
    for name, (restype, argtypes) in rows.items():
        assert getattr(L, name).restype is restype and list(getattr(L, name).argtypes) == argtypes, name


def test_refine_params_mirror_the_header():
    from raytracingtherestofyourlife_amd import _lib

    fields = [(n, t) for n, t in _lib.RtpRefineParams._fields_]
    assert fields == [("threshold", ctypes.c_float), ("spp", ctypes.c_int32), ("max_spp", ctypes.c_int32)]
    body = re.search(r"typedef struct \{(.*?)\} rtp_refine_params;", _abi.source("include/rtp_adaptive.h"),
                     flags=re.S).group(1)
    assert re.findall(r"(\w+)\s+(\w+);", body) == [("float", "threshold"), ("int32_t", "spp"), ("int32_t", "max_spp")]


def test_load_missing_symbol_rule(tmp_path, monkeypatch):
    """A library named by RTP_LIB_PATH may lack symbols (calling one raises
    AttributeError); the in-tree library must export them all."""
    import raytracingtherestofyourlife_amd._lib as L

    src, stub, stub2 = tmp_path / "stub.c", str(tmp_path / "libstub.so"), str(tmp_path / "libstub2.so")
    src.write_text('const char* rtp_last_error(void) { return ""; }\nint rtp_abi_version(void) { return 3; }\n')
    subprocess.run([os.environ.get("CC", "cc"), "-shared", "-fPIC", str(src), "-o", stub], check=True,
                   capture_output=True)
    monkeypatch.setattr(L, "LIB_PATH", stub)
    monkeypatch.setattr(L, "_lib", None)
    monkeypatch.setenv("RTP_LIB_PATH", stub)
    lib = L.load(build_if_missing=False)
    assert lib.rtp_abi_version() == 3
    with pytest.raises(AttributeError):
        lib.rtp_render_views
    monkeypatch.setattr(L, "_lib", None)
    monkeypatch.delenv("RTP_LIB_PATH")
    with pytest.raises(RuntimeError, match="rtp_render_views"):
        L.load(build_if_missing=False)
    assert L._lib is None
    # the same rule for the rows beyond rtp.h: a stub with every public entry point but no
    # adaptive one and no internal hook
    public = [n for g in ("include/rtp.h", "include/rtp_mesh.h") for n in L.SIGNATURES[g]]
    src.write_text("".join(f"int {n}(void) {{ return 3; }}\n" for n in public))
    subprocess.run([os.environ.get("CC", "cc"), "-shared", "-fPIC", str(src), "-o", stub2], check=True,
                   capture_output=True)
    monkeypatch.setattr(L, "LIB_PATH", stub2)
    monkeypatch.setenv("RTP_LIB_PATH", stub2)
    lib = L.load(build_if_missing=False)
    assert lib.rtp_abi_version() == 3
    for name in ("rtp_refine_device", "rtp_plan_steal"):
        with pytest.raises(AttributeError):
            getattr(lib, name)
    monkeypatch.setattr(L, "_lib", None)
    monkeypatch.delenv("RTP_LIB_PATH")
    with pytest.raises(RuntimeError, match="rtp_noise_device.*rtp_plan_steal"):
        L.load(build_if_missing=False)
    assert L._lib is None


def test_debug_counter_names_cover_the_enum():
    from raytracingtherestofyourlife_amd import _lib

    src = open(os.path.join(os.path.dirname(_lib.__file__), "csrc", "rtp_layout.hpp")).read()
    body = re.search(r"enum DbgCounter \{(.*?)\bkDbgCounters\b", src, flags=re.S).group(1)
    enumerators = re.findall(r"\bkDbg\w+", re.sub(r"//[^\n]*", "", body))
    assert len(enumerators) == len(set(enumerators)) == len(_lib.DEBUG_COUNTERS) - 1 == _lib.N_DBG_COUNTERS
    assert _lib.DEBUG_COUNTERS[-1] == "max_wave_cycles"


@pytest.mark.parametrize("variant", [0, 1, 2, 3])
def test_scene_desc_of_cornell_arrays_equals_the_librarys(variant):
    """CornellBox(v).buildDataSet()'s arrays through the package's one scene
    hand-over and device.scene_desc give rtp_cornell_box(v)'s own descriptor."""
    import raytracingtherestofyourlife_amd as rtp
    from raytracingtherestofyourlife_amd import _lib, device, mapper

    class Recorder:
        def set_scene(self, *args):
            self.desc, self.arrays = device.scene_desc(*args)

    cb = rtp.CornellBox(variant)
    cb.buildDataSet()
    rec = Recorder()
    mapper._set_cornell_scene(rec, cb)
    got, want = rec.desc, _lib.RtpSceneDesc()
    _lib.check(rtp.load().rtp_cornell_box(variant, want))
    counts = ("n_points", "n_quads", "n_spheres", "n_mat", "n_tex_type", "n_tex")
    assert [getattr(got, k) for k in counts] == [getattr(want, k) for k in counts]
    assert want.n_quads > 0 and want.n_spheres > 0
    sizes = dict(points=3 * want.n_points, quad_points=4 * want.n_quads, quad_mat=want.n_quads,
                 quad_tex=want.n_quads, sphere_point=want.n_spheres, sphere_radius=want.n_spheres,
                 sphere_mat=want.n_spheres, sphere_tex=want.n_spheres, mat_type=want.n_mat,
                 tex_type=want.n_tex_type, tex_rgb=3 * want.n_tex)
    pointers = [f for f, t in _lib.RtpSceneDesc._fields_ if issubclass(t, ctypes._Pointer)]
    assert sorted(pointers) == sorted(sizes)
    for f, n in sizes.items():
        a = np.ctypeslib.as_array(getattr(got, f), shape=(n,))
        b = np.ctypeslib.as_array(getattr(want, f), shape=(n,))
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), f
    assert list(got.light_quad_points) == list(want.light_quad_points)
    assert got.light_sphere_point == want.light_sphere_point
    assert np.float32(got.ior).tobytes() == np.float32(want.ior).tobytes()


def test_abi_version():
    import raytracingtherestofyourlife_amd as rtp

    assert rtp.load().rtp_abi_version() == 3


def test_create_without_gpu_fails_cleanly():
    import torch

    import raytracingtherestofyourlife_amd as rtp

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(rtp.RtpError) as e:
        rtp.Device(0)
    assert e.value.status == -3


@pytest.mark.parametrize("variant", [0, 1, 2, 3])
def test_product_cornell_box_equals_oracle(oracle, variant):
    import raytracingtherestofyourlife_amd as rtp

    cb = rtp.CornellBox(variant)
    cb.buildDataSet()
    o = oracle.cornell_box(variant)
    assert np.array_equal(cb.coord.view(np.uint32), o.points_np().view(np.uint32))
    assert np.array_equal(cb.ds.cellset.quad_points, o.quad_ids_np()[:, 1:])
    assert np.array_equal(cb.matIdx[0], np.ctypeslib.as_array(o.quad_mat)[: o.n_quads])
    assert np.array_equal(cb.texIdx[0], np.ctypeslib.as_array(o.quad_tex)[: o.n_quads])
    ns = o.n_spheres
    assert cb.ds.cellset.sphere_points.tolist() == list(o.sphere_point[:ns])
    assert np.array_equal(cb.SphereRadii.view(np.uint32), np.ctypeslib.as_array(o.sphere_radius)[:ns].view(np.uint32))
    assert np.array_equal(cb.matIdx[1], np.ctypeslib.as_array(o.sphere_mat)[:ns])
    assert np.array_equal(cb.texIdx[1], np.ctypeslib.as_array(o.sphere_tex)[:ns])
    assert list(cb.light_quad_points) == list(o.light_box_pointids[1:5])
    assert cb.light_sphere_point == o.light_sphere_point
    assert np.array_equal(cb.tex.view(np.uint32), np.ctypeslib.as_array(o.tex)[:4].view(np.uint32))
    assert cb.matType.tolist() == [0, 0, 0, 1, 2] and cb.texType.tolist() == [0, 1, 2, 3, 0]


def test_bad_cornell_variant():
    import raytracingtherestofyourlife_amd as rtp

    d = rtp._lib.RtpSceneDesc()
    assert rtp.load().rtp_cornell_box(7, ctypes.byref(d)) == -1
    assert rtp.load().rtp_cornell_box(4, ctypes.byref(d)) == -1


def test_normalize_matches_oracle(oracle):
    import raytracingtherestofyourlife_amd as rtp

    rng = np.random.default_rng(0)
    x = rng.random((1000, 4), dtype=np.float32) * 50
    x[::7, 1] = np.nan
    x[::11, 0] = np.inf
    want = oracle.normalize(x, 10)
    got = rtp.normalize(x.copy(), 10)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) or np.allclose(got, want, equal_nan=True)
    assert np.array_equal(np.isnan(got), np.isnan(want))


def test_write_pnm_format(tmp_path):
    import raytracingtherestofyourlife_amd as rtp

    c = np.array([[0.5, 1.0, 0.0, 0.0], [np.nan, 0.2, 0.3, 1.0], [1.2, 0.0, 0.999, 0.0]], dtype=np.float32)
    p = str(tmp_path / "o.pnm")
    rtp.save_pnm(p, c, 3, 1)
    lines = open(p).read().splitlines()
    assert lines[0] == "P3" and lines[1] == "3 1 255"
    assert lines[2:] == ["127 255 0", "0 0 0", "307 0 255"]  # unclamped int(255.99*c), NaN pixel -> 0


def test_package_refuses_to_run_without_library(tmp_path, monkeypatch):
    import raytracingtherestofyourlife_amd._lib as L

    monkeypatch.setattr(L, "LIB_PATH", str(tmp_path / "missing.so"))
    monkeypatch.setattr(L, "_lib", None)
    with pytest.raises(RuntimeError):
        L.load(build_if_missing=False)


def test_pool_kernel_reads_kparams_at_its_kernarg_offset(tmp_path):
    """rtp_render_pool re-reads KParams through the kernarg segment pointer at
    byte offset kKParamsOffset = 8 (rtp_pool.hpp kparams()): check that
    against the argument metadata of the gfx950 code object in librtp.so."""
    import shutil

    import raytracingtherestofyourlife_amd as rtp

    llvm = "/opt/rocm/lib/llvm/bin"
    tools = [shutil.which("objcopy"), os.path.join(llvm, "clang-offload-bundler"), os.path.join(llvm, "llvm-readelf")]
    if not all(t and os.path.exists(t) for t in tools):
        pytest.skip("objcopy / clang-offload-bundler / llvm-readelf not available")
    fat, co = str(tmp_path / "fat.bin"), str(tmp_path / "co.o")
    # (on a copy: objcopy without an output file rewrites its input in place,
    # which would replace the loaded product library under the running process)
    lib = str(tmp_path / "librtp_copy.so")
    shutil.copyfile(rtp.LIB_PATH, lib)
    subprocess.run([tools[0], "--dump-section", f".hip_fatbin={fat}", lib], check=True, capture_output=True)
    subprocess.run([tools[1], "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fat}",
                    f"--output={co}", "--unbundle"], check=True, capture_output=True)
    notes = subprocess.run([tools[2], "--notes", co], check=True, capture_output=True, text=True).stdout
    blocks = re.split(r"\n\s*-?\s*\.args:", notes)
    seen = 0
    for i in range(1, len(blocks)):
        # the kernel a .args list belongs to: the next .name after it
        name = re.search(r"\.name:\s+(\S+)", blocks[i])
        if not name or "rtp_render_pool" not in name.group(1):
            continue
        offsets = [int(x) for x in re.findall(r"\.offset:\s+(\d+)", blocks[i].split(".name:")[0])]
        sizes = [int(x) for x in re.findall(r"\.size:\s+(\d+)", blocks[i].split(".name:")[0])]
        assert offsets[:2] == [0, 8] and sizes[1] >= 200, (name.group(1), offsets[:3], sizes[:3])
        seen += 1
    assert seen >= 6, f"found {seen} rtp_render_pool kernels"
