"""Host-side logic that needs no GPU: struct layouts, presets, tile layout, the C-ABI
library's exported symbols, error behaviour."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import raytracingpbr_amd as rt
from raytracingpbr_amd import _capi
from raytracingpbr_amd.config import Config
from raytracingpbr_amd.tiles import TileLayout, default_tile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_struct_layouts_match_header():
    assert C.sizeof(Config) == 164
    assert C.sizeof(rt.Ray) == 40 and C.sizeof(rt.Material) == 40 and C.sizeof(rt.Transform) == 72
    assert C.sizeof(rt.SDFObject) == 116 and C.sizeof(rt.Camera) == 52
    # field order of Config == field order of rtpbr_config in include/rtpbr.h
    hdr = open(os.path.join(ROOT, "include", "rtpbr.h")).read()
    body = hdr[hdr.index("typedef struct rtpbr_config {"):hdr.index("} rtpbr_config;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for line in body.split("\n")[1:]:
        m = re.match(r"\s*(?:int32_t|uint32_t|float)\s+([^;]+);", line)
        if m:
            names += [n.strip() for n in m.group(1).split(",")]
    assert names == [n for n, _ in Config._fields_]


def test_presets_follow_reference_constants():
    c = Config.cornell_v3(512, 512)
    assert c.max_raymarch == 512 and c.max_raytrace == 3 and c.min_dis == pytest.approx(0.05)
    assert c.hit_eps == pytest.approx(0.5 / 512) and c.normal_h == pytest.approx(0.5773 * 0.005)
    assert c.light_quality == 128 and c.box_round == pytest.approx(0.01)
    s = Config.src()
    assert (s.width, s.height) == (768, 432) and s.kernel_form == rt.FORM.PERSISTENT_RAY
    assert s.hit_eps == pytest.approx(1 / 768) and s.min_dis == pytest.approx(2.5 / 768) and s.max_dis == 1e3
    assert s.vis_lo == pytest.approx(1e-4) and s.vis_hi == pytest.approx(1e4) and s.quality_per_sample == pytest.approx(0.8)
    b = Config.bunny_glass()
    assert b.max_raymarch == 2048 and b.omega0 == 0.5 and b.light_quality == 512 and b.exposure == pytest.approx(0.8)
    t = Config.tokyo_ibl()
    assert t.omega_guard == 0 and t.omega_fb_a == 0.5 and t.omega_fb_b == 0.5 and t.fresnel_kind == 1
    with pytest.raises(AttributeError):
        c.copy(no_such_field=1)


def test_tile_layout_partition():
    lay = TileLayout(100, 60, 16, 16, 3)
    assert lay.ntx == 7 and lay.nty == 4 and lay.n_tiles == 28 and lay.n_local_tiles == 10
    own = lay.owner_map()
    seen = np.zeros((100, 60), int)
    for r in range(3):
        x, y, v = lay.pixel_index(r)
        assert len(x) == lay.packed_pixels == 10 * 256
        assert np.all(own[x[v], y[v]] == r)
        seen[x[v], y[v]] += 1
    assert np.all(seen == 1)                         # every pixel owned exactly once
    img = np.random.default_rng(0).random((100, 60, 4)).astype(np.float32)
    out = np.zeros_like(img)
    for r in range(3):
        lay.unpack_into(out, lay.pack(img, r), r)
    assert np.array_equal(out, img)
    assert default_tile(1920, 1080, 1) == (1920, 1080)
    tw, th = default_tile(1920, 1080, 8)
    assert ((1920 + tw - 1) // tw) * ((1080 + th - 1) // th) >= 8 * 16


def test_hip_library_exports_every_declared_symbol():
    """The C-ABI library loads without a GPU and exports every function include/rtpbr.h
    declares (no compute calls here)."""
    assert os.path.exists(_capi.HIP_LIB_PATH), "build the HIP library first: python -m raytracingpbr_amd.build"
    hdr = open(os.path.join(ROOT, "include", "rtpbr.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = sorted(set(re.findall(r"\b(rtpbr_[a-z_]+)\s*\(", hdr)))
    assert len(declared) >= 24
    lib = C.CDLL(_capi.HIP_LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name
    assert sorted("rtpbr_" + n for n in _capi.ENTRY_POINTS) == declared
    lib.rtpbr_backend.restype = C.c_char_p
    assert lib.rtpbr_backend() == b"hip-gfx950"


def test_missing_library_fails_loudly(tmp_path):
    with pytest.raises(FileNotFoundError):
        _capi.CApi(str(tmp_path / "nope.so"))


def test_product_package_does_not_reference_the_oracle():
    """The oracle is test infrastructure: nothing under raytracingpbr_amd/ may mention it."""
    pkg = os.path.join(ROOT, "raytracingpbr_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".h")):
                txt = open(os.path.join(dp, f), errors="replace").read()
                assert "rt_oracle" not in txt and "librt_oracle" not in txt and "rto_" not in txt, os.path.join(dp, f)


def test_synthetic_env_is_deterministic():
    import hashlib
    from raytracingpbr_amd.ibl import preprocess, synthetic_env
    e = synthetic_env(384, 192)
    assert e.shape == (384, 192, 3) and e.dtype == np.uint8
    assert hashlib.sha1(e.tobytes()).hexdigest() == "2606c581d11bcf02e1cd7047fa6ba08fa0f64640"
    p = preprocess(e, 1.4, 2.2)
    assert p.dtype == np.float32 and p.max() == pytest.approx(1.4 ** 2.2, rel=1e-5)   # 2.10


def _signature(scene):
    """Host-only hook of the HIP library (no device call): signature + packed march table."""
    lib = C.CDLL(_capi.HIP_LIB_PATH)
    f = lib.rtpbr_test_signature
    f.restype = C.c_int
    objs = (rt.SDFObject * 8)(*scene.objects)
    sig = C.c_uint32(123)
    table = (C.c_float * 128)()
    assert f(objs, 8, int(scene.scale10), C.byref(sig), table) == 0
    return sig.value, np.array(table, dtype=np.float32)


def test_rotation_signature_and_packed_table():
    """rtpbr_set_scene's host logic for 8-box scenes: the Cornell layouts (and anything made of
    identity / matching single-axis rotations) get the listed signature 0x4db691 and a packed table
    that holds exactly the dwords each class reads; a rotation about another axis, a tilted box or a
    non-box shape fall back to the general instance (signature 0, plain 64-byte blocks)."""
    CORNELL = 0x4DB691          # classes I X X Y Y Y Y X, 3 bits per object (rt_types.hpp)
    for variant in ("v1", "v2", "v3", "shortest"):
        assert _signature(rt.cornell_box(variant))[0] == CORNELL
    sc = rt.cornell_box("v3")
    for o in sc.objects:
        o.transform.rotation[:] = (0, 0, 0)
    assert _signature(sc)[0] == CORNELL                       # an identity fits every single-axis class
    sc = rt.cornell_box("v3")
    sc.objects[3].transform.rotation[:] = (0, 0, 30)          # z-rotation in a slot specialised for y
    assert _signature(sc)[0] == 0
    sc = rt.cornell_box("v3")
    sc.objects[5].transform.rotation[:] = (10, -253, 5)       # tilted block
    assert _signature(sc)[0] == 0
    sc = rt.cornell_box("v3")
    sc.objects[6].type = int(rt.SHAPE.SPHERE)
    assert _signature(sc)[0] == 0

    # packed layout: identity 8 dwords [pos, size, -, -]; X / Y 12 dwords [pos, 4 matrix entries, size, -, -]
    sc = rt.cornell_box("v3")
    sig, tab = _signature(sc)
    objs = sc.objects
    s10 = 10.0 if sc.scale10 else 1.0
    off = 0
    cls = [(sig >> (3 * i)) & 7 for i in range(8)]
    assert cls == [1, 2, 2, 3, 3, 3, 3, 2]
    for i, o in enumerate(objs):
        pos = np.array(list(o.transform.position), np.float32) * np.float32(s10)
        size = np.array(list(o.transform.scale), np.float32) * np.float32(s10)
        assert np.array_equal(tab[off:off + 3], pos)
        if cls[i] == 1:
            assert np.array_equal(tab[off + 3:off + 6], size)
            off += 8
        else:
            assert np.array_equal(tab[off + 7:off + 10], size)
            m = tab[off + 3:off + 7]
            ang = np.deg2rad(o.transform.rotation[0] if cls[i] == 2 else o.transform.rotation[1])
            # X: m4 m5 m7 m8 = c s -s c;  Y: m0 m2 m6 m8 = c -s s c  (row-major world->local)
            want = [np.cos(ang), np.sin(ang), -np.sin(ang), np.cos(ang)] if cls[i] == 2 else \
                   [np.cos(ang), -np.sin(ang), np.sin(ang), np.cos(ang)]
            assert np.allclose(m, want, atol=1e-6), (i, m, want)
            off += 12
    assert off == 8 + 7 * 12 and np.all(tab[off:] == 0)
    # signature 0: plain blocks (position, 9 matrix entries, size, type)
    sc.objects[5].transform.rotation[:] = (10, -253, 5)
    sig, tab = _signature(sc)
    assert sig == 0
    blk = tab.reshape(8, 16)
    assert np.array_equal(blk[0, :3], np.array([0, 0, -10], np.float32)) and np.array_equal(blk[0, 3:12], np.eye(3, dtype=np.float32).ravel())
    assert blk[:, 15].view(np.int32).tolist() == [int(rt.SHAPE.BOX)] * 8


def test_smooth_camera_moving_refresh_contract():
    """src/camera.py:82-112: pose eases by clamp(velocity*dt,0,1) of the difference per frame; moving = any
    component still differs by > 1e-3 (measured BEFORE the step); src/renderer.py:26-27 refreshes while moving."""
    from raytracingpbr_amd.camera import SmoothCamera
    s = SmoothCamera().init((0, -0.2, 4.0))
    assert s.update(1 / 60, (0, -0.2, 4.0), (0, 0, 1), (0, 1, 0)) is False and s.frame == 1
    moved = []
    for _ in range(200):
        moved.append(s.update(1 / 60, (1.0, -0.2, 4.0), (0, 0, 1), (0, 1, 0)))
    assert moved[0] is True and moved[-1] is False                 # converges geometrically, then comes to rest
    n = moved.index(False)
    assert all(moved[:n]) and not any(moved[n:])
    # one step covers 10/60 of the remaining distance: after k steps the residual is (5/6)^k
    t = SmoothCamera().init((0, 0, 0))
    t.update(1 / 60, (6.0, 0, 0), (0, 0, 1), (0, 1, 0))
    assert abs(float(t.position[0]) - 1.0) < 1e-6
    # dt large: clamp to 1 -> jumps to the target
    t.update(1.0, (6.0, 0, 0), (0, 0, 1), (0, 1, 0))
    assert float(t.position[0]) == 6.0


def test_render_interactive_frame_refreshes_while_moving():
    from raytracingpbr_amd import Config, src_scene
    from raytracingpbr_amd.camera import SmoothCamera, render_interactive_frame
    from raytracingpbr_amd.ibl import synthetic_env
    from oracle_backend import OracleRenderer
    r = OracleRenderer(src_scene(aspect=48 / 27), Config.src(48, 27, 0))
    r.set_env(synthetic_env(64, 32), 1.4, 2.2)
    s = SmoothCamera().init((0, -0.2, 4.0))
    counts = []
    for f in range(40):
        tgt = (0.5, -0.2, 4.0) if 5 <= f else (0, -0.2, 4.0)
        s.update(1 / 60, tgt, (0, 0, 1), (0, 1, 0))
        render_interactive_frame(r, s, refreshing=(f == 0))
        counts.append(float(r.image_buffer[..., 3].max()))
    # deposits accumulate while at rest, drop to (almost) nothing each frame while the pose moves, grow again after
    assert counts[4] >= 1 and min(counts[6:20]) <= 1 and counts[-1] >= counts[25]


def test_run_time_instance_compiles_without_a_gpu(tmp_path, monkeypatch):
    """rt_jit.hip: hipcc --genco of rt_jit_tu.hip for a scene key (here the 7-object Tokyo scene: 4 spheres, 2 boxes,
    1 cylinder, all rotations identity) lands in the cache directory; a second request is a cache hit."""
    import ctypes as C
    import time
    from raytracingpbr_amd import _capi
    monkeypatch.setenv("RTPBR_JIT_CACHE", str(tmp_path))
    lib = C.CDLL(_capi.HIP_LIB_PATH)
    f = lib.rtpbr_test_jit_build
    f.argtypes = [C.c_int, C.c_int, C.c_ulonglong, C.c_uint, C.c_int, C.c_int, C.c_char_p, C.c_size_t]
    buf = C.create_string_buffer(512)
    t0 = time.time()
    assert f(0, 7, 0x4332222, 0x249249, 1, 5, buf, 512) == 0, lib.rtpbr_last_error()
    t_build = time.time() - t0
    path = buf.value.decode()
    assert path.startswith(str(tmp_path)) and os.path.getsize(path) > 10000
    assert open(path, "rb").read(4) in (b"\x7fELF", b"__CL")       # code object, or clang offload bundle around it
    t0 = time.time()
    assert f(0, 7, 0x4332222, 0x249249, 1, 5, buf, 512) == 0 and buf.value.decode() == path
    assert time.time() - t0 < 0.5 <= max(t_build, 0.5)
    # no compiler: a clear error for a key that is not cached (the library then keeps its ahead-of-time instance)
    monkeypatch.setenv("HIPCC", "/nonexistent/hipcc")
    lib.rtpbr_last_error.restype = C.c_char_p
    assert f(0, 3, 0x222, 0x49, 1, 5, buf, 512) != 0 and b"run-time compilation failed" in lib.rtpbr_last_error()


def test_run_time_compilation_survives_an_unwritable_home(monkeypatch):
    """A home directory the process cannot write to must not cost the specialised kernels: the cache falls back to a
    per-user directory under /tmp (CPU-only: builds one code object)."""
    import shutil
    from raytracingpbr_amd import _capi
    monkeypatch.delenv("RTPBR_JIT_CACHE", raising=False)
    monkeypatch.delenv("XDG_CACHE_HOME", raising=False)
    monkeypatch.setenv("HOME", "/proc/1/no-such-home")
    lib = C.CDLL(_capi.HIP_LIB_PATH)
    f = lib.rtpbr_test_jit_build
    f.argtypes = [C.c_int, C.c_int, C.c_ulonglong, C.c_uint, C.c_int, C.c_int, C.c_char_p, C.c_size_t]
    lib.rtpbr_last_error.restype = C.c_char_p
    buf = C.create_string_buffer(512)
    assert f(0, 2, 0x32, 0x9, 1, 5, buf, 512) == 0, lib.rtpbr_last_error()
    path = buf.value.decode()
    want = "/tmp/rtpbr-cache-%d/" % os.getuid()
    assert path.startswith(want) and os.path.getsize(path) > 10000
    st = os.stat(want)
    assert st.st_uid == os.getuid() and (st.st_mode & 0o077) == 0            # created private (0700)
    assert (os.stat(path).st_mode & 0o022) == 0
    shutil.rmtree(want, ignore_errors=True)


def _jit_build(lib):
    f = lib.rtpbr_test_jit_build
    f.argtypes = [C.c_int, C.c_int, C.c_ulonglong, C.c_uint, C.c_int, C.c_int, C.c_char_p, C.c_size_t]
    lib.rtpbr_last_error.restype = C.c_char_p
    return f


def test_run_time_cache_refuses_directories_and_files_others_can_write(tmp_path, monkeypatch):
    """A code object runs inside the caller's GPU context, so the cache is only used when nobody else can have put it there
    (ADVICE round 2): a group/world-writable cache directory, a symlinked one, and a cached file that others can write
    are all refused — no compilation into them, no load from them."""
    from raytracingpbr_amd import _capi
    lib = C.CDLL(_capi.HIP_LIB_PATH)
    f = _jit_build(lib)
    buf = C.create_string_buffer(512)
    # (1) directory writable by others
    bad = tmp_path / "shared"
    bad.mkdir()
    os.chmod(bad, 0o777)
    monkeypatch.setenv("RTPBR_JIT_CACHE", str(bad))
    assert f(0, 2, 0x32, 0x9, 1, 5, buf, 512) != 0 and b"run-time compilation is off" in lib.rtpbr_last_error()
    assert os.listdir(bad) == []
    # (2) a symlink where the directory should be (somebody else's target)
    real = tmp_path / "real"
    real.mkdir(mode=0o700)
    link = tmp_path / "link"
    os.symlink(real, link)
    monkeypatch.setenv("RTPBR_JIT_CACHE", str(link))
    assert f(0, 2, 0x32, 0x9, 1, 5, buf, 512) != 0 and os.listdir(real) == []
    # (3) a private directory works, and is created 0700 when missing
    good = tmp_path / "good" / "rtpbr"
    monkeypatch.setenv("RTPBR_JIT_CACHE", str(good))
    assert f(0, 2, 0x32, 0x9, 1, 5, buf, 512) == 0, lib.rtpbr_last_error()
    path = buf.value.decode()
    assert path.startswith(str(good)) and (os.stat(good).st_mode & 0o077) == 0
    # (4) the cached file made writable by others is no longer trusted: it is rebuilt (new inode, private mode), not loaded
    os.chmod(path, 0o666)
    ino = os.stat(path).st_ino
    assert f(0, 2, 0x32, 0x9, 1, 5, buf, 512) == 0 and buf.value.decode() == path
    st = os.stat(path)
    assert (st.st_mode & 0o022) == 0 and st.st_ino != ino
    # (5) a symlink in place of the cached file is not followed
    os.unlink(path)
    other = tmp_path / "evil.hsaco"
    other.write_bytes(b"\x7fELF" + b"\0" * 20000)
    os.symlink(other, path)
    assert f(0, 2, 0x32, 0x9, 1, 5, buf, 512) == 0
    assert not os.path.islink(path) and other.read_bytes()[:4] == b"\x7fELF" and os.path.getsize(other) == 20004


def test_run_time_cache_is_bounded(tmp_path, monkeypatch):
    """RTPBR_JIT_CACHE_MAX: oldest code objects go when the cache holds more than that many."""
    from raytracingpbr_amd import _capi
    lib = C.CDLL(_capi.HIP_LIB_PATH)
    f = _jit_build(lib)
    buf = C.create_string_buffer(512)
    monkeypatch.setenv("RTPBR_JIT_CACHE", str(tmp_path))
    monkeypatch.setenv("RTPBR_JIT_CACHE_MAX", "2")
    for i in range(3):                                      # stale entries, oldest first
        q = tmp_path / ("old%d.hsaco" % i)
        q.write_bytes(b"x")
        os.utime(q, (1000 + i, 1000 + i))
    assert f(0, 2, 0x32, 0x9, 1, 5, buf, 512) == 0, lib.rtpbr_last_error()
    left = sorted(os.listdir(tmp_path))
    assert len(left) == 2 and os.path.basename(buf.value.decode()) in left and "old2.hsaco" in left


def test_c_abi_header_and_c_host_example_compile_as_plain_c(tmp_path):
    """include/rtpbr.h is the drop-in boundary: it must be usable from plain C (what cgo / JNI / a C host see).  The header
    and examples/c_host.c — the Cornell Box rendered through the C ABI without Python — compile as strict C99 and link
    against the library (no GPU needed to link; tests/test_gpu_examples.py runs it)."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib_dir = os.path.dirname(_capi.HIP_LIB_PATH)
    exe = str(tmp_path / "c_host")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-O1", "-I" + os.path.join(root, "include"),
                        os.path.join(root, "examples", "c_host.c"), "-L" + lib_dir, "-lrtpbr_hip", "-Wl,-rpath," + lib_dir, "-lm", "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert os.path.getsize(exe) > 8000


def test_catalog_serves_the_baseline_scenes_without_a_compiler(tmp_path, monkeypatch):
    """raytracingpbr_amd/prebuild.py + rt_jit.hip's catalog lookup (no GPU needed): with HIPCC pointing nowhere and an EMPTY
    code-object cache, the key rtpbr_sample() would form for a BASELINE scene as bench.py sets it up resolves to the code
    object compiled at build time (raytracingpbr_amd/data/jit); a scene that is not in the catalog fails loudly (no compiler),
    and a hidden catalog makes the catalog scene fail the same way."""
    from raytracingpbr_amd import prebuild
    cat = prebuild.prebuild(prebuild.DEFAULT + prebuild.FAST)          # (a lookup per entry when build() has run; compiles otherwise)
    assert len(cat) == len(prebuild.DEFAULT) + len(prebuild.FAST) and len(set(cat.values())) == len(cat)
    assert all(os.path.dirname(os.path.realpath(p)) == os.path.realpath(prebuild.CATALOG_DIR) and os.path.getsize(p) > 10000 for p in cat.values())
    monkeypatch.setenv("HIPCC", "/nonexistent/hipcc")
    monkeypatch.setenv("RTPBR_JIT_CACHE", str(tmp_path))
    lib = prebuild._lib()
    for name, wl, dims, world, opts in (prebuild.DEFAULT[0], prebuild.DEFAULT[4], prebuild.DEFAULT[9], prebuild.DEFAULT[12], prebuild.FAST[0]):
        got = prebuild.prebuild_one(lib, wl, dims, world, opts)
        assert os.path.realpath(got) == os.path.realpath(cat[name]), name
    assert not os.listdir(tmp_path)                                    # nothing was compiled, nothing was cached
    with pytest.raises(RuntimeError):
        prebuild.prebuild_one(lib, "c2", (800, 600), 1, "jit=1 jit_bake=2")     # not a catalog scene: needs the compiler
    monkeypatch.setenv("RTPBR_JIT_CATALOG", str(tmp_path / "nowhere"))
    with pytest.raises(RuntimeError):
        prebuild.prebuild_one(lib, "c2", (0, 0), 1, "jit=1 jit_bake=2")


def test_bench_dump_outputs_samples_a_large_frame_the_same_way_every_time(tmp_path, monkeypatch):
    """bench.py --dump-outputs: a frame within the size cap is written whole; a larger one as a fixed, seeded sample of its
    pixels with their flat indices — the same pixels in every run, so that two builds compare output for output."""
    import importlib.util
    import types
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    img = np.random.default_rng(1).random((64, 48, 4), dtype=np.float32)
    r = types.SimpleNamespace(image_buffer=img)
    bench.dump_outputs(r, str(tmp_path / "whole"))
    assert np.array_equal(np.load(tmp_path / "whole" / "image_buffer.npy"), img)
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", img.nbytes // 4)
    for d in ("a", "b"):
        bench.dump_outputs(r, str(tmp_path / d))
        assert not os.path.exists(tmp_path / d / "image_buffer.npy")
    sizes = 0
    for name in ("image_buffer_sample.npy", "image_buffer_sample_pixel.npy"):
        a, b = np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b)
        sizes += a.nbytes
    assert sizes <= img.nbytes // 4
    vals = np.load(tmp_path / "a" / "image_buffer_sample.npy")
    pix = np.load(tmp_path / "a" / "image_buffer_sample_pixel.npy").astype(np.int64)
    assert len(np.unique(pix)) == len(pix) > 0 and np.array_equal(vals, img.reshape(-1, 4)[pix])


# rtpbr_set_option, key by key: (key, lowest accepted value, highest accepted value or None, the refusal's message)
OPTION_BOUNDS = [
    ("staging_bytes", 1 << 20, None, "staging_bytes must be >= 1 MiB"),
    ("wait_lanes", 1, 64, "wait_lanes must be 1..64"),
    ("shade_lanes", 1, 64, "shade_lanes must be 1..64"),
    ("jit_waves", 0, 8, "jit_waves must be 0 (default) .. 8"),
    ("chunk", 0, 8192, "chunk must be 0 (automatic) .. 8192"),
    ("sparse_lanes", 0, 64, "sparse_lanes must be 0 (never) .. 64"),
    ("src_plan", 0, 1, "src_plan must be 0 or 1"),
    ("plan_interval", 1, 1 << 20, "plan_interval must be 1 .. 2^20 bounce-steps"),
    ("heavy_own", 0, 128, "heavy_own must be 0 (no heavy waves) .. 128"),
    ("src_chain", 0, 2, "src_chain must be 0 (never), 1 (when the device has room beside the pool kernel) or 2 (always: tests)"),
    ("chain_np_max", 0, None, "chain_np_max must be >= 0"),
    ("chain_waves", 1, 2048, "chain_waves must be 1 .. 2048"),
    ("src_split", 0, 256, "src_split must be 0 (never) .. 256 (bounce-steps per launch up to which the wavefront split runs)"),
    ("env_packed", 0, 1, "env_packed must be 0 (float4 texels) or 1 (RGBA8 texels + 256-entry table: 8-bit sources, same values)"),
    ("src_lazy", 0, 1, "src_lazy must be 0 (every one-step launch shades) or 1 (the shading rides with the next launch's gen pass)"),
    ("split_head", -1, 1, "split_head must be -1 (automatic: small frames), 0 (the heavy head fills the first groups) or 1 (interleaved: one head entry per group)"),
    ("split_wait", 1, 64, "split_wait must be 1..64"),
    ("src_track", 0, 2, "src_track must be 0 (never), 1 (one-object bounds only) or 2 (one- and two-object bounds)"),
    ("src_op", 0, 7, "src_op must be 0 .. 7 (bit 0: object-parallel evaluation for sparse waves in the split march and chain kernels, bit 1: in the fused pool kernel, bit 2: the per-lane lean loop for lanes that track different objects)"),
    ("age_weights", 0, 0xffffffff, "age_weights must be 0 (off) or up to 8 hex digits, one per residency slot"),
    ("age_tune", 0, 1, "age_tune must be 0 (equal shares) or 1 (self-tuned age-weighted shares)"),
    ("tiny_waves", 0, 65535, "tiny_waves must be 0 .. 65535"),
    ("tiny_own", 0, 128, "tiny_own must be 0 (no small heavy waves) .. 128"),
    ("leave_x8", 1, 4096, "leave_x8 must be 1 .. 4096 (eighths of a march iteration)"),
    ("heavy_prio", 0, 1, "heavy_prio must be 0 or 1"),
    ("heavy_mean_x16", 0, 1 << 20, "heavy_mean_x16 must be 0 .. 2^20"),
    ("heavy_bulk_x16", 0, 1 << 20, "heavy_bulk_x16 must be 0 .. 2^20"),
    ("grid_blocks", 0, 65535, "grid_blocks must be 0 (automatic) .. 65535"),
    ("residency", 1, 256, "residency must be a power of two, 1..256"),
    ("ready_low", 0, 63, "ready_low must be 0..63"),
    ("refill_lanes", 1, 64, "refill_lanes must be 1..64"),
    ("timing", 0, 1, "timing must be 0 or 1"),
    ("stage_dense", 0, 1, "stage_dense must be 0 (item-linear staging) or 1 (records appended per claim in completion order)"),
    ("primary_split", 0, 2, "primary_split must be 0 (never), 1 (large launches) or 2 (always)"),
    ("drain_lanes", 0, 64, "drain_lanes must be 0..64"),
    ("primary_lean", 0, 1, "primary_lean must be 0 or 1"),
    ("lazy_sqrt", 0, 1, "lazy_sqrt must be 0 or 1"),
    ("jit", -1, 2, "jit must be -1 (when no ahead-of-time specialisation fits), 0 (never), 1 (always, falling back to the ahead-of-time instance if compilation is impossible) or 2 (always, an error otherwise)"),
    ("precision", 0, 1, "precision must be 0 (exactly rounded, the default) or 1 (tolerance flavour: hardware sqrt / rcp / sin / exp, contraction)"),
    ("jit_bake", 0, 2, "jit_bake must be 0, 1 (scene + configuration) or 2 (+ the camera frame: fixed-camera offline renders)"),
    ("specialize", 0, 1, "specialize must be 0 or 1"),
    ("mlp_mfma", 0, 1, "mlp_mfma must be 0 or 1"),
    ("mlp_lanes", 1, 64, "mlp_lanes must be 1..64"),
    ("mlp_full", 1, 65, "mlp_full must be 1..65 (65 = never compute both halves at once)"),
    ("swap_lanes", 0, 64, "swap_lanes must be 0 (automatic: 8 in the complete-path pool kernel, 12 in the src/ one) .. 64"),
    ("scheduler", -1, 1, "scheduler must be -1 (auto), 0 or 1"),
    ("waves_per_cu", 0, 32, "waves_per_cu must be 0..32"),
]


def test_every_option_keeps_its_bounds_and_messages(tmp_path, monkeypatch):
    """rtpbr_set_option on a context without a device: rtpbr_jit_prebuild applies its "key=value ..." string with it before
    anything is compiled, so "key=value nosuchkey=0" answers "unknown option nosuchkey" exactly when the first pair was
    accepted, and the pair's own message when it was refused.  Every key's lowest and highest value is accepted, the values
    next to them are refused in the key's own words.  sample_base takes any value; reserve_spp's accepted values allocate
    (they need a device): its refusal is checked."""
    from raytracingpbr_amd import prebuild, workloads
    from raytracingpbr_amd.dataclass import SDFObject
    monkeypatch.setenv("HIPCC", "/nonexistent/hipcc")          # (a mistake in this test cannot start a compiler)
    monkeypatch.setenv("RTPBR_JIT_CACHE", str(tmp_path))
    lib = prebuild._lib()
    wl = workloads.get("c2", 0, 0)
    n = len(wl.scene.objects)
    arr = (SDFObject * n)(*wl.scene.objects)
    buf = C.create_string_buffer(1024)

    def answer(options):
        rc = lib.rtpbr_jit_prebuild(arr, n, 1 if wl.scene.scale10 else 0, C.byref(wl.cfg), C.byref(wl.scene.camera), 0, 0, 1,
                                    options.encode(), buf, 1024)
        return rc, lib.rtpbr_last_error().decode()

    EINVAL = -1
    unknown = (EINVAL, "unknown option nosuchkey")
    assert answer("wait_lanes=65") == (EINVAL, "wait_lanes must be 1..64")
    assert answer("wait_lanes=64 nosuchkey=0") == unknown
    for key, lo, hi, msg in OPTION_BOUNDS:
        assert answer("%s=%d nosuchkey=0" % (key, lo - 1)) == (EINVAL, msg), key
        assert answer("%s=%d nosuchkey=0" % (key, lo)) == unknown, key
        if hi is not None:
            assert answer("%s=%d nosuchkey=0" % (key, hi)) == unknown, key
            assert answer("%s=%d nosuchkey=0" % (key, hi + 1)) == (EINVAL, msg), key
    for value in (1 << 40, 1 << 62):                           # the two 64-bit options have no upper bound
        assert answer("staging_bytes=%d nosuchkey=0" % value) == unknown
        assert answer("chain_np_max=%d nosuchkey=0" % value) == unknown
    for value in (-1, 0, 12345, 0xffffffff):
        assert answer("sample_base=%d nosuchkey=0" % value) == unknown
    assert answer("residency=48") == (EINVAL, "residency must be a power of two, 1..256")
    assert answer("age_weights=-1") == (EINVAL, "age_weights must be 0 (off) or up to 8 hex digits, one per residency slot")
    assert answer("chain_np_max=-1") == (EINVAL, "chain_np_max must be >= 0")
    assert answer("staging_bytes=5") == (EINVAL, "staging_bytes must be >= 1 MiB")
    assert answer("jit=3")[1].startswith("jit must be -1 (when no ahead-of-time specialisation fits)")
    assert answer("reserve_spp=0") == (EINVAL, "reserve_spp must be >= 1")
    assert len(OPTION_BOUNDS) + 2 == 49 and len({k for k, _, _, _ in OPTION_BOUNDS}) == len(OPTION_BOUNDS)
    assert not os.listdir(tmp_path)                            # nothing was compiled
