"""GPU parity tests (run with -m gpu on an MI355X): the HIP path, called through the C ABI,
against the CPU oracle on the same seeded inputs and against the committed golden fixtures.

Bar (north star): integer work bit-exact; radiance per-pixel L2 < 1e-3.  What is asserted is
stronger: image_buffer (T7) is BIT-IDENTICAL to the oracle, because both sides use the same
exactly-rounded operation sequence and the same counter-based random stream; image_pixels
(T8) agrees to 1e-5 in display space (powf is libm on the host, ocml on the device).
"""
import ctypes as C

import os

import numpy as np
import pytest

from cases import all_cases, case_by_name, fingerprint
from oracle_backend import OracleRenderer, oracle_api
from raytracingpbr_amd import Config, Renderer, cornell_box
from raytracingpbr_amd._capi import RtpbrError, hip_api
from raytracingpbr_amd.tiles import TileLayout
from test_oracle_golden import check_fingerprint

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def l2(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


def test_backend_is_the_hip_library():
    assert hip_api().backend() == "hip-gfx950"


@pytest.mark.parametrize("case", all_cases(), ids=lambda c: c.name)
def test_hip_matches_oracle_bit_exact(case):
    g = Renderer(case.scene, case.cfg)
    o = OracleRenderer(case.scene, case.cfg)
    case.run(g)
    case.run(o)
    a, b = g.image_buffer, o.image_buffer
    cg, co = g.counters(), o.counters()
    assert (cg.samples, cg.raycasts, cg.march_steps, cg.hits, cg.sky_lookups, cg.deposits) == \
           (co.samples, co.raycasts, co.march_steps, co.hits, co.sky_lookups, co.deposits)
    assert np.array_equal(bits(a), bits(b)), f"{int((a != b).any(axis=2).sum())} pixels differ, max {np.abs(a - b).max()}"
    if case.cfg.kernel_form == 1:
        assert np.array_equal(bits(g.ray_buffer), bits(o.ray_buffer))
    # the display transform uses the exactly specified pow_ on both sides -> image_pixels is bit-exact
    # too (NaN patterns included: ACES->gamma variants produce NaN for negative ACES values)
    assert np.array_equal(bits(g.image_pixels), bits(o.image_pixels))
    if case.cfg.adaptive_sampling:
        assert np.array_equal(bits(g.diff_pixels), bits(o.diff_pixels))
        assert np.array_equal(bits(g.diff_buffer), bits(o.diff_buffer))
    check_fingerprint(fingerprint(g), case.name)                   # and against the committed golden vectors
    if case.cfg.kernel_form == 0:
        # these frames are below the size where the primary raycasts get their own kernel: force it
        s = Renderer(case.scene, case.cfg)
        s.set_option("primary_split", 2)
        case.run(s)
        cs = s.counters()
        assert np.array_equal(bits(s.image_buffer), bits(a))
        assert (cs.raycasts, cs.march_steps, cs.hits, cs.sky_lookups) == (co.raycasts, co.march_steps, co.hits, co.sky_lookups)
        s.close()
    g.close()


def test_exact_math_functions_match_oracle_bitwise():
    api = hip_api()
    lib = oracle_api().lib
    g = Renderer(cornell_box("v3"), Config.cornell_v3(16, 16))
    rng = np.random.default_rng(7)
    n = 200000

    def gpu(op, a, b=None, two=False):
        a = np.ascontiguousarray(a, np.float32)
        out, out2 = np.empty_like(a), np.empty_like(a)
        bp = None if b is None else np.ascontiguousarray(b, np.float32).ctypes.data_as(C.c_void_p)
        api.call("test_math", g._ctx, op, a.ctypes.data_as(C.c_void_p), bp, out.ctypes.data_as(C.c_void_p),
                 out2.ctypes.data_as(C.c_void_p), a.size)
        return (out, out2) if two else out

    lib.rto_test_sincos.argtypes = [C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    lib.rto_test_exp.restype = C.c_float; lib.rto_test_exp.argtypes = [C.c_float]
    lib.rto_test_atan2.restype = C.c_float; lib.rto_test_atan2.argtypes = [C.c_float, C.c_float]
    lib.rto_test_asin.restype = C.c_float; lib.rto_test_asin.argtypes = [C.c_float]
    x = np.concatenate([rng.uniform(0, 6.2832, 3000), rng.uniform(-30, 30, 1000)]).astype(np.float32)
    s, c = gpu(0, x, two=True)
    rs, rc = C.c_float(), C.c_float()
    for i, v in enumerate(x):
        lib.rto_test_sincos(float(v), C.byref(rs), C.byref(rc))
        assert s[i] == rs.value and c[i] == rc.value, (v, s[i], rs.value)
    lib.rto_test_sin_pi.restype = C.c_float; lib.rto_test_sin_pi.argtypes = [C.c_float]
    x = rng.uniform(-40, 40, 4000).astype(np.float32)
    sp = gpu(7, x)
    assert all(sp[i] == lib.rto_test_sin_pi(float(v)) for i, v in enumerate(x))
    lib.rto_test_log.restype = C.c_float; lib.rto_test_log.argtypes = [C.c_float]
    lib.rto_test_pow.restype = C.c_float; lib.rto_test_pow.argtypes = [C.c_float, C.c_float]
    x = (10.0 ** rng.uniform(-30, 30, 3000)).astype(np.float32)
    lg = gpu(8, x)
    assert all(lg[i] == lib.rto_test_log(float(v)) for i, v in enumerate(x))
    x = rng.uniform(0, 20, 3000).astype(np.float32); yy = np.where(rng.random(3000) < 0.5, 1 / 2.2, 2.2).astype(np.float32)
    pw = gpu(9, x, yy)
    assert all(pw[i] == lib.rto_test_pow(float(x[i]), float(yy[i])) for i in range(len(x)))
    x = rng.uniform(-8, 8, 3000).astype(np.float32)
    e = gpu(1, x)
    assert all(e[i] == lib.rto_test_exp(float(v)) for i, v in enumerate(x))
    y, xx = rng.normal(size=3000).astype(np.float32), rng.normal(size=3000).astype(np.float32)
    a = gpu(2, y, xx)
    assert all(a[i] == lib.rto_test_atan2(float(y[i]), float(xx[i])) for i in range(len(y)))
    x = rng.uniform(-1, 1, 3000).astype(np.float32)
    a = gpu(3, x)
    assert all(a[i] == lib.rto_test_asin(float(v)) for i, v in enumerate(x))
    # correctly rounded sqrt and divide on the device == numpy float32 (IEEE)
    x = np.abs(rng.normal(size=n).astype(np.float32)) * np.float32(10.0) ** rng.integers(-20, 20, n).astype(np.float32)
    x[:8] = [0.0, 1e-45, 1e-40, 1.17549435e-38, 1.0, 2.0, 3.0, 1e28]      # domain of sqrt_: [0, 2^95)
    assert np.array_equal(bits(gpu(4, x)), bits(np.sqrt(x)))
    num, den = rng.normal(size=n).astype(np.float32), rng.normal(size=n).astype(np.float32)
    assert np.array_equal(bits(gpu(5, num, den)), bits(num / den))
    g.close()


def test_device_sqrt_is_correctly_rounded_exhaustively():
    """The kernels use a slimmed correctly-rounded sqrt (rt_math.hpp sqrt_); compare it with
    the compiler's IEEE sqrt for every float bit pattern in [0, 2^95) on the device."""
    api = hip_api()
    f = api.lib.rtpbr_test_sqrt_exhaustive
    f.restype, f.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_ulonglong)]
    g = Renderer(cornell_box("v3"), Config.cornell_v3(16, 16))
    bad = C.c_ulonglong(123)
    assert f(g._ctx, C.byref(bad)) == 0
    assert bad.value == 0
    g.close()


def test_schedule_independence():
    """Results must not depend on how lanes are scheduled: wait_lanes, occupancy, staging
    chunking and the split of spp into launches (K4) all give identical bits."""
    case = case_by_name("cornell_v3_8b_wide")
    ref = Renderer(case.scene, case.cfg)
    ref.sample(12)
    want = bits(ref.image_buffer)
    for opts in ({"scheduler": 0, "wait_lanes": 1}, {"scheduler": 0, "wait_lanes": 64},
                 {"scheduler": 0, "wait_lanes": 7, "waves_per_cu": 4}, {"scheduler": 0},
                 {"scheduler": 1, "shade_lanes": 1, "swap_lanes": 1}, {"scheduler": 1, "shade_lanes": 64, "swap_lanes": 64},
                 {"scheduler": 1, "shade_lanes": 33, "swap_lanes": 5, "waves_per_cu": 4},
                 {"refill_lanes": 1, "ready_low": 0}, {"refill_lanes": 64, "ready_low": 63}, {"ready_low": 17},
                 {"chunk": 64}, {"chunk": 8192}, {"chunk": 777, "primary_split": 2},
                 {"jit": 2, "jit_waves": 7}, {"jit": 2, "jit_bake": 1, "jit_waves": 4, "chunk": 96}, {"refill_lanes": 40, "shade_lanes": 20, "primary_split": 2},
                 {"staging_bytes": 1 << 20}, {"waves_per_cu": 1},
                 {"primary_split": 0}, {"primary_split": 2}, {"specialize": 0}, {"primary_split": 0, "specialize": 0},
                 {"primary_split": 2, "specialize": 0}, {"primary_split": 2, "staging_bytes": 1 << 20, "shade_lanes": 3},
                 {"lazy_sqrt": 0}, {"lazy_sqrt": 0, "specialize": 0, "scheduler": 0},
                 # the drain's culled wave march (round 5): never / for every wave once the work has run out; with and without its lean loop
                 {"drain_lanes": 0}, {"drain_lanes": 64}, {"drain_lanes": 64, "jit": 2, "chunk": 64}, {"drain_lanes": 3, "primary_lean": 0, "jit": 2, "jit_bake": 1},
                 {"stage_dense": 1, "jit": 1}, {"stage_dense": 1, "chunk": 48, "shade_lanes": 7, "jit": 2}):
        r = Renderer(case.scene, case.cfg)
        for k, v in opts.items():
            r.set_option(k, v)
        r.sample(12)
        assert np.array_equal(bits(r.image_buffer), want), opts
        c0, c1 = ref.counters(), r.counters()
        assert (c0.samples, c0.raycasts, c0.march_steps, c0.hits, c0.sky_lookups) == \
               (c1.samples, c1.raycasts, c1.march_steps, c1.hits, c1.sky_lookups), opts
        r.close()
    r = Renderer(case.scene, case.cfg)
    for n in (1, 4, 7):
        r.sample(n)
    assert np.array_equal(bits(r.image_buffer), want)
    assert np.all(r.image_buffer[..., 3] == 12.0)


def test_dense_staging_equals_item_linear_records_and_the_oracle():
    """Round 6: the pool kernel appends a claim's records in COMPLETION order (rt_trace.hpp stage_sample) and
    accumulate_dense puts them back in sample order.  Samples per launch that are whole multiples / whole fractions of the claim
    (and those that have no such claim size: 257, 5000 -> item-linear records; counter "dense_launches" says which), claims asked for, edge tiles with padding pixels,
    the separate primary kernel, run-time instances and the staging split into several launches: the bits of option
    stage_dense = 0, and — at 12 spp — the oracle's."""
    case = case_by_name("cornell_v3_8b_wide")
    sc, cfg = case.scene, case.cfg
    small = Config.cornell_v3(24, 16, 3, 8)
    small_sc = cornell_box("v3", aspect=24 / 16)
    o = OracleRenderer(sc, cfg); o.sample(12)
    for opts in ({}, {"primary_split": 2}, {"jit": 2, "jit_bake": 1}, {"chunk": 96, "primary_split": 2}, {"chunk": 36}, {"chunk": 240},
                 {"staging_bytes": 1 << 20}, {"shade_lanes": 3, "swap_lanes": 2, "refill_lanes": 1}, {"drain_lanes": 64, "waves_per_cu": 1}):
        r = Renderer(sc, cfg)
        r.set_option("stage_dense", 1); r.set_option("jit", 2)      # (compiled into run-time instances only)
        for k, v in opts.items():
            r.set_option(k, v)
        r.sample(12)
        assert r.counter("dense_launches") >= 1, opts
        assert np.array_equal(bits(r.image_buffer), bits(o.image_buffer)), opts
        assert r.counters().deposits == o.counters().deposits, opts
        r.close()
    for K in (1, 2, 3, 16, 64, 100, 255, 256, 257, 300, 512, 1000, 4096, 5000):
        imgs = []
        for dense in (0, 1):
            r = Renderer(small_sc, small)
            r.set_option("stage_dense", dense); r.set_option("jit", 2)
            if K % 2: r.set_option("primary_split", 2)
            r.set_tiles(16, 16, K % 2, 2)      # 24x16 in 16x16 tiles: the second column of tiles is half padding
            r.sample(K)
            assert r.counter("dense_launches") == (1 if dense and K not in (257, 5000) else 0), (K, dense)
            r.sample(3)                        # a second launch on top (another claim size)
            imgs.append(bits(r.image_buffer).copy())
            dep = r.counters().deposits
            r.close()
            assert dep == r_pixels(small, K % 2) * 3, (K, dense)       # (the work counters are those of the last call)
        assert np.array_equal(imgs[0], imgs[1]), K


def test_lazy_shading_of_one_step_launches_is_invisible():
    """Round 6: a one-step src/ launch leaves its shading to the next launch's gen pass (src_shade_gen: one pass over ray_buffer
    instead of two) and everything that could see the difference flushes it first.  A script of calls that interleaves one-step
    launches with every such observer — ray_buffer read / written / handed out, the counters, setters (camera, scene, config
    fields, tiles-free options), refresh, post_process, fused launches, a switch of n — on the HIP path with src_lazy 1 and 0 and
    on the oracle: ray_buffer, image_buffer and the counters agree bit for bit at every checkpoint."""
    from raytracingpbr_amd import Camera
    case = case_by_name("src_persistent")
    def script(r, hip, lazy):
        case.setup(r)
        if hip:
            r.set_option("src_lazy", lazy)
        out = []
        def check(tag, counters=True):
            out.append((tag, bits(r.ray_buffer).copy(), bits(r.image_buffer).copy()))
            if counters:
                c = r.counters()
                out.append((tag + ":ctr", (c.samples, c.raycasts, c.march_steps, c.hits, c.sky_lookups, c.deposits)))
        for _ in range(5): r.sample(1)                      # five launches, nothing looks in between
        check("five")
        for _ in range(3): r.sample(1)
        c = r.counters(); out.append(("ctr-only", (c.samples, c.hits, c.sky_lookups)))      # the counters alone flush
        r.sample(1); r.post_process(); r.sample(1)          # post_process does not need the shading
        out.append(("pixels", bits(r.image_pixels).copy()))
        check("after-post")
        r.sample(2); r.sample(1)                            # two steps in one call, then one
        cam = case.scene.camera
        r.set_camera(Camera(tuple(float(x) for x in np.array(tuple(cam.lookfrom)) + np.array([0.3, 0.1, 0.0])), tuple(cam.lookat), tuple(cam.vup), cam.vfov, cam.aspect, cam.aperture, cam.focus))
        r.sample(1); r.sample(1)
        check("camera")
        r.sample(1); r.refresh(); r.sample(1); r.sample(1)  # refresh must see the shaded colours (the next deposit adds them)
        check("refresh")
        r.sample(1)
        rb = r.ray_buffer                                   # read, modify, write back while a shading would be pending
        rb2 = rb.copy(); rb2[..., 6:9] *= 0.5
        r.sample(1)
        r.ray_buffer = rb2
        r.sample(1); r.sample(1)
        check("written")
        r.sample(1); r.sample(40)                           # a fused launch after a one-step launch: that one's shading must not count here
        c = r.counters(); out.append(("ctr-fused40", (c.samples, c.raycasts, c.march_steps, c.hits, c.sky_lookups, c.deposits)))
        r.sample(1); r.sample(3)                            # ... and three steps in one call: all three shadings count
        c = r.counters(); out.append(("ctr-three", (c.samples, c.raycasts, c.march_steps, c.hits, c.sky_lookups, c.deposits)))
        r.sample(1)
        check("fused")
        if hip:
            r.sample(1)
            r.device_ptr(2)                                 # ray_buffer handed out: shaded now, and with every launch from here on
        else:
            r.sample(1)
        r.sample(1); r.sample(1)
        check("handed-out")
        return out
    o = script(OracleRenderer(case.scene, case.cfg), False, 0)
    for lazy in (1, 0):
        g = script(Renderer(case.scene, case.cfg), True, lazy)
        assert len(g) == len(o)
        for a, b in zip(g, o):
            assert a[0] == b[0]
            for x, y in zip(a[1:], b[1:]):
                assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y, (lazy, a[0])


def test_lazy_shading_random_call_sequences():
    """Random sequences of API calls around one-step launches — launches of 1 / 2 / 40 steps, post_process, refresh, reads of every
    buffer, the counters, camera / option / scene setters, ray_buffer written back — with src_lazy 1 against src_lazy 0: everything
    observed is identical, observation by observation (the flush hooks of rt_capi.hip)."""
    from raytracingpbr_amd import Camera
    case = case_by_name("src_persistent")
    cam = case.scene.camera
    def run(seed, lazy):
        rng = np.random.default_rng(seed)
        r = Renderer(case.scene, case.cfg)
        case.setup(r)
        r.set_option("src_lazy", lazy)
        seen = []
        for _ in range(70):
            op = int(rng.integers(0, 14))
            if op <= 4: r.sample(1)
            elif op == 5: r.sample(2)
            elif op == 6: r.sample(40)
            elif op == 7: r.post_process(); seen.append(bits(r.image_pixels).copy())
            elif op == 8: r.refresh()
            elif op == 9: seen.append(bits(r.ray_buffer).copy())
            elif op == 10:
                c = r.counters(); seen.append((c.samples, c.raycasts, c.march_steps, c.hits, c.sky_lookups, c.deposits))
            elif op == 11:
                d = rng.uniform(-0.2, 0.2, 3)
                r.set_camera(Camera(tuple(float(x) for x in np.array(tuple(cam.lookfrom)) + d), tuple(cam.lookat), tuple(cam.vup), cam.vfov, cam.aspect, cam.aperture, cam.focus))
            elif op == 12:
                k = int(rng.integers(0, 3))
                if k == 0: r.set_option("split_wait", int(rng.integers(1, 40)))
                elif k == 1: r.set_scene(case.scene)
                else: seen.append(bits(r.image_buffer).copy())
            else:
                rb = r.ray_buffer; rb[..., 6:9] *= np.float32(0.75); r.ray_buffer = rb
        seen.append(bits(r.ray_buffer).copy()); seen.append(bits(r.image_buffer).copy())
        c = r.counters(); seen.append((c.samples, c.raycasts, c.march_steps, c.hits, c.sky_lookups, c.deposits))
        r.close()
        return seen
    for seed in range(6):
        a, b = run(seed, 1), run(seed, 0)
        assert len(a) == len(b)
        for i, (x, y) in enumerate(zip(a, b)):
            assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y, (seed, i)


def test_timing_option_only_removes_the_events():
    """Option timing = 0: rtpbr_sample() records no HIP events (bench.py times its small launches that way) — same bits in both
    kernel forms, rtpbr_last_sample_ms / rtpbr_last_primary_ms answer ESTATE until a timed call has run, and a timed call reports
    a total that covers its kernels."""
    for name, n in (("cornell_v3_8b_wide", 5), ("src_persistent", 3)):
        case = case_by_name(name)
        a = Renderer(case.scene, case.cfg); case.run(a)
        b = Renderer(case.scene, case.cfg); b.set_option("timing", 0); case.run(b)
        assert np.array_equal(bits(a.image_buffer), bits(b.image_buffer)), name
        assert a.counters().samples == b.counters().samples
        with pytest.raises(RtpbrError):
            b.last_sample_ms()
        with pytest.raises(RtpbrError):
            b.last_primary_ms()
        b.set_option("timing", 1); b.sample(n)
        tr, tot, launches = b.last_sample_ms()
        assert launches >= 1 and 0.0 < tr <= tot * 1.001, (name, tr, tot)
        tr, tot, launches = a.last_sample_ms()
        assert launches >= 1 and 0.0 < tr <= tot * 1.001, (name, tr, tot)
        a.close(); b.close()


def r_pixels(cfg, rank):
    """pixels of a 24x16 frame owned by `rank` of 2 with 16x16 tiles dealt round-robin (tile 0: 16x16, tile 1: 8x16)"""
    return 16 * 16 if rank == 0 else (cfg.width - 16) * 16


def test_neural_sdf_pass_policy_independence():
    """The neural SDF is evaluated wave-cooperatively: waiting rays are compacted into 32-slot half passes and which
    rays a pass takes depends on the policy options.  Every policy — and the VALU-only network — must give the
    oracle's bits, the same number of network evaluations, and never more slots than 32 per half pass."""
    case = case_by_name("bunny_glass")
    o = OracleRenderer(case.scene, case.cfg)
    case.run(o)
    want = bits(o.image_buffer)
    evals = o.counter("mlp_lane_evals")
    assert evals > 0
    for opts in ({}, {"mlp_lanes": 1, "mlp_full": 1}, {"mlp_lanes": 1, "mlp_full": 65}, {"mlp_lanes": 64, "mlp_full": 64},
                 {"mlp_lanes": 33, "mlp_full": 34}, {"mlp_lanes": 16, "mlp_full": 48, "shade_lanes": 5, "swap_lanes": 3},
                 {"mlp_lanes": 40, "mlp_full": 60, "waves_per_cu": 4}, {"mlp_mfma": 0}, {"jit": 2, "jit_bake": 1, "mlp_lanes": 7},
                 {"mlp_mfma": 0, "jit": 2, "jit_bake": 1}, {"mlp_mfma": 0, "mlp_lanes": 9, "mlp_full": 33}):
        r = Renderer(case.scene, case.cfg)
        for k, v in opts.items():
            r.set_option(k, v)
        case.run(r)
        assert np.array_equal(bits(r.image_buffer), want), opts
        if opts.get("mlp_mfma", 1):
            halves = r.counter("mlp_wave_evals")
            assert r.counter("mlp_lane_evals") == evals, opts
            assert evals <= 32 * halves, opts
        r.close()


@pytest.mark.parametrize("rots", ["axis_aligned", "mixed_axes", "tilted"])
def test_rotation_signatures_match_oracle(rots):
    """8-box scenes whose rotation signature fits / does not fit the ahead-of-time specialised
    instance (RT_BOX_SIGNATURES): identity matrices fit every single-axis class, a z-rotation or
    a tilted box in a slot specialised for another axis must fall back to the general instance.
    Either way the bits are the oracle's (the sparse matrix products are exact)."""
    case = case_by_name("cornell_v3_8b_wide")
    sc = cornell_box("v3", aspect=96 / 54)
    table = {"axis_aligned": [(0, 0, 0)] * 8,
             "mixed_axes": [(0, 0, 0), (90, 0, 0), (33, 0, 0), (0, 12, 0), (0, 0, 0), (0, -253, 0), (0, 0, 0), (-90, 0, 0)],
             "tilted": [(0, 0, 0), (90, 0, 0), (90, 0, 0), (0, 90, 0), (0, 90, 0), (10, -253, 5), (0, 0, 30), (90, 0, 0)]}[rots]
    for o, rot in zip(sc.objects, table):
        o.transform.rotation[:] = rot
    o = OracleRenderer(sc, case.cfg)
    o.sample(3)
    for opts in ({}, {"primary_split": 2}, {"specialize": 0}, {"primary_split": 2, "specialize": 0}, {"scheduler": 0},
                 {"lazy_sqrt": 0}):
        g = Renderer(sc, case.cfg)
        for k, v in opts.items():
            g.set_option(k, v)
        g.sample(3)
        assert np.array_equal(bits(g.image_buffer), bits(o.image_buffer)), (rots, opts)
        g.close()


def test_persistent_form_schedulers_agree():
    """src/ form: the lock-step kernel (scheduler 0) and the LDS-pool kernel (scheduler 1) give the
    same image_buffer AND the same ray_buffer state, for any launch split."""
    case = case_by_name("src_persistent")
    ref = None
    # grid_blocks forces waves that own MORE pixels than they hold (5184 pixels: 1 block = 1296 per wave, 9 blocks = 144,
    # 10 blocks = 130 — a two-item window, the hand-out waits for stragglers all the time), walked in residencies of 1..32
    # bounce-steps (state through ray_buffer between them); 48 steps with residency 32 ends on a short residency
    for opts, split in (({"scheduler": 0}, (48,)), ({"scheduler": 1}, (48,)), ({"scheduler": 1, "shade_lanes": 9, "swap_lanes": 3}, (5, 43)),
                        ({"scheduler": 1, "shade_lanes": 64, "swap_lanes": 1, "waves_per_cu": 4}, (24, 24)),
                        ({"scheduler": 1, "grid_blocks": 1, "residency": 16}, (48,)),
                        ({"scheduler": 1, "grid_blocks": 1, "residency": 1}, (7, 41)),
                        ({"scheduler": 1, "grid_blocks": 9, "residency": 32}, (48,)),
                        ({"scheduler": 1, "grid_blocks": 10, "residency": 4, "shade_lanes": 20}, (48,)),
                        ({"scheduler": 1, "grid_blocks": 3, "residency": 8, "jit": 0}, (30, 18)),
                        ({"scheduler": 1, "grid_blocks": 64}, (48,)),
                        # cost-ordered ownership (round 4): re-planned from the recorded march steps after the first launch;
                        # heavy waves of 1 .. 128 pixels, every pixel heavy (thresholds 0: capped at half of the waves), none
                        # heavy; tracked-object march steps always / never / in sparse phases only
                        ({"scheduler": 1, "plan_interval": 4}, (5, 43)),
                        ({"scheduler": 1, "plan_interval": 1, "heavy_mean_x16": 0, "heavy_bulk_x16": 0, "sparse_lanes": 64}, (1, 7, 20, 20)),
                        ({"scheduler": 1, "plan_interval": 8, "heavy_mean_x16": 16, "heavy_bulk_x16": 0, "heavy_own": 128, "grid_blocks": 6}, (8, 40)),
                        ({"scheduler": 1, "plan_interval": 8, "heavy_mean_x16": 24, "heavy_bulk_x16": 1, "heavy_own": 1, "sparse_lanes": 0}, (8, 8, 32)),
                        ({"scheduler": 1, "plan_interval": 2, "heavy_mean_x16": 8, "heavy_own": 33, "grid_blocks": 2, "residency": 4, "jit": 0}, (2, 30, 16)),
                        ({"scheduler": 1, "plan_interval": 16, "heavy_own": 0, "sparse_lanes": 64, "jit": 1, "jit_bake": 1}, (16, 32)),
                        ({"scheduler": 1, "plan_interval": 4, "heavy_mean_x16": 20, "heavy_bulk_x16": 0, "tiny_own": 2, "tiny_waves": 7, "leave_x8": 1}, (4, 44)),
                        ({"scheduler": 1, "plan_interval": 4, "heavy_mean_x16": 20, "heavy_bulk_x16": 0, "tiny_own": 8, "tiny_waves": 3, "leave_x8": 400, "src_track": 0}, (4, 44)),
                        # age-weighted shares of the light waves: self-tuned from the lifetimes of the previous launches (a grid of
                        # several blocks per CU is needed for there to be residency slots: 768 blocks = 3 per CU), fixed weights
                        ({"scheduler": 1, "plan_interval": 4, "grid_blocks": 768, "residency": 4}, (4, 4, 4, 12, 24)),
                        ({"scheduler": 1, "plan_interval": 8, "age_weights": 0xf731, "grid_blocks": 1024, "residency": 8}, (8, 40)),
                        ({"scheduler": 1, "plan_interval": 8, "age_tune": 0}, (8, 40)),
                        ({"scheduler": 1, "src_plan": 0, "sparse_lanes": 64}, (48,)),
                        # the wavefront split of a bounce-step (round 5: gen / march / shade kernels, rt_split.hpp) — what launches of
                        # <= src_split steps run: every step split, mixed with fused launches, on the cost-ordered list once a plan
                        # exists (tracked march for its heavy head), tiny grids, odd claim sizes, ahead-of-time and run-time instances
                        # the chain kernel beside the pool kernel (round 5, rt_chain.hpp): on by default whenever the plan finds the launch
                        # chain-bound (every set above that re-plans); off; with every pixel that has a cost on record heavy
                        ({"scheduler": 1, "src_chain": 0, "plan_interval": 4}, (4, 44)),
                        ({"scheduler": 1, "src_chain": 2, "plan_interval": 2, "heavy_mean_x16": 0, "heavy_bulk_x16": 0, "grid_blocks": 8}, (2, 6, 40)),
                        ({"scheduler": 1, "src_chain": 2, "plan_interval": 4, "chain_waves": 5, "grid_blocks": 3, "residency": 8}, (4, 20, 24)),
                        ({"scheduler": 1, "src_chain": 1, "plan_interval": 8, "jit": 0, "src_track": 1}, (8, 40)),
                        ({"scheduler": 1, "src_split": 0}, (1, 1, 46)),
                        ({"scheduler": 1, "src_split": 256}, (48,)),
                        ({"scheduler": 1, "src_split": 256, "plan_interval": 4, "split_wait": 3, "grid_blocks": 2}, (5, 43)),
                        ({"scheduler": 1, "src_split": 1, "plan_interval": 2}, (1, 1, 1, 1, 1, 1, 42)),
                        ({"scheduler": 1, "src_split": 256, "jit": 0, "chunk": 7, "split_wait": 64}, (24, 24)),
                        ({"scheduler": 1, "src_split": 256, "sparse_lanes": 64, "heavy_mean_x16": 0, "heavy_bulk_x16": 0, "plan_interval": 1}, (1, 7, 40)),
                        ({"scheduler": 1, "src_split": 256, "jit": 1, "jit_bake": 1, "src_track": 0, "waves_per_cu": 4}, (3, 45)),
                        # the object-parallel evaluation of sparse waves (round 6, nearest_op3: lane = (ray, object) while at most 8
                        # lanes march) is ON in every set above that runs the split march or the chain kernel; here: off, and on in
                        # tiny grids where nearly every iteration is sparse, ahead-of-time and run-time instances
                        ({"scheduler": 1, "src_split": 256, "src_op": 0, "split_head": 0, "plan_interval": 4}, (6, 42)),
                        ({"scheduler": 1, "src_split": 256, "src_op": 1, "grid_blocks": 64, "split_wait": 1, "jit": 0, "split_head": 1}, (24, 24)),
                        ({"scheduler": 1, "src_split": 256, "src_op": 1, "sparse_lanes": 8, "jit": 1, "jit_bake": 1, "plan_interval": 4}, (5, 43)),
                        ({"scheduler": 1, "src_chain": 2, "src_op": 0, "plan_interval": 2, "heavy_mean_x16": 0, "heavy_bulk_x16": 0, "grid_blocks": 8}, (2, 6, 40)),
                        ({"scheduler": 1, "src_chain": 2, "src_op": 1, "plan_interval": 2, "heavy_mean_x16": 0, "heavy_bulk_x16": 0, "grid_blocks": 8, "jit": 1, "jit_bake": 1}, (2, 6, 40))):
        r = Renderer(case.scene, case.cfg)
        case.setup(r)
        for k, v in opts.items():
            r.set_option(k, v)
        ctr = [0, 0, 0, 0]
        for n in split:
            r.sample(n)
            c = r.counters()
            ctr = [ctr[0] + c.samples, ctr[1] + c.raycasts, ctr[2] + c.march_steps, ctr[3] + c.deposits]
        got = (bits(r.image_buffer), bits(r.ray_buffer), ctr)
        if ref is None:
            ref = got
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and got[2] == ref[2], opts
        r.close()


def test_adaptive_sampling_through_every_src_kernel():
    """ADAPTIVE_SAMPLING = True the way the reference drives it (src/renderer.py:25-32, src/pathtracer.py:94-103,
    src/postprocessor.py:40-43): render() = ONE pathtrace() of ONE bounce-step + post_process(), 48 times; the mask
    (diff_pixels > NOISE_THRESHOLD) starts to bite around launch 20 and has emptied the frame by launch 44.  Through every
    kernel that carries the mask: the wavefront split (src_gen), the fused pool kernel, the chain kernel with every pixel in
    the chain set, the lock-step kernel; ahead-of-time and run-time compiled instances; with and without the object-parallel
    evaluation of sparse waves.  image_buffer, ray_buffer, diff_buffer, diff_pixels and image_pixels bit for bit the oracle's,
    half way and at the end."""
    from raytracingpbr_amd import src_scene
    from cases import _env
    cfg = Config.src(64, 36, 11, steps_per_launch=1).copy(adaptive_sampling=1, noise_threshold=0.05)
    sc = src_scene(aspect=64 / 36)

    def state(r):
        return tuple(bits(x).copy() for x in (r.image_buffer, r.ray_buffer, r.diff_buffer, r.diff_pixels, r.image_pixels))

    o = OracleRenderer(sc, cfg)
    o.set_env(_env(), 1.4, 2.2)
    o.refresh()
    want, masked = {}, []
    for i in range(48):
        o.sample(1)
        o.post_process()
        masked.append(int((o.diff_pixels > cfg.noise_threshold).sum()))
        if i in (29, 47):
            want[i] = state(o)
    assert masked[10] == 64 * 36 and 0 < masked[29] < 64 * 36 and masked[47] == 0      # the mask acts inside the run
    for opts in ({}, {"src_split": 256}, {"src_split": 0}, {"src_split": 0, "src_chain": 0}, {"scheduler": 0},
                 {"src_op": 0}, {"jit": 0}, {"jit": 0, "src_op": 0, "split_wait": 3}, {"jit": 1, "jit_bake": 1},
                 {"jit": 1, "jit_bake": 1, "src_split": 0, "plan_interval": 2},
                 # every pixel with a cost on record in the chain set: the chain kernel's own mask
                 {"src_split": 0, "src_chain": 2, "plan_interval": 2, "heavy_mean_x16": 0, "heavy_bulk_x16": 0, "grid_blocks": 8},
                 {"src_split": 0, "src_chain": 2, "plan_interval": 2, "heavy_mean_x16": 0, "heavy_bulk_x16": 0, "grid_blocks": 8, "jit": 1, "jit_bake": 1},
                 {"src_split": 1, "plan_interval": 1, "heavy_mean_x16": 0, "heavy_bulk_x16": 0, "sparse_lanes": 64, "jit": 1}):
        g = Renderer(sc, cfg)
        g.set_env(_env(), 1.4, 2.2)
        for k, v in opts.items():
            g.set_option(k, v)
        g.refresh()
        for i in range(48):
            g.render()                                      # sample(1) + post_process(), the reference's render()
            if i in want:
                got = state(g)
                for name, a, b in zip(("image_buffer", "ray_buffer", "diff_buffer", "diff_pixels", "image_pixels"), got, want[i]):
                    assert np.array_equal(a, b), (opts, i, name)
        g.close()


def test_persistent_form_tile_partition():
    """src/ pipeline under the multi-GPU tile partition: every virtual rank advances ONLY its own pixels (image_buffer and
    ray_buffer elsewhere stay untouched), edge tiles are padded, and the union of the ranks' pixels is the untiled run bit
    for bit — through the pool kernel's single-pass and multi-pass (residency) walks, and against the oracle's own tiled run."""
    case = case_by_name("src_persistent")
    W, H = case.cfg.width, case.cfg.height
    full = Renderer(case.scene, case.cfg)
    case.setup(full)
    full.sample(20)
    want_ib, want_rb = full.image_buffer, full.ray_buffer
    for world, tile, opts in ((3, (20, 16), {}), (2, (32, 32), {"grid_blocks": 1, "residency": 4}), (5, (8, 8), {"scheduler": 0}),
                              # the cost plan orders LOCAL pixels (padded edge tiles included): re-planned between the two calls
                              (3, (20, 16), {"plan_interval": 4, "heavy_mean_x16": 8, "heavy_bulk_x16": 0, "tiny_own": 2, "sparse_lanes": 64}),
                              (2, (16, 8), {"plan_interval": 12, "grid_blocks": 600, "residency": 2}),
                              (3, (20, 16), {"src_split": 256, "plan_interval": 4})):
        lay = TileLayout(W, H, tile[0], tile[1], world)
        owner = lay.owner_map()
        got_ib, got_rb = np.zeros_like(want_ib), np.zeros_like(want_rb)
        for rank in range(world):
            r = Renderer(case.scene, case.cfg)
            case.setup(r)
            for k, v in opts.items():
                r.set_option(k, v)
            r.set_tiles(tile[0], tile[1], rank, world)
            r.sample(12)
            r.sample(8)
            ib, rb = r.image_buffer, r.ray_buffer
            mine = owner == rank
            assert np.all(ib[~mine] == 0)                                   # nobody else's pixels were touched
            got_ib[mine], got_rb[mine] = ib[mine], rb[mine]
            if rank == 1:
                o = OracleRenderer(case.scene, case.cfg)
                case.setup(o)
                o.set_tiles(tile[0], tile[1], rank, world)
                o.sample(20)
                assert np.array_equal(bits(ib), bits(o.image_buffer)) and np.array_equal(bits(rb[mine]), bits(o.ray_buffer[mine]))
            r.close()
        assert np.array_equal(bits(got_ib), bits(want_ib)) and np.array_equal(bits(got_rb), bits(want_rb)), (world, tile, opts)


def test_tile_partition_pack_unpack_is_bit_exact():
    """G virtual ranks on one device: each renders its tiles, packs them on the device, rank 0
    unpacks -> identical to the untiled frame (SURVEY.md §8(e) testability row)."""
    import torch
    case = case_by_name("cornell_v3_8b_wide")
    W, H = case.cfg.width, case.cfg.height
    full = Renderer(case.scene, case.cfg)
    full.sample(6)
    want = full.image_buffer
    for world, tile in ((3, (16, 16)), (8, (8, 8)), (2, (32, 20))):
        lay = TileLayout(W, H, tile[0], tile[1], world)
        root = Renderer(case.scene, case.cfg)
        root.set_tiles(tile[0], tile[1], 0, world)
        root.sample(6)
        assert root.packed_bytes() == lay.packed_pixels * 16
        for rank in range(1, world):
            r = Renderer(case.scene, case.cfg)
            r.set_tiles(tile[0], tile[1], rank, world)
            r.sample(6)
            buf = torch.empty(lay.packed_pixels * 4, dtype=torch.float32, device="cuda")
            r.pack_tiles(buf.data_ptr())
            r.sync()
            assert np.array_equal(buf.cpu().numpy().reshape(-1, 4), lay.pack(r.image_buffer, rank))
            root.unpack_tiles(buf.data_ptr(), rank)
            root.sync()
            r.close()
        assert np.array_equal(bits(root.image_buffer), bits(want)), (world, tile)
        root.close()


def test_checkpoint_resume_through_write_buffer():
    """image_buffer is a sufficient statistic (SURVEY.md §5 checkpoint row): save it, load it
    into a fresh context, continue with the next sample indices -> identical to one run."""
    case = case_by_name("cornell_v2")
    a = Renderer(case.scene, case.cfg); a.sample(10)
    b = Renderer(case.scene, case.cfg); b.sample(4)
    saved = b.image_buffer
    c = Renderer(case.scene, case.cfg)
    c.image_buffer = saved
    c.set_option("sample_base", 4)
    c.sample(6)
    assert np.array_equal(bits(c.image_buffer), bits(a.image_buffer))


def test_read_into_page_locked_host_buffer():
    """rtpbr_host_alloc / read_into: the page-locked destination holds the same bits as a fresh read; foreign pointers are refused."""
    from raytracingpbr_amd.renderer import BUF_IMAGE_BUFFER, BUF_IMAGE_PIXELS
    case = case_by_name("src_persistent")
    r = Renderer(case.scene, case.cfg)
    case.setup(r)
    pinned = r.host_array(BUF_IMAGE_PIXELS)
    acc = r.host_array(BUF_IMAGE_BUFFER)
    for _ in range(3):
        r.sample(4)
        r.post_process()
        r.read_into(BUF_IMAGE_PIXELS, pinned)
        r.read_into(BUF_IMAGE_BUFFER, acc)
        assert np.array_equal(bits(pinned), bits(r.image_pixels)) and np.array_equal(bits(acc), bits(r.image_buffer))
    with pytest.raises(ValueError):
        r.read_into(BUF_IMAGE_PIXELS, np.zeros((3, 3), np.float32))
    junk = (C.c_char * 64)()
    with pytest.raises(RtpbrError):
        r.api.call("host_free", r._ctx, C.cast(junk, C.c_void_p))
    r.api.call("host_free", r._ctx, C.c_void_p(pinned.ctypes.data))
    r.close()                      # (frees `acc` with the context)


def test_frames_handed_over_without_a_stall_equal_the_synchronous_path():
    """rtpbr_read_buffer_async / rtpbr_read_wait / rtpbr_buffer_device_ptr (round 6): the reference hands image_pixels to its
    window on the device and goes straight on to the next render() (src/main.py:62-64).  Frame k's read-back is enqueued, frame
    k+1 is rendered while it is in flight, and every DELIVERED frame holds the bits the blocking path gives; a read of
    image_buffer followed at once by more samples returns the state at the time of the call (the writer waits on the device);
    more tickets than slots; pageable destinations and unknown tickets are refused; the device pointer is the buffer."""
    import torch
    from raytracingpbr_amd.renderer import BUF_IMAGE_BUFFER, BUF_IMAGE_PIXELS
    case = case_by_name("src_persistent")
    a, b = Renderer(case.scene, case.cfg), Renderer(case.scene, case.cfg)
    case.setup(a)
    case.setup(b)
    want = []
    for k in range(20):
        a.render()
        want.append(bits(a.image_pixels).copy())
    pinned = [b.host_array(BUF_IMAGE_PIXELS) for _ in range(2)]
    prev = None
    for k in range(20):
        b.render()
        t = b.read_async(BUF_IMAGE_PIXELS, pinned[k % 2])
        if prev is not None:
            b.read_wait(prev)
            assert np.array_equal(bits(pinned[(k - 1) % 2]), want[k - 1]), k - 1
        prev = t
    b.read_wait(prev)
    assert np.array_equal(bits(pinned[1]), want[19])
    b.read_wait(0)                                       # a ticket whose slot has long been handed on: done by definition
    # image_buffer: the copy sees the state at the call, although sample() is enqueued right behind it
    acc = b.host_array(BUF_IMAGE_BUFFER)
    snap = bits(b.image_buffer).copy()
    t = b.read_async(BUF_IMAGE_BUFFER, acc)
    b.sample(6)
    b.refresh()
    b.read_wait(t)
    assert np.array_equal(bits(acc), snap)
    # more outstanding tickets than the ring holds
    ts = [b.read_async(BUF_IMAGE_PIXELS, pinned[0]) for _ in range(19)]
    for t in ts:
        b.read_wait(t)
    with pytest.raises(RtpbrError):
        b.read_async(BUF_IMAGE_PIXELS, np.empty_like(pinned[0]))          # pageable memory
    with pytest.raises(RtpbrError):
        b.read_wait(10 ** 6)
    with pytest.raises(ValueError):
        b.read_async(BUF_IMAGE_PIXELS, acc)                               # wrong shape
    # zero copy: a torch tensor ON the renderer's image_pixels
    b.render()
    b.sync()
    tens = torch.as_tensor(b.device_array(BUF_IMAGE_PIXELS), device="cuda")
    addr, nbytes = b.device_ptr(BUF_IMAGE_PIXELS)
    assert tens.data_ptr() == addr and nbytes == tens.numel() * 4 and tuple(tens.shape) == (case.cfg.width, case.cfg.height, 3)
    assert np.array_equal(bits(tens.cpu().numpy()), bits(b.image_pixels))
    b.host_release(acc)
    with pytest.raises(ValueError):
        b.host_release(np.zeros(4, np.float32))
    a.close()
    b.close()


@pytest.mark.parametrize("name", ["tokyo_ibl_env", "src_persistent", "bunny_glass"])
def test_packed_environment_gives_the_same_bits(name):
    """option env_packed (round 6): the environment as SURVEY.md T9 names it for the reference's 8-bit image — RGBA8 texels + the
    256-entry table Image.process() amounts to (src/ibl.py:14-23) — instead of float4 texels: the same floats reach the shading,
    so image_buffer, ray_buffer and the counters are the oracle's bit for bit, in ahead-of-time and run-time instances."""
    case = case_by_name(name)
    o = OracleRenderer(case.scene, case.cfg)
    case.run(o)
    for opts in ({"env_packed": 1}, {"env_packed": 1, "jit": 1, "jit_bake": 1}, {"env_packed": 1, "scheduler": 0, "jit": 0}):
        g = Renderer(case.scene, case.cfg)
        for k, v in opts.items():
            g.set_option(k, v)
        case.run(g)
        assert np.array_equal(bits(g.image_buffer), bits(o.image_buffer)), opts
        assert np.array_equal(bits(g.image_pixels), bits(o.image_pixels)), opts
        if case.cfg.kernel_form == 1:
            assert np.array_equal(bits(g.ray_buffer), bits(o.ray_buffer)), opts
        cg, co = g.counters(), o.counters()
        assert (cg.samples, cg.raycasts, cg.march_steps, cg.hits, cg.sky_lookups) == (co.samples, co.raycasts, co.march_steps, co.hits, co.sky_lookups), opts
        g.close()


def test_refresh_semantics():
    case = case_by_name("src_persistent")
    r = Renderer(case.scene, case.cfg)
    case.setup(r)
    r.sample(10)
    rb = r.ray_buffer
    r.refresh()
    assert np.all(r.image_buffer == 0) and np.all(r.ray_depth() == 0)
    assert np.array_equal(r.ray_buffer[..., :9], rb[..., :9])


def test_staging_allocation_failure_falls_back_to_fewer_samples_per_launch():
    """When the device cannot hold the staging of a whole call (one 12-byte record per pixel-sample), the call must split itself
    into smaller launches instead of failing — same bits."""
    import torch
    W, H, SPP = 1920, 1080, 64                                  # 64 spp: 1.6 GB of staging + 1.1 GB of primary records
    sc, cfg = cornell_box("v3", aspect=W / H), Config.cornell_v3(W, H, 0, 8)
    ref = Renderer(sc, cfg)
    ref.sample(SPP)
    want = bits(ref.image_buffer)
    ref.close()
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < (16 << 30):
        pytest.skip("the device is shared: cannot stage an out-of-memory condition safely")
    try:
        hog = torch.empty(free - (2000 << 20), dtype=torch.uint8, device="cuda")     # leave 2 GB
    except RuntimeError as e:                                                        # pragma: no cover
        pytest.skip("could not fill the device: %s" % e)
    try:
        r = Renderer(sc, cfg)
        r.sample(SPP)
        assert np.array_equal(bits(r.image_buffer), want)
        tr, tot, launches = r.last_sample_ms()
        assert launches >= 2                                     # it did split
        r.close()
    finally:
        del hog
        torch.cuda.empty_cache()


def test_error_channel():
    api = hip_api()
    ctx = C.c_void_p()
    api.call("create", 0, C.byref(ctx))
    with pytest.raises(RtpbrError) as e:
        api.call("sample", ctx, 1)                       # nothing configured yet
    assert e.value.code == -4
    bad = Config.cornell_v3(16, 16).copy(width=0)
    with pytest.raises(RtpbrError):
        api.call("set_config", ctx, C.byref(bad))
    with pytest.raises(RtpbrError):
        api.call("create", 9999, C.byref(C.c_void_p()))  # no such device
    api.call("destroy", ctx)
    r = Renderer(cornell_box("v3"), Config.tokyo_ibl(32, 18))
    with pytest.raises(RtpbrError):
        r.sample(1)                                      # env-map sky without an env map
    with pytest.raises(RtpbrError):
        r.set_option("no_such_option", 1)
    for key, value in (("chunk", 8193), ("residency", 12), ("residency", 512), ("sparse_lanes", 65), ("grid_blocks", -1), ("heavy_own", 129), ("plan_interval", 0), ("tiny_own", 129),
                       ("leave_x8", 0), ("src_plan", 2)):
        with pytest.raises(RtpbrError):                  # out of range (chunk: the 32-bit work counter's overshoot margin)
            r.set_option(key, value)
    with pytest.raises(ValueError):
        r.image_buffer = np.zeros((3, 3, 4), np.float32)
    # a rejected scene leaves the context as it was
    good = cornell_box("v3")
    g = Renderer(good, Config.cornell_v3(32, 32, 1, 3))
    g.sample(2)
    want = bits(g.image_buffer).copy()
    bad_scene = cornell_box("v3")
    bad_scene.objects[5].type = 77
    with pytest.raises(RtpbrError):
        g.set_scene(bad_scene)
    g.refresh()
    g.set_option("sample_base", 0)                       # same sample indices -> same random streams
    g.sample(2)
    assert np.array_equal(bits(g.image_buffer), want)
    g.set_option("reserve_spp", 64)                      # allocation only: results unchanged
    g.refresh()
    g.set_option("sample_base", 0)
    g.sample(2)
    assert np.array_equal(bits(g.image_buffer), want)


_ORACLE_C2 = {}


def _oracle_c2(sc, cfg):
    """the oracle's share of the 1080p checks, computed once for both kernel variants"""
    if not _ORACLE_C2:
        o = OracleRenderer(sc, cfg); o.sample(1)
        os_ = OracleRenderer(sc, cfg); os_.set_tiles(16, 16, 5, 128); os_.sample(256)
        _ORACLE_C2.update(one=o.image_buffer, one_ctr=o.counters(), sub=os_.image_buffer, sub_ctr=os_.counters())
    return _ORACLE_C2


def _ctr(c):
    return (c.samples, c.raycasts, c.march_steps, c.hits, c.sky_lookups, c.deposits)


@pytest.mark.parametrize("variant", ["aot", "jit_baked"])
def test_full_size_cornell_1080p(variant, tmp_path, monkeypatch):
    """BASELINE.json configs[1] geometry: Cornell 1920x1080, 8 bounces, through the ahead-of-time kernels AND through the
    kernels bench.py times (run-time compiled for the scene, object table and configuration baked: jit + jit_bake).  The
    oracle cannot do 256 spp on the full frame in seconds, so: (a) the whole frame at 1 spp is bit-exact, work counters
    included; (b) a sparse 1/128 tile subset at 256 spp is bit-exact, counters included; (c) size-independent properties:
    count == spp everywhere, tile-partition invariance, spp additivity."""
    monkeypatch.setenv("RTPBR_JIT_CACHE", str(tmp_path))
    W, H = 1920, 1080
    sc = cornell_box("v3", aspect=W / H)
    cfg = Config.cornell_v3(W, H, seed=0, max_raytrace=8)

    def make():
        r = Renderer(sc, cfg)
        if variant == "jit_baked":
            r.set_option("jit", 2)                       # strict: an error if the run-time instance cannot be used
            r.set_option("jit_bake", 2)
        else:
            r.set_option("jit", 0)
        return r
    want = _oracle_c2(sc, cfg)
    g = make()
    g.sample(1)
    assert g.counter("jit_active") == (1 if variant == "jit_baked" else 0)
    one = g.image_buffer
    assert np.array_equal(bits(one), bits(want["one"])) and _ctr(g.counters()) == _ctr(want["one_ctr"])
    # (b) sparse subset, 256 spp
    gs = make(); gs.set_tiles(16, 16, 5, 128); gs.sample(256)
    sub = gs.image_buffer
    assert np.array_equal(bits(sub), bits(want["sub"])) and _ctr(gs.counters()) == _ctr(want["sub_ctr"])
    own = TileLayout(W, H, 16, 16, 128).owner_map() == 5
    assert np.all(sub[own][:, 3] == 256.0) and np.all(sub[~own] == 0)
    # (c) full frame 256 spp: counts, additivity (1 + 255 == 256 straight), subset consistency
    g.sample(255)
    full = g.image_buffer
    assert np.all(full[..., 3] == 256.0)
    assert np.array_equal(bits(full[own]), bits(sub[own]))
    assert np.all(np.isfinite(full))
    # display-space parity bar of the north star on what the oracle covered
    g.post_process()
    assert np.all(np.isfinite(g.image_pixels)) and g.image_pixels.min() >= 0 and g.image_pixels.max() <= 1


def _run_bench(args, nproc=0, timeout=900, env=None):
    import json
    import os
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable]
    if nproc:
        s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
        cmd += ["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc), "--master-addr", "127.0.0.1", "--master-port", str(port)]
    out = subprocess.run(cmd + [os.path.join(root, "bench.py")] + args, capture_output=True, text=True, timeout=timeout, cwd=root,
                         env=dict(os.environ, **(env or {})))
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads([l for l in out.stdout.split("\n") if l.startswith("{")][-1])


@pytest.mark.parametrize("workload", ["c2", "c5", "src"])
def test_bench_multirank_path_functional(workload):
    """bench.py's N>1 path (tile partition + one gather + max-over-ranks timing) under torch.distributed.run, exercised with
    2 ranks sharing this box's single GPU and the gather staged through host memory: the RCCL collective itself needs 2
    GPUs, but everything around it (launch, control plane, tiles, per-rank report, JSON contract) runs."""
    j = _run_bench(["--gpus", "2", "--steps", "1", "--warmup", "1", "--workload", workload, "--width", "480", "--height", "270", "--spp", "16",
                    "--transport", "host", "--same-device", "--no-cpu-baseline"], nproc=2)
    assert j["n_gpus"] == 2 and j["scaling"] == "strong" and j["value"] > 0
    assert j["unit"] == ("Mbounce-steps/s" if workload == "src" else "Msamples/s")
    for k in ("metric", "steps", "warmup", "ms_per_step", "higher_is_better", "vs_baseline", "dtype", "data", "config", "roofline", "multi_gpu"):
        assert k in j
    mg = j["multi_gpu"]
    assert [p["rank"] for p in mg["per_rank"]] == [0, 1] and all(p["kernel_ms_per_step"] > 0 for p in mg["per_rank"])
    assert mg["bytes_gathered_per_rank"] > 0 and "host" in mg["transport"]


@pytest.mark.parametrize("workload", ["c1", "c3", "c4", "c5", "src"])
def test_bench_every_workload_single_gpu_contract(workload):
    """bench.py --workload X at N = 1 (small frame): the line keeps the driver's contract and carries its own FLOP model"""
    j = _run_bench(["--gpus", "1", "--steps", "2", "--warmup", "1", "--workload", workload, "--width", "320", "--height", "180", "--spp", "8",
                    "--full", "--no-cpu-baseline", "--no-configs"])
    assert j["n_gpus"] == 1 and j["steps"] == 2 and j["warmup"] == 1 and j["value"] > 0 and j["higher_is_better"] is True
    assert j["unit"] == ("Mbounce-steps/s" if workload == "src" else "Msamples/s") and j["dtype"] == "f32" and j["data"] == "synthetic"
    r = j["roofline"]
    assert r["bound"] == "valu" and r["peak"] == 157.3 and 0 < r["frac"] < 1 and r["algorithmic_flop_per_unit"] > 1000
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3 and r["launches_timed"] >= 2
    assert abs(j["value"] - 320 * 180 * 8 * 2 / (j["ms_per_step"] * 2 / 1e3) / 1e6) < 0.02 * j["value"]
    assert j["config"]["kernels"].startswith("run-time compiled") and j["jit"]["first_use_s"] > 0


def _rccl_stub():
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    stub = os.path.join(root, "tests", "stubs", "libfake_rccl.so")
    src = os.path.join(root, "tests", "stubs", "fake_rccl.cpp")
    if not os.path.exists(stub) or os.path.getmtime(stub) < os.path.getmtime(src):
        subprocess.run(["g++", "-O1", "-fPIC", "-shared", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", src, "-L/opt/rocm/lib", "-lamdhip64", "-lrt",
                        "-o", stub], check=True)
    return stub


@pytest.mark.parametrize("workload,nproc", [("c2", 2), ("src", 3)])
def test_bench_scale_command_with_one_process_per_rank(workload, nproc):
    """The command a SCALE run issues — torch.distributed.run, N processes, bench.py --gpus N with its DEFAULT transport:
    rtpbr_rccl_unique_id on rank 0, the id over the gloo control plane, ncclCommInitRank with N > 1 in every process,
    rtpbr_gather_tiles per step — on this box's one GPU.  RCCL refuses several ranks on one device, so RTPBR_RCCL_LIB points
    the library at tests/stubs/libfake_rccl.so, which moves the packed tiles ACROSS the processes (hipIpcMemHandle) and
    nothing else.  The communicator must report N ranks, every rank must have rendered and gathered, and the frame rank 0
    holds after the gather must equal the untiled frame bit for bit."""
    j = _run_bench(["--gpus", str(nproc), "--steps", "2", "--warmup", "1", "--workload", workload, "--width", "480", "--height", "270", "--spp", "16",
                    "--transport", "rccl", "--same-device", "--check-gather", "--no-cpu-baseline"], nproc=nproc,
                   env={"RTPBR_RCCL_LIB": _rccl_stub(), "HSA_ENABLE_IPC_MODE_LEGACY": "0"})
    mg = j["multi_gpu"]
    assert j["n_gpus"] == nproc and mg["rccl_nranks"] == nproc and mg["rccl_rank"] == 0 and mg["rccl_version"] == 99999
    assert "ncclGather" in mg["transport"] and mg["gathered_equals_untiled"] is True
    assert [p["rank"] for p in mg["per_rank"]] == list(range(nproc))
    assert all(p["kernel_ms_per_step"] > 0 and p["gather_ms_per_step"] > 0 for p in mg["per_rank"])


def test_real_rccl_two_ranks_when_two_devices():
    """First contact with a multi-GPU node checks itself: when this box has >= 2 devices, the SCALE command with N = 2 runs on
    REAL RCCL (no stub) — ncclCommInitRank with two ranks, ncclGather over the fabric, the abort path armed — and the line must
    say so: two ranks, and the gathered frame equal to the untiled one bit for bit (bench.py --full checks that for N > 1).
    Skipped on a one-GPU box (there the stub-backed test above covers everything but RCCL itself)."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    j = _run_bench(["--gpus", "2", "--steps", "2", "--warmup", "1", "--width", "480", "--height", "270", "--spp", "16", "--full", "--no-cpu-baseline"], nproc=2)
    mg = j["multi_gpu"]
    assert j["n_gpus"] == 2 and mg["rccl_nranks"] == 2 and mg["rccl_version"] > 20000
    assert mg["gathered_equals_untiled"] is True


def test_bench_default_transport_is_the_c_abi_rccl_gather():
    """The transport a SCALE run takes by default — rtpbr_rccl_unique_id / rccl_init / gather_tiles, i.e. ROCm's librccl
    behind the C ABI — driven by bench.py itself on this box's one GPU (a 1-rank communicator): RCCL reports the rank
    count, the set-up time is in the line and it is seconds, not minutes."""
    j = _run_bench(["--gpus", "1", "--steps", "2", "--warmup", "1", "--width", "480", "--height", "270", "--spp", "16",
                    "--collective-at-1", "--full", "--no-cpu-baseline", "--no-configs"])
    mg = j["multi_gpu"]
    assert mg["rccl_nranks"] == 1 and mg["rccl_rank"] == 0 and mg["rccl_version"] > 20000
    assert mg["comm_init_s"] < 60 and "ncclGather" in mg["transport"]
    assert j["jit"]["first_use_s"] > 0 and j["roofline"]["frac"] > 0


def test_bench_plain_line_and_dumped_outputs(tmp_path):
    """A plain bench.py run carries the headline only (no --full blocks), and --dump-outputs writes the image_buffer of its
    last timed step: the frame a renderer holds after the same sequence of calls (first use, warm-up, timed steps)."""
    from raytracingpbr_amd import workloads
    W, H, SPP, warmup, steps = 320, 180, 8, 1, 3
    j = _run_bench(["--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--width", str(W), "--height", str(H), "--spp", str(SPP),
                    "--dump-outputs", str(tmp_path)])
    assert j["steps"] == steps and j["ms_per_step"] > 0 and j["value"] > 0
    assert not {"jit", "tolerance", "configs", "frame", "cpu_baseline"} & set(j)
    got = np.load(tmp_path / "image_buffer.npy")
    assert got.dtype == np.float32 and got.shape == (W, H, 4) and np.all(got[..., 3] == SPP)
    wl = workloads.get("c2", W, H, SPP)
    r = Renderer(wl.scene, wl.cfg)
    wl.setup(r)
    r.sample(SPP)
    for _ in range(warmup + steps):
        r.refresh()
        r.sample(SPP)
    assert np.array_equal(bits(got), bits(r.image_buffer))
    r.close()


def test_gathered_frame_equals_single_gpu_frame():
    """TileGather on device tensors with world=1 degenerates to a copy; with virtual ranks the
    packed buffers reproduce the untiled frame (the collective only moves these buffers)."""
    import torch
    from raytracingpbr_amd.distributed import TileGather
    case = case_by_name("cornell_v3_8b_wide")
    r = Renderer(case.scene, case.cfg)
    tg = TileGather(r, 0, 1, tile=(16, 16), device=torch.device("cuda", 0))
    r.sample(4)
    tg.gather()
    ref = Renderer(case.scene, case.cfg); ref.sample(4)
    assert np.array_equal(bits(r.image_buffer), bits(ref.image_buffer))


@pytest.mark.parametrize("seed", range(24))
def test_fuzz_random_scenes_match_oracle(seed):
    """Random object tables (all six analytic shapes, rotations, metal/glass/diffuse/light
    materials), cameras and variant knobs: image_buffer, image_pixels, ray_buffer and the work
    counters must equal the oracle's bit for bit."""
    from fuzz import random_case, run
    sc, cfg, env, n = random_case(seed)
    g = Renderer(sc, cfg)
    g.set_option("jit", 0)                    # the ahead-of-time instances (run-time compiled ones: test_gpu_jit.py)
    if seed % 2:
        g.set_option("primary_split", 2)      # small frames: force the separate primary-raycast kernel on half of the cases
    g = run(g, env, n, cfg.kernel_form == 1)
    o = run(OracleRenderer(sc, cfg), env, n, cfg.kernel_form == 1)
    cg, co = g.counters(), o.counters()
    assert (cg.samples, cg.raycasts, cg.march_steps, cg.hits, cg.sky_lookups, cg.deposits) == \
           (co.samples, co.raycasts, co.march_steps, co.hits, co.sky_lookups, co.deposits)
    assert np.array_equal(bits(g.image_buffer), bits(o.image_buffer))
    assert np.array_equal(bits(g.image_pixels), bits(o.image_pixels))
    if cfg.kernel_form == 1:
        assert np.array_equal(bits(g.ray_buffer), bits(o.ray_buffer))
    g.close()
    if cfg.kernel_form == 1:
        # the src/ pool kernel's cost-ordered ownership and tracked-object march (round 4) on every kind of scene the fuzzer makes
        # (cones, planes, rotated shapes, both nearest_init conventions): re-planned after every launch, every pixel with a
        # recorded cost heavy, waves of 2 / 3 / 80 pixels, tracked steps whenever the scene allows them — in the ahead-of-time
        # and in the run-time compiled instance
        for opts in ({"plan_interval": 1, "heavy_mean_x16": 0, "heavy_bulk_x16": 0, "sparse_lanes": 64, "tiny_own": 2, "jit": 0},
                     {"plan_interval": 1, "heavy_mean_x16": 8, "heavy_bulk_x16": 0, "heavy_own": 3, "tiny_waves": 0, "sparse_lanes": 64, "jit": 1, "jit_bake": seed % 2},
                     {"src_plan": 0, "sparse_lanes": 64, "grid_blocks": 1, "residency": 2, "jit": 1},
                     # the wavefront split of every bounce-step (round 5, rt_split.hpp) with its two-bound tracked march — one- and
                     # two-object lean loops on whatever shapes the fuzzer made, every pixel with a recorded cost on the heavy head —
                     # and with the one-bound march of round 4
                     {"src_split": 256, "plan_interval": 1, "heavy_mean_x16": 0, "heavy_bulk_x16": 0, "sparse_lanes": 64, "jit": seed % 2, "jit_bake": 1},
                     {"src_split": 256, "src_track": 1, "split_wait": 5, "jit": 1 - seed % 2},
                     # the object-parallel evaluation (round 6) off, and with every iteration eligible (tiny waves: one block)
                     {"src_split": 256, "src_op": 0, "jit": seed % 2},
                     {"src_split": 256, "src_op": 1, "grid_blocks": 1, "split_wait": 1, "sparse_lanes": 64, "jit": 1 - seed % 2, "jit_bake": 1}):
            g = Renderer(sc, cfg)
            for k, v in opts.items():
                g.set_option(k, v)
            g = run(g, env, n, True)
            cg = g.counters()
            assert (cg.samples, cg.raycasts, cg.march_steps, cg.hits, cg.sky_lookups, cg.deposits) == \
                   (co.samples, co.raycasts, co.march_steps, co.hits, co.sky_lookups, co.deposits), opts
            assert np.array_equal(bits(g.image_buffer), bits(o.image_buffer)) and np.array_equal(bits(g.ray_buffer), bits(o.ray_buffer)), opts
            g.close()


@pytest.mark.parametrize("seed", range(16))
def test_fuzz_eight_box_scenes_match_oracle(seed):
    """8-box scenes drive the unrolled kernels: signature instances with the packed object table,
    the squared-distance nearest-box search (exact ties between overlapping slabs, rays inside a
    box or inside its rounding shell, both start conventions) and the culled primary kernel."""
    from fuzz import random_box8_case, run
    sc, cfg, env, n = random_box8_case(seed)
    o = run(OracleRenderer(sc, cfg), env, n, cfg.kernel_form == 1)
    co = o.counters()
    for opts in ({}, {"primary_split": 2}, {"lazy_sqrt": 0, "specialize": 0}):
        g = Renderer(sc, cfg)
        g.set_option("jit", 0)
        for k, v in opts.items():
            g.set_option(k, v)
        g = run(g, env, n, cfg.kernel_form == 1)
        cg = g.counters()
        assert (cg.samples, cg.raycasts, cg.march_steps, cg.hits, cg.sky_lookups, cg.deposits) == \
               (co.samples, co.raycasts, co.march_steps, co.hits, co.sky_lookups, co.deposits), opts
        assert np.array_equal(bits(g.image_buffer), bits(o.image_buffer)), opts
        if cfg.kernel_form == 1:
            assert np.array_equal(bits(g.ray_buffer), bits(o.ray_buffer)), opts
        g.close()


def test_edge_cases_match_oracle():
    """Degenerate sizes: 1x1 frame, 32 objects (RTPBR_MAX_OBJECTS), sample(0), a tile larger than
    the frame, more ranks than tiles (a rank that owns nothing), odd frame sizes vs tile edges."""
    from raytracingpbr_amd import SHAPE, Camera, Material, SDFObject, Scene, Transform
    rng = np.random.default_rng(5)
    objs = [SDFObject(SHAPE.BOX if i % 2 else SHAPE.SPHERE, Transform(rng.uniform(-3, 3, 3), rng.uniform(-90, 90, 3), rng.uniform(0.2, 0.8, 3)),
                      Material(rng.uniform(0.2, 1, 3), (1, 1, 1) if i else (30, 30, 30), 1, 0, 0, 1.5)) for i in range(32)]
    sc = Scene(objs, False, Camera((0, 0, 9), (0, 0, 0), (0, 1, 0), 40, 37 / 23, 0.02, 6))
    cfg = Config.scene_demo(37, 23, 3, 6)
    g, o = Renderer(sc, cfg), OracleRenderer(sc, cfg)
    for r in (g, o):
        r.sample(0)
        assert r.counters().samples == 0 and np.all(r.image_buffer == 0)
        r.sample(3)
    assert np.array_equal(bits(g.image_buffer), bits(o.image_buffer))
    # 1x1 frame
    c1 = Config.cornell_v3(1, 1, 0, 4)
    g1, o1 = Renderer(cornell_box("v3"), c1), OracleRenderer(cornell_box("v3"), c1)
    g1.sample(33); o1.sample(33)
    assert np.array_equal(bits(g1.image_buffer), bits(o1.image_buffer)) and g1.image_buffer[0, 0, 3] == 33
    # tile larger than the frame, and 5 ranks over 2 tiles: ranks 2..4 own nothing
    full = Renderer(sc, cfg); full.sample(2)
    merged = np.zeros_like(full.image_buffer)
    lay = TileLayout(37, 23, 32, 32, 5)
    assert lay.n_tiles == 2
    for rank in range(5):
        r = Renderer(sc, cfg); r.set_tiles(32, 32, rank, 5); r.sample(2)
        ib = r.image_buffer
        if rank >= 2:
            assert np.all(ib == 0) and r.counters().samples == 0
        lay.unpack_into(merged, lay.pack(ib, rank), rank)
        r.close()
    assert np.array_equal(bits(merged), bits(full.image_buffer))
    with pytest.raises(RtpbrError):
        g.set_scene(Scene(objs + objs[:1], False, sc.camera))          # 33 objects > RTPBR_MAX_OBJECTS


@pytest.mark.parametrize("scene_kind", ["mirror_ties", "far_camera", "touching", "single_object", "planes_and_none"])
def test_tracked_march_adversarial_scenes(scene_kind):
    """The exact tracked-object march of the src/ pool kernel (one object evaluated per step while a Lipschitz bound proves
    the others farther) on scenes built to break a sloppy bound: EXACT ties (two identical objects mirrored about the
    camera's plane of symmetry: the bound test is strict, a tie must fall back to the full evaluation and the lower index
    must win), a camera a thousand units away (the rounding allowance scales with |p|, rays restart from MAX_DIS after an
    escape), objects that touch (gap 0.001), one object only (nothing to bound: the second distance is 'infinite'), planes
    and NONE shapes mixed in.  Tracked steps whenever allowed (sparse_lanes 64), every pixel heavy, waves of 2; ahead-of-time
    and run-time instances; image_buffer, ray_buffer and the counters bit for bit against the oracle."""
    from raytracingpbr_amd import SHAPE, Camera, Material, SDFObject, Scene, Transform
    W, H = 48, 27
    diffuse = Material((0.7, 0.6, 0.5), (1, 1, 1), 1.0, 0.0, 0.0, 1.5)
    metal = Material((0.9, 0.9, 0.9), (1, 1, 1), 0.1, 1.0, 0.0, 1.2)
    light = Material((1, 1, 1), (8, 8, 8), 1.0, 0.0, 0.0, 1.0)
    ground = SDFObject(SHAPE.SPHERE, Transform((0, -100.5, 0), (0, 0, 0), (100, 100, 100)), diffuse)
    cam = Camera((0, 0.1, 5), (0, 0, 0), (0, 1, 0), 35, W / H, 0.01, 5)
    if scene_kind == "mirror_ties":
        objs = [ground] + [SDFObject(t, Transform((sx * 0.8, 0.0, 0.0), (0, 0, 0), (0.4, 0.4, 0.4)), m)
                           for t, m in ((SHAPE.SPHERE, metal), (SHAPE.BOX, diffuse)) for sx in (-1.0, 1.0)] + \
               [SDFObject(SHAPE.SPHERE, Transform((0, 2.5, 0), (0, 0, 0), (0.5, 0.5, 0.5)), light)]
        objs = [objs[0], objs[1], objs[2], objs[5], objs[3], objs[4]]        # spheres first, as the reference's stable sort leaves them
    elif scene_kind == "far_camera":
        objs = [ground, SDFObject(SHAPE.SPHERE, Transform((0, 0, 0), (0, 0, 0), (0.5, 0.5, 0.5)), metal),
                SDFObject(SHAPE.CYLINDER, Transform((1.2, -0.2, 0), (0, 0, 0), (0.3, 0.3, 0.3)), diffuse)]
        cam = Camera((0, 3, 900), (0, 0, 0), (0, 1, 0), 0.4, W / H, 0.0, 900)
    elif scene_kind == "touching":
        objs = [ground, SDFObject(SHAPE.SPHERE, Transform((0, -0.2, 0), (0, 0, 0), (0.299, 0.299, 0.299)), metal),      # 0.001 above the ground
                SDFObject(SHAPE.SPHERE, Transform((0.599, -0.2, 0), (0, 0, 0), (0.3, 0.3, 0.3)), diffuse),              # 0.0 from its neighbour
                SDFObject(SHAPE.BOX, Transform((-0.63, -0.2, 0), (0, 0, 0), (0.3, 0.3, 0.3)), light)]
    elif scene_kind == "single_object":
        objs = [SDFObject(SHAPE.SPHERE, Transform((0, 0, 0), (0, 0, 0), (1, 1, 1)), metal)]
    else:
        objs = [SDFObject(SHAPE.NONE, Transform((0, 0, 0), (0, 0, 0), (1, 1, 1)), diffuse),
                SDFObject(SHAPE.PLANE, Transform((0, 0, 0), (0, 0, 0), (0, -0.6, 0)), diffuse),
                SDFObject(SHAPE.SPHERE, Transform((0, 0, 0), (0, 0, 0), (0.6, 0.6, 0.6)), metal),
                SDFObject(SHAPE.PLANE, Transform((0, 0, 0), (0, 0, 0), (0, -0.6, 0)), light),                              # an exact duplicate: ties on every step
                SDFObject(SHAPE.BOX, Transform((1.3, 0, 0), (0, 30, 0), (0.3, 0.6, 0.3)), diffuse)]
    sc = Scene(objs, False, cam, scene_kind)
    cfg = Config.src(W, H, 11, steps_per_launch=1)
    cfg.sky_kind = 0
    o = OracleRenderer(sc, cfg)
    for n in (6, 10, 24):
        o.sample(n)
    co = o.counters()
    for opts in ({"sparse_lanes": 64, "plan_interval": 4, "heavy_mean_x16": 0, "heavy_bulk_x16": 0, "tiny_own": 2, "jit": 0},
                 {"sparse_lanes": 64, "plan_interval": 8, "heavy_mean_x16": 12, "heavy_bulk_x16": 0, "heavy_own": 5, "tiny_waves": 0, "jit": 2, "jit_bake": 1},
                 {"sparse_lanes": 64, "src_plan": 0, "grid_blocks": 1, "residency": 4, "jit": 2}):
        g = Renderer(sc, cfg)
        for k, v in opts.items():
            g.set_option(k, v)
        for n in (6, 10, 24):
            g.sample(n)
        cg = g.counters()
        assert (cg.samples, cg.raycasts, cg.march_steps, cg.hits, cg.sky_lookups, cg.deposits) == \
               (co.samples, co.raycasts, co.march_steps, co.hits, co.sky_lookups, co.deposits), (scene_kind, opts)
        assert np.array_equal(bits(g.image_buffer), bits(o.image_buffer)) and np.array_equal(bits(g.ray_buffer), bits(o.ray_buffer)), (scene_kind, opts)
        g.close()


_FAKE_RCCL_SCRIPT = r"""
import sys, numpy as np
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
from cases import case_by_name
from raytracingpbr_amd import Renderer
from raytracingpbr_amd.distributed import gather_group, rccl_group
bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
case = case_by_name("cornell_v3_8b_wide")
W, H = case.cfg.width, case.cfg.height
ref = Renderer(case.scene, case.cfg); ref.sample(4); want = ref.image_buffer

def ranks(world, tile, keep=None):
    rs = keep or []
    while len(rs) < world:
        rs.append(Renderer(case.scene, case.cfg))
    for i, r in enumerate(rs[:world]):
        r.set_tiles(tile[0], tile[1], i, world)
        r.refresh(); r.set_option("sample_base", 0)
        r.sample(4)
    return rs

# G contexts of ONE process on one device: init_all + the grouped gather (SURVEY 8(e)'s single-process design)
for world, tile in ((2, (16, 16)), (3, (16, 16)), (5, (8, 8)), (8, (32, 20))):
    rs = ranks(world, tile)
    rccl_group(rs)
    assert rs[1].rccl_info()[:2] == (world, 1)
    gather_group(rs)
    rs[0].sync()
    assert np.array_equal(bits(rs[0].image_buffer), bits(want)), (world, tile)
    # a second gather after more samples: buffers are reused, the frame is still the untiled one
    for r in rs: r.sample(2)
    gather_group(rs); rs[0].sync()
    ref2 = Renderer(case.scene, case.cfg); ref2.sample(6)
    assert np.array_equal(bits(rs[0].image_buffer), bits(ref2.image_buffer)), (world, tile)
    for r in rs: r.close()
# the receive side must grow when the WORLD grows while the local share stays the same (96x54 in 48x27 tiles = 4 tiles:
# two local tiles for world 2 and for world 3) — rank 0's buffer was sized for 2 ranks first
rs = ranks(2, (48, 27))
rccl_group(rs); gather_group(rs); rs[0].sync()
assert np.array_equal(bits(rs[0].image_buffer), bits(want))
rs = ranks(3, (48, 27), keep=rs)
rccl_group(rs); gather_group(rs); rs[0].sync()
assert np.array_equal(bits(rs[0].image_buffer), bits(want))
print("FAKE-RCCL-OK")
"""


def test_multi_rank_gather_path_on_one_gpu_with_an_in_process_rccl_stand_in():
    """Everything of the N > 1 C-ABI path except RCCL itself, with N up to 8 on this box's one GPU: per-rank packing, the
    receive offsets, rank 0's unpack loop over the other ranks, the grouped launch of G contexts, buffer growth when the
    world changes.  RTPBR_RCCL_LIB points the library at tests/stubs/libfake_rccl.so (device-to-device copies with RCCL's
    stream semantics, built by __graft_entry__.build()); the gathered frame must equal the untiled one bit for bit."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    stub = os.path.join(root, "tests", "stubs", "libfake_rccl.so")
    stub = _rccl_stub()
    env = dict(os.environ, RTPBR_RCCL_LIB=stub)
    out = subprocess.run([sys.executable, "-c", _FAKE_RCCL_SCRIPT.format(root=root, tests=os.path.join(root, "tests"))], env=env,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "FAKE-RCCL-OK" in out.stdout, out.stderr[-3000:]


def test_rccl_gather_through_the_c_abi():
    """The ONE collective on RCCL directly (include/rtpbr.h: rtpbr_rccl_* / rtpbr_gather_tiles), no torch.distributed.
    One GPU here, so the communicators have one rank each: ncclCommInitRank + ncclGather to self run for real (library
    load, communicator, stream-ordered pack -> gather -> unpack), and both host styles are exercised: one process per GPU
    (unique id + init) and one process driving its contexts (init_all + grouped gather)."""
    from raytracingpbr_amd.distributed import gather_group, rccl_group
    case = case_by_name("cornell_v3_8b_wide")
    ref = Renderer(case.scene, case.cfg)
    ref.sample(5)
    want = ref.image_buffer
    r = Renderer(case.scene, case.cfg)
    r.set_tiles(16, 16, 0, 1)
    uid = r.rccl_unique_id()
    assert len(uid) == 128 and any(uid)
    r.rccl_init(uid, 0, 1)
    r.sample(5)
    r.gather_tiles()
    r.sync()
    assert np.array_equal(bits(r.image_buffer), bits(want))
    # rank/world of the communicator must match the tile partition
    r.set_tiles(16, 16, 0, 2)
    with pytest.raises(RtpbrError):
        r.gather_tiles()
    # no communicator yet -> a clear error
    f = Renderer(case.scene, case.cfg)
    with pytest.raises(RtpbrError):
        f.gather_tiles()
    g = Renderer(case.scene, case.cfg)
    g.set_tiles(16, 16, 0, 1)
    rccl_group([g])
    g.sample(5)
    gather_group([g])
    g.sync()
    assert np.array_equal(bits(g.image_buffer), bits(want))
