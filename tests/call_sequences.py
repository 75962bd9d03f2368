"""Seeded random sequences of C-ABI calls that change the context's state in the middle of a run, applied in lock step to two
renderers: the HIP library against the CPU oracle (tests/test_gpu_call_sequences.py) or two oracles of different thread counts
(tests/test_oracle_call_sequences.py).

A script is a base configuration, a first scene and a list of operations drawn from a small grammar over the public Renderer
surface: set_config (kernel form, steps_per_launch 0 included, max_raytrace, adaptive sampling, frame, sky, resolution, ...),
set_scene, set_camera, set_env, set_shape_data, set_tiles, refresh, sample(n), post_process, buffers written back, sample_base,
HIP-only options that must not change the bits, observations, and the first-hit features / denoise (HIP against
tests/feature_ref_lib.py).  Some operations are illegal in the state they are drawn in on purpose: both backends must refuse them
with the same RtpbrError code.  Every operation prints as the Python statement that replays it on a Renderer ``r``; on a mismatch
the message holds the seed, the operation's index, the operations since the last observation that matched and where the buffers
differ, and ``replay(script(seed, ...), upto=i)`` reruns the prefix.

The generator keeps clear of the argument checks only the HIP library makes (max_raymarch / max_raytrace <= 0, the per-rank
pixel limit).  The bunny's weights are a process-wide global in the oracle, so every script that renders the bunny sets the
weights it means to use on both backends first."""
import numpy as np

from oracle_backend import OracleRenderer
from raytracingpbr_amd import SHAPE, Camera, Config, Scene, bunny, cornell_box, src_scene
from raytracingpbr_amd._capi import RtpbrError
from raytracingpbr_amd.ibl import load_bunny_weights, synthetic_env

EINVAL, ESTATE = -1, -4
SIZES = ((23, 17), (40, 24), (31, 9))
COUNTERS = ("samples", "raycasts", "march_steps", "hits", "sky_lookups", "deposits")
BUFFERS = ("image_buffer", "image_pixels", "ray_buffer", "diff_buffer", "diff_pixels")

# HIP-only options whose every value gives the oracle's bits (include/rtpbr.h "Tuning knobs that do not change results", and the
# schedule-independence tests of tests/test_gpu_parity.py).  Never "precision" (the tolerance flavour), never "jit" here (the
# random scripts run the ahead-of-time kernels: no scene may start a compiler).
OPTIONS = {
    "scheduler": (-1, 0, 1), "src_split": (0, 1, 2, 256), "src_lazy": (0, 1), "src_op": tuple(range(8)), "split_wait": (1, 5, 24, 64),
    "src_track": (0, 1, 2), "sparse_lanes": (0, 8, 24, 64), "leave_x8": (1, 24, 400), "src_plan": (0, 1), "plan_interval": (1, 4, 64),
    "env_packed": (0, 1), "primary_split": (0, 1, 2), "chunk": (0, 7, 64, 777), "staging_bytes": (1 << 20, 1 << 34),
    "reserve_spp": (1, 40, 64), "timing": (0, 1),
}


# ------------------------------------------------------------------ the pools the operations draw from
def _fuzz_scene(seed):
    from fuzz import random_case
    return random_case(seed)[0]


def _box8_scene(seed):
    from fuzz import random_box8_case
    return random_box8_case(seed)[0]


# name -> scene: the gates the library branches on — Cornell v3 / v2 (x10 scale), the src/ scene and its Tokyo variant (7 mixed
# shapes), more than 8 objects (the n_obj <= 8 exchange-buffer gate) mixed and all boxes, exactly 8 boxes (rotation signatures),
# small mixed scenes, the neural bunny
SCENES = {
    "cornell_v3": lambda: cornell_box("v3", aspect=40 / 24),
    "cornell_v2": lambda: cornell_box("v2", aspect=40 / 24),
    "src": lambda: src_scene(aspect=40 / 24),
    "tokyo": lambda: src_scene(aspect=40 / 24, tokyo=True),
    "mixed10": lambda: _fuzz_scene(4),
    "boxes11": lambda: _fuzz_scene(9),
    "boxes8": lambda: _fuzz_scene(15),
    "box8_room": lambda: _box8_scene(0),
    "mixed7": lambda: _fuzz_scene(29),
    "mixed8": lambda: _fuzz_scene(7),
    "bunny": lambda: bunny(aspect=40 / 24),
}
_scene_cache = {}


def scene(name):
    if name not in _scene_cache:
        _scene_cache[name] = SCENES[name]()
    return _scene_cache[name]


def camera(name, offset=(0.0, 0.0, 0.0)):
    """the scene's own camera, its eye moved by `offset`"""
    c = scene(name).camera
    lf = tuple(float(np.float32(a + b)) for a, b in zip(c.lookfrom, offset))
    return Camera(lf, tuple(c.lookat), tuple(c.vup), c.vfov, c.aspect, c.aperture, c.focus)


def env(w, h, seed, f32):
    """an environment map as uint8 texels, or the same map as float32 texels (RGB32F: used as is)"""
    e = synthetic_env(w, h, seed=seed)
    return (e.astype(np.float32) / np.float32(255)) ** np.float32(2.2) if f32 else e


def weights(variant, n=625):
    """the bunny's weights (variant 0) or a perturbed copy (variant 1: a different but still bunny-like surface)"""
    w = load_bunny_weights()
    if variant:
        w = w.copy()
        w[-1] += np.float32(0.01)             # the output bias: the surface moves a little
    return w[:n]


def base_config(kind, w, h, seed):
    if kind == "cornell":
        return Config.cornell_v3(w, h, seed, 3)
    if kind == "src":
        return Config.src(w, h, seed, steps_per_launch=1).copy(max_raytrace=4, sky_kind=2)
    return Config.scene_demo(w, h, seed, 4)


# ------------------------------------------------------------------ operations
class Op:
    """one call of the grammar: `kind`, its arguments, the RtpbrError code it must raise (None: it must succeed)"""

    def __init__(self, kind, expect=None, **args):
        self.kind, self.expect, self.args = kind, expect, args

    def code(self):
        a, k = self.args, self.kind
        if k == "set_config":
            return f"r.set_config(BASE.copy(**{a['over']!r}))"
        if k == "set_scene":
            return f"r.set_scene(cs.scene({a['name']!r}))"
        if k == "set_camera":
            return f"r.set_camera(cs.camera({a['name']!r}, {a['offset']!r}))"
        if k == "set_env":
            return f"r.set_env(cs.env({a['w']}, {a['h']}, {a['seed']}, {a['f32']}), {a['exposure']}, {a['gamma']})"
        if k == "set_shape_data":
            return f"r.set_shape_data(SHAPE.BUNNY, cs.weights({a['variant']}, {a['n']}))"
        if k == "set_tiles":
            return f"r.set_tiles(*{a['tiles']!r})"
        if k == "bad_scene":
            return "r.set_scene(Scene(list(cs.scene('src').objects) * 5, False, cs.camera('src')))   # 35 objects"
        if k == "sample":
            return f"r.sample({a['n']})"
        if k == "write_image":
            return "ib = r.image_buffer; ib[..., :3] *= np.float32(0.5); r.image_buffer = ib"
        if k == "write_rays":
            return "rb = r.ray_buffer; rb[..., 6:9] *= np.float32(0.75); r.ray_buffer = rb"
        if k == "sample_base":
            return f"r.set_option('sample_base', {a['value']})   # oracle: r.set_sample_base({a['value']})"
        if k == "option":
            return f"r.set_option({a['key']!r}, {a['value']})   # HIP only"
        if k == "observe":
            return f"# observe {a['what']}"
        if k == "features":
            return "r.render_features()   # HIP only, against tests/feature_ref_lib.py"
        if k == "denoise":
            return f"r.denoise(**{a['params']!r})   # HIP only, against tests/feature_ref_lib.py"
        return f"r.{k}()"

    def __repr__(self):
        return self.code() + ("" if self.expect is None else f"   # must raise RtpbrError {self.expect}")


class Script:
    def __init__(self, seed, base, scene0, ops, jit=0):
        self.seed, self.base, self.scene0, self.ops, self.jit = seed, base, scene0, ops, jit

    def header(self):
        b = self.base
        return (f"BASE = Config.from_buffer_copy(bytes.fromhex({bytes(b).hex()!r}))   # {b.width}x{b.height}, form {b.kernel_form}\n"
                f"r = Renderer(cs.scene({self.scene0!r}), BASE, cs.camera({self.scene0!r}))   # and OracleRenderer(...) alike"
                + ("" if self.jit is None else f"; r.set_option('jit', {self.jit})"))


class Mirror:
    """what the generator knows of the context: enough to keep the script legal where it means to and to compute the features"""

    def __init__(self, base, scene0):
        self.base, self.cfg, self.scene, self.cam = base, base.copy(), scene0, (scene0, (0.0, 0.0, 0.0))
        self.env = False
        self.weights = None
        self.tiles = (0, 0, 0, 1)

    def over(self, cfg):
        """the fields of `cfg` that differ from the base configuration"""
        b = self.base
        return {k: getattr(cfg, k) for k, _ in Config._fields_ if getattr(cfg, k) != getattr(b, k)}


def script(seed, n_ops=60, jit=0, scenes=None, forms=(0, 1)):
    """A reproducible call sequence: seed -> Script.  `scenes`: the scene pool (all of SCENES by default); `forms`: the kernel
    forms set_config may switch between."""
    rng = np.random.default_rng(seed)
    pick = lambda seq: seq[int(rng.integers(0, len(seq)))]      # noqa: E731
    pool = list(scenes or SCENES)
    w, h = pick(SIZES)
    base = base_config(pick(("cornell", "src", "demo")), w, h, seed)
    base.kernel_form = pick(forms)
    scene0 = pick([s for s in pool if s != "bunny"])
    m = Mirror(base, scene0)
    ops = []

    def add(op):
        ops.append(op)
        return op

    def set_config(cfg):
        add(Op("set_config", over=m.over(cfg)))
        m.cfg = cfg

    while len(ops) < n_ops:
        u = rng.random()
        cfg = m.cfg.copy()
        if u < 0.16:                                                        # sample(n)
            n = pick((0, 1, 1, 1, 2, 3, 3, 17, 40)) if m.scene != "bunny" else pick((0, 1, 2))
            if rng.random() < 0.03:
                add(Op("sample", EINVAL, n=-1))
                continue
            add(Op("sample", None if (m.cfg.sky_kind != 1 or m.env) else ESTATE, n=n))
            if rng.random() < 0.5:
                add(Op("observe", what=pick(("image", "image", "all"))))
        elif u < 0.24:
            add(Op("post_process"))
        elif u < 0.28:
            add(Op("refresh"))
        elif u < 0.44:                                                      # set_config at the same resolution
            k = int(rng.integers(0, 10))
            if k <= 2 and len(forms) > 1:
                cfg.kernel_form = 1 - cfg.kernel_form
            if k in (1, 3) or (k == 0 and rng.random() < 0.5):
                cfg.steps_per_launch = pick((0, 1, 1, 2, 3))
            if k == 4:
                cfg.max_raytrace = int(rng.integers(1, 5))
            if k == 5:
                cfg.adaptive_sampling = 1 - cfg.adaptive_sampling
                cfg.noise_threshold = float(pick((0.02, 0.08, 0.3)))
            if k == 6:
                cfg.frame = int(pick((0, 17, 45)))
            if k == 7:
                cfg.sky_kind = int(pick((0, 1, 1, 2)))           # ENVMAP: a sample() before any set_env is refused (ESTATE)
            if k == 8:
                cfg.box_round = float(pick((0.0, 0.01, 0.03)))
                cfg.max_dis = float(pick((1e3, 2000.0)))
            if k == 9:
                cfg.exposure = float(pick((0.6, 1.0, 1.3)))
                cfg.tonemap_order = int(rng.integers(0, 4))
            set_config(cfg)
            if k == 5 and rng.random() < 0.5:
                add(Op("refresh"))
        elif u < 0.48:                                                      # set_config at a new resolution: buffers reallocated
            cfg.width, cfg.height = pick([s for s in SIZES if s != (cfg.width, cfg.height)])
            set_config(cfg)
        elif u < 0.54:                                                      # set_scene (+ its camera, mostly)
            name = pick(pool)
            if name == "bunny" and (m.weights is None or rng.random() < 0.3):
                v = int(rng.integers(0, 2))
                add(Op("set_shape_data", variant=v, n=625))
                m.weights = v
            add(Op("set_scene", name=name))
            m.scene = name
            if rng.random() < 0.7:
                add(Op("set_camera", name=name, offset=(0.0, 0.0, 0.0)))
                m.cam = (name, (0.0, 0.0, 0.0))
        elif u < 0.59:                                                      # set_camera: a small pose offset
            off = tuple(float(np.float32(x)) for x in rng.uniform(-0.3, 0.3, 3))
            add(Op("set_camera", name=m.scene, offset=off))
            m.cam = (m.scene, off)
        elif u < 0.63:                                                      # set_env: RGB8 <-> RGB32F, size, exposure, gamma
            add(Op("set_env", w=int(pick((64, 48, 16))), h=int(pick((32, 24, 8))), seed=int(rng.integers(0, 3)), f32=bool(rng.random() < 0.4),
                   exposure=float(pick((1.0, 1.4, 1.8))), gamma=float(pick((1.0, 2.2)))))
            m.env = True
        elif u < 0.67:                                                      # set_tiles
            world = int(pick((1, 1, 2, 3, 4)))
            tiles = (0, 0, 0, 1) if world == 1 and rng.random() < 0.5 else \
                (int(pick((5, 7, 9, 13, 19))), int(pick((3, 7, 11))), int(rng.integers(0, world)), world)
            add(Op("set_tiles", tiles=tiles))
            m.tiles = tiles
        elif u < 0.71:                                                      # buffers written back (checkpoint / resume)
            add(Op(pick(("write_image", "write_rays"))))
        elif u < 0.74:
            add(Op("sample_base", value=int(rng.integers(0, 1000))))
        elif u < 0.84:                                                      # HIP-only options that keep the bits
            key = pick(list(OPTIONS))
            add(Op("option", key=key, value=int(pick(OPTIONS[key]))))
            if key == "staging_bytes" and ops[-1].args["value"] == 1 << 20 and m.scene != "bunny" and rng.random() < 0.7:
                # a complete-path call of 100 spp outgrows 1 MiB of staging at 40x24 (14 B per sample): several sub-launches
                add(Op("sample", None if (m.cfg.sky_kind != 1 or m.env) else ESTATE, n=100))
                add(Op("observe", what="all"))
        elif u < 0.90:
            add(Op("observe", what=pick(("image", "all"))))
        elif u < 0.95:                                                      # first-hit features / denoise (whole frames only)
            bad = m.tiles[3] > 1
            if rng.random() < 0.4:
                add(Op("features", ESTATE if bad else None))
            else:
                params = pick(({}, {"iterations": 0}, {"iterations": 2, "demodulate": 1}, {"iterations": 3, "sigma_color": 0.5}))
                add(Op("denoise", ESTATE if bad else None, params=params))
        else:                                                               # illegal in any state: refused alike, nothing changes
            k = int(rng.integers(0, 5))
            if k == 0:
                add(Op("set_config", EINVAL, over=dict(m.over(m.cfg), width=0)))
            elif k == 1:
                add(Op("set_tiles", EINVAL, tiles=(8, 8, 2, 2)))
            elif k == 2:
                add(Op("set_shape_data", EINVAL, variant=0, n=624))
            elif k == 3:
                add(Op("set_env", EINVAL, w=0, h=8, seed=0, f32=False, exposure=1.0, gamma=1.0))
            else:
                add(Op("bad_scene", EINVAL))
            add(Op("observe", what="all"))
    add(Op("post_process"))
    add(Op("observe", what="all"))
    return Script(seed, base, scene0, ops, jit)



# ------------------------------------------------------------------ the lock-step driver
def _is_hip(r):
    return not isinstance(r, OracleRenderer)


def _apply(op, r):
    """apply one operation to one renderer; returns None or ("error", code)"""
    a, k = op.args, op.kind
    try:
        if k == "set_config":
            r.set_config(r._cs_base.copy(**a["over"]))
        elif k == "set_scene":
            r.set_scene(scene(a["name"]))
        elif k == "bad_scene":
            r.set_scene(Scene(list(scene("src").objects) * 5, False, camera("src")))
        elif k == "set_camera":
            r.set_camera(camera(a["name"], a["offset"]))
        elif k == "set_env":
            if a["w"] == 0:
                r.set_env(np.zeros((0, a["h"], 3), np.uint8), a["exposure"], a["gamma"])
            else:
                r.set_env(env(a["w"], a["h"], a["seed"], a["f32"]), a["exposure"], a["gamma"])
        elif k == "set_shape_data":
            r.set_shape_data(SHAPE.BUNNY, weights(a["variant"], a["n"]))
        elif k == "set_tiles":
            r.set_tiles(*a["tiles"])
        elif k == "sample":
            r.sample(a["n"])
        elif k == "post_process":
            r.post_process()
        elif k == "refresh":
            r.refresh()
        elif k == "write_image":
            ib = r.image_buffer
            ib[..., :3] *= np.float32(0.5)
            r.image_buffer = ib
        elif k == "write_rays":
            rb = r.ray_buffer
            rb[..., 6:9] *= np.float32(0.75)
            r.ray_buffer = rb
        elif k == "sample_base":
            if _is_hip(r):
                r.set_option("sample_base", a["value"])
            else:
                r.set_sample_base(a["value"])
        elif k == "option":
            if _is_hip(r):
                r.set_option(a["key"], a["value"])
        elif k == "features":
            if _is_hip(r):
                r.render_features()
        elif k == "denoise":
            if _is_hip(r):
                r.denoise(**a["params"])
    except RtpbrError as e:
        return ("error", e.code)
    return None


def observe(r, what):
    """{name: array or tuple} of what an observation reads"""
    if what == "image":
        return {"image_buffer": r.image_buffer}
    out = {b: getattr(r, b) for b in BUFFERS}
    c = r.counters()
    out["counters"] = tuple(getattr(c, k) for k in COUNTERS)
    return out


def _first_diff(x, y):
    if isinstance(x, tuple):
        return None if x == y else f"{x} != {y}"
    if x.shape != y.shape:
        return f"shapes {x.shape} != {y.shape}"
    bad = np.ascontiguousarray(x).view(np.uint32) != np.ascontiguousarray(y).view(np.uint32)
    if not bad.any():
        return None
    return f"{int(bad.sum())} of {bad.size} words differ, first at {[tuple(int(v) for v in p) for p in np.argwhere(bad)[:4]]}"


class Mismatch(AssertionError):
    pass


def new_renderer(s, cls, **kw):
    """the script's renderer: `cls` is Renderer (HIP) or OracleRenderer"""
    r = cls(scene(s.scene0), s.base, camera(s.scene0), **kw)
    r._cs_base = s.base
    if _is_hip(r) and s.jit is not None:
        r.set_option("jit", s.jit)
    return r


def _feature_mirror(s, upto):
    """(scene name, config, camera, bunny weights variant) after the first `upto` operations that succeeded"""
    m = Mirror(s.base, s.scene0)
    for op in s.ops[:upto]:
        if op.expect is not None:
            continue
        a = op.args
        if op.kind == "set_config":
            m.cfg = s.base.copy(**a["over"])
        elif op.kind == "set_scene":
            m.scene = a["name"]
        elif op.kind == "set_camera":
            m.cam = (a["name"], a["offset"])
        elif op.kind == "set_shape_data":
            m.weights = a["variant"]
    return m


def _check_features(s, i, r):
    import feature_ref_lib as fr
    m = _feature_mirror(s, i + 1)
    sc = scene(m.scene)
    w = weights(m.weights) if any(o.type == SHAPE.BUNNY for o in sc.objects) else None
    ref = fr.features(sc, m.cfg, camera(*m.cam), w)
    got = {"feature_albedo": r.feature_albedo, "feature_normal": r.feature_normal, "feature_depth": r.feature_depth,
           "feature_object": r.feature_object}
    seen = dict(zip(got, (ref["albedo"], ref["normal"], ref["depth"], ref["object"])))
    out = {k: (got[k], seen[k]) for k in got}
    if s.ops[i].kind == "denoise":
        out["denoised_pixels"] = (r.denoised_pixels, fr.denoise(m.cfg, r.image_buffer, ref, **s.ops[i].args["params"]))
    return out


def run(s, a, b, upto=None, features=True):
    """Apply the script's operations to renderers `a` and `b` in lock step and compare every observation bit for bit (a HIP
    renderer's first-hit features and denoised pixels against tests/feature_ref_lib.py when `features`).  Raises Mismatch with a
    replayable report; returns the list of (operation index, observed name, value) of `a`."""
    seen, last_ok, last_ok_of = [], -1, {}
    ops = s.ops if upto is None else s.ops[:upto]

    def fail(i, what, key=None):
        # (the window starts after the last observation that matched this buffer — for the counters, the last counters read)
        start = last_ok_of.get(key, -1) if key is not None else last_ok
        lines = [f"call sequence seed {s.seed}, operation #{i}: {what}", s.header(),
                 f"operations since the last observation that matched (#{start + 1}..#{i}):"]
        lines += [f"  [{j}] {s.ops[j]!r}" for j in range(start + 1, i + 1)]
        lines.append(f"replay: call_sequences.replay(call_sequences.script({s.seed}, ...), upto={i + 1})")
        raise Mismatch("\n".join(lines))

    for i, op in enumerate(ops):
        ra, rb = _apply(op, a), _apply(op, b)
        ca = None if ra is None else ra[1]
        cb = None if rb is None else rb[1]
        # (the features and the denoise have no oracle counterpart: an oracle skips them)
        hip_only = op.kind in ("features", "denoise")
        if (ca != op.expect and (_is_hip(a) or not hip_only)) or (cb != op.expect and (_is_hip(b) or not hip_only)):
            fail(i, f"{op.kind} returned {ca} / {cb}, expected {op.expect}")
        obs = {}
        if op.kind == "observe":
            oa, ob = observe(a, op.args["what"]), observe(b, op.args["what"])
            obs = {k: (oa[k], ob[k]) for k in oa}
        elif op.kind == "post_process":
            obs = {k: (getattr(a, k), getattr(b, k)) for k in ("image_pixels", "diff_buffer", "diff_pixels")}
        elif op.kind in ("features", "denoise") and op.expect is None and features and _is_hip(a):
            obs = _check_features(s, i, a)
        for k, (x, y) in obs.items():
            d = _first_diff(x, y)
            if d is not None:
                fail(i, f"{k} differs: {d}", k)
            seen.append((i, k, x))
            last_ok_of[k] = i
        if obs:
            last_ok = i
    return seen


def replay(s, upto=None, threads=0):
    """rerun a script (or its first `upto` operations) on a fresh HIP renderer against a fresh oracle"""
    from raytracingpbr_amd import Renderer
    a, b = new_renderer(s, Renderer), new_renderer(s, OracleRenderer, threads=threads)
    try:
        return run(s, a, b, upto)
    finally:
        a.close()
        b.close()
