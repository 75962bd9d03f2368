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

``post_script(seed)`` draws from the same grammar and, for about half of its operations, from the calls that keep state beside
the sample path: rtpbr_reproject, rtpbr_noise_update / _estimate / rtpbr_denoise_guided, rtpbr_set_noise_estimator, the select
calls, rtpbr_sample_selected, rtpbr_present and a "post" observation of the buffers they own.  Those run on the HIP library
against the model of tests/post_model.py (``run_post``), whose refusal codes are written from include/rtpbr.h.  script() itself
draws what it always drew (tests/test_oracle_call_sequences.py pins a hash of its scripts).

``motion_script(seed)`` draws a third of its operations from script()'s grammar, a third from post_script()'s and a third from
the two newest stateful calls: rtpbr_reproject_scene — rigid moves on top of the pose the context is in (``posed``), with and
without a camera, empty moves, turns of 360 degrees, tables that are no rigid motion (``nonrigid``), on every scene of the pool,
in both normal spaces, under tiles, after a new resolution — and rtpbr_set_noise_tracking with the tracked rtpbr_sample /
rtpbr_sample_selected calls and what they refuse.  It runs against post_model.MotionModel.  post_script() draws what it drew as
well (a second pinned hash): its draws are _Grammar.post_op().

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
POST_SIZES = SIZES + ((67, 45),)      # a multiple of neither the pooled estimator's 16 x 16 tile nor the present kernel's 64 x 64, wider than 64
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


def camera(name, offset=(0.0, 0.0, 0.0), vfov=1.0):
    """the scene's own camera, its eye moved by `offset`, its field of view scaled by `vfov`"""
    c = scene(name).camera
    lf = tuple(float(np.float32(a + b)) for a, b in zip(c.lookfrom, offset))
    return Camera(lf, tuple(c.lookat), tuple(c.vup), float(np.float32(c.vfov * vfov)), c.aspect, c.aperture, c.focus)


def posed(name, pose=()):
    """scene `name` after the moves of `pose`, applied one after the other: each is {object index: (dpos, drot)} as
    reproject_scene_ref_lib.moved_scene takes it (a pose is what rtpbr_reproject_scene calls have done since the last set_scene)"""
    if not pose:
        return scene(name)
    key = (name, repr(pose))
    if key not in _scene_cache:
        import reproject_scene_ref_lib as rs
        sc = scene(name)
        for moves in pose:
            sc = rs.moved_scene(sc, moves)
        _scene_cache[key] = sc
    return _scene_cache[key]


def nonrigid(name, pose, what, k=0, other=None):
    """a table that is no rigid motion of posed(name, pose): the table of scene `other` (another object count), or object k with
    one scale word, one material word or its type changed"""
    if what == "count":
        return scene(other)
    sc = posed(name, pose)
    objs = [type(o).from_buffer_copy(bytes(o)) for o in sc.objects]
    o = objs[k]
    if what == "scale":
        o.transform.scale[2] = o.transform.scale[2] * 1.25 + 0.01
    elif what == "material":
        o.material.albedo[1] = o.material.albedo[1] * 0.5 + 0.05
    else:
        o.type = int(SHAPE.BOX if o.type != SHAPE.BOX else SHAPE.SPHERE)
    return Scene(objs, sc.scale10, sc.camera, sc.name)


def mask(w, h, seed, share):
    """a host mask for select_mask: about `share` of the pixels (0.0: none, 1.0: all)"""
    return (np.random.default_rng(seed).random((w, h)) < share).astype(np.uint8)


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

    def __init__(self, kind, expect=None, why=(), **args):
        self.kind, self.expect, self.args = kind, expect, args
        self.why = tuple(why)               # the reasons for `expect` (post_script: the coverage conditions read them)

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
        if k == "noise_estimate":
            return f"r.noise_estimate({a['threshold']})"
        if k == "denoise_guided":
            return f"r.denoise_guided(**{a['params']!r})"
        if k == "set_noise_estimator":
            return "r.api.call('set_noise_estimator', r._ctx, None)   # NULL: the defaults" if a["e"] is None else f"r.set_noise_estimator(*{a['e']!r})"
        if k == "select_mask":
            return f"r.select_mask(cs.mask(r.config.width, r.config.height, {a['seed']}, {a['share']}))"
        if k == "select_noisy":
            return f"r.select_noisy({a['threshold']}, {a['dilate']})"
        if k == "sample_selected":
            return f"r.sample_selected({a['n']})"
        if k == "reproject":
            return f"r.reproject(cs.camera({a['name']!r}, {a['offset']!r}, {a['vfov']}), **{a['params']!r})"
        if k == "present":
            return f"r.present({a['source']!r}, {a['format']!r}, {a['dither']})"
        if k == "reproject_scene":
            cam = "None" if a["cam"] is None else f"cs.camera({a['cam'][0]!r}, {a['cam'][1]!r}, {a['cam'][2]})"
            table = f"cs.posed({a['name']!r}, {a['pose']!r})" if a["bad"] is None else \
                f"cs.nonrigid({a['name']!r}, {a['pose']!r}, {a['bad']!r}, {a['k']}, {a['other']!r})"
            return f"r.reproject_scene({table}, {cam}, **{a['params']!r})"
        if k == "set_noise_tracking":
            return f"r.set_noise_tracking({bool(a['mode'])})" if a["mode"] in (0, 1) else f"r.api.call('set_noise_tracking', r._ctx, {a['mode']})"
        return f"r.{k}()"                   # refresh, post_process, noise_update

    def __repr__(self):
        return self.code() + ("" if self.expect is None else f"   # must raise RtpbrError {self.expect}")


class Script:
    def __init__(self, seed, base, scene0, ops, jit=0, post=False, motion=False):
        self.seed, self.base, self.scene0, self.ops, self.jit, self.post = seed, base, scene0, ops, jit, post
        self.motion = motion                # a motion_script: runs on post_model.MotionModel

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


class _Grammar:
    """the random stream of one script and the operations drawn from it so far; `state_cls`: the mirror's class (post_script passes
    post_model.PostState, which follows every operation that is meant to succeed through its note())"""

    def __init__(self, seed, scenes, forms, sizes, state_cls=None):
        self.rng = np.random.default_rng(seed)
        self.pool, self.forms, self.sizes = list(scenes or SCENES), forms, sizes
        w, h = self.pick(sizes)
        self.base = base_config(self.pick(("cornell", "src", "demo")), w, h, seed)
        self.base.kernel_form = self.pick(forms)
        self.scene0 = self.pick([s for s in self.pool if s != "bunny"])
        self.m = (state_cls or Mirror)(self.base, self.scene0)
        self.ops = []

    def pick(self, seq):
        return seq[int(self.rng.integers(0, len(seq)))]

    def add(self, op):
        if hasattr(self.m, "stamp"):        # the state may stamp an operation of old_op again, or drop it (None)
            op = self.m.stamp(op)
            if op is None:
                return None
        self.ops.append(op)
        if op.expect is None and hasattr(self.m, "note"):
            self.m.note(op)
        return op

    def old_op(self):
        """one draw of the grammar up to render_features / denoise (one or a few operations)"""
        rng, pick, pool, forms, m, ops, add = self.rng, self.pick, self.pool, self.forms, self.m, self.ops, self.add

        def set_config(cfg):
            add(Op("set_config", over=m.over(cfg)))
            m.cfg = cfg

        u = rng.random()
        cfg = m.cfg.copy()
        if u < 0.16:                                                        # sample(n)
            n = pick((0, 1, 1, 1, 2, 3, 3, 17, 40)) if m.scene != "bunny" else pick((0, 1, 2))
            if rng.random() < 0.03:
                add(Op("sample", EINVAL, n=-1))
                return
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
            cfg.width, cfg.height = pick([s for s in self.sizes if s != (cfg.width, cfg.height)])
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

    # ---- the draws of post_script (tests/test_oracle_call_sequences.py pins their order and their use of the random stream)
    def new(self, kind, **args):
        """an operation of the calls beside the sample path: the state stamps it with the code it must raise"""
        op = Op(kind, **args)
        op.expect, why = self.m.refusal(op)
        op.why = tuple(why)
        return self.add(op)

    def spp(self):
        m, pick = self.m, self.pick
        return int(pick((1, 2)) if m.scene == "bunny" else pick((1, 2, 3)) if m.cfg.kernel_form == 0 else pick((2, 4, 6)))

    def sample(self, n):
        self.add(Op("sample", None if (self.m.cfg.sky_kind != 1 or self.m.env) else ESTATE, n=n))

    def whole_frame(self, p=0.75):
        if self.m.tiles[3] > 1 and self.rng.random() < p:
            self.add(Op("set_tiles", tiles=(0, 0, 0, 1)))

    def clean(self):
        """no reason for ESTATE may hold where a bad argument is drawn"""
        return self.m.tiles[3] == 1

    def reproject(self, **over):
        rng, pick, m = self.rng, self.pick, self.m
        scale = float(pick((1.0, 1.0, 3.0)))
        off = tuple(float(np.float32(x * scale)) for x in rng.uniform(-0.3, 0.3, 3))
        vfov = float(pick((1.0, 1.0, 1.0, 1.1, 0.9)))
        a = dict(name=m.scene, offset=off, vfov=vfov, params=dict(pick(REPROJECT)))
        a.update(over)
        return self.new("reproject", **a)

    def one(self, kind):
        rng, pick, m, new = self.rng, self.pick, self.m, self.new
        if kind == "noise_update":
            new(kind)
        elif kind == "noise_estimate":
            new(kind, threshold=float(pick(THRESHOLDS)))
        elif kind == "denoise_guided":
            new(kind, params=dict(pick(GUIDED)))
        elif kind == "select_mask":
            new(kind, seed=int(rng.integers(0, 1000)), share=float(pick((0.0, 0.1, 0.3, 0.5, 1.0))))
        elif kind == "select_noisy":
            new(kind, threshold=float(pick(THRESHOLDS)), dilate=int(rng.integers(0, 4)))
        elif kind == "sample_selected":
            new(kind, n=int(pick((0, 1, 2)) if m.scene == "bunny" else pick((0, 1, 1, 2, 3))))
        elif kind == "reproject":
            self.reproject()
        elif kind == "present":
            new(kind, source=pick(("pixels", "denoised", "accum")), format=pick(("rgb8", "rgba8")), dither=bool(rng.random() < 0.5))

    def post_op(self):
        """one draw of post_script beside old_op: the calls that keep state beside the sample path (one or a few operations)"""
        rng, pick, m, add, forms = self.rng, self.pick, self.m, self.add, self.forms
        new, spp, sample, whole_frame, clean, reproject, one = self.new, self.spp, self.sample, self.whole_frame, self.clean, self.reproject, self.one
        u = rng.random()
        if u < 0.17:                                                        # one batch of the noise estimate
            whole_frame()
            sample(spp())
            new("noise_update")
        elif u < 0.26:                                                      # noise_estimate
            whole_frame()
            if clean() and rng.random() < 0.06:
                new("noise_estimate", threshold=float(pick((-1.0, -0.02))))
            else:
                one("noise_estimate")
        elif u < 0.35:                                                      # denoise_guided (+ the denoised frame presented)
            whole_frame()
            if clean() and rng.random() < 0.06:
                new("denoise_guided", params=dict(pick(({"iterations": 9}, {"demodulate": 2}, {"sigma_color": 0.0}, {"variance_floor": -1.0}))))
            else:
                one("denoise_guided")
                if rng.random() < 0.5:
                    new("present", source="denoised", format=pick(("rgb8", "rgba8")), dither=bool(rng.random() < 0.5))
        elif u < 0.42:                                                      # the estimator setting: plain state, valid in any state
            e = pick(BAD_ESTIMATORS) if rng.random() < 0.15 else pick(ESTIMATORS)
            new("set_noise_estimator", e=e)
            if rng.random() < 0.5:
                whole_frame()
                one("noise_estimate")
        elif u < 0.48:
            whole_frame()
            one("select_mask")
        elif u < 0.58:                                                      # select_noisy, from moments of two batches mostly
            whole_frame()
            if clean() and rng.random() < 0.06:
                new("select_noisy", threshold=float(pick(THRESHOLDS)), dilate=int(pick((-1, 4))))
            else:
                if "moments" not in m.exists and rng.random() < 0.7:
                    for _ in range(2):
                        sample(spp())
                        new("noise_update")
                one("select_noisy")
        elif u < 0.70:                                                      # sample_selected
            whole_frame()
            if m.cfg.kernel_form != 0 and 0 in forms and rng.random() < 0.7:
                cfg = m.cfg.copy(kernel_form=0)
                add(Op("set_config", over=m.over(cfg)))
                m.cfg = cfg
            if not m.selected and clean() and rng.random() < 0.8:
                one(pick(("select_mask", "select_noisy")))
            if not m.state_reasons(Op("sample_selected", n=1)) and rng.random() < 0.04:
                new("sample_selected", n=-1)
            else:
                one("sample_selected")
                if rng.random() < 0.6:
                    add(Op("observe", what=pick(("image", "all"))))
        elif u < 0.82:                                                      # reproject, mostly with history to warp
            whole_frame()
            if m.dirty and rng.random() < 0.8:
                add(Op("refresh"))
                sample(spp())
                if rng.random() < 0.5:
                    new("noise_update")
            if not m.state_reasons(Op("reproject")) and rng.random() < 0.05:
                reproject(params=dict(pick(({"max_history": 0.0}, {"depth_tolerance": -0.1}, {"normal_cos": 1.5}, {"max_history": -2.0}))))
            else:
                ok = reproject().expect is None
                if ok and rng.random() < 0.4:                               # the warped moments take the next batch
                    sample(spp())
                    new("noise_update")
                    one("noise_estimate")
                elif ok and rng.random() < 0.5:
                    add(Op("observe", what="all"))
        elif u < 0.90:                                                      # present; then nothing else has moved
            one("present")
            if rng.random() < 0.4:
                add(Op("observe", what="all"))
                add(Op("observe", what="post"))
        elif u < 0.94:
            add(Op("observe", what="post"))
        elif u < 0.97:                                                      # every whole-frame call is refused with tiles of world > 1
            add(Op("set_tiles", tiles=(int(pick((5, 7, 9, 13, 19))), int(pick((3, 7, 11))), int(rng.integers(0, 2)), 2)))
            for i in rng.permutation(len(POST_KINDS))[:4]:
                one(POST_KINDS[int(i)])                                     # ... except present
            add(Op("set_tiles", tiles=(0, 0, 0, 1)))
        else:                                                               # reproject after each of the four calls that end a history
            whole_frame(1.0)
            add(Op("refresh"))
            who = pick(("set_config", "set_scene", "set_shape_data", "set_env"))
            if who == "set_config":
                cfg = m.cfg.copy(exposure=float(pick((0.7, 0.9, 1.1))))
                add(Op("set_config", over=m.over(cfg)))
                m.cfg = cfg
            elif who == "set_scene":
                add(Op("set_scene", name=m.scene))
            elif who == "set_shape_data":
                v = int(rng.integers(0, 2))
                add(Op("set_shape_data", variant=v, n=625))
                m.weights = v
            else:
                add(Op("set_env", w=16, h=8, seed=int(rng.integers(0, 3)), f32=False, exposure=1.0, gamma=2.2))
                m.env = True
            reproject()

    # ---- the draws of motion_script: rtpbr_reproject_scene, rtpbr_set_noise_tracking and the tracked sample calls
    def set_config(self, **over):
        cfg = self.m.cfg.copy(**over)
        self.add(Op("set_config", over=self.m.over(cfg)))
        self.m.cfg = cfg

    def history(self, p=0.85):
        """mostly: no reason left to refuse a reprojection, and samples to warp"""
        rng, m = self.rng, self.m
        self.whole_frame(0.9)
        if m.dirty and rng.random() < p:
            self.add(Op("refresh"))
            if m.tracking and m.cfg.kernel_form != 0 and 0 in self.forms:
                self.set_config(kernel_form=0)
                self.add(Op("refresh"))
            self.sample(self.spp())
            if not m.tracking and rng.random() < 0.5:
                self.new("noise_update")

    def move(self):
        """one move: {object index: (dpos, drot)} over one to three objects or all of them; now and then empty, now and then a
        turn of exactly 360 degrees"""
        rng, pick = self.rng, self.pick
        n = len(scene(self.m.scene).objects)
        u = rng.random()
        if u < 0.08:
            return {}
        who = range(n) if u < 0.3 else sorted(int(i) for i in rng.permutation(n)[:int(rng.integers(1, 4))])
        out = {}
        for k in who:
            step = float(pick((0.02, 0.02, 0.05, 0.05, 0.1, 0.2)))
            dpos = tuple(round(float(x), 3) for x in rng.uniform(-step, step, 3))
            drot = [0.0, 0.0, 0.0]
            drot[int(rng.integers(0, 3))] = float(pick((0.0, 0.0, 3.0, -3.0, 7.0, -7.0)))
            out[k] = (dpos, tuple(drot))
        if rng.random() < 0.12:
            k = int(pick(list(out)))
            drot = [0.0, 0.0, 0.0]
            drot[int(rng.integers(0, 3))] = 360.0
            out[k] = (out[k][0] if rng.random() < 0.5 else (0.0, 0.0, 0.0), tuple(drot))
        return out

    def reproject_scene(self, bad=None, **over):
        rng, pick, m = self.rng, self.pick, self.m
        cam = None
        if rng.random() < 0.5:
            scale = float(pick((1.0, 1.0, 3.0)))
            cam = (m.scene, tuple(float(np.float32(x * scale)) for x in rng.uniform(-0.3, 0.3, 3)), float(pick((1.0, 1.0, 1.0, 1.1, 0.9))))
        a = dict(name=m.scene, pose=m.pose + (self.move(),), cam=cam, params=dict(pick(REPROJECT)), bad=bad, k=0, other=None)
        if bad == "count":
            n = len(scene(m.scene).objects)
            a["other"] = pick([s for s in self.pool if len(scene(s).objects) != n])
        elif bad is not None:
            a["pose"], a["k"] = m.pose, int(rng.integers(0, len(scene(m.scene).objects)))
        a.update(over)
        return self.new("reproject_scene", **a)

    def tracking_on(self):
        """tracked mode on where a tracked sample can succeed: whole frame, complete-path form"""
        m = self.m
        self.whole_frame(1.0)
        if m.cfg.kernel_form != 0 and 0 in self.forms:
            self.set_config(kernel_form=0)
        if m.cfg.sky_kind == 1 and not m.env:
            self.set_config(sky_kind=2)
        if not m.tracking:
            self.new("set_noise_tracking", mode=1)

    def tracked_n(self):
        return int(self.pick((1, 2)) if self.m.scene == "bunny" else self.pick((1, 2, 3, 8, 12)))

    def motion_op(self):
        """one draw of the two newest stateful calls (one or a few operations)"""
        rng, pick, m, add, new = self.rng, self.pick, self.m, self.add, self.new
        u = rng.random()
        if u < 0.36:                                                        # reproject_scene, mostly with history to warp
            self.history()
            if not m.state_reasons(Op("reproject_scene")) and rng.random() < 0.17:
                if rng.random() < 0.2:
                    self.reproject_scene(params=dict(pick(({"max_history": 0.0}, {"depth_tolerance": -0.1}, {"normal_cos": 1.5}, {"max_history": -2.0}))))
                else:
                    op = self.reproject_scene(bad=pick(("count", "scale", "material", "type")))
                    assert op.expect == EINVAL, op
                return
            ok = self.reproject_scene().expect is None
            v = rng.random()
            if ok and v < 0.35:                                             # the warped moments take the next batch (or the next samples)
                self.sample(self.tracked_n() if m.tracking else self.spp())
                new("noise_update")
                self.one("noise_estimate")
            elif ok and v < 0.6:                                            # poses accumulate
                if rng.random() < 0.5:
                    self.sample(self.spp())
                self.reproject_scene()
                add(Op("observe", what="all"))
            elif ok and v < 0.8:
                add(Op("observe", what="all"))
                if rng.random() < 0.5:
                    add(Op("observe", what="post"))
        elif u < 0.46:                                                      # the mode, on and off
            if m.tiles[3] == 1 and rng.random() < 0.12:
                new("set_noise_tracking", mode=2)
            elif m.tracking and rng.random() < 0.75:
                new("set_noise_tracking", mode=0)
            else:
                if rng.random() < 0.8:
                    self.whole_frame(1.0)
                new("set_noise_tracking", mode=1)
                if rng.random() < 0.5:
                    add(Op("observe", what="post"))
        elif u < 0.74:                                                      # tracked samples
            self.tracking_on()
            v = rng.random()
            if v < 0.2:                                                     # ... after what acts on the moments and the snapshot
                what = pick(("write_image", "refresh", "resolution"))
                if what == "resolution":
                    w, h = pick([s for s in self.sizes if s != (m.cfg.width, m.cfg.height)])
                    self.set_config(width=w, height=h)
                else:
                    add(Op(what))
            if v < 0.55 or not (m.selected or self.clean()):
                self.sample(self.tracked_n())
                if rng.random() < 0.4:
                    new("noise_update")
                    self.sample(self.tracked_n())
            else:
                if not m.selected or rng.random() < 0.4:
                    if rng.random() < 0.6 or "moments" not in m.exists:
                        new("select_mask", seed=int(rng.integers(0, 1000)), share=float(pick((0.1, 0.3, 0.5, 1.0))))
                    else:
                        self.one("select_noisy")
                new("sample_selected", n=self.tracked_n())
            w = rng.random()
            if w < 0.35:
                self.one("noise_estimate")
            elif w < 0.5:
                new("set_noise_estimator", e=pick(ESTIMATORS[:4]))
                self.one("noise_estimate")
            if rng.random() < 0.5:
                add(Op("observe", what=pick(("all", "post"))))
        elif u < 0.80:                                                      # what tracked mode refuses, tiles and the persistent-ray form
            self.tracking_on()
            if rng.random() < 0.5 and 1 in self.forms:
                self.set_config(kernel_form=1)
                self.sample(self.tracked_n())
                if rng.random() < 0.5:
                    self.set_config(kernel_form=0)
            else:
                add(Op("set_tiles", tiles=(int(pick((5, 7, 9, 13, 19))), int(pick((3, 7, 11))), int(rng.integers(0, 2)), 2)))
                for i in rng.permutation(4)[:3]:
                    if i == 0:
                        self.sample(self.tracked_n())
                    elif i == 1:
                        new("sample_selected", n=self.tracked_n())
                    elif i == 2:
                        new("set_noise_tracking", mode=1)
                    else:
                        self.reproject_scene()
                add(Op("set_tiles", tiles=(0, 0, 0, 1)))
            add(Op("observe", what="post"))
        elif u < 0.92:                                                      # both normal rules of the scene gather
            self.set_config(normal_space=1 - m.cfg.normal_space)
            if rng.random() < 0.8:
                self.history(1.0)
                self.reproject_scene(params=dict(pick(REPROJECT[3:])))
        else:                                                               # reproject_scene after each call that ends a history
            self.whole_frame(1.0)
            add(Op("refresh"))
            who = pick(("set_config", "set_scene", "set_shape_data", "set_env"))
            if who == "set_config":
                self.set_config(exposure=float(pick((0.7, 0.9, 1.1))))
            elif who == "set_scene":
                add(Op("set_scene", name=m.scene))
            elif who == "set_shape_data":
                v = int(rng.integers(0, 2))
                add(Op("set_shape_data", variant=v, n=625))
                m.weights = v
            else:
                add(Op("set_env", w=16, h=8, seed=int(rng.integers(0, 3)), f32=False, exposure=1.0, gamma=2.2))
                m.env = True
            self.reproject_scene()

def script(seed, n_ops=60, jit=0, scenes=None, forms=(0, 1)):
    """A reproducible call sequence: seed -> Script.  `scenes`: the scene pool (all of SCENES by default); `forms`: the kernel
    forms set_config may switch between."""
    g = _Grammar(seed, scenes, forms, SIZES)
    while len(g.ops) < n_ops:
        g.old_op()
    g.add(Op("post_process"))
    g.add(Op("observe", what="all"))
    return Script(seed, g.base, g.scene0, g.ops, jit)


THRESHOLDS = (0.0, 0.02, 0.08, 0.3)       # fixed: a script prints before it runs, so no quantile of the run's own noise
GUIDED = ({}, {"iterations": 0}, {"iterations": 0, "demodulate": 1}, {"iterations": 1, "sigma_color": 4.0},
          {"iterations": 2, "demodulate": 1, "variance_floor": 1e-5}, {"iterations": 3, "sigma_color": 2.0, "sigma_depth": 0.05})
ESTIMATORS = ((4, 1, 0), (8, 2, 0), (8, 3, 6), (64, 3, 0), (0, 3, 4), (3, 2, 16), None)
BAD_ESTIMATORS = ((2, 3, 0), (65, 3, 0), (8, 0, 0), (0, 4, 0), (8, 3, -1), (8, 3, 16777217))
REPROJECT = ({}, {"max_history": 2.0}, {"max_history": 5.0, "depth_tolerance": 0.02}, {"max_history": 1e6, "normal_cos": 0.9},
             {"max_history": 3.0, "depth_tolerance": 0.0, "normal_cos": -1.0})
POST_KINDS = ("noise_update", "noise_estimate", "denoise_guided", "set_noise_estimator", "select_mask", "select_noisy", "sample_selected",
              "reproject", "present")


def post_script(seed, n_ops=60, jit=0, scenes=None, forms=(0, 1)):
    """A call sequence over the whole stateful surface: about half of the draws are those of script() (its state changes land
    between the new calls), the other half are rtpbr_reproject, the noise calls, the estimator setting, the select calls,
    rtpbr_sample_selected, rtpbr_present and the "post" observation.  The expected code of every new operation comes from
    post_model.PostState, which follows the script as it is drawn.  Its random stream is its own: script() draws what it drew."""
    import post_model as pm
    g = _Grammar(seed, scenes, forms, POST_SIZES, pm.PostState)
    while len(g.ops) < n_ops:
        if g.rng.random() < 0.5:
            g.old_op()
        else:
            g.post_op()
    g.add(Op("post_process"))
    g.add(Op("observe", what="all"))
    g.add(Op("observe", what="post"))
    return Script(seed, g.base, g.scene0, g.ops, jit, post=True)


def jit_post_script():
    """the post script that runs through run-time compiled instances: jit = -1 over two scenes that no ahead-of-time specialisation
    serves, both kernel forms (sample_selected promises the same bits whatever jit says; reproject changes the camera, which a
    baked instance may carry)"""
    return post_script(2020, n_ops=50, jit=-1, scenes=("mixed7", "mixed8"), forms=(0, 1))


MOTION_KINDS = ("reproject_scene", "set_noise_tracking")


def motion_script(seed, n_ops=60, jit=0, scenes=None, forms=(0, 1)):
    """A call sequence over the two newest stateful calls: about a third of the draws are those of script(), a third those of
    post_script() and a third rtpbr_reproject_scene (rigid moves on top of the pose so far, with and without a camera, tables that
    are no rigid motion), rtpbr_set_noise_tracking and tracked rtpbr_sample / rtpbr_sample_selected calls with what they refuse.
    Expected codes come from post_model.MotionState; the script runs on post_model.MotionModel.  Its random stream is its own."""
    import post_model as pm
    g = _Grammar(seed, scenes, forms, POST_SIZES, pm.MotionState)
    while len(g.ops) < n_ops:
        u = g.rng.random()
        if u < 0.3:
            g.old_op()
        elif u < 0.6:
            g.post_op()
        else:
            g.motion_op()
    g.add(Op("post_process"))
    g.add(Op("observe", what="all"))
    g.add(Op("observe", what="post"))
    return Script(seed, g.base, g.scene0, g.ops, jit, post=True, motion=True)


def jit_motion_script():
    """the motion script through run-time compiled instances: jit = -1 over two scenes that no ahead-of-time specialisation serves,
    both kernel forms (a moved table is a scene the instance was not acquired for; a tracked launch keeps item-linear staging)"""
    return motion_script(3030, n_ops=40, jit=-1, scenes=("mixed7", "mixed8"), forms=(0, 1))


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


def _short(v):
    return v if isinstance(v, (str, tuple, int)) else f"a {v.dtype} buffer of shape {v.shape}"


def _first_diff(x, y):
    if isinstance(x, (tuple, int, str)) or isinstance(y, (tuple, int, str)):
        return None if type(x) is type(y) and x == y else f"{_short(x)} != {_short(y)}"
    if x.shape != y.shape or x.dtype != y.dtype:
        return f"{x.dtype} {x.shape} != {y.dtype} {y.shape}"
    if x.dtype.itemsize != 4:
        bad = x != y
        return None if not bad.any() else f"{int(bad.sum())} of {bad.size} bytes differ, first at {[tuple(int(v) for v in p) for p in np.argwhere(bad)[:4]]}"
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
    """rerun a script (or its first `upto` operations) on a fresh HIP renderer against a fresh oracle (a post_script: against a
    fresh post_model.PostModel)"""
    from raytracingpbr_amd import Renderer
    if s.post:
        import post_model as pm
        a, b = new_renderer(s, Renderer), pm.model(s, threads)
        try:
            return run_post(s, a, b, upto)
        finally:
            a.close()
            b.close()
    a, b = new_renderer(s, Renderer), new_renderer(s, OracleRenderer, threads=threads)
    try:
        return run(s, a, b, upto)
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------ the driver of post_script: HIP against tests/post_model.py
def _apply_post(op, r):
    """apply one operation to the HIP renderer; (code or None, {name: value} of what the call itself returned)"""
    a, k = op.args, op.kind
    try:
        if k == "noise_update":
            r.noise_update()
        elif k == "noise_estimate":
            st = r.noise_estimate(a["threshold"])
            return None, {"stats": (st.pixels_estimated, st.pixels_above, int(np.float32(st.max_noise).view(np.uint32)))}
        elif k == "denoise_guided":
            r.denoise_guided(**a["params"])
        elif k == "set_noise_estimator":
            if a["e"] is None:
                r.api.call("set_noise_estimator", r._ctx, None)
            else:
                r.set_noise_estimator(*a["e"])
        elif k == "select_mask":
            return None, {"n_selected": r.select_mask(mask(r.config.width, r.config.height, a["seed"], a["share"]))}
        elif k == "select_noisy":
            return None, {"n_selected": r.select_noisy(a["threshold"], a["dilate"])}
        elif k == "sample_selected":
            r.sample_selected(a["n"])
        elif k == "reproject":
            r.reproject(camera(a["name"], a["offset"], a["vfov"]), **a["params"])
        elif k == "present":
            r.present(a["source"], a["format"], a["dither"])
        elif k == "reproject_scene":
            table = posed(a["name"], a["pose"]) if a["bad"] is None else nonrigid(a["name"], a["pose"], a["bad"], a["k"], a["other"])
            r.reproject_scene(table, None if a["cam"] is None else camera(*a["cam"]), **a["params"])
        elif k == "set_noise_tracking":
            if a["mode"] in (0, 1):
                r.set_noise_tracking(bool(a["mode"]))
            else:
                r.api.call("set_noise_tracking", r._ctx, a["mode"])
        else:
            res = _apply(op, r)
            return (None if res is None else res[1]), {}
    except RtpbrError as e:
        return e.code, {}
    return None, {}


def _read_post(r, name):
    """what the HIP renderer holds under an expected value's name; a buffer that does not exist reads as post_model.MISSING"""
    import post_model as pm
    if name.startswith("counters"):
        c = r.counters()
        return (c.samples, c.deposits) if name == "counters.samples_deposits" else tuple(getattr(c, k) for k in COUNTERS)
    try:
        return getattr(r, name)
    except RtpbrError as e:
        if e.code != ESTATE:
            raise
        return pm.MISSING


def run_post(s, hip, model, upto=None):
    """Apply a post_script to the HIP renderer `hip` and the PostModel `model` in lock step: every call must return the code the
    script and the model expect, and everything the model expects of it — returned values and buffers — must be there bit for
    bit.  `hip` None: the model alone (the code against the script's).  Raises Mismatch with a replayable report; returns the
    list of (operation index, name, expected value)."""
    seen, last_ok_of = [], {}
    ops = s.ops if upto is None else s.ops[:upto]

    def fail(i, what, key=None):
        start = last_ok_of.get(key, -1)
        lines = [f"post call sequence seed {s.seed}, operation #{i}: {what}", s.header(),
                 f"operations since " + (f"{key} last matched" if key else "the start") + f" (#{start + 1}..#{i}):"]
        lines += [f"  [{j}] {s.ops[j]!r}" for j in range(start + 1, i + 1)]
        lines.append(f"replay: call_sequences.replay(call_sequences.{'motion' if s.motion else 'post'}_script({s.seed}, ...), upto={i + 1})")
        raise Mismatch("\n".join(lines))

    for i, op in enumerate(ops):
        want_code, want = model.apply(op)
        if want_code != op.expect:
            fail(i, f"{op.kind}: the model expects {want_code}, the script {op.expect}")
        got = {}
        if hip is not None:
            code, got = _apply_post(op, hip)
            if code != op.expect:
                fail(i, f"{op.kind} returned {code}, expected {op.expect}")
        for k, y in want.items():
            if hip is not None:
                d = _first_diff(got[k] if k in got else _read_post(hip, k), y)
                if d is not None:
                    fail(i, f"{k} differs from the model: {d}", k)
            seen.append((i, k, y))
            last_ok_of[k] = i
    return seen
