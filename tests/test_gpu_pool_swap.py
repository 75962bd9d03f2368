"""The pool kernels' swap (rt_trace.hpp pool_swap) exchanges a lane's record with its slot IN PLACE, word by word, in
the lane's own registers: one exec-masked group of LDS exchanges for "finished lane + READY slot" (a swap), "finished lane +
free slot" (the words that come back are dead) and "idle lane + READY slot" (the words written are dead).  Nothing of the
schedule or the arithmetic may show in the results: every case below compares the image_buffer bits and the samples /
raycasts / march_steps / hits counters with the CPU oracle.  One oracle render per frame, shared by its option sets.
"""
import functools
import itertools

import numpy as np
import pytest

from cases import Case
from oracle_backend import OracleRenderer
from raytracingpbr_amd import SHAPE, Config, Renderer, bunny, cornell_box, src_scene
from raytracingpbr_amd.dataclass import Material, SDFObject, Transform, vec3
from raytracingpbr_amd.ibl import synthetic_env
from raytracingpbr_amd.scene import Scene

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def work(r):
    c = r.counters()
    return (c.samples, c.raycasts, c.march_steps, c.hits)


def render(case, cls, opts=()):
    r = cls(case.scene, case.cfg)
    for k, v in opts:
        r.set_option(k, v)
    case.setup(r)
    for _ in range(case.rounds):
        r.sample(case.n)
    out = bits(r.image_buffer).copy(), work(r)
    if hasattr(r, "close"):
        r.close()
    return out


@functools.lru_cache(maxsize=None)
def frame(name):
    """(case, oracle image bits, oracle counters) of a named frame; rendered by the oracle once and never modified"""
    env = synthetic_env(64, 32, seed=0)
    if name.startswith("cornell"):                      # Cornell v3, 24x20, 8 bounces; 5 spp: K is not a power of two
        spp = int(name[len("cornell"):])
        case = Case(name, cornell_box("v3", aspect=24 / 20), Config.cornell_v3(24, 20, 3, 8), spp)
    elif name == "tiny":                                # 64 items: the pool never fills, idle lanes take without parking
        case = Case(name, cornell_box("v3"), Config.cornell_v3(8, 8, 4, 8), 1)
    elif name == "far_box":                             # nearly every raycast misses: finished lanes park into free slots
        box = SDFObject(SHAPE.BOX, Transform((0.3, -0.2, -1.0), (0, 30, 0), (0.05, 0.05, 0.05)),
                        Material((0.9, 0.9, 0.9), vec3(1), 1, 0, 0, 1.53))
        sc = cornell_box("v3", aspect=24 / 20)
        case = Case(name, Scene([box], True, sc.camera, "far_box"), Config.cornell_v3(24, 20, 5, 8), 8)
    elif name == "src":                                 # the src/ form: the other caller of pool_swap (15-word records)
        case = Case(name, src_scene(aspect=1.0), Config.src(32, 32, 7, steps_per_launch=1), 8, env=env, env_exposure=1.4, env_gamma=2.2)
    elif name == "bunny":                               # the c3 kind: the neural-SDF pool
        case = Case(name, bunny(aspect=1.0), Config.bunny_glass(16, 16, 9, 16, frame=0).copy(max_raymarch=512), 2,
                    env=env, env_exposure=1.8, env_gamma=2.2)
    else:
        raise KeyError(name)
    img, ctr = render(case, OracleRenderer)
    img.setflags(write=False)
    return case, img, ctr


def check(name, opts):
    case, want, ctr = frame(name)
    got, c = render(case, Renderer, opts)
    assert c == ctr, (name, opts, c, ctr)
    assert np.array_equal(got, want), (name, opts, int((got != want).any(axis=2).sum()), "pixels differ")


SWEEP = [(("swap_lanes", s), ("ready_low", r), ("refill_lanes", f)) for s, r, f in itertools.product((1, 8, 64), (0, 4), (1, 24))]
INSTANCES = {"aot": (("jit", 0),), "baked": (("jit", 2), ("jit_bake", 1))}


@pytest.mark.parametrize("inst", list(INSTANCES))
@pytest.mark.parametrize("spp", (5, 8))
def test_cornell_swap_schedules_match_the_oracle(spp, inst):
    for opts in SWEEP:
        check("cornell%d" % spp, INSTANCES[inst] + opts)
        # a frame this small is spread over so many waves that each holds about 64 paths; with claims of 480 items a few waves
        # do all the work, their pools are full and finished lanes meet READY slots (the swap proper) all the time
        check("cornell%d" % spp, INSTANCES[inst] + opts + (("chunk", 480),))


@pytest.mark.parametrize("inst", list(INSTANCES))
def test_pool_that_never_fills(inst):
    """8x8 at 1 spp = 64 items: one wave's refill makes them all READY, idle lanes take them, no lane ever swaps."""
    for opts in ((), (("swap_lanes", 1),), (("swap_lanes", 64), ("refill_lanes", 24))):
        check("tiny", INSTANCES[inst] + opts)


@pytest.mark.parametrize("inst", list(INSTANCES))
def test_finished_lanes_park_into_free_slots(inst):
    """One small box far away: the samples end at their first miss, so READY rays run out and finished lanes find free slots only."""
    _, _, ctr = frame("far_box")
    assert ctr[3] * 10 < ctr[1], ctr          # hits << raycasts: the frame is what the case is about
    for opts in ((), (("swap_lanes", 1), ("ready_low", 0)), (("swap_lanes", 8), ("ready_low", 4), ("refill_lanes", 24)), (("swap_lanes", 64),)):
        check("far_box", INSTANCES[inst] + opts)


@pytest.mark.parametrize("swap", (1, 12))
def test_src_form_pool(swap):
    check("src", (("swap_lanes", swap),))
    check("src", (("swap_lanes", swap), ("jit", 2), ("jit_bake", 1)))


def test_neural_sdf_pool():
    check("bunny", ())
    check("bunny", (("swap_lanes", 3), ("shade_lanes", 5)))
