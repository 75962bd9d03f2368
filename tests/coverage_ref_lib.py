"""Test helper: the CPU reference of rtpbr_render_coverage / rtpbr_denoise_coverage.  The coverage is, by the definition in
include/rtpbr.h, the object plane of fr_features (tests/post_ref) at the g-fold size binned per pixel: numpy does the binning and
the candidate rule here.  The filter and the resolve are tests/coverage_ref/coverage_ref.c, built on demand by ref_build."""
import os

import numpy as np

import feature_ref_lib as fl
from raytracingpbr_amd.dataclass import CoverageParams, DenoiseParams
from ref_build import F, I, ORACLE_DEPS, P, ROOT, Library, cfg_ptr, feats_of, fields, ptr, stats_of

COVERAGE_REF = Library("coverage_ref", {"cr_denoise_coverage": [P] * 7 + [I, I, F, F, F, F, I, I, P, P]},
                       deps=ORACLE_DEPS + [os.path.join(ROOT, "tests", "post_ref", s + ".h") for s in ("common", "filter")])
build, lib = COVERAGE_REF.build, COVERAGE_REF.lib


def candidates(obj):
    """(W,H) bool: some pixel of the 3x3 neighbourhood inside the frame holds another object index"""
    W, H = obj.shape
    pad = np.pad(obj, 1, mode="edge")      # (a border pixel repeats itself: the frame's border makes no candidate)
    cand = np.zeros((W, H), bool)
    for dx in range(3):
        for dy in range(3):
            cand |= pad[dx:dx + W, dy:dy + H] != obj
    return cand


def bin_coverage(obj, sub_obj, grid):
    """(W,H,4) int32 (n_own, second_object, n_second, n_sub) from the frame's object plane (W,H) and the g-fold frame's (gW,gH)"""
    W, H = obj.shape
    S = grid * grid
    sub = sub_obj.reshape(W, grid, H, grid).transpose(0, 2, 1, 3).reshape(W, H, S)
    cov = np.empty((W, H, 4), np.int32)
    cov[..., 0] = (sub == obj[..., None]).sum(-1)
    cov[..., 1], cov[..., 2], cov[..., 3] = -2, 0, S
    for v in range(-1, int(sub.max()) + 1):      # ascending: a tie stays with the smaller index
        cnt = np.where(obj == v, 0, (sub == v).sum(-1))
        better = cnt > cov[..., 2]
        cov[..., 1] = np.where(better, v, cov[..., 1])
        cov[..., 2] = np.where(better, cnt, cov[..., 2])
    cov[~candidates(obj)] = (S, -2, 0, S)
    return cov


def coverage(scene, cfg, grid=None, camera=None, bunny_weights=None, feats=None):
    """(W,H,4) int32 — what rtpbr_render_coverage writes (grid None = the library default)"""
    g = CoverageParams.DEFAULTS["grid"] if grid is None else grid
    obj = (feats if feats is not None else fl.features(scene, cfg, camera, bunny_weights))["object"]
    big = fl.features(scene, cfg.copy(width=g * cfg.width, height=g * cfg.height), camera, bunny_weights)["object"]
    return bin_coverage(obj, big, g)


def denoise_coverage(cfg, image_buffer, feats, cov, power=None, resolve=None, iterations=None, demodulate=None, sigma_color=None,
                     sigma_normal=None, sigma_depth=None, sigma_albedo=None):
    """((W,H,3), (resolved, candidates, largest 1 - a)) — what rtpbr_denoise_coverage writes and returns"""
    p = DenoiseParams.pack(False, iterations, demodulate, sigma_color, sigma_normal, sigma_depth, sigma_albedo)
    c = CoverageParams.pack(False, power=power, resolve=resolve)
    ib = np.ascontiguousarray(image_buffer, dtype=np.float32)
    cov = np.ascontiguousarray(cov, dtype=np.int32)
    f = feats_of(feats)
    out = np.empty((cfg.width, cfg.height, 3), np.float32)
    st = np.zeros(3, np.uint32)
    rc = lib().cr_denoise_coverage(cfg_ptr(cfg), ptr(ib), *map(ptr, f), ptr(cov), *fields(p), c.power, c.resolve, ptr(out), ptr(st))
    assert rc == 0, rc
    st[1] = int(candidates(f[3]).sum())
    return out, stats_of(st)


def error_sets(obj, cov):
    """the three pixel sets of the quality scores, (W,H) bool each: interior (the 5x5 neighbourhood inside the frame holds one
    object), coverage below 1 (n_own < n_sub), the whole frame"""
    W, H = obj.shape
    pad = np.pad(obj, 2, mode="edge")
    interior = np.ones((W, H), bool)
    for dx in range(5):
        for dy in range(5):
            interior &= pad[dx:dx + W, dy:dy + H] == obj
    return {"interior": interior, "edge": cov[..., 0] < cov[..., 3], "frame": np.ones((W, H), bool)}
