"""A deterministic rig of general cameras for the kernel tests: fx != fy, an
off-centre principal point, a real rotation, source views of other sizes
(narrower, wider, portrait) with intrinsics and poses of their own, and an
optional skew term — every quantity the per-view paths of the kernels handle,
set to something other than its trivial value. Shared by
test_general_rig_cpu.py (oracle vs float64) and test_gpu_general_rig.py (the
same inputs through the HIP kernels).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from acmmp_amd import default_params, make_camera
from test_oracle_kat import _rot, _texture

REF_SIZE = (96, 72)                         # width, height
REF_F = (130.0, 112.0)
REF_C = (40.3, 43.7)
REF_ROT = (0.2, -0.3, 0.5)
REF_T = (1.0, -2.0, 0.5)
DEPTH_RANGE = (15.0, 60.0)
SRC_SIZES = [(80, 60), (112, 84), (64, 90)]  # narrower, wider, portrait
SKEW = 1.5
TEXEL_BITS = {"u8": 8, "h16": 16, "f32": 32}


def _K(fx, fy, cx, cy, skew):
    return np.array([[fx, SKEW if skew else 0.0, cx], [0, fy, cy], [0, 0, 1]], np.float64)


def ref_camera(width=REF_SIZE[0], height=REF_SIZE[1], skew=False, depth_range=DEPTH_RANGE):
    """The rig's reference camera; at another size the principal point keeps
    its relative place and the focal lengths their values."""
    cx = REF_C[0] * width / REF_SIZE[0]
    cy = REF_C[1] * height / REF_SIZE[1]
    return make_camera(_K(REF_F[0], REF_F[1], cx, cy, skew), _rot(*REF_ROT), np.array(REF_T), width, height,
                       *depth_range)


def source_camera(i, rng, skew=False, depth_range=DEPTH_RANGE):
    """Source view i: size SRC_SIZES[i % 3], focal lengths within 10 % of the
    reference's scaled by w / 96, a principal point of its own, a rotation of
    up to 0.05 rad per axis on top of the reference's, the centre moved by up
    to (1, 1, 0.2) in the reference camera frame."""
    w, h = SRC_SIZES[i % len(SRC_SIZES)]
    s = w / REF_SIZE[0]
    fx = REF_F[0] * s * rng.uniform(0.9, 1.1)
    fy = REF_F[1] * s * rng.uniform(0.9, 1.1)
    cx = w * rng.uniform(0.42, 0.58)
    cy = h * rng.uniform(0.42, 0.58)
    Rr = _rot(*REF_ROT)
    Rs = _rot(*rng.uniform(-0.05, 0.05, 3)) @ Rr
    Cr = -Rr.T @ np.array(REF_T)
    Cs = Cr + Rr.T @ (rng.uniform(-1, 1, 3) * [1.0, 1.0, 0.2])
    return make_camera(_K(fx, fy, cx, cy, skew), Rs, -Rs @ Cs, w, h, *depth_range)


def _smooth(h, w, seed):
    """_texture before its rounding: arbitrary floats."""
    rng = np.random.default_rng(seed)
    img = rng.uniform(0, 255, (h, w))
    k = np.array([1, 2, 1], np.float64) / 4
    img = np.apply_along_axis(lambda r: np.convolve(r, k, mode="same"), 1, img)
    img = np.apply_along_axis(lambda c: np.convolve(c, k, mode="same"), 0, img)
    return img


def image(h, w, seed, texels="u8"):
    """A smoothed random texture in the form the named texel storage holds
    exactly and the more compact ones do not: integers (u8 quads), the 0.5
    grid (f16 difference quads), arbitrary floats (fp32 row pairs)."""
    if texels == "u8":
        return _texture(h, w, seed)
    raw = _smooth(h, w, seed)
    if texels == "h16":
        return (np.round(raw * 2) / 2).astype(np.float32)
    return raw.astype(np.float32)


def random_planes(cam, seed, lo=20.0, hi=50.0):
    """Camera-frame planes (n, d), n facing the camera, the depth at the
    pixel in [lo, hi] (as _random_planes of test_gpu_parity.py)."""
    rng = np.random.default_rng(seed)
    H, W = cam.height, cam.width
    K = np.array(cam.K[:], np.float64).reshape(3, 3)
    n = rng.normal(size=(H, W, 3))
    n[..., 2] = -np.abs(n[..., 2]) - 0.5
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    depth = rng.uniform(lo, hi, size=(H, W))
    ys, xs = np.mgrid[0:H, 0:W]
    X = np.stack([depth * (xs - K[0, 2]) / K[0, 0], depth * (ys - K[1, 2]) / K[1, 1], depth], -1)
    d = -(n * X).sum(-1)
    return np.concatenate([n, d[..., None]], -1).astype(np.float32)


def random_depth_map(h, w, rng, zeros=0.10):
    d = rng.uniform(*DEPTH_RANGE, size=(h, w)).astype(np.float32)
    d[rng.random((h, w)) < zeros] = 0.0
    return d


def world_state(cam, seed, lo=DEPTH_RANGE[0], hi=DEPTH_RANGE[1], quantum=None):
    """(world normal, depth) state planes for the geometric-branch init: the
    camera-frame normal has n_z <= -0.3 before normalising (1 / |n . ray| stays
    below 3.5), the depth is uniform in [lo, hi] (rounded to `quantum`)."""
    rng = np.random.default_rng(seed)
    H, W = cam.height, cam.width
    R = np.array(cam.R[:], np.float64).reshape(3, 3)
    n = rng.normal(size=(H, W, 3)) * [0.3, 0.3, 1.0]
    n[..., 2] = -np.abs(n[..., 2]) - 0.3
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    depth = rng.uniform(lo, hi, size=(H, W))
    if quantum:
        depth = np.round(depth / quantum) * quantum
    return np.concatenate([n @ R, depth[..., None]], -1).astype(np.float32)  # world = R^T n_cam


def rig_params(cam, nviews, **kw):
    """default_params with the depth and disparity range InputInitialization
    would derive (src/ACMMP.cpp:600-606), for use without an engine and with
    set_images(keep_depth_range=True)."""
    p = default_params()
    p.num_images = nviews
    p.depth_min = cam.depth_min
    p.depth_max = cam.depth_max
    p.disparity_min = cam.K[0] * p.baseline / p.depth_max
    p.disparity_max = cam.K[0] * p.baseline / p.depth_min
    for k, v in kw.items():
        setattr(p, k, v)
    return p


@dataclass
class Rig:
    cams: list
    imgs: list
    depths: list  # one per view, at the view's own size


def make_rig(nsrc=3, texels="u8", skew=False, seed=0):
    rng = np.random.default_rng(1000 + seed)
    cams = [ref_camera(skew=skew)] + [source_camera(i, rng, skew=skew) for i in range(nsrc)]
    imgs = [image(c.height, c.width, 50 + seed * 100 + i, texels) for i, c in enumerate(cams)]
    depths = [random_depth_map(c.height, c.width, rng) for c in cams]
    return Rig(cams, imgs, depths)
