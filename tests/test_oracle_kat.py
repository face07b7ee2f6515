"""Known-answer tests that pin the CPU oracle (oracle/acmmp_oracle.c) before it
is trusted as the parity reference for the HIP path.

The reference ships no tests or fixtures for PatchMatch and cannot be built
here, so the oracle is pinned three ways:

1. analytic answers the reference's formulas must give: identity homography
   for coincident cameras, zero NCC cost for a correctly hypothesised plane in
   a rectified stereo rig with integer disparity, NCC invariance to affine
   intensity changes, the cost_max / kMinVar exits, the geometric cost of a
   consistent depth map and of a hole;
2. an independent float64 restatement, written here directly from the
   reference lines (ComputeHomography src/ACMMP.cu:262-322,
   ComputeCorrespondingPoint :324-331, ComputeBilateralWeight :353-358,
   ComputeBilateralNCC :360-432, Get3DPointonWorld_cu/ProjectonCamera_cu/
   ComputeGeomConsistencyCost :480-543), compared at a stated tolerance
   (the oracle computes in fp32 with the pins of DESIGN.md §2, so bit-equality
   with fp64 is not expected);
3. the aggregation logic of ComputeMultiViewInitialCostandSelectedViews
   (:434-471), restated here and checked bit-exactly on the oracle's own cost
   vectors.
"""
from __future__ import annotations

import math

import numpy as np
import pytest

import oracle
from acmmp_amd import default_params
from acmmp_amd.engine import make_camera
# the float64 restatements of the reference device code (test-local, independent
# of the C oracle) live in ref64.py, shared with the general-rig tests
from ref64 import ref_geom_cost, ref_homography, ref_ncc

# fp32 oracle vs fp64 restatement: NCC costs live in [0, 2]; the fp32 sums of
# 36 weighted samples of 0..255 intensities carry ~1e-6 relative error, which
# the 1 - cov/sqrt(var*var) step amplifies by 1/NCC-denominator.
NCC_TOL = 2e-4
H_TOL = 1e-5


def _cam(f=100.0, cx=32.0, cy=24.0, R=None, t=(0, 0, 0), w=64, h=48, dmin=1.0, dmax=100.0):
    K = np.array([[f, 0, cx], [0, f, cy], [0, 0, 1]], np.float64)
    R = np.eye(3) if R is None else np.asarray(R, np.float64)
    return make_camera(K, R, np.asarray(t, np.float64), w, h, dmin, dmax)


def _texture(h, w, seed):
    rng = np.random.default_rng(seed)
    img = rng.uniform(0, 255, (h, w))
    # mild smoothing keeps bilinear interpolation meaningful
    k = np.array([1, 2, 1], np.float64) / 4
    img = np.apply_along_axis(lambda r: np.convolve(r, k, mode="same"), 1, img)
    img = np.apply_along_axis(lambda c: np.convolve(c, k, mode="same"), 0, img)
    return np.round(img).astype(np.float32)


def _rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = math.cos(ax), math.sin(ax), math.cos(ay), math.sin(ay), math.cos(az), math.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


# ---------------------------------------------------------------------------
# 1. analytic answers


def test_homography_identity_for_coincident_cameras():
    c = _cam()
    H = oracle.homography(c, c, np.array([0.1, -0.2, -0.97, 30.0], np.float32))
    np.testing.assert_allclose(H, np.eye(3), atol=1e-6)


@pytest.mark.parametrize("Z0", [20.0, 25.0, 50.0])
def test_homography_rectified_stereo_is_a_shift(Z0):
    """Src camera centre at (b,0,0): a fronto-parallel plane z=Z0 induces
    x_src = x - f*b/Z0 (plane (0,0,-1,Z0): d = -n.X, src/ACMMP.cu:144-149)."""
    f, b = 100.0, 1.0
    rc, sc = _cam(f=f), _cam(f=f, t=(-b, 0, 0))
    H = oracle.homography(rc, sc, np.array([0, 0, -1, Z0], np.float32))
    expect = np.array([[1, 0, -f * b / Z0], [0, 1, 0], [0, 0, 1]])
    np.testing.assert_allclose(H, expect, atol=1e-5)


def test_homography_matches_fp64_restatement():
    rng = np.random.default_rng(7)
    for _ in range(20):
        R1 = _rot(*rng.uniform(-0.3, 0.3, 3))
        R2 = _rot(*rng.uniform(-0.3, 0.3, 3))
        rc = _cam(f=rng.uniform(80, 3000), cx=rng.uniform(20, 40), cy=rng.uniform(15, 30), R=R1,
                  t=rng.uniform(-5, 5, 3))
        sc = _cam(f=rng.uniform(80, 3000), cx=rng.uniform(20, 40), cy=rng.uniform(15, 30), R=R2,
                  t=rng.uniform(-5, 5, 3))
        n = rng.normal(size=3)
        n[2] = -abs(n[2]) - 0.5
        n /= np.linalg.norm(n)
        plane = np.array([*n, rng.uniform(10, 100)], np.float32)
        H = oracle.homography(rc, sc, plane).astype(np.float64)
        Href = ref_homography(rc, sc, plane.astype(np.float64))
        scale = np.abs(Href).max()
        np.testing.assert_allclose(H, Href, atol=H_TOL * scale)


def test_ncc_identical_views_is_zero():
    prm = default_params()
    img = _texture(48, 64, 1)
    c = _cam()
    for (x, y) in [(32, 24), (10, 10), (50, 40)]:
        cost = oracle.ncc(prm, c, c, img, img, x, y, np.array([0, 0, -1, 30], np.float32))
        assert cost < 1e-5, cost


@pytest.mark.parametrize("a,b,expect", [(2.0, 10.0, 0.0), (0.5, 3.0, 0.0), (-1.0, 255.0, 2.0)])
def test_ncc_affine_intensity_invariance(a, b, expect):
    """NCC is invariant to src = a*ref + b for a > 0 (cost 0); a < 0 gives
    perfect anti-correlation, 1 - (-1) = 2 = cost_max (src/ACMMP.cu:427-428)."""
    prm = default_params()
    img = _texture(48, 64, 2)
    c = _cam()
    cost = oracle.ncc(prm, c, c, img, (a * img + b).astype(np.float32), 30, 20,
                      np.array([0, 0, -1, 30], np.float32))
    assert abs(cost - expect) < 1e-4, cost


def test_ncc_textureless_returns_cost_max():
    """var < kMinVar -> cost_max (src/ACMMP.cu:423-425), on either side.

    Flat value 0 (and a small one): var = E[s^2] - E[s]^2 is formed in fp32
    after scaling by 1/sum(w), so for a mid-grey flat patch (e.g. 77) it can
    come out as a few ulps of 77^2 ~ 5e-4 > 1e-5 and miss the exit — a literal
    fp32 property of the reference expression, not something to 'fix'."""
    prm = default_params()
    tex = _texture(48, 64, 3)
    c = _cam()
    pl = np.array([0, 0, -1, 30], np.float32)
    for v in (0.0, 0.25):
        flat = np.full((48, 64), v, np.float32)
        assert oracle.ncc(prm, c, c, flat, tex, 30, 20, pl) == 2.0
        assert oracle.ncc(prm, c, c, tex, flat, 30, 20, pl) == 2.0


def test_ncc_centre_outside_source_returns_cost_max():
    """The centre maps outside the source image -> 2 (src/ACMMP.cu:368-370)."""
    prm = default_params()
    img = _texture(48, 64, 4)
    rc, sc = _cam(), _cam(t=(-1.0, 0, 0))
    # disparity 100/2 = 50 px: pixel x=20 lands at x=-30
    assert oracle.ncc(prm, rc, sc, img, img, 20, 24, np.array([0, 0, -1, 2.0], np.float32)) == 2.0


@pytest.mark.parametrize("disp", [2, 4, 5])
def test_ncc_rectified_stereo_true_depth_scores_zero(disp):
    """Integer disparity: src[:, x] = ref[:, x + disp]. The true plane maps
    every sample onto an exact texel, so the cost is 0; a wrong depth is not."""
    prm = default_params()
    f, b = 100.0, 1.0
    ref = _texture(48, 96, 5)
    src = np.empty_like(ref)
    src[:, : 96 - disp] = ref[:, disp:]
    src[:, 96 - disp:] = ref[:, -1:]
    rc, sc = _cam(f=f, cx=48, w=96), _cam(f=f, cx=48, t=(-b, 0, 0), w=96)
    Z0 = f * b / disp
    good = oracle.ncc(prm, rc, sc, ref, src, 48, 24, np.array([0, 0, -1, Z0], np.float32))
    bad = oracle.ncc(prm, rc, sc, ref, src, 48, 24, np.array([0, 0, -1, f * b / (disp + 1.5)], np.float32))
    assert good < 1e-4, good
    assert bad > 0.05, bad


# ---------------------------------------------------------------------------
# 2. independent fp64 restatement


def test_ncc_matches_fp64_restatement():
    prm = default_params()
    rng = np.random.default_rng(11)
    W, H = 96, 72
    ref = _texture(H, W, 20)
    checked = 0
    for k in range(60):
        R2 = _rot(*rng.uniform(-0.05, 0.05, 3))
        rc = _cam(f=120.0, cx=48, cy=36, w=W, h=H)
        sc = _cam(f=rng.uniform(110, 130), cx=48, cy=36, R=R2, t=rng.uniform(-1, 1, 3) * [1, 1, 0.2], w=W, h=H)
        src = _texture(H, W, 100 + k) if k % 3 == 0 else ref  # unrelated or same texture
        n = rng.normal(size=3) * [0.3, 0.3, 1]
        n[2] = -abs(n[2]) - 0.3
        n /= np.linalg.norm(n)
        plane = np.array([*n, rng.uniform(15, 60)], np.float32)
        px, py = int(rng.integers(0, W)), int(rng.integers(0, H))  # borders exercise clamp-to-edge
        got = oracle.ncc(prm, rc, sc, ref, src, px, py, plane)
        want = ref_ncc(prm, rc, sc, ref, src, px, py, plane.astype(np.float64))
        assert abs(got - want) <= NCC_TOL, (k, px, py, got, want)
        checked += want < 2.0
    assert checked >= 20  # most cases are real NCC values, not early exits


def test_geom_cost_matches_fp64_restatement_and_kats():
    """Consistent depth maps give ~0 px; holes give max_cost 3; a biased src
    depth gives the fp64 reprojection error (src/ACMMP.cu:518-543)."""
    prm = default_params()
    W, H = 64, 48
    f, b, Z0 = 100.0, 1.0, 25.0
    rc, sc = _cam(f=f, w=W, h=H), _cam(f=f, t=(-b, 0, 0), w=W, h=H)
    img = _texture(H, W, 30)
    planes = np.zeros((H, W, 4), np.float32)
    planes[...] = [0, 0, -1, Z0]
    cases = {
        "consistent": np.full((H, W), Z0, np.float32),
        "hole": np.zeros((H, W), np.float32),
        "biased": np.full((H, W), Z0 * 1.04, np.float32),
    }
    for name, sdep in cases.items():
        depths = [np.full((H, W), Z0, np.float32), sdep]
        out = oracle.eval_geom_costs(prm, [rc, sc], [img, img], depths, planes)[..., 0]
        for (x, y) in [(10, 5), (32, 24), (63, 47), (0, 0)]:
            want = ref_geom_cost(rc, sc, sdep, np.array([0, 0, -1, Z0], np.float64), x, y)
            assert abs(out[y, x] - want) <= 1e-3 * max(1.0, want), (name, x, y, out[y, x], want)
        if name == "consistent":
            assert np.abs(out).max() < 1e-3
        if name == "hole":
            assert np.all(out == 3.0)


# ---------------------------------------------------------------------------
# 3. aggregation of ComputeMultiViewInitialCostandSelectedViews (bit-exact)


def _init_cost_restated(vec, top_k):
    """src/ACMMP.cu:434-471 on one pixel's cost vector (fp32 arithmetic)."""
    vec = [np.float32(c) for c in vec]
    valid = sum(1 for c in vec if c < 2.0)
    srt = sorted(vec)  # sort_small (:24-33) is a stable insertion sort; values only
    k = min(valid, top_k)
    if k <= 0:
        return np.float32(2.0), 0
    cost = np.float32(0.0)
    for i in range(k):
        cost = np.float32(cost + srt[i])
    thr = srt[k - 1]
    mask = 0
    for i, c in enumerate(vec):
        if c <= thr:
            mask |= 1 << i
    return np.float32(cost / np.float32(k)), mask


def test_initial_cost_and_selected_views_aggregation():
    from acmmp_amd import scene

    sc = scene.make_scene(num_views=6, width=80, height=60)
    cams, imgs = sc.problem(0, 5)
    prm = default_params()
    rng = np.random.default_rng(3)
    H, W = 60, 80
    n = rng.normal(size=(H, W, 3)) * [0.2, 0.2, 1]
    n[..., 2] = -np.abs(n[..., 2]) - 0.3
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    planes = np.concatenate([n, rng.uniform(400, 700, (H, W, 1))], -1).astype(np.float32)
    vec, init, views = oracle.eval_costs(prm, cams, imgs, planes)
    n_mixed = 0
    for y in range(0, H, 3):
        for x in range(0, W, 3):
            c, m = _init_cost_restated(vec[y, x], prm.top_k)
            assert init[y, x].view(np.uint32) == c.view(np.uint32), (x, y)
            assert views[y, x] == m, (x, y, hex(views[y, x]), hex(m))
            n_mixed += 0 < (vec[y, x] < 2).sum() < 5
    assert n_mixed > 10  # partial-validity pixels exercise top_k = min(valid, 4)


def test_p3_forms_selectable_and_differ_only_where_documented():
    """Pin P3 is inferred (parity unpinned): the oracle keeps
    r01's unfused form selectable. On a textured patch both forms give the
    same NCC to rounding; on a flat mid-grey patch they part: the fused
    moments leave independent residuals (here cost 0), the unfused ones
    identical residuals below kMinVar (cost_max)."""
    prm = default_params()
    c = _cam()
    pl = np.array([0, 0, -1, 30], np.float32)
    tex = _texture(48, 64, 3)
    src = (tex * 1.1 + 3).astype(np.float32)
    fused = oracle.ncc(prm, c, c, tex, src, 30, 20, pl)
    flat = np.full((48, 64), 77.0, np.float32)
    flat_fused = oracle.ncc(prm, c, c, flat, flat, 30, 20, pl)
    with oracle.p3_unfused():
        unfused = oracle.ncc(prm, c, c, tex, src, 30, 20, pl)
        flat_unfused = oracle.ncc(prm, c, c, flat, flat, 30, 20, pl)
    assert abs(fused - unfused) < 1e-5
    assert flat_fused == 0.0 and flat_unfused == 2.0
    # the default is restored: the product's form
    assert oracle.ncc(prm, c, c, flat, flat, 30, 20, pl) == 0.0
