"""The sweep's refinement drops a hypothesis once its partial cost can no
longer beat the pixel's current cost (refine_costs_compact: per-lane alive
mask, only live (lane, t) items packed into the wave's passes). The result
must stay the reference's (src/ACMMP.cu:743-783): every case is end-to-end
RunPatchMatch, bit-exact against the oracle, at the smallest shape that
reaches its path:
- a converged state, where most hypotheses die early (photometric, then
  geometric from its state);
- partial waves and an image smaller than a block (few lanes build the list);
- the NS 20 and NS 32 buckets (ViewCounts::hi in use);
- one source view (nothing to prune, the view loop runs once);
- a planar pass whose mask is a checkerboard of 3 x 3 cells: prior lanes are
  never pruned, their neighbours in the same wave are;
- NaN, infinite and extreme geometric costs; constant images, where every
  cost is the same and a partial sum ties the bound exactly (level 77: all
  costs 0, so 0 >= 0 kills every hypothesis at its first view) or is NaN
  (level 100), alone and next to textured columns in the same waves;
- the hierarchy gate with pre-costs.
"""
import numpy as np
import pytest

import oracle
from acmmp_amd import ACMMP, default_params, make_camera, scene
from parity_util import assert_bit_exact

pytestmark = pytest.mark.gpu


def _params(iters, **kw):
    p = default_params()
    p.max_iterations = iters
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _gpu(p, cams, imgs, depths=None, state=None):
    with ACMMP(0) as eng:
        eng.set_params(p)
        eng.set_images(cams, imgs)
        if depths is not None:
            eng.set_depth_maps(depths)
        if state is not None:
            eng.set_plane_hypotheses(*state)
        prm = eng.params
        eng.RunPatchMatch()
        return prm, (eng.plane_hypotheses(), eng.costs(), eng.selected_views())


def _same(got, ref, what):
    assert_bit_exact(got[0], ref["planes"], f"planes ({what})")
    assert_bit_exact(got[1], ref["costs"], f"costs ({what})")
    assert_bit_exact(got[2], ref["selected_views"], f"selected views ({what})")


def _photo_then_geom(sc, nsrc, it_photo, it_geom, what, depths=None):
    cams, imgs = sc.problem(0, nsrc)
    if depths is None:
        depths = [sc.views[i].depth for i in [0] + sc.pairs[0][:nsrc]]
    prm, got = _gpu(_params(it_photo), cams, imgs)
    ref = oracle.run_patchmatch(prm, cams, imgs)
    _same(got, ref, what + ", photometric")
    state = (ref["planes"], ref["costs"])
    prm, got = _gpu(_params(it_geom, geom_consistency=1), cams, imgs, depths=depths, state=state)
    refg = oracle.run_patchmatch(prm, cams, imgs, depths=depths, planes=state[0], costs=state[1])
    _same(got, refg, what + ", geometric")
    return ref, refg


def test_converged_state():
    sc = scene.make_scene(num_views=6, width=64, height=48, arc_deg=4.0)
    ref, _ = _photo_then_geom(sc, 5, 6, 3, "converged")
    # the state did converge: low costs are what lets partial sums pass them
    assert np.nanmedian(ref["costs"]) < 0.3


@pytest.mark.parametrize("nsrc,W,H", [(9, 37, 29), (3, 13, 11)])
def test_partial_waves_and_sub_block_image(nsrc, W, H):
    sc = scene.make_scene(num_views=nsrc + 1, width=W, height=H, arc_deg=4.0)
    cams, imgs = sc.problem(0, nsrc)
    prm, got = _gpu(_params(3), cams, imgs)
    _same(got, oracle.run_patchmatch(prm, cams, imgs), f"{W}x{H} nsrc={nsrc}")


@pytest.mark.parametrize("nsrc,W,H", [(20, 45, 33), (25, 40, 29)])
def test_high_view_count_buckets(nsrc, W, H):
    sc = scene.make_scene(num_views=nsrc + 1, width=W, height=H, arc_deg=2.0)
    ref, refg = _photo_then_geom(sc, nsrc, 3, 3, f"nsrc={nsrc}")
    # views of the second count word (j >= 16) are sampled
    assert (ref["selected_views"] >> 16).any() and (refg["selected_views"] >> 16).any()


def test_one_source():
    sc = scene.make_scene(num_views=2, width=61, height=45, arc_deg=4.0)
    cams, imgs = sc.problem(0, 1)
    prm, got = _gpu(_params(3), cams, imgs)
    _same(got, oracle.run_patchmatch(prm, cams, imgs), "one source")


def _cam_planes_from_truth(view, cam):
    """Camera-frame plane hypotheses (n, d) from the analytic ground truth."""
    H, W = view.depth.shape
    K = np.array(cam.K).reshape(3, 3)
    R = np.array(cam.R).reshape(3, 3)
    n = view.normal @ R.T
    n[n[..., 2] > 0] *= -1
    ys, xs = np.mgrid[0:H, 0:W]
    z = np.where(view.depth > 0, view.depth, 600.0)
    X = np.stack([z * (xs - K[0, 2]) / K[0, 0], z * (ys - K[1, 2]) / K[1, 1], z], -1)
    return np.concatenate([n, -(n * X).sum(-1)[..., None]], -1).astype(np.float32)


def test_planar_prior_checkerboard_mask():
    """Second run with a planar prior on every other 3 x 3 cell: nearly every
    wave mixes prior lanes (never pruned) and plain lanes (pruned)."""
    W, H = 48, 36
    sc = scene.make_scene(num_views=5, width=W, height=H, arc_deg=4.0)
    cams, imgs = sc.problem(1, 4)
    planes_gt = _cam_planes_from_truth(sc.views[1], cams[0])
    cy, cx = np.arange(H)[:, None] // 3, np.arange(W)[None, :] // 3
    lab = cy * (W // 3) + cx
    mask = np.where((cy + cx) % 2 == 0, lab + 1, 0).astype(np.uint32)
    plane_params = np.zeros((int(lab.max()) + 1, 4), np.float32)
    plane_params[lab[1::3, 1::3].ravel()] = planes_gt[1::3, 1::3].reshape(-1, 4)  # the cell centres' planes
    with ACMMP(0) as eng:
        eng.set_params(_params(2))
        eng.set_images(cams, imgs)
        prm0 = eng.params
        eng.RunPatchMatch()
        eng.SetPlanarPriorParams()
        eng.CudaPlanarPriorInitialization(plane_params, mask)
        prm1 = eng.params
        eng.RunPatchMatch()
        got = (eng.plane_hypotheses(), eng.costs(), eng.selected_views())
    assert prm1.planar_prior == 1 and 0.4 < (mask > 0).mean() < 0.6
    ref0 = oracle.run_patchmatch(prm0, cams, imgs)
    per_pixel = np.where(mask[..., None] > 0, plane_params[np.maximum(mask.astype(np.int64) - 1, 0)], 0)
    ref1 = oracle.run_patchmatch(prm1, cams, imgs, planes=ref0["planes"], costs=ref0["costs"],
                                 prior_planes=per_pixel, masks=mask)
    _same(got, ref1, "planar prior, checkerboard mask")


def test_geometric_extreme_source_depths():
    """Source depth maps with 0, +-inf, NaN, a subnormal and 2^+-61 in
    stripes: geometric costs that are NaN, infinite or huge enter the sums."""
    nsrc = 5
    sc = scene.make_scene(num_views=nsrc + 1, width=40, height=30, arc_deg=4.0)
    special = np.array([0.0, np.inf, -np.inf, np.nan, 1e-40, 2.0 ** -61, 2.0 ** 61], np.float32)
    depths = []
    for n, i in enumerate([0] + sc.pairs[0][:nsrc]):
        d = sc.views[i].depth.astype(np.float32).copy()
        for k, v in enumerate(special):  # 2-column stripes, shifted per view, true depths between
            d[:, (3 * n + 5 * k) % 40:(3 * n + 5 * k) % 40 + 2] = v
        depths.append(d)
    _, refg = _photo_then_geom(sc, nsrc, 2, 2, "extreme depths", depths=depths)
    assert np.isfinite(refg["costs"]).mean() > 0.5


def _flat_rig(W, H, n):
    K = np.array([[100.0, 0, W / 2], [0, 100.0, H / 2], [0, 0, 1]])
    return [make_camera(K, np.eye(3), np.array([-5.0 * i, 0, 0]), W, H, 300, 800) for i in range(n)]


@pytest.mark.parametrize("level", [100.0, 77.0])
def test_constant_images_tie_the_bound(level):
    """Level 77: every NCC is 0 where the centre maps into the source, so
    every partial sum equals the bound (0 >= 0). Level 100: every NCC is 2 and
    no view is sampled, costs NaN (tests/test_gpu_parity.py, textureless)."""
    W, H = 48, 40
    cams = _flat_rig(W, H, 4)
    imgs = [np.full((H, W), level, np.float32) for _ in range(4)]
    prm, got = _gpu(_params(3), cams, imgs)
    _same(got, oracle.run_patchmatch(prm, cams, imgs), f"constant {level}")


def test_textureless_reference_columns():
    """A reference image constant in its left half (every cost there 2.0 or
    NaN) and textured in its right half, against textured sources: the waves
    along the seam hold both kinds of lane."""
    W, H = 48, 40
    sc = scene.make_scene(num_views=4, width=W, height=H, arc_deg=4.0)
    cams, imgs = sc.problem(0, 3)
    imgs = [im.copy() for im in imgs]
    imgs[0][:, :W // 2] = 100.0
    prm, got = _gpu(_params(3), cams, imgs)
    _same(got, oracle.run_patchmatch(prm, cams, imgs), "textureless reference half")


def test_hierarchy_gate_with_pre_costs():
    """hierarchy = 1 through the upsample init, which fills the pre-costs the
    gate (src/ACMMP.cu:1163-1172) compares the refined cost with."""
    W, H = 48, 36
    sc = scene.make_scene(num_views=5, width=W, height=H, arc_deg=4.0)
    cams, imgs = sc.problem(0, 4)
    v = sc.views[0]
    rng = np.random.default_rng(9)
    scaled = np.concatenate([v.normal[::2, ::2], rng.uniform(0, 1, (H // 2, W // 2, 1))], -1).astype(np.float32)
    up_depth = np.where(v.depth > 0, v.depth, 700.0).astype(np.float32)
    with ACMMP(0) as eng:
        eng.set_params(_params(2, hierarchy=1))
        eng.set_images(cams, imgs)
        eng.set_hierarchy_inputs(scaled, up_depth)
        prm = eng.params
        eng.RunPatchMatch()
        got = (eng.plane_hypotheses(), eng.costs())
    assert prm.upsample == 1
    planes_in = np.zeros((H, W, 4), np.float32)
    planes_in[..., 3] = up_depth
    ref = oracle.run_patchmatch(prm, cams, imgs, planes=planes_in, pre_costs=np.zeros((H, W), np.float32),
                                scaled_planes=scaled)
    assert (ref["pre_costs"] != 0).any()
    assert_bit_exact(got[0], ref["planes"], "planes (hierarchy gate)")
    assert_bit_exact(got[1], ref["costs"], "costs (hierarchy gate)")
