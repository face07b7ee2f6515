"""The inputs of test_general_rig_cpu.py through the HIP kernels: general
cameras (fx != fy, off-centre principal point, real rotation, optional skew),
source views and depth maps of other sizes than the reference view, and the
stages no float64 restatement covered before (GetDepthandNormal, the
checkerboard filter, JBU, the prior-plane fit and range check, the random
init's plane generators).

Each case compares the GPU with the oracle bit-for-bit and, where ref64.py
restates the stage, with float64 at the CPU tier's tolerances, so a failure
names the wrong side.
"""
import numpy as np
import pytest

import oracle
import general_rig as rig
import test_general_rig_cpu as cpu
from acmmp_amd import ACMMP, joint_bilateral_upsample
from parity_util import assert_bit_exact
from test_oracle_kat import _init_cost_restated

pytestmark = pytest.mark.gpu


def _engine(prm, cams, imgs):
    eng = ACMMP(0)
    eng.set_params(prm)
    eng.set_images(cams, imgs, keep_depth_range=True)
    return eng


@pytest.mark.parametrize("texels", ["u8", "h16", "f32"])
def test_eval_costs_general_rig(texels):
    r = rig.make_rig(nsrc=3, texels=texels)
    planes = rig.random_planes(r.cams[0], 7)
    with _engine(rig.rig_params(r.cams[0], 4), r.cams, r.imgs) as eng:
        assert eng.texel_bits() == rig.TEXEL_BITS[texels]
        prm = eng.params
        g_cost, g_init, g_views = eng.eval_costs(planes)
    assert (prm.depth_min, prm.depth_max) == rig.DEPTH_RANGE
    r_cost, r_init, r_views = oracle.eval_costs(prm, r.cams, r.imgs, planes)
    assert_bit_exact(g_cost, r_cost, f"ncc cost vectors ({texels})")
    assert_bit_exact(g_init, r_init, f"initial cost ({texels})")
    assert_bit_exact(g_views, r_views, f"initial selected views ({texels})")
    cpu.check_cost_vectors(r, prm, planes, g_cost, f"gpu {texels}")
    H, W = g_init.shape
    for y in range(0, H, 3):  # the aggregation, restated on the GPU's own vectors
        for x in range(0, W, 3):
            c, m = _init_cost_restated(g_cost[y, x], prm.top_k)
            assert g_init[y, x].view(np.uint32) == c.view(np.uint32) and g_views[y, x] == m, (x, y)


@pytest.mark.parametrize("skew", [False, True])
def test_eval_geom_costs_general_rig(skew):
    r = rig.make_rig(nsrc=3, skew=skew)
    planes = rig.random_planes(r.cams[0], 5)
    with _engine(rig.rig_params(r.cams[0], 4, geom_consistency=1), r.cams, r.imgs) as eng:
        eng.set_depth_maps(r.depths)
        prm = eng.params
        g = eng.eval_geom_costs(planes)
    o = oracle.eval_geom_costs(prm, r.cams, r.imgs, r.depths, planes)
    assert_bit_exact(g, o, f"geometric cost (skew={skew})")
    cpu.check_geom_costs(r, planes, g, f"gpu, skew={skew}")


@pytest.mark.parametrize("nsrc", [3, 10])
@pytest.mark.parametrize("geom", [False, True])
def test_one_iteration_general_rig(geom, nsrc):
    """nsrc = 3 runs the 4-source kernels, nsrc = 10 the 16-source ones with
    the per-view path above 9 sources."""
    r = rig.make_rig(nsrc=nsrc)
    H, W = r.imgs[0].shape
    kw = {}
    with _engine(rig.rig_params(r.cams[0], nsrc + 1, max_iterations=1, geom_consistency=int(geom)),
                 r.cams, r.imgs) as eng:
        if geom:
            state = rig.world_state(r.cams[0], seed=nsrc, lo=20.0, hi=50.0)
            costs = np.random.default_rng(nsrc).uniform(0, 0.3, (H, W)).astype(np.float32)
            eng.set_depth_maps(r.depths)
            eng.set_plane_hypotheses(state, costs)
            kw = dict(depths=r.depths, planes=state, costs=costs)
        prm = eng.params
        eng.RunPatchMatch()
        pl, co, sv = eng.plane_hypotheses(), eng.costs(), eng.selected_views()
    ref = oracle.run_patchmatch(prm, r.cams, r.imgs, **kw)
    assert_bit_exact(pl, ref["planes"], "planes")
    assert_bit_exact(co, ref["costs"], "costs")
    assert_bit_exact(sv, ref["selected_views"], "selected views")
    assert np.isfinite(ref["costs"]).mean() > 0.9 and (ref["costs"] < 1.0).mean() > 0.1


def _roundtrip(W, H, kind):
    prm, cams, imgs, depths, state = cpu.roundtrip_problem(W, H, kind)
    zeros = np.zeros((H, W), np.float32)
    with _engine(prm, cams, imgs) as eng:
        eng.set_depth_maps(depths)
        eng.set_plane_hypotheses(state, zeros)
        prm = eng.params
        eng.RunPatchMatch()
        pl, co = eng.plane_hypotheses(), eng.costs()
    ref = oracle.run_patchmatch(prm, cams, imgs, depths=depths, planes=state, costs=zeros)
    assert_bit_exact(pl, ref["planes"], f"planes ({kind} {W}x{H})")
    assert_bit_exact(co, ref["costs"], f"costs ({kind} {W}x{H})")
    cpu.check_roundtrip(cams, state, pl, co, kind, f"gpu {kind} {W}x{H}")


@pytest.mark.parametrize("W,H", cpu.ROUNDTRIP_SIZES)
def test_roundtrip_and_filter_general_cameras(W, H):
    _roundtrip(W, H, "general")


def test_roundtrip_and_filter_exact_kat():
    _roundtrip(33, 33, "exact")


def test_filter_skips_converged_pixels():
    _roundtrip(48, 40, "skip")


@pytest.mark.parametrize("W,H,sw,sh", cpu.JBU_SHAPES)
def test_jbu_matches_oracle_and_fp64(W, H, sw, sh):
    img, dep = cpu.jbu_problem(W, H, sw, sh)
    got, isc = joint_bilateral_upsample(img, dep)
    ref, risc = oracle.jbu(img, dep)
    assert isc == risc == max(H // sh, W // sw)
    assert_bit_exact(got, ref, f"jbu {W}x{H}<-{sw}x{sh}")
    cpu.check_jbu(img, dep, got, f"gpu {W}x{H}<-{sw}x{sh}")


def test_prior_plane_and_range_check():
    cam, depth = cpu.prior_problem()
    H, W = depth.shape
    cams = [cam, rig.source_camera(0, np.random.default_rng(3), depth_range=cpu.PRIOR_RANGE)]
    imgs = [rig.image(c.height, c.width, 80 + i) for i, c in enumerate(cams)]
    state = np.zeros((H, W, 4), np.float32)
    state[..., :3] = cpu.PRIOR_N
    state[..., 3] = depth
    with _engine(rig.rig_params(cam, 2), cams, imgs) as eng:
        eng.set_plane_hypotheses(state, np.zeros((H, W), np.float32))
        prm = eng.params
        planes, mask = eng.build_planar_prior(cpu.PRIOR_TRIS)
    assert (prm.depth_min, prm.depth_max) == cpu.PRIOR_RANGE
    r_planes, r_mask, _ = oracle.planar_prior(cam, depth, prm.depth_min, prm.depth_max, cpu.PRIOR_TRIS)
    assert_bit_exact(planes, r_planes, "prior plane params")
    np.testing.assert_array_equal(mask, r_mask)
    cpu.check_prior(cam, depth, planes, mask, "gpu")


def test_random_init_properties():
    r = rig.make_rig(nsrc=3)
    with _engine(rig.rig_params(r.cams[0], 4, max_iterations=0), r.cams, r.imgs) as eng:
        prm = eng.params
        eng.RunPatchMatch()
        pl, co = eng.plane_hypotheses(), eng.costs()
    ref = oracle.run_patchmatch(prm, r.cams, r.imgs)
    assert_bit_exact(pl, ref["planes"], "planes")
    assert_bit_exact(co, ref["costs"], "costs")
    cpu.check_random_init(r.cams[0], prm, pl, "gpu")
