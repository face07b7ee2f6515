"""The CPU oracle against the float64 restatements of ref64.py on the general
rig (general_rig.py): cameras with fx != fy, an off-centre principal point, a
real rotation, source views of other sizes, an optional skew — and the stages
the suite compared only with the oracle until now: GetDepthandNormal,
CheckerboardFilter, JBU, the prior-plane fit and range check, the plane
generators of the random init. test_gpu_general_rig.py runs the same inputs
through the HIP kernels.

Every tolerance is stated where it is used, with the worst error measured on
the CPU oracle next to it.
"""
import numpy as np
import pytest

import oracle
import general_rig as rig
import ref64
from test_oracle_kat import H_TOL, NCC_TOL

# Round trip (geometric-branch init, then GetDepthandNormal) and filter: about
# a dozen fp32 roundings (6e-8 each) times the conditioning 1 / |n . ray| <= 3.5
# of the normals world_state draws. The median is 1-Lipschitz in the sup norm,
# so the filtered depth carries no more error than the unfiltered round trip.
ROUNDTRIP_DEPTH_RTOL = 4e-6    # measured: 1.9e-7 (2.1e-7 in the skip mix)
ROUNDTRIP_NORMAL_ATOL = 1e-6   # measured: 1.4e-7
# JBU: the fp32 rounding of the exponent argument; depths up to 800.
JBU_ATOL = 1e-5 * 800          # measured: 3.0e-4 (3.8e-7 x 800) at scale 2, 1.4e-3 (1.8e-6 x 800) at scale 4
# Prior plane, against the float64 fit of the same float32 depths: the fp32
# X, Y back-projection times the conditioning of a triangle of >= 20 px at
# f ~ 130.
PRIOR_NORMAL_ATOL = 5e-6       # measured: 6.4e-8
PRIOR_D_RTOL = 5e-6            # measured: 6.6e-8

ROUNDTRIP_SIZES = [(7, 6), (33, 33), (45, 31), (12, 65)]
JBU_SHAPES = [(24, 18, 12, 9), (21, 17, 10, 8), (24, 16, 6, 4)]


# ---------------------------------------------------------------------------
# shared inputs and checks (also used by the GPU tier)


def ncc_cases(n=200, seed=21):
    """(source index, px, py, plane) cases across the three source sizes."""
    rng = np.random.default_rng(seed)
    r = rig.make_rig(nsrc=3)
    W, H = rig.REF_SIZE
    planes = rig.random_planes(r.cams[0], seed)
    out = []
    for k in range(n):
        px, py = int(rng.integers(0, W)), int(rng.integers(0, H))
        out.append((1 + k % 3, px, py, planes[py, px]))
    return r, out


def check_cost_vectors(r, prm, planes, cost, what, step=5):
    """eval_costs' (H, W, nsrc) NCC vectors against ref_ncc on every
    step-th pixel; near-threshold cases may be left out, at most 2 %."""
    H, W = planes.shape[:2]
    worst, real, left_out, n = 0.0, 0, 0, 0
    for y in range(0, H, step):
        for x in range(y % step, W, step):
            for s in range(1, len(r.cams)):
                near = []
                want = ref64.ref_ncc(prm, r.cams[0], r.cams[s], r.imgs[0], r.imgs[s], x, y,
                                     planes[y, x].astype(np.float64), near)
                n += 1
                got = float(cost[y, x, s - 1])
                if near and abs(got - want) > NCC_TOL:
                    left_out += 1
                    continue
                assert abs(got - want) <= NCC_TOL, (what, x, y, s, got, want)
                worst = max(worst, abs(got - want))
                real += want < 2.0
    print(f"{what}: worst NCC error {worst:.3g}, {real} of {n} real, {left_out} left out")
    assert left_out <= 0.02 * n
    assert real >= 0.4 * n
    return worst


def check_geom_costs(r, planes, cost, what, step=3):
    H, W = planes.shape[:2]
    worst, left_out, n, graded = 0.0, 0, 0, 0
    for y in range(0, H, step):
        for x in range(0, W, step):
            for s in range(1, len(r.cams)):
                near = []
                want = ref64.ref_geom_cost(r.cams[0], r.cams[s], r.depths[s], planes[y, x].astype(np.float64),
                                           x, y, near)
                n += 1
                err = abs(float(cost[y, x, s - 1]) - want) / max(1.0, want)
                if near and err > 1e-3:
                    left_out += 1
                    continue
                assert err <= 1e-3, (what, x, y, s, float(cost[y, x, s - 1]), want)
                worst = max(worst, err)
                graded += 0.0 < want < 3.0
    print(f"{what}: worst geometric-cost error {worst:.3g}, {graded} of {n} below max_cost, {left_out} left out")
    assert left_out <= 0.02 * n
    assert graded >= 0.2 * n  # the cases do reach the reprojection error, not only the exits
    return worst


def roundtrip_problem(W, H, kind="general"):
    """Two views, geom_consistency = 1, max_iterations = 0, state planes =
    (world normal, depth). kind: "general" (rig cameras), "exact" (R = I,
    fx = fy = 128, normal (0, 0, -1), depths on the 1/4 grid: every fp32 step
    of the round trip is exact, and ties occur in the median), "skip" (the
    source camera is the reference camera, its image the reference image on
    the left half and another texture on the right)."""
    from acmmp_amd import make_camera
    rng = np.random.default_rng(W * 100 + H)
    if kind == "exact":
        K = np.array([[128.0, 0, W // 2 + 0.5], [0, 128.0, H // 2 - 0.5], [0, 0, 1]])
        cams = [make_camera(K, np.eye(3), np.zeros(3), W, H, *rig.DEPTH_RANGE),
                make_camera(K, np.eye(3), np.array([-1.0, 0, 0]), W, H, *rig.DEPTH_RANGE)]
        state = np.zeros((H, W, 4), np.float32)
        state[..., 2] = -1.0
        state[..., 3] = np.round(rng.uniform(*rig.DEPTH_RANGE, (H, W)))  # coarse: many ties
        state[..., 3] += rng.integers(0, 4, (H, W)) / 4
    else:
        cams = [rig.ref_camera(W, H), rig.ref_camera(W, H) if kind == "skip" else rig.source_camera(0, rng)]
        state = rig.world_state(cams[0], seed=W + H)
    imgs = [rig.image(c.height, c.width, 70 + i) for i, c in enumerate(cams)]
    if kind == "skip":
        imgs[1] = imgs[0].copy()
        imgs[1][:, W // 2:] = rig.image(H, W, 99)[:, W // 2:]
    depths = [rig.random_depth_map(c.height, c.width, rng) for c in cams]
    prm = rig.rig_params(cams[0], 2, geom_consistency=1, max_iterations=0)
    return prm, cams, imgs, depths, state


def check_roundtrip(cams, state, planes, costs, kind, what):
    """planes/costs: RunPatchMatch's output for roundtrip_problem."""
    H, W = state.shape[:2]
    rt = ref64.ref_roundtrip(cams[0], state)
    # the restated chain is the identity on its input: the depth to float64
    # rounding, the normal to the orthogonality of the camera's float32 R
    # (R^T R - I is a few 1e-8; the kernels read the same R, so rt is the target)
    assert np.abs(rt[..., 3] - state[..., 3]).max() < 1e-12 * rig.DEPTH_RANGE[1]
    assert np.abs(rt[..., :3] - state[..., :3]).max() < 3e-7
    want = ref64.ref_filter(rt[..., 3], costs, ref64.ref_checkerboard_rows(H))
    skipped = costs < np.float32(0.001)
    if kind == "exact":
        assert np.array_equal(planes[..., 3].view(np.uint32), want.astype(np.float32).view(np.uint32)), what
        assert np.all(planes[..., :3] == np.array([0, 0, -1], np.float32)), what
        # ties and both median forms do occur, and the filter does change depths
        assert (planes[..., 3] != state[..., 3]).mean() > 0.5
        return 0.0, 0.0
    derr = np.abs(planes[..., 3] - want) / want
    nerr = np.abs(planes[..., :3] - rt[..., :3])
    print(f"{what}: depth {derr.max():.3g} relative, normals {nerr.max():.3g}, skipped {skipped.mean():.3f}")
    assert derr.max() <= ROUNDTRIP_DEPTH_RTOL, (what, derr.max())
    assert nerr.max() <= ROUNDTRIP_NORMAL_ATOL, (what, nerr.max())
    if kind == "skip":
        assert 0.2 <= skipped.mean() <= 0.8, skipped.mean()
        kept = np.abs(planes[..., 3][skipped] - state[..., 3][skipped]) / state[..., 3][skipped]
        assert kept.max() <= ROUNDTRIP_DEPTH_RTOL
        assert (planes[..., 3] != state[..., 3])[~skipped].mean() > 0.5  # the others are filtered
    return derr.max(), nerr.max()


def jbu_problem(W, H, sw, sh):
    rng = np.random.default_rng(W * 1000 + sw)
    img = rig.image(H, W, W + H)
    dep = rng.uniform(400, 800, (sh, sw)).astype(np.float32)
    dep[rng.random((sh, sw)) < 0.05] = 0.0
    return img, dep


def check_jbu(img, dep, got, what):
    want = ref64.ref_jbu(img, dep)
    err = np.abs(got - want).max()
    print(f"{what}: worst JBU error {err:.3g} ({err / 800:.3g} x 800)")
    assert err <= JBU_ATOL, (what, err)
    return err


PRIOR_N = np.array([0.2, -0.3, -0.93]) / np.linalg.norm([0.2, -0.3, -0.93])
PRIOR_D = 500.0
# triangles (x1 y1 x2 y2 x3 y3) of the 96 x 72 view, shortest edge >= 20 px,
# disjoint; the last one's corner depths are moved out of [dmin, dmax]
PRIOR_TRIS = np.array([[5, 5, 40, 8, 12, 36], [50, 4, 90, 10, 70, 30], [8, 42, 30, 66, 45, 44],
                       [52, 38, 91, 45, 60, 68], [70, 33, 95, 12, 93, 36]], np.int32)
PRIOR_MOVED = 4
PRIOR_RANGE = (300.0, 800.0)


def prior_problem():
    cam = rig.ref_camera(depth_range=PRIOR_RANGE)
    W, H = rig.REF_SIZE
    ys, xs = np.mgrid[0:H, 0:W]
    depth = ref64.ref_depth_from_plane(cam, np.array([*PRIOR_N, PRIOR_D]), xs, ys).astype(np.float32)
    for k in range(3):  # a parallel plane at twice the distance: depth ~ 1080 > dmax
        x, y = PRIOR_TRIS[PRIOR_MOVED, 2 * k], PRIOR_TRIS[PRIOR_MOVED, 2 * k + 1]
        depth[y, x] *= 2
    assert PRIOR_RANGE[0] < depth.min() and np.sort(depth.ravel())[-4] < PRIOR_RANGE[1]
    return cam, depth


def _barycentric(tri, xs, ys):
    x1, y1, x2, y2, x3, y3 = [float(v) for v in tri]
    det = (y2 - y3) * (x1 - x3) + (x3 - x2) * (y1 - y3)
    a = ((y2 - y3) * (xs - x3) + (x3 - x2) * (ys - y3)) / det
    b = ((y3 - y1) * (xs - x3) + (x1 - x3) * (ys - y3)) / det
    return np.stack([a, b, 1 - a - b], -1)


def check_prior(cam, depth, planes, mask, what):
    H, W = depth.shape
    ys, xs = np.mgrid[0:H, 0:W]
    worst_n = worst_d = 0.0
    claimed = np.zeros((H, W), bool)
    for k, tri in enumerate(PRIOR_TRIS):
        want = ref64.ref_prior_plane(cam, tri, depth)
        assert want[3] >= 0
        if k != PRIOR_MOVED:  # the fit recovers the analytic plane
            assert np.abs(want[:3] - PRIOR_N).max() < 1e-5 and abs(want[3] - PRIOR_D) < 1e-5 * PRIOR_D
        worst_n = max(worst_n, np.abs(planes[k, :3] - want[:3]).max())
        worst_d = max(worst_d, abs(planes[k, 3] - want[3]) / want[3])
        bc = _barycentric(tri, xs, ys)
        inside = (bc > 0.06).all(-1)      # clear of the edges: the raster must label it
        claimed |= (bc > -0.06).all(-1)   # anything it may label
        d = ref64.ref_depth_from_plane(cam, want, xs, ys)
        in_range = (d >= PRIOR_RANGE[0]) & (d <= PRIOR_RANGE[1])
        assert in_range[inside].all() != (k == PRIOR_MOVED) and in_range[inside].any() != (k == PRIOR_MOVED)
        assert inside.sum() > 100
        assert np.all(mask[inside] == (0 if k == PRIOR_MOVED else k + 1)), (what, k)
    assert np.all(mask[~claimed] == 0)
    print(f"{what}: prior plane normal {worst_n:.3g}, d {worst_d:.3g} relative")
    assert worst_n <= PRIOR_NORMAL_ATOL and worst_d <= PRIOR_D_RTOL, (what, worst_n, worst_d)
    return worst_n, worst_d


def check_random_init(cam, prm, planes, what):
    """Properties of the plane generators (GenerateRandomPlaneHypothesis,
    src/ACMMP.cu:170-196, :235-241) seen through max_iterations = 0:
    (world normal, depth) after GetDepthandNormal and the filter."""
    H, W = planes.shape[:2]
    K, R, _ = ref64.cam_np(cam)
    n = planes[..., :3].astype(np.float64)
    assert np.abs(np.linalg.norm(n, axis=-1) - 1).max() <= 1e-6
    ys, xs = np.mgrid[0:H, 0:W]
    ray = np.stack([(xs - K[0, 2]) / K[0, 0], (ys - K[1, 2]) / K[1, 1], np.ones((H, W))], -1)
    ray /= np.linalg.norm(ray, axis=-1, keepdims=True)
    facing = ((n @ R.T) * ray).sum(-1)
    assert facing.max() <= 1e-5, facing.max()
    d = planes[..., 3].astype(np.float64)
    assert d.min() >= prm.depth_min * (1 - 1e-5) and d.max() <= prm.depth_max * (1 + 1e-5)
    u = (d - prm.depth_min) / (prm.depth_max - prm.depth_min)
    bound = 4 * 0.2887 / np.sqrt(d.size)  # 4 sigma of the mean of N uniform draws; the median filter narrows it
    print(f"{what}: max n.ray {facing.max():.3g}, mean depth share {u.mean():.4f} (bound +-{bound:.4f})")
    assert abs(u.mean() - 0.5) <= bound, u.mean()
    # the normals do spread over the hemisphere and the depths over the range
    assert facing.min() < -0.95 and (facing > -0.3).mean() > 0.1 and u.std() > 0.05


# ---------------------------------------------------------------------------
# the CPU tier


def test_homography_and_ncc_match_fp64_on_general_cameras():
    """H_TOL, NCC_TOL of test_oracle_kat.py. Measured: worst NCC error 1.6e-5,
    worst homography error 2.0e-6 of the largest entry; 172 of 200 cases are
    real NCC values, 0 left out."""
    r, cases = ncc_cases()
    prm = rig.rig_params(r.cams[0], 2)
    worst, worst_h, real, left_out = 0.0, 0.0, 0, 0
    for s, px, py, plane in cases:
        H = oracle.homography(r.cams[0], r.cams[s], plane).astype(np.float64)
        Href = ref64.ref_homography(r.cams[0], r.cams[s], plane.astype(np.float64))
        scale = np.abs(Href).max()
        np.testing.assert_allclose(H, Href, atol=H_TOL * scale)
        worst_h = max(worst_h, np.abs(H - Href).max() / scale)
        got = oracle.ncc(prm, r.cams[0], r.cams[s], r.imgs[0], r.imgs[s], px, py, plane)
        near = []
        want = ref64.ref_ncc(prm, r.cams[0], r.cams[s], r.imgs[0], r.imgs[s], px, py, plane.astype(np.float64), near)
        if near and abs(got - want) > NCC_TOL:
            left_out += 1
            continue
        assert abs(got - want) <= NCC_TOL, (s, px, py, got, want)
        worst = max(worst, abs(got - want))
        real += want < 2.0
    print(f"worst NCC error {worst:.3g}, homography {worst_h:.3g}, {real} of {len(cases)} real, {left_out} left out")
    assert left_out <= 0.02 * len(cases)
    assert real >= 0.4 * len(cases)


@pytest.mark.parametrize("skew", [False, True])
def test_geom_cost_matches_fp64_on_general_cameras(skew):
    """1e-3 * max(1, want), every third pixel, depth maps at each view's own
    size (80 x 60, 112 x 84, 64 x 90). Measured: worst error 2.8e-5 (no
    skew), 2.6e-5 (skew); 0 cases left out."""
    r = rig.make_rig(nsrc=3, skew=skew)
    prm = rig.rig_params(r.cams[0], 4, geom_consistency=1)
    planes = rig.random_planes(r.cams[0], 5)
    out = oracle.eval_geom_costs(prm, r.cams, r.imgs, r.depths, planes)
    check_geom_costs(r, planes, out, f"oracle, skew={skew}")


def test_skew_reaches_the_projection_only():
    """K[0][1] enters ProjectonCamera_cu (src/ACMMP.cu:514), not the
    homography (:313-321): the geometric cost changes, the NCC does not."""
    a, b = rig.make_rig(nsrc=3), rig.make_rig(nsrc=3, skew=True)
    planes = rig.random_planes(a.cams[0], 5)
    prm = rig.rig_params(a.cams[0], 4, geom_consistency=1)
    ga = oracle.eval_geom_costs(prm, a.cams, a.imgs, a.depths, planes)
    gb = oracle.eval_geom_costs(prm, b.cams, b.imgs, b.depths, planes)
    assert (ga != gb).mean() > 0.3
    ca = oracle.eval_costs(prm, a.cams, a.imgs, planes)
    cb = oracle.eval_costs(prm, b.cams, b.imgs, planes)
    for x, y in zip(ca, cb):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("W,H", ROUNDTRIP_SIZES)
def test_roundtrip_and_filter_match_fp64(W, H):
    """Measured: depth 1.9e-7 relative, normals 1.4e-7 (worst of the four sizes)."""
    prm, cams, imgs, depths, state = roundtrip_problem(W, H)
    out = oracle.run_patchmatch(prm, cams, imgs, depths=depths, planes=state, costs=np.zeros((H, W), np.float32))
    check_roundtrip(cams, state, out["planes"], out["costs"], "general", f"oracle {W}x{H}")
    if H in (33, 65):
        assert ref64.ref_checkerboard_rows(H) == H - 1


def test_roundtrip_and_filter_exact_kat():
    prm, cams, imgs, depths, state = roundtrip_problem(33, 33, "exact")
    out = oracle.run_patchmatch(prm, cams, imgs, depths=depths, planes=state, costs=np.zeros((33, 33), np.float32))
    check_roundtrip(cams, state, out["planes"], out["costs"], "exact", "oracle exact KAT")


def test_filter_skips_converged_pixels():
    """Measured: 0.39 of the pixels skipped; depth 2.1e-7 relative, normals 1.2e-7."""
    prm, cams, imgs, depths, state = roundtrip_problem(48, 40, "skip")
    out = oracle.run_patchmatch(prm, cams, imgs, depths=depths, planes=state, costs=np.zeros((40, 48), np.float32))
    check_roundtrip(cams, state, out["planes"], out["costs"], "skip", "oracle skip mix")


@pytest.mark.parametrize("W,H,sw,sh", JBU_SHAPES)
def test_jbu_matches_fp64(W, H, sw, sh):
    img, dep = jbu_problem(W, H, sw, sh)
    got, isc = oracle.jbu(img, dep)
    assert isc == max(H // sh, W // sw) >= 2
    check_jbu(img, dep, got, f"oracle {W}x{H}<-{sw}x{sh}")


def test_prior_plane_and_range_check_match_fp64():
    cam, depth = prior_problem()
    planes, mask, prior = oracle.planar_prior(cam, depth, *PRIOR_RANGE, PRIOR_TRIS)
    check_prior(cam, depth, planes, mask, "oracle")
    lab = mask.astype(np.int64) - 1
    assert np.array_equal(prior[mask > 0], planes[lab[mask > 0]]) and np.all(prior[mask == 0] == 0)


def test_random_init_properties():
    """Measured: max n.ray -1.5e-5, |mean depth share - 0.5| = 0.0034
    (bound 0.0139 at N = 6912)."""
    r = rig.make_rig(nsrc=3)
    prm = rig.rig_params(r.cams[0], 4, max_iterations=0)
    out = oracle.run_patchmatch(prm, r.cams, r.imgs)
    check_random_init(r.cams[0], prm, out["planes"], "oracle")
