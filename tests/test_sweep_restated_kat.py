"""Known answers for the restatement of the sweep's decision layer
(tests/ref_sweep.py), small enough to check by hand against the reference's
lines (rlav440/ACMMP, src/ACMMP.cu), so that the restatement is more than a
third copy: the sampling pattern (:813-991), the view selection (:994-1056),
the refinement's order and accept rules (:707-784), the rows the checkerboard
grid covers (:1399).

The NCC never enters: where a chain is run it gets a stand-in backend whose
cost is a stated function of the plane. Transcendentals and uniform draws are
the pinned ones of tests/test_detmath.py.
"""
import math

import numpy as np
import pytest

import ref_sweep as rs
from acmmp_amd import default_params, make_camera

F = np.float32
W53, H49 = 53, 49


# ------------------------------------------------------------ sampling pattern
def _offsets(table, r, y, x, H=H49, W=W53):
    return [(py - y, px - x) for py, px in rs.region_samples(table, r, y, x, H, W)]


def test_interior_pixel_reads_full_strips_and_v_areas():
    """(x 26, y 24) of a 53x49 image has 23 pixels of room on every side."""
    t = rs.sampling_table()
    far = [3 + 2 * i for i in range(11)]
    assert far == [3, 5, 7, 9, 11, 13, 15, 17, 19, 21, 23]
    assert _offsets(t, 1, 24, 26) == [(-k, 0) for k in far]          # up_far, :814-828
    assert _offsets(t, 3, 24, 26) == [(k, 0) for k in far]           # down_far
    assert _offsets(t, 5, 24, 26) == [(0, -k) for k in far]          # left_far
    assert _offsets(t, 7, 24, 26) == [(0, k) for k in far]           # right_far
    # up_near, :890-911: center - width, then up_near - (1+i) width -/+ i for i = 0, 1, 2
    assert _offsets(t, 0, 24, 26) == [(-1, 0), (-2, 0), (-2, 0), (-3, -1), (-3, 1), (-4, -2), (-4, 2)]
    assert _offsets(t, 2, 24, 26) == [(1, 0), (2, 0), (2, 0), (3, -1), (3, 1), (4, -2), (4, 2)]
    # left_near, :942-964: left_near - (1+i) -/+ i width
    assert _offsets(t, 4, 24, 26) == [(0, -1), (0, -2), (0, -2), (-1, -3), (1, -3), (-2, -4), (2, -4)]
    assert _offsets(t, 6, 24, 26) == [(0, 1), (0, 2), (0, 2), (-1, 3), (1, 3), (-2, 4), (2, 4)]
    # every V sample has the pixel's own colour, every strip sample the other one
    for r in range(8):
        for s, (dy, dx) in enumerate(_offsets(t, r, 24, 26)):
            assert (dy + dx) % 2 == (0 if (r % 2 == 0 and s > 0) else 1)


def test_full_strips_need_23_pixels_of_room_on_every_side():
    t = rs.sampling_table()
    full = lambda H, W: any(all(len(rs.region_samples(t, r, y, x, H, W)) == 11 for r in (1, 3, 5, 7))
                            for y in range(H) for x in range(W))
    assert full(49, 53) and full(47, 47) and not full(46, 53) and not full(49, 46)


def test_borders_and_corners_truncate():
    t = rs.sampling_table()
    # corner (0, 0): nothing above or to the left
    for r in (0, 1, 4, 5):
        assert _offsets(t, r, 0, 0) == []
    # down_near at x = 0: the left arm needs p.x > i, so even its i = 0 sample (dx = 0) is left out (:922)
    assert _offsets(t, 2, 0, 0) == [(1, 0), (2, 0), (3, 1), (4, 2)]
    assert _offsets(t, 6, 0, 0) == [(0, 1), (0, 2), (1, 3), (2, 4)]
    assert len(_offsets(t, 3, 0, 0)) == 11 and len(_offsets(t, 7, 0, 0)) == 11
    # corner (52, 48)
    for r in (2, 3, 6, 7):
        assert _offsets(t, r, 48, 52) == []
    assert _offsets(t, 0, 48, 52) == [(-1, 0), (-2, 0), (-3, -1), (-4, -2)]
    assert _offsets(t, 4, 48, 52) == [(0, -1), (0, -2), (-1, -3), (-2, -4)]
    # near the top-left: y = 5 gives up_far 3 and 5 (p.y > 2 + 2i, :820), x = 4 gives left_far 3 only
    assert _offsets(t, 1, 5, 4) == [(-3, 0), (-5, 0)]
    assert _offsets(t, 5, 5, 4) == [(0, -3)]
    assert _offsets(t, 1, 2, 4) == [] and _offsets(t, 1, 3, 4) == [(-3, 0)]
    # p.y > 1 + i (:896): at y = 2 only the i = 0 arms; at y = 1 the start alone
    assert _offsets(t, 0, 2, 26) == [(-1, 0), (-2, 0), (-2, 0)]
    assert _offsets(t, 0, 1, 26) == [(-1, 0)]
    # right border: x = 50 = W - 3 has no right_far (p.x < width - 3), x = 49 the start alone
    assert _offsets(t, 7, 24, 50) == [] and _offsets(t, 7, 24, 49) == [(0, 3)]
    assert _offsets(t, 6, 24, 51) == [(0, 1)] and _offsets(t, 6, 24, 52) == []


@pytest.mark.parametrize("r", range(8))
def test_planted_extremum_is_chosen(r):
    """Costs 1 everywhere; a planted 0.5 at any sample of a region is the
    position that region picks, except in right_far, whose compare is reversed
    (:879): it picks a planted 1.5 and never a planted 0.5."""
    t = rs.sampling_table()
    ys, xs = np.array([24]), np.array([26])
    samples = rs.region_samples(t, r, 24, 26, H49, W53)
    for s, (py, px) in enumerate(samples):
        costs = np.ones((H49, W53), F)
        costs[py, px] = 1.5 if r == 7 else 0.5
        flag, pos_y, pos_x, _ = rs.choose_candidates(t, costs, ys, xs)
        assert flag.all()
        assert (pos_y[0, r], pos_x[0, r]) == (py, px), (r, s)
        for q in range(8):          # the other regions stay at their start samples
            if q != r and (py, px) not in rs.region_samples(t, q, 24, 26, H49, W53):
                assert (pos_y[0, q], pos_x[0, q]) == rs.region_samples(t, q, 24, 26, H49, W53)[0]
    if r == 7:
        costs = np.ones((H49, W53), F)
        costs[24, 26 + 9] = 0.5
        _, pos_y, pos_x, _ = rs.choose_candidates(t, costs, ys, xs)
        assert (pos_y[0, 7], pos_x[0, 7]) == (24, 29)
        # two maxima: the strict compare keeps the first
        costs[24, 26 + 5] = costs[24, 26 + 11] = 1.5
        _, pos_y, pos_x, _ = rs.choose_candidates(t, costs, ys, xs)
        assert (pos_y[0, 7], pos_x[0, 7]) == (24, 31)


def test_tied_minimum_keeps_the_first_sample():
    t = rs.sampling_table()
    costs = np.ones((H49, W53), F)
    costs[24 - 7, 26] = costs[24 - 13, 26] = 0.25
    _, pos_y, _, _ = rs.choose_candidates(t, costs, np.array([24]), np.array([26]))
    assert pos_y[0, 1] == 24 - 7


# -------------------------------------------------------------- view selection
def _stub_draws(values):
    return lambda k: np.array([values[k]], F)


def _hand_array():
    """One pixel, four views: 0 all costs 0; 1 three costs above 1.2;
    2 two costs below the threshold; 3 three costs of 0.3, the rest 1.0."""
    ca = np.zeros((1, 8, 4), F)
    ca[0, :, 1] = [1.3, 1.3, 1.3, 0, 0, 0, 0, 0]
    ca[0, :, 2] = [0.1, 0.1, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]
    ca[0, :, 3] = [0.3, 0.3, 0.3, 1.0, 1.0, 1.0, 1.0, 1.0]
    return ca


def test_view_selection_probabilities():
    ca = _hand_array()
    flags = np.ones((1, 4), bool)
    #                 up      down    left    right      (bit j = view j)
    views = np.array([[0b0001, 0b0101, 0b1111, 0b0000]], np.uint32)
    draws = [(k + 0.5) / 15 for k in range(15)]
    out = rs.select_views(ca, flags, views, 0, _stub_draws(draws))
    votes = [0.9 + 0.9 + 0.9 + 0.1, 0.1 + 0.1 + 0.9 + 0.1, 0.1 + 0.9 + 0.9 + 0.1, 0.1 + 0.1 + 0.9 + 0.1]
    thr = 0.8
    expect = [1.0 * votes[0], 0.0, math.exp(thr * thr / -0.32) * votes[2], math.exp(-0.09 / 0.18) * votes[3]]
    assert out["branch"].tolist() == [[0, 2, 1, 0]]
    # float32 sums of four terms and expf within 2 ulp: 1e-6 relative covers both
    np.testing.assert_allclose(out["probs"][0], expect, rtol=1e-6, atol=0)
    assert out["probs"][0, 1] == 0.0
    np.testing.assert_allclose(out["cdf"][0], np.cumsum(expect) / np.sum(expect), rtol=1e-6)
    w = out["weights"][0]
    assert w[1] == 0 and np.all(w == np.round(w)) and w.sum() == 15 == out["weight_norm"][0]
    assert out["mask"][0] == sum(1 << j for j in range(4) if w[j] > 0) == 0b1101
    # the stub draws are the 15 midpoints of [0, 1): view j gets the midpoints inside its CDF step
    cdf = np.cumsum(expect) / np.sum(expect)
    assert w.tolist() == [sum(1 for u in draws if (cdf[j - 1] if j else 0) <= u < cdf[j]) for j in range(4)]


def test_view_selection_absent_neighbours_do_not_vote():
    ca = _hand_array()
    views = np.array([[0b0001, 0b0001, 0b0001, 0b0001]], np.uint32)
    flags = np.array([[True, False, False, True]])
    out = rs.select_views(ca, flags, views, 0, _stub_draws([0.5] * 15))
    np.testing.assert_allclose(out["probs"][0, 0], 1.8, rtol=1e-6)
    np.testing.assert_allclose(out["probs"][0, 3], math.exp(-0.5) * 0.2, rtol=1e-6)


def test_draw_equal_to_cdf_step_selects_that_view():
    """:1036-1040: prob > rand - FLT_EPSILON, so a draw exactly on a CDF step
    still lands in that step's view."""
    ca = np.zeros((1, 8, 2), F)
    flags = np.ones((1, 4), bool)
    views = np.array([[3, 3, 3, 3]], np.uint32)
    out = rs.select_views(ca, flags, views, 0, _stub_draws([0.5] * 15))
    assert out["cdf"][0].tolist() == [0.5, 1.0]
    assert out["weights"][0].tolist() == [15, 0]
    out = rs.select_views(ca, flags, views, 0, _stub_draws([0.5] * 15), variant="no_epsilon")
    assert out["weights"][0].tolist() == [0, 15]
    out = rs.select_views(ca, flags, views, 0, _stub_draws([0.5] * 15), variant="samples14")
    assert out["weights"][0].tolist() == [14, 0]


def test_all_views_rejected_gives_zero_weight_norm():
    ca = np.full((1, 8, 3), 1.5, F)
    out = rs.select_views(ca, np.ones((1, 4), bool), np.zeros((1, 4), np.uint32), 0, _stub_draws([0.3] * 15))
    assert out["weights"].sum() == 0 and out["weight_norm"][0] == 0 and out["mask"][0] == 0
    assert np.isnan(out["cdf"]).all()       # 0 * (1 / 0), :113-119


def test_cost_array_initialiser():
    """:805: {2.0f} sets [0][0] alone; an absent region keeps those values."""
    costs = np.full((1, 8, 3), 0.7, F)
    flag = np.array([[False, True, False, True, True, True, True, True]])
    ca = rs.fill_cost_array(flag, costs)
    assert ca[0, 0].tolist() == [2.0, 0.0, 0.0] and ca[0, 2].tolist() == [0.0, 0.0, 0.0]
    assert np.all(ca[0, [1, 3, 4, 5, 6, 7]] == F(0.7))
    flag[0, 0] = True
    assert np.all(rs.fill_cost_array(flag, costs)[0, 0] == F(0.7))
    # what it does to the selection at the top row: view 0 has the 2.0 (above 1.2, not below the threshold)
    # where the other views have a 0 that counts with exp(0) = 1; the absent down_near is 0 for all three
    out = rs.select_views(ca, np.ones((1, 4), bool), np.zeros((1, 4), np.uint32), 0, _stub_draws([0.5] * 15))
    p = out["probs"][0] / F(0.4)
    e = math.exp(-0.49 / 0.18)
    np.testing.assert_allclose(p, [(6 * e + 1) / 7, (6 * e + 2) / 8, (6 * e + 2) / 8], rtol=1e-6)


@pytest.mark.parametrize("it", [0, 1, 2])
def test_cost_threshold(it):
    """:1011 against 0.8 exp(-iter^2 / 90) in float64: the float quotient, the
    pinned expf (within 2 ulp) and the final rounding, 4 ulp = 4.8e-7 relative."""
    assert abs(float(rs.cost_threshold(it)) / (0.8 * math.exp(-it * it / 90.0)) - 1) < 4.8e-7
    if it == 0:
        assert rs.cost_threshold(0) == F(0.8)


# ------------------------------------------------------------------ refinement
def test_refinement_pairings_order():
    """:740-741"""
    got = rs.refinement_pairings("d", "n", "d_rand", "n_rand", "d_pert", "n_pert")
    assert got == [("d_rand", "n"), ("d", "n_rand"), ("d_rand", "n_rand"), ("d", "n_pert"), ("d_pert", "n")]


class _Backend:
    """Stand-in primitives: the cost of a plane at a pixel is fn(depth there),
    the same for every view."""

    def __init__(self, cam, nsrc, fn):
        self.K = np.array(list(cam.K), F)
        self.H, self.W, self.V, self.fn = cam.height, cam.width, nsrc, fn

    def cost_vectors(self, planes):
        ys, xs = np.mgrid[0:self.H, 0:self.W]
        c = self.fn(rs.depth_from_plane(self.K, np.asarray(planes, F), ys, xs)).astype(F)
        return np.repeat(c[..., None], self.V, -1)

    def init_cost(self, planes):
        return self.cost_vectors(planes)[..., 0], np.full((self.H, self.W), (1 << self.V) - 1, np.uint32)


def _fronto_problem(W, H, depth_of_pixel, nsrc=2, **kw):
    """Seeded init (:634) from fronto-parallel planes n = (0, 0, -1), d = depth."""
    K = np.array([[100.0, 0, W / 2], [0, 100.0, H / 2], [0, 0, 1]])
    cams = [make_camera(K, np.eye(3), [-5.0 * i, 0, 0], W, H, 300, 800) for i in range(nsrc + 1)]
    p = default_params()
    p.max_iterations, p.num_images, p.depth_min, p.depth_max, p.seeded = 1, nsrc + 1, 300, 800, 1
    for k, v in kw.items():
        setattr(p, k, v)
    seed = np.zeros((H, W, 4), F)
    seed[..., 2] = -1
    seed[..., 3] = depth_of_pixel
    return rs.Problem(p, cams, [np.zeros((H, W), F)] * (nsrc + 1), seed_planes=seed), cams


def test_hypothesis_outside_the_depth_range_is_never_accepted():
    """Every pixel starts at 799.9 of [300, 800]; the stand-in cost is 0 beyond
    800 and 1 inside, so the perturbed-depth hypothesis (up to +2 %, :732-735)
    has the best cost wherever it leaves the range, and :777 still rejects it."""
    prob, cams = _fronto_problem(9, 7, 799.9)
    be = _Backend(cams[0], 2, lambda d: np.where(d > 800, 0.0, 1.0))
    r = rs.SweepRestated(prob, be)
    r.init()
    r.half_sweep(0, 0)
    tr = r.traces[0]
    outside = tr.extra["hyp_depth"][:, 4] > 800
    assert outside.sum() >= 5 and (~outside).sum() >= 5
    assert np.all(tr.extra["hyp_cost"][outside, 4] == 0) and not tr.hyp_accepted[outside, 4].any()
    assert not tr.hyp_accepted.any()        # inside the range every cost ties at 1: `<` is strict
    assert np.all(rs.depth_from_plane(r.cam.K, r.planes, *np.mgrid[0:7, 0:9]) <= 800)


def _prior_problem(depth_of_pixel):
    W, H = 9, 7
    prob, cams = _fronto_problem(W, H, depth_of_pixel, planar_prior=1)
    prior = np.zeros((H, W, 4), F)
    prior[..., 2], prior[..., 3] = -1, 600.0
    prob.prior_planes, prob.masks = prior, np.ones((H, W), np.uint32)
    return prob, _Backend(cams[0], 2, lambda d: np.full(d.shape, 0.5))


def test_restricted_cost_starts_from_zero_without_a_planar_accept():
    """Every pixel already lies on its prior plane and all costs tie, so no
    candidate's posterior exceeds the current one (:1129 is strict) and
    restricted_cost stays 0 (:1094). The refinement compares against that 0
    (:769), not against the current plane's posterior: its first hypothesis,
    whose posterior is lower than the current plane's, is accepted."""
    prob, be = _prior_problem(600.0)
    r = rs.SweepRestated(prob, be)
    r.init()
    r.half_sweep(0, 0)
    tr = r.traces[0]
    assert not tr.planar_accept.any() and np.all(tr.extra["restricted_in"] == 0)
    assert tr.hyp_accepted[:, 0].all()
    assert np.all(tr.extra["hyp_depth"][:, 0] != 600.0)     # a worse plane than the one it replaced


def test_shadowed_depth_now_after_a_planar_accept():
    """:1119 declares a second depth_now inside the prior block, and :1130
    assigns to it: after a posterior accept the refinement still perturbs the
    OLD plane's depth. Black pixels start at depth 500, red ones on the prior
    plane at 600 (sigma is 7.8): every black pixel accepts a red neighbour's
    plane, restricted_cost becomes that posterior, and hypotheses 1 and 3 are
    built on depth 500."""
    ys, xs = np.mgrid[0:7, 0:9]
    prob, be = _prior_problem(np.where((ys + xs) % 2 == 0, 500.0, 600.0))
    r = rs.SweepRestated(prob, be)
    r.init()
    r.half_sweep(0, 0)
    tr = r.traces[0]
    assert tr.planar_accept.all() and tr.shadowed.all() and (tr.region >= 0).all()
    post = math.exp(-0.25 / 0.18) * 1.5                     # exp(-c^2 / beta) (gamma + 1 * 1), :1112-1113
    np.testing.assert_allclose(tr.extra["restricted_in"], post, rtol=1e-6)
    assert np.all(tr.extra["depth_into_refinement"] == 500.0)
    assert np.all(tr.extra["hyp_depth"][:, 1] == 500.0) and np.all(tr.extra["hyp_depth"][:, 3] == 500.0)
    lo, hi = tr.extra["hyp_depth"][:, 4].min(), tr.extra["hyp_depth"][:, 4].max()
    assert 490.0 <= lo < hi <= 510.0                        # (1 -/+ 0.02) * 500, :732-735
    assert not tr.hyp_accepted.any()                        # nothing beats the prior plane itself
    black = (ys + xs) % 2 == 0
    assert np.all(r.planes[black][:, 3] == 600.0)
    mask = ((tr.weights > 0) * (1 << np.arange(tr.weights.shape[1]))).sum(1)
    assert np.all(r.sv[tr.ys, tr.xs] == mask)               # :1134


# ------------------------------------------------------------------------ rows
def test_last_row_of_37x33_is_read_but_never_swept_or_filtered():
    """:1399: (33 / 2 + 15) / 16 = 1 block of 16 row pairs: rows 0..31."""
    assert rs.sweep_rows(33) == 32 and rs.sweep_rows(49) == 49 and rs.sweep_rows(7) == 7
    assert rs.sweep_rows(65) == 64 and rs.sweep_rows(64) == 64 and rs.sweep_rows(31) == 31
    W, H = 37, 33
    ys, xs = np.mgrid[0:H, 0:W]
    depth = 500.0 + 3.0 * ((ys * 7 + xs * 3) % 11)
    prob, cams = _fronto_problem(W, H, depth)
    be = _Backend(cams[0], 2, lambda d: np.abs(d - 520.0) / 100.0 + 0.01)
    r = rs.SweepRestated(prob, be)
    out = r.run()
    swept = np.zeros((H, W), int)
    read_last = False
    for tr in out["traces"]:
        swept[tr.ys, tr.xs] += 1
        read_last |= bool((tr.flags & (tr.pos_y == H - 1)).any())
    assert np.all(swept[:32] == 1) and np.all(swept[32] == 0)
    assert read_last                                        # rows 31, 29 ... reach it through the down regions
    # never filtered: the last row holds its seeded depths, which no median of neighbours reproduces everywhere
    assert np.all(out["planes"][32, :, 3] == depth[32].astype(F))
    assert np.all(out["selected_views"][32] == 3)
