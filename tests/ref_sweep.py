"""The decision layer of RunPatchMatch restated from the reference's lines
(rlav440/ACMMP, src/ACMMP.cu), not from oracle/ or the HIP kernels: a second
reading of RandomInitialization (:609-705), CheckerboardPropagation (:786-1173),
PlaneHypothesisRefinement (:707-784), GetDepthandNormal (:1199-1212) and the
checkerboard filter (:1214-1352), chained as RunPatchMatch chains them
(:1378-1456).

What it takes from outside (each pinned elsewhere in the suite):
  - NCC cost vectors, the initial cost with its selected views and the
    geometric cost, through a backend (OracleBackend / EngineBackend below);
  - uniform draws, oracle.uniform (Philox, tests/test_detmath.py); WHICH draw
    each use consumes is restated here;
  - expf / sinf / cosf / acosf, oracle.math_fn (tests/test_detmath.py).
Everything else is numpy float32 arithmetic in the reference's operation
order (IEEE, no contraction), so the outputs compare bit for bit.

Structure: whole half-sweeps on arrays of pixels; the eight sampling regions
come from one offset table (sampling_table) built from a direction and a
"room" guard per sample, not from eight unrolled blocks.

Documented pins followed (SURVEY Appendix A / DESIGN §3):
  A1  curand -> Philox, counter (pixel, draw, phase, stream); phase 0 is the
      init, phase 1 + iter a half-sweep; the draw counter of a pixel runs on
      from the view selection into the refinement.
  A2  every read of another pixel in a half-sweep sees the state at the start
      of that half-sweep (the same-colour V reads race in the reference).
  A3  plane_hypotheses_now starts as plane_hypotheses[center] as it stands at
      :1149.
  A6  rsqrtf is 1 / sqrt (include/acmmp_detmath.h); exp/acos of floats are
      the float functions (--use_fast_math).
  The upsampling Gaussians (pinned semantics): in SpatialGauss /
      RangeGauss (:151-161) pow(v, 2) is v * v in float, and the double
      `-1.0 * dis / (2 sigma^2)` is rounded to float before the float expf.

`variant=` changes one rule at a time (VARIANTS) for the sensitivity test.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

import oracle

F = np.float32
FLT_EPSILON = F(1.1920928955078125e-07)

REGIONS = ("up_near", "up_far", "down_near", "down_far", "left_near", "left_far", "right_near", "right_far")
_DIR = {"up": (-1, 0), "down": (1, 0), "left": (0, -1), "right": (0, 1)}

VARIANTS = (
    "right_far_min",       # :879 as a minimum search
    "strip10",             # :819 etc. with i < 10
    "v_live",              # pin A2 dropped for the V areas: rows see the rows already swept
    "vote_swapped",        # :1002-1004 with 0.1 for a set bit
    "count_ge2",           # :1025 as count >= 2
    "no_epsilon",          # :1036 without - FLT_EPSILON
    "samples14",           # :1035 with 14 draws
    "refine_draws_swapped",  # :728-729 normal drawn before depth_rand
    "cost_array_zero",     # :805 as {0.0f}
    "gate_no_margin",      # :1164 without - 0.1f
)


# ---------------------------------------------------------------- primitives
def _mathv(name, x):
    """oracle.math_fn over an array (float32 in, float32 out)."""
    x = np.asarray(x, F)
    flat = x.ravel().tolist()
    out = np.array([oracle.math_fn(name, v) for v in flat], F)
    return out.reshape(x.shape)


def cost_threshold(it):
    """:1011  float cost_threshold = 0.8 * expf(iter * iter / -90.0f)"""
    e = oracle.math_fn("expf", float(F(it * it) / F(-90.0)))
    return F(0.8 * e)  # double product, rounded once to float


def sweep_rows(height):
    """Rows the checkerboard grid covers (:1399, :1178-1182): grid.y blocks of
    16 threads, each thread one row pair."""
    return min(height, 32 * ((height // 2 + 15) // 16))


def _room(d, ys, xs, H, W):
    return {"up": ys, "down": H - 1 - ys, "left": xs, "right": W - 1 - xs}[d]


def sampling_table(variant=None):
    """The eight regions of :813-991 as data. Each region: its flag guard
    (direction, k): room > k; how it picks; and its samples in scan order as
    (dy, dx, guards). The first sample is the start value (:817, :893 ...)."""
    strip = 10 if variant == "strip10" else 11
    table = []
    for name in REGIONS:
        d, kind = name.split("_")
        uy, ux = _DIR[d]
        if kind == "far":
            # :814-828: start at 3 steps, then 3 + 2i while room > 2 + 2i
            flag = (d, 2)
            samples = [(3 * uy, 3 * ux, ())]
            for i in range(1, strip):
                samples.append(((3 + 2 * i) * uy, (3 + 2 * i) * ux, ((d, 2 + 2 * i),)))
        else:
            # :890-911: start at 1 step; arms (2 + i) steps out and i sideways,
            # first the left/up arm, then the right/down one; i = 0 names the
            # same pixel twice
            flag = (d, 0)
            sides = ("left", "right") if d in ("up", "down") else ("up", "down")
            samples = [(uy, ux, ())]
            for i in range(3):
                for s in sides:
                    vy, vx = _DIR[s]
                    samples.append(((2 + i) * uy + i * vy, (2 + i) * ux + i * vx, ((d, 1 + i), (s, i))))
        pick = "max" if (name == "right_far" and variant != "right_far_min") else "min"  # :879
        table.append({"name": name, "flag": flag, "pick": pick, "samples": samples})
    return table


def region_samples(table, r, y, x, H, W):
    """Positions region r reads for pixel (x, y), in scan order, duplicates
    included; [] when the region is absent."""
    reg = table[r]
    ys, xs = np.array([y]), np.array([x])
    d, k = reg["flag"]
    if not _room(d, ys, xs, H, W)[0] > k:
        return []
    out = []
    for dy, dx, guards in reg["samples"]:
        if all(_room(g, ys, xs, H, W)[0] > gk for g, gk in guards):
            out.append((y + dy, x + dx))
    return out


def choose_candidates(table, costs, ys, xs, costs_v=None):
    """:813-991 for the pixels (ys, xs): per region the flag and the position
    picked. `costs_v`: where the V samples are read (default: `costs`).
    Returns flag (P, 8) bool, pos_y, pos_x (P, 8) int, from_v (P, 8) bool."""
    H, W = costs.shape
    if costs_v is None:
        costs_v = costs
    P = len(ys)
    flag = np.zeros((P, 8), bool)
    pos_y = np.tile(ys[:, None], (1, 8))
    pos_x = np.tile(xs[:, None], (1, 8))
    from_v = np.zeros((P, 8), bool)
    with np.errstate(invalid="ignore"):
        for r, reg in enumerate(table):
            d, k = reg["flag"]
            fl = _room(d, ys, xs, H, W) > k
            flag[:, r] = fl
            cur = None
            for s, (dy, dx, guards) in enumerate(reg["samples"]):
                ok = fl.copy()
                for g, gk in guards:
                    ok &= _room(g, ys, xs, H, W) > gk
                py = np.where(ok, ys + dy, ys)
                px = np.where(ok, xs + dx, xs)
                is_v = s > 0 and reg["name"].endswith("near")
                c = (costs_v if is_v else costs)[py, px]
                if s == 0:
                    cur = np.where(fl, c, F(0))
                    better = fl
                elif reg["pick"] == "min":
                    better = ok & (c < cur)
                else:
                    better = ok & (cur < c)   # :879, reversed
                cur = np.where(better, c, cur)
                pos_y[:, r] = np.where(better, py, pos_y[:, r])
                pos_x[:, r] = np.where(better, px, pos_x[:, r])
                from_v[:, r] = np.where(better, is_v, from_v[:, r])
    return flag, pos_y, pos_x, from_v


def select_views(cost_array, near_flags, near_views, it, draws, variant=None):
    """Multi-hypothesis joint view selection, :994-1056.
    cost_array (P, 8, V) as :805 leaves it; near_flags (P, 4) = flag[0, 2, 4, 6];
    near_views (P, 4) the selected_views of up, down, left, right;
    draws(k) -> (P,) the k-th uniform of each pixel.
    Returns dict(weights, mask, weight_norm, probs, cdf, branch, threshold);
    branch (P, V): 0 weighted mean (:1026), 1 threshold fallback (:1029),
    2 zero probability (count_false >= 3)."""
    P, _, V = cost_array.shape
    hit, miss = (F(0.1), F(0.9)) if variant == "vote_swapped" else (F(0.9), F(0.1))
    priors = np.zeros((P, V), F)
    for i in range(4):                                       # :998-1008
        bits = ((near_views[:, i, None] >> np.arange(V, dtype=np.uint32)[None, :]) & 1) == 1
        add = np.where(bits, hit, miss).astype(F)
        priors = np.where(near_flags[:, i, None], priors + add, priors)
    thr = cost_threshold(it)
    count = np.zeros((P, V), F)
    count_false = np.zeros((P, V), np.int32)
    tmpw = np.zeros((P, V), F)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for j in range(8):                                   # :1016-1024
            c = cost_array[:, j, :]
            below = c < thr
            e = np.zeros((P, V), F)
            if below.any():
                e[below] = _mathv("expf", (c[below] * c[below]) / F(-0.18))
            tmpw = np.where(below, tmpw + e, tmpw)
            count = np.where(below, count + F(1), count)
            count_false += (c > F(1.2))
        enough = (count >= 2) if variant == "count_ge2" else (count > 2)
        fallback = F(oracle.math_fn("expf", float((thr * thr) / F(-0.32))))
        mean = tmpw / np.where(count > 0, count, F(1))
        probs = np.where(enough & (count_false < 3), mean,
                         np.where(count_false < 3, fallback, F(0))).astype(F)
        branch = np.where(count_false >= 3, 2, np.where(enough, 0, 1))
        probs = probs * priors                               # :1031
        s = np.zeros(P, F)                                   # TransformPDFToCDF, :107-121
        for i in range(V):
            s = s + probs[:, i]
        inv = F(1) / s
        cdf = np.zeros((P, V), F)
        cum = np.zeros(P, F)
        for i in range(V):
            cum = cum + probs[:, i] * inv
            cdf[:, i] = cum
        weights = np.zeros((P, V), F)
        nsamples = 14 if variant == "samples14" else 15
        for k in range(nsamples):                            # :1035-1045
            u = draws(k)
            rp = u if variant == "no_epsilon" else (u - FLT_EPSILON)
            above = cdf > rp[:, None]
            first = above & (np.cumsum(above, axis=1) == 1)
            weights = weights + first.astype(F)
    mask = np.zeros(P, np.uint32)
    wn = np.zeros(P, F)
    for i in range(V):                                       # :1047-1056
        on = weights[:, i] > 0
        mask |= np.where(on, np.uint32(1) << np.uint32(i), np.uint32(0)).astype(np.uint32)
        wn = np.where(on, wn + weights[:, i], wn)
    return {"weights": weights, "mask": mask, "weight_norm": wn, "probs": probs, "cdf": cdf,
            "branch": branch, "threshold": thr, "nsamples": nsamples}


def fill_cost_array(flag, region_costs, variant=None):
    """:805 `float cost_array[8][32] = {2.0f}` sets [0][0] alone, the rest is
    0; a present region then writes all its views (:829 ...)."""
    P, _, V = region_costs.shape
    ca = np.zeros((P, 8, V), F)
    if variant != "cost_array_zero":
        ca[:, 0, 0] = F(2.0)
    return np.where(flag[:, :, None], region_costs, ca).astype(F)


def refinement_pairings(depth, normal, depth_rand, normal_rand, depth_pert, normal_pert):
    """:740-741: the five (depth, normal) hypotheses in order."""
    return [(depth_rand, normal), (depth, normal_rand), (depth_rand, normal_rand),
            (depth, normal_pert), (depth_pert, normal)]


# ------------------------------------------------------------- camera algebra
class _Cam:
    def __init__(self, cam):
        self.K = np.array(list(cam.K), F)
        self.R = np.array(list(cam.R), F)
        self.W, self.H = int(cam.width), int(cam.height)


def depth_from_plane(K, pl, ys, xs):
    """ComputeDepthfromPlaneHypothesis, :163-168."""
    xf, yf = xs.astype(F), ys.astype(F)
    with np.errstate(all="ignore"):
        den = ((xf - K[2]) * pl[..., 0] + (K[0] / K[4]) * (yf - K[5]) * pl[..., 1]) + K[0] * pl[..., 2]
        return (-pl[..., 3] * K[0]) / den


def _point(K, ys, xs, depth):
    """Get3DPoint, :123-128."""
    xf, yf = xs.astype(F), ys.astype(F)
    return (depth * (xf - K[2])) / K[0], (depth * (yf - K[5])) / K[4], depth


def distance_to_origin(K, ys, xs, depth, n):
    """GetDistance2Origin, :144-149."""
    with np.errstate(all="ignore"):
        X0, X1, X2 = _point(K, ys, xs, depth)
        return -((n[..., 0] * X0 + n[..., 1] * X1) + n[..., 2] * X2)


def _view_direction(K, ys, xs, depth):
    """GetViewDirection, :130-142."""
    with np.errstate(all="ignore"):
        X0, X1, X2 = _point(K, ys, xs, depth)
        norm = np.sqrt((X0 * X0 + X1 * X1) + X2 * X2)
        return np.stack([X0 / norm, X1 / norm, X2 / norm], -1)


def _dot3(a, b):
    """Vec3DotVec3, :93-96."""
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _normalize(n):
    """NormalizeVec3, :98-105, rsqrtf pinned to 1 / sqrt (A6)."""
    with np.errstate(all="ignore"):
        inv = F(1) / np.sqrt((n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2])
        return n * inv[..., None]


def perturbed_normal(K, ys, xs, normal, u1, u2, u3, perturbation):
    """GeneratePerturbedNormal, :198-233, from its three uniforms."""
    view = _view_direction(K, ys, xs, np.ones(len(ys), F))
    a1, a2, a3 = ((u - F(0.5)) * perturbation for u in (u1, u2, u3))
    s1, s2, s3 = (_mathv("sinf", a) for a in (a1, a2, a3))
    c1, c2, c3 = (_mathv("cosf", a) for a in (a1, a2, a3))
    R = [c2 * c3, c3 * s1 * s2 - c1 * s3, s1 * s3 + c1 * c3 * s2,
         c2 * s3, c1 * c3 + s1 * s2 * s3, c1 * s2 * s3 - c3 * s1,
         -s2, c2 * s1, c1 * c2]
    x, y, z = normal[..., 0], normal[..., 1], normal[..., 2]
    out = np.stack([(R[0] * x + R[1] * y) + R[2] * z, (R[3] * x + R[4] * y) + R[5] * z,
                    (R[6] * x + R[7] * y) + R[8] * z], -1).astype(F)
    with np.errstate(invalid="ignore"):
        back = _dot3(out, view) >= F(0)
    out = np.where(back[:, None], normal[..., :3], out)
    return _normalize(out)


# ------------------------------------------------------------------- backends
@dataclass
class Problem:
    prm: object
    cams: list
    images: list
    depths: list | None = None
    planes: np.ndarray | None = None
    costs: np.ndarray | None = None
    pre_costs: np.ndarray | None = None
    prior_planes: np.ndarray | None = None
    masks: np.ndarray | None = None
    scaled_planes: np.ndarray | None = None
    seed_planes: np.ndarray | None = None


class OracleBackend:
    """The pinned primitives from the CPU oracle's evaluation entry points."""

    def __init__(self, prob):
        self.p = prob

    def cost_vectors(self, planes):
        return oracle.eval_costs(self.p.prm, self.p.cams, self.p.images, planes)[0]

    def init_cost(self, planes):
        _, c, v = oracle.eval_costs(self.p.prm, self.p.cams, self.p.images, planes)
        return c, v

    def geom_costs(self, planes):
        return oracle.eval_geom_costs(self.p.prm, self.p.cams, self.p.images, self.p.depths, planes)


class EngineBackend:
    """The same primitives from an ACMMP engine that holds the problem's images
    (and depth maps): its eval_costs / eval_geom_costs kernels."""

    def __init__(self, eng):
        self.eng = eng

    def cost_vectors(self, planes):
        return self.eng.eval_costs(planes)[0]

    def init_cost(self, planes):
        _, c, v = self.eng.eval_costs(planes)
        return c, v

    def geom_costs(self, planes):
        return self.eng.eval_geom_costs(planes)


# ------------------------------------------------------------------ the chain
@dataclass
class Trace:
    """Per-pixel record of one half-sweep (pixels in (ys, xs) order)."""
    it: int
    colour: int
    ys: np.ndarray
    xs: np.ndarray
    flags: np.ndarray = None         # (P, 8)
    pos_y: np.ndarray = None
    pos_x: np.ndarray = None
    weights: np.ndarray = None       # (P, V)
    branch: np.ndarray = None        # (P, V)
    region: np.ndarray = None        # accepted candidate region, -1 none
    planar_accept: np.ndarray = None  # posterior accept (:1129), the shadowed depth_now path
    plain_accept: np.ndarray = None   # mask 0 accept under planar_prior (:1141)
    shadowed: np.ndarray = None       # posterior accept whose depth_now stayed the old plane's (:1119, :1130)
    hyp_accepted: np.ndarray = None  # (P, 5) which hypotheses were accepted, in order
    gate: np.ndarray = None          # hierarchy: 1 passed, 0 blocked, -1 no gate
    draws: np.ndarray = None         # uniforms consumed
    extra: dict = field(default_factory=dict)


class SweepRestated:
    def __init__(self, prob, backend, variant=None):
        assert variant is None or variant in VARIANTS, variant
        self.p, self.be, self.variant = prob, backend, variant
        self.prm = prob.prm
        self.cam = _Cam(prob.cams[0])
        self.W, self.H = self.cam.W, self.cam.H
        self.V = len(prob.cams) - 1
        self.table = sampling_table(variant)
        self.traces = []
        H, W = self.H, self.W
        z = lambda a, shape, dt: np.zeros(shape, dt) if a is None else np.array(a, dt, copy=True).reshape(shape)
        self.planes = z(prob.planes, (H, W, 4), F)
        self.costs = z(prob.costs, (H, W), F)
        self.pre_costs = z(prob.pre_costs, (H, W), F)
        self.sv = np.zeros((H, W), np.uint32)
        self.dmin, self.dmax = F(self.prm.depth_min), F(self.prm.depth_max)

    # -- RNG (pin A1)
    def _uniform(self, pix, draw, phase):
        prm = self.prm
        return np.array([oracle.uniform(prm.seed_lo, prm.seed_hi, int(p), int(d), phase, prm.rng_stream)
                         for p, d in zip(pix.tolist(), draw.tolist())], F)

    class _Rng:
        def __init__(self, outer, pix, phase):
            self.o, self.pix, self.phase = outer, pix, phase
            self.draw = np.zeros(len(pix), np.int64)

        def next(self, sel=None):
            """The next uniform of every pixel (of those in `sel`)."""
            if sel is None:
                sel = np.ones(len(self.pix), bool)
            u = np.zeros(len(self.pix), F)
            u[sel] = self.o._uniform(self.pix[sel], self.draw[sel], self.phase)
            self.draw[sel] += 1
            return u

    def random_normal(self, rng, ys, xs, depth, sel=None):
        """GenerateRandomNormal, :170-196: the rejection loop draws pairs until
        q1^2 + q2^2 < 1."""
        P = len(ys)
        q1, q2 = np.ones(P, F), np.ones(P, F)
        s = np.full(P, 2.0, F)
        pending = np.ones(P, bool) if sel is None else sel.copy()
        while pending.any():
            a = F(2) * rng.next(pending) - F(1)
            b = F(2) * rng.next(pending) - F(1)
            q1 = np.where(pending, a, q1)
            q2 = np.where(pending, b, q2)
            s = np.where(pending, q1 * q1 + q2 * q2, s)
            pending &= s >= F(1)
        with np.errstate(all="ignore"):
            sq = np.sqrt(F(1) - s)
            n = np.stack([F(2) * q1 * sq, F(2) * q2 * sq, F(1) - F(2) * s], -1).astype(F)
            view = _view_direction(self.cam.K, ys, xs, depth)
            n = np.where((_dot3(n, view) > F(0))[:, None], -n, n)
        return _normalize(n)

    # -- RandomInitialization, :609-705
    def init(self):
        prm, K, Rm = self.prm, self.cam.K, self.cam.R
        H, W = self.H, self.W
        ys, xs = (a.ravel() for a in np.mgrid[0:H, 0:W])
        rng = self._Rng(self, ys * W + xs, 0)
        pl = self.planes.reshape(-1, 4)

        def to_ref_cam(h):  # TransformNormal2RefCam, :343-351
            return np.stack([(Rm[0] * h[:, 0] + Rm[1] * h[:, 1]) + Rm[2] * h[:, 2],
                             (Rm[3] * h[:, 0] + Rm[4] * h[:, 1]) + Rm[5] * h[:, 2],
                             (Rm[6] * h[:, 0] + Rm[7] * h[:, 1]) + Rm[8] * h[:, 2], h[:, 3]], -1).astype(F)

        if not prm.geom_consistency and not prm.hierarchy and not prm.seeded:      # :626
            depth = rng.next() * (self.dmax - self.dmin) + self.dmin               # :237
            n = self.random_normal(rng, ys, xs, depth)
            new = np.concatenate([n, distance_to_origin(K, ys, xs, depth, n)[:, None]], -1)
            self.branch_init = np.zeros(H * W, np.int8)
        elif prm.seeded:                                                            # :634
            new = np.array(self.p.seed_planes, F).reshape(-1, 4).copy()
            self.branch_init = np.full(H * W, 1, np.int8)
        elif prm.planar_prior:                                                      # :640
            masks = np.asarray(self.p.masks).reshape(-1)
            prior = np.asarray(self.p.prior_planes, F).reshape(-1, 4)
            pert = (masks > 0) & (self.costs.reshape(-1) >= F(0.1))                 # :641
            p3 = F(3) * F(0.02)
            dp = prior[:, 3]
            lo, hi = (F(1) - p3) * dp, (F(1) + p3) * dp                             # :646-647
            d = rng.next(pert) * (hi - lo) + lo                                     # :648
            u1, u2, u3 = rng.next(pert), rng.next(pert), rng.next(pert)
            ang = F(float(p3) * math.pi)                                            # :649, double product
            n = perturbed_normal(K, ys, xs, prior, u1, u2, u3, ang)
            a = np.concatenate([n, d[:, None]], -1)                                 # :650, .w a depth
            b = pl.copy()                                                           # :655-658
            b[:, 3] = distance_to_origin(K, ys, xs, pl[:, 3], pl)
            new = np.where(pert[:, None], a, b)
            self.branch_init = np.where(pert, 2, 3).astype(np.int8)
        elif prm.upsample:                                                          # :663
            n_total = self._upscale_normal(ys, xs)
            c, v = self.be.init_cost(self.planes)                                   # :680, the incoming planes
            self.pre_costs = c.copy()                                               # :681
            h = to_ref_cam(np.concatenate([n_total, np.zeros((H * W, 1), F)], -1))  # :683-684
            h[:, 3] = distance_to_origin(K, ys, xs, pl[:, 3], h)                    # :685-686
            new = h
            self.branch_init = np.full(H * W, 4, np.int8)
        else:                                                                       # :690-703
            src = np.asarray(self.p.scaled_planes, F).reshape(-1, 4)[:H * W] if prm.hierarchy else pl
            h = to_ref_cam(src)
            h[:, 3] = distance_to_origin(K, ys, xs, h[:, 3], h)
            new = h
            self.branch_init = np.full(H * W, 5, np.int8)
        self.planes = np.ascontiguousarray(new, F).reshape(H, W, 4)
        self.costs, self.sv = self.be.init_cost(self.planes)
        self.costs, self.sv = self.costs.copy(), self.sv.copy()

    def _upscale_normal(self, ys, xs):
        """upscale_normal, :548-607, with :664-673; SpatialGauss / RangeGauss
        :151-161 (pow(v, 2) as v * v and the double `-1.0 *` kept, A6)."""
        prm, H, W = self.prm, self.H, self.W
        sc, sr = F(prm.scaled_cols), F(prm.scaled_rows)
        scaled = np.asarray(self.p.scaled_planes, F).reshape(-1, 4)
        img = np.asarray(self.p.images[0], F)
        scale = F(1.0 * float(sc) / W)                                              # :664
        sigmad, sigmar = F(0.50), F(25.5)
        image_scale = int(max(F(W) / sc, F(H) / sr))                                # :667
        nn = (image_scale * image_scale + 1) // 2                                   # :668-669
        o_y, o_x = ys.astype(F) * scale, xs.astype(F) * scale
        ref_pix = img[ys, xs]

        def gauss(sq, sigma):  # exp(-1.0 * sq / (2 * sigma * sigma)) in double, expf of its float
            den = float(F(2) * sigma * sigma)
            return _mathv("expf", (-1.0 * sq.astype(np.float64) / den).astype(F))

        P = len(ys)
        norm, c_total = np.zeros(P, F), np.zeros(P, F)
        nt = np.zeros((P, 3), F)
        for j in range(-nn, nn + 1):
            r_y = (o_y + F(j)).astype(np.int32)                                     # :574
            r_y = np.where(r_y > 0, np.where(r_y.astype(F) < sr, r_y, int(sr - F(1))), 0)
            r_ys = np.clip(ys + j, 0, H - 1)                                        # clamp-to-edge texel
            for i in range(-nn, nn + 1):
                r_x = (o_x + F(i)).astype(np.int32)
                r_x = np.where(r_x > 0, np.where(r_x.astype(F) < sc, r_x, int(sc - F(1))), 0)
                s_center = (r_y.astype(F) * sc + r_x.astype(F)).astype(np.int64)    # :582
                src = scaled[s_center]
                nb = img[r_ys, np.clip(xs + i, 0, W - 1)]
                dx, dy = o_x - r_x.astype(F), o_y - r_y.astype(F)
                sg = gauss(dx * dx + dy * dy - F(0), sigmad)
                xp = np.abs(ref_pix - nb) - F(0)
                rg = gauss(xp * xp, sigmar)
                tg = sg * rg
                norm = norm + tg
                c_total = c_total + src[:, 3] * tg
                nt = nt + src[:, :3] * tg[:, None]
        with np.errstate(all="ignore"):
            self.costs = (c_total / norm).reshape(H, W)                             # :603 (overwritten at :680)
            nt = nt / norm[:, None]
        return _normalize(nt)

    # -- weighted costs, :1058-1076 / :749-760
    def _weighted(self, weights, wn, cv, geom, only_selected=True, unflagged=None):
        P, V = weights.shape
        acc = np.zeros(P, F)
        with np.errstate(all="ignore"):
            for j in range(V):
                term = cv[:, j]
                if geom is not None:
                    g = term + F(0.2) * geom[:, j]
                    if unflagged is not None:
                        g = np.where(unflagged, term + F(0.1) * F(3.0), g)          # :1067
                    term = g
                add = acc + weights[:, j] * term
                acc = np.where(weights[:, j] > 0, add, acc) if only_selected else add
            return acc / wn

    def _eval(self, ys, xs, cand, geom):
        """Cost vectors (and geometric costs) of candidate planes `cand` (P, 4)
        at the pixels (ys, xs): gathered into a plane map, one whole-image call."""
        m = self.planes.copy()
        m[ys, xs] = cand
        cv = self.be.cost_vectors(m)[ys, xs]
        gv = self.be.geom_costs(m)[ys, xs] if geom else None
        return cv, gv

    def _posterior(self, cost, depth, plane, prior, depth_prior):
        """:1108-1113 / :764-768"""
        rng = self.dmax - self.dmin
        depth_sigma = rng / F(64.0)
        two_ds = F(2) * depth_sigma * depth_sigma
        angle_sigma = F(math.pi * float(F(5.0) / F(180.0)))                         # :715, double product
        two_as = F(2) * angle_sigma * angle_sigma
        with np.errstate(all="ignore"):
            dd = depth - depth_prior
            ad = _mathv("acosf", _dot3(prior, plane))
            pr = F(0.5) + _mathv("expf", -dd * dd / two_ds) * _mathv("expf", -ad * ad / two_as)
            return _mathv("expf", -cost * cost / F(0.18)) * pr

    # -- CheckerboardPropagation, :786-1173, for the pixels (ys, xs)
    def _update(self, it, colour, ys, xs, snap_planes, snap_costs, v_planes, v_costs):
        prm, K, V = self.prm, self.cam.K, self.V
        geom = bool(prm.geom_consistency)
        P = len(ys)
        tr = Trace(it, colour, ys, xs)
        rng = self._Rng(self, ys * self.W + xs, 1 + it)
        flag, py, px, from_v = choose_candidates(self.table, snap_costs, ys, xs, v_costs)
        cand = np.where(from_v[..., None], v_planes[py, px], snap_planes[py, px])   # (P, 8, 4)
        own = self.planes[ys, xs]
        cvs = np.zeros((P, 8, V), F)
        gc = np.zeros((P, 8, V), F)
        for r in range(8):
            cv, gv = self._eval(ys, xs, np.where(flag[:, r, None], cand[:, r], own), geom)
            cvs[:, r, :] = cv
            if geom:
                gc[:, r, :] = gv
        ca = fill_cost_array(flag, cvs, self.variant)
        # view selection
        H, W = self.H, self.W
        nb = [(np.clip(ys - 1, 0, H - 1), xs), (np.clip(ys + 1, 0, H - 1), xs),
              (ys, np.clip(xs - 1, 0, W - 1)), (ys, np.clip(xs + 1, 0, W - 1))]     # :997
        near_views = np.stack([self.sv[a, b] for a, b in nb], 1)
        sel = select_views(ca, flag[:, [0, 2, 4, 6]], near_views, it, lambda k: rng.next(), self.variant)
        w, wn, tmask = sel["weights"], sel["weight_norm"], sel["mask"]
        final = np.stack([self._weighted(w, wn, ca[:, r], gc[:, r] if geom else None,
                                         unflagged=~flag[:, r] if geom else None) for r in range(8)], 1)
        with np.errstate(invalid="ignore"):
            best = np.zeros(P, np.int64)                                            # FindMinCostIndex, :50-61
            bc = final[:, 0].copy()
            for r in range(1, 8):
                le = final[:, r] <= bc
                bc = np.where(le, final[:, r], bc)
                best = np.where(le, r, best)
        cv_now, gv_now = self._eval(ys, xs, own, geom)
        cost_now = self._weighted(w, wn, cv_now, gv_now, only_selected=False)       # :1082-1091
        new_cost = cost_now.copy()                                                  # :1092
        new_plane = own.copy()
        new_sv = self.sv[ys, xs].copy()
        depth_now = depth_from_plane(K, own, ys, xs)                                # :1093
        restricted = np.zeros(P, F)
        ar = np.arange(P)
        region = np.full(P, -1, np.int64)
        planar_accept = np.zeros(P, bool)
        plain_accept = np.zeros(P, bool)
        has_prior = np.zeros(P, bool)
        shadowed = np.zeros(P, bool)
        prior = depth_prior = None
        with np.errstate(invalid="ignore"):
            in_range = lambda d: (d >= self.dmin) & (d <= self.dmax)
            if prm.planar_prior:                                                    # :1095-1147
                prior = np.asarray(self.p.prior_planes, F)[ys, xs]
                has_prior = np.asarray(self.p.masks)[ys, xs] > 0
                depth_prior = depth_from_plane(K, prior, ys, xs)
                rf = np.zeros((P, 8), F)
                for r in range(8):
                    d_r = depth_from_plane(K, cand[:, r], ys, xs)
                    post = self._posterior(final[:, r], d_r, cand[:, r], prior, depth_prior)
                    rf[:, r] = np.where(flag[:, r] & has_prior, post, F(0))
                bmax = np.zeros(P, np.int64)                                        # FindMaxCostIndex, :63-74
                bv = rf[:, 0].copy()
                for r in range(1, 8):
                    ge = rf[:, r] >= bv
                    bv = np.where(ge, rf[:, r], bv)
                    bmax = np.where(ge, r, bmax)
                r_now = self._posterior(cost_now, depth_now, own, prior, depth_prior)   # :1118-1124
                d_before = depth_from_plane(K, cand[ar, bmax], ys, xs)
                planar_accept = has_prior & flag[ar, bmax] & in_range(d_before) & (rf[ar, bmax] > r_now)
                shadowed = planar_accept & (d_before != depth_now)
                # :1130 assigns the inner, shadowing depth_now: the outer one keeps the old plane's depth
                new_plane = np.where(planar_accept[:, None], cand[ar, bmax], new_plane)
                new_cost = np.where(planar_accept, final[ar, bmax], new_cost)
                restricted = np.where(planar_accept, rf[ar, bmax], restricted)
                new_sv = np.where(planar_accept, tmask, new_sv)
                d_before = depth_from_plane(K, cand[ar, best], ys, xs)              # :1138-1146
                plain_accept = ~has_prior & flag[ar, best] & in_range(d_before) & (final[ar, best] < cost_now)
                depth_now = np.where(plain_accept, d_before, depth_now)
                new_plane = np.where(plain_accept[:, None], cand[ar, best], new_plane)
                new_cost = np.where(plain_accept, final[ar, best], new_cost)
                region = np.where(planar_accept, bmax, np.where(plain_accept, best, -1))
            plane_now = new_plane.copy()                                            # :1149, pin A3
            if not prm.planar_prior:                                                # :1150-1159
                d_before = depth_from_plane(K, cand[ar, best], ys, xs)
                acc = flag[ar, best] & in_range(d_before) & (final[ar, best] < cost_now)
                depth_now = np.where(acc, d_before, depth_now)
                plane_now = np.where(acc[:, None], cand[ar, best], plane_now)
                cost_now = np.where(acc, final[ar, best], cost_now)
                new_sv = np.where(acc, tmask, new_sv)
                region = np.where(acc, best, -1)
        tr.extra["depth_into_refinement"] = depth_now.copy()
        plane_now, cost_now, hyp = self._refine(rng, ys, xs, plane_now, depth_now, cost_now, w, wn, restricted,
                                                has_prior, prior, depth_prior, geom)
        gate = np.full(P, -1, np.int8)
        if prm.hierarchy:                                                           # :1163-1168
            margin = F(0) if self.variant == "gate_no_margin" else F(0.1)
            with np.errstate(invalid="ignore"):
                ok = cost_now < self.pre_costs[ys, xs] - margin
            new_cost = np.where(ok, cost_now, new_cost)
            new_plane = np.where(ok[:, None], plane_now, new_plane)
            gate = ok.astype(np.int8)
        else:
            new_cost, new_plane = cost_now, plane_now
        tr.flags, tr.pos_y, tr.pos_x = flag, py, px
        tr.weights, tr.branch = w, sel["branch"]
        tr.extra["cdf"] = sel["cdf"]
        tr.extra.update(self._last_refine)
        tr.shadowed = shadowed
        tr.region, tr.planar_accept, tr.plain_accept = region, planar_accept, plain_accept
        tr.hyp_accepted, tr.gate, tr.draws = hyp, gate, rng.draw.copy()
        self.traces.append(tr)
        return new_plane.astype(F), new_cost.astype(F), new_sv.astype(np.uint32)

    # -- PlaneHypothesisRefinement, :707-784
    def _refine(self, rng, ys, xs, plane, depth, cost, w, wn, restricted, has_prior, prior, depth_prior, geom):
        K = self.cam.K
        P = len(ys)
        pert = F(0.02)
        depth_sigma = (self.dmax - self.dmin) / F(64.0)
        angle_sigma = F(math.pi * float(F(5.0) / F(180.0)))
        swapped = self.variant == "refine_draws_swapped"
        free = ~has_prior
        with np.errstate(all="ignore"):
            depth_rand = np.zeros(P, F)
            normal_rand = np.zeros((P, 3), F)
            if has_prior.any():                                                     # :722-726
                u = rng.next(has_prior)
                dr = u * F(6) * depth_sigma + (depth_prior - F(3) * depth_sigma)
                u1, u2, u3 = rng.next(has_prior), rng.next(has_prior), rng.next(has_prior)
                nr = perturbed_normal(K, ys, xs, prior, u1, u2, u3, angle_sigma)
                depth_rand = np.where(has_prior, dr, depth_rand)
                normal_rand = np.where(has_prior[:, None], nr, normal_rand)
            if free.any():                                                          # :727-730
                if swapped:
                    nr = self.random_normal(rng, ys, xs, depth, free)
                    u = rng.next(free)
                else:
                    u = rng.next(free)
                    nr = self.random_normal(rng, ys, xs, depth, free)
                dr = u * (self.dmax - self.dmin) + self.dmin
                depth_rand = np.where(free, dr, depth_rand)
                normal_rand = np.where(free[:, None], nr, normal_rand)
            lo, hi = (F(1) - pert) * depth, (F(1) + pert) * depth                   # :731-736, one pass
            depth_pert = rng.next() * (hi - lo) + lo
            u1, u2, u3 = rng.next(), rng.next(), rng.next()
            normal_pert = perturbed_normal(K, ys, xs, plane, u1, u2, u3, F(float(pert) * math.pi))  # :737
            hyps = refinement_pairings(depth, plane[:, :3], depth_rand, normal_rand, depth_pert, normal_pert)
            accepted = np.zeros((P, 5), bool)
            self._last_refine = {"hyp_depth": np.stack([np.broadcast_to(d, (P,)) for d, _ in hyps], 1),
                                 "hyp_cost": np.zeros((P, 5), F), "restricted_in": restricted.copy()}
            plane, depth, cost, restricted = plane.copy(), depth.copy(), cost.copy(), restricted.copy()
            for i, (d_i, n_i) in enumerate(hyps):                                   # :743-783
                temp = np.concatenate([n_i, distance_to_origin(K, ys, xs, d_i, n_i)[:, None]], -1).astype(F)
                cv, gv = self._eval(ys, xs, temp, geom)
                tc = self._weighted(w, wn, cv, gv)
                self._last_refine["hyp_cost"][:, i] = tc
                d_before = depth_from_plane(K, temp, ys, xs)
                ok = (d_before >= self.dmin) & (d_before <= self.dmax)
                if has_prior.any():
                    rt = self._posterior(tc, d_i, temp, prior, depth_prior)
                    a_prior = has_prior & ok & (rt > restricted)
                    restricted = np.where(a_prior, rt, restricted)
                else:
                    a_prior = np.zeros(P, bool)
                acc = a_prior | (free & ok & (tc < cost))
                depth = np.where(acc, d_before, depth)
                plane = np.where(acc[:, None], temp, plane)
                cost = np.where(acc, tc, cost)
                accepted[:, i] = acc
        return plane, cost, accepted

    def half_sweep(self, it, colour):
        H, W = self.H, self.W
        rows = sweep_rows(H)
        yy, xx = np.mgrid[0:H, 0:W]
        todo = ((yy + xx) % 2 == colour) & (yy < rows)      # :1178-1182 black, :1190-1194 red
        snap_p, snap_c = self.planes.copy(), self.costs.copy()                      # pin A2
        if self.variant == "v_live":
            for y in range(rows):
                ys, xs = np.nonzero(todo & (yy == y))
                pl, co, sv = self._update(it, colour, ys, xs, snap_p, snap_c, self.planes.copy(), self.costs.copy())
                self.planes[ys, xs], self.costs[ys, xs], self.sv[ys, xs] = pl, co, sv
            return
        ys, xs = np.nonzero(todo)
        pl, co, sv = self._update(it, colour, ys, xs, snap_p, snap_c, snap_p, snap_c)
        self.planes[ys, xs], self.costs[ys, xs], self.sv[ys, xs] = pl, co, sv

    # -- GetDepthandNormal :1199-1212, filters :1214-1352
    def finalize(self):
        K, Rm, H, W = self.cam.K, self.cam.R, self.H, self.W
        ys, xs = (a.ravel() for a in np.mgrid[0:H, 0:W])
        h = self.planes.reshape(-1, 4).copy()
        h[:, 3] = depth_from_plane(K, h, ys, xs)
        with np.errstate(all="ignore"):
            out = np.stack([(Rm[0] * h[:, 0] + Rm[3] * h[:, 1]) + Rm[6] * h[:, 2],   # TransformNormal, :333-341
                            (Rm[1] * h[:, 0] + Rm[4] * h[:, 1]) + Rm[7] * h[:, 2],
                            (Rm[2] * h[:, 0] + Rm[5] * h[:, 1]) + Rm[8] * h[:, 2], h[:, 3]], -1).astype(F)
        self.planes = out.reshape(H, W, 4)
        for colour in (0, 1):
            self._filter(colour)

    # (dy, dx, guards) in the order of :1249-1319
    FILTER = [(-1, 0, (("up", 0),)), (-3, 0, (("up", 2),)), (-5, 0, (("up", 4),)),
              (1, 0, (("down", 0),)), (3, 0, (("down", 2),)), (5, 0, (("down", 4),)),
              (0, -1, (("left", 0),)), (0, -3, (("left", 2),)), (0, -5, (("left", 4),)),
              (0, 1, (("right", 0),)), (0, 3, (("right", 2),)), (0, 5, (("right", 4),)),
              (-1, 2, (("up", 0), ("right", 1))), (1, 2, (("down", 0), ("right", 1))),
              (-1, -2, (("up", 0), ("left", 1))), (1, -2, (("down", 0), ("left", 1))),
              (-2, -1, (("left", 0), ("up", 2))), (-2, 1, (("right", 0), ("up", 2))),
              (2, -1, (("left", 0), ("down", 1))), (2, 1, (("right", 0), ("down", 1)))]

    def _filter(self, colour):
        H, W = self.H, self.W
        rows = sweep_rows(H)
        depth = self.planes[..., 3]
        new = depth.copy()
        for y in range(rows):
            for x in range((y + colour) % 2, W, 2):
                if self.costs[y, x] < F(0.001):                                     # :1245
                    continue
                vals = [float(depth[y, x])]
                one = np.array([0])
                for dy, dx, guards in self.FILTER:
                    if all(_room(g, one + y, one + x, H, W)[0] > k for g, k in guards):
                        vals.append(float(depth[y + dy, x + dx]))
                for i in range(1, len(vals)):                                       # sort_small, :24-33
                    tmp, j = vals[i], i
                    while j >= 1 and tmp < vals[j - 1]:
                        vals[j] = vals[j - 1]
                        j -= 1
                    vals[j] = tmp
                m = len(vals) // 2
                new[y, x] = (F(vals[m - 1]) + F(vals[m])) / F(2) if len(vals) % 2 == 0 else F(vals[m])
        self.planes[..., 3] = new

    def run(self):
        self.init()
        for it in range(self.prm.max_iterations):
            self.half_sweep(it, 0)
            self.half_sweep(it, 1)
        self.finalize()
        return {"planes": self.planes, "costs": self.costs, "selected_views": self.sv,
                "pre_costs": self.pre_costs, "traces": self.traces}


def run_restated(prob, backend=None, variant=None):
    r = SweepRestated(prob, backend or OracleBackend(prob), variant)
    out = r.run()
    out["restated"] = r
    return out


def run_oracle(prob):
    p = prob
    return oracle.run_patchmatch(p.prm, p.cams, p.images, depths=p.depths, planes=p.planes, costs=p.costs,
                                 pre_costs=p.pre_costs, prior_planes=p.prior_planes, masks=p.masks,
                                 scaled_planes=p.scaled_planes, seed_planes=p.seed_planes)


# ------------------------------------------------------------------ coverage
def coverage(traces):
    """Shares the cases assert on, from the per-pixel traces of a run."""
    P = sum(len(t.ys) for t in traces)
    region = np.concatenate([t.region for t in traces])
    hyp = np.concatenate([t.hyp_accepted for t in traces])
    branch = np.concatenate([t.branch.ravel() for t in traces])
    gate = np.concatenate([t.gate for t in traces])
    return {
        "pixels": P,
        "region": [float((region == r).sum()) / P for r in range(8)],
        "none": float((region < 0).sum()) / P,
        "hyp": [float(hyp[:, i].sum()) / P for i in range(5)],
        "branch": [float((branch == b).sum()) / branch.size for b in range(3)],
        "planar_accept": float(np.concatenate([t.planar_accept for t in traces]).sum()) / P,
        "plain_accept": float(np.concatenate([t.plain_accept for t in traces]).sum()) / P,
        "shadowed": float(np.concatenate([t.shadowed for t in traces]).sum()) / P,
        "gate_pass": float((gate == 1).sum()) / P,
        "gate_block": float((gate == 0).sum()) / P,
    }


# --------------------------------------------------------------------- cases
# Scenes of acmmp_amd.scene (consistent views of one surface) on a wide arc:
# at 25 degrees between views about half of the (pixel, view) pairs have three
# costs above 1.2 and the fallback branch is reached on more than 5 %.
ARC_DEG = 25.0


def _params(cams, iters, **kw):
    from acmmp_amd import default_params
    p = default_params()
    p.max_iterations = iters
    p.num_images = len(cams)
    # the host's depth range, src/ACMMP.cpp:600-601
    p.depth_min, p.depth_max = float(F(cams[0].depth_min) * F(0.6)), float(F(cams[0].depth_max) * F(1.2))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _truth(view, cam, rng, world, wild_share=0.9):
    """A noisy state around the analytic truth: (normal, depth) per pixel, the
    normal in the world frame (a previous pass's output) or the camera frame."""
    H, W = view.depth.shape
    R = np.array(list(cam.R), np.float64).reshape(3, 3)
    n = view.normal.astype(np.float64) + rng.normal(scale=0.15, size=(H, W, 3))
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    nc = n @ R.T
    n[nc[..., 2] > 0] *= -1
    depth = np.where(view.depth > 0, view.depth, 600.0) * (1 + rng.normal(scale=0.03, size=(H, W)))
    wild = rng.random((H, W)) < wild_share          # pixels far from the truth, as after a random init
    depth = np.where(wild, rng.uniform(cam.depth_min, cam.depth_max, (H, W)), depth)
    nw = rng.normal(size=(H, W, 3))
    nw /= np.linalg.norm(nw, axis=-1, keepdims=True)
    nw[(nw @ R.T)[..., 2] > 0] *= -1
    n = np.where(wild[..., None], nw, n)
    return np.concatenate([n if world else n @ R.T, depth[..., None]], -1).astype(F)


def _cam_plane(cam, nd):
    """(camera normal, depth) -> (camera normal, distance)."""
    H, W = nd.shape[:2]
    K = np.array(list(cam.K), np.float64).reshape(3, 3)
    ys, xs = np.mgrid[0:H, 0:W]
    z = nd[..., 3].astype(np.float64)
    X = np.stack([z * (xs - K[0, 2]) / K[0, 0], z * (ys - K[1, 2]) / K[1, 1], z], -1)
    out = nd.copy()
    out[..., 3] = -(nd[..., :3] * X).sum(-1)
    return out.astype(F)


# seeds at which every coverage condition of the CPU tests holds with a margin
CASE_SEEDS = {"geom": 1, "planar": 6, "hier_up": 8, "hier_swap": 6, "hier_seeded": 1}


def make_case(name, nsrc=3, seed=None, pre_costs=None, **prm_kw):
    """Problem of a named case (tests/test_sweep_restated_cpu.py lists them)."""
    from acmmp_amd import scene
    W, H, iters = {"photo": (53, 49, 2), "small37": (37, 33, 1), "small9": (9, 7, 1)}.get(name, (45, 33, 1))
    sc = scene.make_scene(num_views=nsrc + 1, width=W, height=H, arc_deg=ARC_DEG if nsrc <= 3 else 75.0 / nsrc)
    ref = 0
    cams, imgs = sc.problem(ref, nsrc)
    ids = [ref] + list(sc.pairs[ref][:nsrc])
    view = sc.views[ref]
    rng = np.random.default_rng(CASE_SEEDS.get(name, 7) if seed is None else seed)
    if name in ("photo", "small37", "small9", "photo45"):
        return Problem(_params(cams, iters, **prm_kw), cams, imgs)
    if name in ("geom", "planar"):
        depths = []
        for i in ids:                      # source depth maps with holes (:530)
            d = sc.views[i].depth.astype(F).copy()
            d[rng.random(d.shape) < 0.15] = 0.0
            depths.append(d)
        state = _truth(view, cams[0], rng, world=True)
        if name == "geom":
            # The init of this case draws nothing, so the CDFs of the first half-sweep do not depend
            # on the RNG key; with key 641 the second draw of pixel (x 6, y 12), 0.8515803, lies
            # within FLT_EPSILON above the CDF step 0.85158026: the one place where :1036's
            # `- FLT_EPSILON` picks another view (tools/find_epsilon_key.py finds such a key again
            # when these inputs change).
            prm_kw.setdefault("seed_lo", 641)
            return Problem(_params(cams, iters, geom_consistency=1, **prm_kw), cams, imgs, depths=depths,
                           planes=state, costs=rng.uniform(0, 1, (H, W)).astype(F))
        prior = _cam_plane(cams[0], _truth(view, cams[0], np.random.default_rng(8), world=False))
        masks = ((rng.random((H, W)) < 0.5) * (np.arange(H * W).reshape(H, W) + 1)).astype(np.uint32)
        prior = np.where(masks[..., None] > 0, prior, F(0)).astype(F)
        return Problem(_params(cams, iters, geom_consistency=1, planar_prior=1, **prm_kw), cams, imgs,
                       depths=depths, planes=state, costs=rng.uniform(0, 0.2, (H, W)).astype(F),
                       prior_planes=prior, masks=masks)
    up_depth = _truth(view, cams[0], rng, world=True)[..., 3]
    planes_in = np.zeros((H, W, 4), F)     # xyz never set on the host (src/ACMMP.cpp:797-804), pinned 0
    planes_in[..., 3] = up_depth
    if name == "hier_up":
        sh, sw = H // 2, W // 2
        low = _truth(view, cams[0], rng, world=True)[::2, ::2][:sh, :sw].copy()
        low[..., 3] = rng.uniform(0, 1, (sh, sw))          # .w a cost (src/ACMMP.cpp:785)
        prm = _params(cams, iters, hierarchy=1, upsample=1, scaled_cols=sw, scaled_rows=sh, **prm_kw)
        return Problem(prm, cams, imgs, planes=planes_in, pre_costs=np.zeros((H, W), F), scaled_planes=low)
    # same size through the rows/cols swap (src/ACMMP.cpp:766): a W-row, H-column map read flat
    scaled = _truth(view, cams[0], rng, world=True).reshape(W, H, 4)
    pre = rng.uniform(0.0, 1.2, (H, W)).astype(F)
    if pre_costs is not None:      # what an earlier pass left (an engine has no other pre_costs input)
        pre = np.array(pre_costs, F)
    if name == "hier_swap":
        prm = _params(cams, iters, hierarchy=1, upsample=0, **prm_kw)
        return Problem(prm, cams, imgs, planes=planes_in, pre_costs=pre, scaled_planes=scaled)
    seed = _cam_plane(cams[0], _truth(view, cams[0], rng, world=False))
    prm = _params(cams, iters, hierarchy=1, upsample=0, seeded=1, **prm_kw)
    return Problem(prm, cams, imgs, planes=planes_in, pre_costs=pre, scaled_planes=scaled, seed_planes=seed)
