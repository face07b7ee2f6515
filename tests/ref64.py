"""Float64 restatements of the reference's device and host formulas, written
from the reference lines (rlav440/ACMMP, src/ACMMP.cu and src/ACMMP.cpp), not
from oracle/ or the HIP kernels: the independent side of the known-answer
tests (test_oracle_kat.py, test_general_rig_cpu.py, test_gpu_general_rig.py).

Nothing here assumes anything about K beyond what the reference line itself
reads: projections use the full K rows (skew included, src/ACMMP.cu:506-516),
back-projections and the homography use K[0], K[2], K[4], K[5] only
(:123-128, :262-322, :480-487).
"""
from __future__ import annotations

import math

import numpy as np


def cam_np(cam):
    K = np.array(cam.K[:], np.float64).reshape(3, 3)
    R = np.array(cam.R[:], np.float64).reshape(3, 3)
    t = np.array(cam.t[:], np.float64)
    return K, R, t


def ref_homography(rc, sc, plane):
    """ComputeHomography, src/ACMMP.cu:262-322."""
    Kr, Rr, tr = cam_np(rc)
    Ks, Rs, ts = cam_np(sc)
    Cr = -Rr.T @ tr
    Cs = -Rs.T @ ts
    Rrel = Rs @ Rr.T
    trel = Rs @ (Cr - Cs)
    n = np.asarray(plane[:3], np.float64)
    H = Rrel - np.outer(trel, n) / plane[3]
    tmp = np.empty((3, 3))
    for r in range(3):
        tmp[r, 0] = H[r, 0] / Kr[0, 0]
        tmp[r, 1] = H[r, 1] / Kr[1, 1]
        tmp[r, 2] = -H[r, 0] * Kr[0, 2] / Kr[0, 0] - H[r, 1] * Kr[1, 2] / Kr[1, 1] + H[r, 2]
    out = np.empty((3, 3))
    # :313-321 read K[0], K[2], K[4], K[5] (and K[8]) of the source camera: no skew term
    out[0] = Ks[0, 0] * tmp[0] + Ks[0, 2] * tmp[2]
    out[1] = Ks[1, 1] * tmp[1] + Ks[1, 2] * tmp[2]
    out[2] = Ks[2, 2] * tmp[2]
    return out


def _tex_bilinear(img, x, y):
    """tex2D linear filtering with clamp-to-edge at (x, y) in texel-centre
    coordinates as passed by the reference (pt + 0.5)."""
    h, w = img.shape
    xs, ys = x - 0.5, y - 0.5
    x0, y0 = math.floor(xs), math.floor(ys)
    a, b = xs - x0, ys - y0

    def t(r, c):
        return float(img[min(max(r, 0), h - 1), min(max(c, 0), w - 1)])

    top = (1 - a) * t(y0, x0) + a * t(y0, x0 + 1)
    bot = (1 - a) * t(y0 + 1, x0) + a * t(y0 + 1, x0 + 1)
    return (1 - b) * top + b * bot


def _near_int(v, eps=1e-3):
    return abs(v - round(v)) < eps


def ref_ncc(prm, rc, sc, rimg, simg, px, py, plane, near=None):
    """ComputeBilateralNCC, src/ACMMP.cu:360-432 (float64). `near`, when a
    list, receives the name of every branch whose operand lies so close to its
    threshold that an fp32 evaluation may take the other side: the projected
    centre within 1e-3 px of a source border (:368), a variance within a
    factor 2 of kMinVar (:423)."""
    H = ref_homography(rc, sc, plane)

    def corr(x, y):
        v = H @ np.array([x, y, 1.0])
        return v[0] / v[2], v[1] / v[2]

    cx, cy = corr(px, py)
    if near is not None and (min(abs(cx), abs(cx - sc.width), abs(cy), abs(cy - sc.height)) < 1e-3):
        near.append("border")
    if cx >= sc.width or cx < 0 or cy >= sc.height or cy < 0:
        return 2.0
    radius = prm.patch_size // 2
    centre = float(rimg[py, px])
    sr = srr = ss = sss = srs = sw = 0.0
    for i in range(-radius, radius + 1, prm.radius_increment):
        for j in range(-radius, radius + 1, prm.radius_increment):
            rx, ry = px + i, py + j
            r = _tex_bilinear(rimg, rx + 0.5, ry + 0.5)
            ux, uy = corr(rx, ry)
            s = _tex_bilinear(simg, ux + 0.5, uy + 0.5)
            wgt = math.exp(-math.sqrt(i * i + j * j) / (2 * prm.sigma_spatial ** 2)
                           - abs(r - centre) / (2 * prm.sigma_color ** 2))
            sr += wgt * r
            srr += wgt * r * r
            ss += wgt * s
            sss += wgt * s * s
            srs += wgt * r * s
            sw += wgt
    sr, srr, ss, sss, srs = (v / sw for v in (sr, srr, ss, sss, srs))
    vr, vs = srr - sr * sr, sss - ss * ss
    if near is not None and any(0.5e-5 < v < 2e-5 for v in (vr, vs)):
        near.append("variance")
    if vr < 1e-5 or vs < 1e-5:
        return 2.0
    return max(0.0, min(2.0, 1.0 - (srs - sr * ss) / math.sqrt(vr * vs)))


def ref_depth_from_plane(cam, plane, x, y):
    """ComputeDepthfromPlaneHypothesis, src/ACMMP.cu:163-168, and the host's
    GetDepthFromPlaneParam, src/ACMMP.cpp:955-958 (the same expression).
    x, y may be arrays."""
    K, _, _ = cam_np(cam)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    pl = np.asarray(plane, np.float64)
    return -pl[..., 3] * fx / ((x - cx) * pl[..., 0] + (fx / fy) * (y - cy) * pl[..., 1] + fx * pl[..., 2])


def _to_world(K, R, t, x, y, d):
    """Get3DPointonWorld_cu, src/ACMMP.cu:480-504."""
    X = np.array([d * (x - K[0, 2]) / K[0, 0], d * (y - K[1, 2]) / K[1, 1], d])
    return R.T @ X - R.T @ t


def _project(K, R, t, X):
    """ProjectonCamera_cu, src/ACMMP.cu:506-516: the full K rows."""
    c = R @ X + t
    d = K[2] @ c
    return (K[0] @ c) / d, (K[1] @ c) / d


def ref_geom_cost(rc, sc, src_depth, plane, px, py, near=None):
    """ComputeGeomConsistencyCost, src/ACMMP.cu:518-543 (float64). `near`
    receives "trunc" when a source coordinate lies within 1e-3 of an integer,
    where the (int) of :528 may pick the neighbouring texel in fp32."""
    Kr, Rr, tr = cam_np(rc)
    Ks, Rs, ts = cam_np(sc)
    depth = float(ref_depth_from_plane(rc, np.asarray(plane, np.float64), px, py))
    X = _to_world(Kr, Rr, tr, px, py, depth)
    sx, sy = _project(Ks, Rs, ts, X)
    if near is not None and (_near_int(sx) or _near_int(sy)):
        near.append("trunc")
    hh, ww = src_depth.shape
    # tex2D(depth, (int)x + 0.5f, (int)y + 0.5f): truncation, clamp-to-edge
    ix = min(max(int(sx), 0), ww - 1)
    iy = min(max(int(sy), 0), hh - 1)
    d = float(src_depth[iy, ix])
    if d == 0.0:
        return 3.0
    Y = _to_world(Ks, Rs, ts, sx, sy, d)
    bx, by = _project(Kr, Rr, tr, Y)
    return min(3.0, math.hypot(px - bx, py - by))


def ref_roundtrip(cam, planes_world_depth):
    """The geom-branch init followed by GetDepthandNormal on an (H, W, 4) map
    of (world normal, depth): TransformNormal2RefCam (src/ACMMP.cu:343-351),
    GetDistance2Origin (:144-149, with Get3DPoint :123-128),
    ComputeDepthfromPlaneHypothesis (:163-168), TransformNormal (:333-341),
    as RandomInitialization's last branch (:696-701) and GetDepthandNormal
    (:1199-1212) chain them. The identity in exact arithmetic; returns the
    float64 (world normal, depth) the chain gives."""
    K, R, _ = cam_np(cam)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    pw = np.asarray(planes_world_depth, np.float64)
    H, W = pw.shape[:2]
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    n_cam = pw[..., :3] @ R.T  # :346-348: row r of R dot the normal
    depth = pw[..., 3]
    X = np.stack([depth * (xs - cx) / fx, depth * (ys - cy) / fy, depth], -1)
    dist = -(n_cam * X).sum(-1)
    depth_out = -dist * fx / ((xs - cx) * n_cam[..., 0] + (fx / fy) * (ys - cy) * n_cam[..., 1]
                              + fx * n_cam[..., 2])
    n_world = n_cam @ R  # :336-338: column c of R dot the normal
    return np.concatenate([n_world, depth_out[..., None]], -1)


def ref_checkerboard_rows(height):
    """Rows the checkerboard kernels reach: grid.y = ((height / 2) + 16 - 1) / 16
    blocks (src/ACMMP.cu:1397-1399) of 16 thread rows, each thread row covering
    image rows 2k and 2k + 1 (:1332-1337)."""
    grid_y = ((height // 2) + 16 - 1) // 16
    return min(height, grid_y * 16 * 2)


# CheckerboardFilter's taps after the centre, in the reference's order
# (src/ACMMP.cu:1249-1319): (dx, dy, condition on (x, y, width, height)).
_FILTER_TAPS = [
    (0, -1, lambda x, y, w, h: y > 0),
    (0, -3, lambda x, y, w, h: y > 2),
    (0, -5, lambda x, y, w, h: y > 4),
    (0, 1, lambda x, y, w, h: y < h - 1),
    (0, 3, lambda x, y, w, h: y < h - 3),
    (0, 5, lambda x, y, w, h: y < h - 5),
    (-1, 0, lambda x, y, w, h: x > 0),
    (-3, 0, lambda x, y, w, h: x > 2),
    (-5, 0, lambda x, y, w, h: x > 4),
    (1, 0, lambda x, y, w, h: x < w - 1),
    (3, 0, lambda x, y, w, h: x < w - 3),
    (5, 0, lambda x, y, w, h: x < w - 5),
    (2, -1, lambda x, y, w, h: y > 0 and x < w - 2),
    (2, 1, lambda x, y, w, h: y < h - 1 and x < w - 2),
    (-2, -1, lambda x, y, w, h: y > 0 and x > 1),
    (-2, 1, lambda x, y, w, h: y < h - 1 and x > 1),
    (-1, -2, lambda x, y, w, h: x > 0 and y > 2),
    (1, -2, lambda x, y, w, h: x < w - 1 and y > 2),
    (-1, 2, lambda x, y, w, h: x > 0 and y < h - 2),
    (1, 2, lambda x, y, w, h: x < w - 1 and y < h - 2),
]


def ref_filter(depth, cost, rows):
    """BlackPixelFilter then RedPixelFilter (src/ACMMP.cu:1214-1352), in
    place, over the first `rows` image rows (ref_checkerboard_rows): black is
    (x + y) even (:1333-1337 with a block width of 32), red is odd. A pixel
    whose fp32 cost is below 0.001f keeps its depth (:1245); the others take
    the median of the centre and the up to 20 taps the edge conditions admit,
    the mean of the two middle values when their count is even (:1321-1327).
    Returns float64."""
    d = np.array(depth, np.float64, copy=True)
    c = np.asarray(cost, np.float32)
    h, w = d.shape
    thr = np.float32(0.001)
    for colour in (0, 1):
        for y in range(min(rows, h)):
            for x in range((y + colour) & 1, w, 2):
                if c[y, x] < thr:
                    continue
                vals = [d[y, x]]
                for dx, dy, ok in _FILTER_TAPS:
                    if ok(x, y, w, h):
                        vals.append(d[y + dy, x + dx])
                vals.sort()
                m = len(vals) // 2
                d[y, x] = (vals[m - 1] + vals[m]) / 2 if len(vals) % 2 == 0 else vals[m]
    return d


def ref_jbu(img, depth):
    """JBU_cu (src/ACMMP.cu:1458-1516) with RunJBU's Imagescale
    (src/ACMMP.cpp:1030): None when Imagescale == 1. The tap indices
    (int)(o + j) are evaluated in float32 as written (:1472-1479, :1491,
    :1498); the Gaussians (:151-161) and the sums are float64."""
    img = np.asarray(img, np.float64)
    dep = np.asarray(depth, np.float64)
    H, W = img.shape
    sh, sw = dep.shape
    isc = max(H // sh, W // sw)
    if isc == 1:
        return None
    nn = (isc * isc + 1) // 2
    scale = np.float32(1.0 * sw / W)
    o_y = (np.arange(H, dtype=np.float32) * scale).astype(np.float32)
    o_x = (np.arange(W, dtype=np.float32) * scale).astype(np.float32)
    sigmad, sigmar = 0.5, 25.5
    total = np.zeros((H, W))
    norm = np.zeros((H, W))
    ys, xs = np.arange(H), np.arange(W)
    for j in range(-nn, nn + 1):
        r_y = np.clip((o_y + np.float32(j)).astype(np.float32).astype(np.int64), 0, sh - 1)  # trunc, then clamp
        r_ys = np.clip(ys + j, 0, H - 1)
        for i in range(-nn, nn + 1):
            r_x = np.clip((o_x + np.float32(i)).astype(np.float32).astype(np.int64), 0, sw - 1)
            r_xs = np.clip(xs + i, 0, W - 1)
            src = dep[r_y[:, None], r_x[None, :]]
            nb = img[r_ys[:, None], r_xs[None, :]]
            dis = (o_x.astype(np.float64)[None, :] - r_x[None, :]) ** 2 + \
                  (o_y.astype(np.float64)[:, None] - r_y[:, None]) ** 2
            sg = np.exp(-dis / (2 * sigmad * sigmad))
            rg = np.exp(-((img - nb) ** 2) / (2 * sigmar * sigmar))
            g = sg * rg
            norm += g
            total += src * g
    return total / norm


def ref_prior_plane(cam, tri, depths):
    """GetPriorPlaneParams, src/ACMMP.cpp:920-953: the plane (n, w) with
    n . X + w = 0 through the three corners (x1 y1 x2 y2 x3 y3) back-projected
    at depths[y, x] (Get3DPointonRefCam, :230-239), |n| = 1, signed so that
    w >= 0 (:943-950). Float64 from the given (float32) depths."""
    K, _, _ = cam_np(cam)
    P = []
    for k in range(3):
        x, y = int(tri[2 * k]), int(tri[2 * k + 1])
        d = float(depths[y, x])
        P.append(np.array([d * (x - K[0, 2]) / K[0, 0], d * (y - K[1, 2]) / K[1, 1], d]))
    n = np.cross(P[1] - P[0], P[2] - P[0])
    n /= np.linalg.norm(n)
    w = -float(n @ P[0])
    if w < 0:
        n, w = -n, -w
    return np.array([n[0], n[1], n[2], w])
