"""RunPriorAwareFusion in Jacobi order (acmmp_run_prior_aware_fusion_jacobi,
DESIGN.md §8) restated in numpy float32 — TEST INFRASTRUCTURE, the checker of
k_prior_test / k_prior_apply in acmmp_amd/csrc/acmmp_fusion_dev.hip.

The rule: RunPriorAwareFusion (src/acmmp_definitions.cpp:573-826) as
tests/oracle_fusion.py:run_prior_aware_fusion restates it, except that every
pixel of a view reads the masks (its own and every source's) as they stood
before the view's first pixel, and that acosf / expf are the project's pinned
ones. A view is whole-array arithmetic per hypothesis (0 = fusion_folder's
maps, 1 = output_folder's) and source slot; there is no used_list: an approved
pixel masks the targets of its chosen hypothesis's below-threshold candidates.
int(p + 0.5f) as ref_fusion_jacobi._pixel_coord.

`variant` restates the rule wrongly on purpose, for the tests that show the
cloud depends on each pinned detail: "strict_tie" (hypothesis 1 wins only if
n_1 > n_0), "min" (min for fmax where both of a source's maps pass),
"mask_unchosen" (an approval masks the unchosen hypothesis's candidates).
"""
import os

import numpy as np

from acmmp_amd import io as aio
from oracle_fusion import _load_view, _project, _world, f32
from ref_fusion_jacobi import _acosf, _expf, _pixel_coord

TRACE_KEYS = ("live", "approved", "both_choose_1", "both_choose_0", "only_1", "only_0", "penalty_rejected",
              "cand_both_maps", "cand_one_map")


def _map_passes(i, cams, cc, rr, ref_depth, ref_normal, s, src_r, src_c, src_depth, src_normal):
    """metric_of and the three thresholds for one of a source's two maps, over
    arrays of pixels: (passes, exp(-index) where it passes, else 0)."""
    n = len(cc)
    passes, dc = np.zeros(n, bool), np.zeros(n, f32)
    k = np.nonzero(src_depth > 0)[0]  # else all three metrics are 1e6
    tX = _world(src_c[k], src_r[k], src_depth[k], cams[s])
    tx, ty, proj_depth = _project(tX, cams[i])
    dx, dy = (f32(cc[k]) - tx).astype(np.float64), (f32(rr[k]) - ty).astype(np.float64)
    reproj = np.sqrt(dx * dx + dy * dy).astype(f32)
    rel = np.abs(proj_depth - ref_depth[k]) / ref_depth[k]
    first = (reproj < f32(2.0)) & (rel < f32(0.01))
    k, reproj, rel = k[first], reproj[first], rel[first]
    a, b = ref_normal[k], src_normal[k]
    ang = _acosf(a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2])
    ang[ang != ang] = f32(0.0)  # GetAngle
    third = ang < f32(0.174533)
    k, reproj, rel, ang = k[third], reproj[third], rel[third], ang[third]
    passes[k] = True
    dc[k] = _expf(-(reproj + f32(200) * rel + ang * f32(10)))
    return passes, dc


def run_prior_aware_fusion_jacobi(dense, out, fusion_folder, geom=True, consistency_scalar=0.3, con_num_thresh=1,
                                  penalty=0, variant=None):
    """Returns (cloud, trace): the cloud as ref_fusion_jacobi's (xyz, normals,
    rgb) in view order, then pixel order; trace[i] = view i's counts under
    TRACE_KEYS (cand_*: below-threshold candidates of every evaluated
    hypothesis, by whether both of the source's maps passed or one)."""
    assert variant in (None, "strict_tie", "min", "mask_unchosen")
    problems = aio.read_pair(os.path.join(dense, "pair.txt"))
    index = {p.ref_image_id: i for i, p in enumerate(problems)}
    suffix = "depths_geom.dmb" if geom else "depths.dmb"
    imgs, cams, masks = [], [], []
    maps = ([], []), ([], [])  # [map pair m] = (depths, normals); m = 0 fusion_folder's, 1 output_folder's
    for p in problems:
        for m, folder in enumerate((fusion_folder, out)):
            rf = aio.result_folder(folder, p.ref_image_id)
            maps[m][0].append(aio.read_dmb(os.path.join(rf, suffix)).astype(f32))
            maps[m][1].append(aio.read_dmb(os.path.join(rf, "normals.dmb")).astype(f32))
        assert maps[0][0][-1].shape == maps[1][0][-1].shape
        img, cam = _load_view(dense, p.ref_image_id, maps[0][0][-1].shape)
        imgs.append(img)
        cams.append(cam)
        masks.append(np.zeros(maps[0][0][-1].shape, np.uint8))
    xyz, nrm, rgb, trace = [], [], [], []
    with np.errstate(all="ignore"):
        for i, p in enumerate(problems):
            H, W = masks[i].shape
            srcs = [index[s] for s in p.src_image_ids]
            d = (maps[0][0][i], maps[1][0][i])
            live = (masks[i] != 1) & ~((d[0] <= 0) & (d[1] <= 0))  # a NaN in either depth keeps the pixel live
            rr, cc = np.nonzero(live)  # row-major: ascending pixel index
            L = len(rr)
            num = np.zeros((2, L), np.int64)
            dyn = np.zeros((2, L), f32)
            hit = np.zeros((2, L, max(len(srcs), 1)), bool)
            target = np.zeros((2, L, max(len(srcs), 1)), np.int64)
            X = [None, None]
            cand_both = cand_one = 0
            for b in (0, 1):  # every test of the view against the masks as they stand: nothing is written yet
                ref_depth = d[b][rr, cc]
                ref_normal = maps[b][1][i][rr, cc]
                X[b] = _world(cc, rr, ref_depth, cams[i])
                ev = ref_depth > 0  # the hypothesis is evaluated
                for j, s in enumerate(srcs):
                    sh, sw = masks[s].shape
                    px, py, _ = _project(X[b], cams[s])
                    src_r, in_r = _pixel_coord(py, sh)
                    src_c, in_c = _pixel_coord(px, sw)
                    k = np.nonzero(ev & in_r & in_c)[0]
                    k = k[masks[s][src_r[k], src_c[k]] != 1]
                    t, dc = [], []
                    for m in (0, 1):  # both of the source's maps
                        tm, dcm = _map_passes(i, cams, cc[k], rr[k], ref_depth[k], ref_normal[k], s, src_r[k],
                                              src_c[k], maps[m][0][s][src_r[k], src_c[k]],
                                              maps[m][1][s][src_r[k], src_c[k]])
                        t.append(tm)
                        dc.append(dcm)
                    both, either = t[0] & t[1], t[0] | t[1]
                    two = np.minimum(dc[0], dc[1]) if variant == "min" else np.maximum(dc[0], dc[1])
                    val = np.where(both, two, np.where(t[0], dc[0], dc[1]))
                    k, val = k[either], val[either]
                    dyn[b, k] = dyn[b, k] + val  # ascending slot order
                    num[b, k] += 1
                    hit[b, k, j] = True
                    target[b, k, j] = src_r[k] * sw + src_c[k]
                    cand_both += int(both.sum())
                    cand_one += int((either & ~both).sum())
            t = (num >= con_num_thresh) & (dyn > f32(consistency_scalar) * num.astype(f32))
            both = t[0] & t[1]
            one_wins = (num[1] > num[0]) if variant == "strict_tie" else (num[1] >= num[0])
            pick = np.where(both, one_wins, t[1]).astype(np.int64)  # (:754-789)
            n_pick = np.where(pick == 1, num[1], num[0])
            single = (t[0] | t[1]) & ~both
            ok = both | (single & (n_pick >= con_num_thresh + penalty))
            sel = pick[ok]
            pts = [np.where(sel == 1, X[1][a][ok], X[0][a][ok]) for a in range(3)]
            xyz.append(np.stack(pts, -1).astype(f32).reshape(-1, 3))
            nrm.append(np.where(sel[:, None] == 1, maps[1][1][i][rr[ok], cc[ok]],
                                maps[0][1][i][rr[ok], cc[ok]]).reshape(-1, 3))
            rgb.append(imgs[i][rr[ok], cc[ok]][:, ::-1].reshape(-1, 3))
            masked = 1 - pick if variant == "mask_unchosen" else pick
            for j, s in enumerate(srcs):  # apply: single bits, any order
                for b in (0, 1):
                    a = ok & (masked == b) & hit[b, :, j]
                    masks[s].reshape(-1)[target[b, a, j]] = 1
            trace.append(dict(zip(TRACE_KEYS, (
                L, int(ok.sum()), int((both & (pick == 1)).sum()), int((both & (pick == 0)).sum()),
                int((ok & single & (pick == 1)).sum()), int((ok & single & (pick == 0)).sum()),
                int((single & ~ok).sum()), cand_both, cand_one))))
    return (np.concatenate(xyz), np.concatenate(nrm), np.concatenate(rgb).astype(np.uint8)), trace


def trace_totals(trace):
    return {key: sum(t[key] for t in trace) for key in TRACE_KEYS}


# ---- the folders the CPU and GPU tests share

def prior_reconstruction(d, out, views):
    """The prior run's output folder <d>/ACMMP_PRIOR: test_fusion.py's
    _prior_reconstruction at any view count (`out`'s depths, 30 % of them x 1.05,
    then 10 % zeroed) with the normals perturbed as well. depths.dmb, where
    `out` has one, gets the same treatment from a generator of its own, so the
    geometric maps do not depend on it."""
    prior = d + "/ACMMP_PRIOR"
    rng, rng_photo = np.random.default_rng(2), np.random.default_rng(3)
    for i in range(views):
        src, dst = aio.result_folder(out, i), aio.result_folder(prior, i)
        os.makedirs(dst, exist_ok=True)
        dep = aio.read_dmb(os.path.join(src, "depths_geom.dmb"))
        dep = np.where(rng.random(dep.shape) < 0.3, dep * 1.05, dep).astype(np.float32)
        dep[rng.random(dep.shape) < 0.1] = 0.0
        aio.write_dmb(os.path.join(dst, "depths_geom.dmb"), dep)
        nrm = aio.read_dmb(os.path.join(src, "normals.dmb")).astype(np.float64)
        nrm = nrm + rng.normal(0, 0.02, nrm.shape)
        nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
        aio.write_dmb(os.path.join(dst, "normals.dmb"), nrm.astype(np.float32))
        if os.path.exists(os.path.join(src, "depths.dmb")):
            dep = aio.read_dmb(os.path.join(src, "depths.dmb"))
            dep = np.where(rng_photo.random(dep.shape) < 0.3, dep * 1.05, dep).astype(np.float32)
            dep[rng_photo.random(dep.shape) < 0.1] = 0.0
            aio.write_dmb(os.path.join(dst, "depths.dmb"), dep)
    return prior


def order_free_folder(tmp_path):
    """72 x 54, 4 views with 3 sources each; views 1-3 take view 0's camera
    file and view 0's maps with N(0, 0.003) relative depth noise and 20 % holes.
    Every pixel then falls on its own coordinates in every source: no two pixels
    of a view share a target, so the order within a view cannot matter.
    Returns (dense, synthetic folder, perturbed folder)."""
    import shutil
    from ref_fusion_jacobi import synthetic_folder
    d, out = synthetic_folder(tmp_path, 72, 54, 4, 3)
    rng = np.random.default_rng(5)
    rf0 = aio.result_folder(out, 0)
    depth0 = aio.read_dmb(os.path.join(rf0, "depths_geom.dmb"))
    for i in range(1, 4):
        shutil.copy(os.path.join(d, "cams", "%08d_cam.txt" % 0), os.path.join(d, "cams", "%08d_cam.txt" % i))
        rf = aio.result_folder(out, i)
        dep = (depth0 * (1 + rng.normal(0, 0.003, depth0.shape))).astype(np.float32)
        dep[rng.random(dep.shape) < 0.2] = 0.0
        aio.write_dmb(os.path.join(rf, "depths_geom.dmb"), dep)
        shutil.copy(os.path.join(rf0, "normals.dmb"), os.path.join(rf, "normals.dmb"))
        os.remove(os.path.join(rf, "depths.dmb"))
    os.remove(os.path.join(rf0, "depths.dmb"))
    return d, out, prior_reconstruction(d, out, 4)
