"""RunFusion in Jacobi order (acmmp_run_fusion_jacobi) restated
in numpy float32 — TEST INFRASTRUCTURE, the checker of
acmmp_amd/csrc/acmmp_fusion_dev.hip.

The rule: RunFusion (src/acmmp_definitions.cpp:828-1043) as
tests/oracle_fusion.py:run_fusion restates it, except that every pixel of a
view reads the masks as they stood before the view's first pixel, and that
acosf / expf are the project's pinned ones (oracle.math_fn). A view is then
whole-array arithmetic (numpy's float32 element operations are the IEEE
ones, unfused), followed by used_list stated from its definition instead of
the walk: at every approved pixel a, per source slot j, the target of the
last pixel <= a that passed slot j's tests is masked (a searchsorted over the
slot's hit pixels).

int(p + 0.5f): a value that is not finite or lies outside [-2^31, 2^31) is
out of bounds (what the host's conversion gives, INT_MIN), tested before the
conversion.
"""
import os

import numpy as np

import oracle
from acmmp_amd import io as aio
from oracle_fusion import _initial_mask, _load_view, _project, _world, f32


def _acosf(x):
    return np.array([oracle.math_fn("acosf", v) for v in x], f32)


def _expf(x):
    return np.array([oracle.math_fn("expf", v) for v in x], f32)


def _pixel_coord(p, n):
    """int(p + 0.5f) and whether it lies in [0, n)."""
    v = p + f32(0.5)
    ok = np.isfinite(v) & (v >= f32(-2.0 ** 31)) & (v < f32(2.0 ** 31))
    k = np.where(ok, v, f32(0)).astype(np.int64)  # truncates, as int()
    return k, ok & (k >= 0) & (k < n)


def run_fusion_jacobi(dense, out, geom=True, consistency_scalar=0.3, con_num_thresh=1, mask_folder=None):
    """Returns (cloud, trace). cloud = (xyz float32 [n, 3], normals float32
    [n, 3], rgb uint8 [n, 3]) in view order, then pixel order. trace[i], for
    view i: `hits` [slot j] = (hit pixels ascending, their target pixels in the
    source), `approved` = the approved pixels, and the applied used_list
    entries (slot, hit pixel), each once: `fresh` = set at an approved pixel
    itself, `stale` = set at an unapproved pixel and applied by a later
    approval."""
    problems = aio.read_pair(os.path.join(dense, "pair.txt"))
    index = {p.ref_image_id: i for i, p in enumerate(problems)}
    imgs, cams, depths, normals, masks = [], [], [], [], []
    for p in problems:
        rf = aio.result_folder(out, p.ref_image_id)
        depths.append(aio.read_dmb(os.path.join(rf, "depths_geom.dmb" if geom else "depths.dmb")).astype(f32))
        normals.append(aio.read_dmb(os.path.join(rf, "normals.dmb")).astype(f32))
        img, cam = _load_view(dense, p.ref_image_id, depths[-1].shape)
        imgs.append(img)
        cams.append(cam)
        masks.append(np.zeros(depths[-1].shape, np.uint8) if mask_folder is None else
                     _initial_mask(dense, mask_folder, p.ref_image_id, depths[-1].shape).copy())
    xyz, nrm, rgb, trace = [], [], [], []
    with np.errstate(all="ignore"):
        for i, p in enumerate(problems):
            H, W = depths[i].shape
            srcs = [index[s] for s in p.src_image_ids]
            d = depths[i]
            live = (masks[i] != 1) & ~((d <= 0) | (d >= f32(cams[i].depth_max)))  # a NaN depth is live
            rr, cc = np.nonzero(live)  # row-major: ascending pixel index
            q = rr * W + cc
            ref_depth = d[rr, cc]
            ref_normal = normals[i][rr, cc]
            X = _world(cc, rr, ref_depth, cams[i])
            num = np.zeros(len(q), np.int64)
            dyn = np.zeros(len(q), f32)
            hits = []
            for s in srcs:  # every test of the view against the masks as they stand: nothing is written yet
                sh, sw = depths[s].shape
                px, py, _ = _project(X, cams[s])
                src_r, in_r = _pixel_coord(py, sh)
                src_c, in_c = _pixel_coord(px, sw)
                k = np.nonzero(in_r & in_c)[0]
                k = k[masks[s][src_r[k], src_c[k]] != 1]
                src_depth = depths[s][src_r[k], src_c[k]]
                k, src_depth = k[~(src_depth <= 0)], src_depth[~(src_depth <= 0)]
                tX = _world(src_c[k], src_r[k], src_depth, cams[s])
                tx, ty, proj_depth = _project(tX, cams[i])
                dx, dy = (f32(cc[k]) - tx).astype(np.float64), (f32(rr[k]) - ty).astype(np.float64)
                reproj = np.sqrt(dx * dx + dy * dy).astype(f32)
                rel = np.abs(proj_depth - ref_depth[k]) / ref_depth[k]
                first = (reproj < f32(2.0)) & (rel < f32(0.01))
                k, reproj, rel = k[first], reproj[first], rel[first]
                a, b = ref_normal[k], normals[s][src_r[k], src_c[k]]
                ang = _acosf(a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2])
                ang[ang != ang] = f32(0.0)  # GetAngle
                third = ang < f32(0.174533)
                k, reproj, rel, ang = k[third], reproj[third], rel[third], ang[third]
                tmp_index = reproj + f32(200) * rel + ang * f32(10)
                dyn[k] = dyn[k] + _expf(-tmp_index)  # ascending slot order
                num[k] += 1
                hits.append((q[k], src_r[k] * sw + src_c[k]))
            ok = (num >= con_num_thresh) & (dyn > f32(consistency_scalar) * num.astype(f32))
            approved = q[ok]
            xyz.append(np.stack([X[0][ok], X[1][ok], X[2][ok]], -1).astype(f32).reshape(-1, 3))
            nrm.append(ref_normal[ok].reshape(-1, 3))
            rgb.append(imgs[i][rr[ok], cc[ok]][:, ::-1].reshape(-1, 3))
            fresh, stale = [], []
            for j, (s, (hq, target)) in enumerate(zip(srcs, hits)):
                last = np.unique(np.searchsorted(hq, approved, side="right") - 1)
                last = last[last >= 0]  # the slot's hits that some approval applies
                masks[s].reshape(-1)[target[last]] = 1
                at_approved = np.isin(hq[last], approved)
                fresh += [(j, int(v)) for v in hq[last][at_approved]]
                stale += [(j, int(v)) for v in hq[last][~at_approved]]
            trace.append({"hits": hits, "approved": approved, "fresh": fresh, "stale": stale})
    return (np.concatenate(xyz), np.concatenate(nrm), np.concatenate(rgb).astype(np.uint8)), trace


def cloud_of_list(points):
    """oracle_fusion.run_fusion's list of (X, normal, (r, g, b)) as the arrays above."""
    return (np.array([p[0] for p in points], f32).reshape(-1, 3), np.array([p[1] for p in points], f32).reshape(-1, 3),
            np.array([p[2] for p in points], np.uint8).reshape(-1, 3))


def cloud_of_ply(ply):
    return (np.stack([ply["x"], ply["y"], ply["z"]], -1), np.stack([ply["nx"], ply["ny"], ply["nz"]], -1),
            np.stack([ply["r"], ply["g"], ply["b"]], -1))


def assert_clouds_equal(got, ref):
    """Point count, order, xyz and normals as 32-bit words, colours as bytes."""
    assert len(got[0]) == len(ref[0])
    np.testing.assert_array_equal(np.ascontiguousarray(got[0], f32).view(np.uint32),
                                  np.ascontiguousarray(ref[0], f32).view(np.uint32))
    np.testing.assert_array_equal(np.ascontiguousarray(got[1], f32).view(np.uint32),
                                  np.ascontiguousarray(ref[1], f32).view(np.uint32))
    np.testing.assert_array_equal(got[2], ref[2])


def point_set(cloud):
    """The cloud's points as a set of byte records (order-free comparison)."""
    rec = np.concatenate([np.ascontiguousarray(cloud[0], f32).view(np.uint8).reshape(-1, 12),
                          np.ascontiguousarray(cloud[1], f32).view(np.uint8).reshape(-1, 12),
                          np.ascontiguousarray(cloud[2], np.uint8).reshape(-1, 3)], -1)
    return {r.tobytes() for r in rec}


# ---- the folders the CPU and GPU tests share

def stale_entry_folder(tmp_path):
    """The known answer for used_list's stale entries: four views of 72x54
    that share view 0's camera, every view a source of every other, all depths
    0 except the mid-range depth at pixel A = (row 2, column 5) and B = (row 50,
    column 60). View 0 holds A with the tilted normal n' and B with n; its
    slot-0 and slot-1 sources hold A with n, its slot-2 source holds B with n.
    View 0's A passes slots 0 and 1 but stays unapproved (each exp(-1.7)); its B
    is approved through slot 2 and applies A's two stale entries as well, which
    masks A in both sources. With consistency_scalar 0.3 and con_num_thresh 1
    the cloud is view 0's B alone; with used_list reset per pixel the two
    sources' A would support each other and add a second point."""
    import shutil
    from acmmp_amd import scene
    from PIL import Image
    W, H = 72, 54
    d = str(tmp_path / "stale")
    sc = scene.make_scene(num_views=4, width=W, height=H)
    scene.write_dense_folder(sc, d, num_src=3)
    for i in range(1, 4):
        shutil.copy(os.path.join(d, "cams", "%08d_cam.txt" % 0), os.path.join(d, "cams", "%08d_cam.txt" % i))
    aio.write_pair(os.path.join(d, "pair.txt"), [[(s, 3 - k) for k, s in enumerate(x for x in range(4) if x != i)]
                                                 for i in range(4)])
    cam = aio.read_camera(os.path.join(d, "cams", "%08d_cam.txt" % 0))
    mid = np.float32((cam.depth_min + cam.depth_max) / 2)
    assert mid == 550
    srcs = list(aio.read_pair(os.path.join(d, "pair.txt"))[0].src_image_ids)
    A, B = (2, 5), (50, 60)
    n, n2 = (0.0, 0.0, -1.0), (np.sin(0.17), 0.0, -np.cos(0.17))
    content = {0: [(A, n2), (B, n)], srcs[0]: [(A, n)], srcs[1]: [(A, n)], srcs[2]: [(B, n)]}
    out = d + "/ACMMP"
    for i in range(4):
        g = np.clip(np.rint(sc.views[i].image), 0, 255).astype(np.uint8)
        Image.fromarray(np.stack([g, 255 - g, np.roll(g, 3, 1)], -1), "RGB").save(
            os.path.join(d, "images", "%08d.jpg" % i), "JPEG", quality=92)
        depth, nrm = np.zeros((H, W), np.float32), np.zeros((H, W, 3), np.float32)
        nrm[..., 2] = -1
        for (r, c), normal in content[i]:
            depth[r, c], nrm[r, c] = mid, normal
        rf = aio.result_folder(out, i)
        os.makedirs(rf, exist_ok=True)
        aio.write_dmb(os.path.join(rf, "depths_geom.dmb"), depth)
        aio.write_dmb(os.path.join(rf, "normals.dmb"), nrm)
    return d, out, (A, B)


def synthetic_folder(tmp_path, W, H, views, num_src, seed=1):
    """test_fusion.py's recipe at any size: colour images, ground-truth depth
    and normal maps with noise and 5 % holes, as depths_geom.dmb and (another
    20 % of the depths moved) depths.dmb; every view's first `num_src` other
    views as its sources."""
    from acmmp_amd import scene
    from PIL import Image
    d = str(tmp_path / "dense")
    sc = scene.make_scene(num_views=views, width=W, height=H)
    scene.write_dense_folder(sc, d)
    aio.write_pair(os.path.join(d, "pair.txt"),
                   [[(s, num_src - k) for k, s in enumerate([x for x in range(views) if x != i][:num_src])]
                    for i in range(views)])
    out = d + "/ACMMP"
    rng = np.random.default_rng(seed)
    for i, v in enumerate(sc.views):
        g = np.clip(np.rint(v.image), 0, 255).astype(np.uint8)
        Image.fromarray(np.stack([g, 255 - g, np.roll(g, 3, 1)], -1), "RGB").save(
            os.path.join(d, "images", "%08d.jpg" % i), "JPEG", quality=92)
        rf = aio.result_folder(out, i)
        os.makedirs(rf, exist_ok=True)
        depth = np.where(v.depth > 0, v.depth * (1 + rng.normal(0, 0.002, v.depth.shape)), 0).astype(np.float32)
        depth[rng.random(depth.shape) < 0.05] = 0.0
        nrm = v.normal + rng.normal(0, 0.02, v.normal.shape)
        nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
        aio.write_dmb(os.path.join(rf, "depths_geom.dmb"), depth)
        aio.write_dmb(os.path.join(rf, "depths.dmb"),
                      np.where(rng.random(depth.shape) < 0.2, depth * np.float32(1.004), depth).astype(np.float32))
        aio.write_dmb(os.path.join(rf, "normals.dmb"), nrm.astype(np.float32))
    return d, out


def shrink_maps(out, view, w, h):
    """`view`'s maps at w x h (nearest sampling) under its full-size image and
    camera, as test_fusion.py's _shrink_maps_of_view_1: the other views then
    see a source of another size."""
    rf = aio.result_folder(out, view)
    H, W = aio.read_dmb(os.path.join(rf, "normals.dmb")).shape[:2]
    rows = np.minimum(((np.arange(h) + 0.5) * H / h).astype(int), H - 1)
    cols = np.minimum(((np.arange(w) + 0.5) * W / w).astype(int), W - 1)
    for name in ("depths_geom.dmb", "depths.dmb", "normals.dmb"):
        path = os.path.join(rf, name)
        if os.path.exists(path):
            aio.write_dmb(path, aio.read_dmb(path)[rows][:, cols])
