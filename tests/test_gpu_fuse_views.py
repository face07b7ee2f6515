"""Fusion of device-resident maps (acmmp_fuse_views_jacobi through
acmmp_amd.fusion) against the rule's numpy restatement
(tests/ref_fusion_jacobi.py) and against the folder call over the same maps.
The inputs are the small folders of the folder call's tests, loaded into
tensors. Every comparison is exact: point count and order, xyz and normals as
32-bit words, colours as bytes."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from acmmp_amd import _abi
from acmmp_amd import fusion
from acmmp_amd import io as aio
from acmmp_amd import pipeline, scene
from oracle_fusion import _initial_mask, _load_view, read_ply
from ref_fusion_jacobi import (assert_clouds_equal, cloud_of_ply, run_fusion_jacobi, shrink_maps, stale_entry_folder,
                               synthetic_folder)
from test_fusion import _dense_with_maps

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda", 0)


def load_views(d, out, geom=True, mask_folder=None, layout="planes"):
    """The folder's views as FusionViews on the device. layout "planes": one
    (H, W, 4) tensor a view (strides 4 / 4); "separate": a depth plane and a
    normal map (strides 1 / 3)."""
    problems = aio.read_pair(os.path.join(d, "pair.txt"))
    index = {p.ref_image_id: i for i, p in enumerate(problems)}
    views = []
    for p in problems:
        rf = aio.result_folder(out, p.ref_image_id)
        depth = aio.read_dmb(os.path.join(rf, "depths_geom.dmb" if geom else "depths.dmb")).astype(np.float32)
        normal = aio.read_dmb(os.path.join(rf, "normals.dmb")).astype(np.float32)
        bgr, cam = _load_view(d, p.ref_image_id, depth.shape)
        bgr = torch.from_numpy(np.ascontiguousarray(bgr)).to(DEV)
        mask = None
        if mask_folder is not None:
            mask = torch.from_numpy(_initial_mask(d, mask_folder, p.ref_image_id, depth.shape).copy()).to(DEV)
        src = [index[s] for s in p.src_image_ids]
        if layout == "planes":
            planes = torch.from_numpy(np.concatenate([normal, depth[..., None]], -1)).to(DEV)
            views.append(fusion.FusionView.from_planes(planes, cam, src, bgr=bgr, mask=mask))
        else:
            views.append(fusion.FusionView(cam, src, torch.from_numpy(depth).to(DEV), torch.from_numpy(normal).to(DEV),
                                           bgr=bgr, mask=mask))
    return views


def host(cloud):
    return tuple(t.cpu().numpy() for t in cloud)


@pytest.fixture(scope="module")
def fixture_folder(tmp_path_factory):
    """The 72 x 54 fixture (4 views, 2 sources) and the restatement's cloud for it."""
    d, out = _dense_with_maps(tmp_path_factory.mktemp("fx"))
    ref, _ = run_fusion_jacobi(d, out)
    assert len(ref[0]) > 1000
    return d, out, ref


def test_fixture_matches_restatement_and_folder_call(fixture_folder, tmp_path):
    d, out, ref = fixture_folder
    cloud = fusion.fuse_views(load_views(d, out))
    assert all(t.is_cuda for t in cloud) and cloud[2].dtype == torch.uint8
    assert_clouds_equal(host(cloud), ref)
    again = fusion.fuse_views(load_views(d, out))
    assert all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                           b.view(torch.int32) if b.dtype == torch.float32 else b) for a, b in zip(cloud, again))
    n = pipeline.run_fusion(d, out, order="jacobi")
    mine = str(tmp_path / "mine.ply")
    assert fusion.write_ply(mine, *cloud) == n
    assert open(mine, "rb").read() == open(os.path.join(out, "ACMMP_model.ply"), "rb").read()


def test_strides_separate_maps_and_planes_give_the_same_cloud(fixture_folder):
    d, out, ref = fixture_folder
    separate = load_views(d, out, layout="separate")
    planes = load_views(d, out, layout="planes")
    arr_s, arr_p = fusion.c_views(separate), fusion.c_views(planes)
    assert (arr_s[0].depth_stride, arr_s[0].normal_stride) == (1, 3)
    assert (arr_p[0].depth_stride, arr_p[0].normal_stride) == (4, 4)
    assert_clouds_equal(host(fusion.fuse_views(separate)), ref)
    assert_clouds_equal(host(fusion.fuse_views(planes)), ref)


@pytest.fixture(scope="module")
def odd_folder(tmp_path_factory):
    """131 x 67 (odd, no multiple of a mask word or of a ballot; more than two
    scan chunks), 5 views with 4 sources each, view 1's maps at 100 x 50, a
    gray 8-bit mask per view at its maps' size."""
    from PIL import Image
    d, out = synthetic_folder(tmp_path_factory.mktemp("odd"), 131, 67, 5, 4)
    shrink_maps(out, 1, 100, 50)
    os.makedirs(os.path.join(d, "masks"))
    rng = np.random.default_rng(5)
    for i in range(5):
        h, w = aio.read_dmb(os.path.join(aio.result_folder(out, i), "depths_geom.dmb")).shape
        Image.fromarray(rng.integers(70, 256, (h, w)).astype(np.uint8), "L").save(
            os.path.join(d, "masks", "%08d.png" % i))
    return d, out


@pytest.mark.parametrize("options", ["photometric_thresholds_masks", "defaults"])
def test_odd_sizes_mixed_views_and_masks(odd_folder, options):
    d, out = odd_folder
    chunk = _abi.load_library().acmmp_fusion_jacobi_scan_chunk()
    assert 131 * 67 > 2 * chunk and (131 * 67) % 64 and (131 * 67) % 32 and (100 * 50) % 64
    if options == "defaults":
        got = fusion.fuse_views(load_views(d, out))
        ref, _ = run_fusion_jacobi(d, out)
    else:
        got = fusion.fuse_views(load_views(d, out, geom=False, mask_folder="masks"), consistency_scalar=0.5,
                                num_consistent_thresh=2)
        ref, _ = run_fusion_jacobi(d, out, geom=False, consistency_scalar=0.5, con_num_thresh=2, mask_folder="masks")
    print(options, "points:", len(ref[0]))
    assert len(ref[0]) > (1000 if options == "defaults" else 100)  # (0.5 is above most pixels' average score)
    assert_clouds_equal(host(got), ref)


def test_stale_entries_known_answer(tmp_path):
    d, out, _ = stale_entry_folder(tmp_path)
    got = fusion.fuse_views(load_views(d, out), consistency_scalar=0.3, num_consistent_thresh=1)
    ref, _ = run_fusion_jacobi(d, out, consistency_scalar=0.3, con_num_thresh=1)
    assert len(got[0]) == 1
    assert_clouds_equal(host(got), ref)


def _own_source(d, out):
    problems = aio.read_pair(os.path.join(d, "pair.txt"))
    sel = [[(s, len(p.src_image_ids) - k) for k, s in enumerate(p.src_image_ids)] for p in problems]
    sel[2] = [(2, 3)] + sel[2]
    aio.write_pair(os.path.join(d, "pair.txt"), sel)
    assert list(aio.read_pair(os.path.join(d, "pair.txt"))[2].src_image_ids)[0] == 2


def _non_finite(d, out):
    rng = np.random.default_rng(9)
    for view in (0, 2):  # view 0: a reference before any mask is written; view 2: a source of the others
        path = os.path.join(aio.result_folder(out, view), "depths_geom.dmb")
        dep = aio.read_dmb(path)
        for value in (np.nan, np.inf, -np.inf):
            dep[rng.integers(0, dep.shape[0], 12), rng.integers(0, dep.shape[1], 12)] = value
        aio.write_dmb(path, dep)


def _empty_middle_view(d, out):
    path = os.path.join(aio.result_folder(out, 1), "depths_geom.dmb")
    aio.write_dmb(path, np.zeros_like(aio.read_dmb(path)))


def _view_without_sources(d, out):
    problems = aio.read_pair(os.path.join(d, "pair.txt"))
    sel = [[(s, len(p.src_image_ids) - k) for k, s in enumerate(p.src_image_ids)] for p in problems]
    sel[1] = []
    aio.write_pair(os.path.join(d, "pair.txt"), sel)
    assert len(aio.read_pair(os.path.join(d, "pair.txt"))[1].src_image_ids) == 0


SPECIAL = {"own_source": _own_source, "non_finite_depths": _non_finite, "empty_middle_view": _empty_middle_view,
           "view_without_sources": _view_without_sources}


@pytest.mark.parametrize("case", sorted(SPECIAL))
def test_special_views(tmp_path, case):
    """The running total across a view that approves nothing, a view's own
    mask read as a source's (pin 1), and the pixel_coord guard."""
    d, out = _dense_with_maps(tmp_path)
    SPECIAL[case](d, out)
    ref, trace = run_fusion_jacobi(d, out)
    if case in ("empty_middle_view", "view_without_sources"):
        assert len(trace[1]["approved"]) == 0 and len(trace[2]["approved"]) > 0
    assert len(ref[0]) > 1000
    assert_clouds_equal(host(fusion.fuse_views(load_views(d, out))), ref)


def test_seven_source_slots(tmp_path):
    d, out = synthetic_folder(tmp_path, 40, 30, 8, 7)
    ref, trace = run_fusion_jacobi(d, out)
    assert {j for t in trace for j, _ in t["fresh"]} == set(range(7)) and len(ref[0]) > 500
    assert_clouds_equal(host(fusion.fuse_views(load_views(d, out))), ref)


SENTINEL_F, SENTINEL_B = -12345.5, 0xA5


def _raw_call(views, capacity, extra=64):
    """The C call with arrays of capacity + extra points pre-filled with a
    sentinel: (status, num_points, message, the three whole arrays)."""
    lib = _abi.load_library()
    arr = fusion.c_views(views)
    xyz = torch.full((capacity + extra, 3), SENTINEL_F, dtype=torch.float32, device=DEV)
    nrm = torch.full((capacity + extra, 3), SENTINEL_F, dtype=torch.float32, device=DEV)
    rgb = torch.full((capacity + extra, 3), SENTINEL_B, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    out = _abi.CloudBuffers(xyz.data_ptr(), nrm.data_ptr(), rgb.data_ptr(), capacity)
    n = C.c_int64(-1)
    rc = lib.acmmp_fuse_views_jacobi(0, arr, len(views), 0.3, 1, C.byref(out), None, C.byref(n))
    return rc, n.value, lib.acmmp_fusion_last_error().decode(), (xyz.cpu().numpy(), nrm.cpu().numpy(), rgb.cpu().numpy())


def test_capacity(fixture_folder):
    d, out, ref = fixture_folder
    views = load_views(d, out)
    n = len(ref[0])
    lib = _abi.load_library()
    count = C.c_int64(-1)
    arr = fusion.c_views(views)
    for buffers in (None, C.byref(_abi.CloudBuffers(None, None, None, 0))):  # the counting calls
        assert lib.acmmp_fuse_views_jacobi(0, arr, len(views), 0.3, 1, buffers, None, C.byref(count)) == 0
        assert count.value == n
    rc, got_n, msg, arrays = _raw_call(views, n - 1)
    assert rc == _abi.ERR_ARG and got_n == n and str(n) in msg and str(n - 1) in msg, (rc, got_n, msg)
    for a, r, sentinel in zip(arrays, ref, (SENTINEL_F, SENTINEL_F, SENTINEL_B)):
        assert (a[n - 1:] == sentinel).all()  # nothing at or beyond the capacity
        np.testing.assert_array_equal(a[:n - 1].view(np.uint32 if a.dtype == np.float32 else np.uint8),
                                      np.ascontiguousarray(r[:n - 1]).view(np.uint32 if a.dtype == np.float32
                                                                            else np.uint8))
    rc, got_n, msg, arrays = _raw_call(views, n)
    assert rc == 0 and got_n == n, msg
    assert_clouds_equal(tuple(a[:n] for a in arrays), ref)
    assert all((a[n:] == s).all() for a, s in zip(arrays, (SENTINEL_F, SENTINEL_F, SENTINEL_B)))
    with pytest.raises(fusion.AcmmpError, match=str(n)):
        fusion.fuse_views(views, capacity=n - 1)


def test_non_default_stream_with_inputs_produced_on_it(fixture_folder):
    d, out, ref = fixture_folder
    base = load_views(d, out, layout="separate")
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s):
        views = []
        for v in base:  # the planes are assembled on s, just before the fusion reads them
            planes = torch.cat([v.normal * 1.0, (v.depth + 0.0)[..., None]], -1)
            views.append(fusion.FusionView.from_planes(planes, v.cam, v.sources, bgr=v.bgr.clone(), mask=None))
        cloud = fusion.fuse_views(views)
    assert_clouds_equal(host(cloud), ref)


@pytest.fixture(scope="module")
def driver_run(tmp_path_factory):
    from acmmp_amd.distributed import ViewParallelPipeline
    d = str(tmp_path_factory.mktemp("drv") / "dense")
    scene.write_dense_folder(scene.make_scene(num_views=4, width=96, height=72), d, num_src=3)
    pipe = ViewParallelPipeline(d, device=0)
    pipe.run()
    cloud = pipe.fuse()
    path = os.path.join(d, "ACMMP", "ACMMP_model.ply")
    fused = open(path, "rb").read()
    os.remove(path)
    n = pipeline.run_fusion(d, d + "/ACMMP", order="jacobi")  # over the .dmb files that run wrote
    return d, host(cloud), fused, n, open(path, "rb").read()


def test_driver_fuse_matches_folder_call(driver_run):
    d, cloud, fused, n, folder_ply = driver_run
    print("points:", n)
    assert n > 0 and fused == folder_ply
    assert_clouds_equal(cloud, cloud_of_ply(read_ply(os.path.join(d, "ACMMP", "ACMMP_model.ply"))))
    assert np.isfinite(cloud[0]).all()  # (so the PLY's zeroing rule changed no coordinate)


def test_driver_cli_fuse_flag(driver_run):
    d, _, _, n, folder_ply = driver_run
    r = subprocess.run([sys.executable, "-m", "acmmp_amd.distributed", d, "--output_dir", "/CLI", "--fuse"],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    assert f"{n} points" in r.stdout
    assert open(os.path.join(d, "CLI", "ACMMP_model.ply"), "rb").read() == folder_ply
