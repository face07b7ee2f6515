"""Jacobi-order fusion on the GPU (acmmp_run_fusion_jacobi,
acmmp_amd/csrc/acmmp_fusion_dev.hip) against the rule's numpy
restatement (tests/ref_fusion_jacobi.py). Every comparison is exact: point
count and order, xyz and normals as 32-bit words, colours as bytes."""
import os
import subprocess

import numpy as np
import pytest

from acmmp_amd import _abi
from acmmp_amd import io as aio
from acmmp_amd import pipeline, scene
from oracle_fusion import read_ply
from ref_fusion_jacobi import (assert_clouds_equal, cloud_of_ply, point_set, run_fusion_jacobi, shrink_maps,
                               stale_entry_folder, synthetic_folder)
from test_fusion import _dense_with_maps

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "acmmp_amd", "lib", "acmmp_main")


def _fuse(d, out, **kw):
    n = pipeline.run_fusion(d, out, order="jacobi", **kw)
    cloud = cloud_of_ply(read_ply(os.path.join(out, "ACMMP_model.ply")))
    assert n == len(cloud[0])
    return cloud


def test_fixture_matches_restatement_and_differs_from_literal(tmp_path):
    d, out = _dense_with_maps(tmp_path)
    path = os.path.join(out, "ACMMP_model.ply")
    got = _fuse(d, out)
    first = open(path, "rb").read()
    ref, _ = run_fusion_jacobi(d, out)
    assert len(got[0]) > 1000
    assert_clouds_equal(got, ref)
    _fuse(d, out)
    assert open(path, "rb").read() == first  # two runs, the same bytes
    pipeline.run_fusion(d, out)
    literal = cloud_of_ply(read_ply(path))
    assert point_set(literal) != point_set(got)


def test_stale_entries_known_answer(tmp_path):
    d, out, (A, B) = stale_entry_folder(tmp_path)
    got = _fuse(d, out, consistency_scalar=0.3, num_consistent_thresh=1)
    ref, _ = run_fusion_jacobi(d, out, consistency_scalar=0.3, con_num_thresh=1)
    assert len(got[0]) == 1
    assert_clouds_equal(got, ref)


@pytest.fixture(scope="module")
def odd_folder(tmp_path_factory):
    """131 x 67 (odd, no multiple of a mask word; more than two scan chunks),
    5 views with 4 sources each, view 1's maps at 100 x 50, a gray 8-bit mask
    per view at its maps' size."""
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


def test_image_spans_more_than_two_scan_chunks():
    assert 131 * 67 > 2 * _abi.load_library().acmmp_fusion_jacobi_scan_chunk()


@pytest.mark.parametrize("options", ["photometric_thresholds_masks", "defaults"])
def test_odd_sizes_mixed_views_and_options(odd_folder, options):
    d, out = odd_folder
    if options == "defaults":
        got = _fuse(d, out)
        ref, _ = run_fusion_jacobi(d, out)
    else:
        got = _fuse(d, out, geom_consistency=False, consistency_scalar=0.5, num_consistent_thresh=2,
                    mask_folder="masks")
        ref, _ = run_fusion_jacobi(d, out, geom=False, consistency_scalar=0.5, con_num_thresh=2, mask_folder="masks")
    print(options, "points:", len(ref[0]))
    assert len(ref[0]) > (1000 if options == "defaults" else 100)  # (0.5 is above most pixels' average score)
    assert_clouds_equal(got, ref)


def test_view_that_is_its_own_source(tmp_path):
    """View 2 lists itself as its first source: its own mask, read as a
    source's, is the one from before the view began."""
    d, out = _dense_with_maps(tmp_path)
    problems = aio.read_pair(os.path.join(d, "pair.txt"))
    sel = [[(s, len(p.src_image_ids) - k) for k, s in enumerate(p.src_image_ids)] for p in problems]
    sel[2] = [(2, 3)] + sel[2]
    aio.write_pair(os.path.join(d, "pair.txt"), sel)
    assert list(aio.read_pair(os.path.join(d, "pair.txt"))[2].src_image_ids)[0] == 2
    got = _fuse(d, out)
    ref, _ = run_fusion_jacobi(d, out)
    assert len(ref[0]) > 1000
    assert_clouds_equal(got, ref)


def test_non_finite_depths(tmp_path):
    """NaN and infinite depths in view 0's map (a NaN depth is live: its
    projection is NaN, which int() cannot hold) and in view 2's (a source of
    the others): a coordinate that is not finite is out of bounds, before any
    conversion."""
    d, out = _dense_with_maps(tmp_path)
    rng = np.random.default_rng(9)
    for view in (0, 2):
        path = os.path.join(aio.result_folder(out, view), "depths_geom.dmb")
        dep = aio.read_dmb(path)
        for value in (np.nan, np.inf, -np.inf):
            dep[rng.integers(0, dep.shape[0], 12), rng.integers(0, dep.shape[1], 12)] = value
        aio.write_dmb(path, dep)
    got = _fuse(d, out)
    ref, _ = run_fusion_jacobi(d, out)
    assert len(ref[0]) > 1000
    assert_clouds_equal(got, ref)


def test_seven_source_slots(tmp_path):
    d, out = synthetic_folder(tmp_path, 40, 30, 8, 7)
    got = _fuse(d, out)
    ref, trace = run_fusion_jacobi(d, out)
    slots = {j for t in trace for j, _ in t["fresh"]}
    print("points:", len(ref[0]), "slots with applied entries:", sorted(slots))
    assert slots == set(range(7)) and len(ref[0]) > 500
    assert_clouds_equal(got, ref)


def test_cli_fusion_jacobi_matches_python_call(tmp_path):
    """acmmp_main --fusion jacobi over the maps its own passes wrote (a tiny
    single-scale folder) writes the PLY of pipeline.run_fusion(order="jacobi")
    over the same maps."""
    d = str(tmp_path / "dense")
    sc = scene.make_scene(num_views=4, width=96, height=72)
    scene.write_dense_folder(sc, d, num_src=3)
    r = subprocess.run([EXE, d, "--quiet", "--no_triangulation", "--fusion", "jacobi"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    path = os.path.join(d, "ACMMP", "ACMMP_model.ply")
    cli = open(path, "rb").read()
    os.remove(path)
    n = pipeline.run_fusion(d, d + "/ACMMP", order="jacobi")
    print("points:", n)
    assert n > 0 and open(path, "rb").read() == cli
