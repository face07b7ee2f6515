"""Jacobi-order prior-aware fusion on the GPU
(acmmp_run_prior_aware_fusion_jacobi, acmmp_amd/csrc/acmmp_fusion_dev.hip,
DESIGN.md §8) against the rule's numpy restatement
(tests/ref_prior_fusion_jacobi.py). Every comparison is exact: point count and
order, xyz and normals as 32-bit words, colours as bytes. Call convention as
test_fusion.py: the output folder is the perturbed reconstruction, the fusion
folder the synthetic one."""
import os
import subprocess

import numpy as np
import pytest

from acmmp_amd import _abi
from acmmp_amd import io as aio
from acmmp_amd import pipeline, scene
from oracle_fusion import read_ply
from ref_fusion_jacobi import assert_clouds_equal, cloud_of_ply, point_set, shrink_maps, synthetic_folder
from ref_prior_fusion_jacobi import (order_free_folder, prior_reconstruction, run_prior_aware_fusion_jacobi,
                                     trace_totals)
from test_gpu_prior_drivers import write_scene_priors

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "acmmp_amd", "lib", "acmmp_main")


def _ply(folder):
    return os.path.join(folder, "ACMMP_prior_model.ply")


def _fuse(d, prior, out, **kw):
    n = pipeline.run_prior_aware_fusion(d, prior, out, order="jacobi", **kw)
    cloud = cloud_of_ply(read_ply(_ply(prior)))
    assert n == len(cloud[0])
    return cloud


@pytest.mark.parametrize("penalty", [0, 1])
def test_fixture_matches_restatement_and_differs_from_literal(tmp_path, penalty):
    d, out = synthetic_folder(tmp_path, 72, 54, 4, 2)
    prior = prior_reconstruction(d, out, 4)
    got = _fuse(d, prior, out, single_match_penalty=penalty, num_consistent_thresh=1)
    first = open(_ply(prior), "rb").read()
    ref, _ = run_prior_aware_fusion_jacobi(d, prior, out, penalty=penalty, con_num_thresh=1)
    assert len(got[0]) > 1000
    assert_clouds_equal(got, ref)
    _fuse(d, prior, out, single_match_penalty=penalty, num_consistent_thresh=1)
    assert open(_ply(prior), "rb").read() == first  # two runs, the same bytes
    pipeline.run_prior_aware_fusion(d, prior, out, single_match_penalty=penalty, num_consistent_thresh=1)
    literal = cloud_of_ply(read_ply(_ply(prior)))
    assert point_set(literal) != point_set(got)


def test_order_free_folder_equals_the_literal_library(tmp_path):
    d, out, prior = order_free_folder(tmp_path)
    got = _fuse(d, prior, out, single_match_penalty=1)
    ref, _ = run_prior_aware_fusion_jacobi(d, prior, out, penalty=1)
    assert len(ref[0]) > 2000
    assert_clouds_equal(got, ref)
    pipeline.run_prior_aware_fusion(d, prior, out, single_match_penalty=1)
    assert_clouds_equal(cloud_of_ply(read_ply(_ply(prior))), got)


@pytest.fixture(scope="module")
def odd_folder(tmp_path_factory):
    """131 x 67 (odd, no multiple of a mask word; more than two scan chunks),
    5 views with 4 sources each, view 1's maps at 100 x 50 in both folders."""
    d, out = synthetic_folder(tmp_path_factory.mktemp("prior_odd"), 131, 67, 5, 4)
    prior = prior_reconstruction(d, out, 5)
    shrink_maps(out, 1, 100, 50)
    shrink_maps(prior, 1, 100, 50)
    return d, out, prior


def test_image_spans_more_than_two_scan_chunks():
    assert 131 * 67 > 2 * _abi.load_library().acmmp_fusion_jacobi_scan_chunk()


@pytest.mark.parametrize("penalty,thresh,scalar,geom", [(1, 1, 0.3, True), (2, 2, 0.25, True), (1, 1, 0.3, False)])
def test_odd_sizes_mixed_views_and_options(odd_folder, penalty, thresh, scalar, geom):
    d, out, prior = odd_folder
    got = _fuse(d, prior, out, single_match_penalty=penalty, num_consistent_thresh=thresh, consistency_scalar=scalar,
                geom_consistency=geom)
    ref, trace = run_prior_aware_fusion_jacobi(d, prior, out, geom=geom, consistency_scalar=scalar,
                                               con_num_thresh=thresh, penalty=penalty)
    print(penalty, thresh, scalar, geom, trace_totals(trace))
    assert len(ref[0]) > 1000
    assert_clouds_equal(got, ref)


def test_view_that_is_its_own_source(tmp_path):
    """View 2 lists itself as its first source: its own mask, read as a
    source's, is the one from before the view began."""
    d, out = synthetic_folder(tmp_path, 72, 54, 4, 2)
    prior = prior_reconstruction(d, out, 4)
    problems = aio.read_pair(os.path.join(d, "pair.txt"))
    sel = [[(s, len(p.src_image_ids) - k) for k, s in enumerate(p.src_image_ids)] for p in problems]
    sel[2] = [(2, 3)] + sel[2]
    aio.write_pair(os.path.join(d, "pair.txt"), sel)
    assert list(aio.read_pair(os.path.join(d, "pair.txt"))[2].src_image_ids)[0] == 2
    got = _fuse(d, prior, out)
    ref, _ = run_prior_aware_fusion_jacobi(d, prior, out)
    assert len(ref[0]) > 1000
    assert_clouds_equal(got, ref)


def test_non_finite_depths(tmp_path):
    """NaN, +inf and -inf depths in each of the four roles: view 0's map and
    its prior (a NaN in either keeps the pixel live; an infinite depth projects
    to a coordinate int() cannot hold), view 2's map and prior read as a
    source's by the others."""
    d, out = synthetic_folder(tmp_path, 72, 54, 4, 2)
    prior = prior_reconstruction(d, out, 4)
    rng = np.random.default_rng(9)
    for folder in (out, prior):
        for view in (0, 2):
            path = os.path.join(aio.result_folder(folder, view), "depths_geom.dmb")
            dep = aio.read_dmb(path)
            for value in (np.nan, np.inf, -np.inf):
                dep[rng.integers(0, dep.shape[0], 12), rng.integers(0, dep.shape[1], 12)] = value
            aio.write_dmb(path, dep)
    got = _fuse(d, prior, out)
    ref, _ = run_prior_aware_fusion_jacobi(d, prior, out)
    assert len(ref[0]) > 1000
    assert_clouds_equal(got, ref)


def test_seven_source_slots(tmp_path):
    d, out = synthetic_folder(tmp_path, 40, 30, 8, 7)
    prior = prior_reconstruction(d, out, 8)
    got = _fuse(d, prior, out, single_match_penalty=1)
    ref, _ = run_prior_aware_fusion_jacobi(d, prior, out, penalty=1)
    print("points:", len(ref[0]))
    assert len(ref[0]) > 500
    assert_clouds_equal(got, ref)


def test_cli_prior_fusion_jacobi_matches_python_call(tmp_path):
    """acmmp_main -p --force_fusion --fusion jacobi over a tiny single-scale
    folder whose /ACMMP a run without -p wrote: the PLY of
    pipeline.run_prior_aware_fusion(order="jacobi") over the same maps."""
    d = str(tmp_path / "dense") + "/"
    sc = scene.make_scene(num_views=3, width=96, height=72)
    scene.write_dense_folder(sc, d, num_src=2)
    write_scene_priors(d, sc)
    common = [EXE, d, "--quiet", "--no_triangulation"]
    for extra in (["--no_fusion"], ["-p", "--force_fusion", "--fusion", "jacobi"]):
        r = subprocess.run(common + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-3000:]
    prior, out = d + "/ACMMP_PRIOR", d + "/ACMMP"
    cli = open(_ply(prior), "rb").read()
    os.remove(_ply(prior))
    n = pipeline.run_prior_aware_fusion(d, prior, out, order="jacobi")
    print("points:", n)
    assert n > 0 and open(_ply(prior), "rb").read() == cli
