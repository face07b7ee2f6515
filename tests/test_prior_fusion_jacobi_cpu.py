"""Jacobi-order prior-aware fusion (acmmp_run_prior_aware_fusion_jacobi,
DESIGN.md §8) without a GPU: the rule's restatement
(tests/ref_prior_fusion_jacobi.py) against the literal restatement
(tests/oracle_fusion.py) where the two must agree and where they must differ,
that the restated cases reach every branch of the choice and depend on each
pinned detail, and the host side of the mode: ABI, the no-device error, the
order argument. The kernels are checked in test_gpu_prior_fusion_jacobi.py."""
import ctypes as C
import os

import pytest

from acmmp_amd import _abi, pipeline
from acmmp_amd.engine import AcmmpError
from oracle_fusion import run_prior_aware_fusion
from ref_fusion_jacobi import assert_clouds_equal, cloud_of_list, point_set, synthetic_folder
from ref_prior_fusion_jacobi import (order_free_folder, prior_reconstruction, run_prior_aware_fusion_jacobi,
                                     trace_totals)


@pytest.fixture(scope="module")
def order_free(tmp_path_factory):
    return order_free_folder(tmp_path_factory.mktemp("prior_order_free"))


@pytest.mark.parametrize("penalty,thresh", [(0, 1), (1, 1), (1, 2)])
def test_order_free_folder_equals_the_literal_restatement(order_free, penalty, thresh):
    """No two pixels of a view share a target, so the two orders are one: the
    same points, order and bytes. (Prototype of the rule: 3636 / 3581 / 3186
    points, 176 and 796 penalty rejections.)"""
    d, out, prior = order_free
    literal = cloud_of_list(run_prior_aware_fusion(d, prior, out, con_num_thresh=thresh, penalty=penalty))
    jacobi, trace = run_prior_aware_fusion_jacobi(d, prior, out, con_num_thresh=thresh, penalty=penalty)
    totals = trace_totals(trace)
    print("penalty", penalty, "thresh", thresh, "points", len(literal[0]), totals)
    assert len(literal[0]) > 2000
    assert (totals["penalty_rejected"] > 0) == (penalty > 0)
    assert_clouds_equal(jacobi, literal)


def test_orders_differ_on_the_synthetic_fixture(tmp_path):
    """(Prototype: literal 4579 points, Jacobi 4660, 106 only literal, 187 only Jacobi.)"""
    d, out = synthetic_folder(tmp_path, 72, 54, 4, 2)
    prior = prior_reconstruction(d, out, 4)
    literal = cloud_of_list(run_prior_aware_fusion(d, prior, out))
    jacobi, _ = run_prior_aware_fusion_jacobi(d, prior, out)
    only_l, only_j = point_set(literal) - point_set(jacobi), point_set(jacobi) - point_set(literal)
    print("points: literal", len(literal[0]), "jacobi", len(jacobi[0]), "only literal", len(only_l), "only jacobi",
          len(only_j))
    assert len(literal[0]) > 1000 and len(jacobi[0]) > 1000
    assert only_l and only_j


@pytest.fixture(scope="module")
def branches(tmp_path_factory):
    """131 x 67, 5 views, 4 sources, penalty 1, thresh 1: the folder, and its
    Jacobi cloud and trace."""
    d, out = synthetic_folder(tmp_path_factory.mktemp("prior_branches"), 131, 67, 5, 4)
    prior = prior_reconstruction(d, out, 5)
    cloud, trace = run_prior_aware_fusion_jacobi(d, prior, out, penalty=1, con_num_thresh=1)
    return d, out, prior, cloud, trace


def test_every_branch_of_the_choice_is_reached(branches):
    """Each outcome of the choice (:754-789) at least 1 % of the approved
    pixels, each kind of candidate at least 10 % of the candidates.
    (Prototype: 8457 points; both-pass choosing 1 4354, choosing 0 179, only-1
    317, only-0 3607, penalty rejections 1290; candidates on both maps 48177,
    on one 32514.)"""
    totals = trace_totals(branches[4])
    print(totals)
    assert totals["approved"] == len(branches[3][0]) > 5000
    assert totals["approved"] == sum(totals[k] for k in ("both_choose_1", "both_choose_0", "only_1", "only_0"))
    for key in ("both_choose_1", "both_choose_0", "only_1", "only_0", "penalty_rejected"):
        assert totals[key] >= 0.01 * totals["approved"], key
    cands = totals["cand_both_maps"] + totals["cand_one_map"]
    assert totals["cand_both_maps"] >= 0.1 * cands and totals["cand_one_map"] >= 0.1 * cands


@pytest.mark.parametrize("variant", ["strict_tie", "min", "mask_unchosen"])
def test_the_cloud_depends_on_each_pinned_detail(branches, variant):
    d, out, prior, cloud, _ = branches
    wrong, _ = run_prior_aware_fusion_jacobi(d, prior, out, penalty=1, con_num_thresh=1, variant=variant)
    print(variant, "points", len(wrong[0]), "against", len(cloud[0]))
    assert point_set(wrong) != point_set(cloud)


def test_abi_has_the_jacobi_prior_aware_fusion():
    lib = _abi.load_library()
    assert "acmmp_run_prior_aware_fusion_jacobi" in _abi.SIGNATURES
    assert lib.acmmp_run_prior_aware_fusion_jacobi.argtypes[-2] is C.c_int  # device


def test_no_usable_device_is_a_clean_error(order_free):
    """Device -1: ACMMP_ERR_HIP with a message, before any load, no PLY."""
    d, out, prior = order_free
    lib = _abi.load_library()
    with pytest.raises(AcmmpError) as err:
        pipeline.run_prior_aware_fusion(d, prior, out, order="jacobi", device=-1)
    assert "(status %d)" % _abi.ERR_HIP in str(err.value)
    assert lib.acmmp_fusion_last_error().decode().strip()
    assert not os.path.exists(os.path.join(prior, "ACMMP_prior_model.ply"))
    with pytest.raises(ValueError):
        pipeline.run_prior_aware_fusion(d, prior, out, order="x")
