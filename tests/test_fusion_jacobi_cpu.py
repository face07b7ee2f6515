"""Jacobi-order fusion (acmmp_run_fusion_jacobi) without a GPU:
the rule's restatement (tests/ref_fusion_jacobi.py) against the literal
restatement (tests/oracle_fusion.py) where the two must agree and where they
must differ, and the host side of the mode: ABI, the no-device error, the CLI
option. The kernels themselves are checked in test_gpu_fusion_jacobi.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from acmmp_amd import _abi, pipeline
from acmmp_amd.engine import AcmmpError
from oracle_fusion import run_fusion
from ref_fusion_jacobi import (assert_clouds_equal, cloud_of_list, point_set, run_fusion_jacobi,
                               stale_entry_folder)
from test_fusion import _dense_with_maps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "acmmp_amd", "lib", "acmmp_main")


@pytest.fixture(scope="module")
def fixture_clouds(tmp_path_factory):
    """test_fusion.py's fixture (72x54, 4 views, 2 sources) in both orders, once."""
    d, out = _dense_with_maps(tmp_path_factory.mktemp("jacobi_cpu"))
    jacobi, trace = run_fusion_jacobi(d, out)
    return cloud_of_list(run_fusion(d, out)), jacobi, trace


def test_stale_entries_known_answer(tmp_path):
    """One point, view 0's B, in both orders (no view of this case has two
    pixels on one target, so the orders agree): A's unapproved hits are
    applied by B's approval, 3511 pixels later. (The libm of the literal
    restatement and the pinned one of the Jacobi restatement agree on this
    point's tests: the cloud holds no libm result.)"""
    d, out, (A, B) = stale_entry_folder(tmp_path)
    literal = cloud_of_list(run_fusion(d, out, consistency_scalar=0.3, con_num_thresh=1))
    jacobi, trace = run_fusion_jacobi(d, out, consistency_scalar=0.3, con_num_thresh=1)
    assert len(literal[0]) == 1
    assert_clouds_equal(jacobi, literal)
    a, b = A[0] * 72 + A[1], B[0] * 72 + B[1]
    assert b - a == 3511
    assert list(trace[0]["approved"]) == [b]
    assert sorted(trace[0]["stale"]) == [(0, a), (1, a)] and trace[0]["fresh"] == [(2, b)]
    assert all(len(t["approved"]) == 0 for t in trace[1:])


def test_orders_differ_on_the_synthetic_fixture(fixture_clouds):
    literal, jacobi, _ = fixture_clouds
    nl, nj = len(literal[0]), len(jacobi[0])
    print("points: literal", nl, "jacobi", nj, "only literal", len(point_set(literal) - point_set(jacobi)),
          "only jacobi", len(point_set(jacobi) - point_set(literal)))
    assert nl > 1000 and nj > 1000
    assert point_set(literal) != point_set(jacobi)
    assert abs(nl - nj) <= 0.02 * nl


def test_trace_covers_fresh_and_stale_entries(fixture_clouds):
    _, _, trace = fixture_clouds
    fresh, stale = sum(len(t["fresh"]) for t in trace), sum(len(t["stale"]) for t in trace)
    print("applied used_list entries: fresh", fresh, "stale", stale)
    assert stale >= 100 and fresh >= 1000


def test_abi_has_the_jacobi_fusion():
    lib = _abi.load_library()
    assert "acmmp_run_fusion_jacobi" in _abi.SIGNATURES
    assert lib.acmmp_run_fusion_jacobi.argtypes[-2] is C.c_int  # device
    chunk = lib.acmmp_fusion_jacobi_scan_chunk()
    assert 64 <= chunk < 3511  # the stale-entry case's two pixels lie in different chunks


def test_no_usable_device_is_a_clean_error(tmp_path):
    """Device index = the number of devices (0 on a machine without a GPU, one
    past the last on one with): ACMMP_ERR_HIP with a message, no PLY."""
    d, out = _dense_with_maps(tmp_path)
    lib = _abi.load_library()
    with pytest.raises(AcmmpError) as err:
        pipeline.run_fusion(d, out, order="jacobi", device=lib.acmmp_device_count())
    assert "(status %d)" % _abi.ERR_HIP in str(err.value)
    assert lib.acmmp_fusion_last_error().decode().strip()
    assert not os.path.exists(os.path.join(out, "ACMMP_model.ply"))
    with pytest.raises(ValueError):
        pipeline.run_fusion(d, out, order="gauss")


def test_cli_refuses_a_bad_fusion_order(tmp_path):
    """Status 2 from the option itself, before any file is touched: the folder
    does not exist."""
    p = subprocess.run([EXE, str(tmp_path / "nowhere"), "--fusion", "bogus"], capture_output=True, text=True)
    assert p.returncode == 2
    assert "--fusion literal|jacobi" in p.stderr and "unknown option" not in p.stderr
    assert not os.path.exists(str(tmp_path / "nowhere"))
    p = subprocess.run([EXE, "--help"], capture_output=True, text=True)
    assert "--fusion literal|jacobi" in p.stdout
