"""acmmp_export_results' depth (include/acmmp.h) after every writer of the
result planes. A full run leaves the depths in a plane of their own, which
the export copies; any other writer of the planes (the plane-hypothesis and
hierarchy setters, a band run, a resize) must send the export back to the
planes' .w channel, or it hands the geometric pass the previous run's depths
without any error. Every case writes, after a run, state that differs from
the run's depths at every pixel, and compares bit for bit (uint32 views)."""
import numpy as np
import pytest
import torch

from acmmp_amd import ACMMP, AcmmpError, _abi, default_params, scene

pytestmark = pytest.mark.gpu

W, H = 160, 120


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _export(eng):
    """(planes, depth) as acmmp_export_results writes them into torch tensors."""
    w, h = eng.size
    planes = torch.full((h, w, 4), -1.0, dtype=torch.float32, device="cuda:0")
    depth = torch.full((h, w), -1.0, dtype=torch.float32, device="cuda:0")
    eng.export_results(planes.data_ptr(), 0, depth.data_ptr())
    eng.synchronize()
    return planes.cpu().numpy(), depth.cpu().numpy()


@pytest.fixture(scope="module")
def problem():
    return scene.make_scene(num_views=5, width=W, height=H).problem(0, 4)


@pytest.fixture
def ran(problem):
    """An engine after one full run, and that run's depths."""
    p = default_params()
    p.max_iterations = 1
    with ACMMP(0) as eng:
        eng.set_params(p)
        eng.set_images(*problem)
        eng.RunPatchMatch()
        yield eng, eng.plane_hypotheses()[..., 3].copy()


def _new_planes(first, base):
    """Planes whose depth is base + pixel index: outside the scene's depth
    range, so different from the run's depth at every pixel."""
    pl = np.zeros((H, W, 4), np.float32)
    pl[..., 2] = 1.0
    pl[..., 3] = base + np.arange(H * W, dtype=np.float32).reshape(H, W)
    assert (_bits(pl[..., 3]) != _bits(first)).all()
    return pl


def test_full_run(ran):
    eng, first = ran
    planes, depth = _export(eng)
    assert _same(planes, eng.plane_hypotheses())
    assert _same(depth, first)


@pytest.mark.parametrize("device_src", [False, True], ids=["host", "device"])
def test_run_then_set_plane_hypotheses(ran, device_src):
    eng, first = ran
    pl = _new_planes(first, 1000.0)
    costs = np.full((H, W), 0.5, np.float32)
    if device_src:
        d_pl, d_co = torch.from_numpy(pl).cuda(), torch.from_numpy(costs).cuda()
        eng.set_plane_hypotheses_device(d_pl.data_ptr(), d_co.data_ptr())
    else:
        eng.set_plane_hypotheses(pl, costs)
    planes, depth = _export(eng)
    assert _same(depth, pl[..., 3])
    assert _same(planes, pl)


@pytest.mark.parametrize("device_src", [False, True], ids=["host", "device"])
def test_run_then_set_hierarchy_inputs(ran, device_src):
    eng, first = ran
    up = _new_planes(first, 2000.0)[..., 3].copy()
    scaled = np.zeros((H // 2, W // 2, 4), np.float32)
    if device_src:
        d_sc, d_up = torch.from_numpy(scaled).cuda(), torch.from_numpy(up).cuda()
        eng.set_hierarchy_inputs_device(d_sc.data_ptr(), W // 2, H // 2, d_up.data_ptr())
    else:
        eng.set_hierarchy_inputs(scaled, up)
    planes, depth = _export(eng)
    assert _same(depth, up)
    assert _same(planes[..., 3], up)
    assert not _bits(planes[..., :3]).any()


def test_run_then_band_run(ran):
    eng, first = ran
    # one participant, no neighbours: the halo rows are the band's own init
    eng.run_band(40, 80, exchange=lambda halo: None)
    planes, depth = _export(eng)
    now = eng.plane_hypotheses()
    assert _same(planes, now)
    assert _same(depth, now[..., 3])
    assert (_bits(depth[40:80]) != _bits(first[40:80])).any()  # the band run did write new depths


def test_run_then_refused_run(ran):
    eng, first = ran
    eng.update_params(geom_consistency=1)  # no depth maps: refused on the host, nothing launched
    with pytest.raises(AcmmpError, match=f"status {_abi.ERR_STATE}:"):
        eng.RunPatchMatch()
    planes, depth = _export(eng)
    assert _same(depth, eng.plane_hypotheses()[..., 3])
    assert _same(depth, first)


def test_run_then_resize(ran):
    eng, _ = ran
    eng.set_images(*scene.make_scene(num_views=5, width=96, height=64).problem(0, 4))
    planes, depth = _export(eng)
    assert planes.shape == (64, 96, 4) and depth.shape == (64, 96)
    assert not _bits(planes).any() and not _bits(depth).any()
