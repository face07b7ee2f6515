"""k_seed_planes (acmmp_seed_planes_device) and acmmp_set_seed_prior_device on
the GPU: the seeded planes of pSampler::GetPriorPlaneEstimate
(src/acmmp_definitions.cpp:99-177) built on the device from decoded 16-bit
prior maps, against the oracle restatement and the host loop
(pipeline.prior_plane_estimate), and the engine's device setter against the
oracle run and the host setter. Every comparison is on bit patterns
(NaN == NaN)."""
import numpy as np
import pytest
import torch

import oracle
from acmmp_amd import ACMMP, AcmmpError, _abi, make_camera, pipeline
from acmmp_amd.engine import seed_planes_device
from parity_util import assert_bit_exact
from test_gpu_parity import _cam_planes_from_truth, _params, small_scene  # noqa: F401 (fixture)
from test_gpu_prior_drivers import write_png16

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def _camera(cols, rows, general):
    """The camera of test_seeded_priors.py, or one with fx != fy and the
    principal point off the centre."""
    if general:
        K = [[131.25, 0, 0.31 * cols + 2.75], [0, 97.5, 0.64 * rows - 1.5], [0, 0, 1]]
        return make_camera(K, np.eye(3), np.zeros(3), cols, rows, 287.5, 912.25)
    return make_camera([[100.0, 0, 7.5], [0, 100.0, 5.5], [0, 0, 1]], np.eye(3), np.zeros(3), cols, rows, 300.0, 800.0)


def _maps(seed, dh, dw, dc, nh, nw, scale):
    """Random depth words (dh, dw[, dc]) and unit normals as words, both as the
    reader returns them (channels in B, G, R order), with the edge values
    planted where a view with step `scale` samples: depth words 0 and 65535,
    the zero normal (32768, 32768, 32768), and a normal on either side of the
    flip."""
    rng = np.random.default_rng(seed)
    depth = rng.integers(0, 65536, size=(dh, dw) if dc == 1 else (dh, dw, dc), dtype=np.uint16)
    n = rng.normal(size=(nh, nw, 3))
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    normals = np.clip((n + 1.0) * 32768.0, 0, 65535).astype(np.uint16)
    s = scale
    if s:  # (step 0 samples (0, 0) alone)
        for (r, c), word in (((s, 2 * s), 0), ((2 * s, s), 65535), ((3 * s, 3 * s), 30000), ((3 * s, 2 * s), 30000)):
            depth.reshape(-1)[r * dw * dc + c] = word  # the word the loop reads, whatever the channel count
        normals[2 * s, 2 * s] = 32768
        normals[3 * s, 3 * s] = (32768, 32768, 0)      # (0, 0, -1): faces the camera, kept
        normals[3 * s, 2 * s] = (32768, 32768, 65535)  # (0, 0, ~1): faces away, flipped
    return depth, normals


def _write_priors(tmp_path, cam_num, depth_read, normals_bgr):
    """The two PNGs of camera cam_num (a PNG stores R, G, B); returns the dense folder."""
    dense = str(tmp_path / "dense") + "/"
    for kind, arr in (("depths", depth_read), ("normals", normals_bgr)):
        (tmp_path / "dense" / "priors" / kind).mkdir(parents=True, exist_ok=True)
        write_png16(dense + "priors/%s/%08d.png" % (kind, cam_num), arr if arr.ndim == 2 else arr[..., ::-1])
    return dense


def _device_planes(depth, normals_bgr, cam, rows, cols, stream=None, fill=None):
    """seed_planes_device on uploaded words; (rows, cols, 4) float32 back on the host."""
    d = torch.from_numpy(np.ascontiguousarray(depth).view(np.int16)).to(DEV)
    n = torch.from_numpy(np.ascontiguousarray(normals_bgr).view(np.int16)).to(DEV)
    out = torch.full((rows, cols, 4), float("nan") if fill is None else fill, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize(DEV)
    dh, dw = depth.shape[:2]
    try:
        seed_planes_device(d.data_ptr(), dw, dh, 1 if depth.ndim == 2 else depth.shape[2], n.data_ptr(),
                           normals_bgr.shape[1], normals_bgr.shape[0], cam, rows, cols, out.data_ptr(), 0, stream)
    finally:
        torch.cuda.synchronize(DEV)
    return out.cpu().numpy()


# rows, cols, prior rows, prior cols, depth channels, general camera
CASES = {
    "12x16_step1": (12, 16, 12, 16, 1, False),
    "12x16_step2": (12, 16, 24, 32, 1, False),
    # 64 x 4 blocks: 3 x 10 of them, neither side a multiple; 113 = 3 * 37 + 2, 452 = 3 * 150 + 2
    "37x150_step3_blocks": (37, 150, 113, 452, 1, True),
    "12x16_step2_depth_rgb": (12, 16, 24, 32, 3, True),
    "12x16_step0_small_prior": (12, 16, 5, 7, 1, True),
    "12x16_step1_general_camera": (12, 16, 12, 16, 1, True),
}


@pytest.mark.parametrize("case", list(CASES))
def test_kernel_matches_oracle_and_host(tmp_path, case):
    rows, cols, dh, dw, dc, general = CASES[case]
    scale = dh // rows
    depth_read, normals_bgr = _maps(len(case), dh, dw, dc, dh, dw, scale)
    cam = _camera(cols, rows, general)
    dense = _write_priors(tmp_path, 3, depth_read, normals_bgr)
    rd, rn = pipeline.read_prior_maps(dense, 3)
    np.testing.assert_array_equal(rd, depth_read)
    np.testing.assert_array_equal(rn, normals_bgr)

    ref = oracle.prior_plane_estimate(depth_read, normals_bgr, cam, rows, cols)
    host = pipeline.prior_plane_estimate(dense, 3, cam, rows, cols)
    got = _device_planes(depth_read, normals_bgr, cam, rows, cols)
    assert_bit_exact(host, ref, f"{case}: host loop vs oracle")
    assert_bit_exact(got, ref, f"{case}: kernel vs oracle")
    assert_bit_exact(got, host, f"{case}: kernel vs host loop")
    assert not np.isnan(got).any()

    if scale == 0:  # every pixel samples word (0, 0): only the pixel coordinates vary
        assert len(np.unique(got[..., :3].reshape(-1, 3), axis=0)) <= 2  # the normal, or its flip
        return
    # the sampled words hold the edge values, and they come out as the host's rule says
    ys, xs = np.mgrid[0:rows, 0:cols]
    words = depth_read.reshape(-1)[(ys * scale) * dw * dc + xs * scale]
    assert words.min() == 0 and words.max() == 65535
    sampled = normals_bgr[ys * scale, xs * scale]
    zero = (sampled == 32768).all(-1)
    assert zero.any()
    assert (got[zero][:, :3] == 0).all() and (got[zero][:, 3] == 0).all()  # the zero normal: a zero plane
    assert (got[3, 3, :3] == np.float32([0, 0, -1])).all()  # facing the camera: kept
    assert -1 < got[3, 2, 2] < 0                            # facing away: flipped (and scaled by its norm)
    n = sampled.astype(np.float32) * np.float32(2.0 / 65536.0) + np.float32(-1.0)
    flipped = np.sign(got[..., 2]) != np.sign(n[..., 2])
    assert flipped[~zero].any() and (~flipped[~zero]).any()


@pytest.mark.parametrize("what,dh,dw,nh,nw", [
    ("columns", 24, 20, 24, 20),        # step 2: column 30 of 20
    ("normal_rows", 24, 32, 20, 32),    # step 2: normal row 22 of 20
    ("normal_columns", 24, 32, 24, 30),  # step 2: normal column 30 of 30
])
def test_maps_too_small_are_refused_before_any_launch(tmp_path, what, dh, dw, nh, nw):
    rows, cols = 12, 16
    rng = np.random.default_rng(7)
    depth = rng.integers(0, 65536, size=(dh, dw), dtype=np.uint16)
    normals_bgr = rng.integers(0, 65536, size=(nh, nw, 3), dtype=np.uint16)
    cam = _camera(cols, rows, True)
    d = torch.from_numpy(depth.view(np.int16)).to(DEV)
    n = torch.from_numpy(np.ascontiguousarray(normals_bgr).view(np.int16)).to(DEV)
    out = torch.full((rows, cols, 4), -7.0, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize(DEV)
    with pytest.raises(AcmmpError) as dev_err:
        seed_planes_device(d.data_ptr(), dw, dh, 1, n.data_ptr(), nw, nh, cam, rows, cols, out.data_ptr(), 0)
    torch.cuda.synchronize(DEV)
    assert dev_err.value.status == _abi.ERR_ARG
    message = f"prior maps {dw}x{dh} smaller than {cols}x{rows}"
    assert message in str(dev_err.value)
    assert (out.cpu().numpy() == -7.0).all()  # nothing was written
    # the host function's message for the same maps
    dense = _write_priors(tmp_path, 0, depth, normals_bgr)
    with pytest.raises(AcmmpError) as host_err:
        pipeline.prior_plane_estimate(dense, 0, cam, rows, cols)
    assert message in str(host_err.value)


def test_bad_arguments_are_refused():
    cam = _camera(16, 12, False)
    out = torch.zeros((12, 16, 4), dtype=torch.float32, device=DEV)
    for args in ((0, 16, 12, 1, out.data_ptr(), 16, 12, cam, 12, 16, out.data_ptr()),
                 (out.data_ptr(), 16, 12, 1, out.data_ptr(), 16, 12, cam, 0, 16, out.data_ptr()),
                 (out.data_ptr(), 16, 12, 0, out.data_ptr(), 16, 12, cam, 12, 16, out.data_ptr())):
        with pytest.raises(AcmmpError) as e:
            seed_planes_device(*args)
        assert e.value.status == _abi.ERR_ARG


def test_engine_device_setter_matches_oracle_and_host_setter(small_scene):  # noqa: F811
    """The scene and comparison of test_gpu_parity.test_seeded_init, the seed
    set from a device buffer."""
    cams, imgs = small_scene.problem(5, 4)
    seed = _cam_planes_from_truth(small_scene.views[5], cams[0])
    d_seed = torch.from_numpy(seed).to(DEV)
    with ACMMP(0) as eng:
        eng.set_params(_params(2))
        eng.set_images(cams, imgs)
        eng.set_seed_prior_device(d_seed.data_ptr())
        prm = eng.params
        eng.RunPatchMatch()
        got = (eng.plane_hypotheses(), eng.costs())
        # a second seed on the same engine goes into the same buffer: the run repeats
        eng.set_params(prm)
        eng.set_seed_prior_device(d_seed.data_ptr())
        eng.RunPatchMatch()
        again = (eng.plane_hypotheses(), eng.costs())
    assert prm.seeded == 1
    ref = oracle.run_patchmatch(prm, cams, imgs, seed_planes=seed)
    assert_bit_exact(got[0], ref["planes"], "planes")
    assert_bit_exact(got[1], ref["costs"], "costs")
    assert_bit_exact(again[0], got[0], "planes, second run")
    assert_bit_exact(again[1], got[1], "costs, second run")
    with ACMMP(0) as eng:
        eng.set_params(_params(2))
        eng.set_images(cams, imgs)
        eng.SetPlanarPrior(seed)
        eng.RunPatchMatch()
        host = (eng.plane_hypotheses(), eng.costs())
    assert_bit_exact(got[0], host[0], "planes vs the host setter")
    assert_bit_exact(got[1], host[1], "costs vs the host setter")


def test_engine_device_setter_needs_images():
    with ACMMP(0) as eng:
        with pytest.raises(AcmmpError):
            eng.set_seed_prior_device(0)
