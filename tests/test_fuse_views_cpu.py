"""The host side of the in-memory fusion (acmmp_fuse_views_jacobi, DESIGN.md
§8) without a GPU: the argument checks, which come before any device call,
acmmp_write_ply_points against the PLY the literal fusion writes,
acmmp_resize_bilinear_u8 against the oracle's resize, and the Python driver's
argument checks."""
import ctypes as C
import os

import numpy as np
import pytest

from acmmp_amd import _abi, AcmmpError
from acmmp_amd import pipeline
from oracle_fusion import _resize_u8, read_ply
from test_fusion import _dense_with_maps

FAKE = 0x10000  # a device address the host never reads


@pytest.fixture(scope="module")
def lib():
    return _abi.load_library()


def _views(n=3, w=40, h=30):
    arr = (_abi.FusionView * n)()
    for i in range(n):
        v = arr[i]
        v.cam.width, v.cam.height = w, h
        v.num_src = n - 1
        for j, s in enumerate(x for x in range(n) if x != i):
            v.src[j] = s
        v.d_depth, v.depth_stride = FAKE, 1
        v.d_normal, v.normal_stride = FAKE, 3
    return arr


def _call(lib, arr, count, out=None, with_count=True, device=0):
    n = C.c_int64(-7)
    rc = lib.acmmp_fuse_views_jacobi(device, arr, count, 0.3, 1, None if out is None else C.byref(out), None,
                                     C.byref(n) if with_count else None)
    return rc, lib.acmmp_fusion_last_error().decode()


def _set(field, value, view=1):
    def change(arr):
        obj = arr[view]
        *path, last = field.split(".")
        for name in path:
            obj = getattr(obj, name)
        setattr(obj, last, value)
    return change


def _bad_source(arr):
    arr[2].src[1] = 3


def _negative_source(arr):
    arr[0].src[0] = -1


BAD_VIEWS = {
    "num_src_below_0": _set("num_src", -1),
    "num_src_above_32": _set("num_src", 33),
    "source_index_at_count": _bad_source,
    "source_index_negative": _negative_source,
    "zero_width": _set("cam.width", 0),
    "negative_height": _set("cam.height", -30),
    "above_2_27_pixels": _set("cam.width", (1 << 27) // 30 + 1),
    "null_depth": _set("d_depth", None),
    "null_normal": _set("d_normal", None),
    "depth_stride_0": _set("depth_stride", 0),
    "normal_stride_2": _set("normal_stride", 2),
}


@pytest.mark.parametrize("case", sorted(BAD_VIEWS))
def test_bad_view_is_err_arg_with_a_message(lib, case):
    arr = _views()
    BAD_VIEWS[case](arr)
    rc, msg = _call(lib, arr, 3)
    assert rc == _abi.ERR_ARG and msg, (rc, msg)


def test_bad_call_arguments_are_err_arg(lib):
    arr = _views()
    for count in (0, -1):
        rc, msg = _call(lib, arr, count)
        assert rc == _abi.ERR_ARG and "count" in msg
    rc, msg = _call(lib, None, 3)
    assert rc == _abi.ERR_ARG and "views" in msg
    rc, msg = _call(lib, arr, 3, with_count=False)
    assert rc == _abi.ERR_ARG and "num_points" in msg
    rc, msg = _call(lib, arr, 3, out=_abi.CloudBuffers(FAKE, None, FAKE, 10))
    assert rc == _abi.ERR_ARG and msg


def test_limits_themselves_are_accepted_then_no_device(lib, has_gpu):
    """2^27 pixels, 32 sources (a view may list itself), strides 4 / 4 and a
    counting call pass the checks; the next thing the call needs is a device
    (one that does not exist: device 0 where there is none, else a number no
    machine has)."""
    device = 1 << 20 if has_gpu else 0
    arr = _views()
    arr[1].cam.width, arr[1].cam.height = 1 << 14, 1 << 13
    arr[0].num_src = 32
    for j in range(32):
        arr[0].src[j] = j % 3
    arr[2].num_src = 0
    arr[2].depth_stride = arr[2].normal_stride = 4
    for out in (None, _abi.CloudBuffers(None, None, None, 0), _abi.CloudBuffers(FAKE, FAKE, FAKE, 5)):
        rc, msg = _call(lib, arr, 3, out=out, device=device)
        assert rc == _abi.ERR_HIP and "device" in msg, (rc, msg)


# ---- acmmp_write_ply_points

def _write_points(lib, path, xyz, nrm, rgb):
    fp = C.POINTER(C.c_float)
    xyz, nrm, rgb = (np.ascontiguousarray(a) for a in (xyz, nrm, rgb))
    return lib.acmmp_write_ply_points(str(path).encode(), xyz.ctypes.data_as(fp), nrm.ctypes.data_as(fp),
                                      rgb.ctypes.data_as(C.POINTER(C.c_uint8)), len(xyz))


@pytest.fixture(scope="module")
def literal_ply(tmp_path_factory):
    d, out = _dense_with_maps(tmp_path_factory.mktemp("ply"))
    n = pipeline.run_fusion(d, out)
    path = os.path.join(out, "ACMMP_model.ply")
    assert n > 1000
    return open(path, "rb").read(), read_ply(path)


def _arrays(ply):
    return (np.stack([ply["x"], ply["y"], ply["z"]], -1).astype(np.float32),
            np.stack([ply["nx"], ply["ny"], ply["nz"]], -1).astype(np.float32),
            np.stack([ply["r"], ply["g"], ply["b"]], -1).astype(np.uint8))


@pytest.mark.parametrize("chunk", [None, "257"])
def test_write_ply_points_round_trip(lib, literal_ply, tmp_path, monkeypatch, chunk):
    """The literal fusion's PLY, rewritten from its own arrays: the same bytes,
    also with chunks of 257 points (the file is several chunks, the last one
    partial)."""
    data, ply = literal_ply
    if chunk:
        monkeypatch.setenv("ACMMP_PLY_CHUNK_POINTS", chunk)
        assert len(ply) > 3 * 257 and len(ply) % 257
    path = tmp_path / "again.ply"
    assert _write_points(lib, path, *_arrays(ply)) == 0
    assert path.read_bytes() == data


def test_write_ply_points_zeroes_non_finite_points(lib, literal_ply, tmp_path):
    _, ply = literal_ply
    xyz, nrm, rgb = (a[:9].copy() for a in _arrays(ply))
    xyz[1, 0], xyz[3, 1], xyz[4, 2], xyz[6, 2] = np.inf, -np.inf, np.nan, np.inf
    want = xyz.copy()
    want[[1, 3, 4, 6]] = 0
    path = tmp_path / "nf.ply"
    assert _write_points(lib, path, xyz, nrm, rgb) == 0
    got = _arrays(read_ply(str(path)))
    np.testing.assert_array_equal(got[0].view(np.uint32), want.view(np.uint32))
    np.testing.assert_array_equal(got[1].view(np.uint32), nrm.view(np.uint32))
    np.testing.assert_array_equal(got[2], rgb)


def test_write_ply_points_empty_and_bad_arguments(lib, tmp_path):
    path = tmp_path / "empty.ply"
    assert lib.acmmp_write_ply_points(str(path).encode(), None, None, None, 0) == 0
    assert len(read_ply(str(path))) == 0 and path.read_bytes().endswith(b"end_header\n")
    assert lib.acmmp_write_ply_points(str(path).encode(), None, None, None, 3) == _abi.ERR_ARG
    assert lib.acmmp_write_ply_points(None, None, None, None, 0) == _abi.ERR_ARG
    xyz = np.zeros((1, 3), np.float32)
    assert _write_points(lib, tmp_path / "no_such_folder" / "x.ply", xyz, xyz, np.zeros((1, 3), np.uint8)) == _abi.ERR_IO


def test_python_write_ply_matches(literal_ply, tmp_path):
    from acmmp_amd import fusion
    data, ply = literal_ply
    path = str(tmp_path / "py.ply")
    assert fusion.write_ply(path, *_arrays(ply)) == len(ply)
    assert open(path, "rb").read() == data


# ---- acmmp_resize_bilinear_u8

@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("size", [(100, 50), (140, 70)])
def test_resize_bilinear_u8_matches_oracle(lib, size, channels):
    rng = np.random.default_rng(3)
    src = rng.integers(0, 256, (67, 131, channels), dtype=np.uint8)
    dw, dh = size
    dst = np.full((dh, dw, channels), 7, np.uint8)
    u8 = C.POINTER(C.c_uint8)
    assert lib.acmmp_resize_bilinear_u8(src.ctypes.data_as(u8), 131, 67, channels, dst.ctypes.data_as(u8), dw, dh) == 0
    np.testing.assert_array_equal(dst, _resize_u8(src, dw, dh))
    from acmmp_amd import fusion
    np.testing.assert_array_equal(fusion.resize_bilinear_u8(src[..., 0] if channels == 1 else src, dw, dh),
                                  dst[..., 0] if channels == 1 else dst)
    assert lib.acmmp_resize_bilinear_u8(src.ctypes.data_as(u8), 131, 67, 5, dst.ctypes.data_as(u8), dw, dh) == _abi.ERR_ARG
    assert lib.acmmp_resize_bilinear_u8(None, 131, 67, channels, dst.ctypes.data_as(u8), dw, dh) == _abi.ERR_ARG


# ---- the Python driver's argument checks

def test_fuse_before_run_and_above_world_1_are_rejected(tmp_path):
    from acmmp_amd import scene
    from acmmp_amd.distributed import ViewParallelPipeline
    d = str(tmp_path / "dense")
    scene.write_dense_folder(scene.make_scene(num_views=3, width=48, height=36), d, num_src=2)
    pipe = ViewParallelPipeline(d, compute=lambda t, eng: None, write_outputs=False)
    with pytest.raises(AcmmpError, match="run\\(\\) first"):
        pipe.fuse()
    pipe.world = 2
    with pytest.raises(AcmmpError, match="pipeline.run_fusion"):
        pipe.fuse()


def test_fusion_view_strides():
    """from_planes is strides 4 / 4 over the one tensor; separate maps are 1 / 3."""
    import torch
    from acmmp_amd import fusion
    planes = torch.zeros((5, 7, 4))
    v = fusion.FusionView.from_planes(planes, _abi.Camera(), [])
    assert v.depth.data_ptr() == planes.data_ptr() + 12 and v.normal.data_ptr() == planes.data_ptr()
    assert fusion._pixel_stride(v.depth, "depth", 1) == 4 and fusion._pixel_stride(v.normal, "normal", 3) == 4
    assert fusion._pixel_stride(torch.zeros((5, 7)), "depth", 1) == 1
    assert fusion._pixel_stride(torch.zeros((5, 7, 3)), "normal", 3) == 3
    with pytest.raises(AcmmpError):
        fusion._pixel_stride(torch.zeros((7, 5)).t(), "depth", 1)
    with pytest.raises(AcmmpError):
        fusion.FusionView.from_planes(torch.zeros((5, 7, 3)), _abi.Camera(), [])
