"""acmmp_view_size: the size of a view at a scale, from the image header and
InputInitialization's rescale rule (src/ACMMP.cpp:578-583: float factor,
std::round — halves away from zero; unchanged when both sides fit). It must be
the size acmmp_load_view produces and the size the test oracle's rescale
states, halves included: an even longer side and an odd shorter one give x.5
where the factor is exactly 0.5. CPU only: host code."""
import ctypes as C
import os

import numpy as np
import pytest

from acmmp_amd import _abi, scene
from acmmp_amd import io as aio
from oracle_pipeline import load_gray, rescale

# w, h, max_image_size, expected (w, h)
ROWS = [
    (1004, 753, 502, (502, 377)),     # 376.5
    (1002, 501, 501, (501, 251)),     # 250.5
    (2002, 1001, 1001, (1001, 501)),  # 500.5
    (1010, 760, 505, (505, 380)),     # the multi-scale fixtures: no half
    (1600, 1200, 800, (800, 600)),
    (753, 1004, 502, (377, 502)),     # portrait: the half on the width
    (96, 72, 6400, (96, 72)),         # fits: unchanged
]


def _std_round(x):
    """std::round of a positive float32: the fraction x - floor(x) is exact."""
    x = np.float32(x)
    lo = np.floor(x)
    return int(lo) + (1 if x - lo >= np.float32(0.5) else 0)


def _reference_size(w, h, m):
    """src/ACMMP.cpp:574-583 in float32."""
    if w <= m and h <= m:
        return w, h
    f32 = np.float32
    factor = min(f32(m) / f32(w), f32(m) / f32(h))
    return _std_round(f32(w) * factor), _std_round(f32(h) * factor)


def _folder(tmp_path, w, h):
    d = str(tmp_path / f"dense_{w}x{h}")
    scene.write_dense_folder(scene.make_scene(num_views=1, width=w, height=h), d, fmt="pgm")
    return d


def _load_view(dense, m):
    lib = _abi.load_library()
    cam = _abi.Camera()
    rc = lib.acmmp_load_view(dense.encode(), 0, m, None, 0, C.byref(cam))
    assert rc in (0, _abi.ERR_ARG), lib.acmmp_pipeline_last_error().decode()
    img = np.empty((cam.height, cam.width), dtype=np.float32)
    rc = lib.acmmp_load_view(dense.encode(), 0, m, img.ctypes.data_as(C.POINTER(C.c_float)), img.size, C.byref(cam))
    assert rc == 0, lib.acmmp_pipeline_last_error().decode()
    return img, cam


def _oracle_view(dense, m):
    img = load_gray(os.path.join(dense, "images", "00000000.pgm"))
    cam = aio.read_camera(os.path.join(dense, "cams", "00000000_cam.txt"))
    cam.height, cam.width = img.shape
    return rescale(img, cam, m)


@pytest.mark.parametrize("w,h,m,expected", ROWS)
def test_view_size_is_the_reference_rule(tmp_path, w, h, m, expected):
    assert _reference_size(w, h, m) == expected
    dense = _folder(tmp_path, w, h)
    assert aio.view_size(dense, 0, m) == expected
    assert aio.view_size(dense, 0, 0) == (w, h) == aio.view_size(dense, 0)
    img, cam = _load_view(dense, m)
    assert (cam.width, cam.height) == expected and img.shape == expected[::-1]
    oimg, ocam = _oracle_view(dense, m)
    assert oimg.shape == expected[::-1] and (ocam.width, ocam.height) == expected


@pytest.mark.parametrize("w,h,m,expected", ROWS[:2])
def test_load_view_equals_the_oracle_rescale_at_a_half(tmp_path, w, h, m, expected):
    """Pixels and K bit for bit: the oracle's rescale states what the library does."""
    dense = _folder(tmp_path, w, h)
    img, cam = _load_view(dense, m)
    oimg, ocam = _oracle_view(dense, m)
    np.testing.assert_array_equal(img.view(np.uint32), np.ascontiguousarray(oimg, np.float32).view(np.uint32))
    assert np.array_equal(np.array(list(cam.K), np.float32).view(np.uint32),
                          np.array(list(ocam.K), np.float32).view(np.uint32))
