"""Fusion of device-resident maps (acmmp_fuse_views_jacobi):
RunFusion's rule in Jacobi order over views whose depth / normal maps, colours
and initial masks already lie in HBM as torch tensors, the cloud returned as
device tensors. `pipeline.run_fusion(order="jacobi")` is the same rule over a
folder; point k here is the point it puts k-th in its PLY.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Optional, Sequence

import numpy as np
import torch

from . import _abi
from .engine import AcmmpError


@dataclass
class FusionView:
    """One view: its camera at the maps' size (width / height are taken from
    the maps), its sources as indices into the list of views, and its maps.

    depth   (H, W) float32, element strides (W * s, s): s = 1 for a depth
            plane, 4 for the .w of an (H, W, 4) planes tensor
    normal  (H, W, 3) float32 world normals, strides (W * s, s, 1): s = 3 for a
            normal map, 4 for the xyz of a planes tensor
    bgr     optional (H, W, 3) uint8, B, G, R (None: colour 0, 0, 0)
    mask    optional (H, W) uint8 or bool, nonzero = masked before view 0
    """
    cam: _abi.Camera
    sources: Sequence[int]
    depth: torch.Tensor
    normal: torch.Tensor
    bgr: Optional[torch.Tensor] = None
    mask: Optional[torch.Tensor] = None
    keep: list = field(default_factory=list, repr=False)  # tensors made contiguous for the call

    @classmethod
    def from_planes(cls, planes_hw4: torch.Tensor, cam: _abi.Camera, sources: Sequence[int],
                    bgr: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None) -> "FusionView":
        """Over one (H, W, 4) tensor of world normal xyz + depth (what a
        PatchMatch run leaves on the device): strides 4 / 4, nothing copied."""
        if planes_hw4.ndim != 3 or planes_hw4.shape[2] != 4 or not planes_hw4.is_contiguous():
            raise AcmmpError(f"planes must be a contiguous (H, W, 4) tensor, not {tuple(planes_hw4.shape)}")
        return cls(cam, sources, planes_hw4[..., 3], planes_hw4[..., :3], bgr, mask)


def _pixel_stride(t: torch.Tensor, name: str, channels: int) -> int:
    """The stride, in elements, between neighbouring pixels of a map."""
    H, W = t.shape[:2]
    s = t.stride(1) if W > 1 else (t.stride(0) if H > 1 else max(channels, 1))
    want = (W * s, s) + ((1,) if channels > 1 else ())
    ok = all(t.shape[d] == 1 or t.stride(d) == want[d] for d in range(t.ndim))
    if not ok or s < channels:
        raise AcmmpError(f"{name}: strides {tuple(t.stride())} are not a pixel-strided {tuple(t.shape)} map")
    return s


def c_views(views: Sequence[FusionView], device: int = 0):
    """The views as the C-ABI's array (acmmp_fusion_view), checked: shapes,
    dtypes, device and strides. The tensors must outlive the call."""
    if not len(views):
        raise AcmmpError("no views to fuse")
    arr = (_abi.FusionView * len(views))()
    for i, v in enumerate(views):
        if v.depth.ndim != 2 or v.normal.ndim != 3 or tuple(v.normal.shape) != tuple(v.depth.shape) + (3,):
            raise AcmmpError(f"view {i}: depth {tuple(v.depth.shape)} and normal {tuple(v.normal.shape)} "
                             "must be (H, W) and (H, W, 3)")
        H, W = v.depth.shape
        tensors = {"depth": v.depth, "normal": v.normal}
        for name in ("bgr", "mask"):
            t = getattr(v, name)
            if t is None:
                continue
            if t.dtype == torch.bool:
                t = t.to(torch.uint8)
            if t.dtype != torch.uint8 or tuple(t.shape) != ((H, W, 3) if name == "bgr" else (H, W)):
                raise AcmmpError(f"view {i}: {name} must be uint8 of the maps' size")
            if not t.is_contiguous():
                t = t.contiguous()
            v.keep.append(t)
            tensors[name] = t
        for name, t in tensors.items():
            if not t.is_cuda or t.device.index != device:
                raise AcmmpError(f"view {i}: {name} is on {t.device}, not on cuda:{device}")
        if v.depth.dtype != torch.float32 or v.normal.dtype != torch.float32:
            raise AcmmpError(f"view {i}: depth and normal must be float32")
        if len(v.sources) > 32:
            raise AcmmpError(f"view {i}: {len(v.sources)} sources, at most 32")
        a = arr[i]
        C.memmove(C.byref(a.cam), C.byref(v.cam), C.sizeof(_abi.Camera))
        a.cam.width, a.cam.height = W, H
        a.num_src = len(v.sources)
        for j, s in enumerate(v.sources):
            a.src[j] = int(s)
        a.d_depth = v.depth.data_ptr()
        a.depth_stride = _pixel_stride(v.depth, f"view {i}: depth", 1)
        a.d_normal = v.normal.data_ptr()
        a.normal_stride = _pixel_stride(v.normal, f"view {i}: normal", 3)
        a.d_bgr = tensors["bgr"].data_ptr() if "bgr" in tensors else None
        a.d_mask = tensors["mask"].data_ptr() if "mask" in tensors else None
    return arr


def fuse_views(views: Sequence[FusionView], consistency_scalar: float = 0.3, num_consistent_thresh: int = 1,
               capacity: Optional[int] = None, device: int = 0):
    """Fuses the views on HIP device `device`; returns (xyz (n, 3) float32,
    normal (n, 3) float32, rgb (n, 3) uint8) as device tensors trimmed to the
    number of points. capacity=None allocates for the sum of the views' pixels
    (a cloud has at most one point a pixel); a smaller capacity that the cloud
    exceeds raises AcmmpError, which names both numbers. Runs on torch's
    current stream of the device, so whatever produced the inputs on it is
    ordered before the fusion; the call returns with the cloud complete."""
    lib = _abi.load_library()
    arr = c_views(views, device)
    if capacity is None:
        capacity = sum(int(v.depth.shape[0]) * int(v.depth.shape[1]) for v in views)
    dev = torch.device("cuda", device)
    xyz = torch.empty((capacity, 3), dtype=torch.float32, device=dev)
    normal = torch.empty((capacity, 3), dtype=torch.float32, device=dev)
    rgb = torch.empty((capacity, 3), dtype=torch.uint8, device=dev)
    out = _abi.CloudBuffers(xyz.data_ptr(), normal.data_ptr(), rgb.data_ptr(), capacity)
    n = C.c_int64(0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    rc = lib.acmmp_fuse_views_jacobi(device, arr, len(views), float(consistency_scalar), int(num_consistent_thresh),
                                     C.byref(out), C.c_void_p(stream), C.byref(n))
    if rc != 0:
        raise AcmmpError(f"fuse_views failed (status {rc}): {lib.acmmp_fusion_last_error().decode()}")
    if n.value > capacity:  # (capacity 0 only counts)
        raise AcmmpError(f"fuse_views: the fusion produced {n.value} points, capacity is {capacity}")
    return xyz[:n.value], normal[:n.value], rgb[:n.value]


def _host(a, dtype) -> np.ndarray:
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=dtype).reshape(-1, 3)


def write_ply(path: str, xyz, normal, rgb) -> int:
    """The cloud (tensors or arrays: (n, 3) float32, float32, uint8 r, g, b)
    as the binary PLY RunFusion writes (acmmp_write_ply_points); returns n."""
    lib = _abi.load_library()
    x, nr, c = _host(xyz, np.float32), _host(normal, np.float32), _host(rgb, np.uint8)
    if not len(x) == len(nr) == len(c):
        raise AcmmpError(f"write_ply: {len(x)} points, {len(nr)} normals, {len(c)} colours")
    fp = C.POINTER(C.c_float)
    rc = lib.acmmp_write_ply_points(path.encode(), x.ctypes.data_as(fp), nr.ctypes.data_as(fp),
                                    c.ctypes.data_as(C.POINTER(C.c_uint8)), len(x))
    if rc != 0:
        raise AcmmpError(f"write_ply failed (status {rc}): {lib.acmmp_fusion_last_error().decode()}")
    return len(x)


def resize_bilinear_u8(img: np.ndarray, width: int, height: int) -> np.ndarray:
    """The fusions' stand-in for cv::resize on an 8-bit (H, W[, C]) image
    (acmmp_resize_bilinear_u8)."""
    lib = _abi.load_library()
    src = np.ascontiguousarray(img, dtype=np.uint8)
    ch = 1 if src.ndim == 2 else src.shape[2]
    dst = np.empty((height, width) + src.shape[2:], dtype=np.uint8)
    u8 = C.POINTER(C.c_uint8)
    rc = lib.acmmp_resize_bilinear_u8(src.ctypes.data_as(u8), src.shape[1], src.shape[0], ch, dst.ctypes.data_as(u8),
                                      width, height)
    if rc != 0:
        raise AcmmpError(f"resize_bilinear_u8 failed (status {rc}): {lib.acmmp_fusion_last_error().decode()}")
    return dst


def initial_mask(path: str, width: int, height: int) -> np.ndarray:
    """RunFusion's initial mask of one view (src/acmmp_definitions.cpp:
    881-905) as load_initial_mask (acmmp_fusion_host.h) forms it: the PNG as
    cv::imread(path, -1) gives it, resized to the maps' size if it differs
    (8-bit only), `< 128`, and read as byte c of row r — for a colour mask
    that is channel c % C of pixel c / C. (height, width) uint8, 1 = masked."""
    lib = _abi.load_library()
    w, h, ch, bd = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
    rc = lib.acmmp_read_png(path.encode(), None, 0, C.byref(w), C.byref(h), C.byref(ch), C.byref(bd))
    if rc not in (0, _abi.ERR_ARG) or w.value <= 0:
        raise AcmmpError(f"Couldn't find mask image {path}")
    px = np.empty((h.value, w.value, ch.value), dtype=np.uint16)
    rc = lib.acmmp_read_png(path.encode(), px.ctypes.data_as(C.POINTER(C.c_uint16)), px.size, C.byref(w),
                            C.byref(h), C.byref(ch), C.byref(bd))
    if rc != 0:
        raise AcmmpError(f"Couldn't find mask image {path}")
    if ch.value == 2:  # gray + alpha: the gray value
        px = px[..., :1]
    if (w.value, h.value) != (width, height):
        if bd.value != 8:
            raise AcmmpError(f"16-bit mask {path} needs resizing")
        px = resize_bilinear_u8(px.astype(np.uint8), width, height).reshape(height, width, -1)
    return (px.reshape(height, -1)[:, :width] < 128).astype(np.uint8)
