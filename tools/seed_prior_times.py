"""What the seeded set-up (-p) costs per view in the view-parallel driver.

The first pass of a multi-scale run is the seeded one (src/main_ACMMP.cpp:
107-120): for 1600x1200 views it runs at 800x600 and its seed planes come from
the full-size 16-bit prior PNGs (pSampler::GetPriorPlaneEstimate,
src/acmmp_definitions.cpp:99-177). This tool times that pass of
acmmp_amd.distributed.ViewParallelPipeline at world 1, seeded and unseeded in
interleaved rounds (the same folder, views and keys; .dmb writing off), and
the parts of the seeded set-up of one view on their own:

  png_read   pipeline.read_prior_maps: the two PNGs decoded to 16-bit words
  upload     the words to the device (torch copy, synchronised)
  kernel     acmmp_seed_planes_device (HIP events around repeated launches)
  setter     acmmp_set_seed_prior_device (device-to-device copy, synchronised)

and the host path the sequential driver takes for the same view:
acmmp_prior_plane_estimate (PNG decode + the plane loop on one host thread)
and acmmp_set_seed_prior (synchronous 16 B / pixel upload).

Synthetic scene rendered on the GPU; priors are the rendered depth and normals
from its gradient (realistic entropy for the PNG decoder).
usage: python tools/seed_prior_times.py [views] [width] [height] [nsrc] [rounds] [out.json]
"""
import json
import os
import shutil
import statistics
import struct
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from acmmp_amd import ACMMP, pipeline, scene  # noqa: E402
from acmmp_amd.distributed import DepthExchange, ViewParallelPipeline  # noqa: E402
from acmmp_amd.engine import seed_planes_device  # noqa: E402

_argv = sys.argv if __name__ == "__main__" else []
V = int(_argv[1]) if len(_argv) > 1 else 4
W = int(_argv[2]) if len(_argv) > 2 else 1600
H = int(_argv[3]) if len(_argv) > 3 else 1200
NSRC = int(_argv[4]) if len(_argv) > 4 else 3
ROUNDS = int(_argv[5]) if len(_argv) > 5 else 3
OUT = _argv[6] if len(_argv) > 6 else os.path.join(ROOT, "profiles", "seed_prior_times.json")
DEV = torch.device("cuda", 0)


def write_png16(path, arr):
    """16-bit PNG, (H, W) gray or (H, W, 3) RGB, filter 0 on every row."""
    a = arr if arr.ndim == 3 else arr[..., None]
    h, w, c = a.shape
    raw = np.ascontiguousarray(a.astype(">u2")).view(np.uint8).reshape(h, w * c * 2)
    rows = np.concatenate([np.zeros((h, 1), np.uint8), raw], axis=1)

    def chunk(t, d):
        return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d) & 0xFFFFFFFF)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 16, {1: 0, 3: 2}[c], 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)) + chunk(b"IEND", b""))


def write_dense():
    """The dense folder (trailing '/': the reference appends "priors" to it) with priors of every view."""
    setup = scene.scene_setup(num_views=V, width=W, height=H, arc_deg=1.8)
    views, maps = [], []
    for i in range(V):
        img, dep = scene.render_torch(setup, i, DEV, with_depth=True)
        R, t, _, _ = setup.poses[i]
        views.append(scene.View(K=setup.K.astype(np.float32), R=R.astype(np.float32), t=t.astype(np.float32),
                                image=img.cpu().numpy(), depth=None, normal=None))
        z = torch.where(dep > 0, dep, torch.full_like(dep, 600.0))
        gy, gx = torch.gradient(z)
        n = torch.stack([gx, gy, -torch.full_like(z, 0.2)], -1)  # (a camera-frame normal from the depth gradient)
        n = n / n.norm(dim=-1, keepdim=True)
        words = ((z - 300.0) / 500.0 * 65535.0).clamp(0, 65535).to(torch.int32).cpu().numpy().astype(np.uint16)
        maps.append((words, ((n + 1.0) * 32768.0).clamp(0, 65535).to(torch.int32).cpu().numpy().astype(np.uint16)))
    tmp = tempfile.mkdtemp(prefix="acmmp_seed_")
    dense = os.path.join(tmp, "dense") + "/"
    scene.write_dense_folder(scene.Scene(views=views, pairs=setup.pairs), dense, num_src=NSRC)
    for kind in ("depths", "normals"):
        os.makedirs(dense + "priors/" + kind)
    for i, (d, n) in enumerate(maps):
        write_png16(dense + "priors/depths/%08d.png" % i, d)
        write_png16(dense + "priors/normals/%08d.png" % i, n)
    return tmp, dense


def first_pass(dense, prior):
    """(wall seconds of the first pass, its seeded set-up's share, the loaded pipeline)."""
    pipe = ViewParallelPipeline(dense, "/T", device=0, write_outputs=False, prior=prior)
    pipeline.scale_step(pipe.problems)
    pipe._load_views()
    exchange = DepthExchange(pipe.assignment, pipe._shapes(), pipe.cdev, pipe.group, out_device=pipe.tdev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if prior:
        pipe._load_seed_planes()
    t1 = time.perf_counter()
    pipe.run_pass(False, True, False, False, exchange, seeded=prior)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, t1 - t0, pipe


def parts(dense, pipe):
    """The seeded set-up of view 0 piece by piece, and the host path, in ms."""
    p = pipe.problems[0]
    ids = [p.ref_image_id] + p.sources
    cam = pipe.cams[ids[0]]
    rows, cols = cam.height, cam.width
    out = {}
    t0 = time.perf_counter()
    depth, normals = pipeline.read_prior_maps(dense, 0)
    out["png_read_ms"] = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    d = torch.from_numpy(depth.view(np.int16)).to(DEV)
    n = torch.from_numpy(normals.view(np.int16)).to(DEV)
    torch.cuda.synchronize()
    out["upload_ms"] = (time.perf_counter() - t0) * 1e3
    planes = torch.empty((rows, cols, 4), dtype=torch.float32, device=DEV)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    args = (d.data_ptr(), depth.shape[1], depth.shape[0], 1, n.data_ptr(), normals.shape[1], normals.shape[0], cam,
            rows, cols, planes.data_ptr(), 0, stream)
    seed_planes_device(*args)  # warm
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps = 50
    e0.record()
    for _ in range(reps):
        seed_planes_device(*args)
    e1.record()
    torch.cuda.synchronize()
    out["kernel_ms"] = e0.elapsed_time(e1) / reps
    with ACMMP(0) as eng:
        eng.set_images_device([pipe.cams[i] for i in ids], [pipe.images[i].data_ptr() for i in ids],
                              [pipe.images[i].stride(0) for i in ids])
        eng.synchronize()
        eng.set_seed_prior_device(planes.data_ptr())  # allocates the seed buffer
        eng.synchronize()
        t0 = time.perf_counter()
        eng.set_seed_prior_device(planes.data_ptr())
        eng.synchronize()
        out["setter_ms"] = (time.perf_counter() - t0) * 1e3
        # the parent's path: host estimate (decode + loop), synchronous upload
        t0 = time.perf_counter()
        host = pipeline.prior_plane_estimate(dense, 0, cam, rows, cols)
        out["host_prior_plane_estimate_ms"] = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        eng.SetPlanarPrior(host)
        out["host_set_seed_prior_ms"] = (time.perf_counter() - t0) * 1e3
    out["identical_to_host"] = bool((planes.cpu().numpy().view(np.uint32) == host.view(np.uint32)).all())
    out["pass_shape"] = [rows, cols]
    out["prior_shape"] = list(depth.shape[:2])
    return out


def main():
    tmp, dense = write_dense()
    try:
        first_pass(dense, True)[2]._shutdown()  # warm: file cache, device pools, code objects
        rounds, part_rounds = [], []
        for _ in range(ROUNDS):
            plain, _, pipe = first_pass(dense, False)
            pipe._shutdown()
            seeded, setup, pipe = first_pass(dense, True)
            part_rounds.append(parts(dense, pipe))
            pipe._shutdown()
            rounds.append({"unseeded_s": plain, "seeded_s": seeded, "seed_setup_s": setup})
        med = statistics.median
        keys = [k for k, v in part_rounds[0].items() if isinstance(v, float)]
        res = {"what": "first pass of a view-parallel run at world 1, seeded (-p) and unseeded, interleaved rounds",
               "views": V, "width": W, "height": H, "nsrc": NSRC, "rounds": ROUNDS,
               "pass_shape": part_rounds[0]["pass_shape"], "prior_shape": part_rounds[0]["prior_shape"],
               "unseeded_pass_s": round(med(r["unseeded_s"] for r in rounds), 4),
               "seeded_pass_s": round(med(r["seeded_s"] for r in rounds), 4),
               "seeded_extra_ms_per_view": round(med((r["seeded_s"] - r["unseeded_s"]) / V for r in rounds) * 1e3, 3),
               "seed_setup_ms_per_view": round(med(r["seed_setup_s"] / V for r in rounds) * 1e3, 3),
               "one_view_ms": {k: round(med(p[k] for p in part_rounds), 4) for k in keys},
               "identical_to_host": all(p["identical_to_host"] for p in part_rounds),
               "per_round": [{k: round(v, 4) for k, v in r.items()} for r in rounds]}
        print(json.dumps(res), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
        with open(OUT, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
