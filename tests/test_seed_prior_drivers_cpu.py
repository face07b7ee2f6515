"""Seeded priors (main_ACMMP -p, src/main_ACMMP.cpp:72-90, :107-120) in the
view-parallel Python driver, without a GPU: ViewParallelPipeline(prior=True)
with the stand-in engine of test_distributed_cpu.py on CPU tensors, at world
size 1 and over gloo at world size 2. The first pass's tasks must carry the
seeded planes of pSampler::GetPriorPlaneEstimate (src/acmmp_definitions.cpp:
99-177) for the camera GetCamera(problem index) picks, bit for bit against the
oracle restatement; no later pass may carry any."""
import os
import queue
import time

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import oracle
from acmmp_amd import AcmmpError, scene
from acmmp_amd import io as aio
from acmmp_amd.distributed import ViewParallelPipeline
from test_distributed_cpu import _free_port, fake_compute, fake_jbu
from test_seeded_priors import _write_priors

W, H, VIEWS = 96, 72, 4


def _prior_arrays(i):
    """Depth words and normal words (RGB order, as written) of camera i."""
    rng = np.random.default_rng(100 + i)
    depth = rng.integers(0, 65536, size=(H, W), dtype=np.uint16)
    n = rng.normal(size=(H, W, 3))
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    return depth, np.clip((n + 1.0) * 32768.0, 0, 65535).astype(np.uint16)


@pytest.fixture(scope="module")
def dense(tmp_path_factory):
    """4 views, 2 sources each: problems 1 and 2 take a source's camera,
    problem 3 the camera-0 fallback (3 >= num_images). The planes depend on
    the camera's intrinsics and depth range only, which the synthetic scene
    shares between its views: each camera file is rewritten with its own
    (fx != fy, shifted principal point, own depth range), so a wrong camera
    gives other planes."""
    d = str(tmp_path_factory.mktemp("seed_cpu")) + "/"
    sc = scene.make_scene(num_views=VIEWS, width=W, height=H)
    scene.write_dense_folder(sc, d, fmt="pgm", num_src=2)
    for i, v in enumerate(sc.views):
        K = np.array(v.K, dtype=np.float64)
        K[0, 0] *= 1.0 + 0.05 * i
        K[1, 1] *= 1.0 - 0.03 * i
        K[0, 2] += 1.5 * i
        K[1, 2] -= 2.25 * i
        aio.write_camera(os.path.join(d, "cams", "%08d_cam.txt" % i), K, v.R, v.t, 300.0 + 20.0 * i, 2.5, 192.0,
                         800.0 + 30.0 * i)
    for i in range(VIEWS):
        _write_priors(d, i, *_prior_arrays(i))
    return d


def _expected(dense):
    """{problem index: oracle planes} with GetCamera(idx) of the problem's own camera list."""
    out = {}
    for idx, pr in enumerate(aio.read_pair(os.path.join(dense, "pair.txt"))):
        ids = [pr.ref_image_id] + list(pr.src_image_ids)
        cam = aio.read_camera(os.path.join(dense, "cams", "%08d_cam.txt" % (ids[idx] if idx < len(ids) else ids[0])))
        cam.height, cam.width = H, W
        depth, normals_rgb = _prior_arrays(idx)
        out[idx] = oracle.prior_plane_estimate(depth, normals_rgb[..., ::-1], cam, H, W)
    return out


def _run(dense, log, **kw):
    def compute(t, eng=None):
        log.append((t.index, t.seed_hi, None if t.seed_planes is None else t.seed_planes.cpu().numpy().copy()))
        return fake_compute(t, eng)

    pipe = ViewParallelPipeline(dense, compute=compute, jbu=fake_jbu, tensor_device=torch.device("cpu"),
                                prior=True, **kw)
    return pipe.run()


def _check(log, expected):
    first = {v: planes for v, seed_hi, planes in log if seed_hi == 0}
    assert sorted(first) == sorted(expected)
    for v, planes in first.items():
        assert planes is not None, f"view {v}: the first pass carries no seed planes"
        assert planes.dtype == np.float32 and planes.shape == (H, W, 4)
        np.testing.assert_array_equal(planes.view(np.uint32), expected[v].view(np.uint32), err_msg=f"view {v}")
    later = [(v, seed_hi) for v, seed_hi, planes in log if seed_hi > 0 and planes is not None]
    assert not later, f"later passes carry seed planes: {later}"
    assert sum(1 for _, seed_hi, _ in log if seed_hi > 0) == 2 * len(expected)  # the two geometric passes ran


def test_cameras_cover_the_quirk(dense):
    """The scene exercises all three cases of GetCamera(problem index)."""
    problems = aio.read_pair(os.path.join(dense, "pair.txt"))
    assert [len(p.src_image_ids) for p in problems] == [2] * VIEWS
    exp = _expected(dense)
    # a source's camera gives other planes than the reference's would
    pr = problems[1]
    cam = aio.read_camera(os.path.join(dense, "cams", "%08d_cam.txt" % pr.ref_image_id))
    cam.height, cam.width = H, W
    depth, normals_rgb = _prior_arrays(1)
    own = oracle.prior_plane_estimate(depth, normals_rgb[..., ::-1], cam, H, W)
    assert (own.view(np.uint32) != exp[1].view(np.uint32)).any()


def test_world1_first_pass_tasks_carry_the_seed(dense):
    log = []
    out = _run(dense, log)
    assert out == dense + "/ACMMP_PRIOR" and os.path.isdir(out)
    assert os.path.exists(os.path.join(aio.result_folder(out, VIEWS - 1), "depths_geom.dmb"))
    _check(log, _expected(dense))


def _worker(rank, world, port, dense, q):
    os.environ.setdefault("OMP_NUM_THREADS", "1")
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    try:
        log = []
        out = _run(dense, log)
        q.put((rank, out, log))
    finally:
        dist.destroy_process_group()


def test_world2_gloo_first_pass_tasks_carry_the_seed(dense):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, dense, q)) for r in range(2)]
    for p in procs:
        p.start()
    # read before join (a queue's feeder holds its process until the log is read), but never wait for a rank that failed
    got, deadline = [], time.monotonic() + 300
    while len(got) < 2:
        try:
            got.append(q.get(timeout=0.5))
        except queue.Empty:
            assert all(p.exitcode in (None, 0) for p in procs), [p.exitcode for p in procs]
            assert time.monotonic() < deadline
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    logs = {rank: log for rank, _, log in got}
    assert all(out == dense + "/ACMMP_PRIOR" for _, out, _ in got)
    assert logs[0] and logs[1]  # both ranks computed views
    assert not {v for v, _, _ in logs[0]} & {v for v, _, _ in logs[1]}
    _check(logs[0] + logs[1], _expected(dense))


def test_folder_without_priors_raises_the_reference_message(tmp_path):
    d = str(tmp_path / "dense") + "/"
    sc = scene.make_scene(num_views=3, width=W, height=H)
    scene.write_dense_folder(sc, d, fmt="pgm", num_src=2)
    message = "Initialisation from a prior was requested, but no suitable priors were found"
    with pytest.raises(AcmmpError, match=message):
        ViewParallelPipeline(d, compute=fake_compute, jbu=fake_jbu, tensor_device=torch.device("cpu"), prior=True)
    # without the flag the same folder is accepted and the default folder is the reference's
    pipe = ViewParallelPipeline(d, compute=fake_compute, jbu=fake_jbu, tensor_device=torch.device("cpu"))
    assert pipe.output_folder == d + "/ACMMP" and not pipe.prior
