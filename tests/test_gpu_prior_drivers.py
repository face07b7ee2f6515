"""Seeded priors (main_ACMMP -p, src/main_ACMMP.cpp:72-90, :107-120) in the
view-parallel drivers on the GPU: the Python driver
(acmmp_amd.distributed.ViewParallelPipeline(prior=True)) and the C++ one
(`acmmp_main -p --view_parallel`, `--order jacobi`), at world size 1 and with
two ranks sharing the box's one GPU (gloo / the TCP exchange), the tail view
whole or split in row bands. The first pass of the first scale starts from the
planes k_seed_planes builds on the device from the 16-bit prior PNGs; every
.dmb must equal the oracle pipeline's in Jacobi order bit for bit (NaN == NaN),
in the default output folder /ACMMP_PRIOR."""
import os
import shutil
import struct
import subprocess
import time
import zlib

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from acmmp_amd import scene
from acmmp_amd.distributed import ViewParallelPipeline
from oracle_pipeline import OraclePipeline
from parity_util import mismatch
from test_gpu_pipeline import _compare
from test_gpu_vp_cli import EXE, _free_port

pytestmark = pytest.mark.gpu

OUT = "/ACMMP_PRIOR"


def write_png16(path, arr):
    """16-bit PNG of arr, (H, W) gray or (H, W, 3) in RGB order: every row with
    filter 0, so the whole raster is one numpy byte view (the per-byte encoder
    of test_seeded_priors.py, which also covers the other filters, is too slow
    beyond small maps)."""
    a = np.asarray(arr)
    if a.ndim == 2:
        a = a[..., None]
    H, W, Cn = a.shape
    raw = np.ascontiguousarray(a.astype(">u2")).view(np.uint8).reshape(H, W * Cn * 2)
    rows = np.concatenate([np.zeros((H, 1), np.uint8), raw], axis=1)  # filter type 0 in front of each row

    def chunk(t, d):
        return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d) & 0xFFFFFFFF)

    png = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 16, {1: 0, 3: 2}[Cn], 0, 0, 0))
    png += chunk(b"IDAT", zlib.compress(rows.tobytes(), 1)) + chunk(b"IEND", b"")
    with open(path, "wb") as fh:
        fh.write(png)


def write_scene_priors(dense, sc):
    """The priors of test_gpu_pipeline.test_seeded_pipeline_matches_oracle:
    noisy ground-truth depth and the ground-truth normals of every view as
    16-bit words. Returns {problem index: (depth, normals in BGR)}."""
    os.makedirs(dense + "priors/depths", exist_ok=True)
    os.makedirs(dense + "priors/normals", exist_ok=True)
    rng = np.random.default_rng(5)
    priors = {}
    for i, v in enumerate(sc.views):
        dep = np.clip((v.depth - 300.0) / 500.0 * 65535.0 + rng.normal(0, 300, v.depth.shape), 0, 65535)
        dep = np.where(v.depth > 0, dep, 30000).astype(np.uint16)
        nrm = np.clip((v.normal + 1.0) * 32768.0, 0, 65535).astype(np.uint16)
        write_png16(dense + "priors/depths/%08d.png" % i, dep)
        write_png16(dense + "priors/normals/%08d.png" % i, nrm)
        priors[i] = (dep, nrm[..., ::-1])
    return priors


def _fresh(dense):
    """Every run writes the default folder: the previous run's is removed."""
    shutil.rmtree(dense + OUT, ignore_errors=True)


# ------------------------------------------------------------ the launchers
def _worker(rank, world, port, dense, q, split_tail):
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    try:
        pipe = ViewParallelPipeline(dense, device=0, tensor_device=torch.device("cuda", 0),
                                    comm_device=torch.device("cpu"), split_tail=split_tail, prior=True)
        out = pipe.run()
        q.put((rank, (out, pipe.owned, pipe.split)))
    finally:
        dist.destroy_process_group()


def _spawn_python(dense, split_tail, timeout=300):
    """The Python driver on 2 gloo ranks sharing GPU 0; {rank: (folder, owned, split)}."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, dense, q, split_tail)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        deadline = time.monotonic() + timeout
        while any(p.exitcode is None for p in procs):  # a failed rank ends the wait: its peer would block in gloo
            assert all(p.exitcode in (None, 0) for p in procs), [p.exitcode for p in procs]
            assert time.monotonic() < deadline, "the ranks did not finish in time"
            time.sleep(0.1)
        assert [p.exitcode for p in procs] == [0, 0]
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
    return dict(q.get(timeout=5) for _ in range(2))


def _launch_cli(dense, world, extra, timeout=400, check=True):
    """`world` ranks of acmmp_main on device 0 as test_gpu_vp_cli._launch starts
    them, without --output_dir: -p names the folder. Returns (code, out, err) per rank."""
    port = _free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port - 1), ACMMP_RDZV_PORT=str(port))
        cmd = [EXE, dense, "-p", "--device", "0", "--quiet"] + list(extra)
        procs.append(subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    outs = []
    try:
        for p in procs:
            so, se = p.communicate(timeout=timeout)
            outs.append((p.returncode, so, se))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    if check:
        for rc, so, se in outs:
            assert rc == 0, se[-3000:]
    return outs


# ------------------------------------------------------------- single scale
@pytest.fixture(scope="module")
def seeded(tmp_path_factory):
    """5 views at 160x120, 3 sources each: problems 1-3 take a source's
    camera for their seed (GetCamera(problem index)), problem 4 the camera-0
    fallback. (dense folder, oracle maps in Jacobi order)."""
    d = str(tmp_path_factory.mktemp("prior_vp")) + "/"
    sc = scene.make_scene(num_views=5, width=160, height=120)
    scene.write_dense_folder(sc, d, num_src=3)
    priors = write_scene_priors(d, sc)
    return d, OraclePipeline(d).run_single_scale("jacobi", priors=priors)


def test_the_seed_changes_the_first_pass(seeded):
    """The expectation is a seeded one: problem 0's first pass without the
    seed gives another depths.dmb (which no later pass rewrites)."""
    d, maps = seeded
    plain = OraclePipeline(d).process_problem(0, False, True, False, 0, {})
    assert mismatch(plain["depths"], maps[(0, "depths")]).any()


def test_python_world1(seeded):
    d, maps = seeded
    _fresh(d)
    out = ViewParallelPipeline(d, device=0, prior=True).run()
    assert out == d + OUT
    assert _compare(out, maps) == 5 * 4


@pytest.mark.parametrize("split_tail", [False, True])
def test_python_world2_gloo(seeded, split_tail):
    d, maps = seeded
    _fresh(d)
    got = _spawn_python(d, split_tail)
    assert got[0][0] == got[1][0] == d + OUT
    assert sorted(got[0][1] + got[1][1]) == list(range(5)) and got[0][1] and got[1][1]
    assert got[0][2] == got[1][2] == ([4] if split_tail else [])
    assert _compare(d + OUT, maps) == 5 * 4


def test_cli_world1_rccl(seeded):
    d, maps = seeded
    _fresh(d)
    _launch_cli(d, 1, ["--view_parallel", "--exchange", "rccl"])
    assert _compare(d + OUT, maps) == 5 * 4
    assert os.path.getsize(os.path.join(d + OUT, "ACMMP_model.ply")) > 1000  # RunFusion, as without --multi_fusion


@pytest.mark.parametrize("split", [True, False])
def test_cli_world2_tcp(seeded, split):
    d, maps = seeded
    _fresh(d)
    _launch_cli(d, 2, ["--view_parallel", "--exchange", "tcp"] + ([] if split else ["--no_split_tail"]))
    assert _compare(d + OUT, maps) == 5 * 4
    assert os.path.getsize(os.path.join(d + OUT, "ACMMP_model.ply")) > 1000  # rank 0 fused


def test_cli_order_jacobi(seeded):
    d, maps = seeded
    _fresh(d)
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run([EXE, d, "-p", "--order", "jacobi", "--quiet"], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert _compare(d + OUT, maps) == 5 * 4
    assert os.path.getsize(os.path.join(d + OUT, "ACMMP_model.ply")) > 1000


def test_cli_without_priors_prints_the_reference_message(tmp_path):
    d = str(tmp_path / "dense") + "/"
    sc = scene.make_scene(num_views=3, width=96, height=72)
    scene.write_dense_folder(sc, d, num_src=2)
    (rc, so, se), = _launch_cli(d, 1, ["--view_parallel"], timeout=120, check=False)
    assert "Initialisation from a prior was requested, but no suitable priors were found." in so
    assert "not supported" not in so + se
    assert rc == 255  # main_ACMMP's return -1 (src/main_ACMMP.cpp:86-89)
    assert not os.path.isdir(d + OUT)


# -------------------------------------------------------------- multi-scale
class SeededOraclePipeline(OraclePipeline):
    """run_multi_scale with -p: the first pass of the first scale is seeded
    (flag == 0, src/main_ACMMP.cpp:107-120), from the full-size prior maps at
    that scale's rows x cols and with that scale's cameras."""

    def __init__(self, dense, priors):
        super().__init__(dense)
        self.priors = priors
        self._first = True

    def run_pass(self, geom, planar, multi, seed_hi, order="sequential", hier=False, seeded=False):
        first, self._first = self._first, False
        super().run_pass(geom, planar, multi, seed_hi, order, hier, seeded=first)


@pytest.fixture(scope="module")
def seeded_ms(tmp_path_factory):
    """3 views at 1002x501, 1 source each: two scales, the first 501 wide and
    251 high (250.5 rows rounded by std::round, src/ACMMP.cpp:578-583). The
    prior maps are full size, so GetPriorPlaneEstimate's step is 501 / 251 = 1
    (integer division, src/acmmp_definitions.cpp:126) and the first scale is
    seeded from the maps' top-left 251 x 501 words: the reference's rule, kept.
    Problem 1 takes its source's camera, problem 2 the camera-0 fallback; at
    world 2 the third view is split in row bands."""
    d = str(tmp_path_factory.mktemp("prior_ms")) + "/"
    sc = scene.make_scene(num_views=3, width=1002, height=501)
    scene.write_dense_folder(sc, d, num_src=1)
    priors = write_scene_priors(d, sc)
    maps = SeededOraclePipeline(d, priors).run_multi_scale("jacobi")
    assert maps[(2, "depths_geom")].shape == (501, 1002)
    return d, maps


@pytest.mark.timeout(900)
def test_multi_scale_world2_split_tail_both_drivers(seeded_ms):
    d, maps = seeded_ms
    _fresh(d)
    got = _spawn_python(d, True, timeout=400)
    assert got[0][2] == got[1][2] == [2]
    assert _compare(d + OUT, maps) == 3 * 4
    _fresh(d)
    _launch_cli(d, 2, ["--view_parallel", "--exchange", "tcp", "--no_fusion"], timeout=400)
    assert _compare(d + OUT, maps) == 3 * 4
