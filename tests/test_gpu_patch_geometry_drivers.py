"""patch_size / radius_increment through the drivers: acmmp_process_problem's
pass options (pipeline.run_sequential), `acmmp_main --patch_size N
--radius_increment N` in both pass orders, and the Python view-parallel driver,
at 7 / 1 on a synthetic dense folder. Every .dmb is compared bit-exactly with
the oracle pipeline run with the same two parameters."""
import os
import subprocess

import pytest

import oracle_pipeline
from acmmp_amd import pipeline, scene
from acmmp_amd.distributed import ViewParallelPipeline
from oracle_pipeline import OraclePipeline
from test_gpu_pipeline import _compare

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "acmmp_amd", "lib", "acmmp_main")
PATCH = (7, 1)


@pytest.fixture(scope="module")
def dense(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("dense_patch"))
    sc = scene.make_scene(num_views=5, width=160, height=120)
    scene.write_dense_folder(sc, d, num_src=4)
    return d


@pytest.fixture(scope="module")
def oracle_maps(dense):
    """The oracle pipeline with its parameter set-up wrapped so that every run
    takes the patch geometry (both orders, computed once)."""
    mp = pytest.MonkeyPatch()
    plain = oracle_pipeline._params

    def with_patch(*a, **k):
        p = plain(*a, **k)
        p.patch_size, p.radius_increment = PATCH
        return p
    mp.setattr(oracle_pipeline, "_params", with_patch)
    try:
        maps = {order: OraclePipeline(dense).run_single_scale(order) for order in ("sequential", "jacobi")}
    finally:
        mp.undo()
    default = OraclePipeline(dense).process_problem(0, False, False, False, 0, {})
    assert not (default["depths"] == maps["sequential"][(0, "depths")]).all()  # the geometry changes the maps
    return maps


def test_process_problem_pass_options(dense, oracle_maps):
    out = pipeline.run_sequential(dense, "/PS71", write_triangulation=False, patch_size=PATCH[0],
                                  radius_increment=PATCH[1])
    assert _compare(out, oracle_maps["sequential"]) == 5 * 4


@pytest.mark.parametrize("order", ["sequential", "jacobi"])
def test_cli_both_orders(dense, oracle_maps, order):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    out = "/CLI71" + order
    r = subprocess.run([EXE, dense, "--patch_size", str(PATCH[0]), "--radius_increment", str(PATCH[1]), "--order",
                        order, "--output_dir", out, "--no_fusion", "--no_triangulation", "--quiet"],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert _compare(dense + out, oracle_maps[order]) == 5 * 4


def test_python_view_parallel_world1(dense, oracle_maps):
    out = ViewParallelPipeline(dense, "/VP71", device=0, patch_size=PATCH[0], radius_increment=PATCH[1]).run()
    assert _compare(out, oracle_maps["jacobi"]) == 5 * 4
