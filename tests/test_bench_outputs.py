"""bench.py's options and its --dump-outputs writer: a plain run asks for
nothing beyond the timed steps, and the dump holds the pass results in
float32 at a pixel list that is complete within the budget and a fixed sample
beyond it. One GPU test runs a plain bench at a small size; the rest need no
GPU."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import bench  # conftest puts the repository root on sys.path


def test_plain_run_is_lean_and_full_is_opt_in():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, "", 7, 2)
    a = bench.parse(["--full", "--dump-outputs", "d"])
    assert a.full and a.dump_outputs == "d"


@pytest.mark.gpu
def test_plain_run_line_and_dump_match_the_resident_state(tmp_path):
    """A plain run at a small size: the line carries the headline fields and
    none of the --full blocks, --steps sets the timed steps, and the dump
    equals the per-view state the run holds at its end (the hidden --dump)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    d, per_view = str(tmp_path / "out"), str(tmp_path / "per_view")
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--width", "320", "--height", "240", "--iters", "2", "--dump-outputs", d, "--dump", per_view]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120, cwd=root)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert res["steps"] == 2 and res["ms_per_step"] > 0 and res["value"] > 0
    assert (res["unit"], res["higher_is_better"], res["dtype"]) == ("Mpix/s", True, "f32")
    assert res["metric"] == bench.BASELINE_METRIC
    assert "roofline" not in res and "cpu_baseline" not in res
    np.testing.assert_allclose(res["value"], 2 * 10 * 320 * 240 / (res["ms_per_step"] * 1e3), rtol=1e-3)
    got = _load(d)
    assert got["view_ids"].tolist() == list(range(10)) and got["pixels"].tolist() == list(range(320 * 240))
    for v in range(10):
        for name, shape in (("geom_planes", (240, 320, 4)), ("geom_costs", (240, 320)), ("photo_depth", (240, 320))):
            want = np.load(os.path.join(per_view, f"{name}_{v:03d}.npy"))
            assert got[name].dtype == np.float32 and np.isfinite(got[name]).all()
            want = _finite(want)  # the resident state marks a pixel without a cost by NaN
            np.testing.assert_array_equal(got[name][v].reshape(shape).view(np.uint32), want.view(np.uint32))


def _finite(a):
    return np.nan_to_num(a, nan=np.float32(bench.DUMP_NAN), posinf=np.float32(bench.DUMP_INF),
                         neginf=np.float32(-bench.DUMP_INF))


def _views(n, H, W):
    g = torch.Generator().manual_seed(5)
    return types.SimpleNamespace(planes=torch.rand((n, H, W, 4), generator=g), costs=torch.rand((n, H, W), generator=g),
                                 my_depth=torch.rand((n, H, W), generator=g))


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_whole_maps_within_budget(tmp_path):
    rv = _views(3, 7, 5)
    bench.dump_outputs(str(tmp_path / "o"), rv, [4, 5, 6])
    got = _load(str(tmp_path / "o"))
    assert sorted(got) == ["geom_costs", "geom_planes", "photo_depth", "pixels", "view_ids"]
    assert got["view_ids"].tolist() == [4, 5, 6] and got["pixels"].tolist() == list(range(35))
    assert all(got[k].dtype == np.float32 for k in ("geom_costs", "geom_planes", "photo_depth"))
    np.testing.assert_array_equal(got["geom_planes"], rv.planes.numpy().reshape(3, 35, 4))
    np.testing.assert_array_equal(got["geom_costs"], rv.costs.numpy().reshape(3, 35))
    np.testing.assert_array_equal(got["photo_depth"], rv.my_depth.numpy().reshape(3, 35))


def test_dump_outputs_are_finite(tmp_path):
    """NaN (a pixel without a cost) and infinities are saved as the finite
    stand-ins, which no cost, normal or depth takes; the rest is unchanged."""
    rv = _views(2, 6, 4)
    rv.costs[0, 1, 2] = float("nan")
    rv.costs[1, 5, 3] = float("inf")
    rv.planes[1, 0, 0, 3] = float("-inf")
    rv.my_depth[0, 0, 0] = float("nan")
    bench.dump_outputs(str(tmp_path / "o"), rv, [0, 1])
    got = _load(str(tmp_path / "o"))
    assert all(np.isfinite(v).all() for v in got.values())
    assert got["geom_costs"][0, 1 * 4 + 2] == np.float32(bench.DUMP_NAN) and bench.DUMP_NAN < -1
    assert got["geom_costs"][1, 5 * 4 + 3] == np.float32(bench.DUMP_INF)
    assert got["geom_planes"][1, 0, 3] == np.float32(-bench.DUMP_INF)
    assert got["photo_depth"][0, 0] == np.float32(bench.DUMP_NAN)
    np.testing.assert_array_equal(got["geom_costs"], _finite(rv.costs.numpy().reshape(2, 24)))

def test_dump_outputs_samples_beyond_budget(tmp_path, monkeypatch):
    rv = _views(2, 33, 17)
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4000)
    bench.dump_outputs(str(tmp_path / "a"), rv, [0, 1])
    bench.dump_outputs(str(tmp_path / "b"), _views(2, 33, 17), [0, 1])
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    pix = a["pixels"].astype(np.int64)
    assert 0 < len(pix) < 33 * 17 and (np.diff(pix) > 0).all() and pix.max() < 33 * 17
    assert sum(v.nbytes for v in a.values()) <= 4000 + a["view_ids"].nbytes
    for k in a:  # the same sample and the same values from run to run
        np.testing.assert_array_equal(a[k], b[k])
    np.testing.assert_array_equal(a["geom_planes"], rv.planes.numpy().reshape(2, -1, 4)[:, pix])
    np.testing.assert_array_equal(a["photo_depth"], rv.my_depth.numpy().reshape(2, -1)[:, pix])
