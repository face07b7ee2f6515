"""The HIP kernels' RunPatchMatch against the independent restatement of the
sweep's decision layer (tests/ref_sweep.py, written from src/ACMMP.cu's lines),
bit for bit, every pixel, NaN == NaN.

The restatement takes its cost primitives from the engine under test
(eval_costs / eval_geom_costs, pinned against float64 by
test_gpu_general_rig.py), so what is compared is the kernels' decision logic:
sampling regions, view selection, accept rules, refinement, hierarchy gate,
init branches, RNG draw order. The oracle comparison stands beside it, so a
failure names the side that is wrong.

Cases: those of test_sweep_restated_cpu.py, and the shapes only the device
has: 10 sources (the per-view path above 9) and 20 (the 32-source kernels),
the general patch path, patch 7 / 1, and each texel form.
The engine has no pre_costs input: its pre_costs are what an earlier pass on
the same engine left, as in the pass drivers. The same-size hierarchy cases
therefore run as a second pass after an upsample pass, whose init writes
pre_costs (:681); the restatement and the oracle get that pass's pre_costs, so
the gate passes and blocks here as on the CPU tier.
"""
import numpy as np
import pytest

import ref_sweep as rs
from acmmp_amd import ACMMP
from parity_util import mismatch

pytestmark = pytest.mark.gpu

_KEYS = ("selected_views", "planes", "costs")


def _install(eng, prob, images=True):
    mine = prob.prm
    eng.set_params(mine)
    if images:
        eng.set_images(prob.cams, prob.images)
    if prob.depths is not None:
        eng.set_depth_maps(prob.depths)
    if mine.hierarchy:
        eng.set_hierarchy_inputs(prob.scaled_planes, prob.planes[..., 3])
    elif prob.planes is not None:
        eng.set_plane_hypotheses(prob.planes, prob.costs)
    if mine.planar_prior:
        eng.CudaPlanarPriorInitialization(prob.prior_planes.reshape(-1, 4), prob.masks)
    if mine.seeded:
        eng.SetPlanarPrior(prob.seed_planes)


def _upsample_pass(eng):
    """A first hierarchy pass on `eng` (the hier_up case): returns the
    pre_costs its init left on the engine, as the restatement computes them
    from the engine's eval_costs and as the oracle does."""
    up = rs.make_case("hier_up")
    _install(eng, up)
    up.prm = eng.params
    eng.RunPatchMatch()
    first = rs.SweepRestated(up, rs.EngineBackend(eng))
    first.init()
    assert not mismatch(first.pre_costs, rs.run_oracle(up)["pre_costs"]).any()
    return first.pre_costs


def _run(name, nsrc=3, after_upsample=False, **kw):
    """Engine run, restatement on the engine's primitives, oracle run."""
    with ACMMP(0) as eng:
        if after_upsample:   # the second run of this engine: stream 1, the first pass's pre_costs
            kw.update(pre_costs=_upsample_pass(eng), rng_stream=1)
        prob = rs.make_case(name, nsrc=nsrc, **kw)
        mine = prob.prm
        _install(eng, prob, images=not after_upsample)
        prm = eng.params
        fields = ["depth_min", "depth_max", "num_images", "hierarchy", "upsample", "seeded", "planar_prior",
                  "geom_consistency", "patch_size", "radius_increment", "seed_lo", "rng_stream", "max_iterations"]
        for f in fields + (["scaled_cols", "scaled_rows"] if mine.upsample else []):
            assert getattr(prm, f) == getattr(mine, f), f   # the engine runs the problem the case describes
        prob.prm = prm
        bits = eng.texel_bits()
        eng.RunPatchMatch()
        got = {"planes": eng.plane_hypotheses(), "costs": eng.costs(), "selected_views": eng.selected_views()}
        out = rs.run_restated(prob, rs.EngineBackend(eng))
    ref = rs.run_oracle(prob)
    bad = lambda a, b: sum(int(mismatch(a[k], b[k]).sum()) for k in _KEYS)
    k_r, k_o, o_r = bad(got, out), bad(got, ref), bad(ref, out)
    kw.pop("pre_costs", None)
    print(f"{name} nsrc={nsrc} {kw}: words differing kernels/restated {k_r}, kernels/oracle {k_o}, "
          f"oracle/restated {o_r}")
    if k_r or k_o or o_r:
        side = ("the kernels" if k_r and k_o and not o_r else
                "the oracle" if k_o and o_r and not k_r else
                "the restatement (or a misreading shared by oracle and kernels)" if k_r and o_r and not k_o else
                "more than one side")
        first = next(k for k in _KEYS if mismatch(got[k], out[k]).any() or mismatch(got[k], ref[k]).any())
        idx = np.argwhere(mismatch(got[first], out[first]) | mismatch(got[first], ref[first]))[0]
        raise AssertionError(
            f"{name}: {side} stands alone: kernels/restated {k_r}, kernels/oracle {k_o}, oracle/restated {o_r} "
            f"words differ; first in {first} at {idx.tolist()}: kernels {got[first][tuple(idx)]}, "
            f"restated {out[first][tuple(idx)]}, oracle {ref[first][tuple(idx)]}")
    return prob, out, rs.coverage(out["traces"]), bits


@pytest.mark.parametrize("name", ["photo", "small37", "small9", "geom", "planar", "hier_up", "hier_swap",
                                  "hier_seeded"])
def test_cases_of_the_cpu_tier(name):
    prob, out, cov, _ = _run(name, after_upsample=name in ("hier_swap", "hier_seeded"))
    if name != "small9":
        assert min(cov["region"]) >= 0.01 and min(cov["hyp"]) > 0 and min(cov["branch"]) >= 0.05, cov
    if name == "planar":
        assert cov["planar_accept"] > 0.05 and cov["plain_accept"] > 0.05 and cov["shadowed"] > 0.05
    if name.startswith("hier"):
        assert cov["gate_pass"] >= 0.10 and cov["gate_block"] >= 0.10
        assert (out["pre_costs"] != 0).all() and prob.prm.rng_stream == (0 if name == "hier_up" else 1)


@pytest.mark.parametrize("nsrc", [10, 20])
@pytest.mark.parametrize("name", ["photo45", "geom"])
def test_more_sources_than_the_small_builds(name, nsrc):
    """45x33, 1 iteration: 10 sources take the per-view path above 9, 20 the
    32-source kernels."""
    prob, out, cov, _ = _run(name, nsrc=nsrc)
    assert out["traces"][0].weights.shape[1] == nsrc
    used = np.concatenate([t.weights for t in out["traces"]]).sum(0)
    assert (used > 0).all()                 # every source is sampled somewhere


def test_general_patch_path_at_default_geometry(monkeypatch):
    monkeypatch.setenv("ACMMP_GENERAL_PATCH", "1")
    _run("photo45")


def test_patch_7_step_1():
    prob, _, _, _ = _run("photo45", patch_size=7, radius_increment=1)
    assert (prob.prm.patch_size, prob.prm.radius_increment) == (7, 1)


@pytest.mark.parametrize("form,bits", [("u8", 8), ("h16", 16), ("f32", 32)])
def test_texel_forms(monkeypatch, form, bits):
    monkeypatch.setenv("ACMMP_TEXEL", form)
    assert _run("photo45")[3] == bits
