"""The CPU oracle's RunPatchMatch against the independent restatement of its
decision layer (tests/ref_sweep.py, written from src/ACMMP.cu's lines): planes,
costs and selected views bit for bit, every pixel, NaN == NaN.

Both sides take the cost primitives from oracle.eval_costs /
eval_geom_costs (pinned against float64 by test_oracle_kat.py and
test_general_rig_cpu.py), so what is compared is everything between them:
the sampling regions, the view selection, the weighted, geometric and
posterior costs, the accept rules, the refinement, the hierarchy gate, the
init branches and the order of the RNG's draws.

Each case asserts from the restatement's trace that its inputs reach the
rules it is there for; the sensitivity test changes one rule at a time and
requires the oracle to notice.
"""
import functools

import numpy as np
import pytest

import ref_sweep as rs
from parity_util import assert_bit_exact, mismatch

@functools.lru_cache(maxsize=None)
def _case(name):
    prob = rs.make_case(name)
    ref = rs.run_oracle(prob)
    out = rs.run_restated(prob)
    return prob, ref, out


def _assert_equal(name):
    prob, ref, out = _case(name)
    assert_bit_exact(ref["selected_views"], out["selected_views"], f"{name}: selected views (oracle vs restated)")
    assert_bit_exact(ref["planes"], out["planes"], f"{name}: planes (oracle vs restated)")
    assert_bit_exact(ref["costs"], out["costs"], f"{name}: costs (oracle vs restated)")
    if prob.prm.hierarchy:
        assert_bit_exact(ref["pre_costs"], out["pre_costs"], f"{name}: pre_costs")
    return prob, out, rs.coverage(out["traces"])


def _assert_sweep_coverage(cov):
    """The shares every swept case must reach (conditions on the inputs)."""
    print({k: ([round(x, 4) for x in v] if isinstance(v, list) else round(v, 4)) for k, v in cov.items()})
    assert min(cov["region"]) >= 0.01, cov["region"]        # each region supplies >= 1 % of accepted candidates
    assert min(cov["hyp"]) > 0, cov["hyp"]                  # each refinement hypothesis accepted somewhere
    assert min(cov["branch"]) >= 0.05, cov["branch"]        # weighted, fallback and zero-probability, >= 5 % each


def test_photometric_random_init_two_iterations():
    """53x49, 3 sources, 2 iterations: full strips exist, iter 1 lowers the
    threshold (:1011) and draws from phase 2."""
    prob, out, cov = _assert_equal("photo")
    _assert_sweep_coverage(cov)
    assert {t.it for t in out["traces"]} == {0, 1} and len(out["traces"]) == 4
    assert rs.cost_threshold(1) < rs.cost_threshold(0)
    table = rs.sampling_table()
    assert all(len(rs.region_samples(table, r, 24, 26, 49, 53)) == 11 for r in (1, 3, 5, 7))
    draws = np.concatenate([t.draws for t in out["traces"]])
    # 15 view draws, depth_rand, k >= 1 rejection pairs, the perturbed depth, three perturbation angles
    assert draws.min() == 22 and draws.max() >= 28 and np.all(draws % 2 == 0)
    assert (out["restated"].branch_init == 0).all()


def test_photometric_small_37x33_skips_the_last_row():
    prob, out, cov = _assert_equal("small37")
    _assert_sweep_coverage(cov)
    table = rs.sampling_table()
    assert not any(all(len(rs.region_samples(table, r, y, x, 33, 37)) == 11 for r in (1, 3, 5, 7))
                   for y in range(33) for x in range(37))
    assert max(t.ys.max() for t in out["traces"]) == 31 and rs.sweep_rows(33) == 32
    assert any((t.flags & (t.pos_y == 32)).any() for t in out["traces"])


def test_photometric_small_9x7_every_strip_truncated():
    """9x7: no strip holds more than three samples and two of the four are
    absent for most pixels; with 63 pixels the shares of the larger cases mean
    nothing here (about 97 % of the pixels accept no candidate whatever the RNG
    key, and the fallback branch stays below 5 %): the case is about the
    truncated sets and the {2.0f} array."""
    prob, out, cov = _assert_equal("small9")
    table = rs.sampling_table()
    assert max(len(rs.region_samples(table, r, y, x, 7, 9)) for r in (1, 3, 5, 7)
               for y in range(7) for x in range(9)) == 3
    flags = np.concatenate([t.flags for t in out["traces"]])
    assert (~flags).any(axis=1).mean() > 0.9                # all but the centre pixels lack a region
    assert (~flags[:, 0]).sum() == 9                        # the top row keeps cost_array[0][0] = 2
    assert sum(cov["hyp"]) > 0
    draws = np.concatenate([t.draws for t in out["traces"]])
    assert draws.min() == 22 and np.all(draws % 2 == 0)     # 15 + 1 + 2k + 1 + 3
    assert sum(len(t.ys) for t in out["traces"]) == 63      # every pixel swept once


def test_geometric_given_state():
    prob, out, cov = _assert_equal("geom")
    _assert_sweep_coverage(cov)
    assert all((d == 0).mean() > 0.1 for d in prob.depths)
    r = rs.SweepRestated(prob, rs.OracleBackend(prob))
    r.init()
    g = r.be.geom_costs(r.planes)
    assert (g == 3.0).mean() > 0.1 and (g < 3.0).mean() > 0.05   # zero depths and round trips both reached
    assert (r.branch_init == 5).all()


def test_planar_prior_both_init_branches():
    prob, out, cov = _assert_equal("planar")
    _assert_sweep_coverage(cov)
    init = out["restated"].branch_init
    assert 0.4 < (prob.masks > 0).mean() < 0.6
    assert (init == 2).sum() > 100 and (init == 3).sum() > 100          # :641 both ways
    assert ((prob.masks > 0) & (prob.costs < 0.1)).sum() > 100          # masked, yet below 0.1
    assert cov["planar_accept"] > 0.05 and cov["plain_accept"] > 0.05 and cov["shadowed"] > 0.05


@pytest.mark.parametrize("name", ["hier_up", "hier_swap", "hier_seeded"])
def test_hierarchy(name):
    """The upsample branch (upscale_normal, pre_costs written at :681), the
    same-size branch behind the rows/cols swap with given pre_costs, and the
    seeded init under the hierarchy gate."""
    prob, out, cov = _assert_equal(name)
    _assert_sweep_coverage(cov)
    assert cov["gate_pass"] >= 0.10 and cov["gate_block"] >= 0.10
    init = out["restated"].branch_init
    assert (init == {"hier_up": 4, "hier_swap": 5, "hier_seeded": 1}[name]).all()
    if name == "hier_up":
        assert prob.prm.upsample == 1 and (out["pre_costs"] != 0).all()
    else:
        assert prob.scaled_planes.shape[:2] == (45, 33) and prob.prm.upsample == 0


_WHERE = ("small37", "geom", "hier_swap", "planar", "photo")


@pytest.mark.parametrize("variant", rs.VARIANTS)
def test_every_changed_rule_is_noticed(variant):
    """One rule of the restatement changed: the oracle must disagree on at
    least one pixel of the cases above."""
    words = 0
    for name in _WHERE:
        prob, ref, _ = _case(name)
        out = rs.run_restated(prob, variant=variant)
        words = sum(int(mismatch(out[k], ref[k]).sum()) for k in ("planes", "costs", "selected_views"))
        if words:
            print(f"{variant}: {words} words differ in {name}")
            break
    assert words > 0, f"{variant} agrees with the oracle on every case: the inputs do not test that rule"
