"""patch_size / radius_increment other than the reference defaults 11 / 2:
the general-patch kernels (k_init_g, k_sweep_g, k_eval_costs_g;
acmmp_amd/csrc/acmmp_general.h) against the CPU oracle, which loops
`for (i = -radius; i < radius + 1; i += radius_increment)` as the reference
does (src/ACMMP.cu:382-412). Everything is held to bit-exactness.

Geometries: symmetric and dense (7/1, 21/1), the smallest (3/1), the default
increment at another size (5/2), offsets that are asymmetric and never 0
(8/3: {-4, -1, 2}; 12/5: {-6, -1, 4}), the largest radius with a sparse step
(21/4). Every init branch, source-count bucket and texel form of the general
kernels, the row-band run, ACMMP_GENERAL_PATCH=1 (11 / 2 through the general
kernels) and the engine's envelope check are covered."""
import numpy as np
import pytest

import oracle
from acmmp_amd import ACMMP, default_params, scene
from acmmp_amd.engine import AcmmpError
from parity_util import assert_bit_exact
from test_gpu_parity import _cam_planes_from_truth, _random_planes

pytestmark = pytest.mark.gpu


def _params(patch, iters=2, **kw):
    p = default_params()
    p.max_iterations = iters
    p.patch_size, p.radius_increment = patch
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _gpu_run(p, cams, imgs, depths=None, state=None, setup=None):
    with ACMMP(0) as eng:
        eng.set_params(p)
        eng.set_images(cams, imgs)
        if depths is not None:
            eng.set_depth_maps(depths)
        if state is not None:
            eng.set_plane_hypotheses(*state)
        if setup is not None:
            setup(eng)
        prm = eng.params
        bits = eng.texel_bits()
        eng.RunPatchMatch()
        return prm, eng.plane_hypotheses(), eng.costs(), eng.selected_views(), bits


def _check(got, ref, what):
    assert_bit_exact(got[1], ref["planes"], f"planes ({what})")
    assert_bit_exact(got[2], ref["costs"], f"costs ({what})")
    assert_bit_exact(got[3], ref["selected_views"], f"selected views ({what})")


# ------------------------------------------------------------- cost vectors
@pytest.mark.parametrize("nsrc,patch", [(4, (3, 1)), (4, (5, 2)), (4, (7, 1)), (4, (8, 3)), (4, (12, 5)),
                                        (4, (21, 4)), (4, (21, 1)), (20, (7, 1)), (20, (12, 5))])
def test_cost_vectors(nsrc, patch):
    sc = scene.make_scene(num_views=nsrc + 1, width=80, height=60, arc_deg=4.0)
    cams, imgs = sc.problem(0, nsrc)
    H, W = imgs[0].shape
    planes = _random_planes(cams, H, W, seed=nsrc)
    with ACMMP(0) as eng:
        eng.set_params(_params(patch))
        eng.set_images(cams, imgs)
        prm = eng.params
        g_cost, g_init, g_views = eng.eval_costs(planes)
    assert (prm.patch_size, prm.radius_increment) == patch
    r_cost, r_init, r_views = oracle.eval_costs(prm, cams, imgs, planes)
    assert_bit_exact(g_cost, r_cost, "ncc cost vectors")
    assert_bit_exact(g_init, r_init, "initial cost")
    assert_bit_exact(g_views, r_views, "initial selected views")
    assert (r_cost < 2).mean() > 0.05  # the hypotheses do exercise the full NCC


# --------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def odd_scene():
    """Odd width, a ragged last colour-split column, three block rows (the
    last one partial)."""
    return scene.make_scene(num_views=10, width=67, height=45)


def _geom_inputs(sc, ref, nsrc):
    """The scene's depth maps of the problem's views and a start state for the
    geometric pass (the true normals and depths, cost 0.5)."""
    v = sc.views[ref]
    depths = [sc.views[i].depth for i in [ref] + sc.pairs[ref][:nsrc]]
    planes = np.concatenate([v.normal, np.where(v.depth > 0, v.depth, 700.0)[..., None]], -1).astype(np.float32)
    return depths, (planes, np.full(v.depth.shape, 0.5, np.float32))


@pytest.fixture(scope="module")
def odd_default(odd_scene):
    """The same runs at 11 / 2 (the fast kernels), photometric and geometric."""
    cams, imgs = odd_scene.problem(0, 9)
    depths, state = _geom_inputs(odd_scene, 0, 9)
    return {False: _gpu_run(_params((11, 2)), cams, imgs)[1],
            True: _gpu_run(_params((11, 2), geom_consistency=1), cams, imgs, depths=depths, state=state)[1]}


@pytest.mark.parametrize("geom,patch", [(False, (7, 1)), (False, (8, 3)), (False, (21, 1)),
                                        (True, (7, 1)), (True, (12, 5))])
def test_end_to_end(odd_scene, odd_default, geom, patch):
    cams, imgs = odd_scene.problem(0, 9)
    depths, state = _geom_inputs(odd_scene, 0, 9) if geom else (None, None)
    got = _gpu_run(_params(patch, geom_consistency=int(geom)), cams, imgs, depths=depths, state=state)
    kw = dict(depths=depths, planes=state[0], costs=state[1]) if geom else {}
    ref = oracle.run_patchmatch(got[0], cams, imgs, **kw)
    _check(got, ref, f"{patch}, geom {geom}")
    assert not np.array_equal(got[1], odd_default[geom])  # the geometry reaches the kernels


def test_skipped_last_row():
    """H = 33: the reference grid never reaches the last row (it keeps its
    initial state), also at 7 / 1."""
    sc = scene.make_scene(num_views=4, width=37, height=33)
    cams, imgs = sc.problem(1, 3)
    assert oracle.checkerboard_rows(33) == 32
    got = _gpu_run(_params((7, 1)), cams, imgs)
    _check(got, oracle.run_patchmatch(got[0], cams, imgs), "37x33, 7/1")


# ------------------------------------------------- the other init branches
@pytest.fixture(scope="module")
def small_scene():
    return scene.make_scene(num_views=10, width=128, height=96)


def test_planar_prior_init_branch(small_scene):
    """As test_gpu_parity.test_planar_prior_init_branch_with_geom, at 7 / 1."""
    cams, imgs = small_scene.problem(2, 3)
    ids = [2] + small_scene.pairs[2][:3]
    depths = [small_scene.views[i].depth for i in ids]
    H, W = imgs[0].shape
    rng = np.random.default_rng(5)
    state_planes = np.concatenate([small_scene.views[2].normal, small_scene.views[2].depth[..., None]], -1)
    state_costs = rng.uniform(0, 0.3, size=(H, W)).astype(np.float32)
    prior = _cam_planes_from_truth(small_scene.views[2], cams[0])
    prior[..., 3] = small_scene.views[2].depth
    mask = (rng.uniform(size=(H, W)) < 0.7).astype(np.uint32)
    labels = (np.arange(H * W) + 1).astype(np.uint32).reshape(H, W) * mask
    p = _params((7, 1), 1, geom_consistency=1, planar_prior=1)
    got = _gpu_run(p, cams, imgs, depths=depths, state=(state_planes, state_costs),
                   setup=lambda eng: eng.CudaPlanarPriorInitialization(prior.reshape(-1, 4), labels))
    per_pixel = np.where(mask[..., None] > 0, prior, 0).astype(np.float32)
    ref = oracle.run_patchmatch(got[0], cams, imgs, depths=depths, planes=state_planes, costs=state_costs,
                                prior_planes=per_pixel, masks=labels)
    _check(got, ref, "planar-prior init, 7/1")


@pytest.mark.parametrize("same_size", [False, True])
def test_hierarchy_init(small_scene, same_size):
    """As test_gpu_parity.test_hierarchy_init (host inputs), at 7 / 1."""
    cams, imgs = small_scene.problem(4, 4)
    H, W = imgs[0].shape
    rng = np.random.default_rng(9)
    v = small_scene.views[4]
    if same_size:
        sh, sw = W, H
        scaled = np.zeros((sh, sw, 4), np.float32)
        scaled.reshape(-1, 4)[:] = np.concatenate([v.normal, v.depth[..., None]], -1).reshape(-1, 4)
    else:
        sh, sw = H // 2, W // 2
        scaled = np.concatenate([v.normal[::2, ::2], rng.uniform(0, 1, (sh, sw, 1))], -1).astype(np.float32)
    up_depth = np.where(v.depth > 0, v.depth, 700.0).astype(np.float32)
    got = _gpu_run(_params((7, 1), hierarchy=1), cams, imgs,
                   setup=lambda eng: eng.set_hierarchy_inputs(scaled, up_depth))
    assert got[0].upsample == (0 if same_size else 1)
    planes_in = np.zeros((H, W, 4), np.float32)
    planes_in[..., 3] = up_depth
    ref = oracle.run_patchmatch(got[0], cams, imgs, planes=planes_in, pre_costs=np.zeros((H, W), np.float32),
                                scaled_planes=scaled)
    _check(got, ref, "hierarchy init, 7/1")


def test_seeded_init(small_scene):
    """As test_gpu_parity.test_seeded_init, at 7 / 1."""
    cams, imgs = small_scene.problem(5, 4)
    seed = _cam_planes_from_truth(small_scene.views[5], cams[0])
    got = _gpu_run(_params((7, 1)), cams, imgs, setup=lambda eng: eng.SetPlanarPrior(seed))
    assert got[0].seeded == 1
    ref = oracle.run_patchmatch(got[0], cams, imgs, seed_planes=seed)
    _check(got, ref, "seeded init, 7/1")


# ------------------------------------------------------ source-count buckets
@pytest.mark.parametrize("nsrc", [20, 25])
def test_source_count_buckets(nsrc):
    """The NS 20 and NS 32 instantiations of the general sweep."""
    sc = scene.make_scene(num_views=nsrc + 1, width=64, height=48)
    cams, imgs = sc.problem(0, nsrc)
    got = _gpu_run(_params((5, 2), 1), cams, imgs)
    _check(got, oracle.run_patchmatch(got[0], cams, imgs), f"{nsrc} sources, 5/2")


# -------------------------------------------------------------- texel forms
@pytest.fixture(scope="module")
def texel_prob():
    return scene.make_scene(num_views=6, width=112, height=84).problem(0, 5)


@pytest.fixture(scope="module")
def texel_ref():
    """One oracle run serves every form (the form changes the memory format
    only): made by the first case, from the engine's parameters."""
    return {}


@pytest.mark.parametrize("env,bits", [({"ACMMP_TEXEL": "u8"}, 8), ({"ACMMP_TEXEL": "h16"}, 16),
                                      ({"ACMMP_TEXEL": "f32"}, 32), ({"ACMMP_WIDE_INDEX": "1"}, 8)])
def test_texel_forms(texel_prob, texel_ref, monkeypatch, env, bits):
    cams, imgs = texel_prob
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    got = _gpu_run(_params((7, 1), 1), cams, imgs)
    assert got[4] == bits
    if not texel_ref:
        texel_ref["prm"] = bytes(got[0])
        texel_ref["out"] = oracle.run_patchmatch(got[0], cams, imgs)
    assert bytes(got[0]) == texel_ref["prm"]  # the oracle ran with this run's parameters
    _check(got, texel_ref["out"], f"{env}, 7/1")


# ------------------------------------------------------ forced general path
@pytest.mark.parametrize("geom", [False, True])
def test_forced_general_path_at_default_geometry(small_scene, monkeypatch, geom):
    """ACMMP_GENERAL_PATCH=1: 11 / 2 through the general kernels gives what the
    oracle and the fast kernels give."""
    cams, imgs = small_scene.problem(0, 9)
    depths, state = _geom_inputs(small_scene, 0, 9) if geom else (None, None)
    p = _params((11, 2), geom_consistency=int(geom))
    fast = _gpu_run(p, cams, imgs, depths=depths, state=state)
    monkeypatch.setenv("ACMMP_GENERAL_PATCH", "1")
    general = _gpu_run(p, cams, imgs, depths=depths, state=state)
    kw = dict(depths=depths, planes=state[0], costs=state[1]) if geom else {}
    _check(general, oracle.run_patchmatch(general[0], cams, imgs, **kw), "forced general path")
    assert_bit_exact(general[1], fast[1], "planes, general against fast kernels")
    assert_bit_exact(general[2], fast[2], "costs, general against fast kernels")
    assert_bit_exact(general[3], fast[3], "selected views, general against fast kernels")


# ---------------------------------------------------------------- row bands
def _band_setup(eng, W, H):
    """test_gpu_band's photometric inputs, with the patch set to 7 / 1."""
    from test_gpu_band import _setup
    _setup(eng, "photometric", W, H)
    p = eng.params
    p.patch_size, p.radius_increment = 7, 1
    eng.set_params(p)


def _band_worker(rank, world, port, W, H, q):
    import datetime
    import traceback

    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world,
                            timeout=datetime.timedelta(seconds=60))
    try:
        from acmmp_amd.band import bands, run_split
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(dev)
        with ACMMP(0) as eng:
            _band_setup(eng, W, H)
            planes, costs = run_split(eng, bands(H, world), list(range(world)), rank, dev, torch.device("cpu"))
            if rank == 0:
                q.put(("ok", planes.cpu().numpy(), costs.cpu().numpy()))
    except BaseException:
        q.put(("error", rank, traceback.format_exc()))
        raise
    finally:
        dist.destroy_process_group()


def test_two_row_bands_match_unsplit():
    """acmmp_run_patchmatch_band at 7 / 1: the 23-row halo comes from the far
    searches, not from the patch, so the split needs nothing else."""
    import torch.multiprocessing as mp
    from test_gpu_band import _free_port
    world, W, H = 2, 120, 100
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_band_worker, args=(r, world, port, W, H, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = q.get(timeout=150)
    assert got[0] == "ok", f"rank {got[1]} failed:\n{got[2]}"
    for p in procs:
        p.join(timeout=90)
        assert p.exitcode == 0
    with ACMMP(0) as eng:
        _band_setup(eng, W, H)
        assert (eng.params.patch_size, eng.params.radius_increment) == (7, 1)
        eng.RunPatchMatch()
        ref = eng.plane_hypotheses(), eng.costs()
    assert_bit_exact(got[1], ref[0], "planes, 2 bands at 7/1")
    assert_bit_exact(got[2], ref[1], "costs, 2 bands at 7/1")


# ----------------------------------------------------------------- envelope
@pytest.mark.parametrize("bad", [dict(patch_size=1), dict(patch_size=23), dict(radius_increment=0),
                                 dict(patch_size=7, radius_increment=7), dict(texture_filter8=1)])
def test_envelope(bad):
    """Outside 1 <= patch_size / 2 <= 10, 1 <= radius_increment <= 2 * radius
    (and texture_filter8 off the default geometry): ACMMP_ERR_UNSUPPORTED with
    the envelope in the message, from the run and from eval_costs; the engine
    stays usable."""
    sc = scene.make_scene(num_views=4, width=48, height=40)
    cams, imgs = sc.problem(0, 3)
    H, W = imgs[0].shape
    with ACMMP(0) as eng:
        eng.set_params(_params((7, 1), 1))
        eng.set_images(cams, imgs)
        p = eng.params
        for k, v in bad.items():
            setattr(p, k, v)
        eng.set_params(p)
        for call in (eng.RunPatchMatch, lambda: eng.eval_costs(_random_planes(cams, H, W, seed=1))):
            with pytest.raises(AcmmpError, match=r"status -5.*envelope.*1 <= patch_size / 2 <= 10"):
                call()
        with pytest.raises(AcmmpError, match=r"status -5.*envelope"):
            eng.set_images(cams, imgs)  # the setters refuse it too
        p.patch_size, p.radius_increment, p.texture_filter8 = 7, 1, 0
        eng.set_params(p)
        eng.set_images(cams, imgs)
        prm = eng.params
        eng.RunPatchMatch()
        got = (prm, eng.plane_hypotheses(), eng.costs(), eng.selected_views())
    _check(got, oracle.run_patchmatch(prm, cams, imgs), "7/1 after a refused geometry")
