"""The observation raster kernel (csrc/raster_kernels.hip, cld_rasterize) against the recording of the reference's rasterize_agents and
against the fp64 restatement of tests/raster_cases.py, and `SceneObserver` over a closed loop.  The cases are built so that fp32 cannot
decide differently from fp64 (tests/test_raster_host.py asserts the margins on the CPU), hence the comparisons are exact: the history planes
everywhere, the semantic planes outside the pixels the restatement leaves out (fp64 map coordinate within 1e-3 px of a rounding boundary)."""
import numpy as np
import pytest
import torch

from cld_amd import synth
from tests import raster_cases as RC
from tests.test_raster_host import golden_as_case

pytestmark = pytest.mark.gpu
T = RC.T_HIST


@pytest.fixture(scope="module")
def eng():
    from cld_amd.engine import Engine
    return Engine(n_timesteps=10, device="cuda:0")          # no weights: the rasteriser needs none


def run(eng, case, row0=0, B=None, **override):
    cfg = dict(case["cfg"], **override)
    maps = case.get("maps")
    out = eng.rasterize(case["hist_world"], case["hist_avail"], case["scene_start"], maps, case.get("scene_map"), case.get("map_from_world"),
                        row0=row0, B=B, **cfg)
    torch.cuda.synchronize()
    return out


def check(out, ref, what=""):
    img, drv, rfw = (t.cpu().numpy() for t in out)
    assert img.shape == ref["image"].shape and drv.shape == ref["drivable"].shape
    bad = img[:, :T] != ref["image"][:, :T]
    assert not bad.any(), f"{what}: {int(bad.sum())} history pixels differ, first at (row, plane, y, x) = {np.argwhere(bad)[0].tolist()}"
    keep = ~ref["left_out"]
    bad = (img[:, T:] != ref["image"][:, T:]) & keep
    assert not bad.any(), f"{what}: {int(bad.sum())} semantic pixels differ, first at (row, layer, y, x) = {np.argwhere(bad)[0].tolist()}"
    assert np.array_equal(drv, (img[:, T] != 0).astype(np.uint8)), what                     # the kernel's own first semantic plane, everywhere
    assert np.array_equal(drv[keep[:, 0]], ref["drivable"][keep[:, 0]]), what
    # raster_from_world: rotation entries of magnitude <= ppm, translations of magnitude < 1,000 px from a handful of fp32 roundings and cosf / sinf
    assert np.abs(rfw - ref["raster_from_world"]).max() <= 5e-4, what


def test_reference_recording_24x40(eng, golden):
    """The planes recorded from the reference's rasterize_agents, exact; the other 20 rows of the same call against the restatement."""
    case, planes = golden_as_case(golden)
    out = run(eng, case, max_neighbor_dist=0.0)
    img = out[0].cpu().numpy()
    for s, r in enumerate(case["scene_start"][:-1]):
        assert np.array_equal(img[r, :T], planes[s].astype(np.float32)), s
    assert (img[:, T:] == -1.0).all()
    check(out, RC.restate(case, max_neighbor_dist=0.0), "golden")


@pytest.mark.parametrize("dist", [30.0, 0.0])
def test_eight_agents_at_224(eng, dist):
    """The ContextEncoder's raster size: scene 0 on a map, scene 1 without one; the ego on flat pixels 0 and H W - 1, a neighbour on the ego's
    pixel, unavailable frames, an agent absent now, agents beyond 30 m; both neighbour rules."""
    case = RC.case("eight")
    ref = RC.restate(case, max_neighbor_dist=dist)
    assert ref["pix_margin"] >= RC.PIX_MARGIN and ref["dist_margin"] >= RC.DIST_MARGIN and ref["left_out"].mean() <= 0.01
    check(run(eng, case, max_neighbor_dist=dist), ref, f"eight D={dist}")


def test_scene_sizes_1_2_65_in_one_call(eng):
    case = RC.case("sizes")
    ref = RC.restate(case)
    assert ref["pix_margin"] >= RC.PIX_MARGIN and ref["dist_margin"] >= RC.DIST_MARGIN
    out = run(eng, case)
    check(out, ref, "sizes")
    assert (out[0][:, T:] == -1.0).all() and (out[1] == 1).all()                                # no maps: fill everywhere, all drivable
    assert (out[0][0, :T] == -1).sum() == 0                                                    # the scene of one has no neighbours


@pytest.mark.parametrize("name", ["small_map", "odd"])
def test_map_smaller_than_the_crop_and_dword_store_path(eng, name):
    case = RC.case(name)
    ref = RC.restate(case)
    assert ref["pix_margin"] >= RC.PIX_MARGIN and ref["dist_margin"] >= RC.DIST_MARGIN and ref["left_out"].mean() <= 0.01
    check(run(eng, case), ref, name)


def test_shard_rows_are_bit_identical_to_the_whole_call(eng):
    case = RC.case("eight")
    whole = run(eng, case)
    part = run(eng, case, row0=2, B=4)                       # starts inside scene 0 and runs into scene 1
    for w, p in zip(whole, part):
        assert torch.equal(w[2:6], p)
    buf = torch.full((6, T + 3, 224, 224), 7.0, device="cuda")
    cfg = case["cfg"]
    img, _, _ = eng.rasterize(case["hist_world"], case["hist_avail"], case["scene_start"], case["maps"], case["scene_map"], case["map_from_world"],
                              row0=2, B=4, out=buf, **cfg)
    assert img.data_ptr() == buf.data_ptr() and torch.equal(img, part[0]) and bool((buf[4:] == 7.0).all())      # a reused buffer: only B rows written


def test_limits_are_errors(eng):
    from cld_amd._lib import CldError
    case = RC.case("odd")
    a = (case["hist_world"], case["hist_avail"], case["scene_start"])
    with pytest.raises(CldError, match="CLD_RASTER_MAX_PIXELS"):
        eng.rasterize(*a, height=512, width=512)
    with pytest.raises(CldError, match="row0"):
        eng.rasterize(*a, row0=3, B=3, height=22, width=37)


def test_scene_observer_over_a_closed_loop(precision):
    """2 scenes x 3 agents, 3 sim steps.  Each step's image equals the restatement built from the observer's own history at that step.  The
    histories now hold positions the kernels computed, which keep no margin, so a history plane is compared only when every coordinate painted
    into it is >= 1e-3 px away from a rounding or clamp boundary in fp64 -- ten times the fp32 error of a coordinate (differences of
    |coordinates| < 300 m, cosf / sinf, five roundings: < 1e-4 px); at most 10 % of the planes may drop out.  The observer's poses are the
    rollout's, bit for bit; consecutive images differ; encode=True in chunks of 2 gives the cond_feat of one pass, bit for bit."""
    from cld_amd.dm_model import DmModel
    from cld_amd.engine import Engine
    from cld_amd.observe import SceneObserver
    from cld_amd.policy import CldPolicy, closed_loop_rollout
    from cld_amd.vae_model import VaeModel
    n, S = 10, 3
    e = Engine(n_timesteps=n, device="cuda:0", precision=precision)
    for sd in (synth.make_unet_weights(0, affine_jitter=True), synth.make_decoder_weights(0), synth.make_context_weights(0)):
        e.load_state_dict(sd)
    e.finalize()
    pol = CldPolicy(DmModel(None, None, n_timesteps=n, engine=e), VaeModel(engine=e))
    case = RC.build_case(21, [3, 3], spread=6.0, with_maps=[(320, 256)])
    B = 6
    args = (case["scene_start"], case["hist_world"], case["hist_avail"], case["maps"], case["scene_map"], case["map_from_world"])
    obs = SceneObserver(e, *args, n_step_action=5)
    g = torch.Generator(device="cuda").manual_seed(7)
    noise = {"x_T": torch.randn(B, 52, 4, device="cuda", generator=g), "noise": torch.randn(n, B, 52, 4, device="cuda", generator=g)}
    cs = torch.zeros(B, 4, device="cuda"); cs[:, 2] = torch.rand(B, device="cuda", generator=g) * 10.0
    seen = []

    def cond_fn(step, world, c, plans):
        o = obs(step, world, c, plans)
        assert torch.equal(world, obs.poses)                                               # the rollout's poses and the observer's: the same bits
        seen.append(dict(hist_world=obs.hist_world.cpu().numpy(), hist_avail=obs.hist_avail.cpu().numpy(), image=o["image"].cpu().numpy(),
                         drivable=o["drivable_map"].cpu().numpy(), keys=set(o)))
        return o
    hw = torch.from_numpy(case["hist_world"])
    poses = closed_loop_rollout(pol, cond_fn, hw[:, -1, :2], hw[:, -1, 2], cs, n_sim_steps=S, n_step_action=5, gather=lambda traj: traj, noise=noise)
    assert poses.shape == (S, B, 3) and bool(torch.isfinite(poses).all())
    assert seen[0]["keys"] >= {"image", "history_positions", "history_yaws", "history_availabilities", "curr_speed", "drivable_map",
                               "raster_from_agent", "raster_from_world", "world_from_agent", "agent_from_world", "agent_hist"}
    dropped = total = 0
    for s in range(S):
        ref = RC.restate(dict(case, hist_world=seen[s]["hist_world"], hist_avail=seen[s]["hist_avail"]))
        assert ref["dist_margin"] >= RC.DIST_MARGIN
        ok = ref["plane_margin"] >= 1e-3
        dropped, total = dropped + int((~ok).sum()), total + ok.size
        assert np.array_equal(seen[s]["image"][:, :T][ok], ref["image"][:, :T][ok]), s
        keep = ~ref["left_out"]
        assert keep.mean() >= 0.99 and np.array_equal(seen[s]["image"][:, T:][keep], ref["image"][:, T:][keep]), s
        assert np.array_equal(seen[s]["drivable"], (seen[s]["image"][:, T] != 0).astype(np.uint8))
        if s:
            assert (seen[s]["image"] != seen[s - 1]["image"]).any()
            assert np.array_equal(seen[s]["hist_world"][:, :T - 5], seen[s - 1]["hist_world"][:, 5:])       # the ring moved by n_step_action
            assert seen[s]["hist_avail"][:, T - 5:].all()
    print(f"history planes compared: {total - dropped} of {total}")
    assert dropped <= 0.1 * total
    # encode=True: chunks of 2 through one buffer against one pass against context_encode of the whole image
    one = SceneObserver(e, *args, encode=True).observe(cs)
    two_obs = SceneObserver(e, *args, encode=True, chunk_agents=2)
    two = two_obs.observe(cs)
    plain = SceneObserver(e, *args).observe(cs)
    assert two_obs._buf.shape[0] == 2 and "image" not in two and torch.equal(two["curr_states"], cs)
    assert torch.equal(one["cond_feat"], two["cond_feat"]) and torch.equal(one["cond_feat"], e.context_encode(plain["image"], cs))
    assert torch.equal(one["drivable_map"], two["drivable_map"]) and torch.equal(two["drivable_map"], plain["drivable_map"])
    assert torch.equal(two["raster_from_world"], plain["raster_from_world"])
    assert bool(torch.isfinite(one["cond_feat"]).all()) and float(one["cond_feat"].std()) > 0
