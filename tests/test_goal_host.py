"""Host-side checks of the global waypoint guidance (global_target_pos / global_target_pos_at_time): the fp64 yardstick
(tests/goal_yardstick.py) against the recording made from the reference's own classes (tests/golden/global_goal.npz,
tests/tools/record_goal_golden.py), the configuration adapter, the policy's closed-loop state and the ctypes layout of `cld_goal`."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from cld_amd import synth
from tests import goal_yardstick as Y

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["pos", "pos2", "time", "time2"]


def recorded_case(golden, name):
    """-> (meta, arrays, plans [A,N,52,6] float32, goal dict (fp64, flags as the yardstick's own state update gives them), config's agents)."""
    meta, g = golden("global_goal")
    A, N = meta["A"], meta["N"]
    speed = synth.make_collision_scene([A], meta["seed"])["curr_speed"]
    tag = name.rstrip("2")
    reached = None
    for step in ([tag] if name == tag else [tag, name]):              # the flags of step 2 build on step 1's
        case = meta["cases"][step]
        goal, idx = Y.goal_from_meta(case, g, case["frames"], A, N)
        if reached is None:
            reached = torch.zeros(len(idx), dtype=torch.bool)
        W = torch.from_numpy(g[case["frames"] + "world_from_agent"]).double()
        hist = torch.from_numpy(g[case["frames"] + "agent_hist"]).double()
        reached, tol_margin = Y.reached_update(reached, goal["target_pos"][idx], W[idx], hist[idx], case["target_tolerance"], case["action_num"])
        assert tol_margin >= 1e-3
    goal["reached"][idx] = reached
    plans = torch.from_numpy(synth.make_collision_trajectories(A, N, speed, case["plans_seed"]))
    return meta, g, plans, goal, idx


@pytest.mark.parametrize("name", CASES)
def test_yardstick_matches_the_reference_recording(golden, name):
    """Values <= 2e-5 max(1, max|ref|), gradient <= 1e-4 max|ref grad| (the bars of the map-collision recording), flags equal; and the
    recorded rows keep the distance from every kink that the kernel tests rely on."""
    meta, g, plans, goal, idx = recorded_case(golden, name)
    ref_v, ref_g = g[name + "_values"], g[name + "_grad"]
    assert np.array_equal(goal["reached"].numpy(), g[name + "_reached"])
    outside = np.ones(meta["A"], bool); outside[idx] = False
    assert np.isnan(ref_v[outside]).all() and not np.isnan(ref_v[idx]).any()
    v, grad = Y.value_and_grad(plans.double(), goal)
    err_v = np.abs(v.numpy()[idx] - ref_v[idx]).max()
    err_g = np.abs(grad.numpy() - ref_g).max()
    kink, dmin = Y.margins(plans.double(), goal)
    print(f"{name}: branches {Y.branches(goal)}; value error {err_v:.2e} (max|ref| {np.abs(ref_v[idx]).max():.3f}), gradient error {err_g:.2e} "
          f"(max|ref| {np.abs(ref_g).max():.3e}); kink margin {kink:.3e} m, smallest distance read {dmin:.3e} m")
    assert kink >= 1e-3 and dmin >= 1e-2
    assert err_v <= 2e-5 * max(1.0, np.abs(ref_v[idx]).max())
    assert np.abs(ref_g).max() > 0 and err_g <= 1e-4 * np.abs(ref_g).max()
    assert abs(float(Y.total(plans.double(), goal)) - float(g[name + "_total"][0])) <= 2e-5 * max(1.0, abs(float(g[name + "_total"][0])))


def test_the_recording_holds_the_cases_it_is_meant_to(golden):
    br = {name: Y.branches(recorded_case(golden, name)[3]) for name in CASES}
    assert br["pos"].count("exact") >= 2 and br["pos"].count("progress") >= 2 and br["pos"].count("reached") == 2 and br["pos"].count("off") == 2
    meta, g, plans, goal, idx = recorded_case(golden, "pos")
    v = Y.values(plans.double(), goal)
    prog = [a for a in range(8) if br["pos"][a] == "progress"]
    assert any(float(goal["urgency"][a] * 52 * 0.1 * goal["pref_speed"][a]) < 0.5 and float(v[a].min()) > 0 for a in prog)      # the min_progress_dist floor
    assert any(float(v[a].max()) == 0.0 for a in prog)                                                                   # an inactive relu
    # one of the two arrived agents is flagged through ANOTHER agent's history point only: its own points are all out of tolerance
    case = meta["cases"]["pos"]
    W, hist = torch.from_numpy(g["world_from_agent"]).double(), torch.from_numpy(g["agent_hist"]).double()
    own, _ = Y.reached_update(torch.zeros(len(idx), dtype=torch.bool), goal["target_pos"][idx], W[idx], hist[idx], case["target_tolerance"], 5, by="own")
    assert int(own.sum()) == 1 and int(goal["reached"].sum()) == 2 and bool(goal["reached"][idx][own].all())
    assert set(br["time"]) == {"passed", "at_time", "on_time"}
    meta, g, plans, goal, idx = recorded_case(golden, "time")
    v = Y.values(plans.double(), goal)
    on = [a for a in range(8) if br["time"][a] == "on_time"]
    assert any(float(v[a].min()) > 0 for a in on) and any(float(v[a].max()) == 0 for a in on)
    changed = [(a, b) for a, b in zip(br["pos"] + br["time"], br["pos2"] + br["time2"]) if a != b]
    assert ("progress", "exact") in changed and ("on_time", "at_time") in changed
    for one, two in (("pos", "pos2"), ("time", "time2")):                    # flags persist
        assert all(b == "reached" for a, b in zip(br[one], br[two]) if a == "reached")


def _cfg_pair():
    scene_index = torch.tensor([4, 4, 4, 9, 9, 9, 9, 9])
    tp0 = np.arange(4, dtype=np.float32).reshape(2, 2) + 10.0
    tp1 = np.arange(6, dtype=np.float32).reshape(3, 2) - 5.0
    cfg = [[{"name": "global_target_pos", "weight": 3.0, "agents": [0, 2],
             "params": {"target_pos": tp0, "urgency": [0.25, 0.75], "pref_speed": [1.0, 2.0], "dt": 0.1, "min_progress_dist": 0.7, "target_tolerance": 1.5}}],
           [{"name": "global_target_pos_at_time", "weight": 0.5, "agents": [1, 3, 4],
             "params": {"target_pos": tp1, "target_time": [30, 80, 5], "urgency": [0.1, 0.2, 0.3]}},
            {"name": "speed_limit", "weight": 3.0, "params": {"speed_limit": 6.0}, "agents": None}]]
    return cfg, scene_index, tp0, tp1


def test_guidance_from_config_accepts_the_two_goal_losses():
    from cld_amd.policy import guidance_from_config
    cfg, scene_index, tp0, tp1 = _cfg_pair()
    g = guidance_from_config(cfg, scene_index)
    goal = g["goal"]
    assert "speed_limit" in g
    assert goal["kind"].tolist() == [1, 0, 1, 0, 2, 0, 2, 2]                 # the configs' `agents` index their scene's members
    assert torch.equal(goal["target_pos"][[0, 2]], torch.from_numpy(tp0)) and torch.equal(goal["target_pos"][[4, 6, 7]], torch.from_numpy(tp1))
    assert goal["target_time"].tolist() == [0, 0, 0, 0, 30, 0, 80, 5]
    assert torch.allclose(goal["scale"], torch.tensor([1.5, 0, 1.5, 0, 0.5 / 3, 0, 0.5 / 3, 0.5 / 3]))      # weight / agents of the config
    assert torch.allclose(goal["urgency"], torch.tensor([0.25, 0, 0.75, 0, 0.1, 0, 0.2, 0.3]))
    assert torch.allclose(goal["pref_speed"][[0, 2, 4, 6, 7]], torch.tensor([1.0, 2.0, 1.42, 1.42, 1.42]))          # upstream's default 1.42
    assert goal["dt"] == 0.1 and goal["min_progress_dist"] == 0.7
    # upstream's constructor defaults: no tolerance for global_target_pos, 2 for global_target_pos_at_time; action_num 5
    cfg[0][0]["params"].pop("target_tolerance")
    goal = guidance_from_config(cfg, scene_index)["goal"]
    assert [(i.tolist(), t, n) for i, t, n in goal["configs"]] == [([0, 2], None, 5), ([4, 6, 7], 2.0, 5)]


def test_guidance_from_config_goal_errors_and_what_stays_unbuilt():
    from cld_amd.policy import guidance_from_config
    cfg, scene_index, tp0, tp1 = _cfg_pair()
    at = lambda **kw: {"name": "global_target_pos_at_time", "weight": 1.0, "agents": [0],
                       "params": dict({"target_pos": [[0.0, 0.0]], "target_time": [5], "urgency": [0.5]}, **kw)}
    with pytest.raises(ValueError, match="two goal losses"):
        guidance_from_config([cfg[0] + [at()], []], scene_index)
    with pytest.raises(ValueError, match="one dt"):
        guidance_from_config([cfg[0], [at(dt=0.2)]], scene_index)
    pos = {"name": "global_target_pos", "weight": 1.0, "agents": [0], "params": {"target_pos": [[0.0, 0.0]], "urgency": [0.5], "min_progress_dist": 0.3}}
    with pytest.raises(ValueError, match="one min_progress_dist"):
        guidance_from_config([cfg[0], [pos]], scene_index)
    with pytest.raises(ValueError):                                          # the parameters are indexed by the config's agents, not by the batch
        guidance_from_config([[dict(cfg[0][0], agents=None)], []], scene_index)
    for name in ("social_group", "stop_sign", "global_stop_sign", "gptcollision"):
        with pytest.raises(NotImplementedError, match="global_target_pos"):
            guidance_from_config([[{"name": name, "weight": 1.0, "params": {}, "agents": None}], []], scene_index)


def _state_case():
    """Three agents in one scene standing at x = 0, 10, 20 (identity headings).  Agent 0's target lies 1 m from where agent 1 stands and
    9 m from itself; agent 2's lies 5 m ahead of itself, which its history only reaches at the second observation."""
    from cld_amd.policy import CldPolicy
    W = torch.eye(3).repeat(3, 1, 1)
    W[:, 0, 2] = torch.tensor([0.0, 10.0, 20.0])
    hist = torch.zeros(3, 8, 2)
    hist[:, :, 0] = -0.1 * torch.arange(7, -1, -1.0)
    cfg = [[{"name": "global_target_pos", "weight": 1.0, "agents": None,
             "params": {"target_pos": [[9.0, 0.0], [100.0, 0.0], [25.0, 0.0]], "urgency": [0.5] * 3, "target_tolerance": 2.0, "action_num": 5}}]]
    return CldPolicy(None, None), cfg, W, hist


def test_policy_carries_the_goal_state_from_one_get_action_to_the_next():
    pol, cfg, W, hist = _state_case()
    pol.set_guidance(cfg, torch.zeros(3, dtype=torch.long))
    goal = pol._guidance["goal"]
    assert pol.goal_reached.tolist() == [False] * 3 and pol.goal_global_t is None
    g0 = pol._goal_for_step(goal, {"world_from_agent": W, "agent_hist": hist}, 0, True)
    assert g0["global_t"] == 0 and g0["reached"].tolist() == [True, False, False]          # "any": agent 1 stands next to agent 0's target
    assert torch.allclose(g0["agent_from_world"] @ W, torch.eye(3).expand(3, 3, 3))         # computed from world_from_agent
    W2 = W.clone(); W2[:, 0, 2] += torch.tensor([0.5, 0.5, 4.0])                            # agent 2 is now 1 m from its target
    g1 = pol._goal_for_step(goal, {"agent_from_world": torch.linalg.inv(W2), "agent_hist": hist}, 5, True)
    assert g1["global_t"] == 5 and pol.goal_global_t == 5 and g1["reached"].tolist() == [True, False, True]
    W3 = W.clone(); W3[:, 0, 2] += 50.0                                                     # everybody far away again: the flags stay
    assert pol._goal_for_step(goal, {"world_from_agent": W3, "agent_hist": hist}, 10, True)["reached"].tolist() == [True, False, True]
    with pytest.raises(ValueError):
        pol._goal_for_step(goal, {"agent_hist": hist}, 11, True)
    pol.set_guidance(cfg, torch.zeros(3, dtype=torch.long))                                 # a new configuration: nobody has arrived
    assert pol.goal_reached.tolist() == [False] * 3 and pol.goal_global_t is None
    pol._goal_for_step(pol._guidance["goal"], {"world_from_agent": W, "agent_hist": hist}, 0, True)
    pol.clear_guidance()
    assert pol.goal_reached is None and pol._guidance is None


def test_goal_reached_by_own_differs_from_the_reference_broadcast():
    pol, cfg, W, hist = _state_case()
    pol.set_guidance(cfg, torch.zeros(3, dtype=torch.long), goal_reached_by="own")
    g0 = pol._goal_for_step(pol._guidance["goal"], {"world_from_agent": W, "agent_hist": hist}, 0, True)
    assert g0["reached"].tolist() == [False, False, False]                                  # agent 0 itself is 9 m from its target
    # its own arrival is seen in this mode too
    W2 = W.clone(); W2[2, 0, 2] = 24.0
    assert pol._goal_for_step(pol._guidance["goal"], {"world_from_agent": W2, "agent_hist": hist}, 1, True)["reached"].tolist() == [False, False, True]
    with pytest.raises(ValueError):
        pol.set_guidance(cfg, torch.zeros(3, dtype=torch.long), goal_reached_by="nearest")
    # the policy's update agrees with the yardstick's in both modes
    from cld_amd.policy import update_goal_reached
    for by in ("any", "own"):
        pol.set_guidance(cfg, torch.zeros(3, dtype=torch.long), goal_reached_by=by)
        goal = pol._guidance["goal"]
        got = update_goal_reached(torch.zeros(3, dtype=torch.bool), goal, W, hist, by)
        ref, _ = Y.reached_update(torch.zeros(3, dtype=torch.bool), goal["target_pos"].double(), W.double(), hist.double(), 2.0, 5, by=by)
        assert torch.equal(got, ref)


def test_repeat_guidance_keeps_the_goal_per_agent():
    from cld_amd.dm_model import repeat_guidance
    goal = {"kind": torch.ones(3, dtype=torch.int32), "scale": torch.ones(3)}
    g = repeat_guidance({"goal": goal, "loss_scale": torch.ones(3)}, 4)
    assert g["goal"]["num_samp"] == 4 and g["goal"]["kind"].shape == (3,) and g["loss_scale"].shape == (12,) and "num_samp" not in goal


def test_cld_goal_layout_matches_the_header():
    """ctypes mirror of `cld_goal` against include/cld.h, field by field in declaration order; the three pinned structs keep their size."""
    from cld_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "cld.h")).read()
    body = re.search(r"typedef struct cld_goal \{(.*?)\} cld_goal;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [(m.group(2), "*" in m.group(1)) for m in re.finditer(r"([A-Za-z_0-9 ]+\*?)\s*\b([a-z_]+);", body)]
    assert [n for n, _ in fields] == [n for n, _ in _lib.CldGoal._fields_]
    off = 0
    for (name, is_ptr), (_, ctype) in zip(fields, _lib.CldGoal._fields_):
        size = 8 if is_ptr else 4
        assert (ctype is ctypes.c_void_p) == is_ptr and ctypes.sizeof(ctype) == size, name
        off = (off + size - 1) // size * size
        assert getattr(_lib.CldGoal, name).offset == off, name
        off += size
    assert ctypes.sizeof(_lib.CldGoal) == 80 and _lib.CldGoal.num_samp.offset == 64 and _lib.CldGoal.min_progress_dist.offset == 76
    assert ctypes.sizeof(_lib.CldGuidance) == 144 and ctypes.sizeof(_lib.CldCollision) == 88 and ctypes.sizeof(_lib.CldMapCollision) == 80
    assert _lib.GOAL_KINDS == {"global_target_pos": 1, "global_target_pos_at_time": 2}
    for sym in ("cld_goal_loss", "cld_set_goal_term"):
        assert sym in _lib.SIGNATURES and re.search(r"\b" + sym + r"\s*\(", hdr)
