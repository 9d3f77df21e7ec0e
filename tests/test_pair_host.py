"""Host-side checks of the pair-relation guidance (`gptcollision`, `gptkeepdistance` and the three project names of the same family):
the fp64 yardstick (tests/pair_yardstick.py) against the recording made from the reference's own classes
(tests/golden/pair_guidance.npz, tests/tools/record_pair_golden.py), the configuration adapter, the gather lists and the ctypes
layout of `cld_pair_term`."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from cld_amd import synth
from tests import pair_yardstick as Y

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["keepdistance", "collision", "stayaway", "keepdistance2", "front", "left", "two"]


def recorded_case(golden, name):
    """-> (meta, arrays, plans [A,N,52,6] float32, yardstick term)."""
    meta, g = golden("pair_guidance")
    A, N = meta["A"], meta["N"]
    plans = torch.from_numpy(g["plans"])
    term = Y.term_from_meta(meta["cases"][name], g["world_from_agent"], g["agent_from_world"], N)
    return meta, g, plans, term


def check_margins(plans, term):
    """The fixture conditions, no row excluded: no distance read below 1e-2 m, no |d - bound|, |Dx| or |Dy| within 1e-3 of a kink."""
    dmin, kink = Y.margins(plans.double(), term)
    assert dmin >= 1e-2 and kink >= 1e-3, (dmin, kink)
    return dmin, kink


@pytest.mark.parametrize("name", CASES)
def test_yardstick_matches_the_reference_recording(golden, name):
    """Values <= 2e-5 max(1, max|ref|), gradient <= 1e-4 max|ref grad| (the bars of the social recording); the class's [N] value sits
    under every agent of the scene; only the two agents of a pair and only x, y receive gradient; the recorded rows keep the margins
    the kernel tests rely on."""
    meta, g, plans, term = recorded_case(golden, name)
    ref_g = g[name + "_grad"]
    v, grad = Y.value_and_grad(plans.double(), term)
    dmin, kink = check_margins(plans, term)
    for k in range(len(term["target"])):
        ref_v = g[f"{name}_values_{k}"]
        assert ref_v.shape == (meta["A"], meta["N"]) and not np.isnan(ref_v).any() and np.array_equal(ref_v, np.broadcast_to(ref_v[:1], ref_v.shape))
        err_v = np.abs(v.numpy()[k] - ref_v[0]).max()
        print(f"{name}[{k}]: value error {err_v:.2e} (max|ref| {np.abs(ref_v).max():.4f})")
        assert err_v <= 2e-5 * max(1.0, np.abs(ref_v).max())
    err_g = np.abs(grad.numpy() - ref_g).max()
    print(f"{name}: gradient error {err_g:.2e} (max|ref| {np.abs(ref_g).max():.3e}); margins: distance {dmin:.3e} m, kink {kink:.3e}")
    assert np.abs(ref_g).max() > 0 and err_g <= 1e-4 * np.abs(ref_g).max()
    assert abs(float(Y.total(plans.double(), term)) - float(g[name + "_total"][0])) <= 2e-5 * max(1.0, abs(float(g[name + "_total"][0])))
    quiet = np.ones(meta["A"], bool)
    quiet[term["target"] + term["ref"]] = False
    assert float(np.abs(grad.numpy()[quiet]).max()) == 0.0 and float(np.abs(ref_g[quiet]).max()) == 0.0
    assert float(np.abs(grad.numpy()[..., 2:]).max()) == 0.0 and float(np.abs(ref_g[..., 2:]).max()) == 0.0
    assert all(float(np.abs(ref_g[a]).max()) > 0.0 for a in term["target"] + term["ref"])          # both ends: nothing is detached


def test_the_recording_holds_the_cases_it_is_meant_to(golden):
    meta, g = golden("pair_guidance")
    cases = meta["cases"]
    assert list(cases) == CASES and meta["A"] == 6 and meta["N"] == 2
    sc = synth.make_collision_scene([6], meta["seed"])                  # the stored inputs are the synthetic scene the meta names
    assert np.array_equal(g["plans"], synth.make_collision_trajectories(6, 2, sc["curr_speed"], meta["seed"])) and g["plans"].shape == (6, 2, 52, 6)
    assert np.array_equal(g["world_from_agent"], sc["world_from_agent"])
    assert [cases[n]["configs"] for n in CASES] == [["gptkeepdistance"], ["gptcollision"], ["StayAwayLoss"], ["KeepDistanceLoss2"], ["FrontCollisionLoss"],
                                                   ["CollideLeftSideLoss"], ["gptcollision", "gptkeepdistance"]]
    assert [[q["kind"] for q in cases[n]["pairs"]] for n in CASES] == [["keep_distance"], ["collision"], ["stay_away"], ["stay_away"], ["front_collision"],
                                                                      ["collide_left"], ["collision", "keep_distance"]]
    # agent_from_world is the inverse of world_from_agent; one agent of `two` is the ref of one pair and the target of the other
    W, F = torch.from_numpy(g["world_from_agent"]).double(), torch.from_numpy(g["agent_from_world"]).double()
    assert float((F @ W - torch.eye(3, dtype=torch.float64)).abs().max()) <= 1e-4
    two = cases["two"]["pairs"]
    assert two[0]["ref"] == two[1]["target"] and len({two[0]["target"], two[0]["ref"], two[1]["ref"]}) == 3
    assert all(q["decay"] > 0 for n in ("stayaway", "keepdistance2") for q in cases[n]["pairs"]) and cases["keepdistance"]["pairs"][0]["decay"] == 0
    assert all(q["lo"] <= q["hi"] for n in ("keepdistance", "stayaway", "keepdistance2") for q in cases[n]["pairs"])
    # every clip branch is active at some step of some sample in one case, and one is idle for a whole sample (recomputed here)
    active, idle = set(), set()
    for n in CASES:
        _, _, plans, term = recorded_case(golden, n)
        for k in range(len(term["target"])):
            for b, (some, _) in Y.branches(plans.double(), term, k).items():
                if bool(some.any()):
                    active.add((term["kind"][k], b))
                if not bool(some.all()):
                    idle.add((n, b))
            assert {b: [a.tolist(), e.tolist()] for b, (a, e) in Y.branches(plans.double(), term, k).items()} == cases[n]["branches"][k]
    assert active >= {("keep_distance", "below_min"), ("keep_distance", "above_max"), ("collision", "above"), ("stay_away", "below_min"),
                      ("stay_away", "above_max"), ("front_collision", "y"), ("collide_left", "y")}
    assert ("keepdistance2", "below_min") in idle and ("left", "y") in idle
    for n in CASES:                                                   # the reference's own float32 error, which a float32 kernel's bar may lean on
        assert cases[n]["ref_value_err"] <= 2e-5 * max(1.0, cases[n]["max_value"])


def test_decay_weights_are_normalised_and_averaged():
    """The yardstick's decayed mean on a constant term: sum_t (decay^t / sum decay^t) / 52 = 1 / 52 of the term, not the term."""
    A, N = 2, 1
    plans = torch.zeros(A, N, 52, 6, dtype=torch.float64)
    W = torch.eye(3, dtype=torch.float64).repeat(A, 1, 1)
    W[1, 0, 2] = 10.0                                                     # 10 m apart at every step
    term = dict(target=[0], ref=[1], kind=["stay_away"], lo=[1.0], hi=[4.0], decay=[0.9], scale=[1.0], world_from_agent=W, agent_from_world=None)
    assert abs(float(Y.values(plans, term)[0, 0]) - 6.0 / 52) <= 1e-12
    assert abs(float(Y.values(plans, dict(term, kind=["keep_distance"], decay=[0.0]))[0, 0]) - 6.0) <= 1e-12


def _cfg():
    scene_index = torch.tensor([4, 4, 4, 4, 9, 9, 9, 9, 9])
    cfg = [[{"name": "gptcollision", "weight": 3.0, "agents": None, "params": {"target_ind": 3, "ref_ind": 0, "collision_radius": 2.0}},
            {"name": "speed_limit", "weight": 3.0, "params": {"speed_limit": 6.0}, "agents": None},
            {"name": "gptstayaway", "weight": 1.0, "agents": None, "params": {"target_ind": 0, "ref_ind": 2}}],
           [{"name": "speed_limit", "weight": 1.0, "params": {"speed_limit": 6.0}, "agents": None},
            {"name": "gptkeepdistance", "weight": 0.5, "agents": None, "params": {"target_ind": 4, "ref_ind": 1}},
            {"name": "gptfrontcollision", "weight": 2.0, "agents": None, "params": {}},
            {"name": "gptcollideleftside", "weight": 4.0, "agents": None, "params": {"target_ind": 0, "ref_ind": 4}}]]
    db = {"world_from_agent": torch.eye(3).repeat(9, 1, 1)}
    return cfg, scene_index, db


def test_pair_terms_from_config_peels_the_pairs_and_folds_the_scales():
    from cld_amd.policy import guidance_from_config, pair_terms_from_config
    cfg, scene_index, db = _cfg()
    rest, term = pair_terms_from_config(cfg, scene_index, db)
    assert [[c["name"] for c in s] for s in rest] == [["speed_limit"], ["speed_limit"]] and rest[0][0] is cfg[0][1]
    assert [len(s) for s in cfg] == [3, 4]                                 # the input is not modified
    assert term["target"] == [3, 0, 8, 6, 4] and term["ref"] == [0, 2, 5, 7, 8]      # scene-local -> batch indices; upstream's defaults 2, 3
    assert term["kind"] == ["collision", "stay_away", "keep_distance", "front_collision", "collide_left"]
    assert term["lo"] == [2.0, 5.0, 5.0, 0.0, 0.0] and term["hi"] == [0.0, 15.0, 15.0, 0.0, 0.0] and term["decay"] == [0.0, 0.9, 0.0, 0.0, 0.0]
    assert term["weight"] == [3.0, 1.0, 0.5, 2.0, 4.0] and "scale" not in term
    assert term["configs"] == [(0, 0), (0, 2), (1, 1), (1, 2), (1, 3)] and term["names"][0] == "gptcollision"
    assert term["world_from_agent"] is db["world_from_agent"] and term["agent_from_world"] is None
    _, term4 = pair_terms_from_config(cfg, scene_index, dict(db, agent_from_world=db["world_from_agent"]), num_samp=4)
    assert np.allclose(term4["scale"], [0.75, 0.25, 0.125, 0.5, 1.0]) and term4["agent_from_world"] is db["world_from_agent"]    # weight / num_samp
    assert "speed_limit" in guidance_from_config(rest, scene_index)
    plain = [[cfg[0][1]], [cfg[1][0]]]
    rest2, term2 = pair_terms_from_config(plain, scene_index, None)        # nothing to peel: no data_batch needed
    assert term2 is None and rest2 == plain
    # upstream's defaults: gptcollision 2 -> 3 (radius 1), gptkeepdistance 20 -> 1 (5 .. 15): the latter needs a scene of 21
    _, t3 = pair_terms_from_config([[{"name": "gptcollision", "weight": 1.0, "agents": None, "params": {}}]], torch.zeros(4, dtype=torch.long), {"world_from_agent": torch.eye(3).repeat(4, 1, 1)})
    assert (t3["target"], t3["ref"], t3["lo"]) == ([2], [3], [1.0])
    _, t4 = pair_terms_from_config([[{"name": "gptkeepdistance", "weight": 1.0, "agents": None, "params": {}}]], torch.zeros(21, dtype=torch.long), {"world_from_agent": torch.eye(3).repeat(21, 1, 1)})
    assert (t4["target"], t4["ref"], t4["lo"], t4["hi"]) == ([20], [1], [5.0], [15.0])


def test_pair_terms_from_config_errors():
    from cld_amd.policy import pair_terms_from_config
    cfg, scene_index, db = _cfg()
    pc = lambda name="gptcollision", **kw: [[dict({"name": name, "weight": 1.0, "agents": None, "params": {}}, **kw)], []]
    with pytest.raises(ValueError, match="world_from_agent"):
        pair_terms_from_config(cfg, scene_index, None)
    with pytest.raises(ValueError, match="world_from_agent"):
        pair_terms_from_config(cfg, scene_index, {"extent": torch.ones(9, 3)})
    with pytest.raises(ValueError, match="outside scene"):
        pair_terms_from_config(pc(params={"target_ind": 4, "ref_ind": 0}), scene_index, db)          # scene 0 has 4 agents
    with pytest.raises(ValueError, match="outside scene"):
        pair_terms_from_config(pc(params={"target_ind": 1, "ref_ind": -1}), scene_index, db)
    with pytest.raises(ValueError, match="outside scene"):
        pair_terms_from_config(pc("gptkeepdistance"), scene_index, db)                               # upstream's default target_ind = 20
    with pytest.raises(ValueError, match="target_ind == ref_ind"):
        pair_terms_from_config(pc(params={"target_ind": 1, "ref_ind": 1}), scene_index, db)
    with pytest.raises(ValueError, match="min"):
        pair_terms_from_config(pc("gptkeepdistance", params={"target_ind": 0, "ref_ind": 1, "min_distance": 9.0, "max_distance": 8.0}), scene_index, db)
    with pytest.raises(ValueError, match="min"):
        pair_terms_from_config(pc("gptstayaway", params={"target_ind": 0, "ref_ind": 1, "min_dist": 16.0}), scene_index, db)
    with pytest.raises(NotImplementedError, match="agents"):
        pair_terms_from_config(pc(agents=[0, 1], params={"target_ind": 0, "ref_ind": 1}), scene_index, db)


def test_guidance_from_config_still_refuses_the_names_and_set_guidance_takes_them():
    from cld_amd.dm_model import repeat_guidance
    from cld_amd.policy import PAIR_NAMES, CldPolicy, guidance_from_config, refresh_pair_term
    cfg, scene_index, db = _cfg()
    for name in PAIR_NAMES:
        with pytest.raises(NotImplementedError, match="is not built"):
            guidance_from_config([[{"name": name, "weight": 1.0, "agents": None, "params": {"target_ind": 0, "ref_ind": 1}}], []], scene_index, data_batch=db)
    pol = CldPolicy(None, None)
    pol.set_guidance(cfg, scene_index, data_batch=db, lr=0.05)
    g = pol._guidance
    assert g["pair"]["target"] == [3, 0, 8, 6, 4] and "speed_limit" in g and g["lr"] == 0.05 and "social_group" not in g
    assert pol._guidance_cfg[0] is cfg
    only = [[cfg[0][0]], []]                                               # nothing but a pair: still a guidance
    pol.set_guidance(only, scene_index, data_batch=db)
    assert set(pol._guidance) == {"pair"}
    both = [[cfg[0][0], {"name": "social_group", "weight": 1.0, "agents": [1, 2], "params": {}}], []]
    pol.set_guidance(both, scene_index, data_batch=db)
    assert set(pol._guidance) == {"pair", "social_group"} and pol._guidance["social_group"]["groups"] == [[1, 2]]
    with pytest.raises(ValueError):
        pol.set_guidance([[], []], scene_index, data_batch=db)
    rep = repeat_guidance({"pair": g["pair"]}, 4)
    assert rep["pair"]["num_samp"] == 4 and "num_samp" not in g["pair"]
    W2 = torch.eye(3).repeat(9, 1, 1) * 2
    g2 = refresh_pair_term(g, {"world_from_agent": W2})
    assert g2["pair"]["world_from_agent"] is W2 and g2["pair"]["agent_from_world"] is None and g["pair"]["world_from_agent"] is db["world_from_agent"]
    g3 = refresh_pair_term(g, {"world_from_agent": W2, "agent_from_world": db["world_from_agent"]})
    assert g3["pair"]["agent_from_world"] is db["world_from_agent"]
    assert refresh_pair_term(g, {}) is g


def test_pair_incidences_list_every_agent_once_in_ascending_order():
    from cld_amd.engine import pair_incidences
    #        pair 0      1       2       3 (ref outside)  4 (target == ref)
    target = [5, 2, 5, 1, 4]
    ref = [2, 7, 0, 9, 4]
    ids, start, inc = pair_incidences(target, ref, 8)
    assert ids == [0, 1, 2, 4, 5, 7] and start == [0, 1, 2, 4, 6, 8, 9]
    assert inc == [5, 6, 1, 2, 8, 9, 0, 4, 3]          # agent 2: ref of pair 0 (1), target of pair 1 (2); agent 5: target of 0 and 2
    assert pair_incidences([], [], 4) == ([], [0], [])


def test_cld_pair_term_layout_matches_the_header():
    """ctypes mirror of `cld_pair_term` against include/cld.h, field by field in declaration order; the pinned structs keep their size."""
    from cld_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "cld.h")).read()
    body = re.search(r"typedef struct cld_pair_term \{(.*?)\} cld_pair_term;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [(m.group(2), "*" in m.group(1)) for m in re.finditer(r"([A-Za-z_0-9 ]+\*?)\s*\b([a-z_]+);", body)]
    assert [n for n, _ in fields] == [n for n, _ in _lib.CldPairTerm._fields_]
    off = 0
    for (name, is_ptr), (_, ctype) in zip(fields, _lib.CldPairTerm._fields_):
        size = 8 if is_ptr else 4
        assert (ctype is ctypes.c_void_p) == is_ptr and ctypes.sizeof(ctype) == size, name
        assert getattr(_lib.CldPairTerm, name).offset == off, name
        off += size
    assert ctypes.sizeof(_lib.CldPairTerm) == 112 and _lib.CldPairTerm.num_pairs.offset == 96
    assert ctypes.sizeof(_lib.CldGuidance) == 144 and ctypes.sizeof(_lib.CldCollision) == 88 and ctypes.sizeof(_lib.CldGoal) == 80 and ctypes.sizeof(_lib.CldSocialGroup) == 104
    enum = dict((m.group(1).lower(), int(m.group(2))) for m in re.finditer(r"CLD_PAIR_([A-Z_]+) = (\d)", hdr))
    assert enum == _lib.PAIR_KINDS and tuple(sorted(enum, key=enum.get)) == Y.KINDS
    for sym in ("cld_pair_loss", "cld_set_pair_term"):
        assert sym in _lib.SIGNATURES and re.search(r"\b" + sym + r"\s*\(", hdr)
    assert len(_lib.SIGNATURES) == 88 and all(re.search(r"\b" + s + r"\s*\(", hdr) for s in _lib.SIGNATURES)      # 88 entry points in all
    if os.path.exists(_lib.LIB_PATH):                                      # where the library is built: it exports both
        lib = _lib.load()
        assert lib.cld_pair_loss.argtypes[2]._type_ is _lib.CldPairTerm and lib.cld_set_pair_term.restype is ctypes.c_int
