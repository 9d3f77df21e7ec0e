"""Host-side checks of the social-group guidance (`social_group`): the fp64 yardstick (tests/social_yardstick.py) against the
recording made from the reference's own class (tests/golden/social_group.npz, tests/tools/record_social_golden.py), the numpy
replica of the on-device draws, the configuration adapter and the ctypes layout of `cld_social_group`."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from cld_amd import synth
from tests import social_replica as SR
from tests import social_yardstick as Y

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["coh0", "coh06", "coh1", "noleader"]


def recorded_case(golden, name):
    """-> (meta, arrays, plans [A,N,52,6] float32, yardstick term, draws r / u [A,N,52], the config's agents)."""
    meta, g = golden("social_group")
    A, N = meta["A"], meta["N"]
    speed = synth.make_collision_scene([A], meta["seed"])["curr_speed"]
    plans = torch.from_numpy(synth.make_collision_trajectories(A, N, speed, meta["seed"]))
    case = meta["cases"][name]
    term = Y.term_from_meta(case, g["world_from_agent"], N)
    r = torch.from_numpy(g[name + "_draw_r"]).reshape(A, N, 52)
    u = torch.from_numpy(g[name + "_draw_u"]).reshape(A, N, 52)
    return meta, g, plans, term, r, u, list(case["agents"])


def check_margins(plans, term, r, u):
    """The fixture conditions, no row excluded: where the nearest neighbour is used the second-nearest is >= 1e-3 m farther, no read
    distance below 1e-2 m, no u within 1e-6 of cohesion."""
    gap, dmin, umin = Y.margins(plans.double(), term, r, u)
    assert gap >= 1e-3 and dmin >= 1e-2 and umin >= 1e-6, (gap, dmin, umin)
    return gap, dmin, umin


@pytest.mark.parametrize("name", CASES)
def test_yardstick_matches_the_reference_recording(golden, name):
    """Values <= 2e-5 max(1, max|ref|), gradient <= 1e-4 max|ref grad| (the bars of the goal recording); exactly zero gradient for the
    leader and outside the group; the recorded rows keep the margins the kernel tests rely on."""
    meta, g, plans, term, r, u, idx = recorded_case(golden, name)
    ref_v, ref_g = g[name + "_values"], g[name + "_grad"]
    outside = np.ones(meta["A"], bool); outside[idx] = False
    assert np.isnan(ref_v[outside]).all() and not np.isnan(ref_v[idx]).any()
    v, grad = Y.value_and_grad(plans.double(), term, r, u)
    err_v = np.abs(v.numpy()[idx] - ref_v[idx]).max()
    err_g = np.abs(grad.numpy() - ref_g).max()
    gap, dmin, umin = check_margins(plans, term, r, u)
    print(f"{name}: value error {err_v:.2e} (max|ref| {np.abs(ref_v[idx]).max():.3f}), gradient error {err_g:.2e} (max|ref| {np.abs(ref_g).max():.3e}); "
          f"margins: neighbour {gap:.3e} m, distance {dmin:.3e} m, u {umin:.3e}")
    assert err_v <= 2e-5 * max(1.0, np.abs(ref_v[idx]).max())
    assert np.abs(ref_g).max() > 0 and err_g <= 1e-4 * np.abs(ref_g).max()
    assert abs(float(Y.total(plans.double(), term, r, u)) - float(g[name + "_total"][0])) <= 2e-5 * max(1.0, abs(float(g[name + "_total"][0])))
    leader = meta["cases"][name]["leader_idx"]
    quiet = outside.copy()
    if leader in idx:
        quiet[leader] = True
    assert float(np.abs(grad.numpy()[quiet]).max()) == 0.0 and float(np.abs(ref_g[quiet]).max()) == 0.0
    assert float(np.abs(grad.numpy()[..., 2:]).max()) == 0.0
    assert all(float(np.abs(ref_g[a]).max()) > 0.0 for a in idx if a != leader)


def test_the_recording_holds_the_cases_it_is_meant_to(golden):
    meta, g = golden("social_group")
    cases = meta["cases"]
    assert [cases[n]["cohesion"] for n in CASES] == [0.0, 0.6, 1.0, 0.6]
    assert all(cases[n]["leader_idx"] in cases[n]["agents"] for n in CASES[:3]) and cases["noleader"]["leader_idx"] not in cases["noleader"]["agents"]
    assert len(cases["coh0"]["agents"]) == 6 and meta["A"] == 8 and meta["N"] == 2
    # the same draws with and without a leader: equal values, and the detached member's gradient is the difference
    assert np.array_equal(g["coh06_draw_r"], g["noleader_draw_r"]) and np.array_equal(g["coh06_values"], g["noleader_values"], equal_nan=True)
    lead = cases["coh06"]["leader_idx"]
    assert float(np.abs(g["coh06_grad"][lead]).max()) == 0.0 and float(np.abs(g["noleader_grad"][lead]).max()) > 0.0
    # cohesion 0.6 takes both kinds of neighbour, cohesion 1 only drawn ones, and the draws stay inside [0, M - 2]
    M = len(cases["coh06"]["agents"])
    rows = np.repeat(np.isin(np.arange(meta["A"]), cases["coh06"]["agents"]), meta["N"])
    u = g["coh06_draw_u"][rows]
    assert 0.4 < float((u < np.float32(0.6)).mean()) < 0.8
    for n in CASES:
        r = g[n + "_draw_r"][rows]
        assert r.min() >= 0 and r.max() <= M - 2
    for n in CASES:                                                   # the reference's own float32 error, which a float32 kernel's bar may lean on
        assert cases[n]["ref_value_err"] <= 2e-5 * max(1.0, cases[n]["max_value"])


def test_replica_draws_stay_in_range_and_have_the_moments_of_uniform_draws():
    A, N = 40, 3
    groups = [list(range(0, 2)), list(range(5, 8)), list(range(10, 35))]
    size = SR.group_size_of_row(groups, A, N)
    assert size.shape == (A * N,) and size[0] == 2 and size[3 * N] == 0 and size[5 * N] == 3 and size[34 * N + 2] == 25 and size[35 * N] == 0
    r, u = SR.draws(7, 3, 1, size)
    assert r.dtype == np.int32 and u.dtype == np.float32 and r.shape == (A * N, 52) == u.shape
    assert float(u.min()) > 0.0 and float(u.max()) <= 1.0
    for M in (2, 3, 25):
        rows = size == M
        rr = r[rows].astype(np.float64)
        assert rr.min() >= 0 and rr.max() <= M - 2
        n = rr.size
        if M > 2:                                                    # uniform on {0 .. M-2}: mean (M-2)/2, variance ((M-1)^2 - 1)/12
            assert rr.max() == M - 2 and rr.min() == 0
            assert abs(rr.mean() - (M - 2) / 2) <= 5 * np.sqrt(((M - 1) ** 2 - 1) / 12 / n)
            assert abs(rr.var() - ((M - 1) ** 2 - 1) / 12) <= 0.1 * ((M - 1) ** 2 - 1) / 12
    assert np.all(r[size == 0] == 0)
    uu = u.astype(np.float64)
    assert abs(uu.mean() - 0.5) <= 5 * np.sqrt(1 / 12 / uu.size) and abs(uu.var() - 1 / 12) <= 0.05 / 12
    # another evaluation index, another seed: other draws; the same key: the same draws
    r2, u2 = SR.draws(7, 3, 2, size)
    r3, u3 = SR.draws(7, 4, 1, size)
    r4, u4 = SR.draws(8, 3, 1, size)
    for ub in (u2, u3, u4):
        assert float((ub == u).mean()) < 0.01
    ra, ua = SR.draws(7, 3, 1, size)
    assert np.array_equal(ra, r) and np.array_equal(ua, u)
    # no value is shared with the diffusion noise of the same seed: the keys differ (splitmix64 is a bijection)
    from tests import noise_replica as NR
    assert SR.eval_index(3, 1) == (3 << 16) + 1 and SR.TAG != 0
    assert int(NR.splitmix64(np.uint64(SR.TAG ^ SR.eval_index(0, 0)))) != 0


def _cfg():
    scene_index = torch.tensor([4, 4, 4, 4, 9, 9, 9, 9, 9])
    cfg = [[{"name": "social_group", "weight": 3.0, "agents": [3, 0, 2], "params": {"leader_idx": 2, "social_dist": 2.0, "cohesion": 0.25}},
            {"name": "speed_limit", "weight": 3.0, "params": {"speed_limit": 6.0}, "agents": None}],
           [{"name": "speed_limit", "weight": 1.0, "params": {"speed_limit": 6.0}, "agents": None},
            {"name": "social_group", "weight": 0.5, "agents": None, "params": {}}]]
    db = {"world_from_agent": torch.eye(3).repeat(9, 1, 1)}
    return cfg, scene_index, db


def test_social_groups_from_config_peels_the_groups_and_folds_the_scales():
    from cld_amd.policy import guidance_from_config, social_groups_from_config
    cfg, scene_index, db = _cfg()
    rest, term = social_groups_from_config(cfg, scene_index, db)
    assert [[c["name"] for c in s] for s in rest] == [["speed_limit"], ["speed_limit"]] and rest[0][0] is cfg[0][1]
    assert [[c["name"] for c in s] for s in cfg] == [["social_group", "speed_limit"], ["speed_limit", "social_group"]]        # the input is not modified
    assert term["groups"] == [[0, 2, 3], [4, 5, 6, 7, 8]]                  # `agents` index the scene's members; ascending
    assert term["leader"] == [2, 0]                                        # batch indices, upstream's default 0 (names no member of scene 1)
    assert term["social_dist"] == [2.0, 1.5] and term["cohesion"] == [0.25, 0.8]
    assert np.allclose(term["scale"], [3.0 / 3, 0.5 / 5])                  # weight / members
    assert term["world_from_agent"] is db["world_from_agent"]
    assert "speed_limit" in guidance_from_config(rest, scene_index)
    plain = [[cfg[0][1]], [cfg[1][0]]]
    rest2, term2 = social_groups_from_config(plain, scene_index, None)     # nothing to peel: no data_batch needed
    assert term2 is None and rest2 == plain


def test_social_groups_from_config_errors():
    from cld_amd.policy import social_groups_from_config
    cfg, scene_index, db = _cfg()
    sg = lambda **kw: dict({"name": "social_group", "weight": 1.0, "agents": None, "params": {}}, **kw)
    with pytest.raises(ValueError, match="world_from_agent"):
        social_groups_from_config(cfg, scene_index, None)
    with pytest.raises(ValueError, match="world_from_agent"):
        social_groups_from_config(cfg, scene_index, {"extent": torch.ones(9, 3)})
    with pytest.raises(ValueError, match="at least 2"):
        social_groups_from_config([[sg(agents=[1])], []], scene_index, db)
    with pytest.raises(ValueError, match="two groups"):
        social_groups_from_config([[sg(agents=[0, 1]), sg(agents=[1, 2])], []], scene_index, db)
    with pytest.raises(ValueError, match="two groups"):
        social_groups_from_config([[sg(agents=[1, 1])], []], scene_index, db)
    for coh in (-0.1, 1.5):
        with pytest.raises(ValueError, match="cohesion"):
            social_groups_from_config([[sg(params={"cohesion": coh})], []], scene_index, db)


def test_guidance_from_config_still_refuses_social_group_and_set_guidance_takes_it():
    from cld_amd.policy import CldPolicy, guidance_from_config
    cfg, scene_index, db = _cfg()
    with pytest.raises(NotImplementedError, match="global_target_pos"):
        guidance_from_config(cfg, scene_index, data_batch=db)
    pol = CldPolicy(None, None)
    pol.set_guidance(cfg, scene_index, data_batch=db, lr=0.05, social_seed=11)
    g = pol._guidance
    assert g["social_group"]["groups"] == [[0, 2, 3], [4, 5, 6, 7, 8]] and g["social_group"]["seed"] == 11 and "speed_limit" in g and g["lr"] == 0.05
    assert pol._guidance_cfg[0] is cfg and pol.social_iter == 0
    only = [[cfg[0][0]], []]                                               # nothing but a social group: still a guidance
    pol.set_guidance(only, scene_index, data_batch=db)
    assert set(pol._guidance) == {"social_group"}
    with pytest.raises(ValueError):
        pol.set_guidance([[], []], scene_index, data_batch=db)
    from cld_amd.dm_model import repeat_guidance
    rep = repeat_guidance({"social_group": g["social_group"]}, 4)
    assert rep["social_group"]["num_samp"] == 4 and "num_samp" not in g["social_group"]
    from cld_amd.policy import refresh_social_term
    W2 = torch.eye(3).repeat(9, 1, 1) * 2
    g2 = refresh_social_term(g, {"world_from_agent": W2})
    assert g2["social_group"]["world_from_agent"] is W2 and g["social_group"]["world_from_agent"] is db["world_from_agent"]
    assert refresh_social_term(g, {}) is g


def test_cld_social_group_layout_matches_the_header():
    """ctypes mirror of `cld_social_group` against include/cld.h, field by field in declaration order; the pinned structs keep their size."""
    from cld_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "cld.h")).read()
    body = re.search(r"typedef struct cld_social_group \{(.*?)\} cld_social_group;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [(m.group(2), "*" in m.group(1), "64" in m.group(1)) for m in re.finditer(r"([A-Za-z_0-9 ]+\*?)\s*\b([a-z_]+);", body)]
    assert [n for n, _, _ in fields] == [n for n, _ in _lib.CldSocialGroup._fields_]
    off = 0
    for (name, is_ptr, wide), (_, ctype) in zip(fields, _lib.CldSocialGroup._fields_):
        size = 8 if is_ptr or wide else 4
        assert (ctype is ctypes.c_void_p) == is_ptr and ctypes.sizeof(ctype) == size, name
        off = (off + size - 1) // size * size
        assert getattr(_lib.CldSocialGroup, name).offset == off, name
        off += size
    assert ctypes.sizeof(_lib.CldSocialGroup) == 104 and _lib.CldSocialGroup.seed.offset == 72 and _lib.CldSocialGroup.n_opt.offset == 100
    assert ctypes.sizeof(_lib.CldGuidance) == 144 and ctypes.sizeof(_lib.CldCollision) == 88 and ctypes.sizeof(_lib.CldGoal) == 80
    assert _lib.SOCIAL_MAX_MEMBERS == 128 and re.search(r"2 <= max_members <= 128", hdr)
    for sym in ("cld_social_group_loss", "cld_set_social_term"):
        assert sym in _lib.SIGNATURES and re.search(r"\b" + sym + r"\s*\(", hdr)
    if os.path.exists(_lib.LIB_PATH):                                      # where the library is built: it exports both
        lib = _lib.load()
        assert lib.cld_social_group_loss.argtypes[2]._type_ is _lib.CldSocialGroup and lib.cld_set_social_term.restype is ctypes.c_int
