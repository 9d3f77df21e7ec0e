"""Host side of the guidance satisfaction metrics: the float64 restatement (tests/guide_metrics_cases.py) against
tests/golden/guide_metrics.npz, which tests/tools/record_guide_metrics_golden.py recorded from the reference's own GuidanceMetric
classes; upstream's key names and order; the errors; and the conversion from the config `set_guidance` takes (excluded_agents and
target_speed by batch row) to what the classes index by scene-local agent.  No GPU.

The restatement and the reference are both float64; they may differ in the order of a sum and in a fused multiply-add inside a
matrix product, so distance and speed values are compared within (n + 16) 2^-52 max(|term|, |coordinate|), n the summed terms -- the
bound the kernel test uses -- and flag-derived values exactly.
"""
import json
import os

import numpy as np
import pytest

from tests import guide_metrics_cases as GC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "guide_metrics.npz")


@pytest.fixture(scope="module")
def gold():
    z = np.load(GOLDEN)
    return z, json.loads(bytes(z["meta"]).decode())


def close(got, ref, n, scale):
    if np.isnan(ref) or np.isinf(ref):
        return (np.isnan(got) and np.isnan(ref)) or got == ref
    return abs(got - ref) <= (n + 16) * 2.0 ** -52 * scale


@pytest.mark.parametrize("name", ["main", "small"])
def test_restatement_equals_the_golden(gold, name):
    z, meta = gold
    case = GC.case(name)
    pre = "" if name == "main" else "small_"
    for k in ("world", "speed", "acc", "extent", "scene_start"):
        assert np.array_equal(case[k], z[pre + k], equal_nan=True), k
    if name == "main":
        for k in ("maps", "scene_map", "map_from_world"):
            assert np.array_equal(case[k], z[k]), k
    rs = case["restated"]
    keys = meta[pre + "keys"]
    assert [e["key"] for e in rs["table"]] == keys
    assert np.array_equal(rs["partner"], z[pre + "partner"])
    for ent, ref in zip(rs["table"], z[pre + "values"]):
        got = rs["values"][ent["key"]]
        if ent["kind"] in GC.FLAG_KINDS:
            assert got == ref, (ent["key"], got, ref)
        else:
            assert close(got, ref, rs["n_terms"][ent["key"]], rs["scale"][ent["key"]]), (ent["key"], got, ref)


def test_the_case_covers_what_it_should():
    case = GC.case("main")
    rs = case["restated"]
    assert rs["rel_margin"] >= GC.REL_MARGIN and rs["pix_margin"] >= GC.PIX_MARGIN
    kinds = {e["kind"] for e in rs["table"]}
    from cld_amd._lib import GUIDE_METRIC_KINDS
    assert kinds == set(GUIDE_METRIC_KINDS)                                     # every kind at least once
    ss = case["scene_start"]
    p0 = rs["partner"][0]
    assert p0[ss[0]] == ss[0] + 1 and p0[ss[0] + 1] == ss[0]                    # an excluded pair; the partner of 0 is above it
    assert rs["per_member"]["guide_agent_collision_s0g0"][:3].tolist() == [0.0, 0.0, 1.0]
    assert (rs["partner"][:, ss[1] + 68] == ss[1] + 69).any()                   # a partner in the second stride of 64
    assert np.isinf(rs["values"]["guide_social_group_s2g0"])
    v = rs["values"]
    assert 0.0 < v["guide_map_collision_s0g1"] < 1.0 and 0.0 < v["guide_agent_collision_disk_s1g0"] < v["guide_social_dist_s1g0"] < 1.0
    small = GC.case("small")["restated"]["values"]
    assert np.isnan(small["guide_global_target_pos_at_time_s0g0"]) and np.isnan(small["guide_target_pos_at_time_s0g1"])
    assert np.isnan(small["guide_speed_limit_s0g4"]) and np.isfinite(small["guide_target_speed_s0g3"])
    assert small["guide_global_target_pos_s0g2"] == 0.75


def test_key_names_and_order_are_upstreams(gold):
    from cld_amd.metrics import guidance_metric_names
    _, meta = gold
    main, small = GC.case("main"), GC.case("small")
    assert guidance_metric_names(main["config"], main["constraint"]) == meta["keys"]
    assert guidance_metric_names(small["config"]) == meta["small_keys"]
    assert meta["keys"][:3] == ["guide_agent_collision_disk_s0g0", "guide_social_dist_s0g0", "guide_agent_collision_s0g0"]
    assert meta["keys"][3:5] == ["guide_map_collision_s0g1", "guide_map_collision_disk_s0g1"]
    assert meta["keys"][-3:] == ["guide_constraint_s0", "guide_constraint_s1", "guide_constraint_s2"]
    assert "guide_agent_collision_s0g5" in meta["keys"]                         # two configs of one name in a scene
    assert guidance_metric_names([[], []], [None, dict(locs=[[0.0, 0.0]], times=[1], agents=[0])]) == ["guide_constraint_s1"]


@pytest.mark.parametrize("name", ["stop_sign", "global_stop_sign", "gpt", "gptcollision", "gptkeepdistance", "lane_keeping"])
def test_unknown_names_raise(name):
    from cld_amd.metrics import guidance_metric_names, guidance_metric_table
    cfg = [[dict(name="speed_limit", weight=1.0, params=dict(speed_limit=1.0), agents=None)],
           [dict(name=name, weight=1.0, params={}, agents=None)]]
    with pytest.raises(ValueError, match=f"Unknown guidance metric: {name}"):
        guidance_metric_names(cfg)
    with pytest.raises(ValueError, match=f"Unknown guidance metric: {name}"):
        guidance_metric_table(cfg, [0, 2, 5])


def test_batch_rows_become_scene_local():
    from cld_amd.metrics import guidance_metric_table
    ts = np.arange(9 * 4, dtype=np.float64).reshape(9, 4)
    cfg = [[dict(name="agent_collision", weight=1.0, params=dict(excluded_agents=[3, 1, 8]), agents=[0, 1, 3])],
           [],
           [dict(name="target_speed", weight=1.0, params=dict(target_speed=ts), agents=[2, 0]),
            dict(name="agent_collision", weight=1.0, params=dict(excluded_agents=[8, 6, 0], buffer_dist=0.75), agents=None)]]
    t = {e["key"]: e for e in guidance_metric_table(cfg, [0, 4, 6, 9], [None, dict(locs=[[1.0, 2.0]], times=[3], agents=[1]), None])}
    a = t["guide_agent_collision_s0g0"]
    assert a["members"] == [0, 1, 3] and a["excluded"] == [1, 3] and a["excluded_local"] == [1, 3]      # row 8 is another scene's
    assert t["guide_social_dist_s0g0"]["params"] == [0.2]
    s = t["guide_target_speed_s2g0"]
    assert s["members"] == [8, 6] and s["params"] == [4.0] + ts[8].tolist() + ts[6].tolist()             # by batch row, in `agents` order
    b = t["guide_social_dist_s2g1"]
    assert b["members"] == [6, 7, 8] and b["excluded"] == [6, 8] and b["excluded_local"] == [0, 2] and b["params"] == [0.75]
    c = t["guide_constraint_s1"]
    assert c["members"] == [5] and c["kind"] == "target_pos_at_time" and c["params"] == [1.0, 2.0, 3.0]
    with pytest.raises(ValueError, match="one entry per scene"):
        guidance_metric_table(cfg, [0, 4, 9])
    with pytest.raises(ValueError, match="agents"):
        guidance_metric_table([[dict(name="speed_limit", weight=1.0, params=dict(speed_limit=1.0), agents=[4])]], [0, 4])
