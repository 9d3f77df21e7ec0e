"""CPU tests of tests/guide_cases.py: that the inputs of tests/test_gpu_guide.py reach the branches of the roll-out gradient
(chain_grad / chain_grad_group in csrc/guide_kernels.hip) they claim to reach, shown with the float64 oracle alone, and that the kink
shares stay under their caps.

  * `chain` (the quantities the roll-out compares) is the oracle's roll-out: its v, acc and yaw rate equal the trajectory bit for bit;
  * every regime on at least 20 (agent, step) pairs of agents that are not kink-adjacent, in the weight sets named in REACH;
  * every per-agent variant (zero scale, NaN targets, target_time 0 / 51, m = 0 / 51) on at least three such agents;
  * the condition of the GPU tests: at most 2 % of the agents of a case kink-adjacent (none, at 41 agents), at most 1 % of the rows of a
    large batch;
  * on the cool set both float32 references lie inside the absolute bars of tests/test_gpu_parity.py around float64;
  * rows of a large batch mean the same as rows of a small one.

Measured (seed 45; pairs of non-kink agents out of 41 x 52 = 2132):
  hot    acceleration below acce_lo 43, above acce_hi 701, inside 1388; raw speed below v_lo 39, above v_hi 167, inside 1926; speed limit
         on 1717, off 415; acceleration limit +1241, -329, off 562; yaw-rate clip off 1672, 0.5 |v| 49, max_yawvel / |v| 392
  steer  yaw-rate clip off 1111, 0.5 |v| 252, max_yawvel / |v| 500, 0.1 floor 269, active below v = 0 (sign(v) = -1) 99; v_k < 0 313
  cool   raw speed below v_lo 156 and above v_hi 52 (agents that start outside the bounds and stay there), inside 1924
  kink-adjacent agents: none in any of the 21 (set, case) pairs; large batches (seed 51) 0.29 .. 0.80 % of the rows.
"""
import pytest
import torch

import guide_cases as GC
from oracle import cld_oracle as O

REACH = {
    "hot": ("acc_lo", "acc_hi", "acc_in", "v_lo", "v_hi", "v_in", "sl_on", "sl_off", "al_pos", "al_neg", "al_off", "yaw_free", "yaw_steer",
            "yaw_yawvel", "v_negative"),
    "steer": ("yaw_free", "yaw_steer", "yaw_yawvel", "yaw_floor", "yaw_bound_backwards", "v_negative", "sl_on", "sl_off", "al_pos",
              "al_neg", "al_off", "acc_in", "v_in"),
    "cool": ("acc_in", "v_lo", "v_hi", "v_in", "yaw_free", "sl_on", "sl_off", "al_pos", "al_off", "v_negative"),
}
# the absolute bars of tests/test_gpu_parity.py, as fractions of max|g|: 2e-5, and 1e-4 wherever the gradient runs through positions
COOL_BAR = {"target_speed": 2e-5, "speed_limit": 2e-5, "acc_limit": 2e-5, "waypoint": 1e-4, "target_pos": 1e-4, "ext_grad": 1e-4,
            "combined": 1e-4}


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_chain_is_the_oracles_rollout(dtype):
    inp = GC.inputs(GC.B_REG)
    for kind in GC.KINDS:
        f = GC.forward(kind, inp, dtype)
        traj = O.decode(O.to_torch(GC.decoder_weights(kind), dtype), inp["mean"].to(dtype), inp["cond"].to(dtype),
                        inp["curr_states"].to(dtype), True)
        assert torch.equal(f["traj"], traj)
        assert torch.equal(f["v"][:, 1:], traj[..., 2]) and torch.equal(f["acc"], traj[..., 4]) and torch.equal(f["wr"], traj[..., 5])
        yb = f["yb"]
        yaw = torch.cumsum(torch.cat((inp["curr_states"][:, 3:4].to(dtype), torch.maximum(torch.minimum(f["wr"], yb), -yb) * 0.1), 1), 1)
        assert torch.equal(yaw[:, 1:], traj[..., 3])


@pytest.mark.parametrize("kind", GC.KINDS)
def test_every_regime_is_reached(kind):
    adj, _ = GC.regime_kinks(kind, "combined")           # the combined case makes every comparison: the widest set of kink-adjacent agents
    rg = GC.regimes(kind, GC.forwards(kind)["f64"])
    counts = {k: int(v[~adj].sum()) for k, v in rg.items()}
    print(f"\n[guide host] {kind}: {counts}")
    for name in REACH[kind]:
        assert counts[name] >= GC.MIN_PAIRS, (kind, name, counts[name])
    for name in ("acc_lo", "acc_hi", "acc_in", "v_lo", "v_hi", "v_in", "yaw_free", "yaw_steer", "yaw_yawvel", "yaw_floor",
                 "yaw_bound_backwards", "v_negative", "sl_on", "sl_off", "al_pos", "al_neg", "al_off"):
        assert any(name in REACH[k] for k in GC.KINDS), name


@pytest.mark.parametrize("kind", GC.KINDS)
def test_every_per_agent_variant_is_held(kind):
    inp = GC.inputs(GC.B_REG)
    live = inp["tp_scale"] != 0
    for case, variants in (("target_speed", {"zero scale": inp["loss_scale"] == 0,
                                             "NaN targets": torch.isnan(inp["target_speed"]).any(dim=1) & (inp["loss_scale"] != 0),
                                             "both signs": torch.ones(GC.B_REG, dtype=torch.bool)}),
                           ("speed_limit", {"zero scale": inp["sl_scale"] == 0}), ("acc_limit", {"zero scale": inp["al_scale"] == 0}),
                           ("waypoint", {"zero scale": ~live, "time 0": live & (inp["time_at"] == 0), "time 51": live & (inp["time_at"] == 51),
                                         "between": live & (inp["time_at"] > 0) & (inp["time_at"] < 51)}),
                           ("target_pos", {"m = 0": live & (inp["time_from"] == -1), "m = 51": live & (inp["time_from"] == -52),
                                           "between": live & (inp["time_from"] < -1) & (inp["time_from"] > -52)}),
                           ("combined", {"time 0": live & (inp["row"] % 2 == 0) & (inp["time_at"] == 0),
                                         "time 51": live & (inp["row"] % 2 == 0) & (inp["time_at"] == 51),
                                         "m = 0": live & (inp["row"] % 2 == 1) & (inp["time_from"] == -1),
                                         "m = 51": live & (inp["row"] % 2 == 1) & (inp["time_from"] == -52)})):
        adj, _ = GC.regime_kinks(kind, case)
        for name, mask in variants.items():
            assert int((mask & ~adj).sum()) >= GC.MIN_AGENTS, (kind, case, name)
    # both signs of v - target, on steps with a target, of agents with a scale
    f = GC.forwards(kind)["f64"]
    df = (f["v"][:, 1:] - inp["target_speed"].double())[inp["loss_scale"] != 0]
    assert int((df > 0).sum()) >= GC.MIN_PAIRS and int((df < 0).sum()) >= GC.MIN_PAIRS


@pytest.mark.parametrize("case", GC.CASES)
@pytest.mark.parametrize("kind", GC.KINDS)
def test_kink_share_of_the_regime_batch(kind, case):
    adj, record = GC.regime_kinks(kind, case)
    print(f"\n[guide host] {kind} {case}: {int(adj.sum())} kink-adjacent of {GC.B_REG}; deviations "
          + ", ".join(f"{k} {d:.2g}" for k, (d, _) in record.items()))
    assert float(adj.double().mean()) <= 0.02, (kind, case, record)
    assert not bool(adj[0]), "the B = 1 prefix is kink-adjacent"


@pytest.mark.parametrize("form,B,passes,other", GC.BIG_CASES)
def test_kink_share_of_the_large_batches(form, B, passes, other):
    rows, groups = GC.big_subset(form, B)
    n, per = GC.GROUP["mfma" if form == "auto" else form], GC.GRID["mfma" if form == "auto" else form]
    assert len(rows) <= 64 and (B + n - 1) // n > (passes - 1) * per and (B + n - 1) // n <= passes * per
    assert {0, per - 1, per, (B - 1) // n} <= set(groups) and any(0 < g < per - 1 and g != 1 for g in groups)
    no, pero = GC.GROUP[other], GC.GRID[other]
    # the form it is paired with splits the rows into another number of passes (fewer, but for the 16-agent kernel, which has none fewer)
    assert ((B + no - 1) // no + pero - 1) // pero != passes
    adj, record = GC.big_kinks(form, B)
    both = adj | GC.big_kinks(other, B)[0]
    print(f"\n[guide host] hot combined {form} B={B}: {100 * float(adj.double().mean()):.2f} % of the rows kink-adjacent "
          f"({100 * float(both.double().mean()):.2f} % with the subset of {other}); {len(rows)} rows with references, groups {groups}")
    assert float(adj.double().mean()) <= 0.01 and float(both.double().mean()) <= 0.01, record
    assert float(adj[list(rows)].double().mean()) <= 0.02


@pytest.mark.parametrize("case", GC.CASES)
def test_float32_references_inside_the_absolute_bars_on_the_cool_set(case):
    g = GC.grads("cool", case)
    adj, _ = GC.regime_kinks("cool", case)
    gmax = float(g["f64"].abs().max())
    for p in ("f32", "f32fast"):
        err = float((g[p].double() - g["f64"])[~adj].abs().max())
        print(f"\n[guide host] cool {case} {p}: {err / gmax:.3g} of max|g| = {gmax:.3g}")
        assert err < COOL_BAR[case] * gmax, (case, p, err / gmax)


@pytest.mark.parametrize("kind", GC.KINDS)
def test_references_are_finite_and_zero_where_every_term_is_off(kind):
    inp = GC.inputs(GC.B_REG)
    off = inp["loss_scale"] == 0
    assert int(off.sum()) >= GC.MIN_AGENTS
    for case in GC.CASES:
        for p, g in GC.grads(kind, case).items():
            assert bool(torch.isfinite(g).all()), (kind, case, p)
            if case not in ("ext_grad", "combined"):
                assert float(g[off].abs().max()) == 0.0, (kind, case, p)
        # (an agent held on a speed bound for the whole horizon has no gradient through its speed either, nor one that stays below the limit)
        assert int((GC.grads(kind, case)["f64"][~off].abs().amax(dim=(1, 2)) > 0).sum()) >= 10, (kind, case)


def test_rows_of_a_large_batch_are_rows_of_a_small_one():
    """Agents are independent in the reference: the subset of a large batch, its halves on their own, and the regime batch's prefix."""
    form, B = "quad", 2049
    rows, _ = GC.big_subset(form, B)
    whole = GC.grads("hot", "combined", B, rows)["f64"]
    half = len(rows) // 2
    parts = torch.cat([GC.oracle_grad("hot", "combined", GC.take(GC.inputs(B), r), torch.float64) for r in (rows[:half], rows[half:])])
    assert float((whole - parts).abs().max()) <= 1e-12 * float(whole.abs().max())
    one = GC.oracle_grad("hot", "combined", GC.take(GC.inputs(GC.B_REG), (0,)), torch.float64)
    ref = GC.grads("hot", "combined")["f64"]
    assert float((one - ref[:1]).abs().max()) <= 1e-12 * float(ref.abs().max())
    small, large = GC.inputs(100), GC.inputs(300)
    for k in small:
        assert torch.equal(small[k], large[k][:100], ) or (k == "target_speed" and torch.equal(torch.nan_to_num(small[k]), torch.nan_to_num(large[k][:100])))


def test_float_running_sums_are_what_put_a_position_gradient_over_the_bar():
    """Why chain_grad / chain_grad_group carry their running sums in double.  The oracle's own float32 arithmetic with the roll-out's
    running sums (and their adjoints) carried in float32 -- what the kernels did -- against the same with torch.cumsum, which carries a
    float32 sum in float64: on the single slow agent of B = 1 (TargetPosLoss from the first step on, gradient 9e-7) the float sums are
    3.6e-12 off float64, torch's 0.6e-12 .. 1.0e-12; the three kernel forms measured 3.6e-12 .. 3.9e-12 there, 1.2 .. 1.5 times the bar,
    and 0.3e-12 .. 0.9e-12 with the sums in double."""
    inp = GC.take(GC.inputs(GC.B_REG), (0,))
    g64 = GC.grads("cool", "target_pos")["f64"][:1]
    dev = {}
    for fast in (False, True):
        for fs in (False, True):
            g = GC.oracle_grad("cool", "target_pos", inp, torch.float32, fast=fast, float_sums=fs)
            dev[fast, fs] = float((g.double() - g64).abs().max())
    print(f"\n[guide host] cool target_pos B=1, max|g32 - g64|: torch sums {dev[False, False]:.3g} / {dev[True, False]:.3g} (MFMA gate forms), "
          f"float sums {dev[False, True]:.3g} / {dev[True, True]:.3g}; max|g64| {float(g64.abs().max()):.3g}")
    assert dev[False, True] >= 2 * dev[False, False] and dev[True, True] >= 2 * dev[True, False]
    # with the switch off the decoder plugged in is the oracle's own
    assert torch.equal(GC.oracle_grad("cool", "target_pos", inp, torch.float32), GC.grads("cool", "target_pos", GC.B_REG, (0,))["f32"])
