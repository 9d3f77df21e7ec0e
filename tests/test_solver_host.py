"""CPU tests of the few-step samplers' yardstick and cases (tests/solver_yardstick.py, tests/solver_cases.py): what tests/test_gpu_solver.py
relies on, shown without a GPU.  The reference has no few-step sampler; what pins the mode is the float64 restatement and two anchors that
do not depend on it:

  * DDIM with eta = 1 on the full consecutive sequence is the reference's ancestral chain: coefficient by coefficient against
    oracle.schedule's float32 tables, chain against oracle.sample in float64, and against the reference's recorded 10-step chain;
  * on data ~ N(0, s^2), where the noise prediction and the probability flow are known in closed form, DDIM converges with order one and
    DPM-Solver++(2M) with order two.

Measured here (float64 unless said): table identities -- x_t_cof 1.0e-7, noise_cof 2.9e-5, sigma 6.9e-6 relative (the float32 tables'
rounding; noise_cof carries the cancellation of alphas - alphas_cumprod * alphas); the 100-step eta = 1 chain against oracle.sample
1.25e-7 of max|x0| = 9.3e3; order anchor DDIM 4.4e-2 / 2.2e-2 / 1.1e-2 (ratios 1.98, 1.99), 2M 1.0e-2 / 2.9e-3 / 7.6e-4 (3.55, 3.76).
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from cld_amd import _lib, synth
from cld_amd import dm_model as DM
from cld_amd import engine as EN
from oracle import cld_oracle as O
from tests import grad_bar
from tests import solver_cases as SC
from tests import solver_yardstick as Y

F64, F32 = torch.float64, torch.float32


# ------------------------------------------------------------------------------------------------------------- 1. table identities
@pytest.mark.parametrize("n,ts", [(100, SC.STEP_LISTS["low"]), (100, SC.STEP_LISTS["top"]), (100, tuple(range(99, -1, -1))), (10, (9, 4, 0)), (100, (50,))])
@pytest.mark.parametrize("eta", [0.0, 0.5, 1.0])
def test_ddim_x_eps_form_equals_the_x0_form(n, ts, eta):
    """A x + B eps == sqrt(acp_p) x0_hat + sqrt(1 - acp_p - var) eps_hat, eps_hat = (x - sqrt(acp_s) x0_hat) / sqrt(1 - acp_s), to 1e-12
    of the result's scale; the last step is x0_hat."""
    t = Y.tables(n, "ddim", ts, eta)
    g = torch.Generator().manual_seed(3)
    x, eps = torch.randn(3, 52, 4, dtype=F64, generator=g), torch.randn(3, 52, 4, dtype=F64, generator=g)
    a_s, _ = Y._pairs(n, ts)
    for k in range(len(ts)):
        x0 = t["rc"][k] * x - t["rm1"][k] * eps
        eps_hat = (x - torch.sqrt(a_s[k]) * x0) / torch.sqrt(1.0 - a_s[k])
        one = t["a"][k] * x + t["b"][k] * eps
        two = t["b_x0"][k] * x0 + t["dir"][k] * eps_hat
        # the x0 form goes through x0_hat = rc (x - ...): its own rounding is 1e-16 rc, so the identity is held relative to rc's scale
        assert float((one - two).abs().max()) <= 1e-12 * max(1.0, float(t["rc"][k])) * float(x.abs().max()), (k, ts[k])
        assert float((eps_hat - eps).abs().max()) <= 1e-12 * float(t["rc"][k])
    k = len(ts) - 1
    assert float(t["sigma"][k]) == 0.0
    assert abs(float(t["a"][k] - t["rc"][k])) <= 1e-12 * float(t["rc"][k]) and abs(float(t["b"][k] + t["rm1"][k])) <= 1e-12 * float(t["rc"][k])


def test_2m_single_step_and_last_step_are_the_clean_prediction():
    for ts in ((50,), SC.STEP_LISTS["low"], SC.STEP_LISTS["top"], (9, 4, 0)):
        n = 10 if ts[0] < 10 else 100
        t = Y.tables(n, "dpmpp_2m", ts)
        k = len(ts) - 1
        assert float(t["a"][k]) == 0.0 and float(t["b"][k]) == 1.0 and float(t["c0"][k]) == 1.0 and float(t["c1"][k]) == 0.0
        x, eps = torch.randn(2, 52, 4, dtype=F64), torch.randn(2, 52, 4, dtype=F64)
        u = Y.update(t, "dpmpp_2m", k, len(ts), x, eps, torch.randn(2, 52, 4, dtype=F64), None)
        assert torch.equal(u["x_next"], u["x0_hat"]) and torch.equal(u["mu"], u["x0_hat"])
        assert float(t["c1"][0]) == 0.0 and all(float(t["c1"][j]) > 0 for j in range(1, k))
    # 2M's first-order step is DDIM(0)'s, two ways of writing one update
    d, m = Y.tables(100, "ddim", SC.STEP_LISTS["low"]), Y.tables(100, "dpmpp_2m", SC.STEP_LISTS["low"])
    x, eps = torch.randn(2, 52, 4, dtype=F64), torch.randn(2, 52, 4, dtype=F64)
    a, b = Y.update(d, "ddim", 0, 6, x, eps, None, None)["mu"], Y.update(m, "dpmpp_2m", 0, 6, x, eps, None, None)["mu"]
    assert float((a - b).abs().max()) <= 1e-10 * float(a.abs().max())


# measured relative deviations of the eta = 1 coefficients from oracle.schedule's float32 tables (n = 100; see the module docstring)
ETA1_MEASURED = {"x_t_cof": 1.03e-7, "noise_cof": 2.88e-5, "sigma": 6.95e-6}


@pytest.mark.parametrize("n", [100, 10])
def test_eta_one_on_the_full_sequence_has_the_ancestral_coefficients(n):
    """A_k, -B_k, sigma_k, sigma^g_k against x_t_cof, noise_cof, exp(plvc / 2): those tables are float32 in the reference's operation
    order, so the agreement is to their rounding -- asserted at 4 x the measured value."""
    ts = list(range(n - 1, -1, -1))
    t = Y.tables(n, "ddim", ts, 1.0)
    s = O.schedule(n)
    idx = torch.tensor(ts)
    sig = (0.5 * s["posterior_log_variance_clipped"][idx]).exp().double()
    rel = lambda a, b: float(((a - b.double()).abs() / b.double().abs()).max())
    got = {"x_t_cof": rel(t["a"], s["x_t_cof"][idx]), "noise_cof": rel(-t["b"], s["noise_cof"][idx]),
           "sigma": max(rel(t["sigma_g"], sig), rel(t["sigma"][:-1], sig[:-1]))}
    print(f"\n[solver host] eta = 1 coefficients vs the float32 tables, n = {n}: " + ", ".join(f"{k} {v:.3g}" for k, v in got.items()))
    for k, v in got.items():
        assert v <= 4 * ETA1_MEASURED[k], (k, v)
    assert float(t["sigma"][-1]) == 0.0 and abs(float(t["sigma_g"][-1]) - 1e-10) <= 1e-22


# ------------------------------------------------------------------------------------------------------------- 2. the eta = 1 anchor
def test_eta_one_chain_is_the_ancestral_chain_in_float64():
    torch.set_num_threads(8)
    n, B = 100, 4
    wn = SC.unet_weights()
    nz = synth.make_noise(B, n, 17)
    x_T, noise = torch.from_numpy(nz["x_T"]), torch.from_numpy(nz["noise"])
    cond = torch.from_numpy(synth.make_inputs(B, 17)["cond_feat"])
    ref = O.sample(O.to_torch(wn, F64), {k: v.double() for k, v in O.schedule(n).items()}, x_T.double(), noise.double(), cond.double())["pred_traj"]
    got, _ = Y.chain(wn, None, n, "ddim", list(range(n - 1, -1, -1)), 1.0, x_T, noise, cond, dtype=F64)
    rel = float((got - ref).abs().max()) / float(ref.abs().max())
    print(f"\n[solver host] eta = 1, 100 steps, float64: max|d| / max|x0| = {rel:.3g} (max|x0| = {float(ref.abs().max()):.3g})")
    # the coefficient deviations above (up to 2.9e-5 on noise_cof at single steps) enter a chain whose x0 is 9.3e3: measured 1.25e-7
    assert rel <= 4 * 1.2e-7


def test_eta_one_chain_meets_the_reference_recording(golden):
    """n_timesteps = 10: the float64 DDIM chain against the reference's recorded ancestral chain, bar calibrated by the float32 chain."""
    torch.set_num_threads(8)
    meta, g = golden("sample_n10_jitter")
    n, B = 10, meta["B"]
    wn = synth.make_unet_weights(0, affine_jitter=True)
    nz = synth.make_noise(B, n, meta["noise_seed"])
    x_T, noise = torch.from_numpy(nz["x_T"]), torch.from_numpy(nz["noise"])
    cond = torch.from_numpy(synth.make_inputs(B, meta["in_seed"])["cond_feat"])
    ts = list(range(n - 1, -1, -1))
    y64, _ = Y.chain(wn, None, n, "ddim", ts, 1.0, x_T, noise, cond, dtype=F64)
    y32, _ = Y.chain(wn, None, n, "ddim", ts, 1.0, x_T, noise, cond, dtype=F32)
    r = grad_bar.ratio(torch.from_numpy(g["pred_traj"]), y64, y32)
    print(f"\n[solver host] eta = 1, n = 10: the recording against the float64 chain, ratio to the bar {r:.3g}")
    assert r <= 1.0


# ------------------------------------------------------------------------------------------------------------- 3. order of accuracy
def test_order_of_accuracy_on_the_gaussian_problem():
    n, s2 = 100, 9.0
    x = torch.tensor([1.0, -2.0, 0.5], dtype=F64)
    exact = Y.gaussian_flow(n, s2, x, 90, 10)
    err = {}
    for kind in Y.KINDS:
        err[kind] = [float(((Y.integrate(n, kind, list(range(90, 9, -stride)), Y.gaussian_eps(n, s2), x) - exact).abs() / exact.abs()).max())
                     for stride in (4, 2, 1)]
    d, m = err["ddim"], err["dpmpp_2m"]
    print(f"\n[solver host] relative error at strides 4, 2, 1: DDIM {d[0]:.3g} {d[1]:.3g} {d[2]:.3g} (ratios {d[0] / d[1]:.3g}, {d[1] / d[2]:.3g}); "
          f"2M {m[0]:.3g} {m[1]:.3g} {m[2]:.3g} (ratios {m[0] / m[1]:.3g}, {m[1] / m[2]:.3g})")
    assert 1.8 <= d[0] / d[1] <= 2.2 and 1.8 <= d[1] / d[2] <= 2.2
    assert m[0] / m[1] >= 3.0 and m[1] / m[2] >= 3.0
    assert m[1] < 0.25 * d[1]


# ------------------------------------------------------------------------------------------------------------- 4. the kinds are told apart
@pytest.mark.parametrize("cfg", [False, True], ids=["plain", "cfg"])
def test_the_yardstick_tells_the_kinds_apart(cfg):
    """On every 2M step case of tests/test_gpu_solver.py that reads history (the x0_prev of a real preceding step) the 2M and the DDIM(0)
    update of the same (x_t, eps) differ by at least 100 x the bar the GPU is held to."""
    for lst, k in SC.HISTORY_STEPS:
        m64, m32 = SC.step_reference("dpmpp_2m", 0.0, lst, cfg, k, "f64"), SC.step_reference("dpmpp_2m", 0.0, lst, cfg, k, "f32")
        d64 = SC.step_reference("ddim", 0.0, lst, cfg, k, "f64")
        bar = SC.bar(m64["x_next"], m32["x_next"])
        diff = float((m64["x_next"] - d64["x_next"]).abs().max())
        ts = SC.STEP_LISTS[lst]
        print(f"\n[solver host] cfg={cfg} {lst} k={k} ({ts[k]} -> {ts[k + 1]}): |x'_2M - x'_DDIM| = {diff:.3g}, bar {bar:.3g}, ratio {diff / bar:.3g}")
        assert diff >= 100 * bar, (lst, k, diff, bar)


def test_whole_chains_differ_by_far_more_than_float32():
    a64, a32, b64 = SC.free_chain("ddim", "f64"), SC.free_chain("ddim", "f32"), SC.free_chain("dpmpp_2m", "f64")
    scale = float(a64.abs().max())
    apart, f32err = float((a64 - b64).abs().max()) / scale, float((a32.double() - a64).abs().max()) / scale
    print(f"\n[solver host] K = 10 chains: kinds apart {apart:.3g}, float32 error {f32err:.3g} (relative to max|x0| = {scale:.3g})")
    assert apart >= 10 * f32err


# ------------------------------------------------------------------------------------------------------------- 5. the guided cases
@pytest.mark.parametrize("name", list(SC.GUIDED))
def test_guided_cases_clip_some_and_few_sit_on_the_threshold(name):
    B, loss, cfg = SC.GUIDED[name]
    for kind, eta in SC.GUIDE_VARIANTS:
        r64, r32 = (SC.guided_reference(name, kind, eta, "sgd", 0, d) for d in ("f64", "f32"))
        assert r64["th"] == r64["sigma_g"] and r64["lr_eff"] == SC.SGD_LR[(name, kind)]
        amb, d64 = SC.clip_ambiguous(r64, r32)
        clipped = float((d64.abs() > r64["th"]).double().mean())
        share = float(amb.double().mean())
        print(f"\n[solver host] {name} {kind}: {100 * clipped:.1f} % clipped, {100 * share:.2f} % within the bar of the threshold")
        assert 0.1 <= clipped <= 0.9 and share <= 0.02
        # the clip as oracle.guidance_step applies it is the clamp of that delta
        want = r64["mu"] + d64.clamp(-r64["th"], r64["th"])
        assert float((r64["mu_guided"] - want).abs().max()) <= 1e-12 * float(want.abs().max())
        # Adam as the reference's perturb() runs it: lr = sigma^g, no clip, every step +-lr or 0
        a64 = SC.guided_reference(name, kind, eta, "adam", 0, "f64")
        assert a64["th"] is None and a64["lr_eff"] == a64["sigma_g"]
        assert float((a64["mu_guided"] - a64["mu"]).abs().max()) <= a64["sigma_g"] * (1 + 1e-12)
        # the output step: its own settings, sigma^g = 1e-10 there, no noise
        o64 = SC.guided_reference(name, kind, eta, "sgd", 2, "f64")
        assert o64["sigma"] == 0.0 and abs(o64["sigma_g"] - 1e-10) < 1e-20 and o64["lr_eff"] == SC.OUT_SGD_LR and o64["th"] is None
        assert torch.equal(o64["x_next"], o64["mu_guided"]) and float((o64["mu_guided"] - o64["mu"]).abs().max()) > 0


@pytest.mark.parametrize("name", [n for n, v in SC.GUIDED.items() if v[1] == "target_speed"])
def test_kink_margins_hold_on_the_guided_iterate(name):
    """No agent's speed chain on decode(mu) comes within 8 x the float32 yardstick's speed deviation of a kink of the loss or a clip of
    the roll-out (oracle.speed_kink_margin), at the intermediate and at the output step."""
    inp = SC.guided_inputs(name)
    wd = O.to_torch(SC.decoder_weights(), F64)
    tgt = torch.nan_to_num(inp["yard"]["target_speed"].double(), nan=1e6)          # a NaN target is no target: no kink there
    for kind, eta in SC.GUIDE_VARIANTS:
        for k in (0, 2):
            r64, r32 = (SC.guided_reference(name, kind, eta, "adam", k, d) for d in ("f64", "f32"))
            m = O.speed_kink_margin(wd, r64["mu"], inp["cond"].double(), inp["curr_states"].double(), tgt)
            v64 = O.decode(wd, r64["mu"], inp["cond"].double(), inp["curr_states"].double(), True)[..., 2]
            v32 = O.decode(O.to_torch(SC.decoder_weights(), F32), r32["mu"], inp["cond"], inp["curr_states"], True)[..., 2]
            dev = float((v32.double() - v64).abs().max())
            live = inp["yard"]["loss_scale"] != 0
            print(f"\n[solver host] {name} {kind} k={k}: smallest kink margin {float(m[live].min()):.3e} m/s, float32 speed deviation {dev:.3e}")
            assert float(m[live].min()) >= 8 * dev, (name, kind, k)


# ------------------------------------------------------------------------------------------------------------- 6. the host surface
def test_solver_timesteps():
    assert DM.solver_timesteps(100, 10) == [99, 88, 77, 66, 55, 44, 33, 22, 11, 0]
    assert DM.solver_timesteps(100, 1) == [99] and DM.solver_timesteps(100, 2) == [99, 0]
    assert DM.solver_timesteps(10, 10) == list(range(9, -1, -1))
    assert DM.solver_timesteps(10, 50) == list(range(9, -1, -1))                    # the unique values: never more than n_timesteps
    for n, K in ((100, 20), (100, 50), (50, 7)):
        ts = DM.solver_timesteps(n, K)
        assert ts[0] == n - 1 and ts[-1] == 0 and all(a > b for a, b in zip(ts, ts[1:])) and len(ts) <= K
        assert ts == sorted(set(int(v) for v in np.rint(np.linspace(n - 1, 0, K))), reverse=True)
    with pytest.raises(_lib.CldError):
        DM.solver_timesteps(100, 0)


def test_refusals_of_the_python_layer():
    ok = EN.parse_sampler({"kind": "ddim", "steps": 10, "eta": 0.5}, 100)
    assert ok[0] == "ddim" and ok[1].dtype == np.int32 and ok[1].tolist() == DM.solver_timesteps(100, 10) and ok[2] == 0.5
    assert EN.parse_sampler({"kind": "dpmpp_2m", "timesteps": [50, 45, 0]}, 100)[1].tolist() == [50, 45, 0]
    for bad, what in (({"kind": "ddim", "timesteps": [50, 50, 0]}, "not strictly decreasing at index 1"),
                      ({"kind": "ddim", "timesteps": [10, 20]}, "not strictly decreasing"),
                      ({"kind": "ddim", "timesteps": [100, 0]}, r"out of range \[0, n_timesteps\) at index 0"),
                      ({"kind": "ddim", "timesteps": [5, -1]}, "out of range"),
                      ({"kind": "ddim", "timesteps": []}, "K >= 1"),
                      ({"kind": "ddim", "steps": 0}, "K >= 1"),
                      ({"kind": "ddim", "steps": 10, "eta": 1.5}, r"eta outside \[0, 1\]"),
                      ({"kind": "ddim", "steps": 10, "eta": -0.1}, "eta outside"),
                      ({"kind": "dpmpp_2m", "steps": 10, "eta": 0.5}, r"2M\) is deterministic: eta != 0"),
                      ({"kind": "euler", "steps": 10}, "unknown kind 'euler'"),
                      ({"kind": "ddim"}, "exactly one of"),
                      ({"kind": "ddim", "steps": 10, "timesteps": [9, 0]}, "exactly one of"),
                      ({"kind": "ddim", "steps": 10, "order": 2}, "unknown keys")):
        with pytest.raises(_lib.CldError, match=what):
            EN.parse_sampler(bad, 100)
    with pytest.raises(NotImplementedError, match="guide_clean=True"):
        EN.refuse_sampler_guidance({"guide_clean": True})
    with pytest.raises(NotImplementedError, match="video_diff"):
        EN.refuse_sampler_guidance({"reconstruction": {"params": None}})
    EN.refuse_sampler_guidance(None)
    EN.refuse_sampler_guidance({"target_speed": None})
    # the policy refuses the combination before it touches an engine
    from cld_amd.policy import CldPolicy
    pol = CldPolicy.__new__(CldPolicy)
    for gc in (True, "video_diff"):
        with pytest.raises(NotImplementedError, match="sampler= together with guide_clean"):
            pol.get_action({}, sampler={"kind": "ddim", "steps": 10}, guide_clean=gc)


def _header():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return root, open(os.path.join(root, "include", "cld_solver.h")).read()


def test_cld_solver_layout_matches_the_header():
    _, hdr = _header()
    body = re.search(r"typedef struct cld_solver \{(.*?)\} cld_solver;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [m.group(2) for m in re.finditer(r"([A-Za-z_0-9 ]+\*?)\s*\b([a-z_]+);", body)]
    assert fields == [n for n, _ in _lib.CldSolver._fields_] == ["kind", "n_steps", "timesteps", "eta"]
    assert [getattr(_lib.CldSolver, n).offset for n in fields] == [0, 4, 8, 16] and ctypes.sizeof(_lib.CldSolver) == 24
    assert _lib.CldSolver._fields_[2][1] is ctypes.c_void_p and _lib.CldSolver._fields_[3][1] is ctypes.c_float
    assert ctypes.sizeof(_lib.CldGuidance) == 144                                # cld_guidance keeps its size
    for name, v in _lib.SOLVER_KINDS.items():
        assert re.search(r"#define CLD_SOLVER_" + name.upper() + r"\s+" + str(v) + r"\b", hdr), name
    assert re.search(r"#define CLD_SOLVER_TABLE_COLS\s+" + str(len(_lib.SOLVER_TABLE_COLS)) + r"\b", hdr) and Y.COLS[:4] == _lib.SOLVER_TABLE_COLS[:4]


def test_solver_header_matches_its_signature_table_and_the_others_keep_their_size():
    """include/cld_solver.h <=> _lib.SOLVER_SIGNATURES <=> the library's exports, in the manner of tests/test_recon_host.py; include/cld.h
    and the lane / recon / eval tables hold none of the entry points and keep their counts; build.sh compiles the new file and knows
    its headers."""
    root, hdr = _header()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(cld_[a-z0-9_]+)\s*\(", code))
    assert declared == set(_lib.SOLVER_SIGNATURES) == {"cld_solver_workspace_bytes", "cld_solver_tables", "cld_sample_solver", "cld_solver_step",
                                                       "cld_debug_solver_grid_cap", "cld_debug_solver_kernel"}
    for name, (_, args) in _lib.SOLVER_SIGNATURES.items():
        proto = re.search(r"\b" + name + r"\s*\((.*?)\);", code, re.S).group(1)
        assert len(proto.split(",")) == len(args), name
    assert '#include "cld.h"' in code
    main_hdr = open(os.path.join(root, "include", "cld.h")).read()
    others = (_lib.SIGNATURES, _lib.LANE_SIGNATURES, _lib.RECON_SIGNATURES, _lib.EVAL_SIGNATURES)
    assert [len(t) for t in others] == [88, 3, 5, 3]
    assert not any(n in t for t in others for n in _lib.SOLVER_SIGNATURES) and not any(n in main_hdr for n in _lib.SOLVER_SIGNATURES)
    sh = open(os.path.join(root, "controllable-latent-diffusion-for-traffic-simulation_amd", "build.sh")).read()
    assert " solver_kernels " in sh and "csrc/solver_kernels.h -nt" in sh and "../include/cld_solver.h -nt" in sh
    if os.path.exists(_lib.LIB_PATH):                                            # where the library is built: it exports all six
        lib = _lib.load()
        for name, (res, args) in _lib.SOLVER_SIGNATURES.items():
            fn = getattr(lib, name)
            assert fn.restype is res and list(fn.argtypes) == args
        assert lib.cld_sample_solver.argtypes[1]._type_ is _lib.CldSolver and lib.cld_solver_step.argtypes[9]._type_ is _lib.CldGuidance
        assert lib.cld_debug_solver_grid_cap(3) == 3 and lib.cld_debug_solver_grid_cap(0) == 1024
