"""Time of the few-step samplers (include/cld_solver.h) at 2,048 agents with classifier-free guidance (w = 2) and target_speed guidance
(the shape of BASELINE configs[2]): one solver step against one ancestral step of the same build, and whole calls at K = 10, 20, 50
against the 100-step cld_sample_guided call of the same build.  HIP events around every call (the Python wrapper included), median of
20 after a warm-up.
    python3 scripts/solver_time.py [scenes] [agents_per_scene]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from cld_amd import synth
from cld_amd.engine import Engine

argv = [a for a in sys.argv[1:] if not a.startswith("--")]
S = int(argv[0]) if len(argv) > 0 else 32
A = int(argv[1]) if len(argv) > 1 else 64
B, GW, T_STEP = S * A, 2.0, 44
e = Engine(100, "cuda:0"); e.load_state_dict(synth.make_unet_weights(0)); e.load_state_dict(synth.make_decoder_weights(0)); e.finalize()
inp = synth.make_inputs(B, 1)
cond, cs = torch.from_numpy(inp["cond_feat"]).cuda(), torch.from_numpy(inp["curr_states"]).cuda()
non_cond = torch.from_numpy(synth.make_inputs(B, 1001)["cond_feat"]).cuda()
tgt = torch.from_numpy(synth.uniform(1, "tgt", (B, 52), 0.0, 12.0)).cuda()
guide = dict(curr_states=cs, target_speed=tgt, lr=0.3, optimizer="adam")
x_t = torch.randn(B, 52, 4, device="cuda") * 0.7
z = torch.randn(B, 52, 4, device="cuda")
x_T = torch.randn(B, 52, 4, device="cuda")
cfg = dict(non_cond=non_cond, guidance_w=GW)


def timed(fn, n=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return float(np.median(ts))


print(f"{S} scenes x {A} agents = {B} agents, CFG w = {GW} ({2 * B} U-Net rows per step), target_speed guidance; median of 20, HIP events")
ten = {"timesteps": [99, 88, 77, 66, 55, 44, 33, 22, 11, 0]}          # step k = 5 goes 44 -> 33
print(f"  one step at t = {T_STEP} (incl. the Python wrapper), guided / unguided:")
t_anc_g = timed(lambda: e.sample_step(x_t, cond, T_STEP, z=z, guidance=guide, **cfg))
t_anc = timed(lambda: e.sample_step(x_t, cond, T_STEP, z=z, **cfg))
print(f"    ancestral (cld_sample_step)           {t_anc_g:7.0f} us / {t_anc:7.0f} us")
for kind, eta in (("ddim", 0.0), ("ddim", 1.0), ("dpmpp_2m", 0.0)):
    smp = dict(ten, kind=kind, eta=eta)
    t_g = timed(lambda: e.solver_step(x_t, cond, smp, 5, x0_prev=x_t, z=z, guidance=guide, **cfg))
    t_u = timed(lambda: e.solver_step(x_t, cond, smp, 5, x0_prev=x_t, z=z, **cfg))
    print(f"    {kind:9s} eta = {eta:.0f} (cld_solver_step)   {t_g:7.0f} us / {t_u:7.0f} us   ({t_g / t_anc_g:.3f} x / {t_u / t_anc:.3f} x the ancestral step)")
print("  whole calls, guided (ms):")
w_anc = timed(lambda: e.sample(x_T, cond, noise=None, seed=1, guidance=guide, **cfg), n=20, warm=1)
print(f"    ancestral, 100 steps (cld_sample_guided)   {w_anc / 1e3:8.2f}")
for K in (10, 20, 50):
    row = []
    for kind, eta in (("ddim", 0.0), ("ddim", 1.0), ("dpmpp_2m", 0.0)):
        smp = {"kind": kind, "steps": K, "eta": eta}
        w = timed(lambda: e.sample_solver(x_T, cond, smp, noise=None, seed=1, guidance=guide, **cfg), n=20, warm=1)
        row.append(f"{kind} eta = {eta:.0f} {w / 1e3:7.2f} ({w_anc / w:5.2f} x faster)")
    print(f"    K = {K:2d}: " + ";  ".join(row))
