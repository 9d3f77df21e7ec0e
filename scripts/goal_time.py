"""Time of the goal term (csrc/goal_kernels.hip) at 2,048 rows: the kernel alone (value + gradient, one cld_goal_loss call), a
goal-guided sample_step, and the agent_collision-guided sample_step of the same build -- the nearest existing step that also pays the
extra decode.  HIP events around every call, median of 20 after a warm-up.
    python3 scripts/goal_time.py [scenes] [agents_per_scene]"""
import ctypes as C
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from cld_amd import synth
from cld_amd.engine import Engine

S = int(sys.argv[1]) if len(sys.argv) > 1 else 32
A = int(sys.argv[2]) if len(sys.argv) > 2 else 64
B = S * A
e = Engine(100, "cuda:0"); e.load_state_dict(synth.make_unet_weights(0)); e.load_state_dict(synth.make_decoder_weights(0)); e.finalize()
inp = synth.make_inputs(B, 1)
cond, cs = torch.from_numpy(inp["cond_feat"]).cuda(), torch.from_numpy(inp["curr_states"]).cuda()
sc = synth.make_collision_scene([A] * S, 3, spacing=3.0)
sc["curr_speed"] = inp["curr_states"][:, 2].copy()
col = {k: (torch.as_tensor(v).cuda() if isinstance(v, np.ndarray) else v) for k, v in
       dict(extent=sc["extent"], world_from_agent=sc["world_from_agent"], curr_speed=sc["curr_speed"], scene_index=sc["scene_index"], weight=50.0).items()}
W = torch.from_numpy(sc["world_from_agent"]).double()
# a quarter of the agents on each of: the softmin form, the progress form, a target time inside the plan, one beyond it
kind = torch.tensor([1, 1, 2, 2] * (B // 4), dtype=torch.int32)
local = torch.tensor([[3.0, 2.5], [0.5, 12.0], [12.0, 2.0], [150.0, 5.0]] * (B // 4), dtype=torch.float64)
goal = dict(kind=kind.cuda(), target_time=torch.tensor([0, 0, 30, 90] * (B // 4), dtype=torch.int32).cuda(), urgency=torch.full((B,), 0.5).cuda(),
            pref_speed=torch.full((B,), 1.42).cuda(), scale=torch.full((B,), 1.0 / B).cuda(),
            target_pos=(torch.einsum("aij,aj->ai", W[:, :2, :2], local) + W[:, :2, 2]).float().cuda(),
            agent_from_world=torch.linalg.inv(W).float().cuda(), global_t=0)
x_t = torch.randn(B, 52, 4, device="cuda") * 0.7
z = torch.randn(B, 52, 4, device="cuda")
traj = e.decode(x_t * 0.7, cond, cs, descaled_output=True)


def timed(fn, n=20, warm=5):
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


cg, keep = e._goal(goal, B)
loss, grad = torch.empty(B, device="cuda"), torch.empty(B, 52, 6, device="cuda")
p = lambda t: C.c_void_p(t.data_ptr())
kern = lambda: e._check(e.lib.cld_goal_loss(e._h, p(traj), C.byref(cg), None, p(loss), p(grad), B, e._stream()), "cld_goal_loss")
print(f"{S} scenes x {A} agents = {B} rows; median of 20, HIP events")
print(f"  goal kernel (value + gradient, one cld_goal_loss call): {timed(kern):.1f} us   (value sum {float(loss.sum()):.1f}, max|grad| {float(grad.abs().max()):.3e})")
print(f"  decode of the same rows (cld_decode): {timed(lambda: e.decode(x_t, cond, cs, descaled_output=True)):.1f} us")
base = dict(curr_states=cs, lr=0.3, optimizer="adam")
t_goal = timed(lambda: e.sample_step(x_t, cond, 40, z=z, guidance=dict(base, goal=goal)))
t_col = timed(lambda: e.sample_step(x_t, cond, 40, z=z, guidance=dict(base, agent_collision=col)))
t_both = timed(lambda: e.sample_step(x_t, cond, 40, z=z, guidance=dict(base, goal=goal, agent_collision=col)))
t_plain = timed(lambda: e.sample_step(x_t, cond, 40, z=z))
print(f"  sample_step at t = 40 (incl. the Python wrapper): goal-guided {t_goal:.1f} us; agent_collision-guided {t_col:.1f} us; both {t_both:.1f} us; unguided {t_plain:.1f} us")
