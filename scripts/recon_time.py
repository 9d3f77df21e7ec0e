"""Time of reconstruction guidance (include/cld_recon.h) at 2,048 agents with classifier-free guidance (w = 2), target_speed +
agent_collision: one reconstruction-guided step, the mean-guided step (guide_clean=True) of the same build with the same terms as the
comparator, a bare cld_unet_train_forward + cld_unet_backward (dx only) pair on the step's 4,096 rows, and whole 100-step sample calls
of both modes.  HIP events around every call, median of 20 after a warm-up (whole samples: median of 3).
    python3 scripts/recon_time.py [scenes] [agents_per_scene]
    python3 scripts/recon_time.py --trace       20 reconstruction-guided steps and nothing else: the run to put under
                                                rocprofv3 --kernel-trace --stats for the kernels' shares of a step (recon_*_kernel: the
                                                three new kernels; pack_kernel: the weight repack of the two training walks)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from cld_amd import synth
from cld_amd.engine import Engine

trace = "--trace" in sys.argv
argv = [a for a in sys.argv[1:] if not a.startswith("--")]
S = int(argv[0]) if len(argv) > 0 else 32
A = int(argv[1]) if len(argv) > 1 else 64
B, GW, T_STEP = S * A, 2.0, 40
wu = synth.make_unet_weights(0)
e = Engine(100, "cuda:0"); e.load_state_dict(wu); e.load_state_dict(synth.make_decoder_weights(0)); e.finalize()
params = e.unet_flat_params(wu)
inp = synth.make_inputs(B, 1)
cond, cs = torch.from_numpy(inp["cond_feat"]).cuda(), torch.from_numpy(inp["curr_states"]).cuda()
non_cond = torch.from_numpy(synth.make_inputs(B, 1001)["cond_feat"]).cuda()
sc = synth.make_collision_scene([A] * S, 3, spacing=3.0)
sc["curr_speed"] = inp["curr_states"][:, 2].copy()
col = {k: (torch.as_tensor(v).cuda() if isinstance(v, np.ndarray) else v) for k, v in
       dict(extent=sc["extent"], world_from_agent=sc["world_from_agent"], curr_speed=sc["curr_speed"], scene_index=sc["scene_index"], weight=50.0).items()}
tgt = torch.from_numpy(synth.uniform(1, "tgt", (B, 52), 0.0, 12.0)).cuda()
terms = dict(curr_states=cs, target_speed=tgt, agent_collision=col)
recon = dict(terms, reconstruction=dict(params=params, lr=None, perturb_th=None, descend=True))
mean_guided = dict(terms, lr=0.3, optimizer="adam", guide_clean=True)
x_t = torch.randn(B, 52, 4, device="cuda") * 0.7
z = torch.randn(B, 52, 4, device="cuda")
cfg = dict(non_cond=non_cond, guidance_w=GW)
step_recon = lambda: e.recon_step(x_t, cond, T_STEP, recon, z=z, **cfg)

if trace:
    for _ in range(20):
        step_recon()
    torch.cuda.synchronize()
    sys.exit(0)


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


lib = e.lib
tape_row = int(lib.cld_unet_tape_bytes(e._h, 1))
print(f"{S} scenes x {A} agents = {B} agents, CFG w = {GW} ({2 * B} U-Net rows per step), target_speed + agent_collision; median of 20, HIP events")
print(f"  tape: {tape_row} bytes per U-Net row = {2 * tape_row} bytes per agent with CFG ({2 * B * tape_row / 2 ** 30:.2f} GiB at this size); "
      f"workspace of the calls {int(lib.cld_recon_workspace_bytes(e._h, B, 1)) / 2 ** 30:.2f} GiB; second copy of the weights {params.numel() * 4 / 2 ** 20:.1f} MiB")
t_recon = timed(step_recon)
t_mean = timed(lambda: e.sample_step(x_t, cond, T_STEP, z=z, guidance=mean_guided, **cfg))
t_plain = timed(lambda: e.sample_step(x_t, cond, T_STEP, z=z, **cfg))
x2, c2 = torch.cat([x_t, x_t]), torch.cat([cond, non_cond])
tt = torch.full((2 * B,), T_STEP, dtype=torch.long)
d_eps = torch.randn(2 * B, 52, 4, device="cuda")


def pair():
    eps, tape = e.unet_train_forward(params, x2, c2, tt)
    e.unet_backward(params, x2, c2, tt, tape, d_eps, d_params=None, want_dx=True)


t_fwd = timed(lambda: e.unet_train_forward(params, x2, c2, tt))
t_pair = timed(pair)
print(f"  one step at t = {T_STEP} (incl. the Python wrapper): reconstruction-guided {t_recon:.0f} us; mean-guided (guide_clean=True) {t_mean:.0f} us; "
      f"unguided CFG step {t_plain:.0f} us; ratio reconstruction / mean-guided {t_recon / t_mean:.2f}")
print(f"  bare cld_unet_train_forward on {2 * B} rows {t_fwd:.0f} us; forward + cld_unet_backward(dx only) {t_pair:.0f} us "
      f"({100 * t_pair / t_recon:.0f} % of the reconstruction-guided step)")
x_T = torch.randn(B, 52, 4, device="cuda")
w_recon = timed(lambda: e.sample(x_T, cond, noise=None, seed=1, guidance=recon, **cfg), n=3, warm=1)
w_mean = timed(lambda: e.sample(x_T, cond, noise=None, seed=1, guidance=mean_guided, **cfg), n=3, warm=1)
print(f"  whole 100-step sample call: reconstruction-guided {w_recon / 1e3:.1f} ms; mean-guided {w_mean / 1e3:.1f} ms")
