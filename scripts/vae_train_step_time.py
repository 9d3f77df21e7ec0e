"""Time one LSTM-VAE training step (vae_model.py:65-99 without the ContextEncoder: encoder forward, reparametrisation, decoder forward,
compute_vae_loss, then their backward; Adam excluded) on the HIP training path (cld_amd.train.TrainableVae) and on torch-ROCm fp32
autograd of the same architecture built from torch.nn.LSTM (the MIOpen RNN path), with the same weights, masks and noise.  HIP events,
a warm-up first.  Prints one JSON line per batch size.

    python scripts/vae_train_step_time.py [--sizes 128 2048] [--iters 20]

The torch side runs each 2-layer stack as two single-layer nn.LSTM calls with the dropout mask multiplied in between: that is what
nn.LSTM(num_layers=2, dropout=p) computes in train mode, with the draw made explicit so that both sides use the same mask.
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from cld_amd import _lib  # noqa: E402
from cld_amd.train import TrainableVae  # noqa: E402
import vae_yardstick as Y  # noqa: E402


class TorchStack(torch.nn.Module):
    """Two single-layer nn.LSTMs with the reference weights; layer 1 reads mask * layer 0's output."""

    def __init__(self, w, pre, d_in):
        super().__init__()
        self.l0 = torch.nn.LSTM(d_in, 64, 1, batch_first=True)
        self.l1 = torch.nn.LSTM(64, 64, 1, batch_first=True)
        self.c2h = torch.nn.Linear(256, 64)
        with torch.no_grad():
            for l, m in ((0, self.l0), (1, self.l1)):
                for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
                    getattr(m, n + "_l0").copy_(torch.from_numpy(w[f"{pre}.lstm.{n}_l{l}"]))
            self.c2h.weight.copy_(torch.from_numpy(w[pre + ".cond2hidden.weight"]))
            self.c2h.bias.copy_(torch.from_numpy(w[pre + ".cond2hidden.bias"]))

    def forward(self, x, cond, mask):
        h0 = self.c2h(cond).unsqueeze(0)
        c0 = torch.zeros_like(h0)
        y0, _ = self.l0(x, (h0, c0))
        y1, _ = self.l1(y0 * mask, (h0, c0))
        return y1


class TorchVae(torch.nn.Module):
    def __init__(self, w):
        super().__init__()
        self.enc = TorchStack(w, "lstm_enc", 6)
        self.dec = TorchStack(w, "lstm_dec", 4)
        self.mu, self.lv, self.h2a = torch.nn.Linear(64, 4), torch.nn.Linear(64, 4), torch.nn.Linear(64, 2)
        with torch.no_grad():
            for lin, n in ((self.mu, "mu"), (self.lv, "logvar"), (self.h2a, "lstm_dec.hid2act")):
                lin.weight.copy_(torch.from_numpy(w[n + ".weight"]))
                lin.bias.copy_(torch.from_numpy(w[n + ".bias"]))

    def step_loss(self, x6, cond, noise, masks, beta):
        y = self.enc(x6, cond, masks[0])
        mu, lv = self.mu(y), self.lv(y)
        act = self.h2a(self.dec(mu + noise * torch.exp(0.5 * lv), cond, masks[1]))
        recon = F.mse_loss(x6[..., 4:6], act)
        kld = -0.5 * torch.sum(1 + lv - mu.pow(2) - lv.exp()) / (mu.shape[0] * mu.shape[1])
        return recon + beta * kld


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 2048])
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    w = Y.weights(0)
    tv = TrainableVae(w, device="cuda:0")
    tm = TorchVae(w).cuda()
    tape_row = int(_lib.load().cld_vae_tape_bytes(None, 0, 1))
    beta = 0.3
    for B in a.sizes:
        g = torch.Generator(device="cuda")
        g.manual_seed(B)
        x6 = torch.randn(B, 52, 6, device="cuda", generator=g)
        cond = torch.randn(B, 256, device="cuda", generator=g)
        noise = torch.randn(B, 52, 4, device="cuda", generator=g)
        masks = tuple((torch.rand(B, 52, 64, device="cuda", generator=g) >= 0.2).float() / 0.8 for _ in range(2))

        def hip_step():
            tv.zero_grad()
            act, mu, lv = tv(x6, cond, noise=noise, masks=masks)
            tv.compute_vae_loss(x6, act, mu, lv, beta)[0].backward()

        def torch_step():
            tm.zero_grad(set_to_none=True)
            tm.step_loss(x6, cond, noise, masks, beta).backward()

        out = {"B": B}
        hip_step()
        torch_step()
        torch.cuda.synchronize()
        gh = dict(tv.named_parameters())["lstm_enc.lstm.weight_hh_l0"].grad
        gt = tm.enc.l0.weight_hh_l0.grad
        out["enc_weight_hh_l0_grad_rel_diff"] = float((gh - gt).abs().max() / gt.abs().max())
        for name, fn in (("hip", hip_step), ("torch", torch_step)):
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out[f"{name}_ms"] = round(e0.elapsed_time(e1) / a.iters, 3)
        out["speedup_vs_torch"] = round(out["torch_ms"] / out["hip_ms"], 3)
        out["tape_bytes_per_row"] = tape_row
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
