"""Yardstick of the LSTM-VAE training path (tests/test_vae_train_host.py, tests/test_gpu_vae_train.py): a restatement of the reference's
LSTMVAE (models/vae/lstm_vae.py) and VaeModel.compute_vae_loss (models/vae/vae_model.py:89-99) in torch, so that autograd gives its
gradients in float64 (the yardstick) or float32 (the bar's calibration) on the CPU.

It adds to oracle.traj2z / oracle.lstm_decode what training mode has: nn.LSTM(num_layers=2, dropout=p) drops layer 0's output where it
enters layer 1, scaled by 1 / (1 - p); the recurrence and the top layer's output are not dropped.  A mask [B,52,64] of 0 and 1 / (1 - p)
stands for one draw; None is eval mode.
"""
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

from cld_amd import synth

T, H = 52, 64


def weights(seed: int = 0) -> "OrderedDict[str, np.ndarray]":
    """LSTMVAE's 26 tensors in state_dict order (lstm_enc.*, lstm_dec.*, mu.*, logvar.*) from synth's generators."""
    enc, dec = synth.make_encoder_weights(seed), synth.make_decoder_weights(seed)
    out = OrderedDict((k, v) for k, v in enc.items() if k.startswith("lstm_enc."))
    out.update(dec)
    out.update((k, v) for k, v in enc.items() if not k.startswith("lstm_enc."))
    return out


def mask(seed: int, name: str, B: int, p: float = 0.2) -> np.ndarray:
    """One dropout draw [B,52,64]: 0 with probability p, else 1 / (1 - p)."""
    keep = synth.uniform(seed, name, (B, T, H), 0.0, 1.0) >= p
    return (keep / (1.0 - p)).astype(np.float32)


def lstm2(w, pre, x, cond, m=None):
    """The two-layer LSTM of lstm_vae.py:20-26 / 44-49 (h0 = cond2hidden(cond) for both layers, c0 = 0, gate rows i, f, g, o), with
    the dropout mask m on layer 1's input -> the top layer's h [B,52,64]."""
    h0 = F.linear(cond, w[pre + ".cond2hidden.weight"], w[pre + ".cond2hidden.bias"])
    h, c = [h0, h0], [torch.zeros_like(h0), torch.zeros_like(h0)]
    out = []
    for t in range(x.shape[1]):
        inp = x[:, t]
        for l in range(2):
            if l == 1 and m is not None:
                inp = inp * m[:, t]
            g = (F.linear(inp, w[f"{pre}.lstm.weight_ih_l{l}"], w[f"{pre}.lstm.bias_ih_l{l}"])
                 + F.linear(h[l], w[f"{pre}.lstm.weight_hh_l{l}"], w[f"{pre}.lstm.bias_hh_l{l}"]))
            gi, gf, gg, go = g.chunk(4, dim=1)
            c[l] = torch.sigmoid(gf) * c[l] + torch.sigmoid(gi) * torch.tanh(gg)
            h[l] = torch.sigmoid(go) * torch.tanh(c[l])
            inp = h[l]
        out.append(inp)
    return torch.stack(out, dim=1)


def encode(w, x6, cond, m=None):
    """lstm_vae.py:87-93 without the draw -> (mu, logvar) [B,52,4]."""
    y = lstm2(w, "lstm_enc", x6, cond, m)
    return F.linear(y, w["mu.weight"], w["mu.bias"]), F.linear(y, w["logvar.weight"], w["logvar.bias"])


def decode(w, z, cond, m=None):
    """lstm_vae.py:44-52 -> act [B,52,2]."""
    return F.linear(lstm2(w, "lstm_dec", z, cond, m), w["lstm_dec.hid2act.weight"], w["lstm_dec.hid2act.bias"])


def vae_loss(x6, act, mu, logvar, beta):
    """vae_model.py:89-99 -> (loss, recon, kld)."""
    recon = F.mse_loss(x6[..., 4:6], act)
    B, T_, _ = mu.shape
    kld = -0.5 * torch.sum(1 + logvar - mu.pow(2) - logvar.exp()) / (B * T_)
    return recon + beta * kld, recon, kld


def step_loss(w, x6, cond, noise, beta, masks=(None, None)):
    """One training step's loss (vae_model.py:65-70): encode, reparametrise (lstm_vae.py:95-99), decode, compute_vae_loss."""
    mu, lv = encode(w, x6, cond, masks[0])
    act = decode(w, mu + noise * torch.exp(0.5 * lv), cond, masks[1])
    return vae_loss(x6, act, mu, lv, beta)
