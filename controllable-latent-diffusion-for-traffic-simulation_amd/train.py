"""Training surface of the denoiser and of the LSTM-VAE: the U-Net's forward and backward on the HIP training path (include/cld.h,
cld_unet_train_forward / cld_unet_backward) and the VAE's encoder / decoder forward and backward (cld_vae_*_train / cld_vae_*_backward)
behind torch autograd.

The reference trains `self.dm.parameters()` with Adam in two loops (src/trainers/dm_trainer.py:72-80 on
`DmModel.compute_losses`, and src/trainers/guide_dm_trainer.py:127-183 `ppo_update` on `DmModel.log_prob` at t = 0).
`TrainableDm` keeps the U-Net weights in ONE flat fp32 device tensor, exposed as `nn.Parameter` views under the reference's
state_dict names, so `torch.optim.Adam(dm.parameters())` updates them in place and the next forward reads the new values with no
host round trip.  The small loss heads (q_sample, MSE, the Normal log-density) are torch elementwise code around the U-Net.
`TrainableVae` does the same for LSTMVAE (src/trainers/vae_trainer.py: Adam over the VAE's parameters on compute_vae_loss).
Exact fp32 only: a "f16x2" engine refuses these calls.
"""
from __future__ import annotations

import math
from typing import Mapping, Optional

import torch
import torch.nn.functional as F

from ._lib import CldError
from .dm_model import DmModel
from .engine import Engine, copy_into_flat, unet_param_table
from .vae_model import VaeModel


def _keep(ctx, engine: Engine, flat, table, tape, mask, *inputs):
    """What every forward below leaves for its backward: the engine, the flat buffer and the (name, offset, numel, shape) entries of
    `params`, the tape, the dropout mask (None: none) and the detached inputs."""
    ctx.engine, ctx.flat, ctx.table, ctx.tape, ctx.mask = engine, flat, table, tape, mask
    ctx.save_for_backward(*inputs)


def _backward(ctx, new_d_flat, engine_backward):
    """The tail the three backwards share.  `new_d_flat(flat)` allocates the flat gradient buffer when a parameter needs one,
    `engine_backward(d_flat, want_dx, want_dcond)` runs the engine's backward and returns (dx, dcond).  Releases the tape and returns
    the gradients of (x, cond, third input, engine, flat, table, *params): d_flat sliced by the table for the parameters."""
    want_dp = any(ctx.needs_input_grad[6:])
    d_flat = new_d_flat(ctx.flat) if want_dp else None
    dx, dcond = engine_backward(d_flat, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
    ctx.tape = None
    grads = [d_flat[off:off + n].view(shape) for (_, off, n, shape) in ctx.table] if want_dp else [None] * len(ctx.table)
    return (dx, dcond, None, None, None, None, *grads)


class UnetFn(torch.autograd.Function):
    """eps = U-Net(x, cond, t) with the weights of `flat`; `params` are the views of `flat` that receive the gradients."""

    @staticmethod
    def forward(ctx, x, cond, t, engine: Engine, flat, table, *params):
        eps, tape = engine.unet_train_forward(flat, x, cond, t)
        _keep(ctx, engine, flat, table, tape, None, x.detach(), cond.detach(), torch.as_tensor(t))
        return eps

    @staticmethod
    def backward(ctx, d_eps):
        x, cond, t = ctx.saved_tensors
        return _backward(ctx, torch.zeros_like, lambda d_flat, want_dx, want_dcond: ctx.engine.unet_backward(
            ctx.flat, x, cond, t, ctx.tape, d_eps.contiguous(), d_params=d_flat, want_dx=want_dx, want_dcond=want_dcond))


class _FlatParams:
    """The parameter surface of an nn.Module over ONE flat fp32 device tensor: `nn.Parameter` views of it under the reference's
    state_dict names.  A subclass sets `_strip` (a key of a caller's state_dict -> the reference name) and `_KEYS` (the prefixes of
    this model's names: an unknown key under one of them is an error of a strict load, any other key is ignored)."""

    def _init_params(self, table, nflat: int):
        self._flat = torch.zeros(nflat, dtype=torch.float32, device=self.device)
        self._params = {name: torch.nn.Parameter(self._flat[off:off + n].view(shape)) for name, off, n, shape in table}

    @property
    def flat(self) -> torch.Tensor:
        """The flat fp32 device buffer the parameters are views of (cld_unet_param_info / cld_vae_param_info layout)."""
        return self._flat

    def named_parameters(self):
        return iter(self._params.items())

    def parameters(self):
        return iter(self._params.values())

    def state_dict(self) -> dict:
        return {k: p.detach().clone() for k, p in self._params.items()}

    def load_state_dict(self, sd: Mapping, strict: bool = True):
        sd = {self._strip(k): v for k, v in sd.items()}
        missing = [k for k in self._params if k not in sd]
        unknown = [k for k in sd if k not in self._params and k.startswith(self._KEYS)]
        if strict and (missing or unknown):
            raise CldError(f"load_state_dict: missing {missing[:4]}, unknown {unknown[:4]}")
        copy_into_flat(self._params, sd, self.device)
        return self

    def zero_grad(self, set_to_none: bool = True):
        for p in self._params.values():
            if set_to_none:
                p.grad = None
            elif p.grad is not None:
                p.grad.zero_()


def _strip_dm(k: str) -> str:
    return k[3:] if k.startswith("dm.") else k


class _UnetModel:
    """`dm.model(x, aux_info, t)` (TemporalMapUnet.forward, temporal.py:122-180), differentiable."""

    def __init__(self, dm: "TrainableDm"):
        self._dm = dm

    def __call__(self, x, aux_info, time):
        return self._dm._unet(x, aux_info["cond_feat"], time)


class TrainableDm(_FlatParams):
    """A trainable DmModel (models/dm/dm_model.py:15-174) over the HIP training path.

    `weights`: the U-Net state_dict ("model.*" keys, optional "dm." prefix).  `parameters()` / `named_parameters()` /
    `state_dict()` / `load_state_dict()` follow the reference names; `model(x, aux_info, t)`, `compute_losses(aux_info, z0,
    t=None, noise=None)` and `log_prob(x_t, x_tm1, aux_info, t)` are differentiable with respect to the parameters (and to x /
    cond where those require grad).  `to_engine()` gives a finalized DmModel with the current weights for sampling."""

    _strip, _KEYS = staticmethod(_strip_dm), ("model.",)

    def __init__(self, weights: Mapping, n_timesteps: int = 100, device="cuda:0"):
        self.n_timesteps = int(n_timesteps)
        self.device = torch.device(device)
        self.engine = Engine(n_timesteps=self.n_timesteps, device=device)
        sd = {_strip_dm(k): v for k, v in weights.items() if _strip_dm(k).startswith("model.")}
        self.engine.load_state_dict(sd).finalize()     # the training calls need a finalized exact-fp32 U-Net handle
        self._table, nflat = self.engine.unet_param_table()
        self._init_params(self._table, nflat)
        self.load_state_dict(sd)
        self.model = _UnetModel(self)
        f = lambda a: torch.from_numpy(a).to(self.device)       # noqa: E731
        self.x_t_cof, self.noise_cof = f(self.engine.x_t_cof), f(self.engine.noise_cof)
        self.posterior_log_variance_clipped = f(self.engine.posterior_log_variance_clipped)

    # ------------------------------------------------------------------ the U-Net and the loss heads
    def _timesteps(self, t, B: int) -> torch.Tensor:
        t = torch.as_tensor(t, device=self.device).reshape(-1).long()
        if t.numel() == 1 and B != 1:
            t = t.expand(B)
        if t.numel() != B:
            raise CldError(f"expected {B} timesteps, got {t.numel()}")
        return t

    def _unet(self, x, cond, t):
        B = x.shape[0]
        t = self._timesteps(t, B)
        return UnetFn.apply(x.float(), cond.float(), t, self.engine, self._flat, self._table, *self._params.values())

    def compute_losses(self, aux_info, z0, t=None, noise=None):
        """dm_model.py:82-89: F.mse_loss(noise, U-Net(q_sample(z0, t, noise), cond, t)); `t` / `noise` default to the reference's
        draws (torch.randint / randn_like on the device).  q_sample runs without autograd (z0 gets no gradient: in the reference it
        is the frozen VAE's latent)."""
        B = len(z0)
        if t is None:
            t = torch.randint(0, self.n_timesteps, (B,), device=self.device)
        if noise is None:
            noise = torch.randn(B, 52, 4, device=self.device)
        t = self._timesteps(t, B)
        noise = torch.as_tensor(noise).to(self.device, torch.float32)
        z_noisy = self.engine.q_sample(z0, noise, t)
        eps = self._unet(z_noisy, aux_info["cond_feat"], t)
        return torch.nn.functional.mse_loss(noise, eps)

    def log_prob(self, x_t, x_t_minus_1, aux_info, t):
        """dm_model.py:165-174: log N(x_{t-1}; x_t_cof[t] x_t - noise_cof[t] eps, sigma_t) averaged over (T, D), per row.
        At t = 0 sigma_0 = exp(0.5 log 1e-20) = 1e-10: see INTEGRATION.md "Training" for what the gradient is there."""
        x_t = torch.as_tensor(x_t).to(self.device, torch.float32)
        x_tm1 = torch.as_tensor(x_t_minus_1).to(self.device, torch.float32)
        B = x_t.shape[0]
        t = self._timesteps(t, B)
        eps = self._unet(x_t, aux_info["cond_feat"], t)
        mean = self.x_t_cof[t].view(-1, 1, 1) * x_t - self.noise_cof[t].view(-1, 1, 1) * eps
        sigma = (0.5 * self.posterior_log_variance_clipped[t].view(-1, 1, 1)).exp()
        lp = -((x_tm1 - mean) ** 2) / (2 * sigma ** 2) - sigma.log() - math.log(math.sqrt(2 * math.pi))
        return lp.mean(dim=(1, 2))

    # ------------------------------------------------------------------ sampling with the current weights
    def to_engine(self, n_timesteps: Optional[int] = None, precision: str = "f32") -> DmModel:
        """A finalized DmModel (its own Engine, `n_timesteps` defaulting to this model's) holding the current weights, for the
        sampling path.  Call it again after optimiser steps: a finalized handle keeps the weights it was given."""
        n = self.n_timesteps if n_timesteps is None else int(n_timesteps)
        eng = Engine(n_timesteps=n, device=self.device, precision=precision)
        eng.load_state_dict(self.state_dict()).finalize()
        return DmModel(n_timesteps=n, device=self.device, engine=eng)


# ====================================================================== the LSTM-VAE
class VaeEncodeFn(torch.autograd.Function):
    """(mu, logvar) = encoder(x6, cond) with the weights of `flat` and the dropout mask (None: eval mode); `params` are the views of
    the encoder's 14 tensors, which receive the gradients."""

    @staticmethod
    def forward(ctx, x, cond, mask, engine: Engine, flat, table, *params):
        mu, lv, tape = engine.vae_encode_train(flat, x, cond, mask)
        _keep(ctx, engine, flat, table, tape, mask, x.detach(), cond.detach())
        return mu, lv

    @staticmethod
    def backward(ctx, d_mu, d_lv):
        x, cond = ctx.saved_tensors
        d_mu, d_lv = (None if d is None else d.contiguous() for d in (d_mu, d_lv))
        # empty_like: accumulate=0 writes every tensor of the encoder
        return _backward(ctx, torch.empty_like, lambda d_flat, want_dx, want_dcond: ctx.engine.vae_encode_backward(
            ctx.flat, x, cond, ctx.mask, ctx.tape, d_mu, d_lv, d_params=d_flat, want_dx=want_dx, want_dcond=want_dcond))


class VaeDecodeFn(torch.autograd.Function):
    """act = decoder(z, cond) with the weights of `flat` and the dropout mask; `params` are the views of the decoder's 12 tensors."""

    @staticmethod
    def forward(ctx, z, cond, mask, engine: Engine, flat, table, *params):
        act, tape = engine.vae_decode_train(flat, z, cond, mask)
        _keep(ctx, engine, flat, table, tape, mask, z.detach(), cond.detach())
        return act

    @staticmethod
    def backward(ctx, d_act):
        z, cond = ctx.saved_tensors
        # empty_like: accumulate=0 writes every tensor of the decoder
        return _backward(ctx, torch.empty_like, lambda d_flat, want_dz, want_dcond: ctx.engine.vae_decode_backward(
            ctx.flat, z, cond, ctx.mask, ctx.tape, d_act.contiguous(), d_params=d_flat, want_dz=want_dz, want_dcond=want_dcond))


_VAE_KEYS = ("lstm_enc.", "lstm_dec.", "mu.", "logvar.")


def _strip_vae(k: str) -> str:
    for p in ("vae.lstmvae.", "lstmvae."):
        if k.startswith(p):
            return k[len(p):]
    return k


class TrainableVae(_FlatParams):
    """A trainable LSTMVAE (models/vae/lstm_vae.py:54-99) over the HIP training path, with VaeModel.compute_vae_loss.

    `weights`: the LSTMVAE state_dict ('lstmvae.' / 'vae.lstmvae.' prefixes stripped; other keys, e.g. 'context_encoder.*', ignored).
    The 26 tensors live in ONE flat fp32 device tensor (`flat`, the cld_vae_param_info layout) and are exposed as `nn.Parameter` views
    under the reference names.  Like an nn.Module it starts in train mode: nn.LSTM's inter-layer dropout (p = `dropout`) is drawn on the
    device per call; `eval()` turns it off; every call also takes explicit masks [B,52,64] (0 or 1 / (1 - p)).  `traj2z`, `lstm_dec`
    and `forward` are differentiable with respect to the parameters and to x / z / context where those require grad (the encoder's and
    the decoder's dcond add).  `to_vae_model()` gives a finalized VaeModel with the current weights for the sampling path."""

    _strip, _KEYS = staticmethod(_strip_vae), _VAE_KEYS

    def __init__(self, weights: Mapping, device="cuda:0", dropout: float = 0.2):
        self.device = torch.device(device)
        self.p = float(dropout)
        self.training = True
        self.engine = Engine(device=device)       # the training calls read every weight from the flat buffer: no weights, no finalize
        table, nflat = self.engine.vae_param_table()
        self._init_params(table, nflat)
        enc = [e for e in table if not e[0].startswith("lstm_dec.")]
        dec = [e for e in table if e[0].startswith("lstm_dec.")]
        self._enc = (enc, [self._params[e[0]] for e in enc])
        self._dec = (dec, [self._params[e[0]] for e in dec])
        self.load_state_dict(weights)

    # ------------------------------------------------------------------ mode
    def train(self, mode: bool = True):
        self.training = bool(mode)
        return self

    def eval(self):
        return self.train(False)

    # ------------------------------------------------------------------ the model
    def _mask(self, B: int, mask):
        if mask is not None:
            return torch.as_tensor(mask).to(self.device, torch.float32)
        if not self.training or self.p == 0.0:
            return None
        return (torch.rand(B, 52, 64, device=self.device) >= self.p).float() / (1.0 - self.p)

    def _f32(self, t):
        return torch.as_tensor(t).to(self.device, torch.float32)

    def traj2z(self, x, context, noise=None, masks=None):
        """lstm_vae.py:87-99 -> (z, mu, logvar) [B,52,4]; `noise` replaces the reference's randn_like draw (drawn on the device when
        omitted); `masks`: the encoder's dropout mask.  The reparametrisation is torch autograd."""
        x, cond = self._f32(x), self._f32(context)
        B = x.shape[0]
        table, params = self._enc
        mu, lv = VaeEncodeFn.apply(x, cond, self._mask(B, masks), self.engine, self._flat, table, *params)
        noise = torch.randn(B, 52, 4, device=self.device) if noise is None else self._f32(noise)
        return mu + noise * torch.exp(0.5 * lv), mu, lv

    def lstm_dec(self, z, context, mask=None):
        """lstm_vae.py:44-52 -> act [B,52,2]."""
        z, cond = self._f32(z), self._f32(context)
        table, params = self._dec
        return VaeDecodeFn.apply(z, cond, self._mask(z.shape[0], mask), self.engine, self._flat, table, *params)

    def forward(self, x, context, noise=None, masks=None):
        """lstm_vae.py:82-85 -> (act [B,52,2], mu, logvar); masks = (encoder mask, decoder mask) or None."""
        me, md = (None, None) if masks is None else masks
        z, mu, lv = self.traj2z(x, context, noise, me)
        return self.lstm_dec(z, context, md), mu, lv

    __call__ = forward

    @staticmethod
    def compute_vae_loss(input, output, mu, logvar, beta):
        """vae_model.py:89-99 -> (loss, recon, kld): recon = mse(input[..., 4:6], output), kld = -0.5 sum(1 + lv - mu^2 - e^lv) / (B T)."""
        recon = F.mse_loss(input[..., 4:6], output)
        B, T, _ = mu.shape
        kld = -0.5 * torch.sum(1 + logvar - mu.pow(2) - logvar.exp()) / (B * T)
        return recon + beta * kld, recon, kld

    # ------------------------------------------------------------------ sampling with the current weights
    def to_vae_model(self) -> VaeModel:
        """A VaeModel (its own finalized Engine) holding the current weights, for traj2z / lstm_dec / decode on the sampling path.
        Call it again after optimiser steps.  Its state_dict() also loads into a DmModel's shared engine."""
        vae = VaeModel(device=self.device)
        return vae.load_state_dict(self.state_dict())
