"""Engine: one libcld_hip handle + its device workspace, driven with torch CUDA tensors.

PyTorch is plumbing here (device memory, streams); all arithmetic of the path
runs in the HIP library behind the C-ABI of include/cld.h.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math
from typing import Mapping, Optional

import numpy as np
import torch

from . import _lib
from ._lib import CldConfig, CldError

T, D, COND = 52, 4, 256

# the layers of the ContextEncoder's ResNet-18 in cld_debug_context_layer's order: (kernel, stride, input map size, C_in, C_out)
CONTEXT_LAYERS = [(7, 2, 224, 34, 64)]
for _li in range(4):
    _c, _hin = 64 << _li, 56 >> max(_li - 1, 0)
    _s = 1 if _li == 0 else 2
    CONTEXT_LAYERS += [(3, _s, _hin, _c // _s, _c), (3, 1, _hin // _s, _c, _c), (3, 1, _hin // _s, _c, _c), (3, 1, _hin // _s, _c, _c)]
CONTEXT_LAYERS += [(1, 2, 56 >> (_li - 1), 32 << _li, 64 << _li) for _li in range(1, 4)]

# the 12 spans of a U-Net evaluation in cld_debug_unet_span's order: (L, C) of each span's input per agent (span 8 / 11: and of its skip);
# span k's output is span k + 1's input, span 11's the noise prediction [52, 4]
UNET_SPANS = [(52, 4), (26, 64), (26, 128), (26, 128), (13, 128), (13, 256), (13, 256), (13, 256), (13, 256), (13, 128), (13, 128), (26, 128)]

# the raster settings of cld_rasterize (config.yaml:81-86, :96); observe.py re-exports them
RASTER_DEFAULTS = dict(height=224, width=224, px_per_m=2.0, ego_center=(-0.5, 0.0), no_map_fill=-1.0, max_neighbor_dist=30.0, n_sem=3)
# what a `map_source` takes besides its tensors: the same settings (max_neighbor_dist concerns the history planes only and is accepted so
# that a SceneObserver's settings pass as they are) and its own drivable_layer
MAP_SOURCE_DEFAULTS = dict(RASTER_DEFAULTS, drivable_layer=0)


def raster_frames(settings: Mapping, A: int):
    """raster_from_agent [A,3,3] of cld_rasterize for raster settings named as RASTER_DEFAULTS names them (include/cld.h):
    [[ppm, 0, (1 + ego_center[0]) / 2 * width], [0, ppm, (1 + ego_center[1]) / 2 * height], [0, 0, 1]]."""
    cfg = {k: settings.get(k, RASTER_DEFAULTS[k]) for k in ("height", "width", "px_per_m", "ego_center")}
    H, W, ppm, ec = cfg["height"], cfg["width"], cfg["px_per_m"], cfg["ego_center"]
    m = torch.tensor([[ppm, 0.0, (1.0 + ec[0]) / 2.0 * W], [0.0, ppm, (1.0 + ec[1]) / 2.0 * H], [0.0, 0.0, 1.0]], dtype=torch.float32)
    return m.expand(A, 3, 3).contiguous()


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def pair_incidences(target, ref, A: int):
    """The gather lists of a pair term (include/cld.h `cld_pair_term`): -> (agent_id: the agents 0..A-1 that sit in a pair, ascending,
    agent_start: offsets [len(agent_id) + 1], incidence: per agent its pair * 2 + role (0 = target, 1 = ref) in ascending order).
    An end outside 0..A-1 is listed nowhere."""
    per = {}
    for p, (i, j) in enumerate(zip(target, ref)):
        for role, a in enumerate((int(i), int(j))):
            if 0 <= a < A:
                per.setdefault(a, []).append(2 * p + role)
    ids = sorted(per)
    start, inc = [0], []
    for a in ids:
        inc += sorted(per[a])
        start.append(len(inc))
    return ids, start, inc


def solver_timesteps(n_timesteps: int, K: int):
    """The timestep subset of a K-step sampler: the unique values of rint(linspace(n_timesteps - 1, 0, K)), descending
    (n = 100, K = 10: 99, 88, ..., 11, 0)."""
    n_timesteps, K = int(n_timesteps), int(K)
    if n_timesteps < 1 or K < 1:
        raise CldError(f"solver_timesteps: n_timesteps = {n_timesteps} and K = {K} must be >= 1")
    ts = np.unique(np.rint(np.linspace(n_timesteps - 1, 0, K)).astype(np.int64))[::-1]
    return [int(t) for t in ts]


def parse_sampler(sampler: Mapping, n_timesteps: int):
    """A `sampler=` mapping {"kind": "ddim" | "dpmpp_2m", "steps": K or "timesteps": [...], "eta": float} -> (kind name, timesteps as a
    contiguous int32 array, eta), refused with a CldError naming the cause as include/cld_solver.h refuses it.  Needs no device."""
    if not isinstance(sampler, Mapping):
        raise CldError("sampler: expected a mapping {'kind', 'steps' | 'timesteps', 'eta'}")
    unknown = set(sampler) - {"kind", "steps", "timesteps", "eta"}
    if unknown:
        raise CldError(f"sampler: unknown keys {sorted(unknown)}")
    kind = sampler.get("kind")
    if kind not in _lib.SOLVER_KINDS:
        raise CldError(f"sampler: unknown kind '{kind}' (one of {sorted(_lib.SOLVER_KINDS)})")
    if (sampler.get("steps") is None) == (sampler.get("timesteps") is None):
        raise CldError("sampler: give exactly one of 'steps' (K) and 'timesteps' (a strictly decreasing list)")
    if sampler.get("steps") is not None:
        if int(sampler["steps"]) < 1:
            raise CldError("sampler: steps < 1 (K >= 1 timesteps)")
        ts = solver_timesteps(n_timesteps, int(sampler["steps"]))
    else:
        ts = [int(t) for t in sampler["timesteps"]]
    if len(ts) < 1:
        raise CldError("sampler: n_steps < 1 (K >= 1 timesteps)")
    for k, t in enumerate(ts):
        if not 0 <= t < n_timesteps:
            raise CldError(f"sampler: timestep out of range [0, n_timesteps) at index {k}")
        if k and t >= ts[k - 1]:
            raise CldError(f"sampler: timesteps not strictly decreasing at index {k}")
    eta = float(sampler.get("eta", 0.0) or 0.0)
    if not 0.0 <= eta <= 1.0:
        raise CldError("sampler: eta outside [0, 1]")
    if kind == "dpmpp_2m" and eta != 0.0:
        raise CldError("sampler: DPM-Solver++(2M) is deterministic: eta != 0 is refused")
    return kind, np.ascontiguousarray(ts, dtype=np.int32), eta


def refuse_sampler_guidance(guidance: Optional[Mapping]) -> None:
    """guide_clean / reconstruction guidance do not exist on the few-step path (include/cld_solver.h)."""
    if guidance is not None and (guidance.get("guide_clean") or guidance.get("reconstruction") is not None):
        which = "reconstruction (guide_clean=\"video_diff\")" if guidance.get("reconstruction") is not None or guidance.get("guide_clean") == "video_diff" else "guide_clean=True"
        raise NotImplementedError(f"sampler= together with {which} guidance is not built: the few-step samplers guide the mean form only")


def _param_table(lib, h, model):
    lib = lib or _lib.load()
    count, info, floats = (getattr(lib, f"cld_{model}_param_{s}") for s in ("count", "info", "floats"))
    out = []
    name, off, numel = C.c_char_p(), C.c_size_t(), C.c_size_t()
    shape, ndim = (C.c_int32 * 3)(), C.c_int32()
    for i in range(int(count(h))):
        _lib.check(h, info(h, i, C.byref(name), C.byref(off), C.byref(numel), shape, C.byref(ndim)), f"cld_{model}_param_info")
        out.append((name.value.decode(), int(off.value), int(numel.value), tuple(int(shape[d]) for d in range(ndim.value))))
    return out, int(floats(h))


def unet_param_table(lib=None, h=None):
    """cld_unet_param_info for all 148 U-Net tensors: ([(name, offset, numel, shape)], flat buffer length in floats).  The table is
    fixed by the architecture; it needs no handle and no device."""
    return _param_table(lib, h, "unet")


def copy_into_flat(views: Mapping, sd: Mapping, device) -> None:
    """Copy the tensors of `sd` into the views of a flat parameter buffer (`views`: name -> a view shaped as the table says); names
    `sd` lacks are left as they are, a shape that disagrees is an error.  What `train._FlatParams.load_state_dict` and
    `Engine.unet_flat_params` share."""
    with torch.no_grad():
        for k, p in views.items():
            if k in sd:
                v = torch.as_tensor(sd[k]).to(device=device, dtype=torch.float32)
                if tuple(v.shape) != tuple(p.shape):
                    raise CldError(f"load_state_dict: '{k}' expects shape {tuple(p.shape)}, got {tuple(v.shape)}")
                p.copy_(v)


def vae_param_table(lib=None, h=None):
    """cld_vae_param_info for all 26 LSTMVAE tensors, as unet_param_table."""
    return _param_table(lib, h, "vae")


# what a guided call reads from the handle, in the order it is set: (guidance dict key, Engine builder, library setter)
_HANDLE_TERMS = (("goal", "_goal", "cld_set_goal_term"), ("social_group", "_social", "cld_set_social_term"), ("pair", "_pair", "cld_set_pair_term"),
                 ("lane", "_lane", "cld_set_lane_term"), ("map_collision", "_map_source", "cld_set_map_source"))


class Engine:
    """Owns a `cld_handle`.  Weights come in under the reference's state_dict names."""

    def __init__(self, n_timesteps: int = 100, device="cuda:0", dynamics: Optional[Mapping] = None,
                 norm_info=None, step_time: float = 0.1, precision: str = "f32"):
        """precision: "f32" (exact fp32 MFMA) or "f16x2" (fp16 hi/lo split operands, fp32 accumulate; include/cld.h)."""
        self.lib = _lib.load()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise CldError("the CLD sampling path runs on an MI355X only (device must be cuda:N); no CPU fallback")
        if not torch.cuda.is_available():
            raise CldError("no HIP device visible; the CLD sampling path has no CPU fallback")
        cfg = CldConfig()
        self.lib.cld_default_config(C.byref(cfg))
        cfg.n_timesteps = int(n_timesteps)
        cfg.step_time = float(step_time)
        if precision not in _lib.PRECISIONS:
            raise CldError(f"unknown precision '{precision}' (f32 | f16x2)")
        cfg.precision = _lib.PRECISIONS[precision]
        if dynamics is not None:      # config.yaml:134-141
            if "acce_bound" in dynamics:
                cfg.acce_bound[0], cfg.acce_bound[1] = map(float, dynamics["acce_bound"])
            if "max_steer" in dynamics:
                cfg.max_steer = float(dynamics["max_steer"])
            if "max_yawvel" in dynamics:
                cfg.max_yawvel = float(dynamics["max_yawvel"])
        if norm_info is not None:     # config.yaml:161-164: [mean(6), std(6)]
            for i in range(6):
                cfg.norm_mean[i] = float(norm_info[0][i])
                cfg.norm_std[i] = float(norm_info[1][i])
        self.cfg = cfg
        self.n_timesteps = int(n_timesteps)
        self.stride = 1
        self._h = C.c_void_p()
        with torch.cuda.device(self.device):
            rc = self.lib.cld_create(C.byref(cfg), C.byref(self._h))
        if rc != 0:
            raise CldError(f"cld_create failed ({rc})")
        self._ws = self._ctx_ws = self._tws = self._vws = self._rws = self._recon_ws = self._solver_ws = None      # grow-only device scratch (_scratch): sampling, ContextEncoder,
                                                                                # U-Net training, VAE training, sort / Wasserstein,
                                                                                # reconstruction guidance
        self._nc_map_feat = {}
        self._unet_sd = {}
        self._finalized = False
        self.precision = {v: k for k, v in _lib.PRECISIONS.items()}[int(self.lib.cld_get_precision(self._h))]
        n = self.n_timesteps
        xc, nc, lv = (np.empty(n, np.float32) for _ in range(3))
        self._check(self.lib.cld_get_schedule(self._h, xc.ctypes.data, nc.ctypes.data, lv.ctypes.data), "cld_get_schedule")
        self.x_t_cof, self.noise_cof, self.posterior_log_variance_clipped = xc, nc, lv

    # ------------------------------------------------------------------ plumbing
    def _check(self, rc, what):
        _lib.check(self._h, rc, what)

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _scratch(self, slot: str, nbytes: int):
        """(pointer, size) of the scratch buffer kept in attribute `slot`, reallocated only when `nbytes` exceeds its size."""
        buf = getattr(self, slot)
        if buf is None or buf.numel() < nbytes:
            buf = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            setattr(self, slot, buf)
        return C.c_void_p(buf.data_ptr()), C.c_size_t(buf.numel())

    def _workspace(self, B: int):
        return self._scratch("_ws", int(self.lib.cld_workspace_bytes(self._h, B)))

    def _f32(self, t: torch.Tensor, shape=None) -> torch.Tensor:
        if not isinstance(t, torch.Tensor):
            t = torch.as_tensor(np.asarray(t))
        t = t.to(device=self.device, dtype=torch.float32).contiguous()
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise CldError(f"expected shape {tuple(shape)}, got {tuple(t.shape)}")
        return t

    def _per(self, v, n: int, div: float = 1.0) -> torch.Tensor:
        """A scalar weight (divided by `div`) for all n, or a tensor / sequence of length n as it is -> float32 [n] on the device."""
        if not isinstance(v, torch.Tensor) and np.isscalar(v):
            return torch.full((n,), float(v) / div, device=self.device)
        return self._f32(torch.as_tensor(v, dtype=torch.float32), (n,))

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self.lib.cld_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def set_stride(self, stride: int):
        """DmModel.stride (dm_model.py:25,119): the sampling loop visits i in reversed(range(0, n_timesteps, stride))."""
        self._check(self.lib.cld_set_stride(self._h, int(stride)), "cld_set_stride")
        self.stride = int(stride)

    def force_kernel(self, which: str, form: str = "auto"):
        """Tests only (cld_debug_force_kernel): run the "guide" / "decode" / "encode" kernel of this engine in its "valu" or
        "mfma" formulation instead of letting the batch size pick ("auto")."""
        try:
            fid = _lib.form_id(which, form)
        except ValueError as ex:
            raise CldError(f"force_kernel: {ex}") from None
        self._check(self.lib.cld_debug_force_kernel(self._h, _lib.KERNELS[which], fid), "cld_debug_force_kernel")

    def res_fold(self, mode: str = "fused"):
        """Tests only (cld_debug_res_fold): the 1x1 residual projections of spans 1, 4 and 8 inside their block's second conv ("fused":
        wherever that conv runs four-wave whole Winograd items: the default) or as launches of their own ("separate")."""
        if mode not in _lib.RES_FOLD:
            raise CldError(f"res_fold: unknown mode '{mode}' (one of {sorted(_lib.RES_FOLD)})")
        self._check(self.lib.cld_debug_res_fold(self._h, _lib.RES_FOLD[mode]), "cld_debug_res_fold")

    def debug_unet_span(self, span: int, x1, cond, t, x2=None):
        """Tests only (cld_debug_unet_span): span `span` (0..11) of a U-Net evaluation, the same launches `unet_forward` makes for it
        in the form `force_kernel("unet" / "conv5", ...)` holds.  x1 [B, L, C] (span 0: the latent [B,52,4]); x2 the skip [B, L, C]
        of spans 8 (ups.0.0) and 11 (ups.1.*); t one timestep for all rows or a [B] sequence.  Returns [B, L', C'] (span 11: eps [B,52,4])."""
        if not 0 <= span < len(UNET_SPANS):
            raise CldError(f"debug_unet_span: span {span} out of range")
        (L, C), (Lo, Co) = UNET_SPANS[span], (UNET_SPANS + [(52, 4)])[span + 1]
        B = int(x1.shape[0])
        x1 = self._f32(x1, (B, L, C))
        x2 = None if x2 is None else self._f32(x2, (B, L, C))
        cond = self._f32(cond, (B, 256))
        t_rows = None
        if isinstance(t, (int, np.integer)):
            t_idx = int(t)
        else:
            t_rows, t_idx = self._timesteps(t, B), 0
        y = torch.empty(B, Lo, Co, dtype=torch.float32, device=self.device)
        ws, nbytes = self._workspace(B)
        with torch.cuda.device(self.device):
            self._check(self.lib.cld_debug_unet_span(self._h, int(span), _ptr(x1), _ptr(x2), _ptr(cond), t_idx, _ptr(t_rows), _ptr(y), B,
                                                     ws, nbytes, self._stream()), "cld_debug_unet_span")
        return y

    def debug_context_layer(self, layer: int, x, residual=None, relu: bool = True):
        """Tests only (cld_debug_context_layer): layer `layer` of the ContextEncoder's ResNet-18 on n <= 256 agents, in the form
        `force_kernel("context", ...)` holds.  0: the stem, image [n,34,224,224] NCHW -> max-pooled [n,56,56,64] NHWC; 1..16:
        layer{li+1}.{b}.conv{c+1} + bn for layer = 1 + 4 li + 2 b + c; 17..19: the downsample of layer2..4.  NHWC in and out:
        y = [relu](bn(conv x) + residual)."""
        kh, stride, hin, cin, cout = CONTEXT_LAYERS[layer]
        n = int(x.shape[0])
        x = self._f32(x, (n, cin, hin, hin) if layer == 0 else (n, hin, hin, cin))
        ho = 56 if layer == 0 else hin // stride
        res = None if residual is None else self._f32(residual, (n, ho, ho, cout))
        y = torch.empty(n, ho, ho, cout, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self.lib.cld_debug_context_layer(self._h, int(layer), _ptr(x), _ptr(res), _ptr(y), n, int(bool(relu)), self._stream()),
                        "cld_debug_context_layer")
        return y

    @property
    def loop_steps(self) -> int:
        return len(range(0, self.n_timesteps, self.stride))

    # ------------------------------------------------------------------ weights
    def load_state_dict(self, sd: Mapping, strict: bool = True):
        """Accepts reference keys ('model.*', 'lstm_dec.*'; 'dm.' / 'vae.lstmvae.' prefixes stripped)."""
        if self._finalized:
            raise CldError("weights already finalized")
        for k, v in sd.items():
            name = k[3:] if k.startswith("dm.") else k
            if name.startswith("model."):      # references, not copies: what unet_flat_params() builds the training-layout buffer from
                self._unet_sd[name] = v
            a = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
            a = np.ascontiguousarray(a, dtype=np.float32)
            rc = self.lib.cld_load_weight(self._h, k.encode(), a.ctypes.data, a.size)
            if rc != 0 and strict:
                self._check(rc, f"cld_load_weight('{k}')")
        return self

    def finalize(self):
        with torch.cuda.device(self.device):
            self._check(self.lib.cld_finalize(self._h, self._stream()), "cld_finalize")
        self._finalized = True
        return self

    # ------------------------------------------------------------------ compute
    def unet_forward(self, x, cond, t_idx: int):
        x = self._f32(x)
        B = x.shape[0]
        x = self._f32(x, (B, T, D)); cond = self._f32(cond, (B, COND))
        eps = torch.empty_like(x)
        ws, wsn = self._workspace(B)
        with torch.cuda.device(self.device):
            self._check(self.lib.cld_unet_forward(self._h, _ptr(x), _ptr(cond), int(t_idx), _ptr(eps), B, ws, wsn,
                                                  self._stream()), "cld_unet_forward")
        return eps

    def unet_forward_rows(self, x, cond, t):
        """U-Net forward with one timestep per row: t [B] (any integer tensor)."""
        x = self._f32(x)
        B = x.shape[0]
        x = self._f32(x, (B, T, D)); cond = self._f32(cond, (B, COND))
        t = self._timesteps(t, B)
        eps = torch.empty_like(x)
        ws, wsn = self._workspace(B)
        with torch.cuda.device(self.device):
            self._check(self.lib.cld_unet_forward_t(self._h, _ptr(x), _ptr(cond), _ptr(t), _ptr(eps), B, ws, wsn, self._stream()),
                        "cld_unet_forward_t")
        return eps

    #: Device-resident timesteps are CLAMPED to [0, n_timesteps) without a check, to keep the call asynchronous (host values always raise
    #: when out of range).  Set True to have device tensors checked too -- a synchronising read per call; for debugging a caller that
    #: draws timesteps itself (e.g. randint(0, n + 1) would otherwise be mapped to a valid step silently).  INTEGRATION.md, "Timesteps".
    check_device_timesteps = False

    def _timesteps(self, t, B: int) -> torch.Tensor:
        """Per-row timesteps -> int32 [B] on the device.  Host values (lists, CPU tensors) are range-checked here; a device
        tensor is clamped to [0, n_timesteps) on the device instead, so the call stays asynchronous (the kernels index tables
        with these values; training-style callers draw them with torch.randint on the device, dm_model.py:84)."""
        t = torch.as_tensor(t).reshape(-1)
        if t.numel() != B:
            raise CldError(f"expected {B} timesteps, got {t.numel()}")
        if t.device.type == "cpu":
            if t.numel() and (int(t.min()) < 0 or int(t.max()) >= self.n_timesteps):
                raise CldError(f"timestep out of range [0, {self.n_timesteps})")
            return t.to(self.device, torch.int32).contiguous()
        if self.check_device_timesteps:      # opt-in (Engine.check_device_timesteps = True): costs a device round trip per call
            lo, hi = int(t.min()), int(t.max())
            if lo < 0 or hi >= self.n_timesteps:
                raise CldError(f"timestep out of range [0, {self.n_timesteps}): device tensor holds values in [{lo}, {hi}]")
        return t.to(self.device).clamp(0, self.n_timesteps - 1).to(torch.int32).contiguous()

    def q_sample(self, z0, noise, t):
        """DmModel.q_sample (dm_model.py:91-96): sqrt(acp[t]) z0 + sqrt(1 - acp[t]) noise, per-row t."""
        z0 = self._f32(z0)
        B = z0.shape[0]
        z0 = self._f32(z0, (B, T, D)); noise = self._f32(noise, (B, T, D))
        t = self._timesteps(t, B)
        zn = torch.empty_like(z0)
        ws, wsn = self._workspace(B)
        with torch.cuda.device(self.device):
            self._check(self.lib.cld_denoise_loss(self._h, _ptr(z0), _ptr(noise), None, _ptr(t), _ptr(zn), None, B,
                                                  ws, wsn, self._stream()), "cld_denoise_loss")
        return zn

    def denoise_loss(self, z0, noise, cond, t, want_z_noisy=False):
        """Forward half of DmModel.compute_losses (dm_model.py:82-96): per-sample MSE [B] between `noise` and the U-Net's
        prediction on q_sample(z0, t, noise); the reference's scalar loss is its mean."""
        z0 = self._f32(z0)
        B = z0.shape[0]
        z0 = self._f32(z0, (B, T, D)); noise = self._f32(noise, (B, T, D)); cond = self._f32(cond, (B, COND))
        t = self._timesteps(t, B)
        mse = torch.empty(B, dtype=torch.float32, device=self.device)
        zn = torch.empty_like(z0) if want_z_noisy else None
        ws, wsn = self._workspace(B)
        with torch.cuda.device(self.device):
            self._check(self.lib.cld_denoise_loss(self._h, _ptr(z0), _ptr(noise), _ptr(cond), _ptr(t), _ptr(zn), _ptr(mse), B,
                                                  ws, wsn, self._stream()), "cld_denoise_loss")
        return (mse, zn) if want_z_noisy else mse

    def ddpm_step(self, x, cond, t_idx: int, z):
        """DmModel.x_Tminus1 -> (x_next, mean, sigma).  z None: the noise is drawn on the device (seed 0, step 0), as by `sample_step`."""
        x = self._f32(x)
        B = x.shape[0]
        x = self._f32(x, (B, T, D)); cond = self._f32(cond, (B, COND))
        z = None if z is None else self._f32(z, (B, T, D))
        xn, mean = torch.empty_like(x), torch.empty_like(x)
        sigma = C.c_float()
        ws, wsn = self._workspace(B)
        with torch.cuda.device(self.device):
            self._check(self.lib.cld_ddpm_step(self._h, _ptr(x), _ptr(cond), int(t_idx), _ptr(z), _ptr(xn), _ptr(mean),
                                               C.byref(sigma), B, ws, wsn, self._stream()), "cld_ddpm_step")
        return xn, mean, float(sigma.value)

    def _guidance(self, g: Mapping, B: int):
        """dict(curr_states [B,4], target_speed [B,52] | None, loss_scale [B] | None, speed_limit (limit, scale) | None,
        acc_limit (limit, scale) | None, target_pos (pos [B,2], time index [B], scale) | None, lr | None, perturb_th | None | "sigma", optimizer "adam" | "sgd",
        grad_steps = 1, guide_clean = False, agent_collision: dict | None (see _collision), map_collision: dict | None (see _map_collision),
        goal: dict | None (see _goal; not part of the struct: sample / sample_step / guidance_step keep it on the handle for the call),
        social_group: dict | None (see _social; kept on the handle for the call likewise), pair: dict | None (see _pair; likewise),
        lane: dict | None (see _lane; likewise))
        -> (CldGuidance, tensors kept alive).  A `scale` is a per-agent tensor [B] (weight / (agents of the scene * 52),
        as DiffuserGuidance averages) or a scalar weight (divided by 52 here).  lr None = sigma_t; perturb_th None = no clip (what
        the reference's perturb() does), "sigma" = clip to sigma_t, a number = clip to it (include/cld.h)."""
        cs = self._f32(g["curr_states"], (B, 4))
        ts = None if g.get("target_speed") is None else self._f32(g["target_speed"], (B, T))
        ls = None if g.get("loss_scale") is None else self._f32(g["loss_scale"], (B,))
        # optional SpeedLimitLoss / AccLimitLoss terms: (limit, per-agent scale [B] or a scalar weight)
        def term(key):
            v = g.get(key)
            if v is None:
                return 0.0, None
            return float(v[0]), self._per(v[1], B, T)
        sl, sls = term("speed_limit")
        al, als = term("acc_limit")
        eg = None if g.get("ext_grad") is None else self._f32(g["ext_grad"], (B, T, 6))
        tp = tt = tps = None
        if g.get("target_pos") is not None:      # (positions [B,2], time index [B], per-agent scale [B] | scalar weight): TargetPosAtTimeLoss
            pos_, time_, sc = g["target_pos"]
            tp = self._f32(pos_, (B, 2))
            tt = torch.as_tensor(time_).to(self.device, torch.int32).contiguous()
            if tuple(tt.shape) != (B,):
                raise CldError(f"target_pos time index: expected shape ({B},), got {tuple(tt.shape)}")
            tps = self._per(sc, B)
        th = g.get("perturb_th")
        opt = g.get("optimizer", "adam")
        if opt not in _lib.OPTIMIZERS:
            raise CldError(f"unknown guidance optimizer '{opt}' (adam | sgd)")
        # guidance on the t = 0 output (upstream apply_guidance_output + final_step_opt_params, scene_edit_config.py:84-91):
        # "output": True | dict(lr, perturb_th, optimizer); "intermediate": False switches the t > 0 steps off
        fo = g.get("output")
        fo = {} if fo is True else fo
        fopt = (fo or {}).get("optimizer", "adam")
        if fopt not in _lib.OPTIMIZERS:
            raise CldError(f"unknown guidance optimizer '{fopt}' (adam | sgd)")
        fth = (fo or {}).get("perturb_th", None)       # None = no clip: what upstream's perturb() does (guidance_loss.py:2237,2273-2276)
        col = ckeep = mcol = mkeep = None
        if g.get("agent_collision") is not None:
            col, ckeep = self._collision(g["agent_collision"], B)
        if g.get("map_collision") is not None:
            mcol, mkeep = self._map_collision(g["map_collision"], B)
        cg = _lib.CldGuidance(cs.data_ptr(), None if ts is None else ts.data_ptr(), None if ls is None else ls.data_ptr(),
                              float(g["lr"]) if g.get("lr") else 0.0,
                              -1.0 if th is None else (0.0 if th == "sigma" else float(th)), _lib.OPTIMIZERS[opt],
                              sl, al, None if sls is None else sls.data_ptr(), None if als is None else als.data_ptr(),
                              None if tp is None else tp.data_ptr(), None if tt is None else tt.data_ptr(),
                              None if tps is None else tps.data_ptr(), None if eg is None else eg.data_ptr(),
                              0 if fo is None or fo is False else 1, 0 if g.get("intermediate", True) else 1,
                              float((fo or {}).get("lr", 0.3) or 0.0),
                              -1.0 if fth is None else (0.0 if fth == "sigma" else float(fth)), _lib.OPTIMIZERS[fopt],
                              int(g.get("grad_steps", 1) or 1), int((fo or {}).get("grad_steps", 1) or 1), 1 if g.get("guide_clean") else 0,
                              None if col is None else C.addressof(col), None if mcol is None else C.addressof(mcol))
        return cg, (cs, ts, ls, sls, als, tp, tt, tps, eg, col, ckeep, mcol, mkeep)

    def _collision(self, c: Mapping, B: int):
        """dict(extent [A,3], world_from_agent [A,3,3], curr_speed [A], scene_index [A] (consecutive blocks) | scene_sizes,
        weight: scalar or per-scene sequence (0 = scene not guided), agents: optional {scene: local indices} (upstream's
        `agents` of a guidance config), excluded_agents: optional batch indices (upstream's `excluded_agents`), num_samp = 1, num_disks = 5, buffer_dist = 0.2, decay_rate = 0.9,
        guide_moving_speed_th = 0.5) -> (CldCollision, tensors kept alive): upstream's AgentCollisionLoss
        (src/tbsim/utils/guidance_loss.py:442-630) configured per scene as DiffuserGuidance does (:2106-2172).  B = A * num_samp."""
        N = int(c.get("num_samp", 1))
        if B % N:
            raise CldError(f"agent_collision: {B} rows are not a multiple of num_samp = {N}")
        A = B // N
        ext = self._f32(c["extent"], (A, 3)); wfa = self._f32(c["world_from_agent"], (A, 3, 3)); spd = self._f32(c["curr_speed"], (A,))
        if c.get("scene_sizes") is None and c.get("scene_index") is None:       # (one scene by default is the map term's)
            raise CldError("agent_collision: needs scene_sizes or scene_index")
        sizes, start, wts = self._scene_blocks(c, A, "agent_collision")
        S = len(sizes)
        guided = None
        if c.get("agents"):
            gm = np.zeros(A, np.uint8)
            offs = np.concatenate([[0], np.cumsum(sizes)])
            for s_ in range(S):
                sub = c["agents"].get(s_)
                if sub is None:
                    gm[offs[s_]:offs[s_ + 1]] = 1
                else:
                    gm[offs[s_] + np.asarray(sub, dtype=np.int64)] = 1
            guided = torch.from_numpy(gm).to(self.device)
        excluded = None
        if c.get("excluded_agents") is not None:        # upstream's `excluded_agents` (:447,586-593): batch indices; a pair of two flagged agents is not penalised
            em = np.zeros(A, np.uint8)
            idx = np.asarray(list(c["excluded_agents"]), dtype=np.int64).reshape(-1)
            if idx.size and (idx.min() < 0 or idx.max() >= A):
                raise CldError(f"agent_collision: excluded_agents out of range for {A} agents")
            em[idx] = 1
            excluded = torch.from_numpy(em).to(self.device)
        cc = _lib.CldCollision(ext.data_ptr(), wfa.data_ptr(), spd.data_ptr(), start.data_ptr(), wts.data_ptr(),
                               None if guided is None else guided.data_ptr(), S, N, int(c.get("num_disks", 5)), max(sizes),
                               float(c.get("buffer_dist", 0.2)), float(c.get("decay_rate", 0.9)), float(c.get("guide_moving_speed_th", 0.5)),
                               None if excluded is None else excluded.data_ptr())
        return cc, (ext, wfa, spd, start, wts, guided, excluded)

    def _scene_blocks(self, c: Mapping, A: int, what: str):
        """-> (scene sizes, start offsets on the device, per-scene weights on the device) of a scene-structured loss config."""
        if c.get("scene_sizes") is not None:
            sizes = [int(v) for v in c["scene_sizes"]]
        elif c.get("scene_index") is not None:
            _, counts = torch.unique_consecutive(torch.as_tensor(c["scene_index"]).cpu(), return_counts=True)
            sizes = [int(v) for v in counts]
        else:
            sizes = [A]
        if sum(sizes) != A or min(sizes) < 1:
            raise CldError(f"{what}: scene sizes {sizes} do not cover the {A} agents")
        start = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32, device=self.device)
        return sizes, start, self._per(c.get("weight", 1.0), len(sizes))

    def _map_collision(self, c: Mapping, B: int):
        """dict(extent [A,3], raster_from_agent [A,3,3], drivable_map [A,H,W] (non-zero = drivable), curr_speed [A], scene_index |
        scene_sizes (default: one scene), weight: scalar or per-scene sequence, num_samp = 1, num_points_lw = (10, 10),
        decay_rate = 0.9, guide_moving_speed_th = 0.5) -> (CldMapCollision, tensors kept alive): upstream's MapCollisionLoss
        (src/tbsim/utils/guidance_loss.py:717-875).  In place of `drivable_map`: map_source = dict(maps, scene_map, map_from_world,
        world [A,3], drivable_layer = 0, height, width, px_per_m, ego_center, no_map_fill as RASTER_DEFAULTS names them) --
        the term then reads the scene maps themselves (H, W = height, width) and the struct has no drivable_map; the source goes to
        the handle around the library call (_handle_terms)."""
        N = int(c.get("num_samp", 1))
        if B % N:
            raise CldError(f"map_collision: {B} rows are not a multiple of num_samp = {N}")
        A = B // N
        missing = [k for k in ("extent", "raster_from_agent", "curr_speed") if c.get(k) is None]
        if missing:
            raise CldError(f"map_collision: missing {missing}")
        ext = self._f32(c["extent"], (A, 3)); rfa = self._f32(c["raster_from_agent"], (A, 3, 3)); spd = self._f32(c["curr_speed"], (A,))
        ms = c.get("map_source")
        if ms is not None and c.get("drivable_map") is not None:
            raise CldError("map_collision: drivable_map and map_source are two ways to say where the road is; pass one")
        if ms is None and c.get("drivable_map") is None:
            raise CldError("map_collision needs drivable_map or map_source")
        dm = None
        if ms is None:
            dm = torch.as_tensor(c["drivable_map"])
            if dm.dim() != 3 or dm.shape[0] != A:
                raise CldError(f"map_collision: drivable_map must be [{A},H,W], got {tuple(dm.shape)}")
            if not (dm.dtype == torch.uint8 and dm.device == self.device):     # (a resident uint8 map is taken as it is: non-zero = drivable)
                dm = (dm != 0).to(self.device, torch.uint8)
            dm = dm.contiguous()
            H, W = int(dm.shape[1]), int(dm.shape[2])
        else:
            unknown = sorted(set(ms) - set(MAP_SOURCE_DEFAULTS) - {"maps", "scene_map", "map_from_world", "world"})
            if unknown:
                raise CldError(f"map_collision: unknown map_source entries {unknown}")
            H, W = int(ms.get("height", MAP_SOURCE_DEFAULTS["height"])), int(ms.get("width", MAP_SOURCE_DEFAULTS["width"]))
        sizes, start, wts = self._scene_blocks(c, A, "map_collision")
        nl, nw = (int(v) for v in c.get("num_points_lw", (10, 10)))
        cc = _lib.CldMapCollision(ext.data_ptr(), rfa.data_ptr(), None if dm is None else dm.data_ptr(), spd.data_ptr(), start.data_ptr(),
                                  wts.data_ptr(), len(sizes), N, H, W, nl, nw, float(c.get("decay_rate", 0.9)),
                                  float(c.get("guide_moving_speed_th", 0.5)))
        return cc, (ext, rfa, dm, spd, start, wts)

    def _map_source(self, c: Mapping, B: int):
        """The `map_source` of a map_collision dict `c` (see _map_collision) -> (CldMapSource, tensors kept alive).  Tensors already on
        the device in the right type are read in place, as `rasterize` reads them."""
        ms = c["map_source"]
        N = int(c.get("num_samp", 1))
        A = B // N
        S = len(self._scene_blocks(c, A, "map_collision")[0])
        if ms.get("world") is None:
            raise CldError("map_collision: map_source needs world [A,3], the pose every agent's frame stands at")
        world = self._f32(ms["world"], (A, 3))
        mp = sm = mfw = None
        num_maps = map_h = map_w = 0
        n_sem = int(ms.get("n_sem", MAP_SOURCE_DEFAULTS["n_sem"]))
        if ms.get("maps") is not None:
            mp = self._f32(ms["maps"])
            if mp.dim() != 4:
                raise CldError(f"map_collision: map_source maps must be [num_maps,n_sem,map_h,map_w], got {tuple(mp.shape)}")
            if "n_sem" in ms and mp.shape[1] != n_sem:
                raise CldError(f"map_collision: map_source maps hold {mp.shape[1]} layers, n_sem = {n_sem}")
            num_maps, n_sem, map_h, map_w = (int(v) for v in mp.shape)
            if ms.get("scene_map") is None or ms.get("map_from_world") is None:
                raise CldError("map_collision: map_source maps need scene_map and map_from_world")
            sm = torch.as_tensor(ms["scene_map"]).to(self.device, torch.int32).contiguous()
            if tuple(sm.shape) != (S,):
                raise CldError(f"map_collision: map_source scene_map must be [{S}] (the term's scenes), got {tuple(sm.shape)}")
            mfw = self._f32(ms["map_from_world"], (num_maps, 3, 3))
        dp = lambda t: None if t is None else t.data_ptr()
        ec = ms.get("ego_center", MAP_SOURCE_DEFAULTS["ego_center"])
        src = _lib.CldMapSource(dp(mp), dp(sm), dp(mfw), world.data_ptr(), S, num_maps, n_sem, map_h, map_w, int(ms.get("drivable_layer", 0)),
                                float(ms.get("px_per_m", MAP_SOURCE_DEFAULTS["px_per_m"])), (C.c_float * 2)(float(ec[0]), float(ec[1])),
                                float(ms.get("no_map_fill", MAP_SOURCE_DEFAULTS["no_map_fill"])))
        return src, (mp, sm, mfw, world)

    @contextlib.contextmanager
    def _handle_terms(self, guidance: Optional[Mapping], B: int):
        """The entries of a guidance dict that are not part of the cld_guidance struct -- goal, social_group, pair, lane, and the
        `map_source` of a map_collision entry (_HANDLE_TERMS) -- kept on the handle for the library call inside (cld_set_*), in that
        order, and cleared behind it whatever happens, a builder or setter further down the list raising included: no term outlives the
        call that set it.  (World-frame lane polylines are prepared once, here, for the whole call.)"""
        held = []                                        # (setter, struct, tensors kept alive)
        try:
            for key, build, setter in _HANDLE_TERMS:
                c = None if guidance is None else guidance.get(key)
                if c is None or (key == "map_collision" and c.get("map_source") is None):
                    continue
                cs, keep = getattr(self, build)(c, B)
                self._check(getattr(self.lib, setter)(self._h, C.byref(cs)), setter)
                held.append((setter, cs, keep))
            yield
        finally:
            for setter, _, _ in reversed(held):
                getattr(self.lib, setter)(self._h, None)

    def _goal(self, c: Mapping, B: int):
        """dict(kind [A] (0 off | 1 global_target_pos | 2 global_target_pos_at_time, _lib.GOAL_KINDS), target_pos [A,2] (world),
        target_time [A] (rollout steps; kind 2), urgency [A], pref_speed [A], scale [A] (weight / agents of the config),
        agent_from_world [A,3,3], reached [A] | None, global_t = 0, dt = 0.1, min_progress_dist = 0.5, num_samp = 1)
        -> (CldGoal, tensors kept alive): upstream's GlobalTargetPosLoss / GlobalTargetPosAtTimeLoss
        (src/tbsim/utils/guidance_loss.py:876-1135) per agent.  B = A * num_samp."""
        N = int(c.get("num_samp", 1))
        if N < 1 or B % N:
            raise CldError(f"goal: {B} rows are not a multiple of num_samp = {N}")
        A = B // N
        missing = [k for k in ("kind", "target_pos", "urgency", "pref_speed", "scale", "agent_from_world") if c.get(k) is None]
        if missing:
            raise CldError(f"goal: missing {missing}")

        def i32(v, what):
            t = torch.as_tensor(v).to(self.device, torch.int32).contiguous()
            if tuple(t.shape) != (A,):
                raise CldError(f"goal {what}: expected shape ({A},), got {tuple(t.shape)}")
            return t
        kind = i32(c["kind"], "kind")
        tt = i32(c["target_time"], "target_time") if c.get("target_time") is not None else torch.zeros(A, dtype=torch.int32, device=self.device)
        tp = self._f32(c["target_pos"], (A, 2)); afw = self._f32(c["agent_from_world"], (A, 3, 3))
        urg = self._f32(c["urgency"], (A,)); ps = self._f32(c["pref_speed"], (A,)); sc = self._f32(c["scale"], (A,))
        rd = None
        if c.get("reached") is not None:
            rd = (torch.as_tensor(c["reached"]) != 0).to(self.device, torch.uint8).contiguous()
            if tuple(rd.shape) != (A,):
                raise CldError(f"goal reached: expected shape ({A},), got {tuple(rd.shape)}")
        cg = _lib.CldGoal(tp.data_ptr(), afw.data_ptr(), kind.data_ptr(), tt.data_ptr(), urg.data_ptr(), ps.data_ptr(), sc.data_ptr(),
                          None if rd is None else rd.data_ptr(), N, int(c.get("global_t", 0)), float(c.get("dt", 0.1)),
                          float(c.get("min_progress_dist", 0.5)))
        return cg, (tp, afw, kind, tt, urg, ps, sc, rd)

    def _social(self, c: Mapping, B: int):
        """dict(groups: one list of agent indices per group (each sorted ascending here), leader: per group an agent (batch) index | -1
        | None, social_dist = 1.5 and cohesion = 0.8: scalar or per group, scale [G] (d total / d value of a member row: weight /
        (members x samples)), world_from_agent [A,3,3], draw_r (int32) / draw_u: both or neither, [n_iter, n_opt, B, 52] (or [B, 52]
        for one evaluation), seed = 0, iter_base = 0, num_samp = 1, max_members: default the largest group)
        -> (CldSocialGroup, tensors kept alive): upstream's SocialGroupLoss (src/tbsim/utils/guidance_loss.py:1137-1207) over all
        groups of the batch.  B = A * num_samp."""
        N = int(c.get("num_samp", 1))
        if N < 1 or B % N:
            raise CldError(f"social_group: {B} rows are not a multiple of num_samp = {N}")
        A = B // N
        missing = [k for k in ("groups", "scale", "world_from_agent") if c.get(k) is None]
        if missing:
            raise CldError(f"social_group: missing {missing}")
        groups = [sorted(int(a) for a in torch.as_tensor(g).reshape(-1).tolist()) for g in c["groups"]]
        G = len(groups)
        flat = [a for g in groups for a in g]
        if G < 1 or not flat or min(flat) < 0 or max(flat) >= A:
            raise CldError(f"social_group: groups must name agents 0..{A - 1}")
        if len(set(flat)) != len(flat):
            raise CldError("social_group: an agent is in two groups")
        start = torch.tensor(np.concatenate([[0], np.cumsum([len(g) for g in groups])]), dtype=torch.int32, device=self.device)
        member = torch.tensor(flat, dtype=torch.int32, device=self.device)
        ld = c.get("leader")
        ld = [-1] * G if ld is None else [-1 if v is None else int(v) for v in (ld if isinstance(ld, (list, tuple)) else torch.as_tensor(ld).reshape(-1).tolist())]
        if len(ld) != G:
            raise CldError(f"social_group leader: expected {G} entries, got {len(ld)}")
        leader = torch.tensor(ld, dtype=torch.int32, device=self.device)
        sd, coh = self._per(c.get("social_dist", 1.5), G), self._per(c.get("cohesion", 0.8), G)
        sc = self._f32(torch.as_tensor(c["scale"], dtype=torch.float32), (G,))
        wfa = self._f32(c["world_from_agent"], (A, 3, 3))
        dr = du = None
        n_iter = n_opt = 0
        if (c.get("draw_r") is None) != (c.get("draw_u") is None):
            raise CldError("social_group: draw_r and draw_u go together (both or neither)")
        if c.get("draw_r") is not None:
            dr = torch.as_tensor(c["draw_r"]).to(self.device, torch.int32)
            du = self._f32(c["draw_u"])
            if dr.dim() == 2:
                dr, du = dr[None, None], du[None, None]
            if dr.dim() != 4 or tuple(dr.shape[2:]) != (B, T) or dr.shape != du.shape:
                raise CldError(f"social_group: draw_r / draw_u must be [n_iter, n_opt, {B}, {T}], got {tuple(dr.shape)} / {tuple(du.shape)}")
            dr, du = dr.contiguous(), du.contiguous()
            n_iter, n_opt = int(dr.shape[0]), int(dr.shape[1])
        cs = _lib.CldSocialGroup(start.data_ptr(), member.data_ptr(), leader.data_ptr(), sd.data_ptr(), coh.data_ptr(), sc.data_ptr(),
                                 wfa.data_ptr(), None if dr is None else dr.data_ptr(), None if du is None else du.data_ptr(),
                                 int(c.get("seed", 0)) & 0xFFFFFFFFFFFFFFFF, G, N, int(c.get("max_members") or max(len(g) for g in groups)),
                                 int(c.get("iter_base", 0)), n_iter, n_opt)
        return cs, (start, member, leader, sd, coh, sc, wfa, dr, du)

    def _plan_loss(self, call: str, build, traj, cfg: Mapping, grad_in, want_grad: bool, shape=None, want_proj=None, terms=None):
        """What the six stand-alone losses on decoded plans [B,52,6] share: shape the plans, `build(cfg, B)` -> the term's struct, the
        optional grad_in [B,52,6], the outputs -- values [B], or `shape(struct)`; the gradient if wanted; the projections [*shape,52,3] of a
        call that has them (want_proj not None) if wanted -- and the library call -> (values, gradient | None, projections | None)."""
        traj = self._f32(traj)
        B = traj.shape[0]
        traj = self._f32(traj, (B, T, 6))
        cs, keep = build(cfg, B)
        gi = None if grad_in is None else self._f32(grad_in, (B, T, 6))
        vshape = shape(cs) if shape else (B,)
        value = torch.empty(*vshape, dtype=torch.float32, device=self.device)
        grad = torch.empty(B, T, 6, dtype=torch.float32, device=self.device) if want_grad else None
        proj = torch.empty(*vshape, T, 3, dtype=torch.float32, device=self.device) if want_proj else None
        outs = (_ptr(value),) + (() if want_proj is None else (_ptr(proj),)) + (_ptr(grad),)
        with torch.cuda.device(self.device), self._handle_terms(terms, B):
            self._check(getattr(self.lib, call)(self._h, _ptr(traj), C.byref(cs), _ptr(gi), *outs, B, self._stream()), call)
        return value, grad, proj

    def social_group_loss(self, traj, term: Mapping, grad_in=None, want_grad=True):
        """Upstream's SocialGroupLoss on decoded plans [B,52,6] (descaled, sample-minor rows; `term`: see _social) -> (per-row values
        [B], 0 outside the groups, grad_in + d total / d traj [B,52,6]); cld_social_group_loss.  Caller draws: slab [0, 0]."""
        loss, grad, _ = self._plan_loss("cld_social_group_loss", self._social, traj, term, grad_in, want_grad)
        return (loss, grad) if want_grad else loss

    def _pair(self, c: Mapping, B: int):
        """dict(target [P], ref [P]: agent (batch) indices, kind [P]: a name or number of _lib.PAIR_KINDS (scalar or per pair), lo = 0
        (min distance / collision radius), hi = 0 (max distance), decay = 0 (<= 0: a plain mean over the steps): scalar or per pair,
        scale [P] (d total / d value of a (pair, sample)) or weight [P] (scale = weight / num_samp, upstream's weight * mean over the
        samples), world_from_agent [A,3,3], agent_from_world [A,3,3] | None (the inverse rotation of the former), num_samp = 1,
        validate = True: a pair outside the batch or with target == ref is a CldError; False: it reaches the kernel, which gives it
        a NaN value and no gradient) -> (CldPairTerm, tensors kept alive): upstream's pair-relation losses
        (src/tbsim/utils/guidance_loss.py:1631-1791, 1844-1956, 2014-2082) over all pairs of the batch.  B = A * num_samp."""
        N = int(c.get("num_samp", 1))
        if N < 1 or B % N:
            raise CldError(f"pair: {B} rows are not a multiple of num_samp = {N}")
        A = B // N
        missing = [k for k in ("target", "ref", "kind", "world_from_agent") if c.get(k) is None]
        if missing or (c.get("scale") is None and c.get("weight") is None):
            raise CldError(f"pair: missing {missing or ['scale | weight']}")
        tg = [int(v) for v in torch.as_tensor(c["target"]).reshape(-1).tolist()]
        rf = [int(v) for v in torch.as_tensor(c["ref"]).reshape(-1).tolist()]
        P = len(tg)
        if P < 1 or len(rf) != P:
            raise CldError(f"pair: target and ref must name the same number (>= 1) of pairs, got {P} / {len(rf)}")
        if c.get("validate", True):
            for p, (i, j) in enumerate(zip(tg, rf)):
                if not (0 <= i < A and 0 <= j < A) or i == j:
                    raise CldError(f"pair {p}: target {i} / ref {j} must be two different agents of 0..{A - 1}")
        kd = c["kind"]
        kd = [kd] * P if isinstance(kd, (str, int)) else list(kd.tolist() if isinstance(kd, (torch.Tensor, np.ndarray)) else kd)
        if len(kd) != P:
            raise CldError(f"pair kind: expected {P} entries, got {len(kd)}")
        try:
            kd = [_lib.PAIR_KINDS[k] if isinstance(k, str) else int(k) for k in kd]
        except KeyError as e:
            raise CldError(f"pair kind {e.args[0]!r}: one of {sorted(_lib.PAIR_KINDS)}") from None
        if any(k not in _lib.PAIR_KINDS.values() for k in kd):
            raise CldError(f"pair kind: numbers {sorted(_lib.PAIR_KINDS.values())}")
        lo, hi, dec = (self._per(c.get(k, 0.0), P) for k in ("lo", "hi", "decay"))
        sc = self._per(c["scale"], P) if c.get("scale") is not None else self._per(c["weight"], P) / N
        wfa = self._f32(c["world_from_agent"], (A, 3, 3))
        afw = None if c.get("agent_from_world") is None else self._f32(c["agent_from_world"], (A, 3, 3))
        ids, start, inc = pair_incidences(tg, rf, A)
        i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=self.device)
        tgt, reft, kind, start_t, ids_t, inc_t = i32(tg), i32(rf), i32(kd), i32(start), i32(ids if ids else [0]), i32(inc if inc else [0])
        cs = _lib.CldPairTerm(tgt.data_ptr(), reft.data_ptr(), kind.data_ptr(), lo.data_ptr(), hi.data_ptr(), dec.data_ptr(), sc.data_ptr(),
                              wfa.data_ptr(), None if afw is None else afw.data_ptr(), start_t.data_ptr(), ids_t.data_ptr(), inc_t.data_ptr(),
                              P, N, len(ids), len(inc))
        return cs, (tgt, reft, kind, lo, hi, dec, sc, wfa, afw, start_t, ids_t, inc_t)

    def pair_loss(self, traj, term: Mapping, grad_in=None, want_grad=True):
        """Upstream's pair-relation losses on decoded plans [B,52,6] (descaled, sample-minor rows; `term`: see _pair) -> (values
        [P, num_samp] as upstream's classes return them, grad_in + d total / d traj [B,52,6]); cld_pair_loss."""
        value, grad, _ = self._plan_loss("cld_pair_loss", self._pair, traj, term, grad_in, want_grad, shape=lambda cs: (cs.num_pairs, cs.num_samp))
        return (value, grad) if want_grad else value

    def lane_prepare(self, world_lines, line_frame, agent_from_world):
        """World-frame polylines [L,S,3] (x, y, heading; float64, NaN-padded), line_frame [L] (the row of agent_from_world [A,3,3] a
        line is taken into) -> agent-frame float32 polylines [L,S,3] sorted by (x, original index), NaN rows last: what a lane term
        reads (cld_lane_prepare; upstream's get_lane_projection from transform_xyh_np to the sort, trajdata_utils.py:573-656).
        S <= _lib.LANE_MAX_PTS."""
        wl = world_lines if isinstance(world_lines, torch.Tensor) else torch.as_tensor(np.asarray(world_lines))
        wl = wl.to(device=self.device, dtype=torch.float64).contiguous()
        if wl.dim() != 3 or wl.shape[2] != 3 or wl.shape[0] < 1:
            raise CldError(f"lane_prepare: world_lines must be [L,S,3], got {tuple(wl.shape)}")
        L, S = int(wl.shape[0]), int(wl.shape[1])
        afw = self._f32(agent_from_world)
        if afw.dim() != 3 or tuple(afw.shape[1:]) != (3, 3):
            raise CldError(f"lane_prepare: agent_from_world must be [A,3,3], got {tuple(afw.shape)}")
        fr = torch.as_tensor(line_frame).reshape(-1).to(device=self.device, dtype=torch.int32).contiguous()
        if fr.numel() != L:
            raise CldError(f"lane_prepare: {fr.numel()} frame indices for {L} lines")
        out = torch.empty(L, S, 3, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self.lib.cld_lane_prepare(self._h, _ptr(wl), _ptr(fr), _ptr(afw), _ptr(out), L, S, int(afw.shape[0]), self._stream()),
                        "cld_lane_prepare")
        return out

    def _lane(self, c: Mapping, B: int):
        """dict(agent [E]: agent (batch) indices, an agent's entries contiguous; line [E]: indices into the polylines; kind [E]: a name
        or number of _lib.LANE_KINDS (scalar or per entry); decay = 0.9 (follow_decayed), scalar or per entry; scale [E] (d total /
        d value of an (entry, sample)) or weight [E] (scale = weight / num_samp); the polylines either prepared, lines [L,S,3]
        (lane_prepare), or world_lines [L,S,3] float64 + agent_from_world [A,3,3] + line_frame [L] (default: the agent of the first
        entry that reads the line), prepared here; num_samp = 1; validate = True: an entry outside the batch or the polylines, or an
        agent whose entries are not contiguous, is a CldError; False: the entry reaches the kernel, which gives it a NaN value and
        no gradient) -> (CldLaneTerm, tensors kept alive): upstream's lane-projection losses (guidance_loss.py:1574-1628,
        1795-1841, 1958-2011) over all entries of the batch.  B = A * num_samp."""
        N = int(c.get("num_samp", 1))
        if N < 1 or B % N:
            raise CldError(f"lane: {B} rows are not a multiple of num_samp = {N}")
        A = B // N
        missing = [k for k in ("agent", "line", "kind") if c.get(k) is None]
        if missing or (c.get("scale") is None and c.get("weight") is None) or (c.get("lines") is None and c.get("world_lines") is None):
            raise CldError(f"lane: missing {missing or ['scale | weight, lines | world_lines']}")
        ag = [int(v) for v in torch.as_tensor(c["agent"]).reshape(-1).tolist()]
        ln = [int(v) for v in torch.as_tensor(c["line"]).reshape(-1).tolist()]
        E = len(ag)
        if E < 1 or len(ln) != E:
            raise CldError(f"lane: agent and line must name the same number (>= 1) of entries, got {E} / {len(ln)}")
        if c.get("lines") is not None:
            lines = self._f32(c["lines"])
        else:
            if c.get("agent_from_world") is None:
                raise CldError("lane: world_lines need agent_from_world")
            fr = c.get("line_frame")
            if fr is None:
                first = {}
                for a, l in zip(ag, ln):
                    first.setdefault(l, a)
                fr = [first.get(l, -1) for l in range(int(torch.as_tensor(c["world_lines"]).shape[0]))]
            lines = self.lane_prepare(c["world_lines"], fr, c["agent_from_world"])
        if lines.dim() != 3 or lines.shape[2] != 3 or not 2 <= lines.shape[1] <= _lib.LANE_MAX_PTS:
            raise CldError(f"lane: polylines must be [L, 2..{_lib.LANE_MAX_PTS}, 3], got {tuple(lines.shape)}")
        L = int(lines.shape[0])
        if c.get("validate", True):
            seen = set()
            for e, (a, l) in enumerate(zip(ag, ln)):
                if not (0 <= a < A and 0 <= l < L):
                    raise CldError(f"lane entry {e}: agent {a} / line {l} outside 0..{A - 1} / 0..{L - 1}")
                if a in seen and ag[e - 1] != a:
                    raise CldError(f"lane entry {e}: the entries of agent {a} are not contiguous")
                seen.add(a)
        kd = c["kind"]
        kd = [kd] * E if isinstance(kd, (str, int)) else list(kd.tolist() if isinstance(kd, (torch.Tensor, np.ndarray)) else kd)
        if len(kd) != E:
            raise CldError(f"lane kind: expected {E} entries, got {len(kd)}")
        try:
            kd = [_lib.LANE_KINDS[k] if isinstance(k, str) else int(k) for k in kd]
        except KeyError as e:
            raise CldError(f"lane kind {e.args[0]!r}: one of {sorted(_lib.LANE_KINDS)}") from None
        if any(k not in _lib.LANE_KINDS.values() for k in kd):
            raise CldError(f"lane kind: numbers {sorted(_lib.LANE_KINDS.values())}")
        dec = self._per(c.get("decay", 0.9), E)
        sc = self._per(c["scale"], E) if c.get("scale") is not None else self._per(c["weight"], E) / N
        i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=self.device)
        agt, lnt, kind = i32(ag), i32(ln), i32(kd)
        cs = _lib.CldLaneTerm(lines.data_ptr(), agt.data_ptr(), lnt.data_ptr(), kind.data_ptr(), dec.data_ptr(), sc.data_ptr(), E, L,
                              int(lines.shape[1]), N)
        return cs, (lines, agt, lnt, kind, dec, sc)

    def lane_loss(self, traj, term: Mapping, grad_in=None, want_grad=True, want_proj=False):
        """Upstream's lane-projection losses on decoded plans [B,52,6] (descaled, sample-minor rows; `term`: see _lane) -> values
        [E, num_samp] (unweighted) [, grad_in + d total / d traj [B,52,6]] [, the projections [E, num_samp, 52, 3]]; cld_lane_loss."""
        value, grad, proj = self._plan_loss("cld_lane_loss", self._lane, traj, term, grad_in, want_grad, shape=lambda cs: (cs.num_entries, cs.num_samp),
                                            want_proj=bool(want_proj))
        out = (value,) + ((grad,) if want_grad else ()) + ((proj,) if want_proj else ())
        return out if len(out) > 1 else value

    def goal_loss(self, traj, goal: Mapping, grad_in=None, want_grad=True):
        """Upstream's global waypoint losses on decoded plans [B,52,6] (descaled, sample-minor rows; `goal`: see _goal) ->
        (per-row values [B] as upstream files them under guide_losses, grad_in + scale * d value / d traj [B,52,6]); cld_goal_loss."""
        loss, grad, _ = self._plan_loss("cld_goal_loss", self._goal, traj, goal, grad_in, want_grad)
        return (loss, grad) if want_grad else loss

    def map_collision(self, traj, cfg: Mapping, grad_in=None, want_grad=True):
        """Upstream's MapCollisionLoss on decoded plans [B,52,6] (descaled, sample-minor rows) -> (per-plan values [B],
        d total / d traj [B,52,6]); cld_map_collision_loss."""
        loss, grad, _ = self._plan_loss("cld_map_collision_loss", self._map_collision, traj, cfg, grad_in, want_grad, terms={"map_collision": cfg})
        return (loss, grad) if want_grad else loss

    def agent_collision(self, traj, collision: Mapping, grad_in=None, want_grad=True):
        """Upstream's AgentCollisionLoss on decoded plans [B,52,6] (descaled, sample-minor rows) -> (per-agent values [B] as
        upstream files them under guide_losses, d total / d traj [B,52,6]); cld_agent_collision."""
        loss, grad, _ = self._plan_loss("cld_agent_collision", self._collision, traj, collision, grad_in, want_grad)
        return (loss, grad) if want_grad else loss

    def guidance_losses(self, traj, guidance: Mapping):
        """Per-agent values of the built-in guidance losses on decoded trajectories [B,52,6] (descaled) -> [B,4] =
        (target_speed, speed_limit, acc_limit, waypoint), NaN where a term is off for the agent: what upstream reports as
        `guide_losses` and selects samples by (guidance_loss.py:2143-2172, algos.py:2057-2064)."""
        traj = self._f32(traj)
        B = traj.shape[0]
        traj = self._f32(traj, (B, T, 6))
        g = dict(guidance)
        g.setdefault("curr_states", torch.zeros(B, 4, device=self.device))
        cg, keep = self._guidance(g, B)
        out = torch.empty(B, 4, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self.lib.cld_guidance_losses(self._h, _ptr(traj), C.byref(cg), _ptr(out), B, self._stream()), "cld_guidance_losses")
        return out

    def guidance_step(self, mean, cond, guidance: Mapping, sigma: float, z=None, want_grad=False):
        """One guidance step on a posterior mean [B,52,4] (upstream PerturbationGuidance.perturb, guidance_loss.py:2221-2282)
        -> guided mean (and x_next = guided + sigma z when z is given, dL/dmean when want_grad)."""
        mean = self._f32(mean)
        B = mean.shape[0]
        mean = self._f32(mean, (B, T, D)); cond = self._f32(cond, (B, COND))
        z = None if z is None else self._f32(z, (B, T, D))
        cg, keep = self._guidance(guidance, B)
        mg = torch.empty_like(mean)
        xn = torch.empty_like(mean) if z is not None else None
        gr = torch.empty_like(mean) if want_grad else None
        ws, wsn = self._workspace(B)
        with torch.cuda.device(self.device), self._handle_terms(guidance, B):
            self._check(self.lib.cld_guidance_step(self._h, _ptr(mean), _ptr(cond), C.byref(cg), C.c_float(sigma), _ptr(z),
                                                   _ptr(mg), _ptr(xn), _ptr(gr), B, ws, wsn, self._stream()), "cld_guidance_step")
        out = (mg,) + ((xn,) if z is not None else ()) + ((gr,) if want_grad else ())
        return out[0] if len(out) == 1 else out

    def decode_vjp(self, z, cond, curr_states, grad_traj):
        """Vector-Jacobian product of `decode` (LSTM decoder + descale + unicycle roll-out, descaled output): grad_traj
        [B,52,6] = dL/dtraj -> dL/dz [B,52,4].  With it any loss evaluated on decoded trajectories (torch autograd over
        upstream's guidance losses included) can be pulled back to the latent."""
        z = self._f32(z)
        B = z.shape[0]
        gd = {"curr_states": curr_states, "ext_grad": grad_traj, "lr": 1.0, "optimizer": "sgd"}
        _, grad = self.guidance_step(z, cond, gd, sigma=0.0, want_grad=True)
        return grad

    def sample_with_loss(self, x_T, cond, curr_states, noise, loss_fn, lr: Optional[float] = 0.3, optimizer: str = "adam",
                         perturb_th=None):
        """Ancestral loop with a CALLER-DEFINED guidance loss: `loss_fn(traj [B,52,6] descaled) -> scalar` is torch code
        (e.g. upstream's guidance losses, `src/tbsim/utils/guidance_loss.py`, which couple agents or sample rasters).  Per
        step t > 0: U-Net + posterior mean (HIP), decode the mean (HIP), dL/dtraj by torch autograd over `loss_fn` only,
        then decoder + roll-out backward, the optimiser step and the noise add (HIP, `cld_guidance_step` with `ext_grad`).
        Same semantics as `sample(..., guidance=)` (upstream diffuser.py:844-929); slower, because the loop is driven from
        Python.  `noise` [steps,B,52,4] is required.  -> (x0, x1)."""
        x = self._f32(x_T)
        B = x.shape[0]
        cond = self._f32(cond, (B, COND)); cs = self._f32(curr_states, (B, 4))
        n = self.loop_steps
        noise = self._f32(noise, (n, B, T, D))
        x1 = None
        for it in range(n):
            i = (n - 1 - it) * self.stride
            xn, mean, sigma = self.ddpm_step(x, cond, i, noise[it])
            if i == 0:
                x = xn
                break
            traj = self.decode(mean, cond, cs, descaled_output=True).requires_grad_(True)
            with torch.enable_grad():
                (gtraj,) = torch.autograd.grad(loss_fn(traj), traj)
            gd = {"curr_states": cs, "ext_grad": gtraj, "lr": lr, "perturb_th": perturb_th, "optimizer": optimizer}
            _, x = self.guidance_step(mean, cond, gd, sigma, z=noise[it])
            if i == 1:
                x1 = x.clone()
        return x, x1

    def sample(self, x_T, cond, noise=None, seed: int = 0, want_x1=True, want_logp=True,
               non_cond=None, guidance_w: float = 0.0, guidance: Optional[Mapping] = None):
        """Full ancestral loop.  With `non_cond` [B,256] and guidance_w != 0: classifier-free guidance
        (eps = (1+w) eps_cond - w eps_uncond, upstream diffuser.py:787), both passes as one 2B batch per step.
        With `guidance` (see `_guidance`): the posterior mean of every step t > 0 takes one optimiser step on the
        target-speed loss through decoder + roll-out before the noise is added (upstream diffuser.py:844-929).
        With guidance["reconstruction"] (see `_recon`): upstream's guide_clean="video_diff" instead -- the gradient is taken with respect
        to the noisy latent, through the denoiser (cld_sample_recon, include/cld_recon.h)."""
        x_T = self._f32(x_T)
        B = x_T.shape[0]
        x_T = self._f32(x_T, (B, T, D)); cond = self._f32(cond, (B, COND))
        n = self.loop_steps                 # loop iterations = noise slabs (n_timesteps with the reference's stride 1)
        noise = None if noise is None else self._f32(noise, (n, B, T, D))
        x0 = torch.empty_like(x_T)
        # x1 exists only when the loop visits step 1 (dm_model.py:126-127): stride 1 and at least two timesteps
        x1 = torch.empty_like(x_T) if (want_x1 and 1 in range(0, self.n_timesteps, self.stride)) else None
        logp = torch.empty(B, dtype=torch.float32, device=self.device) if want_logp else None
        cfg = non_cond is not None and guidance_w != 0.0
        with torch.cuda.device(self.device), self._handle_terms(guidance, B):
            if guidance is not None and guidance.get("reconstruction") is not None:
                cg, keep = self._guidance(guidance, B)
                rc, rkeep = self._recon(guidance["reconstruction"])
                non_cond = self._f32(non_cond, (B, COND)) if cfg else None
                ws, wsn = self._recon_workspace(B, cfg)
                self._check(self.lib.cld_sample_recon(self._h, _ptr(x_T), _ptr(noise), _ptr(cond), _ptr(non_cond),
                                                      C.c_float(guidance_w), C.byref(cg), C.byref(rc), n, _ptr(x0), _ptr(x1), _ptr(logp),
                                                      B, C.c_uint64(seed), ws, wsn, self._stream()), "cld_sample_recon")
            elif guidance is not None:
                cg, keep = self._guidance(guidance, B)
                non_cond = self._f32(non_cond, (B, COND)) if cfg else None
                ws, wsn = self._workspace(2 * ((B + 15) // 16 * 16) if cfg else B)
                self._check(self.lib.cld_sample_guided(self._h, _ptr(x_T), _ptr(noise), _ptr(cond), _ptr(non_cond),
                                                       C.c_float(guidance_w), C.byref(cg), n, _ptr(x0), _ptr(x1), _ptr(logp), B,
                                                       C.c_uint64(seed), ws, wsn, self._stream()), "cld_sample_guided")
            elif cfg:
                non_cond = self._f32(non_cond, (B, COND))
                ws, wsn = self._workspace(2 * ((B + 15) // 16 * 16))
                self._check(self.lib.cld_sample_cfg(self._h, _ptr(x_T), _ptr(noise), _ptr(cond), _ptr(non_cond),
                                                    C.c_float(guidance_w), n, _ptr(x0), _ptr(x1), _ptr(logp), B,
                                                    C.c_uint64(seed), ws, wsn, self._stream()), "cld_sample_cfg")
            else:
                ws, wsn = self._workspace(B)
                self._check(self.lib.cld_sample(self._h, _ptr(x_T), _ptr(noise), _ptr(cond), n, _ptr(x0), _ptr(x1),
                                                _ptr(logp), B, C.c_uint64(seed), ws, wsn, self._stream()), "cld_sample")
        return x0, x1, logp

    def sample_step(self, x_t, cond, t_idx: int, z=None, non_cond=None, guidance_w: float = 0.0, guidance: Optional[Mapping] = None,
                    want_grad: bool = False):
        """One iteration of `sample` at timestep t_idx on a given x_t (cld_sample_step; upstream p_sample, diffuser.py:844-929)
        -> dict(x_next, mean [posterior mean before guidance], sigma, and on a guided step mean_guided [, grad]).
        z None: the step's noise is drawn on the device, as the first iteration of `sample(noise=None, seed=0)` draws it."""
        x_t = self._f32(x_t)
        B = x_t.shape[0]
        x_t = self._f32(x_t, (B, T, D)); cond = self._f32(cond, (B, COND))
        z = None if z is None else self._f32(z, (B, T, D))
        cfg = non_cond is not None and guidance_w != 0.0
        non_cond = self._f32(non_cond, (B, COND)) if cfg else None
        cg = keep = None
        if guidance is not None:
            cg, keep = self._guidance(guidance, B)
        guided = guidance is not None and (bool(guidance.get("intermediate", True)) if t_idx > 0 else bool(guidance.get("output")))
        xn, mean = torch.empty_like(x_t), torch.empty_like(x_t)
        mg = torch.empty_like(x_t) if guided else None
        gr = torch.empty_like(x_t) if guided and want_grad else None
        ws, wsn = self._workspace(2 * ((B + 15) // 16 * 16) if cfg else B)
        sigma = C.c_float()
        with torch.cuda.device(self.device), self._handle_terms(guidance, B):
            self._check(self.lib.cld_sample_step(self._h, _ptr(x_t), _ptr(cond), _ptr(non_cond), C.c_float(guidance_w),
                                                 None if cg is None else C.byref(cg), int(t_idx), _ptr(z), _ptr(xn), _ptr(mean),
                                                 _ptr(mg), _ptr(gr), C.byref(sigma), B, ws, wsn, self._stream()), "cld_sample_step")
        out = {"x_next": xn, "mean": mean, "sigma": float(sigma.value)}
        if guided:
            out["mean_guided"] = mg
            if want_grad:
                out["grad"] = gr
        return out

    # ------------------------------------------------------------------ reconstruction guidance (include/cld_recon.h)
    def unet_flat_params(self, state_dict: Optional[Mapping] = None) -> torch.Tensor:
        """The U-Net weights of `state_dict` ("model.*" keys, optional "dm." prefix) as ONE flat fp32 device buffer in the layout
        of `unet_param_table`: what the taped forward and the backward of reconstruction guidance read.  Every tensor of the table
        must be present.  None: the tensors `load_state_dict` was given (the engine keeps references to them, not copies: they must
        not have been changed since)."""
        table, nflat = self.unet_param_table()
        sd = {(k[3:] if k.startswith("dm.") else k): v for k, v in (self._unet_sd if state_dict is None else state_dict).items()}
        missing = [name for name, *_ in table if name not in sd]
        if missing:
            raise CldError(f"unet_flat_params: missing {missing[:4]}")
        flat = torch.zeros(nflat, dtype=torch.float32, device=self.device)
        copy_into_flat({name: flat[off:off + n].view(shape) for name, off, n, shape in table}, sd, self.device)
        return flat

    def posterior_mean_coefs(self):
        """(posterior_mean_coef1, posterior_mean_coef2) of dm_model.py:50-53 as the handle holds them, float32 [n_timesteps] each."""
        c1, c2 = (np.empty(self.n_timesteps, np.float32) for _ in range(2))
        self._check(self.lib.cld_recon_get_posterior(self._h, c1.ctypes.data, c2.ctypes.data), "cld_recon_get_posterior")
        return c1, c2

    def _recon(self, r: Mapping):
        """dict(params: the flat buffer of `unet_flat_params` for the weights this engine was finalized with, lr: None = sigma_t,
        perturb_th: None = clip to sigma_t (upstream's `perturb_th is None`) | a number > 0 = upstream's schedule towards it | "none" =
        no clip, descend: False = upstream's sign AS WRITTEN, which ascends the loss | True = the evident intent)
        -> (CldRecon, tensors kept alive)."""
        params = r.get("params")
        if params is not None:
            if not isinstance(params, torch.Tensor) or params.dtype != torch.float32 or not params.is_cuda or not params.is_contiguous():
                raise CldError("reconstruction: params must be a contiguous float32 tensor on the engine's device (Engine.unet_flat_params)")
            if params.numel() != self.unet_param_table()[1]:
                raise CldError(f"reconstruction: params has {params.numel()} floats, the table asks for {self.unet_param_table()[1]}")
        th = r.get("perturb_th")
        if th is not None and th != "none" and not float(th) > 0.0:
            raise CldError("reconstruction: perturb_th is None (sigma_t), a number > 0, or \"none\"")
        rc = _lib.CldRecon(None if params is None else params.data_ptr(), float(r["lr"]) if r.get("lr") else 0.0, 0.0 if th is None else (-1.0 if th == "none" else float(th)),
                           1 if r.get("descend") else 0)
        return rc, (params,)

    def _recon_workspace(self, B: int, cfg: bool):
        return self._scratch("_recon_ws", int(self.lib.cld_recon_workspace_bytes(self._h, B, int(cfg))))

    def recon_step(self, x_t, cond, t_idx: int, guidance: Mapping, z=None, non_cond=None, guidance_w: float = 0.0, seed: int = 0,
                   salt: int = 0):
        """One iteration of `sample(..., guidance=dict(..., reconstruction=...))` at timestep t_idx on a given x_t (cld_recon_step;
        upstream p_sample with guide_clean="video_diff", diffuser.py:844-929) -> dict(x_next, mean, sigma, and at t_idx > 0 x0_hat,
        grad_xt = dL/dx_t, x0_guided).  z None: the step's noise is drawn on the device for (seed, salt)."""
        x_t = self._f32(x_t)
        B = x_t.shape[0]
        x_t = self._f32(x_t, (B, T, D)); cond = self._f32(cond, (B, COND))
        z = None if z is None else self._f32(z, (B, T, D))
        cfg = non_cond is not None and guidance_w != 0.0
        non_cond = self._f32(non_cond, (B, COND)) if cfg else None
        cg, keep = self._guidance(guidance, B)
        rc, rkeep = self._recon(guidance.get("reconstruction") or {})
        guided = t_idx > 0
        xn, mean = torch.empty_like(x_t), torch.empty_like(x_t)
        x0h, gx, x0g = ((torch.empty_like(x_t) for _ in range(3)) if guided else (None, None, None))
        ws, wsn = self._recon_workspace(B, cfg)
        sigma = C.c_float()
        with torch.cuda.device(self.device), self._handle_terms(guidance, B):
            self._check(self.lib.cld_recon_step(self._h, _ptr(x_t), _ptr(cond), _ptr(non_cond), C.c_float(guidance_w), C.byref(cg),
                                                C.byref(rc), int(t_idx), _ptr(z), _ptr(xn), _ptr(x0h), _ptr(gx), _ptr(x0g), _ptr(mean),
                                                C.byref(sigma), B, C.c_uint64(seed), C.c_uint64(salt), ws, wsn, self._stream()),
                        "cld_recon_step")
        out = {"x_next": xn, "mean": mean, "sigma": float(sigma.value)}
        if guided:
            out.update(x0_hat=x0h, grad_xt=gx, x0_guided=x0g)
        return out

    # ------------------------------------------------------------------ few-step sampling (include/cld_solver.h)
    def _solver(self, sampler: Mapping):
        """`sampler=` mapping (parse_sampler) -> (CldSolver, the int32 array it points into, kept alive)."""
        kind, ts, eta = parse_sampler(sampler, self.n_timesteps)
        return _lib.CldSolver(_lib.SOLVER_KINDS[kind], len(ts), ts.ctypes.data, eta), ts

    def _solver_workspace(self, B: int, cfg: bool):
        return self._scratch("_solver_ws", int(self.lib.cld_solver_workspace_bytes(self._h, B, int(cfg))))

    def solver_grid_cap(self, cap: int = 0) -> int:
        """Tests only (cld_debug_solver_grid_cap): the most workgroups the solver step kernel takes; cap < 1 restores the default."""
        return int(self.lib.cld_debug_solver_grid_cap(int(cap)))

    def debug_solver_kernel(self, sampler: Mapping, k: int, x, eps, eps_uncond=None, guidance_w: float = 0.0, x0_prev=None, z=None, seed: int = 0):
        """Tests only (cld_debug_solver_kernel): the step kernel alone on a given noise prediction -> dict(x_next, x0_hat, mu)."""
        sv, ts = self._solver(sampler)
        x = self._f32(x)
        B = x.shape[0]
        x, eps = self._f32(x, (B, T, D)), self._f32(eps, (B, T, D))
        eu, prev, z = (None if v is None else self._f32(v, (B, T, D)) for v in (eps_uncond, x0_prev, z))
        xn, x0h, mu = (torch.empty_like(x) for _ in range(3))
        with torch.cuda.device(self.device):
            self._check(self.lib.cld_debug_solver_kernel(self._h, C.byref(sv), int(k), _ptr(x), _ptr(eps), _ptr(eu), C.c_float(guidance_w), _ptr(prev),
                                                         _ptr(z), _ptr(xn), _ptr(x0h), _ptr(mu), B, C.c_uint64(seed), self._stream()),
                        "cld_debug_solver_kernel")
        return {"x_next": xn, "x0_hat": x0h, "mu": mu}

    def solver_tables(self, sampler: Mapping) -> dict:
        """The fp32 per-step coefficients the library applies (cld_solver_tables): dict(timesteps, a, b, c0, c1, sqrt_recip_acp,
        sqrt_recipm1_acp, sigma, sigma_g), float32 [K] each."""
        sv, ts = self._solver(sampler)
        tab = np.empty((len(ts), len(_lib.SOLVER_TABLE_COLS)), np.float32)
        self._check(self.lib.cld_solver_tables(self._h, C.byref(sv), tab.ctypes.data), "cld_solver_tables")
        out = {name: tab[:, i].copy() for i, name in enumerate(_lib.SOLVER_TABLE_COLS)}
        out["timesteps"] = ts.copy()
        return out

    def sample_solver(self, x_T, cond, sampler: Mapping, noise=None, seed: int = 0, non_cond=None, guidance_w: float = 0.0,
                      guidance: Optional[Mapping] = None):
        """The few-step loop (cld_sample_solver): DDIM(eta) or DPM-Solver++(2M) on the sampler's K timesteps -> x0 [B,52,4].  noise
        [K,B,52,4] or None (the device generator, the draws of `sample`'s iteration k); eta = 0 and 2M draw nothing.  CFG and
        `guidance` (mean form; see `_guidance`) as in `sample`.  The reference has no counterpart of this mode."""
        refuse_sampler_guidance(guidance)
        sv, ts = self._solver(sampler)
        x_T = self._f32(x_T)
        B = x_T.shape[0]
        x_T = self._f32(x_T, (B, T, D)); cond = self._f32(cond, (B, COND))
        noise = None if noise is None else self._f32(noise, (len(ts), B, T, D))
        cfg = non_cond is not None and guidance_w != 0.0
        non_cond = self._f32(non_cond, (B, COND)) if cfg else None
        x0 = torch.empty_like(x_T)
        with torch.cuda.device(self.device), self._handle_terms(guidance, B):
            cg = keep = None
            if guidance is not None:
                cg, keep = self._guidance(guidance, B)
            ws, wsn = self._solver_workspace(B, cfg)
            self._check(self.lib.cld_sample_solver(self._h, C.byref(sv), _ptr(x_T), _ptr(noise), _ptr(cond), _ptr(non_cond), C.c_float(guidance_w),
                                                   None if cg is None else C.byref(cg), _ptr(x0), B, C.c_uint64(seed), ws, wsn, self._stream()),
                        "cld_sample_solver")
        return x0

    def solver_step(self, x_t, cond, sampler: Mapping, k: int, x0_prev=None, z=None, non_cond=None, guidance_w: float = 0.0,
                    guidance: Optional[Mapping] = None, seed: int = 0, want_grad: bool = False):
        """Step k of `sample_solver` on a given x_t (cld_solver_step) -> dict(x_next, x0_hat, mu [the deterministic part before
        guidance], x0_prev [this step's x0_hat: what the next step takes], and on a guided step mu_guided [, grad]).  x0_prev: the
        preceding step's clean prediction, needed by a second-order step (2M, 0 < k < K-1); it is not modified.  z None: the step's
        noise is drawn on the device for (seed, k)."""
        refuse_sampler_guidance(guidance)
        sv, ts = self._solver(sampler)
        x_t = self._f32(x_t)
        B = x_t.shape[0]
        x_t = self._f32(x_t, (B, T, D)); cond = self._f32(cond, (B, COND))
        z = None if z is None else self._f32(z, (B, T, D))
        hist = None if x0_prev is None else self._f32(x0_prev, (B, T, D)).clone()
        cfg = non_cond is not None and guidance_w != 0.0
        non_cond = self._f32(non_cond, (B, COND)) if cfg else None
        last = int(k) == len(ts) - 1
        guided = guidance is not None and (bool(guidance.get("output")) if last else bool(guidance.get("intermediate", True)))
        xn, x0h, mu = (torch.empty_like(x_t) for _ in range(3))
        mg = torch.empty_like(x_t) if guided else None
        gr = torch.empty_like(x_t) if guided and want_grad else None
        with torch.cuda.device(self.device), self._handle_terms(guidance, B):
            cg = keep = None
            if guidance is not None:
                cg, keep = self._guidance(guidance, B)
            ws, wsn = self._solver_workspace(B, cfg)
            self._check(self.lib.cld_solver_step(self._h, C.byref(sv), int(k), _ptr(x_t), _ptr(hist), _ptr(z), _ptr(cond), _ptr(non_cond),
                                                 C.c_float(guidance_w), None if cg is None else C.byref(cg), _ptr(xn), _ptr(x0h), _ptr(mu),
                                                 _ptr(mg), _ptr(gr), B, C.c_uint64(seed), ws, wsn, self._stream()), "cld_solver_step")
        out = {"x_next": xn, "x0_hat": x0h, "mu": mu, "x0_prev": x0h if hist is None else hist}
        if guided:
            out["mu_guided"] = mg
            if want_grad:
                out["grad"] = gr
        return out

    # ------------------------------------------------------------------ training (exact fp32; cld_unet_train_forward / cld_unet_backward)
    def unet_param_table(self):
        """[(name, offset, numel, shape)] of the 148 U-Net tensors in the flat parameter buffer, and the buffer's length in floats."""
        return unet_param_table(self.lib, self._h)

    def unet_train_forward(self, params, x, cond, t):
        """eps [B,52,4] of the U-Net with the weights of `params` (flat fp32 device buffer, `unet_param_table` layout) and one
        timestep per row, plus the tape `unet_backward` needs (a uint8 device tensor)."""
        x = self._f32(x)
        B = x.shape[0]
        x = self._f32(x, (B, T, D)); cond = self._f32(cond, (B, COND))
        t = self._timesteps(t, B)
        eps = torch.empty_like(x)
        tape = torch.empty(int(self.lib.cld_unet_tape_bytes(self._h, B)), dtype=torch.uint8, device=self.device)
        ws, wsn = self._scratch("_tws", int(self.lib.cld_unet_train_workspace_bytes(self._h, B)))
        with torch.cuda.device(self.device):
            self._check(self.lib.cld_unet_train_forward(self._h, _ptr(params), _ptr(x), _ptr(cond), _ptr(t), _ptr(eps), _ptr(tape),
                                                        tape.numel(), B, ws, wsn, self._stream()), "cld_unet_train_forward")
        return eps, tape

    def unet_backward(self, params, x, cond, t, tape, d_eps, d_params=None, want_dx=True, want_dcond=False, accumulate=False):
        """Gradients of the U-Net for the cotangent d_eps [B,52,4] from the tape of `unet_train_forward` on the same params / x /
        cond / t.  d_params: flat fp32 device buffer that receives (accumulate=False) or adds (True) the parameter gradients, or
        None.  Returns (dx [B,52,4] or None, dcond [B,256] or None)."""
        x = self._f32(x)
        B = x.shape[0]
        x = self._f32(x, (B, T, D)); cond = self._f32(cond, (B, COND)); d_eps = self._f32(d_eps, (B, T, D))
        t = self._timesteps(t, B)
        dx = torch.empty_like(x) if want_dx else None
        dcond = torch.empty_like(cond) if want_dcond else None
        ws, wsn = self._scratch("_tws", int(self.lib.cld_unet_train_workspace_bytes(self._h, B)))
        with torch.cuda.device(self.device):
            self._check(self.lib.cld_unet_backward(self._h, _ptr(params), _ptr(x), _ptr(cond), _ptr(t), _ptr(tape), tape.numel(),
                                                   _ptr(d_eps), _ptr(d_params), _ptr(dx), _ptr(dcond), int(bool(accumulate)), B,
                                                   ws, wsn, self._stream()), "cld_unet_backward")
        return dx, dcond

    # ------------------------------------------------------------------ VAE training (exact fp32; cld_vae_*_train / cld_vae_*_backward)
    def vae_param_table(self):
        """[(name, offset, numel, shape)] of the 26 LSTMVAE tensors in the flat parameter buffer, and the buffer's length in floats."""
        return vae_param_table(self.lib, self._h)

    def _vae_args(self, x, width, cond, mask):
        x = self._f32(x)
        B = x.shape[0]
        return (B, self._f32(x, (B, T, width)), self._f32(cond, (B, COND)),
                None if mask is None else self._f32(mask, (B, T, 64)))

    def vae_encode_train(self, params, x6, cond, mask=None):
        """(mu, logvar) [B,52,4] of the encoder with the weights of `params` (flat fp32 device buffer, `vae_param_table` layout) and
        the dropout mask [B,52,64] of layer 0's output (None: eval mode), plus the tape `vae_encode_backward` needs."""
        B, x, cond, mask = self._vae_args(x6, 6, cond, mask)
        mu, lv = (torch.empty(B, T, D, dtype=torch.float32, device=self.device) for _ in range(2))
        tape = torch.empty(int(self.lib.cld_vae_tape_bytes(self._h, 0, B)), dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self.lib.cld_vae_encode_train(self._h, _ptr(params), _ptr(x), _ptr(cond), _ptr(mask), _ptr(mu), _ptr(lv),
                                                      _ptr(tape), tape.numel(), B, self._stream()), "cld_vae_encode_train")
        return mu, lv, tape

    def vae_encode_backward(self, params, x6, cond, mask, tape, d_mu, d_logvar, d_params=None, want_dx=True, want_dcond=False,
                            accumulate=False):
        """Gradients of the encoder for the cotangents d_mu / d_logvar [B,52,4] (None: zero) from the tape of `vae_encode_train` on the
        same params / x6 / cond / mask.  d_params: flat fp32 device buffer whose encoder tensors receive (accumulate=False) or add
        (True) the gradients, or None.  Returns (dx6 [B,52,6] or None, dcond [B,256] or None)."""
        B, x, cond, mask = self._vae_args(x6, 6, cond, mask)
        d_mu = None if d_mu is None else self._f32(d_mu, (B, T, D))
        d_logvar = None if d_logvar is None else self._f32(d_logvar, (B, T, D))
        dx = torch.empty_like(x) if want_dx else None
        dcond = torch.empty_like(cond) if want_dcond else None
        ws, wsn = self._scratch("_vws", int(self.lib.cld_vae_train_workspace_bytes(self._h, B)))
        with torch.cuda.device(self.device):
            self._check(self.lib.cld_vae_encode_backward(self._h, _ptr(params), _ptr(x), _ptr(cond), _ptr(mask), _ptr(tape), tape.numel(),
                                                         _ptr(d_mu), _ptr(d_logvar), _ptr(d_params), _ptr(dx), _ptr(dcond),
                                                         int(bool(accumulate)), B, ws, wsn, self._stream()), "cld_vae_encode_backward")
        return dx, dcond

    def vae_decode_train(self, params, z, cond, mask=None):
        """act [B,52,2] of the decoder with the weights of `params` and the dropout mask (None: eval mode), plus its tape."""
        B, z, cond, mask = self._vae_args(z, D, cond, mask)
        act = torch.empty(B, T, 2, dtype=torch.float32, device=self.device)
        tape = torch.empty(int(self.lib.cld_vae_tape_bytes(self._h, 1, B)), dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self.lib.cld_vae_decode_train(self._h, _ptr(params), _ptr(z), _ptr(cond), _ptr(mask), _ptr(act), _ptr(tape),
                                                      tape.numel(), B, self._stream()), "cld_vae_decode_train")
        return act, tape

    def vae_decode_backward(self, params, z, cond, mask, tape, d_act, d_params=None, want_dz=True, want_dcond=False, accumulate=False):
        """Gradients of the decoder for d_act [B,52,2]; as vae_encode_backward.  Returns (dz [B,52,4] or None, dcond or None)."""
        B, z, cond, mask = self._vae_args(z, D, cond, mask)
        d_act = self._f32(d_act, (B, T, 2))
        dz = torch.empty_like(z) if want_dz else None
        dcond = torch.empty_like(cond) if want_dcond else None
        ws, wsn = self._scratch("_vws", int(self.lib.cld_vae_train_workspace_bytes(self._h, B)))
        with torch.cuda.device(self.device):
            self._check(self.lib.cld_vae_decode_backward(self._h, _ptr(params), _ptr(z), _ptr(cond), _ptr(mask), _ptr(tape), tape.numel(),
                                                         _ptr(d_act), _ptr(d_params), _ptr(dz), _ptr(dcond), int(bool(accumulate)), B,
                                                         ws, wsn, self._stream()), "cld_vae_decode_backward")
        return dz, dcond

    def log_prob(self, x_t, x_tm1, cond, t_idx: int):
        x_t = self._f32(x_t)
        M = x_t.shape[0]
        x_t = self._f32(x_t, (M, T, D)); x_tm1 = self._f32(x_tm1, (M, T, D)); cond = self._f32(cond, (M, COND))
        out = torch.empty(M, dtype=torch.float32, device=self.device)
        ws, wsn = self._workspace(M)
        with torch.cuda.device(self.device):
            self._check(self.lib.cld_log_prob(self._h, _ptr(x_t), _ptr(x_tm1), _ptr(cond), int(t_idx), _ptr(out), M,
                                              ws, wsn, self._stream()), "cld_log_prob")
        return out

    def lstm_decode(self, z, cond):
        z = self._f32(z)
        B = z.shape[0]
        z = self._f32(z, (B, T, D)); cond = self._f32(cond, (B, COND))
        act = torch.empty(B, T, 2, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self.lib.cld_lstm_decode(self._h, _ptr(z), _ptr(cond), _ptr(act), B, self._stream()),
                        "cld_lstm_decode")
        return act

    def action_to_state(self, act, curr_states, scaled_input=True, descaled_output=False):
        act = self._f32(act)
        B = act.shape[0]
        act = self._f32(act, (B, T, 2)); cs = self._f32(curr_states, (B, 4))
        traj = torch.empty(B, T, 6, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self.lib.cld_action_to_state(self._h, _ptr(act), _ptr(cs), _ptr(traj), B, int(scaled_input),
                                                     int(descaled_output), self._stream()), "cld_action_to_state")
        return traj

    def decode(self, z, cond, curr_states, descaled_output=True, want_act=False):
        z = self._f32(z)
        B = z.shape[0]
        z = self._f32(z, (B, T, D)); cond = self._f32(cond, (B, COND)); cs = self._f32(curr_states, (B, 4))
        traj = torch.empty(B, T, 6, dtype=torch.float32, device=self.device)
        act = torch.empty(B, T, 2, dtype=torch.float32, device=self.device) if want_act else None
        with torch.cuda.device(self.device):
            self._check(self.lib.cld_decode(self._h, _ptr(z), _ptr(cond), _ptr(cs), _ptr(traj), _ptr(act), B,
                                            int(descaled_output), self._stream()), "cld_decode")
        return (traj, act) if want_act else traj

    def traj2z(self, x6_scaled, cond, noise=None):
        """LSTMVAE.traj2z: -> (z, mu, logvar), each [B,52,4]."""
        x = self._f32(x6_scaled)
        B = x.shape[0]
        x = self._f32(x, (B, T, 6)); cond = self._f32(cond, (B, COND))
        noise = None if noise is None else self._f32(noise, (B, T, D))
        z, mu, lv = (torch.empty(B, T, D, dtype=torch.float32, device=self.device) for _ in range(3))
        with torch.cuda.device(self.device):
            self._check(self.lib.cld_traj2z(self._h, _ptr(x), _ptr(cond), _ptr(noise), _ptr(z), _ptr(mu), _ptr(lv), B,
                                            self._stream()), "cld_traj2z")
        return z, mu, lv

    def vae_loss(self, x6_scaled, act_out, mu, logvar, beta: float):
        """VaeModel.compute_vae_loss (vae_model.py:89-99), forward only -> tensor [3] = (loss, recon, kld)."""
        x = self._f32(x6_scaled)
        B = x.shape[0]
        x = self._f32(x, (B, T, 6)); a = self._f32(act_out, (B, T, 2)); m = self._f32(mu, (B, T, D)); l = self._f32(logvar, (B, T, D))
        out = torch.empty(3, dtype=torch.float32, device=self.device)
        ws, wsn = self._workspace(B)
        with torch.cuda.device(self.device):
            self._check(self.lib.cld_vae_loss(self._h, _ptr(x), _ptr(a), _ptr(m), _ptr(l), C.c_float(beta), _ptr(out), B, ws, wsn,
                                              self._stream()), "cld_vae_loss")
        return out

    def state_to_state_and_action(self, positions, yaws, curr_speed, scaled_output=False):
        p = self._f32(positions)
        B = p.shape[0]
        p = self._f32(p, (B, T, 2)); y = self._f32(yaws, (B, T, 1)); v = self._f32(curr_speed, (B,))
        out = torch.empty(B, T, 6, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self.lib.cld_state_to_state_and_action(self._h, _ptr(p), _ptr(y), _ptr(v), _ptr(out), B,
                                                               int(scaled_output), self._stream()),
                        "cld_state_to_state_and_action")
        return out

    def context_encode(self, image, curr_states, want_map_feat=False):
        """ContextEncoder.forward (models/context_utils.py:40-61): image [B,34,224,224] NCHW, curr_states [B,4]
        -> cond_feat [B,256] (and the resnet18 fc output [B,256] when `want_map_feat`)."""
        image = self._f32(image)
        B = image.shape[0]
        image = self._f32(image, (B, 34, 224, 224)); cs = self._f32(curr_states, (B, 4))
        cond = torch.empty(B, COND, dtype=torch.float32, device=self.device)
        mf = torch.empty(B, 256, dtype=torch.float32, device=self.device) if want_map_feat else None
        ws, wsn = self._scratch("_ctx_ws", int(self.lib.cld_context_workspace_bytes(self._h, B)))
        with torch.cuda.device(self.device):
            self._check(self.lib.cld_context_encode(self._h, _ptr(image), _ptr(cs), _ptr(cond), _ptr(mf), B,
                                                    ws, wsn, self._stream()), "cld_context_encode")
        return (cond, mf) if want_map_feat else cond

    def non_cond_feat(self, curr_states, cond_fill_value: float = -1.0):
        """Unconditional features of classifier-free guidance (upstream diffuser.py:390-411,459-471): the combine MLP on
        [state features | map features of a raster filled with `cond_fill_value`].  The filled raster is the same for every
        agent, so its map feature is computed once per fill value and broadcast."""
        cs = self._f32(curr_states)
        B = cs.shape[0]
        cs = self._f32(cs, (B, 4))
        key = float(cond_fill_value)
        if key not in self._nc_map_feat:
            img = torch.full((1, 34, 224, 224), key, dtype=torch.float32, device=self.device)
            _, mf = self.context_encode(img, torch.zeros(1, 4, device=self.device), want_map_feat=True)
            self._nc_map_feat[key] = mf
        out = torch.empty(B, COND, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self.lib.cld_context_combine(self._h, _ptr(self._nc_map_feat[key]), 1, _ptr(cs), _ptr(out), B, self._stream()),
                        "cld_context_combine")
        return out

    def compute_reward(self, traj, traj_scaled, raster_from_agent, drivable_map, other_pos=None, other_avail=None,
                       collision_thresh: float = 0.8):
        """models/rl/criticmodel.py:7-64 per agent -> (reward, offroad, collision), each [B]."""
        traj = self._f32(traj)
        B = traj.shape[0]
        traj = self._f32(traj, (B, T, 6))
        ts = None if traj_scaled is None else self._f32(traj_scaled, (B, T, 6))
        R = self._f32(raster_from_agent, (B, 3, 3))
        dm = torch.as_tensor(drivable_map).to(self.device).ne(0).to(torch.uint8).contiguous()
        H, W = int(dm.shape[-2]), int(dm.shape[-1])
        S = To = 0
        op = oa = None
        if other_pos is not None and torch.as_tensor(other_pos).numel() > 0:
            op = self._f32(other_pos)
            S, To = int(op.shape[1]), int(op.shape[2])
            oa = torch.as_tensor(other_avail).to(self.device).ne(0).to(torch.uint8).contiguous()
        r, o, c = (torch.empty(B, dtype=torch.float32, device=self.device) for _ in range(3))
        with torch.cuda.device(self.device):
            self._check(self.lib.cld_compute_reward(self._h, _ptr(traj), _ptr(ts), _ptr(R), _ptr(dm), H, W, _ptr(op), _ptr(oa), S, To,
                                                    C.c_float(collision_thresh), _ptr(r), _ptr(o), _ptr(c), B, self._stream()),
                        "cld_compute_reward")
        return r, o, c

    def failure_rate_compute(self, state_action, batch: Mapping):
        """models/rl/criticmodel.py:114-145: {'offroad_failure_rate', 'collision_failure_rate', 'overall_failure_rate'} from the
        per-agent offroad / collision terms of `compute_reward` (an agent fails if it leaves the drivable area at any step,
        respectively comes within 0.8 m of another agent); same batch keys as the reference."""
        _, off, col = self.compute_reward(state_action, None, batch["raster_from_agent"], batch["drivable_map"],
                                          batch.get("all_other_agents_future_positions"),
                                          batch.get("all_other_agents_future_availability"))
        o = float((off < 0).float().mean())
        c = float((col < 0).float().mean())
        return {"offroad_failure_rate": o, "collision_failure_rate": c, "overall_failure_rate": (o + c) / 2.0}

    def world_step(self, traj, centroid, yaw, k: int):
        """env_trajdata.py:452-468 for plan step k -> (world [B,3] = (x, y, h), next curr_states [B,4])."""
        traj = self._f32(traj)
        B = traj.shape[0]
        traj = self._f32(traj, (B, T, 6)); centroid = self._f32(centroid, (B, 2)); yaw = self._f32(yaw, (B,))
        world = torch.empty(B, 3, dtype=torch.float32, device=self.device)
        ncs = torch.empty(B, 4, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self.lib.cld_world_step(self._h, _ptr(traj), _ptr(centroid), _ptr(yaw), int(k), _ptr(world),
                                                _ptr(ncs), B, self._stream()), "cld_world_step")
        return world, ncs

    def rasterize(self, hist_world, hist_avail, scene_start, maps=None, scene_map=None, map_from_world=None, row0: int = 0,
                  B: Optional[int] = None, height: int = 224, width: int = 224, px_per_m: float = 2.0, ego_center=(-0.5, 0.0),
                  no_map_fill: float = -1.0, max_neighbor_dist: float = 30.0, n_sem: int = 3, out=None, want_drivable: bool = True,
                  want_raster_from_world: bool = True):
        """The observation raster of rows [row0, row0 + B) of a scene set (cld_rasterize; include/cld.h for the definition):
        hist_world [B_all,T,3] world (x, y, yaw), oldest first, frame T - 1 = now; hist_avail [B_all,T]; scene_start [num_scenes + 1]
        (int32, the device-side convention of agent_collision); maps [num_maps,n_sem,map_h,map_w] with scene_map [num_scenes] (< 0: no
        map) and map_from_world [num_maps,3,3], or None.  Tensors already on the device in the right type are read in place.
        -> (image [B,T+n_sem,H,W], drivable_map [B,H,W] uint8 | None, raster_from_world [B,3,3] | None); `out`: an image buffer to
        reuse (its first B rows are written and returned)."""
        hw = self._f32(hist_world)
        if hw.dim() != 3 or hw.shape[2] != 3:
            raise CldError(f"rasterize: hist_world must be [B_all,T,3], got {tuple(hw.shape)}")
        B_all, Th = int(hw.shape[0]), int(hw.shape[1])
        av = torch.as_tensor(hist_avail)
        if not (av.dtype == torch.uint8 and av.device == self.device):
            av = (av != 0).to(self.device, torch.uint8)
        av = av.contiguous()
        if tuple(av.shape) != (B_all, Th):
            raise CldError(f"rasterize: hist_avail must be [{B_all},{Th}], got {tuple(av.shape)}")
        ss = torch.as_tensor(scene_start).to(self.device, torch.int32).contiguous()
        if ss.dim() != 1 or ss.numel() < 2:
            raise CldError("rasterize: scene_start must be [num_scenes + 1]")
        S = int(ss.numel()) - 1
        B = B_all - int(row0) if B is None else int(B)
        mp = sm = mfw = None
        num_maps = map_h = map_w = 0
        if maps is not None:
            mp = self._f32(maps)
            if mp.dim() != 4 or mp.shape[1] != n_sem:
                raise CldError(f"rasterize: maps must be [num_maps,{n_sem},map_h,map_w], got {tuple(mp.shape)}")
            num_maps, map_h, map_w = int(mp.shape[0]), int(mp.shape[2]), int(mp.shape[3])
            if scene_map is None or map_from_world is None:
                raise CldError("rasterize: maps need scene_map and map_from_world")
            sm = torch.as_tensor(scene_map).to(self.device, torch.int32).contiguous()
            if tuple(sm.shape) != (S,):
                raise CldError(f"rasterize: scene_map must be [{S}], got {tuple(sm.shape)}")
            mfw = self._f32(map_from_world, (num_maps, 3, 3))
        C_ = Th + int(n_sem)
        if out is None:
            image = torch.empty(max(B, 0), C_, int(height), int(width), dtype=torch.float32, device=self.device)
        else:
            if not (out.dtype == torch.float32 and out.device == self.device and out.is_contiguous() and out.dim() == 4
                    and out.shape[0] >= B and tuple(out.shape[1:]) == (C_, int(height), int(width))):
                raise CldError(f"rasterize: out must be a contiguous float32 [>= {B},{C_},{height},{width}] on {self.device}")
            image = out[:B]
        drv = torch.empty(max(B, 0), int(height), int(width), dtype=torch.uint8, device=self.device) if want_drivable else None
        rfw = torch.empty(max(B, 0), 3, 3, dtype=torch.float32, device=self.device) if want_raster_from_world else None
        dp = lambda t: None if t is None else t.data_ptr()
        rs = _lib.CldRaster(hw.data_ptr(), av.data_ptr(), ss.data_ptr(), dp(mp), dp(sm), dp(mfw), S, B_all, Th, int(n_sem),
                            int(height), int(width), num_maps, map_h, map_w, float(px_per_m),
                            (C.c_float * 2)(float(ego_center[0]), float(ego_center[1])), float(no_map_fill), float(max_neighbor_dist))
        with torch.cuda.device(self.device):
            self._check(self.lib.cld_rasterize(self._h, C.byref(rs), int(row0), B, _ptr(image), _ptr(drv), _ptr(rfw), self._stream()),
                        "cld_rasterize")
        return image, drv, rfw

    # ------------------------------------------------------------------ closed-loop episode metrics
    def scene_metrics_setup(self, scene_start, extent, maps=None, scene_map=None, map_from_world=None, drivable_layer: int = 0,
                            sim_dt: float = 0.1, stat_dt: float = 0.5, height: int = 224, width: int = 224, px_per_m: float = 2.0,
                            ego_center=(-0.5, 0.0), no_map_fill: float = -1.0, n_sem: int = 3):
        """The `cld_scene_metrics` struct of a scene set (include/cld.h) -> (struct, B_all, num_scenes, the tensors it points to).
        scene_start is checked here to split the agents into scenes -- the library cannot read it without a synchronisation and never
        validates its contents; an int32 tensor already on the device is copied to the host once for the check -- everything else is
        checked by the library."""
        ext = self._f32(extent)
        if ext.dim() != 2 or ext.shape[1] != 3:
            raise CldError(f"scene metrics: extent must be [B_all,3], got {tuple(ext.shape)}")
        B_all = int(ext.shape[0])
        host = torch.as_tensor(scene_start).to(torch.int64).reshape(-1).cpu()
        if host.numel() < 2 or int(host[0]) != 0 or int(host[-1]) != B_all or bool((host[1:] <= host[:-1]).any()):
            raise CldError(f"scene metrics: scene_start {host.tolist()} does not split the {B_all} agents into scenes")
        ss = host.to(self.device, torch.int32).contiguous()
        S = int(ss.numel()) - 1
        mp = sm = mfw = None
        num_maps = map_h = map_w = 0
        if maps is not None:
            mp = self._f32(maps)
            if mp.dim() != 4 or mp.shape[1] != n_sem:
                raise CldError(f"scene metrics: maps must be [num_maps,{n_sem},map_h,map_w], got {tuple(mp.shape)}")
            num_maps, map_h, map_w = int(mp.shape[0]), int(mp.shape[2]), int(mp.shape[3])
            if scene_map is None or map_from_world is None:
                raise CldError("scene metrics: maps need scene_map and map_from_world")
            sm = torch.as_tensor(scene_map).to(self.device, torch.int32).contiguous()
            if tuple(sm.shape) != (S,):
                raise CldError(f"scene metrics: scene_map must be [{S}], got {tuple(sm.shape)}")
            mfw = self._f32(map_from_world, (num_maps, 3, 3))
        dp = lambda t: None if t is None else t.data_ptr()
        st = _lib.CldSceneMetrics(ext.data_ptr(), ss.data_ptr(), dp(mp), dp(sm), dp(mfw), float(sim_dt), float(stat_dt), S, B_all,
                                  int(n_sem), int(height), int(width), num_maps, map_h, map_w, int(drivable_layer), float(px_per_m),
                                  (C.c_float * 2)(float(ego_center[0]), float(ego_center[1])), float(no_map_fill))
        return st, B_all, S, (ext, ss, mp, sm, mfw)

    def scene_metrics_state(self, B_all: int):
        """An empty accumulator buffer for B_all agents (cld_scene_metrics_state_bytes; all-zero = empty)."""
        return torch.zeros(int(self.lib.cld_scene_metrics_state_bytes(int(B_all))), dtype=torch.uint8, device=self.device)

    def _metrics_state(self, setup, state):
        need = int(self.lib.cld_scene_metrics_state_bytes(setup[1]))
        if not (isinstance(state, torch.Tensor) and state.device == self.device and state.dtype == torch.uint8 and state.is_contiguous()
                and state.numel() == need):
            raise CldError(f"scene metrics: state must be a contiguous uint8 tensor of {need} bytes on {self.device} (scene_metrics_state)")
        return state

    def scene_metrics_step(self, setup, world, state, step: int, want_flags: bool = False):
        """One environment step of the episode metrics (cld_scene_metrics_step): world [B_all,3] -> `state` updated in place; with
        want_flags -> (flags [B_all,4] uint8, partner [B_all] int32).  No host synchronisation."""
        st, B_all = setup[0], setup[1]
        state = self._metrics_state(setup, state)
        world = self._f32(world, (B_all, 3))
        flags = torch.empty(B_all, 4, dtype=torch.uint8, device=self.device) if want_flags else None
        partner = torch.empty(B_all, dtype=torch.int32, device=self.device) if want_flags else None
        with torch.cuda.device(self.device):
            self._check(self.lib.cld_scene_metrics_step(self._h, C.byref(st), _ptr(world), _ptr(state), _ptr(flags), _ptr(partner),
                                                        int(step), self._stream()), "cld_scene_metrics_step")
        return (flags, partner) if want_flags else None

    def scene_metrics_read(self, setup, state):
        """cld_scene_metrics_read -> (per_agent [B_all,16], per_scene [num_scenes,16]); columns: include/cld.h."""
        st, B_all, S = setup[0], setup[1], setup[2]
        state = self._metrics_state(setup, state)
        per_agent = torch.empty(B_all, len(_lib.METRICS_AGENT_COLS), dtype=torch.float32, device=self.device)
        per_scene = torch.empty(S, _lib.METRICS_SCENE_COLS, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self.lib.cld_scene_metrics_read(self._h, C.byref(st), _ptr(state), _ptr(per_agent), _ptr(per_scene),
                                                        self._stream()), "cld_scene_metrics_read")
        return per_agent, per_scene

    # ------------------------------------------------------------------ guidance satisfaction metrics (guidance_metrics.py)
    def guide_metrics_setup(self, scene_start, extent, entries, maps=None, scene_map=None, map_from_world=None, drivable_layer: int = 0,
                            height: int = 224, width: int = 224, px_per_m: float = 2.0, ego_center=(-0.5, 0.0),
                            no_map_fill: float = -1.0, n_sem: int = 3):
        """The `cld_guide_metrics` struct of a scene set and an entry table (include/cld.h) -> (struct, B_all, num_scenes, num_entries,
        num_members, the tensors it points to).  `entries`: one dict per metric object with `kind` (a name of _lib.GUIDE_METRIC_KINDS or
        its number), `scene`, `members` (batch rows), optionally `excluded` (batch rows; sorted here) and `params` (floats, the layout of
        include/cld.h).  The table is checked here on the host -- the library never validates the contents of device memory -- and
        laid out as flat device arrays once; the scene set is checked as `scene_metrics_setup` checks it."""
        base, B_all, S, keep = self.scene_metrics_setup(scene_start, extent, maps, scene_map, map_from_world, drivable_layer=drivable_layer,
                                                        height=height, width=width, px_per_m=px_per_m, ego_center=ego_center,
                                                        no_map_fill=no_map_fill, n_sem=n_sem)
        entries = list(entries)
        if not entries:
            raise CldError("guide metrics: no entry (every scene's guidance list is empty)")
        kinds, scenes, members, excluded, params = [], [], [], [], []
        ms, xs, ps = [0], [0], [0]
        for n, ent in enumerate(entries):
            kind = ent["kind"]
            kind = _lib.GUIDE_METRIC_KINDS.get(kind, kind) if isinstance(kind, str) else int(kind)
            if kind not in _lib.GUIDE_METRIC_KINDS.values():
                raise CldError(f"guide metrics: entry {n} has unknown kind {ent['kind']!r} (one of {sorted(_lib.GUIDE_METRIC_KINDS)})")
            sc = int(ent["scene"])
            mem = [int(r) for r in ent["members"]]
            exc = sorted(int(r) for r in (ent.get("excluded") or ()))
            if not 0 <= sc < S:
                raise CldError(f"guide metrics: entry {n} scores scene {sc}, there are {S}")
            if not mem or min(mem + exc) < 0 or max(mem + exc) >= B_all:
                raise CldError(f"guide metrics: entry {n} needs at least one member, and rows within [0, {B_all})")
            kinds.append(kind); scenes.append(sc)
            members += mem; excluded += exc; params += [float(v) for v in (ent.get("params") or ())]
            ms.append(len(members)); xs.append(len(excluded)); ps.append(len(params))
        i32 = lambda v: torch.tensor(v, dtype=torch.int32).to(self.device)
        t = dict(kind=i32(kinds), scene=i32(scenes), ms=i32(ms), members=i32(members), xs=i32(xs), ps=i32(ps),
                 excluded=i32(excluded) if excluded else None,
                 params=torch.tensor(params, dtype=torch.float64).to(self.device) if params else None)
        dp = lambda x: None if x is None else x.data_ptr()
        st = _lib.CldGuideMetrics(base.extent, base.scene_start, base.maps, base.scene_map, base.map_from_world, dp(t["kind"]),
                                  dp(t["scene"]), dp(t["ms"]), dp(t["members"]), dp(t["xs"]), dp(t["excluded"]), dp(t["ps"]),
                                  dp(t["params"]), len(kinds), len(members), len(excluded), len(params), S, B_all, base.n_sem,
                                  base.height, base.width, base.num_maps, base.map_h, base.map_w, base.drivable_layer, base.px_per_m,
                                  base.ego_center, base.no_map_fill)
        return st, B_all, S, len(kinds), len(members), (keep, t)

    def guide_metrics_state(self, setup):
        """An empty state buffer for the entry table of `setup` (cld_guide_metrics_state_bytes; all-zero = empty)."""
        return torch.zeros(int(self.lib.cld_guide_metrics_state_bytes(setup[3], setup[4])), dtype=torch.uint8, device=self.device)

    def _guide_metrics_state(self, setup, state):
        need = int(self.lib.cld_guide_metrics_state_bytes(setup[3], setup[4]))
        if not (isinstance(state, torch.Tensor) and state.device == self.device and state.dtype == torch.uint8 and state.is_contiguous()
                and state.numel() == need):
            raise CldError(f"guide metrics: state must be a contiguous uint8 tensor of {need} bytes on {self.device} (guide_metrics_state)")
        return state

    def guide_metrics_step(self, setup, world, speed, acc, state, global_t: int):
        """One environment step of the guidance metrics (cld_guide_metrics_step): world [B_all,3], speed [B_all], acc [B_all] -> `state`
        updated in place.  One launch, no host synchronisation."""
        st, B_all = setup[0], setup[1]
        state = self._guide_metrics_state(setup, state)
        world, speed, acc = self._f32(world, (B_all, 3)), self._f32(speed, (B_all,)), self._f32(acc, (B_all,))
        with torch.cuda.device(self.device):
            self._check(self.lib.cld_guide_metrics_step(self._h, C.byref(st), _ptr(world), _ptr(speed), _ptr(acc), _ptr(state),
                                                        int(global_t), self._stream()), "cld_guide_metrics_step")

    def guide_metrics_read(self, setup, state):
        """cld_guide_metrics_read -> (per_entry [num_entries], per_member [num_members]) float64; include/cld.h defines them."""
        st, E, M = setup[0], setup[3], setup[4]
        state = self._guide_metrics_state(setup, state)
        per_entry = torch.empty(E, dtype=torch.float64, device=self.device)
        per_member = torch.empty(M, dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self.lib.cld_guide_metrics_read(self._h, C.byref(st), _ptr(state), _ptr(per_entry), _ptr(per_member),
                                                        self._stream()), "cld_guide_metrics_read")
        return per_entry, per_member

    # ------------------------------------------------------------------ occupancy coverage and diversity (env_metrics.py:977-1218)
    def occupancy_setup(self, scene_start, window, offset, step=(2.0, 2.0), sigma: float = 1.0, kernel_cut: float = 0.1, maps=None,
                        scene_map=None, map_from_world=None, drivable_layer: int = 0, no_map_fill: float = -1.0, n_sem: int = 3):
        """The `cld_occupancy` struct of one grid over a scene set (include/cld.h) -> (struct, B_all, num_scenes, cells, half-width N, the
        tensors it points to).  window [num_scenes,4] = (ix0, iy0, nx, ny) in cells.  scene_start and the windows are checked here on the
        host -- the library never validates the contents of device memory -- and cell_start is derived from the windows; everything else
        is checked by the library."""
        host = torch.as_tensor(scene_start).to(torch.int64).reshape(-1).cpu()
        if host.numel() < 2 or int(host[0]) != 0 or bool((host[1:] <= host[:-1]).any()) or int(host[-1]) >= 2 ** 31:
            raise CldError(f"occupancy: scene_start {host.tolist()} does not split agents into scenes")
        B_all, S = int(host[-1]), int(host.numel()) - 1
        ss = host.to(self.device, torch.int32).contiguous()
        win = torch.as_tensor(window).to(torch.int64).cpu()
        if tuple(win.shape) != (S, 4):
            raise CldError(f"occupancy: window must be [{S},4] (ix0, iy0, nx, ny), got {tuple(win.shape)}")
        if bool((win[:, 2:] < 1).any()) or bool((win.abs() >= 2 ** 30).any()):
            raise CldError("occupancy: a window needs nx, ny >= 1 and cell indices below 2^30")
        cs = torch.zeros(S + 1, dtype=torch.int64)
        cs[1:] = torch.cumsum(win[:, 2] * win[:, 3], 0)
        cells = int(cs[-1])
        if cells >= 2 ** 31:
            raise CldError(f"occupancy: the windows hold {cells} cells (fewer than 2^31)")
        try:
            N = int(math.ceil(math.sqrt(-2.0 * float(sigma) * math.log(float(kernel_cut))) / float(step[0]))) + 1
        except (ValueError, ZeroDivisionError, OverflowError):
            N = 1                                                    # (the library names what is wrong with sigma, step or kernel_cut)
        mp = sm = mfw = None
        num_maps = map_h = map_w = 0
        if maps is not None:
            mp = self._f32(maps)
            if mp.dim() != 4 or mp.shape[1] != n_sem:
                raise CldError(f"occupancy: maps must be [num_maps,{n_sem},map_h,map_w], got {tuple(mp.shape)}")
            num_maps, map_h, map_w = int(mp.shape[0]), int(mp.shape[2]), int(mp.shape[3])
            if scene_map is None or map_from_world is None:
                raise CldError("occupancy: maps need scene_map and map_from_world")
            sm = torch.as_tensor(scene_map).to(self.device, torch.int32).contiguous()
            if tuple(sm.shape) != (S,):
                raise CldError(f"occupancy: scene_map must be [{S}], got {tuple(sm.shape)}")
            mfw = self._f32(map_from_world, (num_maps, 3, 3))
        wd, cd = win.to(self.device, torch.int32).contiguous(), cs.to(self.device).contiguous()
        dp = lambda t: None if t is None else t.data_ptr()
        st = _lib.CldOccupancy(ss.data_ptr(), wd.data_ptr(), cd.data_ptr(), dp(mp), dp(sm), dp(mfw), cells,
                               (C.c_double * 2)(float(offset[0]), float(offset[1])), (C.c_double * 2)(float(step[0]), float(step[1])),
                               float(sigma), float(kernel_cut), S, B_all, int(n_sem), num_maps, map_h, map_w, int(drivable_layer),
                               float(no_map_fill))
        return st, B_all, S, cells, N, (ss, wd, cd, mp, sm, mfw, win, cs)

    def _occupancy_plane(self, setup, t, dtype, what: str, count=None):
        count = setup[3] if count is None else count
        if not (isinstance(t, torch.Tensor) and t.device == self.device and t.dtype == dtype and t.is_contiguous() and t.numel() == count):
            raise CldError(f"occupancy: {what} must be a contiguous {dtype} tensor of {count} elements on {self.device}")
        return t

    def occupancy_splat(self, setup, world, grid, dropped):
        """One environment step (cld_occupancy_splat): world [B_all,3] added to the Q40 plane `grid` [cells] (int64 tensor holding the
        unsigned words) and to `dropped` [num_scenes] (int64), both in place.  No host synchronisation."""
        world = self._f32(world, (setup[1], 3))
        grid = self._occupancy_plane(setup, grid, torch.int64, "grid")
        dropped = self._occupancy_plane(setup, dropped, torch.int64, "dropped", setup[2])
        with torch.cuda.device(self.device):
            self._check(self.lib.cld_occupancy_splat(self._h, C.byref(setup[0]), _ptr(world), _ptr(grid), _ptr(dropped), self._stream()),
                        "cld_occupancy_splat")

    def occupancy_mark(self, setup, world, ok, success):
        """cld_occupancy_mark: world [n_steps,B_all,3], the poses of one episode; ok [B_all] (non-zero: the agent did not fail);
        success [cells] uint8, set to 1 in place on every window cell of an ok agent."""
        world = self._f32(world)
        if world.dim() != 3 or tuple(world.shape[1:]) != (setup[1], 3) or world.shape[0] < 1:
            raise CldError(f"occupancy: mark needs world [n_steps >= 1,{setup[1]},3], got {tuple(world.shape)}")
        ok = torch.as_tensor(ok)
        ok = ok if (ok.dtype == torch.uint8 and ok.device == self.device) else (ok != 0).to(self.device, torch.uint8)
        ok = self._occupancy_plane(setup, ok.contiguous(), torch.uint8, "ok", setup[1])
        success = self._occupancy_plane(setup, success, torch.uint8, "success")
        with torch.cuda.device(self.device):
            self._check(self.lib.cld_occupancy_mark(self._h, C.byref(setup[0]), _ptr(world), int(world.shape[0]), _ptr(ok), _ptr(success),
                                                    self._stream()), "cld_occupancy_mark")

    def occupancy_read(self, setup, grid, success=None, threshold: float = 1e-2, counts: bool = True, values: bool = False,
                       lane: bool = False, mass: bool = False):
        """cld_occupancy_read -> dict of the outputs asked for: counts [num_scenes,3] int64 (total, onroad, success), values [cells]
        float64, lane [cells] uint8, mass [num_scenes] int64 (the Q40 sum of the on-road cells).  No host synchronisation."""
        S, cells = setup[2], setup[3]
        grid = self._occupancy_plane(setup, grid, torch.int64, "grid")
        if success is not None:
            success = self._occupancy_plane(setup, success, torch.uint8, "success")
        out = {}
        if counts:
            out["counts"] = torch.empty(S, 3, dtype=torch.int64, device=self.device)
        if values:
            out["values"] = torch.empty(cells, dtype=torch.float64, device=self.device)
        if lane:
            out["lane"] = torch.empty(cells, dtype=torch.uint8, device=self.device)
        if mass:
            out["mass"] = torch.empty(S, dtype=torch.int64, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self.lib.cld_occupancy_read(self._h, C.byref(setup[0]), _ptr(grid), _ptr(success), float(threshold),
                                                    _ptr(out.get("counts")), _ptr(out.get("values")), _ptr(out.get("lane")),
                                                    _ptr(out.get("mass")), self._stream()), "cld_occupancy_read")
        return out

    # ------------------------------------------------------------------ realism deviation (guide_dm_trainer.py:204-295)
    def _flat_f32(self, t, what: str) -> torch.Tensor:
        t = self._f32(t).reshape(-1)
        if t.numel() < 1:
            raise CldError(f"{what}: needs at least one value")
        return t

    def sort(self, values, out: Optional[torch.Tensor] = None):
        """The values ascending in numpy's order (NaN last; cld_sort_f32), flattened.  `out`: a contiguous fp32 device tensor of the same
        count to write to; it may be `values` itself (in place).  No host synchronisation."""
        x = self._flat_f32(values, "sort")
        n = x.numel()
        if out is None:
            out = torch.empty_like(x)
        elif not (isinstance(out, torch.Tensor) and out.device == self.device and out.dtype == torch.float32 and out.is_contiguous()
                  and out.numel() == n):
            raise CldError(f"sort: out must be a contiguous fp32 tensor of {n} values on {self.device}")
        ws, wsn = self._scratch("_rws", int(self.lib.cld_sort_workspace_bytes(n)))
        with torch.cuda.device(self.device):
            self._check(self.lib.cld_sort_f32(self._h, _ptr(x), _ptr(out), n, ws, wsn, self._stream()), "cld_sort_f32")
        return out.reshape(-1)

    def wasserstein_distance(self, u, v, presorted: bool = False):
        """scipy.stats.wasserstein_distance(u, v) of two fp32 samples (cld_wasserstein_f32) -> a 0-d float64 device tensor.  With
        `presorted` both are taken as ascending already (Engine.sort's or np.sort's order).  No host synchronisation."""
        u, v = self._flat_f32(u, "wasserstein_distance"), self._flat_f32(v, "wasserstein_distance")
        if not presorted:
            u, v = self.sort(u), self.sort(v)
        out = torch.empty((), dtype=torch.float64, device=self.device)
        ws, wsn = self._scratch("_rws", int(self.lib.cld_wasserstein_workspace_bytes(u.numel(), v.numel())))
        with torch.cuda.device(self.device):
            self._check(self.lib.cld_wasserstein_f32(self._h, _ptr(u), u.numel(), _ptr(v), v.numel(), _ptr(out), ws, wsn, self._stream()),
                        "cld_wasserstein_f32")
        return out

    def realism_terms(self, sa, dt: float, out=None):
        """sa [M,T,6] (scaled state and action) -> (long_acc [M T], lat_acc [M T], jerk [M (T-1)]) as test_step forms them
        (cld_realism_terms).  `out`: three contiguous fp32 device tensors (or None: not wanted) of at least those counts to write into."""
        sa = self._f32(sa)
        if sa.dim() != 3 or sa.shape[2] != 6 or sa.shape[0] < 1 or sa.shape[1] < 2:
            raise CldError(f"realism_terms: expected [M >= 1, T >= 2, 6], got {tuple(sa.shape)}")
        M, T = int(sa.shape[0]), int(sa.shape[1])
        counts = (M * T, M * T, M * (T - 1))
        if out is None:
            out = tuple(torch.empty(c, dtype=torch.float32, device=self.device) for c in counts)
        else:
            out = tuple(out)
            if len(out) != 3 or all(o is None for o in out):
                raise CldError("realism_terms: out must be three tensors, at least one of them not None")
            for o, c in zip(out, counts):
                if o is not None and not (isinstance(o, torch.Tensor) and o.device == self.device and o.dtype == torch.float32
                                          and o.is_contiguous() and o.numel() >= c):
                    raise CldError(f"realism_terms: an output must be a contiguous fp32 tensor of at least {c} values on {self.device}")
        with torch.cuda.device(self.device):
            self._check(self.lib.cld_realism_terms(self._h, _ptr(sa), M, T, float(dt), _ptr(out[0]), _ptr(out[1]), _ptr(out[2]),
                                                   self._stream()), "cld_realism_terms")
        return out

    # ------------------------------------------------------------------ open-loop sample metrics (tbsim/utils/metrics.py:201-358)
    def sample_metrics(self, pred, gt, avail, out=None):
        """ADE / FDE and the diversity of N sampled futures per agent (cld_sample_metrics; include/cld_eval.h defines every column).
        pred [B,N,T,2] positions or [B,N,T,C <= 8] with the positions in channels 0 and 1 (the [.,.,52,6] tensor `decode` returns is read
        in place); gt [B,T,2]; avail [B,T], bool or float (converted to fp32).  Confidences are uniform, as upstream passes them.
        -> {"per_agent": [B,10] float64, "index": [B,4] int32 (best_ade, best_fde, last, nonfinite), "means": [10] float64}, device
        tensors in the column order of `_lib.SAMPLE_METRIC_COLS`.  `out`: (per_agent, index) contiguous device tensors of at least B
        rows to write into (float64 [.,10], int32 [.,4]).  N > 256 or N T > 8,192 raises: there is no other path.  No host
        synchronisation."""
        pred = self._f32(pred)
        if pred.dim() != 4 or min(pred.shape) < 1 or not 2 <= pred.shape[3] <= 8:
            raise CldError(f"sample_metrics: pred must be [B,N,T,C] with 2 <= C <= 8, got {tuple(pred.shape)}")
        B, N, T, Cc = (int(v) for v in pred.shape)
        gt = self._f32(gt, (B, T, 2))
        avail = self._f32(avail, (B, T))
        cols = len(_lib.SAMPLE_METRIC_COLS)
        if out is None:
            rows = torch.empty(B, cols, dtype=torch.float64, device=self.device)
            index = torch.empty(B, 4, dtype=torch.int32, device=self.device)
        else:
            rows, index = out
            for o, dt, w in ((rows, torch.float64, cols), (index, torch.int32, 4)):
                if not (isinstance(o, torch.Tensor) and o.device == self.device and o.dtype == dt and o.is_contiguous() and o.dim() == 2
                        and o.shape[1] == w and o.shape[0] >= B):
                    raise CldError(f"sample_metrics: out must be contiguous (float64 [>= {B},{cols}], int32 [>= {B},4]) on {self.device}")
            rows, index = rows[:B], index[:B]
        means = torch.empty(cols, dtype=torch.float64, device=self.device)
        ws, wsn = self._scratch("_rws", int(self.lib.cld_sample_metrics_workspace_bytes(B)))
        with torch.cuda.device(self.device):
            self._check(self.lib.cld_sample_metrics(self._h, _ptr(pred), Cc, _ptr(gt), _ptr(avail), B, N, T, _ptr(rows), _ptr(index),
                                                    _ptr(means), ws, wsn, self._stream()), "cld_sample_metrics")
        return {"per_agent": rows, "index": index, "means": means}

    # ------------------------------------------------------------------ measurement
    def profile_enable(self, on: bool = True):
        self._check(self.lib.cld_profile_enable(self._h, int(on)), "cld_profile_enable")

    def profile_read(self):
        """-> (summed ms, launches, algorithmic FLOP) of the dominant conv kernel since profile_enable(True)."""
        ms, n, fl = C.c_double(), C.c_int64(), C.c_double()
        self._check(self.lib.cld_profile_read(self._h, C.byref(ms), C.byref(n), C.byref(fl)), "cld_profile_read")
        return ms.value, n.value, fl.value

    def profile_read_executed(self):
        """-> (MFMA FLOP executed by the launches profile_read timed, in the form each took; algorithmic FLOP, executed MFMA
        FLOP and launch count of the most recent U-Net evaluation)."""
        ex, ea, ee, nl = C.c_double(), C.c_double(), C.c_double(), C.c_int32()
        self._check(self.lib.cld_profile_read_executed(self._h, C.byref(ex), C.byref(ea), C.byref(ee), C.byref(nl)),
                    "cld_profile_read_executed")
        return ex.value, ea.value, ee.value, nl.value
