"""Host-side mirrors of the reference's model objects over the C-ABI.

  FluxModel      <-> diffusion_rs_core::models::flux::Flux            (model.rs:709-838)
  AutoEncoderKl  <-> diffusion_rs_core::models::vaes::AutoEncoderKl   (autoencoder_kl.rs:52-128)
  FlowMatchEuler <-> pipelines::sampling::Sampler + SchedulerConfig   (sampling.rs, scheduler.rs)

torch is used only as the device-memory / stream plumbing (tensors own the buffers whose raw
pointers cross the C-ABI); every FLOP runs in libflux_mi355x.so.
"""
import ctypes as C
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np
import torch

from . import _lib as L

# fmi_flux_quantize_int8's linear mask (include/flux_mi355x.h: FMI_Q8_*)
Q8_DOUBLE_QKV, Q8_DOUBLE_OUT, Q8_DOUBLE_MLP_IN, Q8_DOUBLE_MLP_OUT, Q8_SINGLE_LINEAR1, Q8_SINGLE_LINEAR2 = 1, 2, 4, 8, 16, 32
INT8_DEFAULT_MASK = Q8_DOUBLE_QKV | Q8_DOUBLE_OUT | Q8_SINGLE_LINEAR1 | Q8_SINGLE_LINEAR2  # FMI_INT8_DEFAULT_MASK

FLUX_DEV = dict(in_channels=64, pooled_projection_dim=768, joint_attention_dim=4096, num_attention_heads=24, num_layers=19,
                num_single_layers=38, guidance_embeds=True, axes_dim=[16, 56, 56], theta=10000)
FLUX_SCHNELL = dict(FLUX_DEV, guidance_embeds=False)
VAE_FLUX = dict(in_channels=3, out_channels=3, block_out_channels=[128, 256, 512, 512], layers_per_block=2, latent_channels=16,
                norm_num_groups=32, mid_block_add_attention=True, use_post_quant_conv=False, scaling_factor=0.3611, shift_factor=0.1159)

_TORCH_DT = {torch.float32: L.F32, torch.float16: L.F16, torch.bfloat16: L.BF16, torch.uint8: L.U8, torch.int8: L.I8}
_NP_DT = {np.dtype(np.float32): L.F32, np.dtype(np.float16): L.F16}


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _tensor_arg(t):
    """(pointer, fmi_dtype, shape, keepalive) for a torch tensor (any device) or numpy array."""
    if isinstance(t, np.ndarray):
        a = np.ascontiguousarray(t)
        if a.dtype not in _NP_DT:
            a = a.astype(np.float32)
        return C.c_void_p(a.ctypes.data), _NP_DT[a.dtype], a.shape, a
    t = t.contiguous()
    return C.c_void_p(t.data_ptr()), _TORCH_DT[t.dtype], tuple(t.shape), t


def _linear_arg(x, dtype, raw=False, views=()):
    """(keepalive, pointer, nbytes) of one array of a quantised Linear, host or device (the C side copies with hipMemcpyDefault), checked to be `dtype`.
    A torch tensor, made contiguous (its values cast for the f32 scales; a dtype in `views` reinterpreted), or a numpy array / sequence converted to the
    dtype; raw: anything with the buffer protocol instead, taken as the bytes it holds."""
    if isinstance(x, torch.Tensor):
        keep = x.to(torch.float32).contiguous() if dtype == torch.float32 else x.contiguous()
        if keep.dtype in views:
            keep = keep.view(dtype)
        assert keep.dtype == dtype
        return keep, C.c_void_p(keep.data_ptr()), keep.numel() * keep.element_size()
    if not raw:
        keep = np.ascontiguousarray(x, {torch.uint8: np.uint8, torch.int8: np.int8, torch.float32: np.float32}[dtype])
    else:
        keep = np.ascontiguousarray(x).view(np.uint8).reshape(-1) if isinstance(x, np.ndarray) else np.frombuffer(x, np.uint8)
    return keep, C.c_void_p(keep.ctypes.data), keep.nbytes


def _as_f32(t):
    return np.asarray(t, np.float32) if isinstance(t, np.ndarray) else t.to(torch.float32)


def _like_img(t, name: str, img):
    """One of denoise's x0 / noise / mask: shaped like img, or ValueError; contiguous f32 on img's device.  None stays None."""
    if t is not None and tuple(t.shape) != tuple(img.shape):
        raise ValueError(f"denoise: {name} is {tuple(t.shape)}, img is {tuple(img.shape)}")
    return None if t is None else t.to(device=img.device, dtype=torch.float32).contiguous()


@dataclass
class SchedulerConfig:
    """pipelines/scheduler.rs:4-20 (public FLUX.1 values as defaults)."""
    base_image_seq_len: int = 256
    base_shift: float = 0.5
    max_image_seq_len: int = 4096
    max_shift: float = 1.15
    shift: float = 3.0
    use_dynamic_shifting: bool = True

    def get_timesteps(self, num_steps: int, mu: Optional[float]) -> List[float]:
        if self.use_dynamic_shifting and mu is None:
            raise ValueError("`mu` is required for dynamic shifting")  # scheduler.rs:34
        c = L.SchedulerConfigC(self.base_image_seq_len, self.base_shift, self.max_image_seq_len, self.max_shift, self.shift,
                               int(self.use_dynamic_shifting))
        out = (C.c_double * (num_steps + 1))()
        L.check(L.load().fmi_get_timesteps(C.byref(c), num_steps, C.c_double(mu or 0.0), out))
        return list(out)

    def calculate_shift(self, image_seq_len: int) -> float:
        return L.load().fmi_calculate_shift(image_seq_len, self.base_image_seq_len, self.max_image_seq_len, self.base_shift, self.max_shift)


# Which options of one call do not combine: the table at fmi_flux_denoise_with (include/flux_mi355x.h), which validate() enforces in the library.  Python states it
# once, here, for FluxModel and for Pipeline; the checks below look at each option's own arguments only.  An option is present when it is given and has passed
# its own check: "context", "control" (the model has conditioning channels), "true_cfg", "cache" (a threshold or a forced mask), "blend" (x0 / noise / mask, which
# combines with everything), "controlnet", "ip_adapter".
REFUSED_PAIRS = (("ip_adapter", "context"), ("ip_adapter", "cache"), ("controlnet", "context"), ("controlnet", "control"), ("controlnet", "cache"),
                 ("control", "context"), ("control", "cache"), ("true_cfg", "cache"))
# ... and the modes of the model an option does not run in (sequence parallelism: the step cache's distance would need an all-reduce over the ranks, the others
# are not wired through it; the 8-bit modes: the adapter reads the bf16 q of the q|k|v projection)
REFUSED_MODES = (("ip_adapter", "sequence_parallel"), ("ip_adapter", "fp8"), ("ip_adapter", "int8"), ("controlnet", "sequence_parallel"),
                 ("control", "sequence_parallel"), ("true_cfg", "sequence_parallel"), ("cache", "sequence_parallel"))
# what FluxModel.forward / denoise call each of them in a message (Pipeline has its own keywords: pipeline.REQUEST_NAMES)
OPTION_NAMES = dict(context="context= (a reference image)", control="control= (a channel-conditioned model: FLUX.1 Fill / Canny / Depth)",
                    true_cfg="true CFG (negative_txt= / negative_y=)", cache="the step cache (cache_threshold= / cache_force=)", controlnet="a ControlNet",
                    ip_adapter="an IP-Adapter", sequence_parallel="supported under sequence parallelism",
                    fp8="supported in the fp8 mode (it reads the bf16 q of the q|k|v projection)",
                    int8="supported in the int8 mode (it reads the bf16 q of the q|k|v projection)")


def check_combination(present, names=OPTION_NAMES):
    """ValueError for the first row of REFUSED_PAIRS, then of REFUSED_MODES, whose two members are both in `present` (any container of the names above; the
    modes are "sequence_parallel", "fp8", "int8").  names: what the calling layer calls each of them."""
    for a, b in REFUSED_PAIRS:
        if a in present and b in present:
            raise ValueError(f"{names[a]} is not combined with {names[b]}")
    for a, mode in REFUSED_MODES:
        if a in present and mode in present:
            raise ValueError(f"{names[a]} is not {names[mode]}")


def check_step_scales(step_scales, n_steps, name: str):
    """An option's per-step scales (`name`: its keyword) as a contiguous float32 array; None stays None.  ValueError unless 1-D, n_steps entries (None: any), finite."""
    if step_scales is None:
        return None
    ss = np.asarray(step_scales, np.float32)
    if ss.ndim != 1 or (n_steps is not None and ss.shape[0] != n_steps):
        raise ValueError(f"{name} must have one entry per step ({n_steps}), got shape {ss.shape}")
    if not np.isfinite(ss).all():
        raise ValueError(f"{name} entries must be finite")
    return np.ascontiguousarray(ss)


def check_step_cache_args(n_steps: int, threshold=None, force=None):
    """The arguments of the first-block step cache (FluxModel.denoise / fmi_flux_denoise_cached), checked without the library.
    Returns (threshold as float, force as an int8 array of n_steps entries or None); (None, None) when neither is given: no cache, the plain loop.
    ValueError: a negative or NaN threshold; `force` not n_steps entries of -1 (decide by threshold) / 0 (compute) / 1 (reuse); force[0] == 1 (step 0 has
    nothing to reuse)."""
    if threshold is None and force is None:
        return None, None
    thr = 0.0 if threshold is None else float(threshold)
    if not thr >= 0.0:
        raise ValueError(f"cache_threshold must be >= 0, got {threshold!r}")
    if force is None:
        return thr, None
    f = np.asarray(force)
    if f.ndim != 1 or f.shape[0] != n_steps:
        raise ValueError(f"cache_force must have one entry per step ({n_steps}), got shape {f.shape}")
    if not np.isin(f, (-1, 0, 1)).all():
        raise ValueError("cache_force entries are -1 (decide by threshold), 0 (compute) or 1 (reuse)")
    if n_steps and f[0] == 1:
        raise ValueError("cache_force[0] == 1: step 0 is always computed (there is nothing to reuse yet)")
    return thr, np.ascontiguousarray(f, dtype=np.int8)


SOLVERS = {"euler": 0, "heun": 1, "dpmpp_2m": 2}  # FMI_SOLVER_*


def check_solver_args(solver, timesteps, cache=False, sequence_parallel=False):
    """The integrator of FluxModel.denoise (fmi_flux_denoise_solver), checked without the library.  Returns the FMI_SOLVER_* kind, or None for
    solver None / "euler": the loop as it always was, which keeps accepting any schedule.  ValueError: a name that is none of SOLVERS; for "heun" / "dpmpp_2m" a
    schedule that is not strictly decreasing inside [0, 1]; "heun" with the step cache (cache: one is present); either of them under sequence parallelism.
    These two refusals are the solver's own, not rows of REFUSED_PAIRS / REFUSED_MODES."""
    if solver is None or solver == "euler":
        return None
    if not isinstance(solver, str) or solver not in SOLVERS:
        raise ValueError(f"solver must be None or one of {sorted(SOLVERS)}, got {solver!r}")
    ts = [float(t) for t in timesteps]
    if len(ts) < 1 or not ts[0] <= 1.0 or not ts[-1] >= 0.0 or not all(b < a for a, b in zip(ts, ts[1:])):
        raise ValueError(f"solver={solver!r} needs a strictly decreasing schedule inside [0, 1] (1 >= timesteps[0], timesteps[-1] >= 0)")
    if sequence_parallel:
        raise ValueError(f"solver={solver!r} is not supported under sequence parallelism")
    if solver == "heun" and cache:
        raise ValueError("solver='heun' is not combined with the step cache (cache_threshold= / cache_force=): its two evaluations per step are at different times")
    return SOLVERS[solver]


def check_true_cfg_args(txt_shape, y_shape, negative_txt_shape=None, negative_y_shape=None, true_cfg_scale=None):
    """The arguments of true classifier-free guidance (FluxModel.denoise / fmi_flux_denoise_cfg), checked without the library: the shapes
    of the prompt's txt (B,T,J) and y (B,P), of the negative's, and the scale.  Returns the scale as a float (1.0 when none is given), or None when no
    negative is given: the plain loop.
    ValueError: one negative without the other; a scale without a negative; shapes — and with them T — that differ from the prompt's; B > 4 (the loop
    evaluates 2 B samples and the per-device limit is 8); a scale that is negative, NaN or infinite."""
    if negative_txt_shape is None and negative_y_shape is None:
        if true_cfg_scale is not None:
            raise ValueError("true_cfg_scale= needs negative_txt= and negative_y=")
        return None
    if negative_txt_shape is None or negative_y_shape is None:
        raise ValueError("negative_txt= and negative_y= go together")
    if tuple(negative_txt_shape) != tuple(txt_shape):
        raise ValueError(f"negative_txt is {tuple(negative_txt_shape)}, txt is {tuple(txt_shape)}: the negative takes the prompt's shape (B,T,J), T included")
    if tuple(negative_y_shape) != tuple(y_shape):
        raise ValueError(f"negative_y is {tuple(negative_y_shape)}, y is {tuple(y_shape)}")
    if int(txt_shape[0]) > 4:
        raise ValueError(f"true CFG evaluates 2 B samples per step and the per-device limit is 8: B = {int(txt_shape[0])} > 4")
    scale = 1.0 if true_cfg_scale is None else float(true_cfg_scale)
    if not (scale >= 0.0 and scale != float("inf")):
        raise ValueError(f"true_cfg_scale must be finite and >= 0, got {true_cfg_scale!r}")
    return scale


def state_channels(cfg: dict) -> int:
    """The width of the state, of the prediction and of proj_out's rows: diffusers' out_channels, which a config without one (or with null) takes from
    in_channels.  cfg["in_channels"] keeps diffusers' meaning, x_embedder's K; the difference is the conditioning channels."""
    return int(cfg.get("out_channels") or cfg["in_channels"])


def check_control_args(cond_channels: int, img_shape, control_shape=None):
    """The control of FluxModel.forward / denoise (fmi_flux_forward_control / fmi_flux_denoise_control), checked without the library.
    ValueError: a channel-conditioned model without control=; control= on a plain model; a control that is not (B,S,cond_channels) for img (B,S,C)."""
    if control_shape is None:
        if cond_channels:
            raise ValueError(f"this model has {cond_channels} conditioning channels: control= (B,S,{cond_channels}) is required")
        return
    if not cond_channels:
        raise ValueError("control= needs a channel-conditioned model (in_channels > out_channels: FLUX.1 Fill / Canny / Depth)")
    if tuple(control_shape) != (int(img_shape[0]), int(img_shape[1]), cond_channels):
        raise ValueError(f"control is {tuple(control_shape)}, expected {(int(img_shape[0]), int(img_shape[1]), cond_channels)} for img {tuple(img_shape)}")


def controlnet_index_map(n_main: int, n_net: int) -> List[int]:
    """Which of a ControlNet's n_net samples each of the main model's n_main blocks takes: i // ceil(n_main / n_net), diffusers' interval_control.
    Empty for n_net == 0 (a net without single blocks injects nothing into the single blocks)."""
    if n_net <= 0:
        return []
    k = -(-n_main // n_net)
    return [i // k for i in range(n_main)]


def controlnet_step_scales(n_steps: int, control_guidance_start: float = 0.0, control_guidance_end: float = 1.0) -> List[float]:
    """diffusers' controlnet_keep over the n_steps actually run: keep_i = 0 if i / n < control_guidance_start or (i + 1) / n > control_guidance_end, else 1."""
    return [0.0 if (i / n_steps < control_guidance_start or (i + 1) / n_steps > control_guidance_end) else 1.0 for i in range(n_steps)]


def check_controlnet_args(cfg: dict, net_cfg=None, img_shape=None, cond_shape=None, scale=1.0, step_scales=None, n_steps=None):
    """The ControlNet of FluxModel.forward / denoise (fmi_flux_forward_controlnet / fmi_flux_denoise_controlnet), checked without the library; cfg is
    the main model's config, net_cfg the ControlNet's (None: no ControlNet).  Returns step_scales as a float32 array of n_steps entries, or None.
    ValueError: controlnet_cond= without controlnet= or the reverse; a net whose width-defining fields differ from the main model's; a cond that is not
    (B,S,in_channels) for img (B,S,C); a scale or step scale that is not finite; step_scales not n_steps entries.  Several ControlNets, union modes and the XLabs
    hint block are out of scope."""
    if net_cfg is None:
        if cond_shape is not None:
            raise ValueError("controlnet_cond= needs controlnet=")
        if step_scales is not None:
            raise ValueError("controlnet_step_scales= needs controlnet=")
        return None
    if cond_shape is None:
        raise ValueError("controlnet= needs controlnet_cond=, the packed latents of the control image (B,S,in_channels)")
    for k in ("num_attention_heads", "joint_attention_dim", "pooled_projection_dim", "axes_dim", "theta", "in_channels"):
        a, b = cfg[k], net_cfg[k]
        if (list(a) != list(b)) if k == "axes_dim" else (a != b):
            raise ValueError(f"the ControlNet's {k} is {b!r}, the main model's {a!r}")
    if tuple(cond_shape) != (int(img_shape[0]), int(img_shape[1]), int(net_cfg["in_channels"])):
        raise ValueError(f"controlnet_cond is {tuple(cond_shape)}, expected {(int(img_shape[0]), int(img_shape[1]), int(net_cfg['in_channels']))} for img {tuple(img_shape)}")
    if not np.isfinite(float(scale)):
        raise ValueError(f"controlnet_scale must be finite, got {scale!r}")
    return check_step_scales(step_scales, n_steps, "controlnet_step_scales")


IP_MAX_TOKENS = 32  # fmi_ip_attention's 1 <= N <= 32


def check_ip_adapter_args(cfg: dict, adapter=None, img_shape=None, embeds_shape=None, negative_embeds_shape=None, scale=1.0, step_scales=None, n_steps=None,
                          has_negative: bool = False):
    """The IP-Adapter of FluxModel.forward / denoise (fmi_flux_forward_ip / fmi_flux_denoise_ip), checked without the library.  cfg is the main model's
    config; adapter is None (no adapter) or a dict(num_heads=, joint_attention_dim=, num_layers=, embed_dim=, num_tokens=) — FluxIPAdapter.dims.  Returns step_scales
    as a float32 array of n_steps entries, or None.  ValueError: embeddings, a scale or step scales without ip_adapter= or an adapter without embeddings; an adapter
    whose width, joint_attention_dim or number of double blocks differ from the model's; embeds that are not (B, embed_dim) for img (B,S,C); negative embeddings of
    another shape or without a negative prompt; a scale or step scale that is not finite; step_scales not n_steps entries."""
    if adapter is None:
        for v, nm in ((embeds_shape, "ip_adapter_image_embeds="), (negative_embeds_shape, "negative_ip_adapter_image_embeds="), (step_scales, "ip_adapter_step_scales=")):
            if v is not None:
                raise ValueError(f"{nm} needs ip_adapter=")
        return None
    if embeds_shape is None:
        raise ValueError("ip_adapter= needs ip_adapter_image_embeds=, the image embeddings (B, embed_dim)")
    for k, mk in (("num_heads", "num_attention_heads"), ("joint_attention_dim", "joint_attention_dim"), ("num_layers", "num_layers")):
        if int(adapter[k]) != int(cfg[mk]):
            raise ValueError(f"the IP-Adapter's {k} is {adapter[k]!r}, the main model's {mk} {cfg[mk]!r}")
    if not 1 <= int(adapter["num_tokens"]) <= IP_MAX_TOKENS:
        raise ValueError(f"the IP-Adapter's num_tokens is {adapter['num_tokens']}: 1 <= N <= {IP_MAX_TOKENS} is supported")
    want = (int(img_shape[0]), int(adapter["embed_dim"]))
    if tuple(embeds_shape) != want:
        raise ValueError(f"ip_adapter_image_embeds is {tuple(embeds_shape)}, expected {want} for img {tuple(img_shape)}")
    if negative_embeds_shape is not None:
        if not has_negative:
            raise ValueError("negative_ip_adapter_image_embeds= needs a negative prompt (negative_txt= / negative_y=)")
        if tuple(negative_embeds_shape) != want:
            raise ValueError(f"negative_ip_adapter_image_embeds is {tuple(negative_embeds_shape)}, expected {want}")
    if not np.isfinite(float(scale)):
        raise ValueError(f"ip_adapter_scale must be finite, got {scale!r}")
    return check_step_scales(step_scales, n_steps, "ip_adapter_step_scales")


class FluxModel:
    def __init__(self, cfg: dict, device: int = 0):
        self.lib = L.load()
        self.cfg = dict(cfg)
        # cfg["in_channels"] is x_embedder's K as in diffusers; the state is out_channels wide and the rest are conditioning channels
        self.state_channels = state_channels(cfg)
        self.cond_channels = int(cfg["in_channels"]) - self.state_channels
        L.check(self.lib.fmi_init(device), self.lib)
        c = L.FluxConfig(self.state_channels, cfg["pooled_projection_dim"], cfg["joint_attention_dim"], cfg["num_attention_heads"],
                         cfg["num_layers"], cfg["num_single_layers"], int(cfg["guidance_embeds"]), (C.c_int * 3)(*cfg["axes_dim"]), cfg["theta"])
        h = C.c_void_p()
        if self.cond_channels:  # (a negative or misaligned difference is the library's FMI_ERR_INVALID)
            L.check(self.lib.fmi_flux_create_cond(C.byref(c), self.cond_channels, L.MODEL_BF16, C.byref(h)), self.lib)
        else:
            L.check(self.lib.fmi_flux_create(C.byref(c), L.MODEL_BF16, C.byref(h)), self.lib)
        self.h = h
        self.hidden = cfg["num_attention_heads"] * 128
        self.device = torch.device("cuda", device)

    def close(self):
        if getattr(self, "h", None):
            self.lib.fmi_flux_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def is_guidance(self) -> bool:  # Flux::is_guidance, model.rs:835-837
        return bool(self.cfg["guidance_embeds"])

    def set_tensor(self, name: str, t):
        p, dt, shape, keep = _tensor_arg(t)
        sh = (C.c_int64 * len(shape))(*shape)
        L.check(self.lib.fmi_flux_set_tensor(self.h, name.encode(), p, dt, sh, len(shape)), self.lib)

    def load_state_dict(self, tensors: dict):
        for k, v in tensors.items():
            self.set_tensor(k, v)
        self.assert_complete()

    def get_tensor(self, name: str, dtype=torch.bfloat16):
        """The current value of a tensor set_tensor accepts (with adapters loaded: the merged weight), as a torch tensor on this model's device.
        dtype bfloat16 (the resident bits) or float32 (the same values)."""
        shapes = self._shapes()
        if name not in shapes:
            raise L.FmiError(f"get_tensor: unknown tensor name '{name}'", code=L.ERR_INVALID)
        shape = shapes[name]
        out = torch.empty(shape, dtype=dtype, device=self.device)
        sh = (C.c_int64 * len(shape))(*shape)
        L.check(self.lib.fmi_flux_get_tensor(self.h, name.encode(), _ptr(out), _TORCH_DT[dtype], sh, len(shape)), self.lib)
        return out

    def _shapes(self):
        if getattr(self, "_shape_cache", None) is None:
            from . import synth
            self._shape_cache = synth.flux_tensor_shapes(self.cfg)
        return self._shape_cache

    # ---- LoRA adapters, merged into the resident weights (include/flux_mi355x.h: fmi_flux_lora_*)
    def lora_add(self, adapter: str, prefix: str, A, B, scale: float = 1.0):
        """One (A (r, in), B (out, r)) pair of `adapter` for the Linear `prefix`; torch tensors (any device) or numpy arrays, F32 / F16 / BF16.
        Takes effect before it returns; a pair the adapter already holds for that Linear is replaced."""
        pa, dta, sa, keep_a = _tensor_arg(A)
        pb, dtb, sb, keep_b = _tensor_arg(B)
        if dta != dtb:
            pa, dta, sa, keep_a = _tensor_arg(_as_f32(A))
            pb, dtb, sb, keep_b = _tensor_arg(_as_f32(B))
        if len(sa) != 2 or len(sb) != 2 or sa[0] != sb[1]:
            raise L.FmiError(f"lora_add: {prefix}: A {tuple(sa)} and B {tuple(sb)} are not (r, in) and (out, r)", code=L.ERR_INVALID)
        want = self._shapes().get(prefix + ".weight")
        if want is not None and len(want) == 2 and sa[0] >= 1 and (sb[0], sa[1]) != tuple(want):
            raise L.FmiError(f"lora_add: {prefix}: B A is {(sb[0], sa[1])}, the Linear is {tuple(want)}", code=L.ERR_INVALID)
        L.check(self.lib.fmi_flux_lora_add(self.h, adapter.encode(), prefix.encode(), pa, pb, dta, int(sa[0]), float(scale)), self.lib)

    def lora_add_term(self, adapter: str, prefix: str, term):
        """One term (lora.AdapterTerm: a plain pair, LoHa, LoKr or DoRA) of `adapter` for the Linear `prefix`; its tensors are torch tensors (any device)
        or numpy arrays, F32 / F16 / BF16 (mixed dtypes are widened to F32).  Takes effect before it returns; a term the adapter already holds for that
        Linear is replaced.  The library validates the shapes against the Linear."""
        kinds = {"lora": L.ADAPTER_LORA, "loha": L.ADAPTER_LOHA, "lokr": L.ADAPTER_LOKR, "dora": L.ADAPTER_DORA}
        kind = kinds.get(term.kind, term.kind)
        if not isinstance(kind, int):
            raise L.FmiError(f"lora_add_term: {prefix}: unknown adapter kind {term.kind!r}", code=L.ERR_INVALID)
        tensors = list(term.tensors)
        args = [None if t is None else _tensor_arg(t) for t in tensors]
        if len({a[1] for a in args if a is not None}) > 1:
            args = [None if t is None else _tensor_arg(_as_f32(t)) for t in tensors]
        factors, mag = args[:4], None
        if kind in (L.ADAPTER_LORA, L.ADAPTER_DORA):  # (A, B[, m])
            factors, mag = args[:2], (args[2] if len(args) > 2 else None)
        ct = L.AdapterTermC(kind=kind, dtype=next((a[1] for a in args if a is not None), L.F32), scale=float(term.scale), row_offset=int(term.row_offset))
        for i, a in enumerate(factors):
            if a is None:
                continue
            if len(a[2]) != 2:
                raise L.FmiError(f"lora_add_term: {prefix}: factor {i} has shape {tuple(a[2])}, not a matrix", code=L.ERR_INVALID)
            ct.factor[i], ct.factor_rows[i], ct.factor_cols[i] = a[0], int(a[2][0]), int(a[2][1])
        if mag is not None:
            want = self._shapes().get(prefix + ".weight")
            n = 1
            for v in mag[2]:
                n *= int(v)
            if want is not None and n != want[0]:
                raise L.FmiError(f"lora_add_term: {prefix}: the magnitude has {n} values, the Linear has {want[0]} rows", code=L.ERR_INVALID)
            ct.magnitude = mag[0]
        L.check(self.lib.fmi_flux_lora_add_term(self.h, adapter.encode(), prefix.encode(), C.byref(ct)), self.lib)

    def lora_set_weight(self, adapter: str, weight: float):
        L.check(self.lib.fmi_flux_lora_set_weight(self.h, adapter.encode(), float(weight)), self.lib)

    def lora_remove(self, adapter: Optional[str] = None):
        """Drop one adapter (None: every adapter); a Linear left without one holds its loaded weights again, bit for bit."""
        L.check(self.lib.fmi_flux_lora_remove(self.h, adapter.encode() if adapter is not None else None), self.lib)

    def loras(self) -> List[str]:
        return [self.lib.fmi_flux_lora_name(self.h, i).decode() for i in range(self.lib.fmi_flux_lora_count(self.h))]

    def set_linear_bnb4(self, prefix: str, packed, absmax, blocksize: int, quant_type: str, out_features: int, in_features: int):
        q = {"fp4": 1, "nf4": 2}[quant_type]
        pk, pp, _ = _linear_arg(packed, torch.uint8)
        am, ap, _ = _linear_arg(absmax, torch.float32)
        L.check(self.lib.fmi_flux_set_linear_bnb4(self.h, prefix.encode(), pp, ap, blocksize, q, out_features, in_features), self.lib)

    def set_linear_int8(self, prefix: str, weight, scb, out_features: int, in_features: int):
        """LLM.int8 linear (BnbLinear::Int8): weight int8 (out,in), SCB f32 (out)."""
        w, wp, _ = _linear_arg(weight, torch.int8)
        sc, sp, _ = _linear_arg(scb, torch.float32)
        L.check(self.lib.fmi_flux_set_linear_int8(self.h, prefix.encode(), wp, sp, out_features, in_features), self.lib)

    def set_linear_gguf(self, prefix: str, ggml_type: int, data, out_features: int, in_features: int):
        """A Linear as ggml blocks (llama.cpp's .gguf; include/flux_mi355x.h: fmi_flux_set_linear_gguf): row-major, in_features / block_elems blocks per
        row.  `data`: a uint8 torch tensor (host or device), or anything with the buffer protocol (numpy array, memoryview of an mmap) — not copied here."""
        keep, p, nbytes = _linear_arg(data, torch.uint8, raw=True)
        be, bb = C.c_int(), C.c_int()
        L.check(self.lib.fmi_gguf_block_info(int(ggml_type), C.byref(be), C.byref(bb)), self.lib)
        if in_features % be.value == 0 and nbytes != out_features * (in_features // be.value) * bb.value:
            raise L.FmiError(f"set_linear_gguf: {prefix}: {nbytes} bytes of blocks for a ({out_features}, {in_features}) Linear of ggml type {ggml_type}, expected "
                             f"{out_features * (in_features // be.value) * bb.value}", code=L.ERR_INVALID)
        L.check(self.lib.fmi_flux_set_linear_gguf(self.h, prefix.encode(), int(ggml_type), p, out_features, in_features), self.lib)

    def set_linear_f8(self, prefix: str, fmt, codes, scale: float, out_features: int, in_features: int):
        """A Linear as 8-bit float codes with one scale (include/flux_mi355x.h: fmi_flux_set_linear_f8): row-major (out_features, in_features), one code per
        weight.  fmt: "e4m3" | "e5m2" (or 1 | 2).  `codes`: a torch tensor of dtype float8_e4m3fn / float8_e5m2 / uint8 (host or device), or anything with the
        buffer protocol (numpy uint8 array, memoryview of an mmap) — not copied here."""
        keep, p, nbytes = _linear_arg(codes, torch.uint8, raw=True, views=tuple(F8_TORCH.values()))
        if nbytes != out_features * in_features:
            raise L.FmiError(f"set_linear_f8: {prefix}: {nbytes} codes for a ({out_features}, {in_features}) Linear", code=L.ERR_INVALID)
        L.check(self.lib.fmi_flux_set_linear_f8(self.h, prefix.encode(), f8_format(fmt), p, float(scale), out_features, in_features), self.lib)

    def quantize_fp8(self, stream=None):
        """Switch the DiT block linears to the fp8 (OCP e4m3) MFMA path: weights quantised once per output
        channel from the loaded bf16 values, activations per token on the fly (BASELINE configs[4])."""
        L.check(self.lib.fmi_flux_quantize_fp8(self.h, stream), self.lib)
        self._eight_bit = "fp8"

    def quantize_int8(self, mask: int = None, stream=None):
        """Switch the DiT block linears named by `mask` (Q8_* bits; default INT8_DEFAULT_MASK) to the int8 MFMA path: symmetric per-row
        int8 codes (weights once per output channel, activations per token on the fly), exact int32 accumulation; the other block
        linears and everything else stay on the bf16 path — except the attention operands: as in the fp8 mode (set_fp8_attention, default
        on) the blocks whose q|k|v linear is in the mask hand q and k to the attention as e4m3 with static scales (QK^T on the fp8
        MFMA; P.V stays bf16).  set_fp8_attention(0) keeps bf16 operands."""
        L.check(self.lib.fmi_flux_quantize_int8(self.h, INT8_DEFAULT_MASK if mask is None else int(mask), stream), self.lib)
        self._eight_bit = "int8"

    def calibrate_int8(self, on: bool = True):
        """Start (or drop) the calibration of the smoothed int8 recipe: while on, every forward / denoise evaluation (bf16 mode) also records the per-channel
        absmax of each block linear's input; the next quantize_int8() folds s = sqrt(amax_x / amax_W) per channel into the weight codes and 1 / s into the
        activation quantisation (include/flux_mi355x.h: fmi_flux_calibrate_int8).  Without it quantize_int8() is the unsmoothed recipe."""
        L.check(self.lib.fmi_flux_calibrate_int8(self.h, int(bool(on))), self.lib)

    def set_fp8_attention(self, mode: int):
        """q and k of the attention as e4m3 with static scales, QK^T on the fp8 MFMA: 0 never, 1 (default) in the 8-bit modes, 2 in every
        mode — the bf16 block linears included (opt-in: a reduced-precision attention operand, not the reference's semantics)."""
        L.check(self.lib.fmi_flux_set_fp8_attention(self.h, int(mode)), self.lib)

    def missing(self) -> List[str]:
        n = self.lib.fmi_flux_missing_count(self.h)
        return [self.lib.fmi_flux_missing_name(self.h, i).decode() for i in range(n)]

    def assert_complete(self):
        m = self.missing()
        if m:
            raise L.FmiError(f"{len(m)} tensors missing, e.g. {m[:4]}")

    def size_in_bytes(self) -> int:
        return self.lib.fmi_flux_size_in_bytes(self.h)

    def set_quant_dense_cache(self, mode):
        """Quantised linears, launches above 383 (nf4 / fp4) / 256 (LLM.int8) rows — smaller ones always multiply from the packed codes:
        -1 (default) = by memory: 3 when the device has the room, else 0; 0 / False = packed only: per-call expansion into a 264 MB
        scratch + dense GEMM; 1 / True = every matrix expanded once into the bf16 arenas; 2 = always the fused kernels; 3 = the matrices
        of the large launches expanded once.  Same bits in every mode.  Matrices resident as ggml blocks (set_linear_gguf) or 8-bit float codes (set_linear_f8) have no fused kernel:
        at every row count they are expanded once (1, 3, and -1 with the room) or per call (0, and 2 — which has no fused kernel to select there)."""
        L.check(self.lib.fmi_flux_set_quant_dense_cache(self.h, int(mode)), self.lib)

    def set_split_k(self, on: bool):
        """Latency mode for launches of few rows (sequence-parallel shards): residual projections with fewer than 128 tiles are
        split along K and reduced in a fixed order, and the sequence-parallel attention of few heads walks key ranges in parallel
        (log-sum-exp merge) — deterministic, equal to the unsplit result to rounding (not bit for bit)."""
        L.check(self.lib.fmi_flux_set_split_k(self.h, int(bool(on))), self.lib)

    def set_sequence_parallel(self, rank: int, world_size: int, all_to_all=None):
        """Single-image sequence parallelism (fmi_flux_set_sequence_parallel): from now on forward / denoise take THIS rank's
        token shard (dist.sp_shard) and the joint attention trades heads for tokens through `all_to_all`
        (callable(send_ptr, recv_ptr, bytes_per_peer, stream_ptr) -> None; dist.SequenceParallel provides it on
        torch.distributed).  world_size 1 switches it off."""
        if world_size > 1 and all_to_all is None:
            raise L.FmiError("set_sequence_parallel: world_size > 1 needs an all_to_all callable")

        def _cb(_user, send, recv, nbytes, stream):
            try:
                all_to_all(send, recv, nbytes, stream)
                return 0
            except Exception as e:  # an exception must not unwind through the C frames
                import traceback
                traceback.print_exc()
                self._sp_error = e
                return 1

        self._sp_cb = L.ALL_TO_ALL_FN(_cb) if world_size > 1 else L.ALL_TO_ALL_FN()  # keep the thunk alive with the model
        L.check(self.lib.fmi_flux_set_sequence_parallel(self.h, int(rank), int(world_size), self._sp_cb, None), self.lib)
        self._sp_world = int(world_size)

    def set_sequence_parallel_native(self, rank: int, world_size: int, comm):
        """The same with the exchange done by the library's own RCCL communicator (dist.RcclComm / fmi_comm): the callback is the C
        function fmi_comm_all_to_all itself, so an exchange is one ncclAllToAll enqueued from C on the launch stream — no Python
        between two kernels of a block."""
        fn = C.cast(self.lib.fmi_comm_all_to_all, L.ALL_TO_ALL_FN)
        self._sp_cb, self._sp_comm = fn, comm  # keep both alive with the model
        L.check(self.lib.fmi_flux_set_sequence_parallel(self.h, int(rank), int(world_size), fn, comm.h), self.lib)
        self._sp_world = int(world_size)

    # ---- the weights as flat device buffers (multi-GPU broadcast, dist.broadcast_state)
    def state_export(self) -> bytes:
        n = C.c_size_t()
        L.check(self.lib.fmi_flux_state_export(self.h, None, 0, C.byref(n)), self.lib)
        buf = (C.c_uint8 * n.value)()
        L.check(self.lib.fmi_flux_state_export(self.h, buf, n.value, C.byref(n)), self.lib)
        return bytes(buf)

    def state_adopt(self, blob: bytes):
        buf = (C.c_uint8 * len(blob)).from_buffer_copy(blob)
        L.check(self.lib.fmi_flux_state_adopt(self.h, buf, len(blob)), self.lib)

    def state_buffers(self):
        """[(device pointer, bytes)] of the weight arenas (pointer 0 / 0 bytes for an arena not in use)."""
        out = []
        for i in range(self.lib.fmi_flux_state_buffer_count()):
            p, n = C.c_void_p(), C.c_size_t()
            L.check(self.lib.fmi_flux_state_buffer(self.h, i, C.byref(p), C.byref(n)), self.lib)
            out.append((p.value or 0, n.value))
        return out

    def state_views(self, device=None):
        """One flat uint8 torch tensor per weight arena, aliasing its device memory (None for an arena not in use): what
        dist.broadcast_state hands to the collective — the weights travel in place, without a staging copy."""
        from .dist import _DeviceBytes
        dev = torch.device(device) if device is not None else self.device
        return [torch.as_tensor(_DeviceBytes(p, n), device=dev) if n else None for p, n in self.state_buffers()]

    def _inputs(self, img, img_ids, txt, txt_ids, timesteps, y, guidance):
        B, S = int(img_ids.shape[0]), int(img_ids.shape[1])
        T = int(txt.shape[1])
        keep = [t.contiguous() if t is not None else None for t in (img, img_ids, txt, txt_ids, timesteps, y, guidance)]
        img, img_ids, txt, txt_ids, timesteps, y, guidance = keep
        for t, nm in ((img_ids, "img_ids"), (txt_ids, "txt_ids"), (timesteps, "timesteps"), (guidance, "guidance")):
            if t is not None and t.dtype != torch.float32:
                raise TypeError(f"{nm} must be float32")
        inp = L.FluxInputs(_ptr(img), _TORCH_DT[img.dtype] if img is not None else 0, _ptr(img_ids), _ptr(txt), _TORCH_DT[txt.dtype], _ptr(txt_ids),
                           _ptr(timesteps), _ptr(y), _TORCH_DT[y.dtype], _ptr(guidance), B, S, T, 0)
        return inp, keep

    def _context(self, img_ids, context, context_ids):
        """fmi_flux_context of a reference image's packed latents (B,R,C) f32 | bf16 and their ids (B,R,3) f32, with the tensors it points into."""
        if context is None or context_ids is None:
            raise ValueError("context= and context_ids= go together")
        if context.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError("context must be float32 or bfloat16")
        if context_ids.dtype != torch.float32:
            raise TypeError("context_ids must be float32")
        if context.dim() != 3:
            raise ValueError(f"context must be (B,R,C), got {tuple(context.shape)}")
        B, R = int(context.shape[0]), int(context.shape[1])
        if B != int(img_ids.shape[0]) or tuple(context_ids.shape) != (B, R, 3):
            raise ValueError(f"context is {tuple(context.shape)} and context_ids {tuple(context_ids.shape)} for a batch of {int(img_ids.shape[0])}")
        if int(context.shape[2]) != self.state_channels:
            raise ValueError(f"context has {int(context.shape[2])} channels, the model's state has {self.state_channels}")
        if context.device != img_ids.device or context_ids.device != img_ids.device:
            raise ValueError(f"context is on {context.device} and context_ids on {context_ids.device}, img_ids on {img_ids.device}")
        # (a tensor that is contiguous already is passed as it lies, whatever its address: the library picks the access width)
        keep = [context.contiguous(), context_ids.contiguous()]
        return L.FluxContext(_ptr(keep[0]), _TORCH_DT[context.dtype], _ptr(keep[1]), R), keep

    def _control(self, img, control):
        """fmi_flux_control of the conditioning channels (B,S,cond_channels) f32 | bf16, with the tensor it points into; (None, None) on a plain model."""
        check_control_args(self.cond_channels, tuple(img.shape), None if control is None else tuple(control.shape))
        if control is None:
            return None, None
        if control.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError("control must be float32 or bfloat16")
        if control.device != img.device:
            raise ValueError(f"control is on {control.device}, img on {img.device}")
        keep = control.contiguous()
        return L.FluxControl(_ptr(keep), _TORCH_DT[control.dtype]), keep

    def _controlnet(self, img, controlnet, controlnet_cond, scale, step_scales, n_steps):
        """fmi_flux_controlnet for controlnet= / controlnet_cond=, with what it points into; (None, None) without a ControlNet."""
        ss = check_controlnet_args(self.cfg, None if controlnet is None else controlnet.cfg, tuple(img.shape), None if controlnet_cond is None else tuple(controlnet_cond.shape),
                                   scale, step_scales, n_steps)
        if controlnet is None:
            return None, None
        if not isinstance(controlnet, FluxControlNetModel):
            raise TypeError("controlnet= must be a FluxControlNetModel")
        if controlnet_cond.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError("controlnet_cond must be float32 or bfloat16")
        if controlnet_cond.device != img.device:
            raise ValueError(f"controlnet_cond is on {controlnet_cond.device}, img on {img.device}")
        keep = [controlnet_cond.contiguous(), ss]
        return L.FluxControlNet(controlnet.h, _ptr(keep[0]), _TORCH_DT[controlnet_cond.dtype], float(scale),
                                ss.ctypes.data_as(C.POINTER(C.c_float)) if ss is not None else None), keep

    def _ip(self, img, ip_adapter, embeds, negative_embeds, scale, step_scales, n_steps, has_negative):
        """fmi_flux_ip for ip_adapter= / ip_adapter_image_embeds=, with what it points into; (None, None) without an adapter."""
        if ip_adapter is not None and not isinstance(ip_adapter, FluxIPAdapter):
            raise TypeError("ip_adapter= must be a FluxIPAdapter")
        ss = check_ip_adapter_args(self.cfg, None if ip_adapter is None else ip_adapter.dims, tuple(img.shape), None if embeds is None else tuple(embeds.shape),
                                   None if negative_embeds is None else tuple(negative_embeds.shape), scale, step_scales, n_steps, has_negative)
        if ip_adapter is None:
            return None, None
        for t, nm in ((embeds, "ip_adapter_image_embeds"), (negative_embeds, "negative_ip_adapter_image_embeds")):
            if t is None:
                continue
            if t.dtype not in (torch.float32, torch.bfloat16) or t.dtype != embeds.dtype:
                raise TypeError(f"{nm} must be float32 or bfloat16 (both of one dtype)")
            if t.device != img.device:
                raise ValueError(f"{nm} is on {t.device}, img on {img.device}")
        keep = [embeds.contiguous(), None if negative_embeds is None else negative_embeds.contiguous(), ss]
        return L.FluxIp(ip_adapter.h, _ptr(keep[0]), _TORCH_DT[embeds.dtype], _ptr(keep[1]), float(scale),
                        ss.ctypes.data_as(C.POINTER(C.c_float)) if ss is not None else None), keep

    def _check_combination(self, **given):
        """check_combination of the options a call has (one keyword each, true when present) and the modes this model is in."""
        modes = ("sequence_parallel" if getattr(self, "_sp_world", 1) > 1 else None, getattr(self, "_eight_bit", None))
        check_combination({k for k, v in given.items() if v} | {m for m in modes if m})

    def forward(self, img, img_ids, txt, txt_ids, timesteps, y, guidance=None, context=None, context_ids=None, control=None, controlnet=None, controlnet_cond=None,
                controlnet_scale=1.0, ip_adapter=None, ip_adapter_image_embeds=None, ip_adapter_scale=1.0):
        """== Flux::forward (model.rs:790-833).  Returns the velocity (B,S,C) f32.  One call: fmi_flux_forward_context with a context, else fmi_flux_forward_ip.
        context= / context_ids=: reference-image tokens appended to the image tokens for this evaluation (fmi_flux_forward_context); the velocity is img's.
        control=: the conditioning channels (B,S,cond_channels) f32 | bf16 of a channel-conditioned model (fmi_flux_forward_control): the
        evaluation is Flux::forward on cat([img, control], 2) and the velocity stays img's width.  Required on such a model, refused on any other.
        controlnet= / controlnet_cond= / controlnet_scale=: a FluxControlNetModel evaluated on the same inputs and controlnet_cond (B,S,in_channels) f32 | bf16, the
        packed latents of the control image; its per-block samples, times the scale, are added to this model's stream after every block
        (fmi_flux_forward_controlnet).  Not with context=, control= or sequence parallelism.
        ip_adapter= / ip_adapter_image_embeds= / ip_adapter_scale=: a FluxIPAdapter and one image embedding (B, embed_dim) f32 | bf16 per sample; every double block
        adds scale * softmax(q K^T / sqrt(128)) V of its un-rotated, RMS-normed image queries against the adapter's tokens to the image stream
        (fmi_flux_forward_ip).  Works with control= and controlnet=; not with context=, sequence parallelism or the 8-bit modes."""
        has_ctx = context is not None or context_ids is not None
        # (every keep_*, like keep, holds the tensors behind the pointers until the call has returned)
        cn, keep_cn = self._controlnet(img, controlnet, controlnet_cond, controlnet_scale, None, None)
        ip, keep_ip = self._ip(img, ip_adapter, ip_adapter_image_embeds, None, ip_adapter_scale, None, None, False)
        ctl, keep_ctl = self._control(img, control)
        self._check_combination(context=has_ctx, control=ctl, controlnet=cn, ip_adapter=ip)
        inp, keep = self._inputs(img, img_ids, txt, txt_ids, timesteps, y, guidance)
        pred = torch.empty(img.shape, dtype=torch.float32, device=img.device)
        if has_ctx:  # (alone: the table refuses it next to each of the other three)
            ctx, keep_ctx = self._context(img_ids, context, context_ids)
            L.check(self.lib.fmi_flux_forward_context(self.h, C.byref(inp), C.byref(ctx), _ptr(pred), _stream()), self.lib)
        else:  # fmi_flux_forward_ip with NULL for what is not given is the shorter entry of the rest (include/flux_mi355x.h)
            L.check(self.lib.fmi_flux_forward_ip(self.h, C.byref(inp), ctl and C.byref(ctl), cn and C.byref(cn), ip and C.byref(ip), _ptr(pred), _stream()), self.lib)
        return pred

    def denoise(self, img, img_ids, txt, txt_ids, y, guidance, timesteps: List[float], x0=None, noise=None, mask=None, context=None, context_ids=None,
                cache_threshold=None, cache_force=None, return_cache_stats=False, negative_txt=None, negative_y=None, true_cfg_scale=None, control=None,
                controlnet=None, controlnet_cond=None, controlnet_scale=1.0, controlnet_step_scales=None, ip_adapter=None, ip_adapter_image_embeds=None,
                negative_ip_adapter_image_embeds=None, ip_adapter_scale=1.0, ip_adapter_step_scales=None, solver=None):
        """== Sampler::sample around Flux::forward (sampling.rs:25-48). `img` f32 (B,S,C), updated copy returned.  One fmi_flux_denoise_solver call: the keywords fill its options
        and its ControlNet and adapter arguments; which of them combine is REFUSED_PAIRS / REFUSED_MODES above.
        x0 / noise / mask (all three or none; f32, shaped like img): the inpainting loop fmi_flux_denoise_inpaint — after every step the source
        latents x0, re-noised with `noise` to the step's target time, are blended back in where mask is 0 (include/flux_mi355x.h).
        context= / context_ids=: reference-image tokens every evaluation appends to the state's (fmi_flux_denoise_context); the state stays (B,S,C).
        cache_threshold= / cache_force=: the first-block step cache (fmi_flux_denoise_cached), off unless one of them is given.  Every step runs
        double block 0; a step whose block-0 residual lies within `cache_threshold` (relative L1) of the last computed step's skips every other block and adds
        their cached output residual.  The decision is per CALL: a batch reuses a step only when every sample is under the threshold, so a batched call may differ
        from its single-sample runs.  cache_force: one entry per step, -1 decide by threshold, 0 compute, 1 reuse (step 0 is always computed).  The cached loop
        synchronises the stream once per step.  No threshold is recommended: ParaAttention suggests 0.08 for FLUX.1-dev, which this project has no real weights
        to verify.  return_cache_stats=True: returns (img, {"decisions": int array (n,), "distances": float array (n, B), -1 where not measured}).
        negative_txt= / negative_y= / true_cfg_scale=: true classifier-free guidance (fmi_flux_denoise_cfg).  The negative prompt's embeddings,
        shaped like txt and y (f32 | bf16); every step evaluates the prompt and the negative in ONE batch of 2 B samples on the same state, ids, guidance and
        context, and steps along neg + true_cfg_scale * (pos - neg) (default scale 1.0; any finite scale >= 0).  B <= 4; not with the step cache, not under
        sequence parallelism; works with x0 / noise / mask and with context=.
        control=: the conditioning channels (B,S,cond_channels) f32 | bf16 of a channel-conditioned model (fmi_flux_denoise_control), the same at
        every step and, under true CFG, for the prompt and the negative; the state stays (B,S,C).  Required on such a model, refused on any other; works with
        x0 / noise / mask and the negative, not with context=, the step cache or sequence parallelism.
        controlnet= / controlnet_cond= / controlnet_scale= / controlnet_step_scales=: a FluxControlNetModel (fmi_flux_denoise_controlnet).  Step i
        evaluates it on the step's state and controlnet_cond (B,S,in_channels) f32 | bf16 and adds its samples at controlnet_scale * controlnet_step_scales[i] (one
        entry per step; None: 1 everywhere); a step whose scale is 0 is the plain step.  Works with x0 / noise / mask and with the negative (which the ControlNet
        then sees as well); not with context=, control=, the step cache or sequence parallelism.
        ip_adapter= / ip_adapter_image_embeds= / negative_ip_adapter_image_embeds= / ip_adapter_scale= / ip_adapter_step_scales=: a FluxIPAdapter
        (fmi_flux_denoise_ip) and one image embedding (B, embed_dim) f32 | bf16 per sample.  The adapter's tokens and every block's K / V are
        projected once per call; every double block of step i adds ip_adapter_scale * ip_adapter_step_scales[i] times the image-prompt attention to the image
        stream, and a step whose scale is 0 is the plain step.  Under true CFG the negative half attends to negative_ip_adapter_image_embeds, or to zero
        embeddings through the same projection.  Works with the negative, x0 / noise / mask, control= and controlnet=; not with context=, the step cache,
        sequence parallelism or the 8-bit modes.
        solver=: None | "euler" (the loop as it always was) | "heun" | "dpmpp_2m" (fmi_flux_denoise_solver): a second-order integrator over the
        same schedule, which must then be strictly decreasing inside [0, 1].  "heun" evaluates the model twice per step (once on the last step of a schedule that
        ends at 0), "dpmpp_2m" once, keeping one step of history.  Both work with every option above, except "heun" with the step cache and either under
        sequence parallelism.  A capability, not a recommendation: no step count is suggested for either."""
        n_steps = len(timesteps) - 1
        has_ctx = context is not None or context_ids is not None
        # (every keep_*, like keep, holds the tensors behind the pointers until the call has returned)
        ip, keep_ip = self._ip(img, ip_adapter, ip_adapter_image_embeds, negative_ip_adapter_image_embeds, ip_adapter_scale, ip_adapter_step_scales, n_steps,
                               negative_txt is not None or negative_y is not None)
        cn, keep_cn = self._controlnet(img, controlnet, controlnet_cond, controlnet_scale, controlnet_step_scales, n_steps)
        ctl, keep_ctl = self._control(img, control)
        cfg_scale = check_true_cfg_args(tuple(txt.shape), tuple(y.shape), None if negative_txt is None else tuple(negative_txt.shape),
                                        None if negative_y is None else tuple(negative_y.shape), true_cfg_scale)
        thr, force = check_step_cache_args(n_steps, cache_threshold, cache_force)
        self._check_combination(context=has_ctx, control=ctl, true_cfg=cfg_scale is not None, cache=thr is not None, controlnet=cn, ip_adapter=ip)
        kind = check_solver_args(solver, timesteps, cache=thr is not None, sequence_parallel=getattr(self, "_sp_world", 1) > 1)
        if return_cache_stats and thr is None:
            raise ValueError("return_cache_stats needs cache_threshold= or cache_force=")
        img = img.to(torch.float32).clone().contiguous()
        inp, keep = self._inputs(None, img_ids, txt, txt_ids, None, y, guidance)
        ts = (C.c_double * len(timesteps))(*timesteps)
        keep_blend = [_like_img(t, nm, img) for t, nm in ((x0, "x0"), (noise, "noise"), (mask, "mask"))]
        ctx, keep_ctx = self._context(img_ids, context, context_ids) if has_ctx else (None, None)
        # (a missing one of x0 / noise / mask reaches the library as NULL: it answers FMI_ERR_INVALID)
        opts = L.FluxDenoiseOptions(ctx and C.pointer(ctx), ctl and C.pointer(ctl), None, None, *[_ptr(t) for t in keep_blend])
        if cfg_scale is not None:
            for t, nm in ((negative_txt, "negative_txt"), (negative_y, "negative_y")):
                if t.dtype not in (torch.float32, torch.bfloat16):
                    raise TypeError(f"{nm} must be float32 or bfloat16")
                if t.device != img.device:
                    raise ValueError(f"{nm} is on {t.device}, img on {img.device}")
            keep_neg = [negative_txt.contiguous(), negative_y.contiguous()]
            opts.cfg = C.pointer(L.FluxTrueCfg(_ptr(keep_neg[0]), _TORCH_DT[negative_txt.dtype], _ptr(keep_neg[1]), _TORCH_DT[negative_y.dtype], cfg_scale))
        if thr is not None:
            decisions = np.zeros(max(n_steps, 0), np.int32)
            distances = np.full((max(n_steps, 0), int(img_ids.shape[0])), -1.0, np.float32)
            opts.cache = C.pointer(L.FluxStepCache(thr, force.ctypes.data_as(C.POINTER(C.c_int8)) if force is not None else None,
                                                   decisions.ctypes.data_as(C.POINTER(C.c_int32)), distances.ctypes.data_as(C.POINTER(C.c_float))))
        # (with solver NULL this IS fmi_flux_denoise_ip, with ip NULL too fmi_flux_denoise_controlnet, with cn NULL too fmi_flux_denoise_with: include/flux_mi355x.h)
        sv = None if kind is None else L.FluxSolver(kind)
        L.check(self.lib.fmi_flux_denoise_solver(self.h, C.byref(inp), C.byref(opts), cn and C.byref(cn), ip and C.byref(ip), sv and C.byref(sv), _ptr(img), ts, n_steps,
                                                 _stream()), self.lib)
        return (img, {"decisions": decisions, "distances": distances}) if return_cache_stats else img

    def solver_bytes(self) -> int:
        """Device bytes the solvers' buffers hold: 0 until the first denoise with solver="heun" / "dpmpp_2m" (a loop without a solver never allocates them)."""
        return int(self.lib.fmi_flux_solver_bytes(self.h))

    def step_cache_bytes(self) -> int:
        """Device bytes the step cache holds: 0 until the first denoise with cache_threshold= / cache_force= (the plain loops never allocate it)."""
        return int(self.lib.fmi_flux_step_cache_bytes(self.h))

    def set_profiling(self, on: bool):
        L.check(self.lib.fmi_flux_set_profiling(self.h, int(on)), self.lib)

    def phase_ms(self) -> dict:
        n = self.lib.fmi_flux_phase_count()
        out = (C.c_float * n)()
        L.check(self.lib.fmi_flux_phase_ms(self.h, out), self.lib)
        return {self.lib.fmi_flux_phase_name(i).decode(): out[i] for i in range(n)}


class FluxControlNetModel(FluxModel):
    """A FLUX ControlNet (diffusers' FluxControlNetModel; fmi_flux_create_controlnet): cfg as FluxModel's, with the net's own num_layers (>= 1) and
    num_single_layers (>= 0).  Handed to FluxModel.forward / denoise as controlnet=; eval() runs it alone.  bf16 only: the 8-bit modes, LoRA, the quantised
    setters and sequence parallelism raise FmiError (FMI_ERR_UNSUPPORTED), as do forward() and denoise() on the net itself."""

    def __init__(self, cfg: dict, device: int = 0):
        self.lib = L.load()
        self.cfg = dict(cfg)
        self.state_channels, self.cond_channels = int(cfg["in_channels"]), 0
        L.check(self.lib.fmi_init(device), self.lib)
        c = L.FluxConfig(cfg["in_channels"], cfg["pooled_projection_dim"], cfg["joint_attention_dim"], cfg["num_attention_heads"],
                         cfg["num_layers"], cfg["num_single_layers"], int(cfg["guidance_embeds"]), (C.c_int * 3)(*cfg["axes_dim"]), cfg["theta"])
        h = C.c_void_p()
        L.check(self.lib.fmi_flux_create_controlnet(C.byref(c), L.MODEL_BF16, C.byref(h)), self.lib)
        self.h = h
        self.hidden = cfg["num_attention_heads"] * 128
        self.device = torch.device("cuda", device)

    def _shapes(self):
        if getattr(self, "_shape_cache", None) is None:
            from . import synth
            self._shape_cache = synth.controlnet_tensor_shapes(self.cfg)
        return self._shape_cache

    def eval(self, img, img_ids, txt, txt_ids, timesteps, y, guidance=None, cond=None):
        """The ControlNet alone (fmi_flux_controlnet_eval): returns (double_samples, single_samples), lists of (B,S,D) f32 tensors — the stored bf16 samples, widened."""
        if cond is None or cond.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError("eval: cond (B,S,in_channels) float32 | bfloat16 is required")
        if tuple(cond.shape) != (int(img.shape[0]), int(img.shape[1]), int(self.cfg["in_channels"])):
            raise ValueError(f"cond is {tuple(cond.shape)}, img is {tuple(img.shape)}")
        inp, keep = self._inputs(img, img_ids, txt, txt_ids, timesteps, y, guidance)
        cond = cond.contiguous()
        L.check(self.lib.fmi_flux_controlnet_eval(self.h, C.byref(inp), _ptr(cond), _TORCH_DT[cond.dtype], _stream()), self.lib)
        out = []
        for single, n in ((0, self.cfg["num_layers"]), (1, self.cfg["num_single_layers"])):
            out.append([])
            for i in range(n):
                t = torch.empty((int(img.shape[0]), int(img.shape[1]), self.hidden), dtype=torch.float32, device=img.device)
                L.check(self.lib.fmi_flux_controlnet_sample(self.h, single, i, _ptr(t)), self.lib)
                out[-1].append(t)
        return out[0], out[1]


class FluxIPAdapter:
    """A FLUX IP-Adapter (XLabs flux-ip-adapter; diffusers' FluxIPAdapterMixin; fmi_ip_adapter_create) for a transformer of config cfg: the image
    projection Linear(embed_dim -> num_tokens * joint_attention_dim) + LayerNorm, and to_k_ip / to_v_ip per double block.  Tensor names are the diffusers-converted
    ones (synth.ip_adapter_tensor_shapes; loader.ip_adapter_key_map brings XLabs names to them).  Handed to FluxModel.forward / denoise as ip_adapter=."""

    def __init__(self, cfg: dict, embed_dim: int, num_tokens: int, device: int = 0):
        self.lib = L.load()
        self.cfg = dict(cfg)
        self.embed_dim, self.num_tokens = int(embed_dim), int(num_tokens)
        self.dims = dict(num_heads=int(cfg["num_attention_heads"]), joint_attention_dim=int(cfg["joint_attention_dim"]), num_layers=int(cfg["num_layers"]),
                         embed_dim=self.embed_dim, num_tokens=self.num_tokens)
        L.check(self.lib.fmi_init(device), self.lib)
        c = L.FluxConfig(state_channels(cfg), cfg["pooled_projection_dim"], cfg["joint_attention_dim"], cfg["num_attention_heads"], cfg["num_layers"],
                         cfg["num_single_layers"], int(cfg["guidance_embeds"]), (C.c_int * 3)(*cfg["axes_dim"]), cfg["theta"])
        h = C.c_void_p()
        L.check(self.lib.fmi_ip_adapter_create(C.byref(c), self.embed_dim, self.num_tokens, C.byref(h)), self.lib)
        self.h = h
        self.device = torch.device("cuda", device)

    def close(self):
        if getattr(self, "h", None):
            self.lib.fmi_ip_adapter_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_tensor(self, name: str, t):
        p, dt, shape, keep = _tensor_arg(t)
        sh = (C.c_int64 * len(shape))(*shape)
        L.check(self.lib.fmi_ip_adapter_set_tensor(self.h, name.encode(), p, dt, sh, len(shape)), self.lib)

    def missing(self) -> List[str]:
        n = self.lib.fmi_ip_adapter_missing_count(self.h)
        return [self.lib.fmi_ip_adapter_missing_name(self.h, i).decode() for i in range(n)]

    def load_state_dict(self, tensors: dict):
        for k, v in tensors.items():
            self.set_tensor(k, v)
        m = self.missing()
        if m:
            raise L.FmiError(f"{len(m)} IP-Adapter tensors missing, e.g. {m[:4]}")

    def size_in_bytes(self) -> int:
        return int(self.lib.fmi_ip_adapter_size_in_bytes(self.h))


class AutoEncoderKl:
    def __init__(self, cfg: dict, device: int = 0):
        self.lib = L.load()
        self.cfg = dict(cfg)
        L.check(self.lib.fmi_init(device), self.lib)
        boc = list(cfg["block_out_channels"])
        if len(boc) != 4:
            raise L.FmiError("block_out_channels must have 4 entries (the reference hard-codes i_level != 3, vae.rs:412)")
        c = L.VaeConfig(cfg["in_channels"], cfg["out_channels"], (C.c_int * 4)(*boc), 4, cfg["layers_per_block"], cfg["latent_channels"],
                        cfg["norm_num_groups"], int(cfg["mid_block_add_attention"]), int(cfg.get("use_post_quant_conv", False)),
                        cfg["scaling_factor"], cfg["shift_factor"], int(cfg.get("use_quant_conv", False)))
        h = C.c_void_p()
        L.check(self.lib.fmi_vae_create(C.byref(c), L.MODEL_BF16, C.byref(h)), self.lib)
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.lib.fmi_vae_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_tensor(self, name, t):
        p, dt, shape, keep = _tensor_arg(t)
        sh = (C.c_int64 * len(shape))(*shape)
        L.check(self.lib.fmi_vae_set_tensor(self.h, name.encode(), p, dt, sh, len(shape)), self.lib)

    def missing(self):
        n = self.lib.fmi_vae_missing_count(self.h)
        return [self.lib.fmi_vae_missing_name(self.h, i).decode() for i in range(n)]

    def load_state_dict(self, tensors: dict):
        """Decoder tensors are required; encoder (`encoder.*`, `quant_conv.*`) tensors are optional
        (only `encode` needs them, and it reports what is missing)."""
        for k, v in tensors.items():
            self.set_tensor(k, v)
        m = [n for n in self.missing() if not (n.startswith("encoder.") or n.startswith("quant_conv."))]
        if m:
            raise L.FmiError(f"{len(m)} VAE tensors missing, e.g. {m[0]}")

    def encode(self, image, noise=None, seed=None, return_moments=False):
        """== VAEModel::encode (vaes/mod.rs:15-28, autoencoder_kl.rs:103-110): image (B,3,H,W) f32 ->
        z (B,16,H/8,W/8) f32 = mean + exp(0.5 logvar) * noise.  noise: explicit tensor, or Philox
        N(0,1) from `seed`, or None and seed None -> the distribution mean."""
        image = image.to(torch.float32).contiguous()
        B, _, H, W = image.shape
        lat = self.cfg["latent_channels"]
        if noise is None and seed is not None:
            noise = randn_latents(B, lat, H // 8, W // 8, seed, 0, image.device)
        if noise is not None:
            noise = noise.to(device=image.device, dtype=torch.float32).contiguous()
        z = torch.empty((B, lat, H // 8, W // 8), dtype=torch.float32, device=image.device)
        mom = torch.empty((B, 2 * lat, H // 8, W // 8), dtype=torch.float32, device=image.device) if return_moments else None
        L.check(self.lib.fmi_vae_encode(self.h, _ptr(image), B, H, W, _ptr(noise) if noise is not None else None, _ptr(z),
                                        _ptr(mom) if mom is not None else None, _stream()))
        return (z, mom) if return_moments else z

    def scale_factor(self) -> float:
        return self.lib.fmi_vae_scale_factor(self.h)

    def shift_factor(self) -> float:
        return self.lib.fmi_vae_shift_factor(self.h)

    def mid_attention(self, x_nhwc):
        """AttnBlock::forward (vae.rs:95-111) of the decoder's mid block alone: (B,H,W,C) bf16 NHWC -> same shape."""
        x = x_nhwc.contiguous()
        assert x.dtype == torch.bfloat16 and x.dim() == 4
        out = torch.empty_like(x)
        L.check(self.lib.fmi_vae_mid_attention(self.h, _ptr(x), x.shape[0], x.shape[1], x.shape[2], _ptr(out), _stream()), self.lib)
        return out

    def decode(self, z):
        """== VAEModel::decode (vaes/mod.rs:15-28): z (B,16,h,w) f32 -> (B,3,8h,8w) f32."""
        z = z.to(torch.float32).contiguous()
        B, _, h, w = z.shape
        out = torch.empty((B, self.cfg["out_channels"], 8 * h, 8 * w), dtype=torch.float32, device=z.device)
        L.check(self.lib.fmi_vae_decode(self.h, _ptr(z), B, h, w, _ptr(out), _stream()), self.lib)
        return out


# ---- tensor glue of FluxPipeline::forward (pipelines/flux/mod.rs:270-332), on device
def pack_latents(latent):
    """State::new patchify (flux/sampling.rs:131-148): (B,C,h,w) f32 -> img (B,hw/4,4C), img_ids (B,hw/4,3)."""
    latent = latent.to(torch.float32).contiguous()
    B, Cc, h, w = latent.shape
    img = torch.empty((B, (h // 2) * (w // 2), Cc * 4), dtype=torch.float32, device=latent.device)
    ids = torch.empty((B, (h // 2) * (w // 2), 3), dtype=torch.float32, device=latent.device)
    L.check(L.load().fmi_pack_latents(_ptr(latent), B, Cc, h, w, _ptr(img), _ptr(ids), _stream()))
    return img, ids


def unpack_latents(img, Cc, h, w, scale_factor, shift_factor):
    img = img.to(torch.float32).contiguous()
    B = img.shape[0]
    z = torch.empty((B, Cc, h, w), dtype=torch.float32, device=img.device)
    L.check(L.load().fmi_unpack_latents(_ptr(img), B, Cc, h, w, scale_factor, shift_factor, _ptr(z), _stream()))
    return z


def postprocess_u8(image, interleave=False):
    image = image.to(torch.float32).contiguous()
    B, Cc, H, W = image.shape
    out = torch.empty((B, H, W, Cc) if interleave else (B, Cc, H, W), dtype=torch.uint8, device=image.device)
    L.check(L.load().fmi_postprocess_u8(_ptr(image), B, Cc, H, W, int(interleave), _ptr(out), _stream()))
    return out


# ---- image-to-image / inpainting glue
def preprocess_u8(image, interleaved=False):
    """u8 (B,C,H,W), or (B,H,W,C) with interleaved=True (what output="rgb" returns) -> f32 (B,C,H,W) in [-1,1]: x = (u + 0.5) / 127.5 - 1, the centre of the
    bin postprocess_u8 truncates into u, so postprocess_u8(preprocess_u8(u)) == u."""
    if image.dtype != torch.uint8 or image.dim() != 4:
        raise TypeError("preprocess_u8: a uint8 tensor of 4 dimensions is required")
    image = image.contiguous()
    B, Cc, H, W = (image.shape[0], image.shape[3], image.shape[1], image.shape[2]) if interleaved else image.shape
    out = torch.empty((B, Cc, H, W), dtype=torch.float32, device=image.device)
    L.check(L.load().fmi_preprocess_u8(_ptr(image), B, Cc, H, W, int(interleaved), _ptr(out), _stream()))
    return out


def latent_mask(mask, Cc=16):
    """Pixel mask (B,H,W) f32 in [0,1] (1 = repaint, 0 = keep), H and W multiples of 16 -> (B,(H/16)(W/16),4*Cc) f32: 8x8 block means, broadcast over the
    Cc latent channels, in pack_latents' layout."""
    mask = mask.to(torch.float32).contiguous()
    B, H, W = mask.shape
    if H % 16 or W % 16:
        raise ValueError(f"latent_mask: H and W must be multiples of 16, got {H} x {W}")
    out = torch.empty((B, (H // 16) * (W // 16), Cc * 4), dtype=torch.float32, device=mask.device)
    L.check(L.load().fmi_latent_mask(_ptr(mask), B, Cc, H, W, _ptr(out), _stream()))
    return out


# ---- 8-bit float weights of single-file checkpoints
F8_FORMATS = {"e4m3": 1, "e5m2": 2}  # fmi_f8_dequantize's format argument: OCP e4m3fn / OCP e5m2
F8_TORCH = {1: torch.float8_e4m3fn, 2: torch.float8_e5m2}


def f8_format(fmt) -> int:
    """"e4m3" | "e5m2" | a torch float8 dtype | 1 | 2 as the C ABI's format id; anything else is passed through as an int for the library to refuse."""
    if fmt in F8_FORMATS:
        return F8_FORMATS[fmt]
    for k, dt in F8_TORCH.items():
        if fmt is dt:
            return k
    return int(fmt)


def f8_dequantize(codes, fmt, scale: float = 1.0, dtype=torch.bfloat16):
    """fmi_f8_dequantize: the values of `codes` (a device tensor of dtype uint8 or torch's float8_e4m3fn / float8_e5m2; any shape, contiguous, any byte offset)
    times `scale`, as a new tensor of the same shape: f32(code) exactly, one rounded f32 multiply, and for bfloat16 one RNE rounding."""
    if not codes.is_cuda or not codes.is_contiguous() or codes.element_size() != 1:
        raise TypeError("f8_dequantize: a contiguous device tensor of one-byte elements is required")
    if dtype not in (torch.bfloat16, torch.float32):
        raise TypeError("f8_dequantize: dtype must be bfloat16 or float32")
    out = torch.empty(codes.shape, dtype=dtype, device=codes.device)
    L.check(L.load().fmi_f8_dequantize(f8_format(fmt), _ptr(codes), codes.numel(), float(scale), _ptr(out), _TORCH_DT[dtype], _stream()))
    return out


# ---- channel-concatenated conditioning glue (FLUX.1 Fill / Canny / Depth)
def cast_cols_bf16(src, dst, col0, rows=None):
    """fmi_cast_cols_bf16, in place on dst and returning it: row r of src (rows_src, cols) f32 | bf16, read at r % rows_src, -> dst[r, col0 : col0 + cols] as
    bf16 (round to nearest even), for r < rows (default: dst's rows); dst (rows, dst_ld) bf16, its other columns untouched.  cols, dst_ld, col0 multiples of 8."""
    if src.dim() != 2 or dst.dim() != 2 or dst.dtype != torch.bfloat16 or src.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError("cast_cols_bf16: src (rows_src, cols) float32 | bfloat16 and dst (rows, dst_ld) bfloat16 are required")
    if not (src.is_contiguous() and dst.is_contiguous()) or src.device != dst.device:
        raise TypeError("cast_cols_bf16: contiguous tensors on one device are required")
    rows = int(dst.shape[0]) if rows is None else int(rows)
    if rows > dst.shape[0]:
        raise ValueError(f"cast_cols_bf16: {rows} rows do not fit dst {tuple(dst.shape)}")
    L.check(L.load().fmi_cast_cols_bf16(_ptr(src), _TORCH_DT[src.dtype], rows, int(src.shape[0]), int(src.shape[1]), _ptr(dst), int(dst.shape[1]), int(col0), _stream()))
    return dst


def add_scaled_rows_bf16(x, src, scale, rows=None, row0=0):
    """fmi_add_scaled_rows_bf16, the ControlNet injection kernel on its own, in place on x and returning it: x[b, row0 + r, :] += scale * src[b, r, :]
    in f32, one unfused multiply and add per element, for r < rows (default: all of src's); x (B,Lx,D) float32, src (B,rows,D) bfloat16, both as they lie in memory
    (contiguous; x may be a view that starts anywhere).  Rows outside [row0, row0 + rows) are not touched."""
    if x.dim() != 3 or src.dim() != 3 or x.dtype != torch.float32 or src.dtype != torch.bfloat16 or x.device != src.device:
        raise TypeError("add_scaled_rows_bf16: x (B,Lx,D) float32 and src (B,rows,D) bfloat16 on one device are required")
    if not (x.is_contiguous() and src.is_contiguous()):
        raise TypeError("add_scaled_rows_bf16: contiguous tensors are required")
    Bn, Lx, D = (int(v) for v in x.shape)
    rows = int(src.shape[1]) if rows is None else int(rows)
    if int(src.shape[0]) != Bn or int(src.shape[2]) != D or int(src.shape[1]) != rows or row0 < 0 or row0 + rows > Lx:
        raise ValueError(f"add_scaled_rows_bf16: src {tuple(src.shape)} does not fit rows [{row0}, {row0 + rows}) of x {tuple(x.shape)}")
    L.check(L.load().fmi_add_scaled_rows_bf16(C.c_void_p(x.data_ptr() + 4 * row0 * D), Lx * D, _ptr(src), Bn, rows, D, float(scale), _stream()))
    return x


def ip_attention(q, norm_q, k, v, x, scale, max_row_blocks=0):
    """fmi_ip_attention, the IP-Adapter's image-prompt attention kernel on its own, in place on x and returning it: for every sample, row and head
    x[b, r, h * 128 :][:128] += scale * softmax(rmsnorm(q[b, r, h]) * norm_q . k[b, h]^T / sqrt(128)) . v[b, h].  q (B,S,H,128) bfloat16, possibly a strided view
    (the q third of a (B,S,3,H,128) projection); norm_q (128) bfloat16; k, v (B,H,N,128) bfloat16 contiguous; x (B,S,H*128) float32 whose rows are contiguous and
    whose samples may lie further apart.  max_row_blocks: a cap on the grid's row dimension (0: the launcher's choice) — the bits do not depend on it."""
    if q.dim() != 4 or k.dim() != 4 or x.dim() != 3 or q.dtype != torch.bfloat16 or k.dtype != torch.bfloat16 or v.dtype != torch.bfloat16 or \
            norm_q.dtype != torch.bfloat16 or x.dtype != torch.float32:
        raise TypeError("ip_attention: q (B,S,H,128), norm_q (128), k / v (B,H,N,128) bfloat16 and x (B,S,H*128) float32 are required")
    Bn, S, H, d = (int(t) for t in q.shape)
    N = int(k.shape[2])
    if d != 128 or tuple(k.shape) != (Bn, H, N, 128) or tuple(v.shape) != tuple(k.shape) or tuple(x.shape) != (Bn, S, H * 128) or tuple(norm_q.shape) != (128,):
        raise ValueError(f"ip_attention: shapes q {tuple(q.shape)}, k {tuple(k.shape)}, v {tuple(v.shape)}, x {tuple(x.shape)} do not fit")
    if not (k.is_contiguous() and v.is_contiguous() and norm_q.is_contiguous()) or q.stride(3) != 1 or q.stride(2) != 128 or x.stride(2) != 1 or x.stride(1) != H * 128:
        raise TypeError("ip_attention: k, v, norm_q contiguous, q with unit strides inside a row and x with contiguous rows are required")
    L.check(L.load().fmi_ip_attention(_ptr(q), int(q.stride(1)), int(q.stride(0)), _ptr(norm_q), _ptr(k), _ptr(v), _ptr(x), int(x.stride(0)), Bn, H, S, N, float(scale),
                                      int(max_row_blocks), _stream()))
    return x


def mask_image(image, mask):
    """The masked image of a Fill request: image (B,C,H,W) f32 * (1 - b) with b = mask >= 0.5 (mask (B,H,W) f32, 1 = fill), as diffusers' FluxFillPipeline."""
    image, mask = image.to(torch.float32).contiguous(), mask.to(torch.float32).contiguous()
    B, Cc, H, W = image.shape
    if tuple(mask.shape) != (B, H, W):
        raise ValueError(f"mask_image: mask is {tuple(mask.shape)}, image is {tuple(image.shape)}")
    out = torch.empty_like(image)
    L.check(L.load().fmi_mask_image(_ptr(image), _ptr(mask), B, Cc, H, W, _ptr(out), _stream()))
    return out


def fill_condition(masked_latents, mask):
    """FLUX.1 Fill's 320 conditioning channels (B,S,320) f32: the packed latents of the masked image (B,S,64) next to the binarised mask (B,H,W), pixel-
    unshuffled by 8 and packed 2x2 (256 channels); H and W multiples of 16, S = (H/16)(W/16)."""
    masked_latents, mask = masked_latents.to(torch.float32).contiguous(), mask.to(torch.float32).contiguous()
    B, H, W = mask.shape
    if H % 16 or W % 16:
        raise ValueError(f"fill_condition: H and W must be multiples of 16, got {H} x {W}")
    S = (H // 16) * (W // 16)
    if tuple(masked_latents.shape) != (B, S, 64):
        raise ValueError(f"fill_condition: masked_latents is {tuple(masked_latents.shape)}, expected {(B, S, 64)}")
    out = torch.empty((B, S, 320), dtype=torch.float32, device=mask.device)
    L.check(L.load().fmi_fill_condition(_ptr(masked_latents), _ptr(mask), B, H, W, _ptr(out), _stream()))
    return out


def encode_latents(z, scale_factor, shift_factor):
    """The mirror of unpack_latents: z (B,C,h,w) f32 (AutoEncoderKl.encode) -> x0 (B,hw/4,4C) = pack((z - shift_factor) * scale_factor), img_ids (B,hw/4,3)."""
    z = z.to(torch.float32).contiguous()
    B, Cc, h, w = z.shape
    x0 = torch.empty((B, (h // 2) * (w // 2), Cc * 4), dtype=torch.float32, device=z.device)
    ids = torch.empty((B, (h // 2) * (w // 2), 3), dtype=torch.float32, device=z.device)
    L.check(L.load().fmi_encode_latents(_ptr(z), B, Cc, h, w, scale_factor, shift_factor, _ptr(x0), _ptr(ids), _stream()))
    return x0, ids


def latent_ids(B, h2, w2, id0=0.0, row0=0.0, col0=0.0, device="cuda"):
    """Position ids of an (h2, w2) token grid, (B,h2*w2,3) f32 = (id0, row0 + r, col0 + c): pack_latents' ids at the defaults; a reference image's tokens
    take id0 = 1."""
    ids = torch.empty((B, h2 * w2, 3), dtype=torch.float32, device=device)
    L.check(L.load().fmi_latent_ids(B, h2, w2, float(id0), float(row0), float(col0), _ptr(ids), _stream()))
    return ids


def scale_noise(x0, noise, t):
    """(1 - t) * x0 + t * noise in f32 (any shape; the tensors are used as they lie in memory): noise bit for bit at t = 1, x0 at t = 0."""
    if x0.dtype != torch.float32 or noise.dtype != torch.float32 or x0.shape != noise.shape:
        raise TypeError("scale_noise: two float32 tensors of one shape are required")
    if not (x0.is_contiguous() and noise.is_contiguous()):
        x0, noise = x0.contiguous(), noise.contiguous()
    out = torch.empty_like(x0)
    L.check(L.load().fmi_scale_noise(_ptr(x0), _ptr(noise), float(t), x0.numel(), _ptr(out), _stream()))
    return out


def cfg_euler_step(img, pos, neg, scale, dt, x0=None, noise=None, mask=None, s=0.0):
    """The true-CFG step on its own (fmi_cfg_euler_step), in place on img and returning it: g = neg + scale * (pos - neg), img = img + g * dt —
    or with x0 / noise / mask (all three or none) mask * (img + g * dt) + (1 - mask) * ((1 - s) * x0 + s * noise).  float32 tensors of one shape, used as
    they lie in memory (contiguous); pos == neg or scale == 0 steps along neg bit for bit."""
    blend = [t for t in (x0, noise, mask) if t is not None]
    if len(blend) not in (0, 3):
        raise ValueError("cfg_euler_step: x0, noise and mask go together (all three or none)")
    for t in [img, pos, neg] + blend:
        if t.dtype != torch.float32 or t.shape != img.shape or not t.is_contiguous() or t.device != img.device:
            raise TypeError("cfg_euler_step: contiguous float32 tensors of one shape on one device are required")
    L.check(L.load().fmi_cfg_euler_step(_ptr(img), _ptr(pos), _ptr(neg), float(scale), float(dt), img.numel(), _ptr(x0), _ptr(noise), _ptr(mask), float(s), _stream()))
    return img


def _solver_step_tensors(who, img, others, x0, noise, mask):
    blend = [t for t in (x0, noise, mask) if t is not None]
    if len(blend) not in (0, 3):
        raise ValueError(f"{who}: x0, noise and mask go together (all three or none)")
    for t in [img] + [t for t in others if t is not None] + blend:
        if t.dtype != torch.float32 or t.shape != img.shape or not t.is_contiguous() or t.device != img.device:
            raise TypeError(f"{who}: contiguous float32 tensors of one shape on one device are required")


def heun_predict(img, pos, neg=None, scale=1.0, dt=0.0, x0=None, noise=None, mask=None, s=0.0):
    """The Heun predictor on its own (fmi_heun_predict): returns (x_pred, g1), two new tensors; img is only read.  g1 = pos, or with neg
    neg + scale * (pos - neg); x_pred = img + g1 * dt, or with x0 / noise / mask (all three or none) its blend at the target time s, as in cfg_euler_step."""
    _solver_step_tensors("heun_predict", img, (pos, neg), x0, noise, mask)
    x_pred, g1 = torch.empty_like(img), torch.empty_like(img)
    L.check(L.load().fmi_heun_predict(_ptr(img), _ptr(pos), _ptr(neg), float(scale), float(dt), img.numel(), _ptr(x_pred), _ptr(g1), _ptr(x0), _ptr(noise), _ptr(mask),
                                      float(s), _stream()))
    return x_pred, g1


def heun_correct(img, g1, pos, neg=None, scale=1.0, dt=0.0, x0=None, noise=None, mask=None, s=0.0):
    """The Heun corrector on its own (fmi_heun_correct), in place on img and returning it: img = img + ((g1 + g2) * 0.5) * dt with g2 = pos or the guided
    combination of the evaluation on x_pred, blended like the predictor's."""
    _solver_step_tensors("heun_correct", img, (g1, pos, neg), x0, noise, mask)
    L.check(L.load().fmi_heun_correct(_ptr(img), _ptr(g1), _ptr(pos), _ptr(neg), float(scale), float(dt), img.numel(), _ptr(x0), _ptr(noise), _ptr(mask), float(s),
                                      _stream()))
    return img


def dpmpp_2m_step(img, pos, history, t, a, c, w, neg=None, scale=1.0, x0=None, noise=None, mask=None, s=0.0):
    """The DPM-Solver++ 2M step on its own (fmi_dpmpp_2m_step), in place on img and history, returning img: D = img - t * g, D' = D + w * (D - history) (w == 0: the
    history is not read), img = a * img + c * D', blended; history = D.  a, c, w: dpmpp_2m_coefficients."""
    _solver_step_tensors("dpmpp_2m_step", img, (pos, neg, history), x0, noise, mask)
    L.check(L.load().fmi_dpmpp_2m_step(_ptr(img), _ptr(pos), _ptr(neg), float(scale), float(t), float(a), float(c), float(w), img.numel(), _ptr(history), _ptr(x0),
                                       _ptr(noise), _ptr(mask), float(s), _stream()))
    return img


def dpmpp_2m_coefficients(timesteps, i: int):
    """(a, c, w) of step i of the schedule, as the library's loop uses them (fmi_dpmpp_2m_coefficients: computed in double, rounded once to float32).  No device."""
    ts = (C.c_double * len(timesteps))(*timesteps)
    a, c, w = C.c_float(), C.c_float(), C.c_float()
    L.check(L.load().fmi_dpmpp_2m_coefficients(ts, len(timesteps) - 1, int(i), C.byref(a), C.byref(c), C.byref(w)))
    return a.value, c.value, w.value


def randn_latents(B, Cc, h, w, seed, first_sample=0, device="cuda"):
    """Seedable get_noise (flux/sampling.rs:5-14): Philox4x32-10, sample index = first_sample + b."""
    out = torch.empty((B, Cc, h, w), dtype=torch.float32, device=device)
    L.check(L.load().fmi_randn(_ptr(out), Cc * h * w, B, seed, first_sample, _stream()))
    return out
