"""stable-diffusion-xl-burn_amd -- MI355X-native SDXL sampling engine, host-side mirror of the reference API.

The product is ``lib/libsdxl_mi355.so`` (hand-written HIP kernels for gfx950 + a C++ engine behind the C ABI of
``include/sdxl_mi355.h``).  This module is the thin ctypes binding the test-suite and ``bench.py`` drive -- the same
symbols a Rust ``cc``+``bindgen`` shim would bind -- exposed under the reference's own names
(``Diffuser.sample_latent`` / ``UNet.forward`` / ``LatentDecoder.latent_to_image`` / ``Conditioning`` / ``RawImages`` /
``qkv_attention``; reference src/model/stablediffusion/mod.rs, src/model/unet/mod.rs, src/backend.rs).

PyTorch appears here only as plumbing (device buffers, streams, torch.distributed); no arithmetic of the hot path runs
in torch, and there is NO fallback: if the HIP library is missing or no GPU is visible every entry point raises.
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# SDXL_MEASURE_LIB=1 (tools/ only): the measurement build (`build.py --measure`: A/B partners, measurement modes, timeline stamps)
LIB_PATH = os.path.join(_HERE, "lib", "libsdxl_mi355_measure.so" if os.environ.get("SDXL_MEASURE_LIB") == "1" else "libsdxl_mi355.so")
if os.environ.get("SDXL_LIB_PATH"):      # tools/ only: an explicitly named build of the same library (A/B of two commits on one box)
    LIB_PATH = os.environ["SDXL_LIB_PATH"]

DTYPE_F32 = 0        # strict parity: fp32 storage + exact fp32 MFMA
DTYPE_F16 = 1        # fp16 storage / MFMA operands, fp32 accumulate
DTYPE_F16_F32RES = 2  # fp16 MFMA operands, fp32 residual stream
DTYPE_F32_SPLIT_MIX_F16W = 5  # DTYPE_F32_SPLIT_MIX for f16-representable parameters (the reference's records): + QKV projection, both out-projections, FF-out, cross-attention query projection on f16 operands, LayerNorms through an f16 shadow (csrc/capi_internal.h mix_of); falls back to _MIX's classes on other parameters (UNet.mix_classes())
DTYPE_F32_SPLIT_MIX_F16W_GEGLU2 = 6  # DTYPE_F32_SPLIT_MIX_F16W with the GEGLU projection's activations as (hi, lo) f16 pairs along a doubled K: ~12 % slower, inside the scaled bound on every fixture incl. the 4-step stress one
DTYPE_F32_SPLIT_F16W = 7  # DTYPE_F32_SPLIT for f16-representable parameters: same fp32-class arithmetic, the transformer's linear layers on the f16 kernels (HL16 rows read as f16 rows of twice the width), fused split-precision cross-attention; falls back to DTYPE_F32_SPLIT on other parameters
DTYPE_F32_SPLIT_MIX = 4  # UNet / Diffuser: DTYPE_F32_SPLIT with the self-attention and the GEGLU projection on plain f16 operands (the two classes the measured precision frontier affords)
DTYPE_F32_SPLIT = 3   # fp32-class arithmetic on the f16 matrix pipe (operands as (hi, lo) f16 pairs, 3 MFMAs per product): UNet / Diffuser / LatentDecoder and the conv2d / linear / qkv_attention operators

_c_p = ctypes.c_void_p
_f_p = ctypes.c_void_p   # device pointers travel as integers


SEED_F16_WEIGHTS = 1 << 63   # include/sdxl_mi355.h SDXL_SEED_F16_WEIGHTS: synthetic parameters rounded to f16 (what a real record holds)


class EngineError(RuntimeError):
    pass


class _UNetConfigC(ctypes.Structure):
    _fields_ = [("adm_in_channels", ctypes.c_int32), ("in_channels", ctypes.c_int32), ("out_channels", ctypes.c_int32),
                ("model_channels", ctypes.c_int32), ("n_levels", ctypes.c_int32), ("channel_mults", ctypes.c_int32 * 8),
                ("n_head_channels", ctypes.c_int32), ("transformer_depths", ctypes.c_int32 * 8),
                ("context_dim", ctypes.c_int32), ("is_refiner", ctypes.c_int32)]


class _VaeConfigC(ctypes.Structure):
    _fields_ = [("n_blocks", ctypes.c_int32), ("enc_in", ctypes.c_int32 * 8), ("enc_out", ctypes.c_int32 * 8),
                ("dec_in", ctypes.c_int32 * 8), ("dec_out", ctypes.c_int32 * 8), ("n_group", ctypes.c_int32),
                ("enc_out_channels", ctypes.c_int32), ("scale_factor", ctypes.c_double)]


class _ClipConfigC(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("n_vocab", "n_state", "embed_dim", "n_head", "n_ctx", "n_layer", "quick_gelu")]


class _ConditioningC(ctypes.Structure):
    _fields_ = [("unconditional_context_full", _f_p), ("unconditional_context_open_clip", _f_p),
                ("context_full", _f_p), ("context_open_clip", _f_p), ("unconditional_channel_context", _f_p),
                ("unconditional_channel_context_refiner", _f_p), ("channel_context", _f_p),
                ("channel_context_refiner", _f_p), ("n", ctypes.c_int32), ("n_ctx", ctypes.c_int32),
                ("height", ctypes.c_int32), ("width", ctypes.c_int32)]


class LoraEntry(ctypes.Structure):
    """sdxl_lora_entry: W += scale * left[rows, rank] @ right[rank, cols] on the matrix view of parameter `param_index` (lora_entry builds one
    from PyTorch-style adapter tensors and keeps the arrays alive)"""
    _fields_ = [("param_index", ctypes.c_int32), ("rank", ctypes.c_int32), ("left", _f_p), ("right", _f_p), ("scale", ctypes.c_float)]


class Guidance(ctypes.Structure):
    """sdxl_guidance: a Diffuser handle's guidance options (Diffuser.set_guidance builds one from keywords; guidance_default() is the default)"""
    _fields_ = [("mode", ctypes.c_int32), ("rescale", ctypes.c_float), ("n_scales", ctypes.c_int32), ("scales", ctypes.c_float * 8),
                ("t_lo", ctypes.c_int32), ("t_hi", ctypes.c_int32)]

    def __eq__(self, other):
        return isinstance(other, Guidance) and bytes(self) == bytes(other)

    def __repr__(self):
        return (f"Guidance(mode={self.mode}, rescale={self.rescale}, scales={list(self.scales)[:self.n_scales]}, "
                f"t_range=({self.t_lo}, {self.t_hi}))")


class Control(ctypes.Structure):
    """sdxl_control: how a control net's residuals enter a trajectory, as a scale per iteration and batch entry (make_control builds one from
    keywords; control_default() is the default)"""
    _fields_ = [("scale", ctypes.c_float), ("n_scales", ctypes.c_int32), ("scales", ctypes.c_float * 8), ("t_lo", ctypes.c_int32),
                ("t_hi", ctypes.c_int32), ("cond_only", ctypes.c_int32)]

    def __eq__(self, other):
        return isinstance(other, Control) and bytes(self) == bytes(other)

    def __repr__(self):
        return (f"Control(scale={self.scale}, scales={list(self.scales)[:self.n_scales]}, t_range=({self.t_lo}, {self.t_hi}), "
                f"cond_only={bool(self.cond_only)})")


MAX_CONTROLS = 4     # SDXL_MAX_CONTROLS


GUIDANCE_CFG = 0     # SDXL_GUIDANCE_CFG: classifier-free guidance (default)
GUIDANCE_OFF = 1     # SDXL_GUIDANCE_OFF: the conditional branch alone (distilled checkpoints); unconditional tensors may be None
_GUIDANCE_MODES = {"cfg": GUIDANCE_CFG, "off": GUIDANCE_OFF}

LORA_ROUND_F16 = 1   # SDXL_LORA_ROUND_F16: adapted tensors rounded to f16 values after merging (what a half-precision record saved after merging holds)


# every symbol include/sdxl_mi355.h declares (tests check the library exports all of them)
ABI_SYMBOLS = [
    "sdxl_last_error", "sdxl_build_info", "sdxl_ctx_create", "sdxl_ctx_destroy", "sdxl_ctx_synchronize",
    "sdxl_unet_config_base", "sdxl_unet_config_refiner", "sdxl_vae_config_default",
    "sdxl_unet_param_count", "sdxl_unet_param_spec", "sdxl_vae_param_count", "sdxl_vae_param_spec",
    "sdxl_unet_create", "sdxl_unet_create_synthetic", "sdxl_unet_destroy", "sdxl_unet_forward", "sdxl_unet_set_graph", "sdxl_unet_set_split_cfg", "sdxl_unet_set_fused_cross_attention", "sdxl_unet_set_gn_from_producer", "sdxl_unet_mix_classes", "sdxl_unet_block",
    "sdxl_qkv_attention", "sdxl_attn_decoder_mask",
    "sdxl_diffuser_create", "sdxl_diffuser_create_synthetic", "sdxl_diffuser_destroy", "sdxl_diffuser_unet",
    "sdxl_sample_latent", "sdxl_sample_latent_with_inpainting", "sdxl_refine_latent", "sdxl_step_count",
    "sdxl_diffuser_enable_step_timing", "sdxl_diffuser_step_times", "sdxl_diffuser_set_trace",
    "sdxl_gen_noise", "sdxl_sample_latent_seeded", "sdxl_sample_latent_with_inpainting_seeded", "sdxl_refine_latent_seeded",
    "sdxl_diffuser_set_solver", "sdxl_diffuser_get_solver", "sdxl_solver_coefficients",
    "sdxl_guidance_default", "sdxl_guidance_check", "sdxl_diffuser_set_guidance", "sdxl_diffuser_get_guidance", "sdxl_cfg_rescale_factors",
    "sdxl_sampler_step_replay",
    "sdxl_diffuser_set_prediction", "sdxl_diffuser_get_prediction", "sdxl_rescale_zero_terminal_snr", "sdxl_solver_coefficients_pred",
    "sdxl_sampler_step_replay_pred",
    "sdxl_diffuser_set_timesteps", "sdxl_diffuser_get_timesteps", "sdxl_timestep_schedule", "sdxl_solver_coefficients_ts",
    "sdxl_sampler_step_replay_ts",
    "sdxl_diffuser_set_sigmas", "sdxl_diffuser_get_sigmas", "sdxl_diffuser_set_timesteps_end", "sdxl_diffuser_get_timesteps_end", "sdxl_sigma_schedule",
    "sdxl_sigma_to_timestep", "sdxl_continue_latent", "sdxl_solver_rows", "sdxl_sampler_step_replay_levels",
    "sdxl_vae_create", "sdxl_vae_create_synthetic", "sdxl_vae_destroy", "sdxl_vae_decode_latent",
    "sdxl_latent_to_image", "sdxl_vae_encode_image", "sdxl_image_to_latent",
    "sdxl_unet_weight_arena", "sdxl_vae_weight_arena", "sdxl_diffuser_create_empty", "sdxl_vae_create_empty",
    "sdxl_unet_profile", "sdxl_unet_eager_forward_ms", "sdxl_bench_igemm", "sdxl_bench_attention", "sdxl_debug_set", "sdxl_debug_warm_schedule", "sdxl_debug_upsample_fold", "sdxl_debug_weight_layout", "sdxl_conv2d_upsample_folded", "sdxl_debug_igemm_select", "sdxl_debug_attn_select",
    "sdxl_group_norm", "sdxl_layer_norm", "sdxl_conv2d", "sdxl_linear", "sdxl_gemv", "sdxl_timestep_embedding", "sdxl_vae_attn_block", "sdxl_vae_res_block", "sdxl_layer_norm_linear", "sdxl_ln_query_cross_attention", "sdxl_conv2d_group_norm",
    "sdxl_transformer_projection",
    "sdxl_unet_skip_count", "sdxl_unet_skip_shape", "sdxl_unet_forward_residuals", "sdxl_skip_residual_add",
    "sdxl_skip_residual_add_steps", "sdxl_control_default", "sdxl_control_check",
    "sdxl_skip_residual_add_steps_multi", "sdxl_control_scale_table",
    "sdxl_controlnet_config_default", "sdxl_controlnet_param_count", "sdxl_controlnet_param_spec", "sdxl_controlnet_create", "sdxl_controlnet_create_f16",
    "sdxl_controlnet_create_synthetic", "sdxl_controlnet_destroy", "sdxl_controlnet_embed_hint", "sdxl_controlnet_forward",
    "sdxl_lora_check", "sdxl_lora_merge", "sdxl_unet_create_lora", "sdxl_diffuser_create_lora",
    "sdxl_clip_config_clip_l", "sdxl_clip_config_open_clip_bigg", "sdxl_clip_param_count", "sdxl_clip_param_spec",
    "sdxl_clip_create", "sdxl_clip_create_synthetic", "sdxl_clip_destroy", "sdxl_clip_forward_hidden",
    "sdxl_clip_forward_hidden_pooled", "sdxl_conditioning_embedding", "sdxl_clip_weight_arena",
    "sdxl_unet_create_f16", "sdxl_diffuser_create_f16", "sdxl_vae_create_f16", "sdxl_clip_create_f16",
    "sdxl_comm_unique_id", "sdxl_comm_create", "sdxl_comm_destroy", "sdxl_bcast_buffer", "sdxl_unet_bcast_weights",
    "sdxl_vae_bcast_weights", "sdxl_clip_bcast_weights", "sdxl_bcast_plan",
]

_lib = None


def lib() -> ctypes.CDLL:
    """Loads the HIP engine; fails loudly when it has not been built (no CPU / eager fallback exists)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise EngineError(f"{LIB_PATH} is missing: run `python stable-diffusion-xl-burn_amd/build.py` "
                              "(hipcc --offload-arch=gfx950). There is no fallback path.")
        # torch's ROCm wheel bundles its own libamdhip64: it must be in the process BEFORE this library is loaded, so both
        # bind to ONE HIP runtime.  Loaded the other way round (library first, torch later) the process ends up with two
        # runtimes and the second one reports "no ROCm-capable device" (seen with build() followed by smoke() in one process).
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        l = ctypes.CDLL(LIB_PATH)
        l.sdxl_last_error.restype = ctypes.c_char_p
        l.sdxl_build_info.restype = ctypes.c_char_p
        l.sdxl_diffuser_unet.restype = ctypes.c_void_p
        l.sdxl_diffuser_unet.argtypes = [ctypes.c_void_p]
        for name in ("sdxl_ctx_destroy", "sdxl_unet_destroy", "sdxl_diffuser_destroy", "sdxl_vae_destroy", "sdxl_clip_destroy",
                     "sdxl_comm_destroy"):
            getattr(l, name).restype = None
            getattr(l, name).argtypes = [ctypes.c_void_p]
        if hasattr(l, "sdxl_solver_coefficients"):   # SDXL_LIB_PATH may name an older build (tools/): it fails at the call, not at the load
            l.sdxl_diffuser_set_solver.argtypes = [ctypes.c_void_p, ctypes.c_int]
            l.sdxl_diffuser_get_solver.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
            l.sdxl_solver_coefficients.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double,
                                                   ctypes.c_void_p, ctypes.c_int]
        if hasattr(l, "sdxl_cfg_rescale_factors"):
            l.sdxl_guidance_default.restype = None
            l.sdxl_guidance_default.argtypes = [ctypes.POINTER(Guidance)]
            l.sdxl_guidance_check.argtypes = [ctypes.POINTER(Guidance), ctypes.c_int]
            l.sdxl_diffuser_set_guidance.argtypes = [ctypes.c_void_p, ctypes.POINTER(Guidance)]
            l.sdxl_diffuser_get_guidance.argtypes = [ctypes.c_void_p, ctypes.POINTER(Guidance)]
            l.sdxl_cfg_rescale_factors.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                                   ctypes.c_float, ctypes.c_void_p]
        if hasattr(l, "sdxl_sampler_step_replay"):
            l.sdxl_sampler_step_replay.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        if hasattr(l, "sdxl_solver_coefficients_pred"):
            l.sdxl_diffuser_set_prediction.argtypes = [ctypes.c_void_p, ctypes.c_int]
            l.sdxl_diffuser_get_prediction.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
            l.sdxl_rescale_zero_terminal_snr.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
            l.sdxl_solver_coefficients_pred.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                        ctypes.c_double, ctypes.c_void_p, ctypes.c_int]
            l.sdxl_sampler_step_replay_pred.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
        if hasattr(l, "sdxl_solver_coefficients_ts"):
            l.sdxl_diffuser_set_timesteps.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
            l.sdxl_diffuser_get_timesteps.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
            l.sdxl_timestep_schedule.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
            l.sdxl_solver_coefficients_ts.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                      ctypes.c_double, ctypes.c_void_p, ctypes.c_int]
            l.sdxl_sampler_step_replay_ts.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
        if hasattr(l, "sdxl_solver_rows"):
            l.sdxl_diffuser_set_sigmas.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_int]
            l.sdxl_diffuser_get_sigmas.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)]
            l.sdxl_diffuser_set_timesteps_end.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
            l.sdxl_diffuser_get_timesteps_end.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
            l.sdxl_sigma_schedule.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                              ctypes.c_void_p, ctypes.c_int]
            l.sdxl_sigma_to_timestep.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.POINTER(ctypes.c_double)]
            l.sdxl_continue_latent.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, ctypes.c_int,
                                               ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, ctypes.c_int, ctypes.c_void_p]
            l.sdxl_solver_rows.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_void_p, ctypes.c_int]
            l.sdxl_sampler_step_replay_levels.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
        if hasattr(l, "sdxl_unet_forward_residuals"):
            l.sdxl_unet_skip_shape.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
            l.sdxl_unet_forward_residuals.argtypes = [ctypes.c_void_p] * 6 + [ctypes.c_int] * 4 + [ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p]
            l.sdxl_skip_residual_add.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 6 + [ctypes.c_int]
            l.sdxl_controlnet_destroy.restype = None
            l.sdxl_controlnet_destroy.argtypes = [ctypes.c_void_p]
            l.sdxl_controlnet_config_default.restype = None
        if hasattr(l, "sdxl_skip_residual_add_steps"):
            l.sdxl_skip_residual_add_steps.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 5 + \
                [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
            l.sdxl_control_default.restype = None
            l.sdxl_control_default.argtypes = [ctypes.POINTER(Control)]
            l.sdxl_control_check.argtypes = [ctypes.POINTER(Control), ctypes.c_int]
        if hasattr(l, "sdxl_skip_residual_add_steps_multi"):
            l.sdxl_skip_residual_add_steps_multi.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 3 + [ctypes.c_int] + \
                [ctypes.c_void_p] * 2 + [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
            l.sdxl_control_scale_table.argtypes = [ctypes.POINTER(Control), ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
        _lib = l
    return _lib


def _check(rc: int):
    if rc != 0:
        raise EngineError(lib().sdxl_last_error().decode())


def _torch():
    import torch
    return torch


def _dev(t, dtype=None):
    """contiguous CUDA tensor of the expected dtype -> (tensor kept alive, device pointer)"""
    torch = _torch()
    if dtype is None:
        dtype = torch.float32
    if not t.is_cuda:
        raise EngineError("expected a CUDA (ROCm) tensor: the engine has no CPU path")
    t = t.to(dtype).contiguous()
    return t, ctypes.c_void_p(t.data_ptr())


def _stream() -> ctypes.c_void_p:
    s = _torch().cuda.current_stream().cuda_stream
    return ctypes.c_void_p(s if s else None)


# ----------------------------------------------------------------------------------------------------------------

@dataclass
class UNetConfig:
    """reference UNetConfig (unet/mod.rs:59-69) + DiffuserConfig.is_refiner (stablediffusion/mod.rs:269-278)"""
    adm_in_channels: int
    model_channels: int
    channel_mults: List[int]
    n_head_channels: int
    transformer_depths: List[int]
    context_dim: int
    in_channels: int = 4
    out_channels: int = 4
    is_refiner: bool = False

    def to_c(self) -> _UNetConfigC:
        c = _UNetConfigC()
        c.adm_in_channels, c.in_channels, c.out_channels = self.adm_in_channels, self.in_channels, self.out_channels
        c.model_channels, c.n_levels = self.model_channels, len(self.channel_mults)
        for i, (m, d) in enumerate(zip(self.channel_mults, self.transformer_depths)):
            c.channel_mults[i] = m
            c.transformer_depths[i] = d
        c.n_head_channels, c.context_dim, c.is_refiner = self.n_head_channels, self.context_dim, int(self.is_refiner)
        return c


def sdxl_base_config() -> UNetConfig:
    return UNetConfig(2816, 320, [1, 2, 4], 64, [0, 2, 10], 2048)


def sdxl_refiner_config() -> UNetConfig:
    return UNetConfig(2560, 384, [1, 2, 4, 4], 64, [0, 4, 4, 4], 1280, is_refiner=True)


@dataclass
class VAEConfig:
    enc_channels: List[Tuple[int, int]] = field(default_factory=lambda: [(128, 128), (128, 256), (256, 512), (512, 512)])
    dec_channels: List[Tuple[int, int]] = field(default_factory=lambda: [(512, 512), (512, 512), (512, 256), (256, 128)])
    n_group: int = 32
    enc_out_channels: int = 8
    scale_factor: float = 0.13025

    def to_c(self) -> _VaeConfigC:
        c = _VaeConfigC()
        c.n_blocks = len(self.dec_channels)
        for i, ((ei, eo), (di, do)) in enumerate(zip(self.enc_channels, self.dec_channels)):
            c.enc_in[i], c.enc_out[i], c.dec_in[i], c.dec_out[i] = ei, eo, di, do
        c.n_group, c.enc_out_channels, c.scale_factor = self.n_group, self.enc_out_channels, self.scale_factor
        return c


@dataclass
class ParamSpec:
    name: str
    shape: Tuple[int, ...]
    kind: int
    scale: float
    mean: float


def _specs(count_fn, spec_fn) -> List[ParamSpec]:
    n = count_fn()
    if n < 0:
        raise EngineError(lib().sdxl_last_error().decode())
    out = []
    name = ctypes.c_char_p()
    ndim, kind = ctypes.c_int(), ctypes.c_int()
    shape = (ctypes.c_int64 * 4)()
    sc, mean = ctypes.c_float(), ctypes.c_float()
    for i in range(n):
        _check(spec_fn(i, ctypes.byref(name), ctypes.byref(ndim), shape, ctypes.byref(kind), ctypes.byref(sc),
                       ctypes.byref(mean)))
        out.append(ParamSpec(name.value.decode(), tuple(int(shape[j]) for j in range(ndim.value)), kind.value,
                             sc.value, mean.value))
    return out


def unet_param_specs(cfg: UNetConfig) -> List[ParamSpec]:
    """host-only (no GPU needed): the order / layouts sdxl_unet_create expects its flat weight buffer in"""
    c = cfg.to_c()
    l = lib()
    return _specs(lambda: l.sdxl_unet_param_count(ctypes.byref(c)),
                  lambda i, *a: l.sdxl_unet_param_spec(ctypes.byref(c), i, *a))


class _ControlNetConfigC(ctypes.Structure):
    _fields_ = [("unet", _UNetConfigC), ("hint_in_channels", ctypes.c_int32), ("hint_channels", ctypes.c_int32 * 4)]


@dataclass
class ControlNetConfig:
    """sdxl_controlnet_config: a ControlNet for the UNet `unet` -- that UNet's encoder, a hint embedder (hint_in_channels -> hint_channels ->
    model_channels, 8x down) and one 1x1 convolution per residual tensor"""
    unet: UNetConfig
    hint_in_channels: int = 3
    hint_channels: Tuple[int, int, int, int] = (16, 32, 96, 256)

    def to_c(self) -> _ControlNetConfigC:
        c = _ControlNetConfigC()
        c.unet = self.unet.to_c()
        c.hint_in_channels = int(self.hint_in_channels)
        for i, v in enumerate(self.hint_channels):
            c.hint_channels[i] = int(v)
        return c


def controlnet_param_specs(cfg: ControlNetConfig) -> List[ParamSpec]:
    """host-only (no GPU needed): the order / layouts sdxl_controlnet_create expects its flat weight buffer in"""
    c = cfg.to_c()
    l = lib()
    return _specs(lambda: l.sdxl_controlnet_param_count(ctypes.byref(c)),
                  lambda i, *a: l.sdxl_controlnet_param_spec(ctypes.byref(c), i, *a))


def vae_param_specs(cfg: VAEConfig, encoder: bool) -> List[ParamSpec]:
    c = cfg.to_c()
    l = lib()
    return _specs(lambda: l.sdxl_vae_param_count(ctypes.byref(c), int(encoder)),
                  lambda i, *a: l.sdxl_vae_param_spec(ctypes.byref(c), int(encoder), i, *a))


def clip_param_specs(cfg: "CLIPConfig") -> List[ParamSpec]:
    c = cfg.to_c()
    l = lib()
    return _specs(lambda: l.sdxl_clip_param_count(ctypes.byref(c)),
                  lambda i, *a: l.sdxl_clip_param_spec(ctypes.byref(c), i, *a))


def step_count(n_steps: int, step_start: int = 0, n_train: int = 1000) -> int:
    return lib().sdxl_step_count(n_steps, step_start, n_train)


def flatten_weights(specs: Sequence[ParamSpec], weights: dict) -> np.ndarray:
    """name -> ndarray (reference layouts) => the flat fp32 buffer of the C ABI"""
    parts = []
    for p in specs:
        w = np.asarray(weights[p.name], dtype=np.float32)
        if tuple(w.shape) != tuple(p.shape):
            raise EngineError(f"{p.name}: expected shape {p.shape}, got {w.shape}")
        parts.append(w.reshape(-1))
    return np.ascontiguousarray(np.concatenate(parts))


class Context:
    """one per GPU (reference: LibTorchDevice::Cuda(0), src/bin/sample/main.rs:131)"""

    def __init__(self, device_id: int = 0):
        self.h = ctypes.c_void_p()
        _check(lib().sdxl_ctx_create(device_id, ctypes.byref(self.h)))
        self.device_id = device_id

    def synchronize(self):
        _check(lib().sdxl_ctx_synchronize(self.h))

    def __del__(self):
        if getattr(self, "h", None) and self.h and _lib is not None:
            _lib.sdxl_ctx_destroy(self.h)
            self.h = None


@dataclass
class Conditioning:
    """reference Conditioning<B> (stablediffusion/mod.rs:544-555); CUDA fp32 tensors of the same ranks"""
    context_full: "object" = None                       # [n,77,ctx_full]
    channel_context: "object" = None                    # [n,adm]
    unconditional_context_full: "object" = None         # [77,ctx_full]
    unconditional_channel_context: "object" = None      # [adm]
    context_open_clip: "object" = None                  # [n,77,1280]
    channel_context_refiner: "object" = None
    unconditional_context_open_clip: "object" = None
    unconditional_channel_context_refiner: "object" = None
    resolution: Tuple[int, int] = (1024, 1024)          # (height, width)

    def to_c(self):
        keep = []
        c = _ConditioningC()
        first = None
        for name in ("unconditional_context_full", "unconditional_context_open_clip", "context_full", "context_open_clip",
                     "unconditional_channel_context", "unconditional_channel_context_refiner", "channel_context",
                     "channel_context_refiner"):
            t = getattr(self, name)
            if t is None:
                setattr(c, name, None)
                continue
            t, p = _dev(t)
            keep.append(t)
            setattr(c, name, p)
            if name in ("context_full", "context_open_clip") and first is None:
                first = t
        if first is None:
            raise EngineError("Conditioning needs context_full or context_open_clip")
        c.n, c.n_ctx = int(first.shape[0]), int(first.shape[1])
        c.height, c.width = int(self.resolution[0]), int(self.resolution[1])
        return c, keep


class InvalidArgument(EngineError):
    """SDXL_ERR_INVALID: arguments outside what the entry supports"""


def _check_invalid(rc: int):
    if rc == 1:
        raise InvalidArgument(lib().sdxl_last_error().decode())
    _check(rc)


# ---------------------------------------------------------------------------------------------------------------- adapters

def param_index(specs: Sequence[ParamSpec], name: str) -> int:
    """index of parameter `name` in a spec list (unet_param_specs): the param_index of a LoraEntry"""
    for i, p in enumerate(specs):
        if p.name == name:
            return i
    raise EngineError(f"unknown parameter {name!r}")


def _f32_matrix(a, transpose: bool):
    """(contiguous fp32 2-d array kept alive, pointer): numpy arrays stay on the host, torch tensors stay where they are (host or device)"""
    if hasattr(a, "data_ptr"):      # torch tensor
        torch = _torch()
        t = a.detach().to(torch.float32).reshape(a.shape[0], -1)
        t = (t.t() if transpose else t).contiguous()
        return t, ctypes.c_void_p(t.data_ptr())
    n = np.asarray(a, dtype=np.float32)
    n = n.reshape(n.shape[0], -1)
    n = np.ascontiguousarray(n.T if transpose else n)
    return n, n.ctypes.data_as(ctypes.c_void_p)


def lora_entry(spec_index: int, down_weight, up_weight, alpha: Optional[float] = None, strength: float = 1.0) -> LoraEntry:
    """A LoraEntry from the usual PyTorch adapter pair, numpy arrays or torch tensors (host or device):
      Linear (down_weight [r, d_in], up_weight [d_out, r]) on a [d_in, d_out] parameter: left = down^T, right = up^T;
      Conv2d (down_weight [r, Cin, kh, kw] -- four dimensions --, up_weight [Cout, r] or [Cout, r, 1, 1]) on a [Cout, Cin, kh, kw] parameter:
      left = up, right = down flattened to [r, Cin * kh * kw].
    scale = strength * alpha / r (alpha defaults to r).  The C ABI cannot see the arrays' extents; UNet / Diffuser compare the shapes recorded here
    with the parameter's matrix view before they hand the entries over."""
    conv = len(down_weight.shape) == 4
    rank = int(down_weight.shape[0])
    if int(up_weight.shape[1]) != rank:
        raise EngineError(f"lora_entry: down_weight has rank {rank}, up_weight {tuple(up_weight.shape)}")
    if conv:
        left, pl = _f32_matrix(up_weight, False)
        right, pr = _f32_matrix(down_weight, False)
    else:
        left, pl = _f32_matrix(down_weight, True)
        right, pr = _f32_matrix(up_weight, True)
    e = LoraEntry(int(spec_index), rank, pl, pr, float(strength) * float(rank if alpha is None else alpha) / rank)
    e.keep = (left, right)      # the arrays the pointers name
    e.left_shape, e.right_shape = tuple(left.shape), tuple(right.shape)
    return e


def _lora_array(entries: Sequence[LoraEntry], cfg: Optional[UNetConfig] = None):
    """(sdxl_lora_entry array, count); with cfg: the shapes lora_entry recorded must fit the parameter (a wrong extent would read past the arrays)"""
    n = len(entries)
    if cfg is not None and n:
        specs = unet_param_specs(cfg)
        for i, e in enumerate(entries):
            if 0 <= e.param_index < len(specs) and hasattr(e, "left_shape"):
                shape = specs[e.param_index].shape
                rows, cols = int(shape[0]), int(np.prod(shape[1:], dtype=np.int64))
                if e.left_shape != (rows, e.rank) or e.right_shape != (e.rank, cols):
                    raise EngineError(f"lora entry {i}: {specs[e.param_index].name} {tuple(shape)} takes left {(rows, e.rank)} and right {(e.rank, cols)}, "
                                      f"got {e.left_shape} and {e.right_shape}")
    return ((LoraEntry * n)(*entries) if n else None), n


def _lora_base(weights):
    """(weights_flat, weights_flat_f16, array kept alive) of the *_create_lora calls: at most one base, none = the synthetic seed"""
    if weights is None:
        return None, None, None
    if np.asarray(weights).dtype == np.float16:
        w = np.ascontiguousarray(weights)
        return None, w.ctypes.data_as(ctypes.c_void_p), w
    w = np.ascontiguousarray(weights, dtype=np.float32)
    return w.ctypes.data_as(ctypes.c_void_p), None, w


def lora_check(cfg: UNetConfig, entries: Sequence[LoraEntry]):
    """sdxl_lora_check (host logic, no GPU needed): raises InvalidArgument with the first complaint"""
    c = cfg.to_c()
    arr, n = _lora_array(entries)
    _check_invalid(lib().sdxl_lora_check(ctypes.byref(c), arr, n))


def lora_merge(ctx: Context, w, left, right, scale: float, flags: int = 0):
    """sdxl_lora_merge, the op the models run at create time: returns w + scale * left @ right on the matrix view of w (rows = w.shape[0]) as a new
    CUDA tensor of w's shape (w itself is not written); left [rows, rank], right [rank, cols]: numpy arrays or torch tensors, host or device."""
    w, _ = _dev(w)
    out = w.clone()
    left, pl = _f32_matrix(left, False)
    right, pr = _f32_matrix(right, False)
    rows = int(out.shape[0])
    cols = int(out.numel() // rows) if rows else 0
    if tuple(left.shape) != (rows, int(right.shape[0])) or int(right.shape[1]) != cols:
        raise EngineError(f"lora_merge: w {tuple(out.shape)}, left {tuple(left.shape)}, right {tuple(right.shape)}")
    _check_invalid(lib().sdxl_lora_merge(ctx.h, _stream(), ctypes.c_void_p(out.data_ptr()), rows, cols, pl, pr, int(right.shape[0]),
                                         ctypes.c_float(scale), int(flags)))
    _torch().cuda.synchronize()
    return out


class UNet:
    """reference UNet<B> (src/model/unet/mod.rs:432-493)"""

    def __init__(self, ctx: Context, cfg: UNetConfig, dtype: int = DTYPE_F16, weights: Optional[np.ndarray] = None,
                 seed: int = 0, _borrowed=None, lora: Optional[Sequence[LoraEntry]] = None, lora_flags: int = 0):
        """lora: LoraEntry list (lora_entry) merged into the weights while the model is built, in the order given; lora_flags: LORA_ROUND_F16"""
        self.ctx, self.cfg, self.dtype = ctx, cfg, dtype
        self._owned = _borrowed is None
        if _borrowed is not None:
            self.h = _borrowed
            return
        self.h = ctypes.c_void_p()
        c = cfg.to_c()
        if lora is not None:
            wf, wf16, keep = _lora_base(weights)
            arr, n = _lora_array(lora, cfg)
            _check_invalid(lib().sdxl_unet_create_lora(ctx.h, ctypes.byref(c), dtype, wf, wf16, ctypes.c_uint64(seed), arr, n, int(lora_flags),
                                                       ctypes.byref(self.h)))
        elif weights is None:
            _check(lib().sdxl_unet_create_synthetic(ctx.h, ctypes.byref(c), dtype, ctypes.c_uint64(seed), ctypes.byref(self.h)))
        elif np.asarray(weights).dtype == np.float16:     # flat f16 (burn HalfPrecisionSettings records): no fp32 expansion
            w = np.ascontiguousarray(weights)
            _check(lib().sdxl_unet_create_f16(ctx.h, ctypes.byref(c), dtype, w.ctypes.data_as(ctypes.c_void_p), ctypes.byref(self.h)))
        else:
            w = np.ascontiguousarray(weights, dtype=np.float32)
            _check(lib().sdxl_unet_create(ctx.h, ctypes.byref(c), dtype, w.ctypes.data_as(ctypes.c_void_p), ctypes.byref(self.h)))

    def forward(self, x, timesteps, context, label):
        """UNet::forward(x[B,4,H,W], timesteps[B] int, context[B,n_ctx,ctx], label[B,adm]) -> [B,4,H,W]  (:450-492)"""
        torch = _torch()
        x, px = _dev(x)
        ts, pt = _dev(timesteps, torch.int32)
        context, pc = _dev(context)
        label, pl = _dev(label)
        B, _, H, W = x.shape
        out = torch.empty((B, self.cfg.out_channels, H, W), device=x.device, dtype=torch.float32)
        _check(lib().sdxl_unet_forward(self.h, _stream(), px, pt, pc, pl, B, H, W, int(context.shape[1]),
                                      ctypes.c_void_p(out.data_ptr())))
        return out

    def forward_residuals(self, x, timesteps, context, label, residuals, scale: float = 1.0):
        """sdxl_unet_forward_residuals: forward with ControlNet skip residuals given by the caller -- a list of unet_skip_shapes(cfg, H, W) tensors
        [B,C,h,w] (one per input entry, then the middle block's); scale * r is added into what the decoder reads, in one launch behind the middle
        block.  The handle keeps them attached (another scale or other values replay the captured graph); residuals=None, or forward(), detaches."""
        torch = _torch()
        x, px = _dev(x)
        ts, pt = _dev(timesteps, torch.int32)
        context, pc = _dev(context)
        label, pl = _dev(label)
        B, _, H, W = x.shape
        flat, pr = None, None
        if residuals is not None:
            shapes = unet_skip_shapes(self.cfg, H, W)
            got = [tuple(r.shape) for r in residuals]
            if got != [(B,) + s for s in shapes]:
                raise InvalidArgument(f"forward_residuals: residuals must have the shapes {[(B,) + s for s in shapes]}, got {got}")
            flat, pr = _dev(torch.cat([r.to(torch.float32).reshape(-1) for r in residuals]))
        out = torch.empty((B, self.cfg.out_channels, H, W), device=x.device, dtype=torch.float32)
        _check_invalid(lib().sdxl_unet_forward_residuals(self.h, _stream(), px, pt, pc, pl, B, H, W, int(context.shape[1]), pr, float(scale),
                                                         ctypes.c_void_p(out.data_ptr())))
        return out

    BLOCK_SECTIONS = {"input": 0, "middle": 1, "output": 2, "head": 3}

    def run_block(self, section: str, index: int, x, emb, context):
        """one entry of the block plan through the code forward runs for it (sdxl_unet_block): section "input" / "middle" / "output" / "head";
        x [B,c_in,h,w] at the entry's own resolution (the concat width for output entries), emb [B,4*model_channels] = t_emb + l_emb,
        context [B,n_ctx,ctx] -> [B,c_out,h_out,w_out].  Replaces the handle's context."""
        torch = _torch()
        sec = self.BLOCK_SECTIONS.get(section)
        if sec is None:
            raise InvalidArgument(f"run_block: unknown section {section!r}")
        if x is None or emb is None or context is None or x.dim() != 4 or emb.dim() != 2 or context.dim() != 3:
            raise InvalidArgument("run_block: x must be [B,c_in,h,w], emb [B,4*model_channels], context [B,n_ctx,ctx]")
        x, px = _dev(x)
        emb, pe = _dev(emb)
        context, pc = _dev(context)
        B, c_in, h, w = x.shape
        if tuple(emb.shape) != (B, 4 * self.cfg.model_channels) or context.shape[0] != B or context.shape[2] != self.cfg.context_dim:
            raise InvalidArgument("run_block: emb must be [B,4*model_channels] and context [B,n_ctx,context_dim] for x's B")
        shape = (ctypes.c_int64 * 4)()
        call = lambda out: _check_invalid(lib().sdxl_unet_block(self.h, _stream(), sec, int(index), px, pe, pc, B, c_in, h, w, int(context.shape[1]), out, shape))      # noqa: E731
        call(ctypes.c_void_p(None))      # the entry's output shape (and the refusal of an entry / size outside the plan) before anything is allocated
        out = torch.empty(tuple(int(v) for v in shape), device=x.device, dtype=torch.float32)
        call(ctypes.c_void_p(out.data_ptr()))
        return out

    def set_split_cfg(self, enabled: bool, release_offset: int = 0):
        """per-handle: run the CFG pair (batch-2 forward) as two concurrent batch-1 chains; bit-identical results"""
        _check_invalid(lib().sdxl_unet_set_split_cfg(self.h, int(enabled), int(release_offset)))      # (refused while skip residuals are attached)

    def set_fused_cross_attention(self, enabled: bool):
        """per-handle (default on): cross-attention inside the query projection's epilogue"""
        _check(lib().sdxl_unet_set_fused_cross_attention(self.h, int(enabled)))

    def set_gn_from_producer(self, enabled: bool):
        """per-handle (default on): GroupNorm statistics from the producing convolution's epilogue where its kernel can"""
        _check(lib().sdxl_unet_set_gn_from_producer(self.h, int(enabled)))

    def set_graph(self, enabled: bool):
        _check(lib().sdxl_unet_set_graph(self.h, int(enabled)))

    def mix_classes(self) -> int:
        """MIX_* classes on plain f16 operands (F32_SPLIT_MIX* models; an F16W model on parameters that are not f16 values reports F32_SPLIT_MIX's 1 | 2 | 1024)"""
        v = ctypes.c_int(0)
        _check(lib().sdxl_unet_mix_classes(self.h, ctypes.byref(v)))
        return v.value

    def weight_arena(self) -> Tuple[int, int]:
        base, n = ctypes.c_void_p(), ctypes.c_size_t()
        _check(lib().sdxl_unet_weight_arena(self.h, ctypes.byref(base), ctypes.byref(n)))
        return int(base.value or 0), int(n.value)

    def weight_arena_tensor(self):
        """zero-copy uint8 view of the packed weight arena (for the one-time RCCL broadcast from rank 0)"""
        return arena_as_tensor(*self.weight_arena(), self.ctx.device_id)

    PROFILE_CLASSES = ("igemm", "attention", "groupnorm", "layernorm", "other")

    def profile(self, B: int, H: int, W: int):
        """one eager forward with hipEvents around every launch -> {class: (ms, launches, flops)}"""
        ms, ln, fl = (ctypes.c_float * 5)(), (ctypes.c_int * 5)(), (ctypes.c_double * 5)()
        _check(lib().sdxl_unet_profile(self.h, _stream(), B, H, W, ms, ln, fl))
        return {c: (float(ms[i]), int(ln[i]), float(fl[i])) for i, c in enumerate(self.PROFILE_CLASSES)}

    def eager_forward_ms(self, B: int, H: int, W: int) -> float:
        """the chain profile() runs without the per-launch events (one event pair around it, best of three)"""
        v = ctypes.c_float(0)
        _check(lib().sdxl_unet_eager_forward_ms(self.h, _stream(), B, H, W, ctypes.byref(v)))
        return float(v.value)

    def __del__(self):
        if getattr(self, "_owned", False) and getattr(self, "h", None) and _lib is not None:
            _lib.sdxl_unet_destroy(self.h)
            self.h = None


class ControlNet:
    """A ControlNet (Zhang et al. 2023; sgm ControlNet / diffusers ControlNetModel) for the UNet cfg.unet: DTYPE_F32, DTYPE_F16 or DTYPE_F32_SPLIT, its
    residuals go to a UNet of the same configuration and dtype through UNet.forward_residuals.  weights: flat fp32 or f16 array in controlnet_param_specs order; None: the
    synthetic seed."""

    def __init__(self, ctx: Context, cfg: ControlNetConfig, dtype: int = DTYPE_F16, weights: Optional[np.ndarray] = None, seed: Optional[int] = None):
        self.ctx, self.cfg, self.dtype = ctx, cfg, dtype
        self.h = ctypes.c_void_p()
        c = cfg.to_c()
        if weights is None:
            _check_invalid(lib().sdxl_controlnet_create_synthetic(ctx.h, ctypes.byref(c), dtype, ctypes.c_uint64(seed or 0), ctypes.byref(self.h)))
        elif np.asarray(weights).dtype == np.float16:
            w = np.ascontiguousarray(weights)
            _check_invalid(lib().sdxl_controlnet_create_f16(ctx.h, ctypes.byref(c), dtype, w.ctypes.data_as(ctypes.c_void_p), ctypes.byref(self.h)))
        else:
            w = np.ascontiguousarray(weights, dtype=np.float32)
            _check_invalid(lib().sdxl_controlnet_create(ctx.h, ctypes.byref(c), dtype, w.ctypes.data_as(ctypes.c_void_p), ctypes.byref(self.h)))

    def embed_hint(self, hint):
        """input_hint_block: hint [n, hint_in, H8, W8] -> [n, model_channels, H8 / 8, W8 / 8]"""
        torch = _torch()
        hint, ph = _dev(hint)
        n, _, H8, W8 = hint.shape
        out = torch.empty((n, self.cfg.unet.model_channels, H8 // 8, W8 // 8), device=hint.device, dtype=torch.float32)
        _check_invalid(lib().sdxl_controlnet_embed_hint(self.h, _stream(), ph, n, H8, W8, ctypes.c_void_p(out.data_ptr())))
        return out

    def forward(self, x, timesteps, context, label, hint):
        """the control forward: x [B,4,H,W], timesteps [B] int, context [B,n_ctx,ctx], label [B,adm], hint [B,hint_in,8H,8W] -> the list of residual
        tensors unet_skip_shapes(cfg.unet, H, W), what UNet.forward_residuals takes"""
        torch = _torch()
        x, px = _dev(x)
        ts, pt = _dev(timesteps, torch.int32)
        context, pc = _dev(context)
        label, pl = _dev(label)
        hint, ph = _dev(hint)
        B, _, H, W = x.shape
        if tuple(hint.shape) != (B, self.cfg.hint_in_channels, 8 * H, 8 * W):
            raise InvalidArgument(f"ControlNet.forward: the hint must be {(B, self.cfg.hint_in_channels, 8 * H, 8 * W)}, got {tuple(hint.shape)}")
        shapes = unet_skip_shapes(self.cfg.unet, H, W)
        flat = torch.empty(sum(B * c * h * w for c, h, w in shapes), device=x.device, dtype=torch.float32)
        _check_invalid(lib().sdxl_controlnet_forward(self.h, _stream(), px, pt, pc, pl, ph, B, H, W, int(context.shape[1]), ctypes.c_void_p(flat.data_ptr())))
        out, o = [], 0
        for c, h, w in shapes:
            out.append(flat[o:o + B * c * h * w].view(B, c, h, w))
            o += B * c * h * w
        return out

    def __del__(self):
        try:
            if self.h:
                lib().sdxl_controlnet_destroy(self.h)
        except Exception:
            pass


@dataclass
class CLIPConfig:
    """reference CLIPConfig (src/model/clip/mod.rs:19-28)"""
    n_vocab: int
    n_state: int
    embed_dim: int
    n_head: int
    n_ctx: int
    n_layer: int
    quick_gelu: bool

    def to_c(self) -> _ClipConfigC:
        return _ClipConfigC(self.n_vocab, self.n_state, self.embed_dim, self.n_head, self.n_ctx, self.n_layer,
                            int(self.quick_gelu))


def clip_l_config() -> CLIPConfig:
    return CLIPConfig(49408, 768, 768, 12, 77, 12, True)


def open_clip_bigg_config() -> CLIPConfig:
    return CLIPConfig(49408, 1280, 1280, 20, 77, 32, False)


class CLIP:
    """reference CLIP<B> (src/model/clip/mod.rs:62-151): text transformer on the GPU, token ids in"""

    def __init__(self, ctx: Context, cfg: CLIPConfig, dtype: int = DTYPE_F16, weights: Optional[np.ndarray] = None,
                 seed: int = 0):
        self.ctx, self.cfg, self.dtype = ctx, cfg, dtype
        self.h = ctypes.c_void_p()
        c = cfg.to_c()
        if weights is None:
            _check(lib().sdxl_clip_create_synthetic(ctx.h, ctypes.byref(c), dtype, ctypes.c_uint64(seed), ctypes.byref(self.h)))
        elif np.asarray(weights).dtype == np.float16:
            w = np.ascontiguousarray(weights)
            _check(lib().sdxl_clip_create_f16(ctx.h, ctypes.byref(c), dtype, w.ctypes.data_as(ctypes.c_void_p), ctypes.byref(self.h)))
        else:
            w = np.ascontiguousarray(weights, dtype=np.float32)
            _check(lib().sdxl_clip_create(ctx.h, ctypes.byref(c), dtype, w.ctypes.data_as(ctypes.c_void_p), ctypes.byref(self.h)))

    def max_sequence_length(self) -> int:
        return self.cfg.n_ctx

    def num_layers(self) -> int:
        return self.cfg.n_layer

    def _tokens(self, tokens):
        torch = _torch()
        t = torch.as_tensor(tokens)
        if t.dim() != 2:
            raise EngineError("tokens must be [n_batch, seq_len]")
        if int(t.min()) < 0 or int(t.max()) >= self.cfg.n_vocab:
            raise EngineError("token id outside the vocabulary")
        return _dev(t.to(f"cuda:{self.ctx.device_id}"), torch.int32)

    def forward_hidden(self, tokens, hidden_idx: int):
        """CLIP::forward_hidden (:94-112) -> [n, seq, n_state]"""
        torch = _torch()
        t, pt = self._tokens(tokens)
        n, seq = t.shape
        out = torch.empty((n, seq, self.cfg.n_state), device=t.device, dtype=torch.float32)
        _check(lib().sdxl_clip_forward_hidden(self.h, _stream(), pt, n, seq, int(hidden_idx), ctypes.c_void_p(out.data_ptr())))
        return out

    def forward_hidden_pooled(self, tokens, hidden_idx: int):
        """CLIP::forward_hidden_pooled (:114-151) -> ([n, seq, n_state], [n, embed_dim])"""
        torch = _torch()
        t, pt = self._tokens(tokens)
        n, seq = t.shape
        hidden = torch.empty((n, seq, self.cfg.n_state), device=t.device, dtype=torch.float32)
        pooled = torch.empty((n, self.cfg.embed_dim), device=t.device, dtype=torch.float32)
        _check(lib().sdxl_clip_forward_hidden_pooled(self.h, _stream(), pt, n, seq, int(hidden_idx),
                                                     ctypes.c_void_p(hidden.data_ptr()), ctypes.c_void_p(pooled.data_ptr())))
        return hidden, pooled

    def weight_arena(self) -> Tuple[int, int]:
        base, n = ctypes.c_void_p(), ctypes.c_size_t()
        _check(lib().sdxl_clip_weight_arena(self.h, ctypes.byref(base), ctypes.byref(n)))
        return int(base.value or 0), int(n.value)

    def __del__(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.sdxl_clip_destroy(self.h)
            self.h = None


def conditioning_embedding(ctx: Context, pooled, dim: int, size, crop, ar):
    """reference conditioning_embedding (src/model/unet/mod.rs:41-57): [pooled | timestep_embedding(size|crop|ar)]"""
    torch = _torch()
    pooled, pp = _dev(pooled)
    vals = torch.cat([torch.as_tensor(v).to(pooled.device).reshape(pooled.shape[0], -1) for v in (size, crop, ar)], dim=1)
    vals, pv = _dev(vals, torch.int32)
    n, E = pooled.shape
    w = int(vals.shape[1])
    out = torch.empty((n, E + w * dim), device=pooled.device, dtype=torch.float32)
    _check(lib().sdxl_conditioning_embedding(ctx.h, _stream(), pp, n, E, pv, w, dim, ctypes.c_void_p(out.data_ptr())))
    return out


class Embedder:
    """reference Embedder<B> (stablediffusion/mod.rs:652-757).  The tokenizers are optional: without them (no asset files)
    only tokens_to_conditioning is available -- which is also what a Rust caller of the C ABI uses."""

    def __init__(self, ctx: Context, clip: CLIP, open_clip: CLIP, clip_tokenizer=None, open_clip_tokenizer=None):
        self.ctx, self.clip, self.open_clip = ctx, clip, open_clip
        self.clip_tokenizer, self.open_clip_tokenizer = clip_tokenizer, open_clip_tokenizer

    def _finish(self, full, open_ctx, pooled, size, crop, ar):
        """tail of Embedder::context / unconditional_context (:697-757): the two label vectors of one prompt"""
        torch = _torch()
        n = int(torch.as_tensor(ar).shape[0])
        if pooled.shape[0] != n:
            raise EngineError("the reference concatenates a [1, E] pooled embedding with [n_batch, .] size embeddings: n_batch must be 1")
        aesthetic = torch.full((n, 1), 6, dtype=torch.int32)                                           # :709,740
        return (full, open_ctx, conditioning_embedding(self.ctx, pooled, 256, size, crop, ar),
                conditioning_embedding(self.ctx, pooled, 256, size, crop, aesthetic))

    def tokens_to_conditioning(self, clip_ids, open_ids, uncond_clip_ids, uncond_open_ids, size, crop, ar) -> Conditioning:
        """text_to_conditioning (:661-696) after tokenize_text: ids [1, n_ctx] -- or [c, n_ctx], the c <= 4 chunks of a long prompt
        (tokenizer.tokenize_text_chunks; the same c for all four); size / crop [n, 2] ints, ar [2] ints.  Every chunk is encoded as a
        batch row of its own (the position table stays n_ctx long), the hidden states are concatenated along the token axis to
        [1, c n_ctx, .] and the pooled embedding is chunk 0's."""
        torch = _torch()
        size, crop, ar = torch.as_tensor(size), torch.as_tensor(crop), torch.as_tensor(ar)
        n = int(size.shape[0])
        bar = ar.reshape(1, -1).repeat(n, 1)
        rows = lambda a: torch.as_tensor(a).reshape(-1, torch.as_tensor(a).shape[-1])   # noqa: E731
        ids = [rows(a) for a in (uncond_clip_ids, clip_ids, uncond_open_ids, open_ids)]
        c = int(ids[0].shape[0])
        if any(int(a.shape[0]) != c for a in ids):
            raise ValueError("the four token id tensors must hold the same number of chunks")
        if not 1 <= c <= 4:
            raise ValueError("a prompt is 1 .. 4 chunks of token ids")
        # the reference encodes "" and the prompt in two passes (:680-683); here they ride one batch-2c pass per encoder (the
        # rows of a batch are independent -- bit-identical to separate passes, tests/test_gpu_clip.py) and are split after
        cat = lambda a, b: torch.cat([a, b], dim=0)   # noqa: E731
        clip_ctx = self.clip.forward_hidden(cat(ids[0], ids[1]), self.clip.num_layers() - 1)      # :759-770
        open_ctx, pooled = self.open_clip.forward_hidden_pooled(cat(ids[2], ids[3]), self.open_clip.num_layers() - 1)
        full = torch.cat([clip_ctx, open_ctx], dim=2)
        if c > 1:      # [2c, n_ctx, .] -> [2, c n_ctx, .]: the chunks of a prompt side by side along the token axis; pooled: chunk 0
            full, open_ctx = (t.reshape(2, c * t.shape[1], t.shape[2]) for t in (full, open_ctx))
            pooled = pooled[0::c].contiguous()
        ucf, uco, ucc, uccr = self._finish(full[0:1], open_ctx[0:1], pooled[0:1], size, crop, bar)
        cf, co, cc, ccr = self._finish(full[1:2], open_ctx[1:2], pooled[1:2], size, crop, bar)
        return Conditioning(context_full=cf, channel_context=cc, unconditional_context_full=ucf.squeeze(0),
                            unconditional_channel_context=ucc.squeeze(0), context_open_clip=co, channel_context_refiner=ccr,
                            unconditional_context_open_clip=uco.squeeze(0), unconditional_channel_context_refiner=uccr.squeeze(0),
                            resolution=(int(ar[0]), int(ar[1])))

    def text_to_conditioning(self, text: str, size, crop, ar, *, negative: str = "", max_chunks: int = 1) -> Conditioning:
        """Embedder::text_to_conditioning (:661-696); the unconditional prompt is "" (:703-705) unless `negative` names one.
        max_chunks > 1 (up to 4): a prompt longer than the 77-token window is encoded in chunks of 77 (tokenize_text_chunks) and the
        UNet sees n_ctx = 77 c tokens, c the largest chunk count among the prompt and the negative prompt on both tokenizers; the
        shorter ones are filled with chunks of the empty prompt, so both contexts share n_ctx.  The defaults are the reference's call."""
        if self.clip_tokenizer is None or self.open_clip_tokenizer is None:
            raise EngineError("Embedder was built without tokenizers (asset files not available): use tokens_to_conditioning")
        from .tokenizer import MAX_PROMPT_CHUNKS, tokenize_text_chunks
        if not 1 <= int(max_chunks) <= MAX_PROMPT_CHUNKS:
            raise ValueError(f"max_chunks must be 1 .. {MAX_PROMPT_CHUNKS}")
        torch = _torch()
        pairs = [(t, tok, m.max_sequence_length()) for t in (text, negative)
                 for tok, m in ((self.clip_tokenizer, self.clip), (self.open_clip_tokenizer, self.open_clip))]
        chunks = [tokenize_text_chunks(t, tok, n, int(max_chunks)) for t, tok, n in pairs]
        c = max(len(ch) for ch in chunks)
        for ch, (_, tok, n) in zip(chunks, pairs):
            ch.extend(tokenize_text_chunks("", tok, n, 1) * (c - len(ch)))
        ids = [torch.tensor(ch, dtype=torch.int32) for ch in chunks]      # prompt: clip, open_clip; negative: clip, open_clip
        return self.tokens_to_conditioning(ids[0], ids[1], ids[2], ids[3], size, crop, ar)


class _ArenaView:
    def __init__(self, ptr: int, nbytes: int):
        self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 2}


def arena_as_tensor(ptr: int, nbytes: int, device_id: int = 0):
    torch = _torch()
    return torch.as_tensor(_ArenaView(ptr, nbytes), device=f"cuda:{device_id}")


def debug_set(key: str, value: int):
    _check(lib().sdxl_debug_set(key.encode(), int(value)))


def weight_layout_bytes(cfg, dtype: int, option: int = -1) -> int:
    """sdxl_debug_weight_layout: the bytes the weight arena of a model of this config (UNetConfig, VAEConfig or CLIPConfig) and dtype holds, from the
    layout pass alone -- no GPU needed.  option: UNet -- the MixClass bits in force (-1: the dtype's own); VAE -- with_encoder; CLIP -- unused"""
    c = cfg.to_c()
    slots = [ctypes.byref(c) if isinstance(cfg, k) else None for k in (UNetConfig, VAEConfig, CLIPConfig)]
    if not any(s is not None for s in slots):
        raise EngineError("weight_layout_bytes: a UNetConfig, VAEConfig or CLIPConfig")
    n = ctypes.c_size_t(0)
    _check(lib().sdxl_debug_weight_layout(slots[0], slots[1], slots[2], int(dtype), 0 if isinstance(cfg, CLIPConfig) else int(option), ctypes.byref(n)))
    return int(n.value)


def bench_igemm(ctx: "Context", B: int, H: int, W: int, Cin: int, Cout: int, ksize: int = 1, geglu: bool = False,
                iters: int = 20) -> float:
    """mean launch duration (ms) of the implicit-GEMM kernel alone on seeded random f16 data"""
    ms = ctypes.c_float()
    _check(lib().sdxl_bench_igemm(ctx.h, None, B, H, W, Cin, Cout, ksize, int(geglu), iters, ctypes.byref(ms)))   # geglu: bit0 GEGLU, bit1 LN-folded input, bit2 row statistics out
    return float(ms.value)


def bench_attention(ctx: "Context", B: int, H: int, Nq: int, Nk: int, iters: int = 20) -> float:
    """mean launch duration (ms) of the fused d=64 f16 attention kernel alone on seeded random data"""
    ms = ctypes.c_float()
    _check(lib().sdxl_bench_attention(ctx.h, None, B, H, Nq, Nk, iters, ctypes.byref(ms)))
    return float(ms.value)


def default_alphas_cumprod(n: int = 1000) -> np.ndarray:
    """sgm LegacyDDPMDiscretization (reference python/dump.py:29-31): the loaded `alpha_cumulative_products` param"""
    betas = np.linspace(0.00085 ** 0.5, 0.012 ** 0.5, n, dtype=np.float64) ** 2
    return np.cumprod(1.0 - betas).astype(np.float32)


DRAW_INITIAL = 0        # SDXL_DRAW_INITIAL: noise0 of sampling, the re-noise of refine_latent


def draw_blend(i: int) -> int:
    """SDXL_DRAW_BLEND(i): the inpainting blend in front of iteration i (:463)"""
    return 1 + 2 * i


def draw_sigma(i: int) -> int:
    """SDXL_DRAW_SIGMA(i): the gen_noise() * sigma term of iteration i (:427)"""
    return 2 + 2 * i


SOLVER_DDIM = 0         # SDXL_SOLVER_DDIM: the reference's loop (default)
SOLVER_DPMPP_2M = 1     # SDXL_SOLVER_DPMPP_2M: DPM-Solver++(2M), with eta > 0 its SDE form
SOLVER_LCM = 3          # SDXL_SOLVER_LCM: LCM multistep consistency sampling (takes no eta; needs the seeded calls beyond one iteration)
SOLVER_TCD = 4          # SDXL_SOLVER_TCD: TCD gamma-sampling, the seeded calls' eta read as gamma
SOLVER_DPMPP_3M = 5     # SDXL_SOLVER_DPMPP_3M: DPM++ 3M SDE (eta = 0: its ODE form), two x0 histories
_SOLVER_NAMES = {"ddim": SOLVER_DDIM, "dpmpp_2m": SOLVER_DPMPP_2M, "lcm": SOLVER_LCM, "tcd": SOLVER_TCD, "dpmpp_3m": SOLVER_DPMPP_3M}

SCHEDULE_REFERENCE, SCHEDULE_TRAILING, SCHEDULE_LEADING, SCHEDULE_LCM = 0, 1, 2, 3      # SDXL_SCHEDULE_*
_SCHEDULE_KINDS = {"reference": SCHEDULE_REFERENCE, "trailing": SCHEDULE_TRAILING, "leading": SCHEDULE_LEADING, "lcm": SCHEDULE_LCM}


def timestep_schedule(kind, n_steps: int, n_train: int = 1000, offset: int = 1, origin_steps: int = 50) -> List[int]:
    """sdxl_timestep_schedule (host logic: no GPU needed): a published spacing as a list for Diffuser.set_timesteps.  kind "reference" (the
    default rule: sdxl_step_count entries), "trailing" (Lightning, Turbo), "leading" (diffusers' default with steps_offset = offset) or
    "lcm" (LCM / TCD / Hyper-SD on origin_steps), or the SCHEDULE_* value; what the engine refuses raises InvalidArgument"""
    if isinstance(kind, str):
        if kind not in _SCHEDULE_KINDS:
            raise InvalidArgument(f"unknown schedule kind {kind!r}: one of {sorted(_SCHEDULE_KINDS)}")
        kind = _SCHEDULE_KINDS[kind]
    param = {SCHEDULE_LEADING: int(offset), SCHEDULE_LCM: int(origin_steps)}.get(int(kind), 0)
    cap = max(int(n_train), 1)
    out = np.full((cap,), -1, dtype=np.int32)      # a refusal leaves out untouched: that tells SDXL_ERR_INVALID (1) from a count of 1
    n = lib().sdxl_timestep_schedule(int(kind), int(n_steps), int(n_train), param, out.ctypes.data_as(ctypes.c_void_p), cap)
    if n < 1 or out[0] < 0:
        raise InvalidArgument(lib().sdxl_last_error().decode())
    return [int(v) for v in out[:n]]


def _timesteps(timesteps):
    """int32 array of a list (None stays None)"""
    if timesteps is None:
        return None
    return np.ascontiguousarray(np.asarray(list(timesteps), dtype=np.int64).astype(np.int32).reshape(-1))


def _solver(solver) -> int:
    """a name of _SOLVER_NAMES or an SDXL_SOLVER_* value (an unknown value travels on: the engine reports it)"""
    if isinstance(solver, str):
        if solver not in _SOLVER_NAMES:
            raise EngineError(f"unknown solver {solver!r}: one of {sorted(_SOLVER_NAMES)}")
        return _SOLVER_NAMES[solver]
    return int(solver)


PREDICTION_EPSILON = 0  # SDXL_PREDICTION_EPSILON: the UNet's output is the noise e (default, the reference's reading)
PREDICTION_V = 1        # SDXL_PREDICTION_V: it is v = alpha e - sigma x0 (checkpoints trained on a zero-terminal-SNR schedule)
_PREDICTION_NAMES = {"epsilon": PREDICTION_EPSILON, "v": PREDICTION_V}


def _prediction(prediction) -> int:
    """a name of _PREDICTION_NAMES or an SDXL_PREDICTION_* value (an unknown value travels on: the engine reports it)"""
    if isinstance(prediction, str):
        if prediction not in _PREDICTION_NAMES:
            raise InvalidArgument(f"unknown prediction {prediction!r}: one of {sorted(_PREDICTION_NAMES)}")
        return _PREDICTION_NAMES[prediction]
    return int(prediction)


def rescale_zero_terminal_snr(alphas) -> np.ndarray:
    """sdxl_rescale_zero_terminal_snr (host logic: no GPU needed): the alphas_cumprod table shifted and scaled in sqrt-space so that its last
    value is exactly 0 and its first unchanged (Lin et al. 2023, Algorithm 1) -> float32 array; a table it refuses raises InvalidArgument"""
    a = np.ascontiguousarray(alphas, dtype=np.float32)
    out = np.empty_like(a)
    _check_invalid(lib().sdxl_rescale_zero_terminal_snr(a.ctypes.data_as(ctypes.c_void_p), int(a.shape[0]), out.ctypes.data_as(ctypes.c_void_p)))
    return out


def solver_coefficients(alphas, n_steps: int, step_start: int = 0, solver="dpmpp_2m", eta: float = 0.0, prediction="epsilon",
                        timesteps=None) -> np.ndarray:
    """sdxl_solver_coefficients: float64 [iterations, 4] rows (c_x, c_0, c_1, c_z) of x' = c_x x + c_0 x0 + c_1 x0p + c_z z, the
    table the sampler runs (host logic: no GPU needed).  prediction "v" (sdxl_solver_coefficients_pred) admits a zero-terminal-SNR table.
    timesteps (sdxl_solver_coefficients_ts): one row per entry of the list; n_steps and step_start are not read."""
    a = np.ascontiguousarray(alphas, dtype=np.float32)
    ts = _timesteps(timesteps)
    if ts is not None:
        out = np.zeros((int(ts.size), 4), dtype=np.float64)
        _check_invalid(lib().sdxl_solver_coefficients_ts(a.ctypes.data_as(ctypes.c_void_p), int(a.shape[0]), ts.ctypes.data_as(ctypes.c_void_p),
                                                         int(ts.size), _solver(solver), _prediction(prediction), float(eta),
                                                         out.ctypes.data_as(ctypes.c_void_p), int(ts.size)))
        return out
    iters = max(step_count(n_steps, step_start, int(a.shape[0])), 0) if n_steps >= 1 else 0
    out = np.zeros((iters, 4), dtype=np.float64)
    if _prediction(prediction) == PREDICTION_EPSILON:      # the entry every build has
        _check_invalid(lib().sdxl_solver_coefficients(a.ctypes.data_as(ctypes.c_void_p), int(a.shape[0]), n_steps, step_start, _solver(solver),
                                                     float(eta), out.ctypes.data_as(ctypes.c_void_p), iters))
    else:
        _check_invalid(lib().sdxl_solver_coefficients_pred(a.ctypes.data_as(ctypes.c_void_p), int(a.shape[0]), n_steps, step_start,
                                                           _solver(solver), _prediction(prediction), float(eta),
                                                           out.ctypes.data_as(ctypes.c_void_p), iters))
    return out


SIGMAS_ROUND_T = 1      # SDXL_SIGMAS_ROUND_T: the timestep of a sigma rounded to the nearest integer (diffusers' use_karras_sigmas convention)
SIGMAS_KARRAS, SIGMAS_EXPONENTIAL, SIGMAS_OF_TIMESTEPS = 0, 1, 2      # SDXL_SIGMAS_*
_SIGMA_KINDS = {"karras": SIGMAS_KARRAS, "exponential": SIGMAS_EXPONENTIAL, "of_timesteps": SIGMAS_OF_TIMESTEPS}


def _sigmas(sigmas):
    """float64 array of a list (None stays None)"""
    if sigmas is None:
        return None
    return np.ascontiguousarray(np.asarray(list(sigmas), dtype=np.float64).reshape(-1))


def sigma_schedule(kind, n_steps: int, alphas=None, sigma_min: float = 0.0, sigma_max: float = 0.0, rho: float = 7.0) -> List[float]:
    """sdxl_sigma_schedule (host logic: no GPU needed): a published sigma spacing as a list for Diffuser.set_sigmas.  kind "karras",
    "exponential" or "of_timesteps" (the sigmas of the reference rule's list), or the SIGMAS_* value; sigma_min / sigma_max <= 0 take the
    ends of the table (alphas, default the SDXL table); what the engine refuses raises InvalidArgument"""
    if isinstance(kind, str):
        if kind not in _SIGMA_KINDS:
            raise InvalidArgument(f"unknown sigma schedule kind {kind!r}: one of {sorted(_SIGMA_KINDS)}")
        kind = _SIGMA_KINDS[kind]
    a = np.ascontiguousarray(default_alphas_cumprod() if alphas is None else alphas, dtype=np.float32)
    cap = max(int(a.shape[0]), 1)
    out = np.full((cap,), -1.0, dtype=np.float64)      # a refusal leaves out untouched: that tells SDXL_ERR_INVALID (1) from a count of 1
    n = lib().sdxl_sigma_schedule(int(kind), int(n_steps), a.ctypes.data_as(ctypes.c_void_p), int(a.shape[0]), float(sigma_min), float(sigma_max),
                                  float(rho), out.ctypes.data_as(ctypes.c_void_p), cap)
    if n < 1 or out[0] < 0:
        raise InvalidArgument(lib().sdxl_last_error().decode())
    return [float(v) for v in out[:n]]


def sigma_to_timestep(sigma: float, alphas=None, round_t: bool = False) -> float:
    """sdxl_sigma_to_timestep (host logic: no GPU needed): k-diffusion's sigma_to_t in f64, the timestep a sigma list feeds the UNet"""
    a = np.ascontiguousarray(default_alphas_cumprod() if alphas is None else alphas, dtype=np.float32)
    t = ctypes.c_double(-1.0)
    _check_invalid(lib().sdxl_sigma_to_timestep(a.ctypes.data_as(ctypes.c_void_p), int(a.shape[0]), float(sigma), SIGMAS_ROUND_T if round_t else 0,
                                                ctypes.byref(t)))
    return t.value


class _ScheduleDescC(ctypes.Structure):
    _fields_ = [("alphas_cumprod_host", ctypes.c_void_p), ("n_train_steps", ctypes.c_int32), ("timesteps", ctypes.c_void_p), ("sigmas", ctypes.c_void_p),
                ("n", ctypes.c_int32), ("t_end", ctypes.c_int32), ("sigma_end", ctypes.c_double), ("flags", ctypes.c_int32)]


def _schedule_desc(alphas, timesteps=None, sigmas=None, t_end: int = -1, sigma_end: float = 0.0, flags: int = 0):
    """(sdxl_schedule_desc, the arrays it points into, the number of entries)"""
    a = np.ascontiguousarray(alphas, dtype=np.float32)
    ts, sg = _timesteps(timesteps), _sigmas(sigmas)
    n = int(ts.size) if ts is not None else int(sg.size) if sg is not None else 0
    desc = _ScheduleDescC(a.ctypes.data_as(ctypes.c_void_p), int(a.shape[0]), ts.ctypes.data_as(ctypes.c_void_p) if ts is not None else None,
                          sg.ctypes.data_as(ctypes.c_void_p) if sg is not None else None, n, int(t_end), float(sigma_end), int(flags))
    return desc, (a, ts, sg), n


def solver_rows(alphas, solver="dpmpp_3m", eta: float = 0.0, prediction="epsilon", timesteps=None, sigmas=None, t_end: int = -1,
                sigma_end: float = 0.0, flags: int = 0) -> np.ndarray:
    """sdxl_solver_rows (host logic: no GPU needed): float64 [n, 5] rows (c_x, c_0, c_1, c_2, c_z) of x' = c_x x + c_0 x0 + c_1 x0p + c_2 x0pp
    + c_z z for any solver on a timestep list (with t_end) or a sigma list (with sigma_end and flags): exactly one of the two lists"""
    desc, keep, n = _schedule_desc(alphas, timesteps, sigmas, t_end, sigma_end, flags)
    out = np.zeros((n, 5), dtype=np.float64)
    _check_invalid(lib().sdxl_solver_rows(ctypes.byref(desc), _solver(solver), _prediction(prediction), float(eta),
                                          out.ctypes.data_as(ctypes.c_void_p), n))
    return out


def guidance_default() -> Guidance:
    """sdxl_guidance_default (host logic: no GPU needed)"""
    g = Guidance()
    lib().sdxl_guidance_default(ctypes.byref(g))
    return g


def make_guidance(mode="cfg", rescale: float = 0.0, scales=None, t_range=None) -> Guidance:
    """a Guidance from keywords: mode "cfg" / "off" (or the GUIDANCE_* value), rescale = phi of CFG rescale, scales = one guidance scale per
    batch entry (replaces the call's scalar), t_range = (t_lo, t_hi): guidance only on iterations with t_lo <= t <= t_hi.  Nothing is
    checked here: guidance_check / Diffuser.set_guidance report what the engine refuses."""
    g = guidance_default()
    if isinstance(mode, str):
        if mode not in _GUIDANCE_MODES:
            raise InvalidArgument(f"unknown guidance mode {mode!r}: one of {sorted(_GUIDANCE_MODES)}")
        mode = _GUIDANCE_MODES[mode]
    g.mode, g.rescale = int(mode), float(rescale)
    if scales is not None:
        v = [float(x) for x in scales]
        g.n_scales = len(v)       # more than 8 travels on as a count: the engine reports it
        for b, x in enumerate(v[:8]):
            g.scales[b] = x
    if t_range is not None:
        g.t_lo, g.t_hi = int(t_range[0]), int(t_range[1])
    return g


def control_default() -> Control:
    """sdxl_control_default (host logic: no GPU needed)"""
    c = Control()
    lib().sdxl_control_default(ctypes.byref(c))
    return c


def make_control(scale: float = 1.0, scales=None, t_range=None, cond_only: bool = False) -> Control:
    """a Control from keywords: scale = the conditioning scale of every entry, scales = one per batch entry (replaces scale), t_range = (t_lo, t_hi):
    control only on iterations with t_lo <= t <= t_hi, cond_only: residuals for the conditional entries of the CFG pair only.  Nothing is checked
    here: control_check reports what the engine refuses."""
    c = control_default()
    c.scale = float(scale)
    if scales is not None:
        scales = [float(v) for v in scales]
        c.n_scales = len(scales)
        for i, v in enumerate(scales[:8]):
            c.scales[i] = v
    if t_range is not None:
        c.t_lo, c.t_hi = int(t_range[0]), int(t_range[1])
    c.cond_only = int(bool(cond_only))
    return c


def control_check(c: Control, single_branch: bool = False):
    """sdxl_control_check (host logic, no GPU needed): raises InvalidArgument with the first complaint"""
    _check_invalid(lib().sdxl_control_check(ctypes.byref(c), int(single_branch)))


def control_scale_table(c: Control, n: int, timesteps, single_branch: bool = False):
    """sdxl_control_scale_table (host logic, no GPU needed): the scales of one control net over a trajectory as a float32 numpy array
    [len(timesteps) + 1, 8] -- row i for the iteration at timesteps[i], column b for batch entry b (n entries with single_branch, else the 2 n of the
    CFG pair), the last row zeros.  InvalidArgument: what control_check refuses, a batch above 8, n_scales neither 0 nor n."""
    import numpy as np
    ts = np.ascontiguousarray(np.asarray(timesteps, dtype=np.int32).reshape(-1))
    out = np.full((ts.size + 1, 8), np.nan, dtype=np.float32)
    _check_invalid(lib().sdxl_control_scale_table(ctypes.byref(c), int(n), int(single_branch), ts.ctypes.data_as(ctypes.c_void_p), int(ts.size),
                                                  out.ctypes.data_as(ctypes.c_void_p)))
    return out


def guidance_check(g: Guidance, is_refiner: bool = False):
    """sdxl_guidance_check (host logic, no GPU needed): raises InvalidArgument with the first complaint"""
    _check_invalid(lib().sdxl_guidance_check(ctypes.byref(g), int(is_refiner)))


def cfg_rescale_factors(ctx: Context, eps, scales, rescale: float):
    """sdxl_cfg_rescale_factors, the op the sampler runs under CFG rescale: eps [2n, HW, 4] float32 CUDA tensor (UNet output rows, cond entries
    first), scales: n guidance scales -> float32 CUDA tensor [n] of f_b = fma(rescale, sqrt(M2(ec_b) / M2(ecfg_b)), 1 - rescale)"""
    torch = _torch()
    eps, pe = _dev(eps)
    if eps.dim() != 3 or eps.shape[0] % 2 or eps.shape[2] != 4:
        raise InvalidArgument("eps must be [2n, HW, 4]")
    n, HW = int(eps.shape[0]) // 2, int(eps.shape[1])
    v = [float(x) for x in scales]
    if len(v) != n:
        raise InvalidArgument(f"expected {n} scales (one per batch entry), got {len(v)}")
    out = torch.empty((n,), dtype=torch.float32, device="cuda")
    _check_invalid(lib().sdxl_cfg_rescale_factors(ctx.h, _stream(), pe, n, HW, (ctypes.c_float * max(n, 1))(*v), ctypes.c_float(rescale),
                                                  ctypes.c_void_p(out.data_ptr())))
    return out


class _StepReplayArgsC(ctypes.Structure):
    _fields_ = [("alphas_cumprod_host", _c_p), ("n_train_steps", ctypes.c_int32), ("n_steps", ctypes.c_int32), ("step_start", ctypes.c_int32),
                ("solver", ctypes.c_int32), ("eta", ctypes.c_double), ("unconditional_guidance_scale", ctypes.c_double),
                ("guidance", ctypes.POINTER(Guidance)), ("single", ctypes.c_int32),
                ("n", ctypes.c_int32), ("h", ctypes.c_int32), ("w", ctypes.c_int32), ("input_f16", ctypes.c_int32),
                ("eps", _f_p), ("latent0", _f_p), ("reference", _f_p), ("mask", _f_p), ("step_noise", _f_p), ("seeds", _c_p),
                ("latents_out", _f_p), ("hist_out", _f_p), ("unet_in_out", _f_p), ("timesteps_out", _f_p)]


def sampler_step_replay(ctx: Context, alphas, n_steps: int, step_start: int, eps, latent0, solver="ddim", eta: float = 0.0,
                        cfg_scale: float = 7.5, guidance: Optional[Guidance] = None, single: bool = False, input_f16: bool = False,
                        reference=None, mask=None, step_noise=None, seeds=None, prediction="epsilon", timesteps=None):
    """sdxl_sampler_step_replay, the trajectory without the UNet (a test seam): eps [iterations, B, h*w, 4] and latent0 [n, 4, h, w] float32
    CUDA tensors, B = n where single (or guidance mode "off"), else 2n.  Returns float32 CUDA tensors (latents [iterations + 1, n, 4, h, w],
    hist [n, 4, h, w] -- zeros under DDIM --, unet_in [B, h*w, 4], timesteps [iterations + 1]).  Nothing is checked here but the shapes the
    outputs are sized by: the engine reports what it refuses (InvalidArgument).  prediction "v" (sdxl_sampler_step_replay_pred): the rows
    of eps are v.  timesteps (sdxl_sampler_step_replay_ts): one iteration per entry of the list; n_steps and step_start are not read."""
    torch = _torch()
    pred = _prediction(prediction)
    ts = _timesteps(timesteps)
    a = np.ascontiguousarray(alphas, dtype=np.float32)
    eps, pe = _dev(eps)
    latent0, pl = _dev(latent0)
    n, h, w = int(latent0.shape[0]), int(latent0.shape[2]), int(latent0.shape[3])
    iters = int(eps.shape[0])
    B = n if single or (guidance is not None and guidance.mode == GUIDANCE_OFF) else 2 * n
    want = int(ts.size) if ts is not None else step_count(n_steps, step_start, int(a.shape[0])) if n_steps >= 1 else -1
    if (want >= 0 and iters != want) or tuple(eps.shape[1:]) != (B, h * w, 4) or latent0.shape[1] != 4:
        raise InvalidArgument(f"eps must be [{want}, {B}, {h * w}, 4] and latent0 [n, 4, h, w]")
    for t, lead in ((reference, ()), (mask, ()), (step_noise, (iters,))):
        if t is not None and tuple(t.shape) != lead + (n, 4, h, w):
            raise InvalidArgument(f"reference / mask must be [{n}, 4, {h}, {w}], step_noise [{iters}, {n}, 4, {h}, {w}]")
    keep = [_dev(t, torch.uint8 if t is mask else None) if t is not None else (None, None) for t in (reference, mask, step_noise)]
    out = (torch.zeros((iters + 1, n, 4, h, w), device="cuda"), torch.zeros((n, 4, h, w), device="cuda"),
           torch.zeros((B, h * w, 4), device="cuda"), torch.zeros((iters + 1,), device="cuda"))
    sd = _seeds(seeds, n)
    args = _StepReplayArgsC(a.ctypes.data_as(_c_p), int(a.shape[0]), n_steps, step_start, _solver(solver), float(eta), float(cfg_scale),
                            ctypes.pointer(guidance) if guidance is not None else None, int(single), n, h, w, int(input_f16),
                            pe, pl, keep[0][1], keep[1][1], keep[2][1], ctypes.cast(sd, _c_p) if sd is not None else None,
                            *[ctypes.c_void_p(t.data_ptr()) for t in out])
    if ts is not None:
        _check_invalid(lib().sdxl_sampler_step_replay_ts(ctx.h, _stream(), ctypes.byref(args), pred, ts.ctypes.data_as(ctypes.c_void_p), int(ts.size)))
    elif pred == PREDICTION_EPSILON:      # the entry every build has
        _check_invalid(lib().sdxl_sampler_step_replay(ctx.h, _stream(), ctypes.byref(args)))
    else:
        _check_invalid(lib().sdxl_sampler_step_replay_pred(ctx.h, _stream(), ctypes.byref(args), pred))
    return out


def sampler_step_replay_levels(ctx: Context, alphas, eps, latent0, solver="dpmpp_3m", eta: float = 0.0, cfg_scale: float = 7.5,
                               guidance: Optional[Guidance] = None, single: bool = False, input_f16: bool = False, reference=None, mask=None,
                               step_noise=None, seeds=None, prediction="epsilon", timesteps=None, sigmas=None, t_end: int = -1,
                               sigma_end: float = 0.0, flags: int = 0, hist_fill: Optional[float] = None):
    """sdxl_sampler_step_replay_levels: sampler_step_replay on any schedule (a timestep list with t_end or a sigma list with sigma_end and
    flags) and any solver.  Returns float32 CUDA tensors (latents [n_entries + 1, n, 4, h, w], hist, hist2 [n, 4, h, w], unet_in [B, h*w, 4],
    timesteps [n_entries + 1]); hist and hist2 start from hist_fill (default 0) and keep it where the solver writes none."""
    torch = _torch()
    desc, keep_desc, iters = _schedule_desc(alphas, timesteps, sigmas, t_end, sigma_end, flags)
    eps, pe = _dev(eps)
    latent0, pl = _dev(latent0)
    n, h, w = int(latent0.shape[0]), int(latent0.shape[2]), int(latent0.shape[3])
    B = n if single or (guidance is not None and guidance.mode == GUIDANCE_OFF) else 2 * n
    if tuple(eps.shape) != (iters, B, h * w, 4) or latent0.shape[1] != 4:
        raise InvalidArgument(f"eps must be [{iters}, {B}, {h * w}, 4] and latent0 [n, 4, h, w]")
    for t, lead in ((reference, ()), (mask, ()), (step_noise, (iters,))):
        if t is not None and tuple(t.shape) != lead + (n, 4, h, w):
            raise InvalidArgument(f"reference / mask must be [{n}, 4, {h}, {w}], step_noise [{iters}, {n}, 4, {h}, {w}]")
    keep = [_dev(t, torch.uint8 if t is mask else None) if t is not None else (None, None) for t in (reference, mask, step_noise)]
    fill = 0.0 if hist_fill is None else hist_fill
    latents, hist, hist2 = torch.zeros((iters + 1, n, 4, h, w), device="cuda"), torch.full((n, 4, h, w), fill, device="cuda"), torch.full((n, 4, h, w), fill, device="cuda")
    unet_in, ts_out = torch.zeros((B, h * w, 4), device="cuda"), torch.zeros((iters + 1,), device="cuda")
    sd = _seeds(seeds, n)
    a = keep_desc[0]
    args = _StepReplayArgsC(a.ctypes.data_as(_c_p), int(a.shape[0]), 0, 0, _solver(solver), float(eta), float(cfg_scale),
                            ctypes.pointer(guidance) if guidance is not None else None, int(single), n, h, w, int(input_f16),
                            pe, pl, keep[0][1], keep[1][1], keep[2][1], ctypes.cast(sd, _c_p) if sd is not None else None,
                            *[ctypes.c_void_p(t.data_ptr()) for t in (latents, hist, unet_in, ts_out)])
    _check_invalid(lib().sdxl_sampler_step_replay_levels(ctx.h, _stream(), ctypes.byref(args), _prediction(prediction), ctypes.byref(desc),
                                                         ctypes.c_void_p(hist2.data_ptr())))
    return latents, hist, hist2, unet_in, ts_out


def _seeds(seeds, n: int):
    """host uint64 array [n] (None stays NULL: the engine reports it)"""
    if seeds is None:
        return None
    a = [int(v) & 0xFFFFFFFFFFFFFFFF for v in seeds]
    if len(a) != n:
        raise EngineError(f"expected {n} seeds (one per batch entry), got {len(a)}")
    return (ctypes.c_uint64 * n)(*a)


def _explicit_eta(eta: float):
    if eta != 0.0:
        raise EngineError("eta needs seeds=: the explicit-noise calls carry no noise for the sigma term")


def gen_noise(ctx: Context, seeds, draw: int, n: int, h: int, w: int):
    """gen_noise (:378-388) with a seed: float32 CUDA tensor [n, 4, h, w] (h, w in latent pixels), entry b from seeds[b];
    the values the seeded trajectories draw for (seed, pixel, draw)"""
    torch = _torch()
    out = torch.empty((max(n, 0), 4, max(h, 0), max(w, 0)), dtype=torch.float32, device="cuda")
    _check(lib().sdxl_gen_noise(ctx.h, _stream(), None if seeds is None else _seeds(seeds, n), ctypes.c_uint32(draw), n, h, w,
                               ctypes.c_void_p(out.data_ptr())))
    return out


class Diffuser:
    """reference Diffuser<B> (src/model/stablediffusion/mod.rs:308-542)"""

    def __init__(self, ctx: Context, cfg: UNetConfig, dtype: int = DTYPE_F16, weights: Optional[np.ndarray] = None,
                 seed: int = 0, alphas_cumprod: Optional[np.ndarray] = None, empty: bool = False,
                 lora: Optional[Sequence[LoraEntry]] = None, lora_flags: int = 0):
        """lora / lora_flags: as UNet"""
        self.ctx, self.cfg, self.dtype = ctx, cfg, dtype
        a = np.ascontiguousarray(default_alphas_cumprod() if alphas_cumprod is None else alphas_cumprod, dtype=np.float32)
        self.n_train = int(a.shape[0])
        self.h = ctypes.c_void_p()
        c = cfg.to_c()
        ap = a.ctypes.data_as(ctypes.c_void_p)
        if empty:   # replica rank: arena laid out, contents arrive by broadcast
            if lora is not None:
                raise EngineError("an empty replica receives rank 0's merged arena: it takes no adapters")
            _check(lib().sdxl_diffuser_create_empty(ctx.h, ctypes.byref(c), dtype, ap, self.n_train, ctypes.byref(self.h)))
        elif lora is not None:
            wf, wf16, keep = _lora_base(weights)
            arr, n = _lora_array(lora, cfg)
            _check_invalid(lib().sdxl_diffuser_create_lora(ctx.h, ctypes.byref(c), dtype, wf, wf16, ctypes.c_uint64(seed), arr, n, int(lora_flags),
                                                           ap, self.n_train, ctypes.byref(self.h)))
        elif weights is None:
            _check(lib().sdxl_diffuser_create_synthetic(ctx.h, ctypes.byref(c), dtype, ctypes.c_uint64(seed), ap,
                                                       self.n_train, ctypes.byref(self.h)))
        elif np.asarray(weights).dtype == np.float16:
            w = np.ascontiguousarray(weights)
            _check(lib().sdxl_diffuser_create_f16(ctx.h, ctypes.byref(c), dtype, w.ctypes.data_as(ctypes.c_void_p), ap,
                                                 self.n_train, ctypes.byref(self.h)))
        else:
            w = np.ascontiguousarray(weights, dtype=np.float32)
            _check(lib().sdxl_diffuser_create(ctx.h, ctypes.byref(c), dtype, w.ctypes.data_as(ctypes.c_void_p), ap,
                                             self.n_train, ctypes.byref(self.h)))
        self.diffusion = UNet(ctx, cfg, dtype, _borrowed=ctypes.c_void_p(lib().sdxl_diffuser_unet(self.h)))

    def _latent_shape(self, cond: Conditioning):
        n = int((cond.context_full if cond.context_full is not None else cond.context_open_clip).shape[0])
        return (n, 4, cond.resolution[0] // 8, cond.resolution[1] // 8)

    def sample_latent(self, conditioning: Conditioning, unconditional_guidance_scale: float, n_steps: int, noise0=None, *,
                      seeds=None, eta: float = 0.0):
        """Diffuser::sample_latent (:317-332); noise0 plays gen_noise(), or seeds= (one per batch entry) draws it on the
        device, with eta scaling the sigma term of :427"""
        torch = _torch()
        c, keep = conditioning.to_c()
        if seeds is not None or noise0 is None:
            out = torch.empty(self._latent_shape(conditioning), dtype=torch.float32, device="cuda")
            _check_invalid(lib().sdxl_sample_latent_seeded(self.h, _stream(), ctypes.byref(c), ctypes.c_double(unconditional_guidance_scale),
                                                  n_steps, _seeds(seeds, out.shape[0]), ctypes.c_double(eta),
                                                  ctypes.c_void_p(out.data_ptr())))
            return out
        _explicit_eta(eta)
        noise0, pn = _dev(noise0)
        assert tuple(noise0.shape) == self._latent_shape(conditioning)
        out = torch.empty_like(noise0)
        _check_invalid(lib().sdxl_sample_latent(self.h, _stream(), ctypes.byref(c), ctypes.c_double(unconditional_guidance_scale),
                                       n_steps, pn, ctypes.c_void_p(out.data_ptr())))
        return out

    def sample_latent_with_inpainting(self, conditioning, unconditional_guidance_scale, n_steps, reference, mask, noise0=None,
                                      step_noise=None, *, seeds=None, eta: float = 0.0):
        """Diffuser::sample_latent_with_inpainting (:334-353); mask True = keep generated; step_noise [iters,n,4,h,w], or
        seeds= (one per batch entry): no noise tensor exists, every draw happens inside the per-step kernel"""
        torch = _torch()
        c, keep = conditioning.to_c()
        if seeds is not None or noise0 is None:
            reference, pr = _dev(reference)
            mask, pm = _dev(mask, torch.uint8)
            out = torch.empty_like(reference)
            _check_invalid(lib().sdxl_sample_latent_with_inpainting_seeded(self.h, _stream(), ctypes.byref(c),
                                                                  ctypes.c_double(unconditional_guidance_scale), n_steps, pr, pm,
                                                                  _seeds(seeds, out.shape[0]), ctypes.c_double(eta),
                                                                  ctypes.c_void_p(out.data_ptr())))
            return out
        _explicit_eta(eta)
        noise0, pn = _dev(noise0)
        reference, pr = _dev(reference)
        mask, pm = _dev(mask, torch.uint8)
        step_noise, ps = _dev(step_noise)
        out = torch.empty_like(noise0)
        _check_invalid(lib().sdxl_sample_latent_with_inpainting(self.h, _stream(), ctypes.byref(c),
                                                       ctypes.c_double(unconditional_guidance_scale), n_steps, pr, pm, pn,
                                                       ps, ctypes.c_void_p(out.data_ptr())))
        return out

    def refine_latent(self, latent, conditioning, unconditional_guidance_scale, step_start, n_steps, noise=None, *, seeds=None,
                      eta: float = 0.0):
        """Diffuser::refine_latent (:355-376); noise is the re-noise tensor, or seeds= draws it on the device"""
        torch = _torch()
        c, keep = conditioning.to_c()
        latent, pl = _dev(latent)
        if seeds is not None or noise is None:
            out = torch.empty_like(latent)
            _check_invalid(lib().sdxl_refine_latent_seeded(self.h, _stream(), pl, ctypes.byref(c), ctypes.c_double(unconditional_guidance_scale),
                                                  step_start, n_steps, _seeds(seeds, out.shape[0]), ctypes.c_double(eta),
                                                  ctypes.c_void_p(out.data_ptr())))
            return out
        _explicit_eta(eta)
        noise, pn = _dev(noise)
        out = torch.empty_like(latent)
        _check_invalid(lib().sdxl_refine_latent(self.h, _stream(), pl, ctypes.byref(c), ctypes.c_double(unconditional_guidance_scale),
                                       step_start, n_steps, pn, ctypes.c_void_p(out.data_ptr())))
        return out

    def continue_latent(self, latent, conditioning, unconditional_guidance_scale, n_steps, noise=None, *, seeds=None, eta: float = 0.0,
                        renoise: bool = False):
        """sdxl_continue_latent: the handle's list (set_sigmas / set_timesteps) from a given latent.  renoise False: the latent as it is -- the
        base -> refiner handoff --; True: re-noised to the list's first level with `noise` or the DRAW_INITIAL draw of seeds (exactly one).
        seeds also feed the eta noise.  What the engine refuses raises InvalidArgument."""
        torch = _torch()
        c, keep = conditioning.to_c()
        latent, pl = _dev(latent)
        pn = None
        if noise is not None:
            noise, pn = _dev(noise)
        out = torch.empty_like(latent)
        sd = _seeds(seeds, out.shape[0])
        _check_invalid(lib().sdxl_continue_latent(self.h, _stream(), pl, ctypes.byref(c), ctypes.c_double(unconditional_guidance_scale), int(n_steps),
                                                  pn, ctypes.cast(sd, ctypes.c_void_p) if sd is not None else None, ctypes.c_double(eta), int(renoise),
                                                  ctypes.c_void_p(out.data_ptr())))
        return out

    def set_sigmas(self, sigmas=None, sigma_end: float = 0.0, round_t: bool = False):
        """sdxl_diffuser_set_sigmas: a strictly decreasing list of noise levels sigma = sqrt((1 - a) / a) (sigma_schedule writes the Karras and
        exponential spacings), one UNet evaluation each, with sigma_end behind the last entry (0: the complete trajectory); None or an empty
        list drops it (the handle is back on its timestep list or rule).  A list the engine refuses raises InvalidArgument and the handle
        keeps what it had."""
        sg = _sigmas(sigmas)
        if sg is None or sg.size == 0:
            _check_invalid(lib().sdxl_diffuser_set_sigmas(self.h, None, 0, 0.0, 0))
        else:
            _check_invalid(lib().sdxl_diffuser_set_sigmas(self.h, sg.ctypes.data_as(ctypes.c_void_p), int(sg.size), float(sigma_end),
                                                          SIGMAS_ROUND_T if round_t else 0))

    @property
    def sigmas(self) -> Optional[Tuple[List[float], float, bool]]:
        """(the handle's sigma list, sigma_end, round_t) (sdxl_diffuser_get_sigmas), None without one"""
        out = np.full((4096,), -1.0, dtype=np.float64)
        end, flags = ctypes.c_double(0.0), ctypes.c_int(0)
        n = lib().sdxl_diffuser_get_sigmas(self.h, out.ctypes.data_as(ctypes.c_void_p), int(out.size), ctypes.byref(end), ctypes.byref(flags))
        if n == 0:
            return None
        if out[0] < 0:
            raise InvalidArgument(lib().sdxl_last_error().decode())
        return [float(v) for v in out[:n]], end.value, bool(flags.value & SIGMAS_ROUND_T)

    def set_solver(self, solver):
        """"ddim" (default), "dpmpp_2m", "dpmpp_3m", "lcm" or "tcd" (or the SOLVER_* value): the update every following trajectory of this handle runs"""
        _check(lib().sdxl_diffuser_set_solver(self.h, _solver(solver)))

    def set_timesteps(self, timesteps=None, t_end: int = -1):
        """sdxl_diffuser_set_timesteps: a strictly decreasing list of training timesteps, one UNet evaluation each, for every following
        trajectory of this handle (its n_steps must equal the list's length); None or an empty list: back to the reference's rule.  A list
        the engine refuses raises InvalidArgument and the handle keeps what it had."""
        ts = _timesteps(timesteps)
        if ts is None or ts.size == 0:
            _check_invalid(lib().sdxl_diffuser_set_timesteps(self.h, None, 0))
        else:
            if t_end != -1:      # sdxl_diffuser_set_timesteps_end: the last iteration lands on alphas[t_end], not on the data
                _check_invalid(lib().sdxl_diffuser_set_timesteps_end(self.h, ts.ctypes.data_as(ctypes.c_void_p), int(ts.size), int(t_end)))
                return
            _check_invalid(lib().sdxl_diffuser_set_timesteps(self.h, ts.ctypes.data_as(ctypes.c_void_p), int(ts.size)))

    @property
    def timesteps(self) -> Optional[List[int]]:
        """the handle's list (sdxl_diffuser_get_timesteps), None for the reference's rule"""
        out = np.full((4096,), -1, dtype=np.int32)
        n = lib().sdxl_diffuser_get_timesteps(self.h, out.ctypes.data_as(ctypes.c_void_p), int(out.size))
        if n == 0:
            return None
        if out[0] < 0:      # a refusal leaves out untouched (SDXL_ERR_INVALID and a count of 1 are the same number)
            raise InvalidArgument(lib().sdxl_last_error().decode())
        return [int(v) for v in out[:n]]

    @property
    def timesteps_end(self) -> int:
        """t_end of the handle's timestep list (sdxl_diffuser_get_timesteps_end), -1: the complete trajectory"""
        v = ctypes.c_int(-1)
        _check(lib().sdxl_diffuser_get_timesteps_end(self.h, ctypes.byref(v)))
        return v.value

    @property
    def solver(self) -> str:
        v = ctypes.c_int(-1)
        _check(lib().sdxl_diffuser_get_solver(self.h, ctypes.byref(v)))
        return {v: k for k, v in _SOLVER_NAMES.items()}[v.value]

    def set_prediction(self, prediction):
        """"epsilon" (default) or "v" (or the PREDICTION_* value): what the UNet's output means to every following trajectory of this
        handle.  An unknown value raises InvalidArgument and the handle keeps its own."""
        _check_invalid(lib().sdxl_diffuser_set_prediction(self.h, _prediction(prediction)))

    def get_prediction(self) -> str:
        v = ctypes.c_int(-1)
        _check(lib().sdxl_diffuser_get_prediction(self.h, ctypes.byref(v)))
        return {v: k for k, v in _PREDICTION_NAMES.items()}[v.value]

    def set_guidance(self, guidance: Optional[Guidance] = None, **options):
        """sdxl_diffuser_set_guidance: the guidance options every following trajectory of this handle runs -- a Guidance, or the keywords of
        make_guidance (mode=, rescale=, scales=, t_range=); no argument restores the default.  Options the engine refuses raise
        InvalidArgument and the handle keeps what it had."""
        if guidance is not None and options:
            raise InvalidArgument("give a Guidance or keywords, not both")
        if options:
            guidance = make_guidance(**options)
        _check_invalid(lib().sdxl_diffuser_set_guidance(self.h, None if guidance is None else ctypes.byref(guidance)))

    @property
    def guidance(self) -> Guidance:
        g = Guidance()
        _check(lib().sdxl_diffuser_get_guidance(self.h, ctypes.byref(g)))
        return g

    def enable_step_timing(self, enabled: bool = True):
        _check(lib().sdxl_diffuser_enable_step_timing(self.h, int(enabled)))

    def set_trace(self, trace=None):
        """trace: float32 device tensor [steps, n, 4, h, w] that receives the latent after every DDIM iteration of the
        following trajectories (None switches it off).  The tensor must stay alive while tracing is on."""
        self._trace = trace
        if trace is None:
            _check(lib().sdxl_diffuser_set_trace(self.h, None, 0))
        else:
            assert trace.is_cuda and trace.dtype == _torch().float32 and trace.is_contiguous()
            _check(lib().sdxl_diffuser_set_trace(self.h, ctypes.c_void_p(trace.data_ptr()), int(trace.shape[0])))

    def step_times_ms(self) -> List[float]:
        buf = (ctypes.c_float * 1024)()
        n = lib().sdxl_diffuser_step_times(self.h, buf, 1024)
        return [float(buf[i]) for i in range(max(n, 0))]

    def __del__(self):
        if getattr(self, "h", None) and _lib is not None:
            self.diffusion = None
            _lib.sdxl_diffuser_destroy(self.h)
            self.h = None


@dataclass
class RawImages:
    """reference RawImages (stablediffusion/mod.rs:170-174): u8 HWC buffers"""
    buffer: "object"   # uint8 CUDA tensor [n, height, width, 3]
    width: int
    height: int


class LatentDecoder:
    """reference LatentDecoder<B> (src/model/stablediffusion/mod.rs:193-267) over Autoencoder (autoencoder/mod.rs:46-70)"""

    def __init__(self, ctx: Context, cfg: Optional[VAEConfig] = None, dtype: int = DTYPE_F16,
                 decoder_weights: Optional[np.ndarray] = None, encoder_weights: Optional[np.ndarray] = None,
                 seed: int = 0, with_encoder: bool = False, empty: bool = False):
        self.ctx, self.cfg, self.dtype = ctx, cfg or VAEConfig(), dtype
        self.h = ctypes.c_void_p()
        c = self.cfg.to_c()
        if empty:
            _check(lib().sdxl_vae_create_empty(ctx.h, ctypes.byref(c), dtype, int(with_encoder), ctypes.byref(self.h)))
        elif decoder_weights is None and encoder_weights is None:
            _check(lib().sdxl_vae_create_synthetic(ctx.h, ctypes.byref(c), dtype, ctypes.c_uint64(seed), int(with_encoder),
                                                  ctypes.byref(self.h)))
        elif any(w is not None and np.asarray(w).dtype == np.float16 for w in (decoder_weights, encoder_weights)):
            d = None if decoder_weights is None else np.ascontiguousarray(decoder_weights, dtype=np.float16)
            e = None if encoder_weights is None else np.ascontiguousarray(encoder_weights, dtype=np.float16)
            _check(lib().sdxl_vae_create_f16(ctx.h, ctypes.byref(c), dtype,
                                            None if d is None else d.ctypes.data_as(ctypes.c_void_p),
                                            None if e is None else e.ctypes.data_as(ctypes.c_void_p), ctypes.byref(self.h)))
        else:
            d = None if decoder_weights is None else np.ascontiguousarray(decoder_weights, dtype=np.float32)
            e = None if encoder_weights is None else np.ascontiguousarray(encoder_weights, dtype=np.float32)
            _check(lib().sdxl_vae_create(ctx.h, ctypes.byref(c), dtype,
                                        None if d is None else d.ctypes.data_as(ctypes.c_void_p),
                                        None if e is None else e.ctypes.data_as(ctypes.c_void_p), ctypes.byref(self.h)))

    def decode_latent(self, latent):
        """LatentDecoder::decode_latent (:263-266): [n,4,h,w] -> [n,3,8h,8w]"""
        torch = _torch()
        latent, pl = _dev(latent)
        n, _, h, w = latent.shape
        out = torch.empty((n, 3, 8 * h, 8 * w), device=latent.device, dtype=torch.float32)
        _check(lib().sdxl_vae_decode_latent(self.h, _stream(), pl, n, h, w, ctypes.c_void_p(out.data_ptr())))
        return out

    def latent_to_image(self, latent) -> RawImages:
        """LatentDecoder::latent_to_image (:200-237)"""
        torch = _torch()
        latent, pl = _dev(latent)
        n, _, h, w = latent.shape
        out = torch.empty((n, 8 * h, 8 * w, 3), device=latent.device, dtype=torch.uint8)
        _check(lib().sdxl_latent_to_image(self.h, _stream(), pl, n, h, w, ctypes.c_void_p(out.data_ptr())))
        return RawImages(out, 8 * w, 8 * h)

    def encode_image(self, image):
        """LatentDecoder::encode_image (:257-261): [n,3,H,W] in [-1,1] -> [n,4,H/8,W/8]"""
        torch = _torch()
        image, pi = _dev(image)
        n, _, H, W = image.shape
        out = torch.empty((n, 4, H // 8, W // 8), device=image.device, dtype=torch.float32)
        _check(lib().sdxl_vae_encode_image(self.h, _stream(), pi, n, H, W, ctypes.c_void_p(out.data_ptr())))
        return out

    def image_to_latent(self, images: RawImages):
        """LatentDecoder::image_to_latent (:239-255)"""
        torch = _torch()
        buf, pb = _dev(images.buffer, torch.uint8)
        n = buf.shape[0]
        out = torch.empty((n, 4, images.height // 8, images.width // 8), device=buf.device, dtype=torch.float32)
        _check(lib().sdxl_image_to_latent(self.h, _stream(), pb, n, images.height, images.width, ctypes.c_void_p(out.data_ptr())))
        return out

    def weight_arena(self) -> Tuple[int, int]:
        base, n = ctypes.c_void_p(), ctypes.c_size_t()
        _check(lib().sdxl_vae_weight_arena(self.h, ctypes.byref(base), ctypes.byref(n)))
        return int(base.value or 0), int(n.value)

    def weight_arena_tensor(self):
        return arena_as_tensor(*self.weight_arena(), self.ctx.device_id)

    def __del__(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.sdxl_vae_destroy(self.h)
            self.h = None


# ---------------------------------------------------------------------------------------------------------------- ops

def qkv_attention(ctx: Context, q, k, v, mask, n_head: int, dtype: int = DTYPE_F16):
    """Backend::qkv_attention (src/backend.rs:4-19): q [B,Nq,C], k,v [B,Nk,C], additive mask [Nq,Nk] or None"""
    torch = _torch()
    q, pq = _dev(q)
    k, pk = _dev(k)
    v, pv = _dev(v)
    pm = None
    if mask is not None:
        mask, pm = _dev(mask)
    B, Nq, C = q.shape
    out = torch.empty_like(q)
    _check(lib().sdxl_qkv_attention(ctx.h, _stream(), pq, pk, pv, pm, B, Nq, int(k.shape[1]), C, n_head, dtype,
                                   ctypes.c_void_p(out.data_ptr())))
    return out


def attn_decoder_mask(ctx: Context, seq_length: int):
    """Backend::attn_decoder_mask (src/backend.rs:130-136)"""
    torch = _torch()
    out = torch.empty((seq_length, seq_length), device=f"cuda:{ctx.device_id}", dtype=torch.float32)
    _check(lib().sdxl_attn_decoder_mask(ctx.h, _stream(), seq_length, ctypes.c_void_p(out.data_ptr())))
    torch.cuda.synchronize()
    return out


def group_norm(ctx: Context, x, gamma, beta, n_group: int = 32, eps: float = 1e-5, silu: bool = False,
               dtype: int = DTYPE_F16):
    """GroupNorm::forward (groupnorm/mod.rs:52-73) on NCHW input, optional fused SILU (silu.rs:14-16)"""
    torch = _torch()
    x, px = _dev(x)
    gamma, pg = _dev(gamma)
    beta, pb = _dev(beta)
    B, C = x.shape[0], x.shape[1]
    HW = int(np.prod(x.shape[2:]))
    out = torch.empty_like(x)
    _check(lib().sdxl_group_norm(ctx.h, _stream(), px, pg, pb, B, C, HW, n_group, ctypes.c_float(eps), int(silu), dtype,
                                ctypes.c_void_p(out.data_ptr())))
    return out


def layer_norm(ctx: Context, x, gamma, beta, eps: float = 1e-5, dtype: int = DTYPE_F16):
    """LayerNorm::forward (layernorm/mod.rs:34-40)"""
    torch = _torch()
    x, px = _dev(x)
    gamma, pg = _dev(gamma)
    beta, pb = _dev(beta)
    C = x.shape[-1]
    out = torch.empty_like(x)
    _check(lib().sdxl_layer_norm(ctx.h, _stream(), px, pg, pb, int(x.numel() // C), C, ctypes.c_float(eps), dtype,
                                ctypes.c_void_p(out.data_ptr())))
    return out


def conv2d(ctx: Context, x, weight, bias, stride: int = 1, padding: int = 0, upsample: bool = False,
           dtype: int = DTYPE_F16):
    """burn Conv2d (weight [Cout,Cin,k,k]); upsample=True applies the reference's nearest-2x first (unet/mod.rs:744-750)"""
    torch = _torch()
    x, px = _dev(x)
    weight, pw = _dev(weight)
    pb = None
    if bias is not None:
        bias, pb = _dev(bias)
    B, Cin, H, W = x.shape
    Cout, _, k, _ = weight.shape
    Hs, Ws = (2 * H, 2 * W) if upsample else (H, W)
    Ho, Wo = (Hs + 2 * padding - k) // stride + 1, (Ws + 2 * padding - k) // stride + 1
    out = torch.empty((B, Cout, Ho, Wo), device=x.device, dtype=torch.float32)
    _check(lib().sdxl_conv2d(ctx.h, _stream(), px, pw, pb, B, Cin, H, W, Cout, k, stride, padding, int(upsample), dtype,
                            ctypes.c_void_p(out.data_ptr())))
    return out


def conv2d_upsample_folded(ctx: Context, x, weight, bias, dtype: int = DTYPE_F16):
    """nearest-2x upsample + Conv2d 3x3 pad 1 on the folded phase weights, as the f16 UNet / the split-operand VAE decoder run it; returns
    (out [B,Cout,2H,2W], folded): folded = False where the shape (or debug_set("upsample_fold", 0)) keeps the gather form"""
    torch = _torch()
    x, px = _dev(x)
    weight, pw = _dev(weight)
    pb = None
    if bias is not None:
        bias, pb = _dev(bias)
    B, Cin, H, W = x.shape
    Cout = int(weight.shape[0])
    out = torch.empty((B, Cout, 2 * H, 2 * W), device=x.device, dtype=torch.float32)
    took = ctypes.c_int(0)
    _check(lib().sdxl_conv2d_upsample_folded(ctx.h, _stream(), px, pw, pb, int(B), int(Cin), int(H), int(W), Cout, dtype, ctypes.byref(took),
                                            ctypes.c_void_p(out.data_ptr())))
    return out, bool(took.value)


def linear(ctx: Context, x, weight, bias, geglu: bool = False, dtype: int = DTYPE_F16):
    """burn nn::Linear: x[...,K] @ weight[K,N] + bias; geglu=True -> GEGLU::forward (unet/mod.rs:942-956)"""
    torch = _torch()
    x, px = _dev(x)
    weight, pw = _dev(weight)
    pb = None
    if bias is not None:
        bias, pb = _dev(bias)
    K, N = weight.shape
    M = int(x.numel() // K)
    out = torch.empty(tuple(x.shape[:-1]) + ((N // 2) if geglu else N,), device=x.device, dtype=torch.float32)
    _check(lib().sdxl_linear(ctx.h, _stream(), px, pw, pb, M, K, N, int(geglu), dtype, ctypes.c_void_p(out.data_ptr())))
    return out


def gemv(ctx: Context, x, weight, bias=None, yadd=None, silu_in: bool = False, silu_out: bool = False, dtype: int = DTYPE_F16, out=None):
    """the conditioning path's small-M linear on the UNet's GEMV kernel (time / label MLPs unet/mod.rs:458-468, lin_embed(silu(emb)) :1088-1089):
    silu_out?(silu_in?(x[Bm,K]) @ weight[K,N] + bias) + yadd[Bm,N].  dtype: DTYPE_F32 / DTYPE_F32_SPLIT (fp32 weights) or DTYPE_F16 (f16 weights).
    out: a contiguous fp32 CUDA tensor of at least Bm rows of N to write into (rows past Bm are left alone); returns its first Bm rows."""
    torch = _torch()
    x, px = _dev(x)
    weight, pw = _dev(weight)
    pb = py = None
    if bias is not None:
        bias, pb = _dev(bias)
    if yadd is not None:
        yadd, py = _dev(yadd)
    K, N = weight.shape
    Bm = int(x.numel() // K)
    if out is None:
        out = torch.empty((Bm, N), device=x.device, dtype=torch.float32)
    elif not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.dim() == 2 and out.shape[1] == N and out.shape[0] >= Bm):
        raise EngineError("gemv: out must be a contiguous fp32 CUDA tensor [>= Bm, N]")
    _check(lib().sdxl_gemv(ctx.h, _stream(), px, pw, pb, py, Bm, int(K), int(N), int(silu_in), int(silu_out), dtype, ctypes.c_void_p(out.data_ptr())))
    return out[:Bm]


def timestep_embedding(ctx: Context, t, dim: int):
    """timestep_embedding (unet/mod.rs:21-39) of the fp32 timesteps t [n] -> [n, dim] = [cos(t f) | sin(t f)]"""
    torch = _torch()
    t, pt = _dev(t)
    n = int(t.numel())
    out = torch.empty((n, dim), device=t.device, dtype=torch.float32)
    _check(lib().sdxl_timestep_embedding(ctx.h, _stream(), pt, n, int(dim), ctypes.c_void_p(out.data_ptr())))
    return out


def unet_skip_shapes(cfg: UNetConfig, H: int, W: int) -> List[Tuple[int, int, int]]:
    """(C, h, w) of every ControlNet residual tensor of a UNet on an H x W latent (sdxl_unet_skip_count / _skip_shape; host logic, no GPU needed):
    one per input entry, then the middle block's"""
    c = cfg.to_c()
    n = lib().sdxl_unet_skip_count(ctypes.byref(c))
    if n < 0:
        raise EngineError(lib().sdxl_last_error().decode())
    out = []
    chw = (ctypes.c_int64 * 3)()
    for i in range(n):
        _check_invalid(lib().sdxl_unet_skip_shape(ctypes.byref(c), i, int(H), int(W), chw))
        out.append((int(chw[0]), int(chw[1]), int(chw[2])))
    return out


def _skip_segments(name: str, segments, multi: bool = False):
    """the segment checks and the ctypes arrays behind skip_residual_add* (`name` heads the messages): segments = [(dst, src), ...], or with
    `multi` [(dst, [src_0 .. src_K-1]), ...], whose sources may hold fewer rows than dst (the caller checks what that needs).
    -> ([(dst, [srcs])], K, the arguments n_segments .. C of the C entry, its dtype code)"""
    torch = _torch()
    segments = [(d, list(ss) if multi else [ss]) for d, ss in segments]
    n = len(segments)
    if n < 1:
        raise InvalidArgument(f"{name}: at least one segment")
    K = len(segments[0][1])
    if not 1 <= K <= 4 or any(len(ss) != K for _, ss in segments):
        raise InvalidArgument(f"{name}: the number of sources K must be in 1..4, the same for every segment")
    dt = segments[0][0].dtype
    if dt not in (torch.float32, torch.float16):
        raise InvalidArgument(f"{name}: float32 or float16 tensors")
    for d, ss in segments:
        dst_ok = d.is_cuda and d.dim() == 2 and (d.shape[1] <= 1 or d.stride(1) == 1) and d.stride(0) >= d.shape[1]
        src_ok = dst_ok and d.dtype == dt and all(s.is_cuda and s.dtype == dt and s.dim() == 2 and s.is_contiguous() and s.shape[1] == d.shape[1]
                                                  and (s.shape[0] <= d.shape[0] if multi else s.shape[0] == d.shape[0]) for s in ss)
        if not multi and not src_ok:
            raise InvalidArgument(f"{name}: dst must be a [rows, C] view with contiguous columns and src a dense [rows, C] tensor, one dtype, on the GPU")
        if not dst_ok:
            raise InvalidArgument(f"{name}: dst must be a [rows, C] view with contiguous columns, on the GPU")
        if not src_ok:
            raise InvalidArgument(f"{name}: every src must be a dense [rows, C] tensor of dst's dtype and width, on the GPU")
    dst = (ctypes.c_void_p * n)(*[d.data_ptr() for d, _ in segments])
    src = (ctypes.c_void_p * (n * K))(*[s.data_ptr() for _, ss in segments for s in ss])
    ld = (ctypes.c_int64 * n)(*[int(d.stride(0)) for d, _ in segments])
    rows = (ctypes.c_int64 * n)(*[int(d.shape[0]) for d, _ in segments])
    cols = (ctypes.c_int32 * n)(*[int(d.shape[1]) for d, _ in segments])
    return segments, K, (n, dst, ld, src, rows, cols), DTYPE_F16 if dt == torch.float16 else DTYPE_F32


def _skip_scales(name: str, scales, shape: str, tail, step_idx):
    """the scale table [steps, *tail] and the step index of the trajectory forms -> (step_idx kept alive, its device pointer)"""
    torch = _torch()
    if not (torch.is_tensor(scales) and scales.is_cuda and scales.dtype == torch.float32 and tuple(scales.shape[1:]) == tail and scales.is_contiguous()):
        raise InvalidArgument(f"{name}: scales must be a contiguous float32 CUDA tensor {shape}")
    if not torch.is_tensor(step_idx):
        if not 0 <= int(step_idx) < scales.shape[0]:
            raise InvalidArgument(f"{name}: step_idx outside the scale table")
        step_idx = torch.tensor([int(step_idx)], dtype=torch.int32, device=scales.device)
    return _dev(step_idx, torch.int32)


def skip_residual_add(ctx: Context, segments, scale):
    """sdxl_skip_residual_add, the UNet's per-step ControlNet add on caller tensors, in place and in ONE launch: for every (dst, src) of `segments`
    (at most 16), dst[r, c] = round(fma(scale, src[r, c], dst[r, c])).  dst: a [rows, C] CUDA view whose columns are contiguous (a column slice of a
    wider row-major buffer), src: a dense [rows, C] tensor; all float32 or all float16.  scale: a float or a one-element fp32 CUDA tensor.
    InvalidArgument (nothing written): C % 8 != 0, a slice or a row pitch that is not 16-byte aligned."""
    torch = _torch()
    segments, _, (n, dst, ld, src, rows, cols), dtype = _skip_segments("skip_residual_add", segments)
    if not torch.is_tensor(scale):
        scale = torch.tensor([float(scale)], dtype=torch.float32, device=segments[0][0].device)
    scale, ps = _dev(scale)
    _check_invalid(lib().sdxl_skip_residual_add(ctx.h, _stream(), n, dst, ld, src, rows, cols, ps, dtype))


def skip_residual_add_steps(ctx: Context, segments, B: int, scales, step_idx):
    """sdxl_skip_residual_add_steps, the ControlNet add inside a trajectory: skip_residual_add with the scale of row r of a
    segment read from scales[step_idx, r // (rows // B)] -- scales: a float32 CUDA tensor [steps, 8], step_idx: an int or a one-element int32 CUDA
    tensor.  Rows whose scale is 0 are neither read nor written.  InvalidArgument (nothing written): what skip_residual_add refuses, B outside
    1..8, rows that are no multiple of B."""
    _, _, (n, dst, ld, src, rows, cols), dtype = _skip_segments("skip_residual_add_steps", segments)
    step_idx, pi = _skip_scales("skip_residual_add_steps", scales, "[steps, 8]", (8,), step_idx)
    _check_invalid(lib().sdxl_skip_residual_add_steps(ctx.h, _stream(), n, dst, ld, src, rows, cols, int(B), ctypes.c_void_p(scales.data_ptr()), pi, dtype))


def skip_residual_add_steps_multi(ctx: Context, segments, B: int, scales, step_idx):
    """sdxl_skip_residual_add_steps_multi, the ControlNet add of K nets in one launch: segments = [(dst, [src_0 .. src_K-1]), ...], scales a float32
    CUDA tensor [steps, K, 8]; source k of row r has the scale scales[step_idx, k, r // (rows // B)], the sum runs in fp32 over the sources in order and
    is rounded once.  A source at scale 0 is not read.  A source may hold fewer rows than dst (whole batch entries: a net run on the conditional
    entries alone) where every entry behind its end is at scale 0 in the row step_idx names -- checked here, by reading that row.
    InvalidArgument (nothing written): what skip_residual_add_steps refuses, K outside 1..4."""
    name = "skip_residual_add_steps_multi"
    segments, K, (n, dst, ld, src, rows, cols), dtype = _skip_segments(name, segments, multi=True)
    step_idx, pi = _skip_scales(name, scales, "[steps, K, 8]", (K, 8), step_idx)
    row = None
    for d, ss in segments:
        for k, s in enumerate(ss):
            if s.shape[0] < d.shape[0]:
                if not 1 <= int(B) <= 8 or d.shape[0] % int(B) != 0 or s.shape[0] % (d.shape[0] // int(B)) != 0:
                    raise InvalidArgument(f"{name}: a short source must hold whole batch entries (rows a multiple of B)")
                if row is None:
                    i = int(step_idx.item())
                    if not 0 <= i < scales.shape[0]:
                        raise InvalidArgument(f"{name}: step_idx outside the scale table")
                    row = scales[i].cpu()
                if bool((row[k, s.shape[0] // (d.shape[0] // int(B)):int(B)] != 0).any()):
                    raise InvalidArgument(f"{name}: a short source needs scale 0 for every entry behind its end")
    _check_invalid(lib().sdxl_skip_residual_add_steps_multi(ctx.h, _stream(), n, dst, ld, src, K, rows, cols, int(B), ctypes.c_void_p(scales.data_ptr()), pi,
                                                            dtype))


def _opt(t):
    """(tensor kept alive, device pointer) of an optional fp32 CUDA tensor (None -> a null pointer)"""
    return (None, None) if t is None else _dev(t)


def vae_attn_block(ctx: Context, x, gamma, beta, wq, bq, wk, bk, wv, bv, wo, bo, n_group: int = 32, eps: float = 1e-5, dtype: int = DTYPE_F32_SPLIT):
    """ConvSelfAttentionBlock::forward (autoencoder/mod.rs:550-586) on x [B,C,H,W] through the code the LatentDecoder's mid block runs: GroupNorm, the 1x1
    convolutions wq / wk / wv [C,C,1,1] (biases [C] or None), one head of C channels, wo + residual.  dtype: DTYPE_F32, DTYPE_F16 or DTYPE_F32_SPLIT."""
    torch = _torch()
    keep = [_opt(t) for t in (x, gamma, beta, wq, bq, wk, bk, wv, bv, wo, bo)]
    px, pg, pbe, pwq, pbq, pwk, pbk, pwv, pbv, pwo, pbo = [k[1] for k in keep]
    if x is None or x.dim() != 4:
        raise EngineError("vae_attn_block: x must be [B, C, H, W]")
    B, C, H, W = (int(v) for v in x.shape)
    out = torch.empty((B, C, H, W), device=x.device, dtype=torch.float32)
    _check(lib().sdxl_vae_attn_block(ctx.h, _stream(), px, pg, pbe, ctypes.c_float(eps), pwq, pbq, pwk, pbk, pwv, pbv, pwo, pbo, B, C, H, W, int(n_group),
                                     int(dtype), ctypes.c_void_p(out.data_ptr())))
    return out


def vae_res_block(ctx: Context, x, gamma1, beta1, w1, b1, gamma2, beta2, w2, b2, w_nin=None, b_nin=None, n_group: int = 32, eps1: float = 1e-5,
                  eps2: float = 1e-5, dtype: int = DTYPE_F32_SPLIT):
    """ResnetBlock::forward (autoencoder/mod.rs:500-516) on x [B,Cin,H,W] through the code every block of the LatentDecoder runs: w1 [Cout,Cin,3,3],
    w2 [Cout,Cout,3,3], w_nin [Cout,Cin,1,1] or None where Cin == Cout (biases [Cout] or None).  dtype: DTYPE_F32, DTYPE_F16 or DTYPE_F32_SPLIT."""
    torch = _torch()
    keep = [_opt(t) for t in (x, gamma1, beta1, w1, b1, gamma2, beta2, w2, b2, w_nin, b_nin)]
    px, pg1, pbe1, pw1, pb1, pg2, pbe2, pw2, pb2, pwn, pbn = [k[1] for k in keep]
    if x is None or x.dim() != 4:
        raise EngineError("vae_res_block: x must be [B, Cin, H, W]")
    B, Cin, H, W = (int(v) for v in x.shape)
    Cout = int(w2.shape[0]) if w2 is not None else Cin      # (a missing w2 is the library's error to report)
    out = torch.empty((B, Cout, H, W), device=x.device, dtype=torch.float32)
    _check(lib().sdxl_vae_res_block(ctx.h, _stream(), px, pg1, pbe1, ctypes.c_float(eps1), pw1, pb1, pg2, pbe2, ctypes.c_float(eps2), pw2, pb2, pwn, pbn,
                                    B, Cin, Cout, H, W, int(n_group), int(dtype), ctypes.c_void_p(out.data_ptr())))
    return out


def layer_norm_linear(ctx: Context, x, gamma, beta, weight, bias, eps: float = 1e-5, geglu: bool = False,
                      dtype: int = DTYPE_F16):
    """LayerNorm::forward (layernorm/mod.rs:34-49) then nn::Linear, as TransformerBlock::forward pairs them
    (unet/mod.rs:885-891).  DTYPE_F16 runs the LayerNorm FOLDED into the GEMM (the UNet's f16 path), the other dtypes the
    stand-alone LayerNorm kernel."""
    torch = _torch()
    x, px = _dev(x)
    gamma, pg = _dev(gamma)
    beta, pbeta = _dev(beta)
    weight, pw = _dev(weight)
    pb = None
    if bias is not None:
        bias, pb = _dev(bias)
    K, N = weight.shape
    M = int(x.numel() // K)
    out = torch.empty(tuple(x.shape[:-1]) + ((N // 2) if geglu else N,), device=x.device, dtype=torch.float32)
    _check(lib().sdxl_layer_norm_linear(ctx.h, _stream(), px, pg, pbeta, ctypes.c_float(eps), pw, pb, M, K, N, int(geglu),
                                       dtype, ctypes.c_void_p(out.data_ptr())))
    return out


def ln_query_cross_attention(ctx: Context, x, gamma, beta, wq, k, v, eps: float = 1e-5, fused: bool = True):
    """attn2 of a transformer block up to its output projection (unet/mod.rs:731-795): LayerNorm -> query projection (no
    bias) -> qkv_attention over the projected context k, v [B,Nk,C] with 64 channels per head.  f16 engine arithmetic.
    fused=True runs the attention inside the projection's epilogue (one launch: Nk <= 96, or Nk <= 384 where C % 128 == 0 -- the long form walks the
    context in 96-key blocks; anything else is refused), False as projection + attention kernel; fused=2 (Nk <= 96): that epilogue at
    split precision (context, q and P as (hi, lo) f16 pairs, three MFMAs per product: what SDXL_DTYPE_F32_SPLIT_MIX_F16W runs)."""
    torch = _torch()
    x, px = _dev(x)
    gamma, pg = _dev(gamma)
    beta, pbeta = _dev(beta)
    wq, pw = _dev(wq)
    k, pk = _dev(k)
    v, pv = _dev(v)
    B, Nq, C = x.shape
    Nk = int(k.shape[1])
    out = torch.empty((B, Nq, C), device=x.device, dtype=torch.float32)
    _check(lib().sdxl_ln_query_cross_attention(ctx.h, _stream(), px, pg, pbeta, ctypes.c_float(eps), pw, pk, pv, int(B), int(Nq),
                                              Nk, int(C), int(fused), ctypes.c_void_p(out.data_ptr())))
    return out


def conv2d_group_norm(ctx: Context, x, weight, bias, gamma, beta, eps: float = 1e-5, n_group: int = 32, silu: bool = True,
                      residual=None, fused: bool = True):
    """conv3x3 (pad 1, + residual) -> GroupNorm (+SiLU) as ResBlock::forward pairs them (unet/mod.rs:1082-1106), f16 engine.
    fused=True asks the convolution's epilogue for the GroupNorm statistics.  Returns (out, fused_taken)."""
    torch = _torch()
    x, px = _dev(x)
    weight, pw = _dev(weight)
    gamma, pg = _dev(gamma)
    beta, pbeta = _dev(beta)
    pb = pr = None
    if bias is not None:
        bias, pb = _dev(bias)
    if residual is not None:
        residual, pr = _dev(residual)
    B, Cin, H, W = x.shape
    Cout = int(weight.shape[0])
    out = torch.empty((B, Cout, H, W), device=x.device, dtype=torch.float32)
    took = ctypes.c_int(0)
    _check(lib().sdxl_conv2d_group_norm(ctx.h, _stream(), px, pw, pb, pr, pg, pbeta, ctypes.c_float(eps), int(B), int(Cin), int(H),
                                       int(W), Cout, int(n_group), int(silu), int(fused), ctypes.byref(took),
                                       ctypes.c_void_p(out.data_ptr())))
    return out, bool(took.value)


FORM_NATIVE, FORM_F16, FORM_F16_WHILO, FORM_F16_AHILO, FORM_X2 = 0, 1, 2, 3, 4   # include/sdxl_mi355.h SDXL_FORM_*
PROJ_QKV, PROJ_QUERY, PROJ_GEGLU = 0, 1, 2                                      # include/sdxl_mi355.h SDXL_PROJ_*


def transformer_projection(ctx: Context, r, gamma, beta, weight, bias, proj: int, form: int, eps: float = 1e-5, shadow: bool = False,
                           producer=None, batch: int = 1):
    """One LayerNorm-fed projection of a split-operand UNet's transformer block in form `form` (FORM_*), through the UNet's own code
    (sdxl_transformer_projection).  r [M, C] fp32 (M = batch x rows per entry); producer = (a [M, Kp], wp [Kp, C], bp [C] or None, form) adds
    a @ wp + bp to r the way an out-projection / FF-out writes the residual stream t; shadow=True asks that producer for the LayerNorm shadow.
    Returns (out [M, N] or [M, N/2] for PROJ_GEGLU, t [M, C], shadow_taken).  Unsupported arguments raise InvalidArgument."""
    torch = _torch()
    r, pr = _dev(r)
    gamma, pg = _dev(gamma)
    beta, pbeta = _dev(beta)
    weight, pw = _dev(weight)
    pb = None
    if bias is not None:
        bias, pb = _dev(bias)
    M, C = r.shape
    N = int(weight.shape[1])
    pa = pwp = pbp = None
    Kp, pform = 0, -1
    if producer is not None:
        a, wp, bp, pform = producer
        a, pa = _dev(a)
        wp, pwp = _dev(wp)
        if bp is not None:
            bp, pbp = _dev(bp)
        Kp = int(wp.shape[0])
    assert M % batch == 0
    out = torch.empty((M, N // 2 if proj == PROJ_GEGLU else N), device=r.device, dtype=torch.float32)
    t = torch.empty((M, C), device=r.device, dtype=torch.float32)
    took = ctypes.c_int(0)
    rc = lib().sdxl_transformer_projection(ctx.h, _stream(), int(batch), int(M // batch), int(C), pa, pwp, pbp, pr, Kp, int(pform), pg, pbeta,
                                           ctypes.c_float(eps), pw, pb, N, int(proj), int(form), int(shadow), ctypes.c_void_p(t.data_ptr()),
                                           ctypes.c_void_p(out.data_ptr()), ctypes.byref(took))
    if rc == 1:
        raise InvalidArgument(lib().sdxl_last_error().decode())
    _check(rc)
    return out, t, bool(took.value)


# ---------------------------------------------------------------------------------------------------------------- multi-GPU
def bcast_plan(nbytes: int, world: int, rank: int) -> Tuple[int, int, int, int]:
    """(piece_off, piece_len, tail_off, tail_len) of the library's weight-broadcast schedule for this rank: the root scatters
    `world` equal 256-byte-aligned pieces over its links, an in-place all-gather completes them, the tail is a small
    broadcast (csrc/comm.cpp).  Host-only: works without a GPU."""
    v = [ctypes.c_size_t() for _ in range(4)]
    _check(lib().sdxl_bcast_plan(ctypes.c_size_t(nbytes), world, rank, *[ctypes.byref(x) for x in v]))
    return tuple(int(x.value) for x in v)


class Comm:
    """RCCL communicator of the engine (one process per GPU).  `unique_id()` on rank 0 -> ship the 128 bytes to every rank
    over any host channel (here: the caller's torch.distributed group) -> Comm(device, rank, world, id)."""

    @staticmethod
    def unique_id() -> bytes:
        buf = (ctypes.c_char * 128)()
        _check(lib().sdxl_comm_unique_id(buf))
        return bytes(buf)

    def __init__(self, device_id: int, rank: int, world: int, uid: bytes):
        assert len(uid) == 128
        self.h = ctypes.c_void_p()
        self.rank, self.world = rank, world
        _check(lib().sdxl_comm_create(device_id, rank, world, ctypes.c_char_p(uid), ctypes.byref(self.h)))

    def bcast_unet(self, unet: "UNet", root: int = 0):
        _check(lib().sdxl_unet_bcast_weights(self.h, unet.h, root))

    def bcast_vae(self, vae: "LatentDecoder", root: int = 0):
        _check(lib().sdxl_vae_bcast_weights(self.h, vae.h, root))

    def bcast_clip(self, clip: "CLIP", root: int = 0):
        _check(lib().sdxl_clip_bcast_weights(self.h, clip.h, root))

    def bcast_buffer(self, tensor, root: int = 0):
        _check(lib().sdxl_bcast_buffer(self.h, None, ctypes.c_void_p(tensor.data_ptr()), ctypes.c_size_t(tensor.numel() * tensor.element_size()), root))

    def __del__(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.sdxl_comm_destroy(self.h)
            self.h = None
