"""diffusion-rs_amd — MI355X-native FLUX.1 denoise path (drop-in for the hot path of
EricLBuehler/diffusion-rs).  Import as `diffusion_rs_amd` (see ../diffusion_rs_amd.py)."""
from ._lib import FmiError, LIB_PATH, load  # noqa: F401
from .flux import (AutoEncoderKl, FLUX_DEV, FLUX_SCHNELL, FluxModel, SchedulerConfig, VAE_FLUX, encode_latents, latent_ids, latent_mask, pack_latents,  # noqa: F401
                   postprocess_u8, preprocess_u8, randn_latents, scale_noise, unpack_latents, cfg_euler_step, cast_cols_bf16, fill_condition, mask_image,
                   FluxControlNetModel, add_scaled_rows_bf16, FluxIPAdapter, ip_attention, f8_dequantize, heun_predict, heun_correct, dpmpp_2m_step,
                   dpmpp_2m_coefficients, check_solver_args)
from .pipeline import DiffusionGenerationParams, ModelDType, ModelSource, Offloading, Pipeline, encode_png, img2img_timesteps  # noqa: F401
from .text import (CLIP_L, CLIP_VISION_L, SIGLIP_SO400M, T5_XXL, ClipTextTransformer, ClipVisionModel, ReduxImageEmbedder, SiglipVisionModel, T5EncoderModel,  # noqa: F401
                   load_bpe_tokenizer, tokenize_and_pad)
from . import synth  # noqa: F401
from . import lora  # noqa: F401
from .lora import AdapterTerm, read_adapter, read_lora  # noqa: F401
