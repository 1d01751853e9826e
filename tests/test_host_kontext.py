"""Reference-image (FLUX.1 Kontext) conditioning, the parts that need no device: which pipeline classes the loader accepts, the new
C-ABI symbols, and the shape rules of `reference=`."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from diffusion_rs_amd import _lib as L
from diffusion_rs_amd import loader
from diffusion_rs_amd.pipeline import check_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("fmi_flux_forward_context", "fmi_flux_denoise_context", "fmi_latent_ids")


def test_loader_accepts_flux_and_kontext_pipelines_only():
    assert loader.check_pipeline_class("FluxPipeline") == "FluxPipeline"
    assert loader.check_pipeline_class("FluxKontextPipeline") == "FluxKontextPipeline"
    for other in ("FluxFillPipeline", "StableDiffusionPipeline", "fluxpipeline", "", None):
        with pytest.raises(ValueError, match="^Only FluxPipeline is supported$"):
            loader.check_pipeline_class(other)


def test_new_symbols_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "flux_mi355x.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = L.load()
    for s in NEW_SYMBOLS:
        assert s in L.EXPORTED
        assert re.search(r"\bint\s+" + s + r"\s*\(", code), s
        assert hasattr(lib, s)
    assert re.search(r"typedef\s+struct\s+fmi_flux_context\s*\{", code)
    assert lib.fmi_abi_version() == 6 and "#define FMI_ABI_VERSION 6" in hdr
    # the ctypes mirror of fmi_flux_context: pointer, int, pointer, int with C's padding
    assert [f[0] for f in L.FluxContext._fields_] == ["ctx", "ctx_dtype", "ctx_ids", "R"]
    assert L.FluxContext.ctx_ids.offset == 16 and L.FluxContext.R.offset == 24


def test_latent_ids_rejects_bad_arguments_before_any_launch():
    lib = L.load()
    assert lib.fmi_latent_ids(1, 2, 2, 0.0, 0.0, 0.0, None, None) == L.ERR_INVALID
    out = (C.c_float * 12)()  # a non-null output: the sizes themselves are refused (nothing is launched)
    assert lib.fmi_latent_ids(-1, 2, 2, 0.0, 0.0, 0.0, out, None) == L.ERR_INVALID
    assert lib.fmi_latent_ids(1, -2, 2, 0.0, 0.0, 0.0, out, None) == L.ERR_INVALID


def test_check_reference_shapes():
    B = 2
    u = torch.zeros((96, 64, 3), dtype=torch.uint8)
    assert tuple(check_reference(u, B).shape) == (1, 96, 64, 3)  # one image: a batch dimension is added, the caller broadcasts
    assert tuple(check_reference(torch.zeros((2, 96, 64, 3), dtype=torch.uint8), B).shape) == (2, 96, 64, 3)
    assert tuple(check_reference(torch.zeros((1, 3, 32, 48)), B).shape) == (1, 3, 32, 48)
    assert check_reference(torch.zeros((2, 3, 32, 48), dtype=torch.float64), B).dtype == torch.float64
    with pytest.raises(ValueError, match="multiples of 16"):
        check_reference(torch.zeros((72, 64, 3), dtype=torch.uint8), B)
    with pytest.raises(ValueError, match="multiples of 16"):
        check_reference(torch.zeros((2, 3, 64, 40)), B)
    with pytest.raises(ValueError, match="multiples of 16"):
        check_reference(torch.zeros((0, 64, 3), dtype=torch.uint8), B)
    with pytest.raises(ValueError, match="uint8 reference must be"):
        check_reference(torch.zeros((96, 64), dtype=torch.uint8), B)  # rank
    with pytest.raises(ValueError, match="uint8 reference must be"):
        check_reference(torch.zeros((2, 3, 96, 64), dtype=torch.uint8), B)  # channels first is the float form
    with pytest.raises(ValueError, match="float reference must be"):
        check_reference(torch.zeros((96, 64, 3)), B)
    with pytest.raises(ValueError, match="uint8 or float"):
        check_reference(torch.zeros((96, 64, 3), dtype=torch.int32), B)
    with pytest.raises(ValueError, match="3 samples for 2 prompts"):
        check_reference(torch.zeros((3, 96, 64, 3), dtype=torch.uint8), B)
    with pytest.raises(ValueError, match="numpy array or a torch tensor"):
        check_reference(np.zeros((96, 64, 3), np.uint8), B)  # (Pipeline converts numpy before it checks)
