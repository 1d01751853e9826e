"""The VAE mid-attention switch and the d = 512 op are declared, exported and bound, and Pipeline takes the keyword — without a GPU."""
import inspect
import os

import pytest

import diffusion_rs_amd as d
from diffusion_rs_amd import _lib as L

NAMES = ("fmi_vae_set_mid_attention", "fmi_vae_get_mid_attention", "fmi_sdpa_d512_bf16")


def test_setters_are_declared_exported_and_bound_and_pipeline_takes_the_keyword():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "flux_mi355x.h")).read()
    lib = L.load()
    for name in NAMES:
        assert f"{name}(" in header and name in L.EXPORTED and getattr(lib, name).argtypes is not None
    assert callable(d.sdpa_d512) and callable(d.AutoEncoderKl.set_mid_attention) and callable(d.AutoEncoderKl.get_mid_attention)
    assert inspect.signature(d.Pipeline.__init__).parameters["vae_attention"].default == "default"
    with pytest.raises(ValueError, match=r"vae_attention must be one of \['default', 'flash'\], got 'x'"):
        d.Pipeline(d.ModelSource.ModelId("/nonexistent"), vae_attention="x")
