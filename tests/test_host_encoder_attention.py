"""The encoder-attention switch and its keyword, without a GPU."""
import pytest

import diffusion_rs_amd as d
from diffusion_rs_amd import _lib as L


def test_switch_defaults_to_0_and_returns_what_it_was_given():
    lib = L.load()
    assert lib.fmi_get_encoder_attention() == 0 and d.get_encoder_attention() == "default"
    try:
        assert lib.fmi_set_encoder_attention(1) == 0 and lib.fmi_get_encoder_attention() == 1 and d.get_encoder_attention() == "mfma"
        assert lib.fmi_set_encoder_attention(2) == L.ERR_INVALID and b"kind must be 0 or 1" in lib.fmi_last_error() and lib.fmi_get_encoder_attention() == 1
    finally:
        d.set_encoder_attention("default")
    assert lib.fmi_get_encoder_attention() == 0


def test_bad_keyword_raises_by_name_before_anything_is_loaded():
    with pytest.raises(ValueError, match=r"encoder_attention must be one of \['default', 'mfma'\], got 'x'"):
        d.Pipeline(d.ModelSource.ModelId("/nonexistent"), encoder_attention="x")
    with pytest.raises(ValueError, match="encoder_attention must be one of"):
        d.ClipVisionModel(encoder_attention="fast")
    assert L.load().fmi_get_encoder_attention() == 0
