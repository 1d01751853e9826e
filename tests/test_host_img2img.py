"""Image-to-image / inpainting, the parts that need no GPU: the schedule cut, the C-ABI surface, and the u8 -> f32 constant."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ["fmi_preprocess_u8", "fmi_latent_mask", "fmi_encode_latents", "fmi_scale_noise", "fmi_flux_denoise_inpaint"]


def test_img2img_timesteps_cuts_the_schedule_as_diffusers_does():
    from diffusion_rs_amd.pipeline import img2img_timesteps
    ts = [1.0 - i / 50 for i in range(51)]
    cut = img2img_timesteps(ts, 0.6)
    assert isinstance(cut, list) and len(cut) == 31 and cut == ts[20:] and cut[0] == ts[20]
    ts4 = [1.0, 0.9, 0.7, 0.4, 0.0]
    assert img2img_timesteps(ts4, 0.75) == ts4[1:]
    ts100 = list(np.linspace(1.0, 0.0, 101))
    assert int(100 * 0.29) == 28  # the float truncation diffusers' expression keeps
    assert len(img2img_timesteps(ts100, 0.29)) == 29 and img2img_timesteps(ts100, 0.29) == ts100[72:]
    for t in (ts, ts4, ts100):
        assert img2img_timesteps(t, 1.0) == list(t)
        assert img2img_timesteps(t, 1) == list(t)
    assert img2img_timesteps(tuple(ts4), 0.5) == ts4[2:]  # any sequence, a list comes back
    for bad in (0, 0.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="strength"):
            img2img_timesteps(ts4, bad)
    with pytest.raises(ValueError, match="no step"):
        img2img_timesteps(ts4, 0.2)  # int(4 * 0.2) == 0 steps


def test_new_entries_are_declared_and_listed():
    from diffusion_rs_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "flux_mi355x.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(fmi_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW_ENTRIES:
        assert name in declared, name
        assert name in L.EXPORTED, name
    assert len(set(L.EXPORTED)) == len(L.EXPORTED)
    assert re.search(r"#define\s+FMI_ABI_VERSION\s+6\b", hdr)  # an addition under the same number
    import diffusion_rs_amd as d
    for name in ("preprocess_u8", "latent_mask", "encode_latents", "scale_noise", "img2img_timesteps"):
        assert callable(getattr(d, name)), name


def test_bin_centre_round_trips_all_256_values():
    """x = (u + 0.5) / 127.5 - 1 in f32 is the centre of the bin that the truncating ((clamp(x) + 1) * 127.5) maps to u: all 256 values come back.
    The textbook u / 127.5 - 1 sits on the bin's lower edge and comes back one too low on 63 of them."""
    u = np.arange(256, dtype=np.uint8)
    f = np.float32

    def post(x):
        v = (np.clip(x, f(-1), f(1)) + f(1)) * f(127.5)
        assert v.dtype == np.float32
        return np.clip(np.trunc(v), 0, 255).astype(np.uint8)

    x = (u.astype(np.float32) + f(0.5)) / f(127.5) - f(1)
    assert x.dtype == np.float32 and x.min() > -1
    assert x[254] < 1 < x[255]  # 255 is the one-point bin x = 1: its "centre" lies just outside and the clamp brings it back
    np.testing.assert_array_equal(post(x), u)
    textbook = u.astype(np.float32) / f(127.5) - f(1)
    assert int((post(textbook) != u).sum()) == 63 and (post(textbook).astype(int) - u >= -1).all()
