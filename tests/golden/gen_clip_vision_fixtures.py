#!/usr/bin/env python
"""Generates tests/golden/clip_vision.npz: what PIL and HuggingFace transformers compute on the seeded inputs of tests/clip_vision_ref.py — an INDEPENDENT
derivation that pins that file's restatements (tests/test_host_clip_vision.py), which in turn hold the kernels (tests/test_gpu_clip_vision.py).

  resize_in/<case>, resize_out/<case>   a u8 picture and PIL's Image.resize((nw, nh), Image.BICUBIC) of it, for every case of clip_vision_ref.RESIZE_CASES
  embeds/<config>, hidden/<config>      CLIPVisionModelWithProjection's image_embeds and last_hidden_state (torch CPU, float32, B = 2) for every config of
                                        clip_vision_ref.CONFIGS, on clip_vision_ref.state_dict / pixel_values (the test regenerates both from their seeds)

Only data is stored.  Written with PIL 12.2 and transformers 5.15; the tests need neither.  Run from the repository root:
    python tests/golden/gen_clip_vision_fixtures.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import clip_vision_ref as R  # noqa: E402

HF_BATCH = 2


def main():
    import PIL
    import transformers
    from PIL import Image
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
    out = {}
    for i, (name, (shape, (nh, nw), kind)) in enumerate(R.RESIZE_CASES.items()):
        src = R.picture(shape, kind, seed=100 + i)
        out[f"resize_in/{name}"] = src
        out[f"resize_out/{name}"] = np.asarray(Image.fromarray(src).resize((nw, nh), Image.BICUBIC))
        assert out[f"resize_out/{name}"].shape == (nh, nw, 3)
    for name, cfg in R.CONFIGS.items():
        model = CLIPVisionModelWithProjection(CLIPVisionConfig(**cfg, hidden_act="quick_gelu", layer_norm_eps=1e-5, attention_dropout=0.0)).eval().float()
        sd = {k: torch.from_numpy(v) for k, v in R.state_dict(cfg).items()}
        own = model.state_dict()
        extra = [k for k in own if k not in sd and "position_ids" not in k]
        assert not extra and all(k in own for k in sd), (extra, [k for k in sd if k not in own])
        model.load_state_dict(sd, strict=False)
        with torch.no_grad():
            o = model(pixel_values=torch.from_numpy(R.pixel_values(cfg, HF_BATCH)))
        out[f"embeds/{name}"] = o.image_embeds.numpy().astype(np.float32)
        out[f"hidden/{name}"] = o.last_hidden_state.numpy().astype(np.float32)
    np.savez_compressed(R.GOLDEN, **out)
    print("wrote", R.GOLDEN, os.path.getsize(R.GOLDEN), "bytes;", len(out), "arrays; PIL", PIL.__version__, "transformers", transformers.__version__)


if __name__ == "__main__":
    main()
