#!/usr/bin/env python
"""Generates tests/golden/siglip_redux.npz: what PIL and HuggingFace transformers compute on the seeded inputs of tests/redux_ref.py — an INDEPENDENT
derivation that pins that file's restatements (tests/test_host_redux.py), which in turn hold the kernels (tests/test_gpu_redux.py).

  resize_in/<case>, resize_out/<case>   a u8 picture and PIL's Image.resize((S, S), Image.BICUBIC) of it — straight to the square, as SiglipImageProcessor
                                        resizes — for every case of redux_ref.RESIZE_CASES
  hidden/<config>                       SiglipVisionModel's last_hidden_state (torch CPU, float32, B = 2) for every config of redux_ref.CONFIGS, on
                                        redux_ref.state_dict / pixel_values (the test regenerates both from their seeds); the model's pooling head keeps its
                                        own initialisation and plays no part in last_hidden_state

Only data is stored.  Written with PIL 12.2 and transformers 5.15; the tests need neither.  The summary it prints holds the restatement's distance from both,
which tests/test_host_redux.py asserts at 4 x (the tower) and at the project's resize criteria.  Run from the repository root:
    python tests/golden/gen_siglip_redux_fixtures.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import redux_ref as R  # noqa: E402
from tests.util import rel_l2  # noqa: E402

HF_BATCH = 2


def main():
    import PIL
    import transformers
    from PIL import Image
    from transformers import SiglipVisionConfig, SiglipVisionModel
    out = {}
    S = R.RESIZE_S
    for name, (shape, kind, seed) in R.RESIZE_CASES.items():
        src = R.picture(shape, kind, seed=seed)
        out[f"resize_in/{name}"] = src
        out[f"resize_out/{name}"] = np.asarray(Image.fromarray(src).resize((S, S), Image.BICUBIC))
        assert out[f"resize_out/{name}"].shape == (S, S, 3)
        diff = np.abs(R.resize_bicubic_u8(src, S, S).astype(int) - out[f"resize_out/{name}"].astype(int))
        print(f"resize {name} {shape} -> {S}x{S}: restatement vs PIL max {int(diff.max())}, share {float((diff > 0).mean()):.2e}")
    for name, cfg in R.CONFIGS.items():
        torch.manual_seed(0)
        model = SiglipVisionModel(SiglipVisionConfig(**cfg, hidden_act="gelu_pytorch_tanh", attention_dropout=0.0)).eval().float()
        sd = {k: torch.from_numpy(v) for k, v in R.state_dict(cfg).items()}
        own = model.state_dict()
        pre = "" if any(k.startswith("vision_model.") for k in own) else "vision_model."  # (a bare SiglipVisionModel's keys carry no prefix in transformers 5)
        extra = [k for k in own if pre + k not in sd and "position_ids" not in k and not (pre + k).startswith("vision_model.head.")]
        assert not extra and all(k[len(pre):] in own for k in sd), (extra, [k for k in sd if k[len(pre):] not in own])
        model.load_state_dict({k[len(pre):]: v for k, v in sd.items()}, strict=False)
        with torch.no_grad():
            o = model(pixel_values=torch.from_numpy(R.pixel_values(cfg, HF_BATCH)))
        out[f"hidden/{name}"] = o.last_hidden_state.numpy().astype(np.float32)
        print(f"tower {name}: f32 restatement vs transformers rel-L2 {rel_l2(R.reference(name, HF_BATCH), out[f'hidden/{name}']):.2e}")
    np.savez_compressed(R.GOLDEN, **out)
    print("wrote", R.GOLDEN, os.path.getsize(R.GOLDEN), "bytes;", len(out), "arrays; PIL", PIL.__version__, "transformers", transformers.__version__)


if __name__ == "__main__":
    main()
