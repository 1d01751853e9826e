"""The true-CFG denoise loop composed on the CPU oracle: `om.forward` twice per step — the prompt's and the negative's evaluation on the same
state, ids, guidance and context rows — then the combine, the Euler step and the blend in numpy f32, in the library's expressions:

    d = pos - neg;  g = neg + scale * d;  e = x + g * dt;  [k = (1 - s) * x0 + s * noise;  x = m * e + (1 - m) * k]

Every product and sum below is rounded to f32 on its own; the library may contract a product into the following sum, which moves a value by an ulp and never
changes the two exact cases (pos == neg, scale == 0: g == neg).  VARIANTS are the plumbing mistakes a loop can make; the GPU test measures its result's
distance to each of them on this same reference (tests/test_gpu_true_cfg.py), and the CPU self-test (tests/test_host_true_cfg.py) shows they are far enough
from the correct loop for that to mean something."""
import numpy as np

f32 = np.float32

VARIANTS = ("positive_only", "negative_only", "swapped", "negative_txt_with_positive_y", "other_samples_negative")
SCALE_VARIANT = "scale_3.9"  # a wrong number, not wrong plumbing: 2e-4 from the correct loop at scale 4, below what bf16 evaluations resolve; reported only


def combine(pos, neg, scale):
    d = (pos - neg).astype(np.float32)
    return (neg + f32(scale) * d).astype(np.float32)


def euler(x, g, dt):
    return (x + (g * f32(dt)).astype(np.float32)).astype(np.float32)


def blend(e, x0, noise, mask, s):
    s = f32(s)
    a = f32(1) - s
    k = ((a * x0).astype(np.float32) + (s * noise).astype(np.float32)).astype(np.float32)
    keep = (f32(1) - mask).astype(np.float32)
    return ((mask * e).astype(np.float32) + (keep * k).astype(np.float32)).astype(np.float32)


def _forward(om, x, ids, txt, txt_ids, t, y, g, ctx, rids):
    if ctx is None:
        return om.forward(x, ids, txt, txt_ids, t, y, g)
    S = x.shape[1]
    return om.forward(np.concatenate([x, ctx], 1), np.concatenate([ids, rids], 1), txt, txt_ids, t, y, g)[:, :S]


def cfg_loop(om, x, ids, txt, txt_ids, y, neg_txt, neg_y, g, ts, scale, ctx=None, rids=None, x0=None, noise=None, mask=None, variant=None):
    """The final latents (B,S,C) f32 of the composed loop over the schedule `ts` (len n + 1).  g: the guidance vector or None.  ctx / rids: reference-image rows
    and their ids, appended to both evaluations.  x0 / noise / mask: the inpainting blend after every step.  variant: None for the correct loop, or one of
    VARIANTS (or SCALE_VARIANT)."""
    assert variant is None or variant in VARIANTS or variant == SCALE_VARIANT
    x = np.ascontiguousarray(x, np.float32).copy()
    if variant == "negative_txt_with_positive_y":
        neg_y = y
    if variant == "other_samples_negative":
        neg_txt, neg_y = np.ascontiguousarray(neg_txt[::-1]), np.ascontiguousarray(neg_y[::-1])
    if variant == "scale_3.9":
        scale = 3.9
    for i in range(len(ts) - 1):
        t = np.full(x.shape[0], f32(ts[i]), np.float32)
        pos = neg = None
        if variant != "negative_only":
            pos = _forward(om, x, ids, txt, txt_ids, t, y, g, ctx, rids)
        if variant != "positive_only":
            neg = _forward(om, x, ids, neg_txt, txt_ids, t, neg_y, g, ctx, rids)
        if variant == "positive_only":
            gd = pos
        elif variant == "negative_only":
            gd = neg
        elif variant == "swapped":
            gd = combine(neg, pos, scale)
        else:
            gd = combine(pos, neg, scale)
        x = euler(x, gd, f32(ts[i + 1] - ts[i]))
        if mask is not None:
            x = blend(x, x0, noise, mask, ts[i + 1])
    return x
