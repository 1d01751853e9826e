"""The channel-conditioned denoise loop composed on the CPU oracle, and the numpy references of its glue.

`oracle.Flux(cfg)` takes ONE width for its embedder and its final projection.  Built with in_channels = 64 + Cc and loaded with the GPU model's weights, proj_out
zero-padded to 64 + Cc rows (oracle_state_dict), its prediction's first 64 columns are the conditioned model's and the padded ones come back exactly 0.  One step
is `om.forward(cat([x, cond], 2))[:, :, :64]`; the combine, the Euler step and the blend are tests/true_cfg_ref.py's expressions, on the 64-wide state.

VARIANTS are the plumbing mistakes a conditioned loop can make; the GPU test measures its result's distance to each of them on this same reference
(tests/test_gpu_control.py) and the CPU self-test (tests/test_host_control.py) shows they are far enough from the correct loop for that to mean something."""
import numpy as np

from tests import true_cfg_ref as R

f32 = np.float32
C_STATE = 64

VARIANTS = ("cond_zeroed", "cond_samples_swapped", "cond_columns_moved", "cond_rows_shifted")


def oracle_cfg(cfg):
    """The oracle's configuration for a GPU configuration with out_channels: both of its widths are the embedder's."""
    return {k: v for k, v in cfg.items() if k != "out_channels"}


def oracle_state_dict(sd, cfg):
    """The GPU model's weights for oracle.Flux(oracle_cfg(cfg)): proj_out zero-padded to in_channels rows."""
    K = cfg["in_channels"]
    out = dict(sd)
    w, b = np.asarray(sd["proj_out.weight"], np.float32), np.asarray(sd["proj_out.bias"], np.float32)
    out["proj_out.weight"] = np.concatenate([w, np.zeros((K - w.shape[0], w.shape[1]), np.float32)], 0)
    out["proj_out.bias"] = np.concatenate([b, np.zeros(K - b.shape[0], np.float32)], 0)
    return out


def wrong_cond(cond, variant):
    """The conditioning a wrong composition would feed: zeroed; the two samples' swapped; its columns rolled by 64 (reversed where that is the identity,
    Cc = 64); its rows shifted by one token."""
    if variant is None:
        return cond
    assert variant in VARIANTS
    if variant == "cond_zeroed":
        return np.zeros_like(cond)
    if variant == "cond_samples_swapped":
        return np.ascontiguousarray(cond[::-1])
    if variant == "cond_columns_moved":
        return np.ascontiguousarray(cond[:, :, ::-1]) if cond.shape[2] == 64 else np.roll(cond, 64, axis=2)
    return np.roll(cond, 1, axis=1)


def forward(om, x, cond, ids, txt, txt_ids, t, y, g):
    """One evaluation: the oracle on cat([x, cond], 2); the prediction's state columns."""
    return np.ascontiguousarray(om.forward(np.concatenate([x, cond], 2).astype(np.float32), ids, txt, txt_ids, t, y, g)[:, :, :x.shape[2]])


def control_loop(om, x, cond, ids, txt, txt_ids, y, g, ts, neg_txt=None, neg_y=None, scale=None, x0=None, noise=None, mask=None, variant=None):
    """The final latents (B,S,64) f32 of the composed loop over the schedule `ts` (len n + 1).  neg_txt / neg_y / scale: true CFG (both evaluations see the
    same cond).  x0 / noise / mask: the inpainting blend after every step.  variant: None for the correct loop, or one of VARIANTS."""
    x = np.ascontiguousarray(x, np.float32).copy()
    cond = wrong_cond(np.ascontiguousarray(cond, np.float32), variant)
    for i in range(len(ts) - 1):
        t = np.full(x.shape[0], f32(ts[i]), np.float32)
        gd = forward(om, x, cond, ids, txt, txt_ids, t, y, g)
        if neg_txt is not None:
            gd = R.combine(gd, forward(om, x, cond, ids, neg_txt, txt_ids, t, neg_y, g), scale)
        x = R.euler(x, gd, f32(ts[i + 1] - ts[i]))
        if mask is not None:
            x = R.blend(x, x0, noise, mask, ts[i + 1])
    return x


# ---- the glue kernels in numpy
def mask_bits(mask):
    return (np.asarray(mask, np.float32) >= f32(0.5)).astype(np.float32)


def mask_image(image, mask):
    """image (B,C,H,W) * (1 - b), b = mask >= 0.5 (mask (B,H,W)) — one f32 product per element, as the kernel."""
    return (np.asarray(image, np.float32) * (f32(1) - mask_bits(mask))[:, None]).astype(np.float32)


def pack_mask(mask):
    """The 256 mask channels of FLUX.1 Fill by the index formula of include/flux_mi355x.h: (B,H,W) -> (B,(H/16)(W/16),256)."""
    b = mask_bits(mask)
    B, H, W = b.shape
    h2, w2 = H // 16, W // 16
    out = np.empty((B, h2 * w2, 256), np.float32)
    for py in range(8):
        for px in range(8):
            for dy in range(2):
                for dx in range(2):
                    out[:, :, (py * 8 + px) * 4 + dy * 2 + dx] = b[:, 8 * dy + py::16, 8 * dx + px::16].reshape(B, h2 * w2)
    return out


def pack_mask_view_chain(mask, pack_latents):
    """The same through diffusers' chain: view(B,h,8,w,8).permute(0,2,4,1,3).reshape(B,64,h,w), then pack_latents (oracle.pack_latents)."""
    b = mask_bits(mask)
    B, H, W = b.shape
    h, w = H // 8, W // 8
    return pack_latents(np.ascontiguousarray(b.reshape(B, h, 8, w, 8).transpose(0, 2, 4, 1, 3).reshape(B, 64, h, w)))[0]


def fill_condition(masked_latents, mask):
    return np.concatenate([np.asarray(masked_latents, np.float32), pack_mask(mask)], 2)
