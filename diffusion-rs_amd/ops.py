"""Op-level seams that are not part of a model handle: the d = 64 attention of the encoders and the switch that sends the encoders to it."""
import ctypes as C

import torch

from . import _lib as L
from .flux import _ptr, _stream

ENCODER_ATTENTION = {"default": 0, "mfma": 1}


def encoder_attention_kind(name) -> int:
    """"default" | "mfma" -> fmi_set_encoder_attention's number; anything else raises by name."""
    if name not in ENCODER_ATTENTION:
        raise ValueError(f"encoder_attention must be one of {sorted(ENCODER_ATTENTION)}, got {name!r}")
    return ENCODER_ATTENTION[name]


def set_encoder_attention(name) -> None:
    """The process-wide attention kernel of the T5, CLIP text and CLIP vision layers (fmi_set_encoder_attention): "default" = the lane-per-key kernel (at
    most 1024 tokens), "mfma" = the kernel of sdpa_d64 (any length).  Needs no GPU."""
    L.check(L.load().fmi_set_encoder_attention(encoder_attention_kind(name)))


def get_encoder_attention() -> str:
    kind = L.load().fmi_get_encoder_attention()
    return next(k for k, v in ENCODER_ATTENTION.items() if v == kind)


def sdpa_d64(q, k, v, bias=None, causal=False, scale=None):
    """fmi_sdpa_d64_bf16: softmax(q k^T * scale + bias [+ causal]) v at head dim 64.  q (B,Tq,H,64), k and v (B,Tk,H,64) bfloat16 with unit stride inside a
    head, any other strides (views of a fused projection are read where they lie); bias (H,Tq,Tk) float32 or None; causal: key j > query i is masked; scale:
    1 / sqrt(64) by default (T5 passes 1).  Returns (B,Tq,H,64) bfloat16.  A bias of -inf masks a key, on any part of a row (whole 64-key tiles included);
    a row whose visible keys are all masked that way is unsupported: its output is undefined (the kernel divides by a row sum of 0)."""
    for name, t in (("q", q), ("k", k), ("v", v)):
        if t.dtype != torch.bfloat16 or t.dim() != 4 or t.shape[3] != 64 or t.stride(3) != 1 or not t.is_cuda:
            raise TypeError(f"sdpa_d64: {name} must be a bfloat16 device tensor (B,T,H,64) with contiguous heads, got {t.dtype} {tuple(t.shape)}")
    B, Tq, H, _ = (int(x) for x in q.shape)
    Tk = int(k.shape[1])
    if tuple(k.shape) != (B, Tk, H, 64) or tuple(v.shape) != tuple(k.shape) or Tq < 1 or Tk < 1:
        raise ValueError(f"sdpa_d64: shapes q {tuple(q.shape)}, k {tuple(k.shape)}, v {tuple(v.shape)} do not fit")
    if bias is not None:
        if bias.dtype != torch.float32 or tuple(bias.shape) != (H, Tq, Tk) or not bias.is_cuda:
            raise TypeError(f"sdpa_d64: bias must be a float32 device tensor ({H},{Tq},{Tk}), got {bias.dtype} {tuple(bias.shape)}")
        bias = bias.contiguous()
    out = torch.empty((B, Tq, H, 64), dtype=torch.bfloat16, device=q.device)
    strides = (C.c_int64 * 12)(*(int(t.stride(i)) for t in (q, k, v, out) for i in (0, 1, 2)))
    L.check(L.load().fmi_sdpa_d64_bf16(_ptr(q), _ptr(k), _ptr(v), _ptr(out), B, H, Tq, Tk, strides, float(64 ** -0.5 if scale is None else scale), _ptr(bias),
                                       1 if causal else 0, _stream()))
    return out


def sdpa_d512(q, k, v, scale=None, out=None):
    """fmi_sdpa_d512_bf16: softmax(q k^T * scale) v for one head of width 512.  q (B,Lq,512), k and v (B,Lk,512) bfloat16 device tensors with
    unit stride along the channels, 16-byte aligned, row strides multiples of 8 (column windows of a fused projection are read where they lie); scale:
    1 / sqrt(512) by default.  Returns (B,Lq,512) bfloat16 — a new tensor, or `out` (a view with the same rules) written in place."""
    for name, t in (("q", q), ("k", k), ("v", v)) + ((("out", out),) if out is not None else ()):
        if t.dtype != torch.bfloat16 or t.dim() != 3 or t.shape[2] != 512 or t.stride(2) != 1 or not t.is_cuda:
            raise TypeError(f"sdpa_d512: {name} must be a bfloat16 device tensor (B,L,512) with contiguous channels, got {t.dtype} {tuple(t.shape)}")
    B, Lq, _ = (int(x) for x in q.shape)
    Lk = int(k.shape[1])
    if tuple(k.shape) != (B, Lk, 512) or tuple(v.shape) != tuple(k.shape) or Lq < 1 or Lk < 1 or (out is not None and tuple(out.shape) != tuple(q.shape)):
        raise ValueError(f"sdpa_d512: shapes q {tuple(q.shape)}, k {tuple(k.shape)}, v {tuple(v.shape)} do not fit")
    if out is None:
        out = torch.empty((B, Lq, 512), dtype=torch.bfloat16, device=q.device)
    strides = (C.c_int64 * 8)(*(int(t.stride(i)) for t in (q, k, v, out) for i in (1, 0)))
    L.check(L.load().fmi_sdpa_d512_bf16(_ptr(q), _ptr(k), _ptr(v), _ptr(out), B, Lq, Lk, strides, float(512 ** -0.5 if scale is None else scale), _stream()))
    return out


def sdpa_groups(q, k, v, q_groups, k_groups, scale=None, out_token_major=False, k_weights=None):
    """fmi_sdpa_groups_bf16: softmax(q k^T * scale + M) v at head dim 128 with token group masks — query i sees key j iff
    (q_groups[i] & k_groups[j]) != 0.  q (B,H,Lq,128), k and v (B,H,Lk,128) bfloat16 device tensors; q_groups (Bg,Lq) and k_groups (Bg,Lk) integers that fit
    32 bits (any device; (L,) is Bg = 1), Bg 1 — one set for the batch — or B.  scale: 1 / sqrt(128) by default.  Returns (B,H,Lq,128), or (B,Lq,H*128) with
    out_token_major.  Where Lq == Lk the words are checked for self-visibility (q_groups[i] & k_groups[i]); otherwise the caller guarantees a visible key for
    every query — a row without one is undefined.
    k_weights (fmi_sdpa_groups_weighted_bf16): None — the call above —, or one float weight per key, (Bg,Lk) or (Lk,) for Bg = 1, finite and
    > 0: key j counts w_j-fold in every softmax that sees it, softmax(s + ln w).  Host data is checked here; a device tensor is taken as it is (no wait)."""
    for name, t in (("q", q), ("k", k), ("v", v)):
        if t.dtype != torch.bfloat16 or t.dim() != 4 or t.shape[3] != 128 or not t.is_cuda:
            raise TypeError(f"sdpa_groups: {name} must be a bfloat16 device tensor (B,H,L,128), got {t.dtype} {tuple(t.shape)}")
    B, H, Lq, _ = (int(x) for x in q.shape)
    Lk = int(k.shape[2])
    if tuple(k.shape) != (B, H, Lk, 128) or tuple(v.shape) != tuple(k.shape) or Lq < 1 or Lk < 1:
        raise ValueError(f"sdpa_groups: shapes q {tuple(q.shape)}, k {tuple(k.shape)}, v {tuple(v.shape)} do not fit")
    qg, kg = (torch.atleast_2d(torch.as_tensor(g)).to(torch.int64).bitwise_and(0xFFFFFFFF) for g in (q_groups, k_groups))
    Bg = int(qg.shape[0])
    if tuple(qg.shape) != (Bg, Lq) or tuple(kg.shape) != (Bg, Lk) or Bg not in (1, B):
        raise ValueError(f"sdpa_groups: q_groups {tuple(qg.shape)} and k_groups {tuple(kg.shape)} must be (Bg,{Lq}) and (Bg,{Lk}) with Bg 1 or {B}")
    if Lq == Lk and not bool((qg.cpu() & kg.cpu()).ne(0).all()):
        raise ValueError("sdpa_groups: a token does not see itself ((q_groups[i] & k_groups[i]) == 0): a row without a visible key is not supported")
    # uint32 words as int32 bit patterns on the device (torch has no uint32 arithmetic everywhere)
    qg, kg = (g.where(g < 2 ** 31, g - 2 ** 32).to(torch.int32).to(q.device).contiguous() for g in (qg, kg))
    q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
    out = torch.empty((B, Lq, H * 128) if out_token_major else (B, H, Lq, 128), dtype=torch.bfloat16, device=q.device)
    if k_weights is None:
        L.check(L.load().fmi_sdpa_groups_bf16(_ptr(q), _ptr(k), _ptr(v), _ptr(out), B, H, Lq, Lk, 128, float(128 ** -0.5 if scale is None else scale),
                                              1 if out_token_major else 0, _ptr(qg), _ptr(kg), Bg, _stream()))
        return out
    kw = torch.atleast_2d(torch.as_tensor(k_weights)).to(torch.float32)
    if tuple(kw.shape) != (Bg, Lk):
        raise ValueError(f"sdpa_groups: k_weights {tuple(kw.shape)} must be ({Bg},{Lk}), one weight per key and per sample of the groups")
    if not kw.is_cuda and not bool((torch.isfinite(kw) & (kw > 0)).all()):
        raise ValueError("sdpa_groups: k_weights must be finite and > 0 (a weight of 0 is not a way to hide a key: that is the group words' job)")
    kw = kw.to(q.device).contiguous()
    L.check(L.load().fmi_sdpa_groups_weighted_bf16(_ptr(q), _ptr(k), _ptr(v), _ptr(out), B, H, Lq, Lk, 128, float(128 ** -0.5 if scale is None else scale),
                                                   1 if out_token_major else 0, _ptr(qg), _ptr(kg), _ptr(kw), Bg, _stream()))
    return out


def sdpa_blocks(q, k, v, row_ptr, cols, scale=None, order=None, out_token_major=False):
    """fmi_sdpa_blocks_bf16: softmax(q k^T * scale + M) v at head dim 128 with a block-sparse mask — the queries of block i // 128 see the keys
    of the 64-key tiles cols[row_ptr[i // 128] : row_ptr[i // 128 + 1]] and no others.  q (B,H,Lq,128), k and v (B,H,Lk,128) bfloat16 device tensors; row_ptr
    (ceil(Lq / 128) + 1,) and cols integers, one set for all samples and heads: rows non-empty, tiles strictly ascending in [0, ceil(Lk / 64)).  order: the
    launch order of the query blocks, a permutation (None: long lists first); it changes no bit of the result.  Host lists are checked and uploaded here;
    device tensors (all of row_ptr, cols and order, int32) are taken as they are (no wait).  Returns (B,H,Lq,128), or (B,Lq,H*128) with out_token_major."""
    import numpy as np

    from .flux import attention_blocks_order, check_attention_blocks
    for name, t in (("q", q), ("k", k), ("v", v)):
        if t.dtype != torch.bfloat16 or t.dim() != 4 or t.shape[3] != 128 or not t.is_cuda:
            raise TypeError(f"sdpa_blocks: {name} must be a bfloat16 device tensor (B,H,L,128), got {t.dtype} {tuple(t.shape)}")
    B, H, Lq, _ = (int(x) for x in q.shape)
    Lk = int(k.shape[2])
    if tuple(k.shape) != (B, H, Lk, 128) or tuple(v.shape) != tuple(k.shape) or Lq < 1 or Lk < 1:
        raise ValueError(f"sdpa_blocks: shapes q {tuple(q.shape)}, k {tuple(k.shape)}, v {tuple(v.shape)} do not fit")
    nqb, nt = -(-Lq // 128), -(-Lk // 64)
    lists = (row_ptr, cols) if order is None else (row_ptr, cols, order)
    if all(isinstance(a, torch.Tensor) and a.is_cuda for a in lists):
        if order is None:
            raise ValueError("sdpa_blocks: device lists need a device order (the entry does not wait for the device to sort them)")
        if any(a.dtype != torch.int32 or a.dim() != 1 for a in lists) or row_ptr.numel() != nqb + 1 or order.numel() != nqb:
            raise ValueError(f"sdpa_blocks: device row_ptr ({nqb + 1},), cols and order ({nqb},) must be int32 vectors")
        rp, cl, od = (a.contiguous() for a in lists)
    else:
        rp, cl = check_attention_blocks(*(a.cpu().numpy() if isinstance(a, torch.Tensor) else a for a in (row_ptr, cols)), nqb, nt)
        od = attention_blocks_order(rp) if order is None else np.asarray(order.cpu() if isinstance(order, torch.Tensor) else order).astype(np.int32)
        if od.shape != (nqb,) or not np.array_equal(np.sort(od), np.arange(nqb)):
            raise ValueError(f"sdpa_blocks: order must be a permutation of the {nqb} query blocks")
        rp, cl, od = (torch.from_numpy(np.ascontiguousarray(a)).to(q.device) for a in (rp, cl, od))
    q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
    out = torch.empty((B, Lq, H * 128) if out_token_major else (B, H, Lq, 128), dtype=torch.bfloat16, device=q.device)
    L.check(L.load().fmi_sdpa_blocks_bf16(_ptr(q), _ptr(k), _ptr(v), _ptr(out), B, H, Lq, Lk, 128, float(128 ** -0.5 if scale is None else scale),
                                          1 if out_token_major else 0, _ptr(rp), _ptr(cl), _ptr(od), nqb, int(cl.numel()), _stream()))
    return out
