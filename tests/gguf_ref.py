"""Test helper (not product code) for the GGUF tests: a NumPy restatement of the reference's eight `to_float` functions, a minimal GGUF v3 writer,
and a simple valid encoder per block format.

The restatements follow diffusion_rs_common/src/core/quantized/k_quants.rs loop for loop — Q4_0 :175, Q4_1 :341, Q5_0 :440, Q5_1 :547, Q8_0 :580,
Q4_K :1568, Q5_K :1872, Q6_K :2147, block structs :56-158, get_scale_min_k4 utils.rs:49 — in np.float32 arithmetic with ONE operation per statement,
so every multiply and every add / subtract is rounded on its own as in Rust (which never contracts).  The loops over a block's elements are the
reference's; the blocks of a tensor are the array axis (every statement is element-wise over them, which changes no rounding).
"""
import struct

import numpy as np

Q4_0, Q4_1, Q5_0, Q5_1, Q8_0, Q4_K, Q5_K, Q6_K = 2, 3, 6, 7, 8, 12, 13, 14
F32, F16, BF16 = 0, 1, 30
TYPES = (Q4_0, Q4_1, Q5_0, Q5_1, Q8_0, Q4_K, Q5_K, Q6_K)
NAMES = {Q4_0: "Q4_0", Q4_1: "Q4_1", Q5_0: "Q5_0", Q5_1: "Q5_1", Q8_0: "Q8_0", Q4_K: "Q4_K", Q5_K: "Q5_K", Q6_K: "Q6_K"}
BLOCK = {Q4_0: (32, 18), Q4_1: (32, 20), Q5_0: (32, 22), Q5_1: (32, 24), Q8_0: (32, 34), Q4_K: (256, 144), Q5_K: (256, 176), Q6_K: (256, 210)}
# byte offsets of the f16 scale fields of a block (for sanitising random bytes)
F16_FIELDS = {Q4_0: (0,), Q4_1: (0, 2), Q5_0: (0,), Q5_1: (0, 2), Q8_0: (0,), Q4_K: (0, 2), Q5_K: (0, 2), Q6_K: (208,)}

f32 = np.float32


def _f16(b, off):
    """the f16 at byte `off` of every block, as f32 (exact)"""
    return np.ascontiguousarray(b[:, off:off + 2]).view("<f2")[:, 0].astype(f32)


def _scale_min_k4(j, q):
    """utils.rs:49 — q: (nb, 12) uint8"""
    if j < 4:
        d = q[:, j] & 63
        m = q[:, j + 4] & 63
    else:
        d = (q[:, j + 4] & 0xF) | ((q[:, j - 4] >> 6) << 4)
        m = (q[:, j + 4] >> 4) | ((q[:, j] >> 6) << 4)
    return d, m


def dequantize_f32(ggml_type, raw) -> np.ndarray:
    """`raw`: the bytes of nb consecutive blocks -> (nb * block_elems,) float32."""
    be, bb = BLOCK[ggml_type]
    b = np.frombuffer(bytes(raw), np.uint8).reshape(-1, bb)
    nb = b.shape[0]
    y = np.zeros((nb, be), f32)
    if ggml_type == Q4_0:  # k_quants.rs:175
        d = _f16(b, 0)
        qs = b[:, 2:18]
        for j in range(16):
            x0 = (qs[:, j] & 0x0F).astype(np.int16) - 8
            x1 = (qs[:, j] >> 4).astype(np.int16) - 8
            y[:, j] = x0.astype(f32) * d
            y[:, j + 16] = x1.astype(f32) * d
    elif ggml_type == Q4_1:  # :341
        d, m = _f16(b, 0), _f16(b, 2)
        qs = b[:, 4:20]
        for j in range(16):
            x0 = qs[:, j] & 0x0F
            x1 = qs[:, j] >> 4
            t0 = x0.astype(f32) * d
            y[:, j] = t0 + m
            t1 = x1.astype(f32) * d
            y[:, j + 16] = t1 + m
    elif ggml_type in (Q5_0, Q5_1):  # :440 / :547
        d = _f16(b, 0)
        o = 2
        if ggml_type == Q5_1:
            m = _f16(b, 2)
            o = 4
        qh = np.ascontiguousarray(b[:, o:o + 4]).view("<u4")[:, 0]
        qs = b[:, o + 4:o + 20]
        for j in range(16):
            xh_0 = (((qh >> np.uint32(j)) << np.uint32(4)) & np.uint32(0x10)).astype(np.uint8)
            xh_1 = ((qh >> np.uint32(j + 12)) & np.uint32(0x10)).astype(np.uint8)
            if ggml_type == Q5_0:
                x0 = ((qs[:, j] & 0x0F) | xh_0).astype(np.int32) - 16
                x1 = ((qs[:, j] >> 4) | xh_1).astype(np.int32) - 16
                y[:, j] = x0.astype(f32) * d
                y[:, j + 16] = x1.astype(f32) * d
            else:
                x0 = (qs[:, j] & 0x0F) | xh_0
                x1 = (qs[:, j] >> 4) | xh_1
                t0 = x0.astype(f32) * d
                y[:, j] = t0 + m
                t1 = x1.astype(f32) * d
                y[:, j + 16] = t1 + m
    elif ggml_type == Q8_0:  # :580
        d = _f16(b, 0)
        qs = b[:, 2:34].view(np.int8)
        for j in range(32):
            y[:, j] = qs[:, j].astype(f32) * d
    elif ggml_type in (Q4_K, Q5_K):  # :1568 / :1872
        d, dmin = _f16(b, 0), _f16(b, 2)
        scales = b[:, 4:16]
        if ggml_type == Q4_K:
            q = b[:, 16:144]
        else:
            qh = b[:, 16:48]
            q = b[:, 48:176]
        is_, u1, u2, ys = 0, 1, 2, 0
        for j in range(0, 256, 64):
            ql = q[:, j // 2:j // 2 + 32]
            sc, mn = _scale_min_k4(is_, scales)
            d1 = d * sc.astype(f32)
            m1 = dmin * mn.astype(f32)
            sc, mn = _scale_min_k4(is_ + 1, scales)
            d2 = d * sc.astype(f32)
            m2 = dmin * mn.astype(f32)
            for l in range(32):
                v = (ql[:, l] & 0xF).astype(f32)
                if ggml_type == Q5_K:
                    to_add = np.where(qh[:, l] & u1 != 0, f32(16), f32(0))
                    v = v + to_add
                t = d1 * v
                y[:, ys] = t - m1
                ys += 1
            for l in range(32):
                v = (ql[:, l] >> 4).astype(f32)
                if ggml_type == Q5_K:
                    to_add = np.where(qh[:, l] & u2 != 0, f32(16), f32(0))
                    v = v + to_add
                t = d2 * v
                y[:, ys] = t - m2
                ys += 1
            is_ += 2
            u1 <<= 2
            u2 <<= 2
    elif ggml_type == Q6_K:  # :2147
        d = _f16(b, 208)
        for n in range(0, 256, 128):
            idx = n // 128
            sc = b[:, 192 + 8 * idx:].view(np.int8)
            ql = b[:, 64 * idx:]
            qh = b[:, 128 + 32 * idx:]
            for l in range(32):
                is_ = l // 16
                q1 = ((ql[:, l] & 0xF) | ((qh[:, l] & 3) << 4)).astype(np.int8) - np.int8(32)
                q2 = ((ql[:, l + 32] & 0xF) | (((qh[:, l] >> 2) & 3) << 4)).astype(np.int8) - np.int8(32)
                q3 = ((ql[:, l] >> 4) | (((qh[:, l] >> 4) & 3) << 4)).astype(np.int8) - np.int8(32)
                q4 = ((ql[:, l + 32] >> 4) | (((qh[:, l] >> 6) & 3) << 4)).astype(np.int8) - np.int8(32)
                for k, qq in enumerate((q1, q2, q3, q4)):
                    ds = d * sc[:, is_ + 2 * k].astype(f32)
                    y[:, n + l + 32 * k] = ds * qq.astype(f32)
    else:
        raise ValueError(ggml_type)
    assert y.dtype == f32
    return y.reshape(-1)


def bf16_bits(a) -> np.ndarray:
    """f32 -> bf16 bits, round to nearest even (finite inputs)"""
    u = np.ascontiguousarray(a, f32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_values(a) -> np.ndarray:
    """f32 -> the f32 values of its bf16 rounding"""
    return (bf16_bits(a).astype(np.uint32) << 16).view(f32)


def dequantize_bf16_values(ggml_type, raw) -> np.ndarray:
    return bf16_values(dequantize_f32(ggml_type, raw))


def sanitize(ggml_type, raw: np.ndarray) -> np.ndarray:
    """Random block bytes -> the same with every f16 scale field whose exponent is all ones (Inf / NaN) made finite; every other bit stays."""
    be, bb = BLOCK[ggml_type]
    b = np.array(raw, np.uint8).reshape(-1, bb)
    for off in F16_FIELDS[ggml_type]:
        hi = b[:, off + 1]
        bad = (hi & 0x7C) == 0x7C
        hi[bad] &= 0xBF  # clear one exponent bit
    return b.reshape(-1)


# ---------------------------------------------------------------------------------------------------------------- encoders
def _f16_bytes(v):
    return np.ascontiguousarray(np.asarray(v, f32).astype("<f2")).view(np.uint8).reshape(-1, 2)


def _safe_div(a, b):
    return np.where(b != 0, a / np.where(b != 0, b, 1), 0)


def _pack_k4(sc, mn):
    """eight 6-bit (scale, min) pairs -> the 12 bytes get_scale_min_k4 reads"""
    out = np.zeros((sc.shape[0], 12), np.uint8)
    for j in range(4):
        out[:, j] = (sc[:, j] & 63) | ((sc[:, j + 4] >> 4) << 6)
        out[:, j + 4] = (mn[:, j] & 63) | ((mn[:, j + 4] >> 4) << 6)
        out[:, j + 8] = (sc[:, j + 4] & 0xF) | ((mn[:, j + 4] & 0xF) << 4)
    return out


def encode(ggml_type, x) -> np.ndarray:
    """A simple VALID encoder (not ggml's quantiser: any well-formed blocks are a valid file): absmax (symmetric formats) or min / max (the
    formats with an offset) per (sub-)block, the K formats' 6-bit (Q6_K: 8-bit) sub-block scales rounded UP.  x: (n,) -> uint8 bytes."""
    be, bb = BLOCK[ggml_type]
    x = np.asarray(x, np.float64).reshape(-1, be)
    nb = x.shape[0]
    out = np.zeros((nb, bb), np.uint8)
    if ggml_type in (Q4_0, Q5_0, Q8_0):
        qmax, off = {Q4_0: (7, 8), Q5_0: (15, 16), Q8_0: (127, 0)}[ggml_type]
        d = (np.abs(x).max(1) / qmax).astype("<f2").astype(np.float64)
        q = np.clip(np.rint(_safe_div(x, d[:, None])), -qmax, qmax).astype(np.int32) + off
        out[:, 0:2] = _f16_bytes(d)
        if ggml_type == Q8_0:
            out[:, 2:34] = q.astype(np.int8).view(np.uint8)
        else:
            o = 2
            if ggml_type == Q5_0:
                qh = np.zeros(nb, np.uint32)
                for j in range(32):
                    qh |= ((q[:, j] >> 4) & 1).astype(np.uint32) << np.uint32(j)
                out[:, 2:6] = qh.astype("<u4").view(np.uint8).reshape(-1, 4)
                o = 6
            out[:, o:o + 16] = ((q[:, :16] & 0xF) | ((q[:, 16:] & 0xF) << 4)).astype(np.uint8)
    elif ggml_type in (Q4_1, Q5_1):
        qmax = 15 if ggml_type == Q4_1 else 31
        m = x.min(1).astype("<f2").astype(np.float64)
        d = ((x.max(1) - m) / qmax).astype("<f2").astype(np.float64)
        q = np.clip(np.rint(_safe_div(x - m[:, None], d[:, None])), 0, qmax).astype(np.int32)
        out[:, 0:2], out[:, 2:4] = _f16_bytes(d), _f16_bytes(m)
        o = 4
        if ggml_type == Q5_1:
            qh = np.zeros(nb, np.uint32)
            for j in range(32):
                qh |= ((q[:, j] >> 4) & 1).astype(np.uint32) << np.uint32(j)
            out[:, 4:8] = qh.astype("<u4").view(np.uint8).reshape(-1, 4)
            o = 8
        out[:, o:o + 16] = ((q[:, :16] & 0xF) | ((q[:, 16:] & 0xF) << 4)).astype(np.uint8)
    elif ggml_type in (Q4_K, Q5_K):
        qmax = 15 if ggml_type == Q4_K else 31
        xs = x.reshape(nb, 8, 32)
        mins = np.maximum(0, -xs.min(2))  # value = d * sc * q - dmin * m with m >= 0
        scl = (xs.max(2) + mins) / qmax
        d = (scl.max(1) / 63).astype("<f2").astype(np.float64)
        dmin = (mins.max(1) / 63).astype("<f2").astype(np.float64)
        sc = np.clip(np.ceil(_safe_div(scl, d[:, None])), 0, 63).astype(np.uint8)
        mn = np.clip(np.ceil(_safe_div(mins, dmin[:, None])), 0, 63).astype(np.uint8)
        step = d[:, None] * sc
        q = np.clip(np.rint(_safe_div(xs + (dmin[:, None] * mn)[:, :, None], step[:, :, None])), 0, qmax).astype(np.int32)
        out[:, 0:2], out[:, 2:4] = _f16_bytes(d), _f16_bytes(dmin)
        out[:, 4:16] = _pack_k4(sc, mn)
        o = 16
        if ggml_type == Q5_K:
            qh = np.zeros((nb, 32), np.uint8)
            for s in range(8):
                qh |= (((q[:, s, :] >> 4) & 1) << s).astype(np.uint8)
            out[:, 16:48] = qh
            o = 48
        for g in range(4):
            out[:, o + 32 * g:o + 32 * g + 32] = ((q[:, 2 * g, :] & 0xF) | ((q[:, 2 * g + 1, :] & 0xF) << 4)).astype(np.uint8)
    elif ggml_type == Q6_K:
        xs = x.reshape(nb, 16, 16)
        scl = np.abs(xs).max(2) / 31
        d = (scl.max(1) / 127).astype("<f2").astype(np.float64)
        sc = np.clip(np.ceil(_safe_div(scl, d[:, None])), 0, 127).astype(np.int32)
        step = d[:, None] * sc
        q = (np.clip(np.rint(_safe_div(xs, step[:, :, None])), -32, 31).astype(np.int32) + 32).reshape(nb, 256)
        for idx in range(2):
            qq = q[:, 128 * idx:128 * idx + 128].reshape(nb, 4, 32)  # q1 .. q4 of :2147
            out[:, 64 * idx:64 * idx + 32] = ((qq[:, 0] & 0xF) | ((qq[:, 2] & 0xF) << 4)).astype(np.uint8)
            out[:, 64 * idx + 32:64 * idx + 64] = ((qq[:, 1] & 0xF) | ((qq[:, 3] & 0xF) << 4)).astype(np.uint8)
            out[:, 128 + 32 * idx:160 + 32 * idx] = ((qq[:, 0] >> 4) | ((qq[:, 1] >> 4) << 2) | ((qq[:, 2] >> 4) << 4) | ((qq[:, 3] >> 4) << 6)).astype(np.uint8)
        out[:, 192:208] = sc.astype(np.int8).view(np.uint8)
        out[:, 208:210] = _f16_bytes(d)
    else:
        raise ValueError(ggml_type)
    return out.reshape(-1)


def step_bound(ggml_type, x) -> np.ndarray:
    """Per element: what |x - dequant(encode(x))| cannot exceed, derived per format from encode() above (the f16 rounding of a scale moves a value
    by at most 2^-11 relative; 2^-9 * max|x| covers the scale fields, the clipping they cause, and the f32 evaluation):
      symmetric (Q4_0 / Q5_0 / Q8_0): d = absmax / qmax, round to nearest            -> d / 2
      offset (Q4_1 / Q5_1):            d = (max - min) / qmax, m = min                -> d / 2
      Q4_K / Q5_K:  step = d * sc >= sub-block range / qmax (scales rounded up);
                    the stored minimum dmin * m exceeds the true one by < dmin         -> step / 2 + dmin
      Q6_K:         step = d * sc >= sub-block absmax / 31                             -> step / 2"""
    be, bb = BLOCK[ggml_type]
    x = np.asarray(x, np.float64).reshape(-1, be)
    slack = np.abs(x).max(1, keepdims=True) * 2.0 ** -9
    if ggml_type in (Q4_0, Q5_0, Q8_0):
        qmax = {Q4_0: 7, Q5_0: 15, Q8_0: 127}[ggml_type]
        b = np.abs(x).max(1, keepdims=True) / qmax / 2 + 0 * x
    elif ggml_type in (Q4_1, Q5_1):
        qmax = 15 if ggml_type == Q4_1 else 31
        b = (x.max(1, keepdims=True) - x.min(1, keepdims=True)) / qmax / 2 + 0 * x
    elif ggml_type in (Q4_K, Q5_K):
        qmax = 15 if ggml_type == Q4_K else 31
        xs = x.reshape(-1, 8, 32)
        mins = np.maximum(0, -xs.min(2))
        scl = (xs.max(2) + mins) / qmax
        d, dmin = scl.max(1, keepdims=True) / 63, mins.max(1, keepdims=True) / 63
        step = scl + d  # (rounded up by less than one unit of d)
        b = np.repeat(step / 2 + dmin, 32, axis=1)
    else:
        xs = x.reshape(-1, 16, 16)
        scl = np.abs(xs).max(2) / 31
        d = scl.max(1, keepdims=True) / 127
        b = np.repeat((scl + d) / 2, 16, axis=1)
    return (b + slack).reshape(-1)


# ---------------------------------------------------------------------------------------------------------------- writer
def _gguf_string(s: str) -> bytes:
    b = s.encode("utf-8")
    return struct.pack("<Q", len(b)) + b


_KV_FMT = {"u8": (0, "<B"), "i8": (1, "<b"), "u16": (2, "<H"), "i16": (3, "<h"), "u32": (4, "<I"), "i32": (5, "<i"), "f32": (6, "<f"), "bool": (7, "<?"),
           "u64": (10, "<Q"), "i64": (11, "<q"), "f64": (12, "<d")}


def _gguf_value(kind, v) -> bytes:
    """kind: a scalar kind of _KV_FMT, "str", or ("array", element kind)"""
    if kind == "str":
        return struct.pack("<I", 8) + _gguf_string(v)
    if isinstance(kind, tuple):
        ek = kind[1]
        et = 8 if ek == "str" else _KV_FMT[ek][0]
        body = b"".join(_gguf_string(e) if ek == "str" else struct.pack(_KV_FMT[ek][1], e) for e in v)
        return struct.pack("<IIQ", 9, et, len(v)) + body
    t, fmt = _KV_FMT[kind]
    return struct.pack("<I", t) + struct.pack(fmt, v)


def write_gguf(path, tensors, metadata=(), alignment=32, version=3, magic=b"GGUF"):
    """tensors: [(name, ggml_type, shape outer-first, raw bytes)]; metadata: [(key, kind, value)] (see _gguf_value).  A general.alignment key is
    written when alignment != 32.  Returns {name: absolute file offset of its data}."""
    metadata = list(metadata)
    if alignment != 32:
        metadata.append(("general.alignment", "u32", alignment))
    head = magic + struct.pack("<IQQ", version, len(tensors), len(metadata))
    for key, kind, v in metadata:
        head += _gguf_string(key) + _gguf_value(kind, v)
    offs, cur = [], 0
    for name, t, shape, raw in tensors:
        offs.append(cur)
        cur = (cur + len(raw) + alignment - 1) // alignment * alignment
    for (name, t, shape, raw), off in zip(tensors, offs):
        head += _gguf_string(name) + struct.pack("<I", len(shape)) + b"".join(struct.pack("<Q", d) for d in reversed(shape)) + struct.pack("<IQ", t, off)
    data0 = (len(head) + alignment - 1) // alignment * alignment
    where = {}
    with open(path, "wb") as f:
        f.write(head + b"\0" * (data0 - len(head)))
        for (name, t, shape, raw), off in zip(tensors, offs):
            f.seek(data0 + off)
            f.write(bytes(raw))
            where[name] = data0 + off
    return where


# ---------------------------------------------------------------------------------------------------------------- FLUX files
def plain_bytes(a, ggml_type=F16) -> bytes:
    a = np.asarray(a, f32)
    if ggml_type == F32:
        return a.astype("<f4").tobytes()
    if ggml_type == F16:
        return a.astype("<f2").tobytes()
    return bf16_bits(a).astype("<u2").tobytes()


def plain_values(a, ggml_type=F16) -> np.ndarray:
    a = np.asarray(a, f32)
    return a if ggml_type == F32 else a.astype(np.float16).astype(f32) if ggml_type == F16 else bf16_values(a)


def diffusers_to_bfl(sd: dict, cfg: dict) -> dict:
    """A diffusers-named FLUX state dict ({name: array}) under the BFL names (the inverse of diffusers' convert_flux_transformer_checkpoint_to_diffusers),
    written out independently of the product's map: fused qkv / linear1 by concatenation, the final modulation with its halves exchanged."""
    out = {}
    top = {"time_text_embed.timestep_embedder.linear_1": "time_in.in_layer", "time_text_embed.timestep_embedder.linear_2": "time_in.out_layer",
           "time_text_embed.text_embedder.linear_1": "vector_in.in_layer", "time_text_embed.text_embedder.linear_2": "vector_in.out_layer",
           "time_text_embed.guidance_embedder.linear_1": "guidance_in.in_layer", "time_text_embed.guidance_embedder.linear_2": "guidance_in.out_layer",
           "context_embedder": "txt_in", "x_embedder": "img_in", "proj_out": "final_layer.linear"}
    for kind in ("weight", "bias"):
        for dn, bn in top.items():
            if f"{dn}.{kind}" in sd:
                out[f"{bn}.{kind}"] = sd[f"{dn}.{kind}"]
        a = sd[f"norm_out.linear.{kind}"]
        h = a.shape[0] // 2
        out[f"final_layer.adaLN_modulation.1.{kind}"] = np.concatenate([a[h:], a[:h]])
        for i in range(cfg["num_layers"]):
            d, b = f"transformer_blocks.{i}.", f"double_blocks.{i}."
            out[b + f"img_mod.lin.{kind}"] = sd[d + f"norm1.linear.{kind}"]
            out[b + f"txt_mod.lin.{kind}"] = sd[d + f"norm1_context.linear.{kind}"]
            out[b + f"img_attn.qkv.{kind}"] = np.concatenate([sd[d + f"attn.{n}.{kind}"] for n in ("to_q", "to_k", "to_v")])
            out[b + f"txt_attn.qkv.{kind}"] = np.concatenate([sd[d + f"attn.{n}.{kind}"] for n in ("add_q_proj", "add_k_proj", "add_v_proj")])
            out[b + f"img_attn.proj.{kind}"] = sd[d + f"attn.to_out.0.{kind}"]
            out[b + f"txt_attn.proj.{kind}"] = sd[d + f"attn.to_add_out.{kind}"]
            out[b + f"img_mlp.0.{kind}"] = sd[d + f"ff.net.0.proj.{kind}"]
            out[b + f"img_mlp.2.{kind}"] = sd[d + f"ff.net.2.{kind}"]
            out[b + f"txt_mlp.0.{kind}"] = sd[d + f"ff_context.net.0.proj.{kind}"]
            out[b + f"txt_mlp.2.{kind}"] = sd[d + f"ff_context.net.2.{kind}"]
        for i in range(cfg["num_single_layers"]):
            d, b = f"single_transformer_blocks.{i}.", f"single_blocks.{i}."
            out[b + f"modulation.lin.{kind}"] = sd[d + f"norm.linear.{kind}"]
            out[b + f"linear1.{kind}"] = np.concatenate([sd[d + f"{n}.{kind}"] for n in ("attn.to_q", "attn.to_k", "attn.to_v", "proj_mlp")])
            out[b + f"linear2.{kind}"] = sd[d + f"proj_out.{kind}"]
    for i in range(cfg["num_layers"]):
        d, b = f"transformer_blocks.{i}.attn.", f"double_blocks.{i}."
        out[b + "img_attn.norm.query_norm.scale"] = sd[d + "norm_q.weight"]
        out[b + "img_attn.norm.key_norm.scale"] = sd[d + "norm_k.weight"]
        out[b + "txt_attn.norm.query_norm.scale"] = sd[d + "norm_added_q.weight"]
        out[b + "txt_attn.norm.key_norm.scale"] = sd[d + "norm_added_k.weight"]
    for i in range(cfg["num_single_layers"]):
        d, b = f"single_transformer_blocks.{i}.attn.", f"single_blocks.{i}."
        out[b + "norm.query_norm.scale"] = sd[d + "norm_q.weight"]
        out[b + "norm.key_norm.scale"] = sd[d + "norm_k.weight"]
    return out


def quantize_state_dict(sd: dict, type_of):
    """sd: {name: f32 array}; type_of(name, shape) -> ggml type.  Returns ([(name, type, shape, raw bytes)] for write_gguf, {name: f32 array of the
    values the file holds after dequantisation to bf16 — the dense twin's weights})."""
    tensors, values = [], {}
    for name, a in sd.items():
        a = np.asarray(a, f32)
        t = type_of(name, a.shape)
        if t in (F32, F16, BF16):
            tensors.append((name, t, a.shape, plain_bytes(a, t)))
            values[name] = bf16_values(plain_values(a, t))
        else:
            raw = encode(t, a.reshape(-1))
            tensors.append((name, t, a.shape, raw.tobytes()))
            values[name] = dequantize_bf16_values(t, raw).reshape(a.shape)
    return tensors, values
