"""numpy restatement of RoPE scaling (include/llama2_q4.h, q4_set_rope_scaling): the per-pair frequencies in float64 rounded once to float32, the rotation
table as float64 (cos, sin) of the fp32 product, and the rotation itself with the device's rounding points. Written from the definition, not from the
library's code; nothing here calls the library."""
import math

import numpy as np


def base_freq64(head_size, theta):
    """f_i = pow((double)(float)theta, -(2 i) / head_size), float64"""
    i = np.arange(head_size // 2, dtype=np.float64)
    return np.power(np.float64(np.float32(theta)), -(2.0 * i) / head_size)


def inv_freq64(scaling, head_size, theta):
    """The definition, in float64. scaling: None, or a dict in Hugging Face's spelling (rope_type or type = linear / llama3; factor, low_freq_factor,
    high_freq_factor, original_max_position_embeddings), or dict(kind="custom", inv_freq=...)."""
    f = base_freq64(head_size, theta)
    if scaling is None:
        return f
    kind = scaling.get("kind", scaling.get("rope_type", scaling.get("type")))
    if kind == "custom":
        return np.asarray(scaling["inv_freq"], dtype=np.float32).astype(np.float64)
    factor = float(np.float32(scaling["factor"]))
    if kind == "linear":
        return f / factor
    assert kind == "llama3", kind
    low, high = float(np.float32(scaling["low_freq_factor"])), float(np.float32(scaling["high_freq_factor"]))
    orig = float(scaling["original_max_position_embeddings"])
    out = np.empty_like(f)
    for i, fi in enumerate(f):                       # Hugging Face's _compute_llama3_parameters, pair by pair
        wl = 2.0 * math.pi / fi
        if wl < orig / high:
            out[i] = fi
        elif wl > orig / low:
            out[i] = fi / factor
        else:
            s = (orig / wl - low) / (high - low)
            out[i] = (1.0 - s) * fi / factor + s * fi
    return out


def inv_freq32(scaling, head_size, theta):
    return inv_freq64(scaling, head_size, theta).astype(np.float32)


def llama3_bands(scaling, head_size, theta):
    """(high, middle, low): the pair indices that keep their frequency, that are interpolated, and that are divided by the factor"""
    f = base_freq64(head_size, theta)
    wl = 2.0 * math.pi / f
    orig = float(scaling["original_max_position_embeddings"])
    high = wl < orig / float(scaling["high_freq_factor"])
    low = ~high & (wl > orig / float(scaling["low_freq_factor"]))
    return np.nonzero(high)[0], np.nonzero(~high & ~low)[0], np.nonzero(low)[0]


def angles32(freq32, positions):
    """(float)pos * inv_freq[i]: one fp32 multiply; [len(positions), head_size/2] float32"""
    pos = np.asarray(positions, dtype=np.int64).astype(np.float32)
    return (pos[:, None] * np.asarray(freq32, dtype=np.float32)[None, :]).astype(np.float32)


def table64(freq32, positions):
    """what cosf / sinf approximate: float64 (cos, sin) of the fp32 product, [len(positions), head_size/2, 2]"""
    a = angles32(freq32, positions).astype(np.float64)
    return np.stack([np.cos(a), np.sin(a)], axis=-1)


def ulp_diff32(a, b):
    """distance in fp32 ulps between two float32 arrays of finite, non-negative values"""
    a = np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.abs(a - b)


def rotate(q, k, num_heads, num_kv_heads, head_size, pos, freq32):
    """The rotation of position pos on q [num_heads * head_size] and the position's key row k [num_kv_heads * head_size] (float16), pairs
    (i, i + head_size/2): x0' = half(x0 * c - x1 * s), x1' = half(x0 * s + x1 * c), every operation one fp32 operation; (c, s) = float32 of the float64
    (cos, sin) of the fp32 angle (a correctly rounded cosf / sinf)."""
    hp = head_size // 2
    cs = table64(freq32, [pos])[0].astype(np.float32)
    c, s = cs[:, 0], cs[:, 1]

    def rot(x, heads):
        x = np.asarray(x, dtype=np.float16).astype(np.float32).reshape(heads, head_size)
        x0, x1 = x[:, :hp], x[:, hp:]
        a = (x0 * c).astype(np.float32) - (x1 * s).astype(np.float32)
        b = (x0 * s).astype(np.float32) + (x1 * c).astype(np.float32)
        return np.concatenate([a, b], axis=1).astype(np.float16).reshape(-1)
    return rot(q, num_heads), rot(k, num_kv_heads)
