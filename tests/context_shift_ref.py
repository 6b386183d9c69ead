"""Context shift (csrc/q4_kv_shift.hip, q4_shift_context) restated in numpy: the rows of positions [keep + D, n_pos) move down by D, and every moved
K row is rotated by -D positions. Elementwise float32 numpy and astype(float16) reproduce the kernel bit for bit: every product, sum and difference
is one IEEE fp32 operation, and the rounding to half is round-to-nearest-even.

A K row of one (position, kv head) holds its pairs as (i, i + head_size/2). With (c, s) the rotation of D positions at pair index i:
    k'[i]               = half((a * c) + (b * s))
    k'[i + head_size/2] = half((b * c) - (a * s))
An FP8 row is dequantised first (byte * 2^e: exactly fp16) and its rotated halves are quantised again by the format's rule (kv8_ref)."""
import numpy as np

import kv8_ref


def rope_table_row(pos, head_size, theta):
    """(cos, sin) [head_size/2, 2] float32 of position `pos` by the reference's formula (RoPERotation_kernel), in float32 numpy. The model's own table
    (q4_get_rope_row) comes from the device's powf / cosf / sinf and may differ from this in the last bit; tests that compare bits use the model's."""
    i = np.arange(head_size // 2)
    head_dim = ((i * 2) % head_size).astype(np.float32)
    freq = np.float32(1.0) / np.power(np.float32(theta), head_dim / np.float32(head_size), dtype=np.float32)
    val = (np.float32(pos) * freq).astype(np.float32)
    return np.stack([np.cos(val, dtype=np.float32), np.sin(val, dtype=np.float32)], axis=1)


def rotate(k, head_size, cos_sin):
    """fp16 [..., n * head_size] -> the rows rotated by minus the positions cos_sin ([head_size/2, 2] float32) stands for"""
    k = np.asarray(k, dtype=np.float16)
    hp = head_size // 2
    rows = k.reshape(-1, head_size).astype(np.float32)
    c, s = np.asarray(cos_sin, dtype=np.float32)[:, 0], np.asarray(cos_sin, dtype=np.float32)[:, 1]
    a, b = rows[:, :hp], rows[:, hp:]
    with np.errstate(over="ignore"):
        lo = ((a * c).astype(np.float32) + (b * s).astype(np.float32)).astype(np.float32).astype(np.float16)
        hi = ((b * c).astype(np.float32) - (a * s).astype(np.float32)).astype(np.float32).astype(np.float16)
    return np.concatenate([lo, hi], axis=1).reshape(k.shape)


def rotate_fp8(kb, ke, head_size, cos_sin):
    """(bytes uint8 [..., n * head_size], exponents int8 [..., n]) -> the same of the rotated rows"""
    halves = kv8_ref.dequantise(kb, ke, head_size)
    return kv8_ref.quantise(rotate(halves, head_size, cos_sin), head_size)


def shift_fp16(k, v, n_pos, keep, D, head_size, cos_sin):
    """k, v: [layers, seq_len, kv_dim] float16, changed IN PLACE: rows [keep, n_pos - D). Rows [n_pos - D, n_pos) are unspecified afterwards (left alone
    here)."""
    M = n_pos - keep - D
    if M <= 0:
        return
    k[:, keep:keep + M] = rotate(k[:, keep + D:n_pos].copy(), head_size, cos_sin)
    v[:, keep:keep + M] = v[:, keep + D:n_pos].copy()


def shift_fp8(k, v, k_exp, v_exp, n_pos, keep, D, head_size, cos_sin):
    """k, v: [layers, seq_len, kv_dim] uint8; k_exp, v_exp: [layers, n_kv_heads, seq_len] int8 (the model's layouts), changed IN PLACE"""
    M = n_pos - keep - D
    if M <= 0:
        return
    ke = np.ascontiguousarray(k_exp[:, :, keep + D:n_pos].transpose(0, 2, 1))           # [layers, M, heads]: the order of the rows' heads
    nb, ne = rotate_fp8(k[:, keep + D:n_pos].copy(), ke, head_size, cos_sin)
    k[:, keep:keep + M] = nb
    k_exp[:, :, keep:keep + M] = ne.transpose(0, 2, 1)
    v[:, keep:keep + M] = v[:, keep + D:n_pos].copy()
    v_exp[:, :, keep:keep + M] = v_exp[:, :, keep + D:n_pos].copy()


def tolerance(pair_hypot):
    """|shift(rope(k, p), D) - rope(k, p - D)| per element: three roundings to half (the stored row, the shifted row, the directly rotated row), each
    at most 2^-11 relative to the pair's norm -- a rotation preserves it -- or 2^-25 absolute in the subnormal range"""
    return 3.0 * 2.0 ** -11 * pair_hypot + 3.0 * 2.0 ** -25
