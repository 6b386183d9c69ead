"""Reference for the FP8 (OCP e4m3fn) K / V cache (csrc/attention_kv8.h): the numpy quantiser of the format, and a forward pass
composed from the oracle's per-op functions that can round-trip every K / V row before it enters the cache.

The format: a row of one (position, kv head) is head_size e4m3 bytes plus one signed exponent e, the smallest integer in [-15, 7]
with amax <= 448 * 2^e; element x is stored as e4m3_rne(clamp(float(x) * 2^-e, +-448)). Every byte * 2^e is exactly an fp16 number,
so the mode is "fp16 attention over a cache whose rows were replaced by their round trip"."""
import numpy as np
import torch

import hostile_models
import oracle

E_MIN, E_MAX = -15, 7


def quantise(x, head_size):
    """fp16 [..., n * head_size] -> (e4m3 bytes uint8 of the same shape, exponents int8 [..., n])."""
    x = np.asarray(x, dtype=np.float16)
    rows = x.reshape(-1, head_size).astype(np.float32)
    amax = np.abs(rows).max(axis=1)
    e = np.full(rows.shape[0], E_MIN, dtype=np.int32)
    for k in range(E_MIN, E_MAX):                       # exact comparisons: the smallest e with amax <= 448 * 2^e, capped at 7
        e = np.where(amax > np.float32(448.0 * 2.0 ** k), k + 1, e)
    scaled = rows * (np.float32(2.0) ** (-e)).astype(np.float32)[:, None]      # a power of two: exact in fp32
    scaled = np.clip(scaled, -448.0, 448.0).astype(np.float32)                 # torch yields NaN above the range; rows with amax > 57344 saturate
    b = torch.from_numpy(np.ascontiguousarray(scaled)).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    return b.reshape(x.shape), e.astype(np.int8).reshape(x.shape[:-1] + (x.shape[-1] // head_size,))


def dequantise_f64(b, e, head_size):
    b = np.ascontiguousarray(b, dtype=np.uint8)
    v = torch.from_numpy(b.reshape(-1, head_size)).view(torch.float8_e4m3fn).to(torch.float32).numpy().astype(np.float64)
    return (v * (2.0 ** np.asarray(e, dtype=np.float64).reshape(-1))[:, None]).reshape(b.shape)


def dequantise(b, e, head_size):
    return dequantise_f64(b, e, head_size).astype(np.float16)


def round_trip(x, head_size):
    return dequantise(*quantise(x, head_size), head_size)


def step(a, head_size):
    """the spacing of the row's FP8 grid at each element of the round-tripped fp16 array a [..., n * head_size]: 2^e times e4m3's spacing at the scaled
    magnitude (2^(floor(log2 m) - 3) from 2^-6 on, 2^-9 below)"""
    _, e = quantise(a, head_size)
    scale = np.repeat(2.0 ** e.astype(np.float64), head_size, axis=-1)
    m = np.abs(np.asarray(a, dtype=np.float64)) / scale
    with np.errstate(divide="ignore"):
        ex = np.where(m >= 2.0 ** -6, np.floor(np.log2(np.maximum(m, 2.0 ** -6))), -6.0)
    return scale * 2.0 ** (ex - 3.0)


class Forward:
    """run_llama_network composed from the oracle's per-op functions over a checkpoint file; round_trip=True replaces each K / V row by
    its FP8 round trip before the row enters the cache. With round_trip=False it equals oracle.Model.forward bit for bit."""

    def __init__(self, path, cfg, round_trip=False):
        self.cfg = cfg
        self.rt = round_trip
        t = hostile_models.Tensors(path, cfg, mode="r")
        dim, hidden, layers, heads, kv_heads, vocab, seq_len, theta = cfg
        self.kv_dim = dim * kv_heads // heads
        self.emb, self.wcls, self.rms_final = np.array(t.emb), np.array(t.wcls).reshape(-1), np.array(t.rms_final)
        self.layers = []
        for l in range(layers):
            lay = {m: tuple(np.ascontiguousarray(a) for a in t.qweight(l, m)[:3]) for m in hostile_models.MATS}   # (file order: up before gate; by name here)
            lay["rms_att"], lay["rms_ffn"] = np.array(t.rms(l, "rms_att")), np.array(t.rms(l, "rms_ffn"))
            self.layers.append(lay)
        self.kc = np.zeros((layers, seq_len, self.kv_dim), dtype=np.float16)
        self.vc = np.zeros((layers, seq_len, self.kv_dim), dtype=np.float16)

    def forward(self, token, pos, rows=None):
        """rows: (K [layers, kv_dim], V [layers, kv_dim]) fp16 that enter the cache at `pos` in place of the rows computed here -- the step from another
        evaluation's cache (a row that rounds to the other FP8 neighbour there is then no part of the difference). self.own then holds the rows
        computed here at this position, (K, V) [layers, kv_dim], for the caller to compare."""
        dim, hidden, layers, heads, kv_heads, vocab, seq_len, theta = self.cfg
        hs, kv_dim, orc = dim // heads, self.kv_dim, oracle
        x = np.array(self.emb[token], dtype=np.float16)
        self.own = (np.zeros((layers, kv_dim), dtype=np.float16), np.zeros((layers, kv_dim), dtype=np.float16))
        for l, L in enumerate(self.layers):
            xb = orc.rmsnorm(x, L["rms_att"])
            q = orc.matmul_q4(xb, *L["q"], dim, dim)
            k = orc.matmul_q4(xb, *L["k"], dim, kv_dim)
            v = orc.matmul_q4(xb, *L["v"], dim, kv_dim)
            q, k = orc.rope(q, k, heads, kv_heads, hs, pos, theta)
            if self.rt:
                k, v = round_trip(k, hs), round_trip(v, hs)
            self.own[0][l], self.own[1][l] = k, v
            if rows is not None:
                k, v = rows[0][l], rows[1][l]
            self.kc[l, pos], self.vc[l, pos] = k, v
            xb, _ = orc.attention(q, self.kc[l].reshape(-1), self.vc[l].reshape(-1), heads, hs, heads // kv_heads, pos,
                                  max_seq_len=orc.lib().orc_seq_len_bin(pos, seq_len))
            x = orc.matmul_q4(xb, *L["o"], dim, dim, accum_into=x)
            xb = orc.rmsnorm(x, L["rms_ffn"])
            hb = orc.ffn_matvec_silu(xb, L["gate"], L["up"], dim, hidden)
            x = orc.matmul_q4(hb, *L["down"], hidden, dim, accum_into=x)
        x = orc.rmsnorm(x, self.rms_final)
        return orc.matmul_f16(x, self.wcls, dim, vocab)
