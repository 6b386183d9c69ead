"""Hostile synthetic checkpoints: the ordinary `synth.write_model` file with tensors patched IN PLACE, so that the default writer (bench.py's
models, the committed goldens) stays byte-for-byte what it was. Offsets are computed the way `synth.model_bytes` walks the layout. One trait
per variant, so that a failure points at one cause:

  massive       four fixed channels of every embedding row at +300, -600, +1000, -2000 ("massive activations" that ride the residual
                stream through every layer); rms_att / rms_ffn weights at those channels x 0.01; the final norm weight untouched
  peaked        the scales of the q and k projections x PEAK_SCALE (x 7 sqrt(1024 / dim) above dim 1024; scores of several tens, near-one-hot softmax), and an attention sink at
                position 0: eight SINK channels carry a small shared value in every embedding row and a large one in the BOS row (token 1),
                and the q / k nibbles of those input channels are set to 15 or 0 with one sign per (kv head, head dim) -- the shared part of
                every query then points along the BOS key
  quant_edges   every 8th column: zero points pinned at 0; the next: pinned at 15; the next: q == z in every other group; the scales of
                all other columns log-uniform over [3e-4, 3e-2] (two decades around the default 0.003)
  norm_weights  every rmsnorm weight (attention, FFN, final): magnitudes log-uniform over [1e-3, 8], ~5 % negative, ~2 % exact zeros
  combined      all of the above (quant_edges, peaked, norm_weights, massive, in this order)
"""
import numpy as np

from llama_cu_awq_amd import synth

TRAITS = ["massive", "peaked", "quant_edges", "norm_weights", "combined"]
MASSIVE_VALUES = (300.0, -600.0, 1000.0, -2000.0)
MASSIVE_NORM_FACTOR = 0.01
PEAK_SCALE = 7.0                # q / k scale factor up to dim 1024; wider models x 7 sqrt(1024 / dim), the same score spread (random-weight scores grow with dim)
SINK_SHARED, SINK_BOS = 0.3, 2.5
QE_SCALE_LO, QE_SCALE_HI = 3e-4, 3e-2
NW_LO, NW_HI = 1e-3, 8.0
MATS = ("q", "k", "v", "o", "up", "gate", "down")


def massive_channels(dim):
    return [dim // 8 + 1, 3 * dim // 8 + 3, 5 * dim // 8 + 5, 7 * dim // 8 + 7]


def sink_channels(dim):
    return list(range(dim // 4 + 2, dim // 4 + 18, 2))


def layout(cfg):
    """Byte offsets of every tensor, in the order synth.write_model writes them: {"emb": (off, shape), "wcls", "rms_final",
    "layers": [{mat: (w_off, z_off, s_off, height, width), "rms_att": off, "rms_ffn": off}]}."""
    dim, hidden, layers, heads, kv_heads, vocab, _, _ = cfg
    kv_dim = dim * kv_heads // heads
    off = 32
    out = {"emb": off}
    off += vocab * dim * 2
    out["wcls"] = off
    off += vocab * dim * 2
    out["rms_final"] = off
    off += dim * 2
    out["layers"] = []
    shapes = dict(zip(MATS, ((dim, dim), (dim, kv_dim), (dim, kv_dim), (dim, dim), (dim, hidden), (dim, hidden), (hidden, dim))))
    for _ in range(layers):
        lay = {}
        for m in MATS:
            h, w = shapes[m]
            a, b, c = synth.qweight_sizes(h, w)
            lay[m] = (off, off + a * 4, off + a * 4 + b * 4, h, w)
            off += a * 4 + b * 4 + c * 2
        lay["rms_att"] = off
        lay["rms_ffn"] = off + dim * 2
        off += 2 * dim * 2
        out["layers"].append(lay)
    assert off == synth.model_bytes(cfg), (off, synth.model_bytes(cfg))
    return out


class Tensors:
    """Writable (or read-only) views of one checkpoint's tensors over a memmap of the file."""

    def __init__(self, path, cfg, mode="r+"):
        self.cfg = cfg
        self.lay = layout(cfg)
        self.mm = np.memmap(path, dtype=np.uint8, mode=mode)
        dim, vocab = cfg[0], cfg[5]
        self.emb = self._f16(self.lay["emb"], vocab * dim).reshape(vocab, dim)
        self.wcls = self._f16(self.lay["wcls"], vocab * dim).reshape(vocab, dim)
        self.rms_final = self._f16(self.lay["rms_final"], dim)

    def _f16(self, off, n):
        return self.mm[off: off + 2 * n].view(np.float16)

    def rms(self, layer, which):
        return self._f16(self.lay["layers"][layer][which], self.cfg[0])

    def qweight(self, layer, mat):
        """(weight u32 [width, pwh], zeros u32 [width, pzh], scales f16 [width, groups], height, width)."""
        w_off, z_off, s_off, h, w = self.lay["layers"][layer][mat]
        a, b, c = synth.qweight_sizes(h, w)
        return (self.mm[w_off: w_off + 4 * a].view(np.uint32).reshape(w, -1), self.mm[z_off: z_off + 4 * b].view(np.uint32).reshape(w, -1),
                self._f16(s_off, c).reshape(w, -1), h, w)

    def flush(self):
        self.mm.flush()


_SHIFT = (4 * np.arange(8)).astype(np.uint32)


def unpack(words):
    """u32 [..., n] -> nibbles u8 [..., 8 n] (LSB first)."""
    return ((words[..., None] >> _SHIFT) & 0xF).astype(np.uint8).reshape(*words.shape[:-1], -1)


def pack(nibbles):
    n = nibbles.astype(np.uint32).reshape(*nibbles.shape[:-1], -1, 8)
    return np.bitwise_or.reduce(n << _SHIFT, axis=-1).astype(np.uint32)


def _quant_edges(t, rng):
    for layer in range(t.cfg[2]):
        for mat in MATS:
            W, Z, S, h, w = t.qweight(layer, mat)
            groups = S.shape[1]
            z0, z15, qz = np.arange(1, w, 8), np.arange(2, w, 8), np.arange(3, w, 8)
            Z[z0] = 0
            Z[z15] = 0xFFFFFFFF
            zn = unpack(Z[qz])[:, :groups]                                    # [cols, groups]
            nib = unpack(W[qz])                                               # [cols, padded height]
            k = np.arange(h)
            g = k // synth.GROUP_SIZE
            sel = (g % 2) == 0
            nib[:, k[sel]] = zn[:, g[sel]]
            W[qz] = pack(nib)
            other = np.ones(w, dtype=bool)
            other[np.concatenate([z0, z15, qz])] = False
            S[other] = np.exp(rng.uniform(np.log(QE_SCALE_LO), np.log(QE_SCALE_HI), (int(other.sum()), groups))).astype(np.float16)


def _peaked(t, rng):
    dim, _, layers, heads, kv_heads = t.cfg[:5]
    hs, kv_mul = dim // heads, heads // kv_heads
    S_ch = sink_channels(dim)
    peak = PEAK_SCALE * min(1.0, (1024.0 / dim) ** 0.5)
    sign = rng.choice([0, 15], size=(kv_heads, hs)).astype(np.uint8)         # one sign per (kv head, head dim), shared by q and k
    for layer in range(layers):
        for mat in ("q", "k"):
            W, Z, S, h, w = t.qweight(layer, mat)
            S[:] = (S.astype(np.float32) * peak).astype(np.float16)
            n = np.arange(w)
            kvh = (n // hs) // kv_mul if mat == "q" else n // hs
            nib = unpack(W)
            nib[:, S_ch] = sign[kvh, n % hs][:, None]
            W[:] = pack(nib)
    t.emb[:, S_ch] = SINK_SHARED
    t.emb[1, S_ch] = SINK_BOS * max(1.0, dim / 1024.0)                     # (the sink's score ~ peak^2 x this: the same pull at every width)


def _norm_weights(t, rng):
    def draw(n):
        v = np.exp(rng.uniform(np.log(NW_LO), np.log(NW_HI), n))
        v[rng.random(n) < 0.05] *= -1
        v[rng.random(n) < 0.02] = 0.0
        v[[0, n // 2]] = 0.0, -1.0                                           # at least one exact zero and one negative in every vector
        return v.astype(np.float16)
    dim = t.cfg[0]
    for layer in range(t.cfg[2]):
        t.rms(layer, "rms_att")[:] = draw(dim)
        t.rms(layer, "rms_ffn")[:] = draw(dim)
    t.rms_final[:] = draw(dim)


def _massive(t, rng):
    ch = massive_channels(t.cfg[0])
    t.emb[:, ch] = np.array(MASSIVE_VALUES, dtype=np.float16)
    for layer in range(t.cfg[2]):
        for which in ("rms_att", "rms_ffn"):
            r = t.rms(layer, which)
            r[ch] = (r[ch].astype(np.float32) * MASSIVE_NORM_FACTOR).astype(np.float16)


_PATCH = {"quant_edges": _quant_edges, "peaked": _peaked, "norm_weights": _norm_weights, "massive": _massive}


def write_hostile_model(path, geometry, trait, seed):
    """synth.write_model(path, geometry, seed) with `trait` patched in; returns the byte size."""
    assert trait in TRAITS, trait
    size = synth.write_model(path, geometry, seed=seed)
    cfg = synth.geometry(geometry) if isinstance(geometry, str) else geometry
    t = Tensors(path, cfg)
    for i, name in enumerate(("quant_edges", "peaked", "norm_weights", "massive")):
        if trait in (name, "combined"):
            _PATCH[name](t, np.random.default_rng([seed, 7919, i]))
    t.flush()
    del t
    return size
