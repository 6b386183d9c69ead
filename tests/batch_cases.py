"""Helpers of tests/test_batch_gpu.py (batched decoding, csrc/q4_batch.hip): the run of a sequence alone that a slot is held to, the raw
rows of a slot's caches, and the batch's side of the comparison. The reference is always q4_generate_ids on a SECOND Transformer of the same checkpoint
file, with the greedy screen off so that its logits row is the full one."""
import ctypes as C

import numpy as np

import cache_poison as cp

GEN = 24                  # generated tokens per slot, about


def prompt(n, seed):
    r = np.random.default_rng(seed)
    return [1] + [int(x) for x in r.integers(3, 512, size=n - 1)]       # BOS first, no EOS (2) inside


class Solo:
    """The run alone: generate_ids(prompt, steps) on `t`, everything a slot is compared with kept on the host. first_row: the first K / V row kept."""

    def __init__(self, q4, t, prompt_tokens, steps, first_row=0):
        toks = t.generate_ids(prompt_tokens, steps)[0].copy()
        assert len(toks) == steps + 1, "the run alone stopped early (an EOS): pick another prompt"
        q4.check(q4.lib().q4_handoff_status(t.state))
        self.prompt, self.steps, self.first_row, self.tokens = list(prompt_tokens), steps, first_row, toks
        self.k, self.v = cp.read_rows(q4, t, first_row, steps - first_row)
        self.logits = t.logits().view(np.uint16).copy()


def slot_rows(q4, batch, slot, first_row, n_rows):
    """(K, V) rows [first_row, first_row + n_rows) of every layer of a slot's caches: uint16 [layers, n_rows, kv_dim] each"""
    L = q4.lib()
    cfg = batch.t.config
    kv_dim = cfg.dim * cfg.n_kv_heads // cfg.n_heads
    assert 0 <= first_row and n_rows >= 0 and first_row + n_rows <= cfg.seq_len
    out = [np.empty((cfg.n_layers, n_rows, kv_dim), dtype=np.uint16) for _ in range(2)]
    q4.check(L.q4_stream_synchronize())
    if n_rows:
        for dst, base in zip(out, batch.cache(slot)):
            for layer in range(cfg.n_layers):
                q4.check(L.q4_memcpy_d2h(dst[layer].ctypes.data, base + (layer * cfg.seq_len + first_row) * kv_dim * 2, dst[layer].nbytes))
    return out[0], out[1]


def poison_slot(q4, batch, slot, pattern):
    """every row of both caches of a slot becomes cache_poison's pattern"""
    L = q4.lib()
    cfg = batch.t.config
    kv_dim = cfg.dim * cfg.n_kv_heads // cfg.n_heads
    block = np.ascontiguousarray(np.tile(cp.pattern_row(pattern, kv_dim), (cfg.n_layers * cfg.seq_len, 1)))
    q4.check(L.q4_stream_synchronize())
    for base in batch.cache(slot):
        q4.check(L.q4_memcpy_h2d(base, block.ctypes.data, block.nbytes))
    q4.check(L.q4_stream_synchronize())


def assert_poison_above(q4, batch, slot, first_row, pattern, what):
    cfg = batch.t.config
    want = cp.pattern_row(pattern, cfg.dim * cfg.n_kv_heads // cfg.n_heads)
    for name, rows in zip(("K", "V"), slot_rows(q4, batch, slot, first_row, cfg.seq_len - first_row)):
        bad = np.argwhere((rows != want).any(axis=2))
        assert bad.size == 0, "%s: %s rows written above row %d: (layer, row) %s" % (what, name, first_row, [(int(a), int(b) + first_row) for a, b in bad[:8]])


def slot_tokens(out, slot, first_pass=0):
    """[(pass - first_pass, token)] of a slot's column of Batch.generate's result, for the passes from first_pass on that generated a token"""
    return [(i - first_pass, int(tok)) for i, tok in enumerate(out[:, slot]) if i >= first_pass and tok >= 0]


def assert_slot_equals(q4, batch, slot, solo, out, start, what, first_pass=0, logits=True):
    """The slot that stood at position `start` when pass `first_pass` of `out` ran and ran every pass since, against the run alone over the same
    positions: every generated token, the K / V rows of every layer from solo.first_row on, the logits of the last position -- bytes."""
    n_pass = out.shape[0] - first_pass
    end = start + n_pass
    assert end == solo.steps, "%s: the slot ran to position %d, the run alone to %d" % (what, end, solo.steps)
    assert batch.pos(slot) == end, "%s: device position %d, expected %d" % (what, batch.pos(slot), end)
    n_prompt = len(solo.prompt)
    got = slot_tokens(out, slot, first_pass)
    want = [(i, int(solo.tokens[start + i + 1])) for i in range(n_pass) if start + i + 1 >= n_prompt]
    assert got == want, "%s: tokens differ: %s vs the run alone %s" % (what, got, want)
    k, v = slot_rows(q4, batch, slot, solo.first_row, end - solo.first_row)
    for name, a, b in (("K", k, solo.k), ("V", v, solo.v)):
        assert a.shape == b.shape
        bad = np.argwhere((a != b).any(axis=2))
        assert bad.size == 0, "%s: %s rows differ, first (layer, position) %s" % (what, name, [(int(x), int(y) + solo.first_row) for x, y in bad[:8]])
    if logits:
        mine = batch.logits(slot).view(np.uint16)
        assert np.array_equal(mine, solo.logits), "%s: final logits differ in %d entries" % (what, int((mine != solo.logits).sum()))


def set_sampler(q4, t, temperature, topp, seed):
    """the Transformer's sampler replaced by a fresh one (q4_sampler_new) of these settings"""
    L = q4.lib()
    q4.check(L.q4_stream_synchronize())
    L.q4_reset_graphs()
    L.q4_sampler_delete(t.sampler)
    t.sampler = L.q4_sampler_new(t.config.vocab_size, C.c_float(temperature), C.c_float(topp), seed)
    assert t.sampler
