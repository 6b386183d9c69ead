"""The guide launch (csrc/q4_guide.hip) restated in numpy, on uint16 views: what the launch leaves untouched is compared by its bits."""
import numpy as np

DEAD, NONE, OFFTRACK = 0xFFFF, -1, -2
NEG_INF = 0xFC00


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint16) if a.dtype == np.float16 else a.astype(np.uint16, copy=False)


def advance(table, state_ring, tokens, p):
    """steps 1 and 2: the state of position p, from state_ring[p - 1] and the ring entry tokens[p]"""
    S, V = table.shape
    prev = int(state_ring[p - 1]) if p > 0 else NONE
    if prev == NONE:
        return 0
    if prev == OFFTRACK or not 0 <= prev < S:
        return OFFTRACK
    t = int(tokens[p])
    if not 0 <= t < V or int(table[prev, t]) == DEAD:
        return OFFTRACK
    return int(table[prev, t])


def mask(logits, table, state_ring, tokens, p, seq_len=None):
    """steps 1 - 4 at position p: returns the logits' bits after the launch (a copy, uint16) and the state; writes state_ring[p]. A position outside
    [0, seq_len) (default: the ring's length) does nothing: the state is None"""
    out = bits(logits).copy()
    if not 0 <= p < (len(state_ring) if seq_len is None else seq_len):
        return out, None
    s = advance(table, state_ring, tokens, p)
    state_ring[p] = s
    if s != OFFTRACK:
        out[np.asarray(table[s, :out.shape[0]]) == DEAD] = NEG_INF
    return out, s
