"""numpy restatement of the DRY / no-repeat-n-gram launch (csrc/q4_dry.hip; the rule is written down in include/llama2_q4.h), twice: `apply`, a direct
version that walks back from every candidate, and `apply_naive`, a deliberately naive one that compares every pair of suffixes of the window. Both
return (processed fp16 logits, sorted list of the touched token ids). `pen` is the float32 table of q4_dry_penalty_table: neither restates powf."""
import numpy as np

F = np.float32
CAP = 64
MAX_WINDOW = 4096
DEFAULT = dict(multiplier=0.0, base=1.75, allowed_length=2, last_n=1024, no_repeat_ngram_size=0)


def finish(v):
    """a finite value clamped to +-65504 and rounded to half (nearest even); an infinity stays; a NaN is the quiet NaN 0x7E00"""
    v = F(v)
    if np.isnan(v):
        return np.array([0x7E00], dtype=np.uint16).view(np.float16)[0]
    if np.isfinite(v):
        v = min(max(v, F(-65504.0)), F(65504.0))
    return np.float16(v)


def is_off(multiplier, last_n, no_repeat_ngram_size):
    return (multiplier == 0 and no_repeat_ngram_size == 0) or last_n == 0


def _rewrite(logits, n, M_t, R, pen, multiplier, allowed_length, no_repeat_ngram_size):
    x = np.array(logits, dtype=np.float16)
    touched = []
    with np.errstate(all="ignore"):
        for t in sorted(M_t):
            M = M_t[t]
            if no_repeat_ngram_size >= 2 and M >= no_repeat_ngram_size - 1:
                x[t] = -np.inf
                touched.append(t)
            elif multiplier > 0:
                L = min(M, R)
                if L >= allowed_length:
                    x[t] = finish(F(F(x[t]) - F(pen[L])))
                    touched.append(t)
    return x, touched


def apply(logits, tokens, pos, pen, multiplier=0.0, base=1.75, allowed_length=2, last_n=1024, no_repeat_ngram_size=0, breakers=()):
    """the direct version: R by walking back from ring[pos]; every window slot in front of the last whose token equals ring[pos] walks back in step
    with the suffix (vectorised over the candidates), at most CAP entries and never below the window's start"""
    n = len(logits)
    if tokens is None or pos is None or pos < 0 or is_off(multiplier, last_n, no_repeat_ngram_size):
        return np.array(logits, dtype=np.float16), []
    start = max(0, pos + 1 - last_n)
    w = np.asarray(tokens[start: pos + 1], dtype=np.int64)
    L = w.shape[0]
    brk = set(int(b) for b in breakers)
    R = 0
    while R < min(CAP, L) and int(w[L - 1 - R]) not in brk:
        R += 1
    cand = np.nonzero(w[: L - 1] == w[L - 1])[0]
    M = np.ones(cand.shape[0], dtype=np.int64)
    alive = np.ones(cand.shape[0], dtype=bool)
    for j in range(1, CAP):
        if L - 1 - j < 0 or not alive.any():
            break
        idx = cand - j
        ok = alive & (idx >= 0)
        ok[ok] = w[idx[ok]] == w[L - 1 - j]
        alive = ok
        M += alive
    M_t = {}
    for k, m in zip(cand.tolist(), M.tolist()):
        t = int(w[k + 1])
        if 0 <= t < n:
            M_t[t] = max(M_t.get(t, 0), m)
    return _rewrite(logits, n, M_t, R, pen, multiplier, allowed_length, no_repeat_ngram_size)


def apply_naive(logits, tokens, pos, pen, multiplier=0.0, base=1.75, allowed_length=2, last_n=1024, no_repeat_ngram_size=0, breakers=()):
    """the naive version: for EVERY index i of the window in front of the last, the whole common suffix of window[:i + 1] and the window, compared
    entry by entry with no cap; the cap, the condition ring[i] == ring[pos] and the per-token maximum come afterwards"""
    n = len(logits)
    if tokens is None or pos is None or pos < 0 or is_off(multiplier, last_n, no_repeat_ngram_size):
        return np.array(logits, dtype=np.float16), []
    w = [int(t) for t in tokens[max(0, pos + 1 - last_n): pos + 1]]
    rev = w[::-1]
    nonbreaker_run = 0
    for t in rev:
        if t in set(int(b) for b in breakers):
            break
        nonbreaker_run += 1
    R = min(nonbreaker_run, CAP)
    M_t = {}
    for i in range(len(w) - 1):
        prefix_rev = w[: i + 1][::-1]
        common = 0
        for a, b in zip(prefix_rev, rev):
            if a != b:
                break
            common += 1
        if common == 0:
            continue
        t = w[i + 1]
        if t < 0 or t >= n:
            continue
        M_t[t] = max(M_t.get(t, 0), min(common, CAP))
    return _rewrite(logits, n, M_t, R, pen, multiplier, allowed_length, no_repeat_ngram_size)
