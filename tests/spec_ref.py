"""Python restatements for speculative greedy decoding (csrc/spec_verify.h): the built-in prompt-lookup drafter, the greedy token of a row
of fp16 logits, and what the token loop does with a drafter -- replayed over a finished greedy run, which is what the loop must reproduce."""
import numpy as np

MAX_DRAFT = 7


def draft(tokens, max_draft, ngram_max, ngram_min):
    """q4_spec_draft: for g = ngram_max .. ngram_min, the most recent earlier occurrence of the last g tokens and what followed it"""
    tokens = [int(x) for x in tokens]
    n = len(tokens)
    if n < 2 or max_draft < 1 or ngram_min < 1 or ngram_max < ngram_min:
        return []
    for g in range(min(ngram_max, n - 1), ngram_min - 1, -1):
        tail = tokens[n - g:]
        for j in range(n - g - 1, -1, -1):
            if tokens[j:j + g] == tail:
                return tokens[j + g:j + g + max_draft]          # (a slice stops at the ring's end)
    return []


def greedy_token(row):
    """q4_argmax's rule on a row of float16: the largest value that is neither NaN nor -inf, ties to the lowest index; no such value: 0"""
    v = np.asarray(row, dtype=np.float16).astype(np.float32)
    ok = ~np.isnan(v) & (v > -np.inf)
    if not ok.any():
        return 0
    return int(np.flatnonzero(ok & (v == v[ok].max()))[0])


def accept(rows, drafts):
    """(winners, m): each row's greedy token, and the number of leading drafts that equal the token of the row in front of them"""
    win = [greedy_token(r) for r in rows]
    m = 0
    while m < len(drafts) and win[m] == int(drafts[m]):
        m += 1
    return win, m


def replay(run, n_prompt, steps, drafter, max_draft, group, limit=256):
    """The token loop's passes over `run`, the ring of a finished greedy generation to `steps` (no EOS inside): at every generating position pos the
    drafter sees run[:pos + 1] and may draft up to min(max_draft, steps - 1 - pos, limit - 1 - pos) tokens; a draft makes a pass that accepts its leading
    tokens equal to the run's and moves on by accepted + 1; no draft: the loop's group of steps, then the question again. Returns (passes, drafted, accepted)
    and the (pos, n_draft, accepted) of every pass. group(pos) -> the steps the loop queues at pos without a draft (q4_steps_that_fit)."""
    run = [int(x) for x in run]
    passes = []
    pos = n_prompt - 1
    while pos < steps:
        room = min(max_draft, steps - 1 - pos, limit - 1 - pos)
        d = [int(x) for x in drafter(np.asarray(run[:pos + 1], dtype=np.int32), room)][:room] if room >= 1 else []
        if d:
            m = 0
            while m < len(d) and d[m] == run[pos + 1 + m]:
                m += 1
            passes.append((pos, len(d), m))
            pos += m + 1
        else:
            pos += group(pos)
    return (len(passes), sum(p[1] for p in passes), sum(p[2] for p in passes)), passes

