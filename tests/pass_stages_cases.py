"""What tests/test_pass_stages_host.py and tests/test_pass_stages_gpu.py share: the guides of the end-to-end cases and the drafters that are wrong at a
chosen index. Numpy only."""
import numpy as np

from llama_cu_awq_amd import guide

VOCAB = 512


def forced_choices(n_choices, length, vocab=VOCAB, seed=3):
    """n_choices token sequences of `length` tokens that share their first token and nothing behind it (the second tokens are distinct); no EOS, no BOS"""
    r = np.random.default_rng(seed)
    first = int(r.integers(3, vocab))
    seconds = r.choice(np.arange(3, vocab), size=n_choices, replace=False)
    return [[first, int(s)] + [int(x) for x in r.integers(3, vocab, size=length - 2)] for s in seconds]


def letter_pieces(vocab=VOCAB):
    """a synthetic vocabulary: token i >= 3 is the one-byte piece chr(ord('a') + i % 26), so every letter belongs to 19 or 20 tokens"""
    return [b""] * 3 + [bytes([0x61 + i % 26]) for i in range(3, vocab)]


def regex_table(vocab=VOCAB):
    """from_regex over the letter vocabulary: 900 repetitions of one of a-h then one of i-p -- 1800 tokens before the text may end, so no run of the tests
    meets EOS; about 150 live tokens in every state, 1801 states"""
    return guide.from_regex("(?:[a-h][i-p]){900}", letter_pieces(vocab))


def wrong(tok, vocab=VOCAB):
    w = (int(tok) + 1) % vocab
    return w + 1 if w == 2 else w


class FirstWrong:
    """A drafter over the run's own continuation R that is wrong first at index k, k = 0 .. 7 by call (7: everything right at seven drafts). It keeps what
    it handed out, so the counters the run must show can be worked out: every call with a draft is a pass, and a pass accepts min(k, drafts)."""

    def __init__(self, R):
        self.R = [int(x) for x in R]
        self.calls = 0
        self.passes = self.drafted = self.accepted = 0
        self.seen = set()

    def __call__(self, ring, room):
        k = self.calls % 8
        self.calls += 1
        d = self.R[len(ring):len(ring) + room]
        if not d:
            return d
        if k < len(d):
            d[k] = wrong(d[k])
        self.passes += 1
        self.drafted += len(d)
        self.accepted += min(k, len(d))
        self.seen.add(min(k, len(d)))
        return d

    def stats(self):
        return self.passes, self.drafted, self.accepted
