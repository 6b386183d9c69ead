"""numpy float64 reference of the log-probability records (csrc/q4_logprobs.hip): lse, log-probabilities and the top-k order over fp16 logits,
and the error bound the fp32 kernel is held to."""
import numpy as np


def lse(logits):
    """m + log(sum exp(l - m)) in float64; -inf entries contribute 0."""
    l = np.asarray(logits).astype(np.float64)
    m = l.max()
    with np.errstate(invalid="ignore"):
        return float(m + np.log(np.exp(l - m).sum()))


def logprobs(logits):
    l = np.asarray(logits).astype(np.float64)
    return l - lse(l)


def topk(logits, k):
    """(ids, logprobs) of the k entries of highest logit, ordered by (logit descending, index ascending)."""
    l = np.asarray(logits).astype(np.float64)
    order = np.lexsort((np.arange(l.shape[0]), -l))[:k]
    return order.astype(np.int32), logprobs(l)[order]


def bound(logits, l=None):
    """|fp32 kernel - float64| for lse (l = None: the maximum itself) or for the log-probability of an entry of logit l:
    2^-24 * (2 |l - m| + 3 ln n + 64) -- one rounding of the difference, expf <= 2 ulp, <= 64 sequential adds plus a tree, logf, the final subtraction."""
    x = np.asarray(logits).astype(np.float64)
    n, m = x.shape[0], x.max()
    d = 0.0 if l is None else np.abs(np.asarray(l, dtype=np.float64) - m)
    return 2.0 ** -24 * (2.0 * d + 3.0 * np.log(n) + 64.0)


def within(got, want, tol):
    """elementwise |got - want| <= tol, where equal infinities (a -inf logit's log-probability) agree"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    same_inf = np.isinf(want) & (got == want)
    with np.errstate(invalid="ignore"):
        return bool(np.all(same_inf | (np.abs(got - want) <= tol)))
