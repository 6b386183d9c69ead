"""The log-probability reference against the library's own host perplexity, and the argument checks of the record switch that need no GPU."""
import ctypes as C

import numpy as np

import logprobs_ref


def test_reference_reproduces_compute_perplexity():
    """exp(-mean(reference log-probability of the targets)) is what compute_perplexity (perplexity.h:24-51, a float softmax per row) returns."""
    from llama_cu_awq_amd import api
    L = api.lib()
    rng = np.random.default_rng(77)
    for vocab, rows, scale in ((1024, 48, 1.0), (512, 64, 4.0), (37, 9, 0.3)):
        logits = (rng.standard_normal((rows, vocab)) * scale).astype(np.float32)
        targets = rng.integers(0, vocab, rows).astype(np.int32)
        want = np.exp(-np.mean([logprobs_ref.logprobs(logits[i])[targets[i]] for i in range(rows)]))
        work = logits.copy()                                   # (the host function normalises its argument in place)
        got = L.compute_perplexity(targets.ctypes.data, work.ctypes.data, rows, vocab)
        assert abs(got - want) <= 1e-6 * want, (vocab, got, want)


def test_reference_order_and_special_values():
    x = np.array([1.0, 3.0, -np.inf, 3.0, -0.0, 0.0, 1.0], dtype=np.float16)
    ids, lp = logprobs_ref.topk(x, 7)
    assert ids.tolist() == [1, 3, 0, 6, 4, 5, 2]               # logit descending, index ascending; -0 ties with +0; -inf last
    assert lp[-1] == -np.inf and np.isclose(np.exp(lp[:-1]).sum(), 1.0)
    assert logprobs_ref.within([-np.inf, 1.0], [-np.inf, 1.0 + 1e-9], 1e-8) and not logprobs_ref.within([0.0], [-np.inf], 1.0)


def test_argument_checks_without_a_gpu():
    from llama_cu_awq_amd import api
    L = api.lib()
    foreign = C.create_string_buffer(1024)                     # a zeroed Transformer the library never built
    assert L.q4_set_logprobs(None, 0) == 5                     # Q4_ERR_ARG
    assert L.q4_set_logprobs(foreign, api.MAX_TOP_LOGPROBS + 1) == 5
    assert L.q4_set_logprobs(foreign, -2) == 5
    assert L.q4_set_logprobs(foreign, 5) == 5                  # in range, but not the library's model
    assert L.q4_get_logprobs_k(foreign) == -1
    assert L.q4_get_logprobs_k(None) == -1
    assert L.q4_get_logprobs(foreign, 0, 1, None, None, None) == 5
    out = np.zeros(4, dtype=np.float32)
    toks = np.array([1, 2, 3], dtype=np.int32)
    assert L.q4_score_ids(foreign, None, toks.ctypes.data, 2, out.ctypes.data) == 5
