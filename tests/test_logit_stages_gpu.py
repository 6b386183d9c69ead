"""The four logit stages of a generating step together (csrc/q4_step.hip's stage table: the guide's mask, DRY, the sampling controls, the adaptive
truncation) with log-probability records behind them: the captured graphs against eager mode, bit for bit, and again after the Sampler -- which owns
three of the four parameter blocks the graphs hold by address -- has been deleted and replaced."""
import ctypes as C

import numpy as np
import pytest

from llama_cu_awq_amd import synth

pytestmark = pytest.mark.gpu

PROMPT = [1, 5, 9]
STEPS = 20                       # positions 0, 1 feed the prompt; 2 .. 17 go out as two eight-step replays, 18 and 19 one by one
SEED = 4242
V = 1024                         # synth model `small`


class SamplerStruct(C.Structure):
    """Sampler of include/llama2_q4.h: the test puts rng_state back so that two runs of one Sampler draw the same coins"""
    _fields_ = [("vocab_size", C.c_int), ("indices", C.c_void_p), ("tempStorage_scan", C.c_void_p), ("tempStorage_sort", C.c_void_p),
                ("temp_storage_bytes_scan", C.c_size_t), ("temp_storage_bytes_sort", C.c_size_t), ("temperature", C.c_float), ("topp", C.c_float),
                ("rng_state", C.c_ulonglong)]


@pytest.fixture(scope="module")
def path(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("stages") / "small.bin")
    synth.write_model(p, "small", seed=7)
    return p


def _guide(q4, dead_step):
    """one state; every dead_step-th token is dead, and so is EOS (2): a run never stops early"""
    table = np.zeros((1, V), dtype=np.uint16)
    table[0, 1::dead_step] = q4.GUIDE_DEAD
    table[0, 2] = q4.GUIDE_DEAD
    return q4.Guide(table)


ROUNDS = [
    dict(dead_step=2, dry=dict(multiplier=0.8, base=1.75, allowed_length=1, last_n=64), sampling=dict(top_k=40, repeat_penalty=1.1, penalty_last_n=32),
         bias={4: 1.5, 10: -2.0}, adaptive=dict(typical_p=0.95, top_n_sigma=3.0, mirostat_tau=4.0, mirostat_eta=0.2)),
    dict(dead_step=3, dry=dict(multiplier=1.5, base=1.2, allowed_length=2, last_n=16, no_repeat_ngram_size=3), sampling=dict(top_k=17, min_p=0.02),
         bias={6: -1.0}, adaptive=dict(typical_p=0.8, top_n_sigma=2.0, mirostat_tau=3.0, mirostat_eta=0.5)),
]


def _generate(q4, t, mode):
    L = q4.lib()
    C.cast(t.sampler, C.POINTER(SamplerStruct)).contents.rng_state = SEED
    L.q4_set_use_graphs(mode)
    try:
        toks = t.generate_ids(PROMPT, STEPS)[0].copy()
    finally:
        L.q4_set_use_graphs(1)
    assert len(toks) == STEPS + 1
    tok_lp, ids, top = t.logprobs(0, STEPS)
    return toks, tok_lp.copy(), ids.copy(), top.copy(), t.adaptive_records(0, STEPS).copy()


def _set_all(q4, t, r):
    g = _guide(q4, r["dead_step"])
    t.set_guide(g)
    t.set_dry(**r["dry"])
    t.set_sampling(**r["sampling"])
    t.set_logit_bias(r["bias"])
    t.set_adaptive(**r["adaptive"])
    return g


def test_graphs_equal_eager_with_every_stage_on_and_after_a_new_sampler(q4, path):
    L = q4.lib()
    t = q4.Transformer(path, temperature=0.5, topp=0.9, seed=SEED, logprobs=2)
    assert t.config.vocab_size == V
    guides, runs, captured = [], [], []
    try:
        t.generate_ids(PROMPT, len(PROMPT) - 1)                  # the prompt steps' graph has no stage in it and outlives a Sampler: captured up front
        for i, r in enumerate(ROUNDS):
            if i:                                                # a new Sampler: the allocator may hand back the addresses of the old one's blocks
                L.q4_sampler_delete(t.sampler)
                t.sampler = L.q4_sampler_new(V, 0.5, 0.9, SEED)
                assert t.sampler
                t.set_guide(None)
                guides[-1].close()
            guides.append(_set_all(q4, t, r))
            c0 = L.q4_graph_captures()
            graphs = _generate(q4, t, 1)
            captured.append(L.q4_graph_captures() - c0)
            eager = _generate(q4, t, 2)
            assert L.q4_graph_captures() - c0 == captured[-1], "eager mode captured a graph"
            for name, a, b in zip(("tokens", "token_logprob", "top_ids", "top_logprobs", "adaptive records"), graphs, eager):
                assert a.tobytes() == b.tobytes(), "round %d: %s differ between the graphs and eager mode" % (i, name)
            toks, tok_lp, ids, top, recs = graphs
            gen = len(PROMPT) - 1
            assert not np.isnan(tok_lp[gen:]).any() and not np.isnan(recs[gen:, :5]).any(), "a generating step left no record"
            assert (toks[len(PROMPT):] % r["dead_step"] != 1).all() and (toks[len(PROMPT):] != 2).all(), "a token the guide forbids"
            assert (recs[gen:, 5].copy().view(np.int32) <= r["sampling"]["top_k"]).all(), "the adaptive truncation saw more than top-k left"
            runs.append(toks)
        # the eight-step and the one-step generating variants, both rounds: the new Sampler's graphs are new captures, nothing else is
        assert captured == [2, 2], captured
        assert not np.array_equal(runs[0], runs[1]), "the second round's values changed nothing"
    finally:
        t.close()
        for g in guides[-1:]:
            g.close()
