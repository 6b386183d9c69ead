"""q4_set_pass_13b against the knobs that move the step at dim 5120 off the forms a pass restates (the -DQ4_PROFILING build only): q4_set_half_tail(0)
takes the shared half slot out of q/k/v, o-proj, gate/up and down; q4_set_ksplit(0 | 4) changes the down projection; GEMV form 19 runs the K = 5120
gate/up strips on column units (its bits are the pair units', but the admission takes the product's forms only). With any of them the admission must
refuse and the run must be the steps'. Not collected by the default run (file name); run by tests/test_pass_13b_gpu.py in a subprocess with
Q4_PROFILING_BUILD=1."""
import numpy as np
import pytest

from llama_cu_awq_amd import synth

pytestmark = pytest.mark.gpu

# name: (setter, arguments that select the other form, arguments that put the default back)
KNOBS = {"ksplit 0": ("q4_set_ksplit", (0,), (2,)), "ksplit 4": ("q4_set_ksplit", (4,), (2,)), "half_tail 0": ("q4_set_half_tail", (0,), (1,)),
         "column units": ("q4_set_gemv_early", (11, 19), (11, 0))}


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("pass_13b_prof") / "k5120_one.bin")
    dim, hidden, layers, heads, kv_heads, vocab, seq_len, theta = synth.GEOMETRIES["k5120_pair"]
    synth.write_model(p, (dim, hidden, 1, heads, kv_heads, vocab, 300, theta), seed=11)
    return p


def _run(q4, path, on, ingest):
    L = q4.lib()
    prompt = [1] + [int(x) for x in np.random.default_rng(5).integers(3, 512, size=39)]
    L.q4_set_prompt_ingest(ingest)
    t = q4.Transformer(path, pass_13b=on, speculative=dict(draft=4, ngram=3, min=1))
    try:
        t.set_drafter(lambda ring, room: [5] * room)
        before = L.q4_prompt_passes()
        toks = t.generate_ids(prompt, 60)[0].copy()
        q4.check(L.q4_handoff_status(t.state))
        kv = np.stack([np.concatenate([np.concatenate(t.kv_row(l, pos)) for l in range(t.config.n_layers)]) for pos in range(t.pos())]).view(np.uint16)
        return {"tokens": toks, "kv": kv.copy(), "logits": t.logits().view(np.uint16).copy(), "passes": L.q4_prompt_passes() - before,
                "stats": t.spec_stats(), "covers": [int(L.q4_verify_covers(t.h, p, 4)) for p in (0, 40, 100)]}
    finally:
        t.close()
        L.q4_set_prompt_ingest(8)


@pytest.mark.parametrize("knob", sorted(KNOBS))
def test_step_form_knobs_keep_the_steps(q4, model, knob):
    L = q4.lib()
    fn, value, default = KNOBS[knob]
    admitted = _run(q4, model, True, 8)
    assert admitted["passes"] == 5 and admitted["covers"] == [1, 1, 1] and admitted["stats"][0] > 0     # (the knobs at their defaults: passes run)
    getattr(L, fn)(*value)
    L.q4_reset_graphs()
    try:
        on = _run(q4, model, True, 8)
        off = _run(q4, model, False, 0)
    finally:
        getattr(L, fn)(*default)
        L.q4_reset_graphs()
    assert on["passes"] == 0 and on["stats"] == (0, 0, 0) and on["covers"] == [0, 0, 0], (knob, on["passes"], on["stats"], on["covers"])
    for key in ("tokens", "kv", "logits"):
        assert np.array_equal(on[key], off[key]), "%s: %s differ from the steps'" % (knob, key)
