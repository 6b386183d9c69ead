"""Guided decoding on the device (csrc/q4_guide.hip, q4_set_guide, q4_guide_mask): the launch on crafted logits, tables and rings against the numpy
restatement (tests/guide_ref.py) BIT FOR BIT, and the launch inside the step in every graph form against a ground truth rebuilt from a guide-off
model's raw logits. Synthetic models only."""
import ctypes as C

import numpy as np
import pytest

import guide_ref as ref
import logprobs_ref
from llama_cu_awq_amd import guide, synth

pytestmark = pytest.mark.gpu

ERR_ARG = 5
DEAD, NONE, OFFTRACK = ref.DEAD, ref.NONE, ref.OFFTRACK
SPECIALS = np.array([0x8000, 0x7C00, 0xFC00, 0x7E01, 0xFFFF, 0x7D55, 0x0000, 0xFBFF], dtype=np.uint16)   # -0, +-inf, NaNs with payloads, 0, -65504


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the op against the reference
HIGH = 65536          # a vocabulary beyond 16 bits of token id: every live token and every ring token in range sits at an id >= HIGH


def _row(rng, kind, n, S, lo=0):
    """one row of a table: live entries are random states. lo: no live entry below this id"""
    live = np.zeros(n, dtype=bool)
    if kind == "all":
        live[lo:] = True
    elif kind == "one":
        live[lo + int(rng.integers(n - lo))] = True
    elif kind == "last":
        live[n - 1] = True
    else:
        live[lo:] = rng.random(n - lo) < 0.5
        live[lo + int(rng.integers(n - lo))] = True              # (never empty: q4_guide_new refuses a state nothing leaves)
    row = np.full(n, DEAD, dtype=np.uint16)
    row[live] = rng.integers(0, S, int(live.sum())).astype(np.uint16)
    return row


KINDS = ("half", "one", "last", "all")


def _tables(rng, n, lo=0):
    """(name, table): S = 1 with each kind of row, S = 3, S = 300 with the kinds taking turns"""
    out = [("S 1 " + k, _row(rng, k, n, 1, lo)[None, :]) for k in KINDS]
    for S in (3, 300):
        out.append(("S %d" % S, np.stack([_row(rng, KINDS[r % 4], n, S, lo) for r in range(S)])))
    return out


def _logits(rng, n):
    x = (rng.standard_normal(n) * 2.0).astype(np.float16).view(np.uint16).copy()
    where = rng.random(n) < 0.25
    x[where] = SPECIALS[rng.integers(0, len(SPECIALS), int(where.sum()))]
    return x


def _rings(rng, table, lo=0):
    """(name, state ring, token ring, p): one crafted pair of rings per transition case"""
    S, n = table.shape
    out = []
    junk = lambda k: rng.integers(-5, S + 5, k).astype(np.int32)
    toks = lambda k: rng.integers(lo, n, k).astype(np.int32)
    out.append(("p = 0", junk(4), toks(4), 0))
    st = junk(8)
    st[4] = NONE
    out.append(("prev NONE", st, toks(8), 5))
    for trial in range(4 if S > 1 else 1):                         # valid transitions into several rows
        prev = int(rng.integers(S))
        t = int(rng.choice(np.nonzero(table[prev] != DEAD)[0]))
        st, tk = junk(9), toks(9)
        st[6], tk[7] = prev, t
        out.append(("allowed token %d" % trial, st, tk, 7))
    for prev in rng.permutation(S)[:8].tolist():                   # (an all-live row forbids nothing)
        dead = np.nonzero(table[prev] == DEAD)[0]
        if dead.size:
            st, tk = junk(9), toks(9)
            st[6], tk[7] = prev, int(rng.choice(dead[dead >= lo] if (dead >= lo).any() else dead))
            out.append(("forbidden token", st, tk, 7))
            break
    for name, t in (("t < 0", -1), ("t = -2^31", -2 ** 31), ("t = V", n), ("t > V", n + 9), ("t = 2^31 - 1", 2 ** 31 - 1)):
        st, tk = junk(6), toks(6)
        st[2], tk[3] = int(rng.integers(S)), t
        out.append((name, st, tk, 3))
    for name, p in (("p = -1", -1), ("p = -2^31", -2 ** 31), ("p = Q4_MAX_SEQ_LEN", 128 * 1024), ("p = 2^31 - 1", 2 ** 31 - 1)):
        out.append((name, junk(6), toks(6), p))                     # a position outside the ring: nothing is read through it, nothing written
    for name, prev in (("prev OFFTRACK", OFFTRACK), ("prev = S", S), ("prev garbage", 70000), ("prev = 2^31 - 1", 2 ** 31 - 1), ("prev = -7", -7)):
        st, tk = junk(6), toks(6)
        st[2] = prev
        out.append((name, st, tk, 3))
    return out


@pytest.mark.parametrize("n", [1, 8, 1000, 1027, 32000, 32768, 32776, 40000, 128256, 128259])
def test_op_matches_the_reference_bit_for_bit(q4, n):
    """(128256 / 128259: beyond 16 bits of token id, beside the tables' 16-bit states. There every live token of every table and every ring token in
    range has an id >= 65536, some beyond 98304: asserted on the tables, the rings and the reference's mask.)"""
    rng = np.random.default_rng(7000 + n)
    lo = HIGH if n > HIGH else 0
    pos = q4.DevBuf(nbytes=4)
    seen_nan = [False, False]
    highest = 0
    for tname, table in _tables(rng, n, lo):
        g = q4.Guide(table)
        x = _logits(rng, n)
        if lo:
            assert (table[:, :lo] == DEAD).all(), tname
        for cname, st, tk, p in _rings(rng, table, lo):
            what = "n %d, %s, %s" % (n, tname, cname)
            want_st = st.copy()
            want, s = ref.mask(x, table, want_st, tk, p, seq_len=128 * 1024)
            got = []
            for launch in range(2):
                dl, ds, dt = q4.DevBuf(x), q4.DevBuf(st), q4.DevBuf(tk)
                pos.put(np.array([p], dtype=np.int32))
                q4.guide_mask(dl, n, g, ds, dt, pos)
                q4.synchronize()
                got.append((dl.get(np.uint16, n), ds.get(np.int32, st.shape[0])))
            out, out_st = got[0]
            bad = np.nonzero(out != want)[0]
            assert bad.size == 0, "%s: %d entries differ, first %d: got %04x, reference %04x (input %04x)" % (what, bad.size, bad[0], out[bad[0]], want[bad[0]], x[bad[0]])
            assert np.array_equal(out_st, want_st), "%s: state ring %s, reference %s" % (what, out_st, want_st)
            assert got[1][0].tobytes() == out.tobytes() and got[1][1].tobytes() == out_st.tobytes(), what + ": a second launch gave other bytes"
            if s is None:
                assert out.tobytes() == x.tobytes() and out_st.tobytes() == st.tobytes(), what + ": a position outside the ring touched something"
            elif s == OFFTRACK:
                assert out.tobytes() == x.tobytes(), what + ": an off-track step touched the logits"
            else:
                nan = (x & 0x7FFF) > 0x7C00
                seen_nan[0] |= bool((nan & (table[s] != DEAD)).any())
                seen_nan[1] |= bool((nan & (table[s] == DEAD)).any())
                assert np.array_equal(out[table[s] != DEAD], x[table[s] != DEAD]) and (out[table[s] == DEAD] == 0xFC00).all()
                if lo:                                               # on the reference's mask: what stays is beyond 16 bits
                    kept = np.flatnonzero(want != 0xFC00)
                    assert kept.size == 0 or kept.min() >= lo, what
                    assert ((tk >= lo) | (tk < 0)).all(), what
                    highest = max(highest, int(np.flatnonzero(table[s] != DEAD).max()))
        g.close()
    if n >= 1000:
        assert seen_nan == [True, True], "no NaN in an allowed and in a forbidden slot"
    assert not lo or highest > 98304, highest


def test_op_arguments(q4):
    L = q4.lib()
    table = np.zeros((2, 100), dtype=np.uint16)
    g = q4.Guide(table)
    d, s, t, p = q4.DevBuf(nbytes=200), q4.DevBuf(nbytes=16), q4.DevBuf(nbytes=16), q4.DevBuf(nbytes=4)
    assert L.q4_guide_mask(d.ptr, 99, g.h, s.ptr, t.ptr, p.ptr) == ERR_ARG          # n must be the guide's vocabulary
    assert L.q4_guide_mask(d.ptr, 100, None, s.ptr, t.ptr, p.ptr) == ERR_ARG
    assert L.q4_guide_mask(None, 100, g.h, s.ptr, t.ptr, p.ptr) == ERR_ARG
    assert L.q4_guide_mask(d.ptr, 100, g.h, s.ptr, t.ptr, p.ptr) == 0
    q4.synchronize()
    g.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. inside the step
@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    d = tmp_path_factory.mktemp("guide")
    out = {}
    for name in ("tiny", "small", "v32k", "v40k"):
        out[name] = str(d / (name + ".bin"))
        synth.write_model(out[name], name, seed=7)
    return out


def _random_table(seed, S, V, live=0.3):
    """a seeded random automaton: about `live` of every row allowed, every row non-empty, EOS (which would end generate_ids) never"""
    rng = np.random.default_rng(seed)
    t = np.full((S, V), DEAD, dtype=np.uint16)
    on = rng.random((S, V)) < live
    on[:, 2] = False
    on[np.arange(S), rng.integers(3, V, S)] = True
    t[on] = rng.integers(0, S, int(on.sum())).astype(np.uint16)
    return t


def _poke(t, index, token):
    """writes ring entry `index` of the model's pinned token ring (SharedData: int pos; int tokens[])"""
    C.c_int.from_address(t.state.contents.shared_data + 4 + 4 * index).value = int(token)


def _set_device_pos(q4, t, p):
    """a rewind: the device keeps its own position"""
    q4.synchronize()
    v = np.array([p], dtype=np.int32)
    q4.check(q4.lib().q4_memcpy_h2d(t.state.contents.pos, v.ctypes.data, 4))


def _truth(q4, path, table, prompt, steps):
    """A guide-off model driven step by step (one run_transformer_at per step, synchronised, in the library's current graph mode and fusion level): its
    raw logits masked by the reference and argmaxed (lowest index on ties) give every generated token. Returns (ring [steps + 1], states [steps],
    raw logits [steps], masked bits [steps])."""
    t = q4.Transformer(path)
    t.reset(prompt)
    tokens = np.zeros(steps + 1, dtype=np.int32)
    tokens[:len(prompt)] = prompt
    states = np.full(steps, NONE, dtype=np.int32)
    raws, masked = [], []
    for pos in range(steps):
        t.run_transformer_at(pos, 0)
        raw = t.logits()
        out = ref.bits(raw).copy()
        if pos >= len(prompt) - 1:
            out, _ = ref.mask(raw, table, states, tokens, pos)
            tokens[pos + 1] = int(np.argmax(out.view(np.float16).astype(np.float32)))
            _poke(t, pos + 1, tokens[pos + 1])
        raws.append(raw)
        masked.append(out)
    t.close()
    return tokens, states, np.stack(raws), np.stack(masked)


def _stepwise(q4, t, prompt, steps):
    t.reset(prompt)
    for pos in range(steps):
        t.run_transformer_at(pos, pos >= len(prompt) - 1)
    q4.synchronize()
    return np.array([t.token(i) for i in range(steps + 1)], dtype=np.int32)


def _check_run(what, toks, states, truth):
    want_toks, want_states = truth[0], truth[1]
    assert len(toks) == len(want_toks), what + ": the run stopped early"
    bad = np.nonzero(toks != want_toks)[0]
    assert bad.size == 0, "%s: %d tokens differ, first at ring index %d: %d, reference %d" % (what, bad.size, bad[0], toks[bad[0]], want_toks[bad[0]])
    assert np.array_equal(states, want_states), "%s: states %s, reference %s" % (what, states, want_states)


TINY_STEPS = 40
PROMPTS = {1: [1], 7: [1, 20, 300, 7, 44, 9, 130]}


@pytest.fixture(scope="module")
def tiny_guide(q4):
    table = _random_table(11, 40, 512)
    g = q4.Guide(table)
    yield table, g
    g.close()


@pytest.mark.parametrize("n_prompt", [1, 7])
@pytest.mark.parametrize("fusion", [5, 1])
def test_guided_greedy_run_in_every_graph_form(q4, paths, tiny_guide, fusion, n_prompt):
    """tokens and states of generate_ids (eight steps per replay), of one single-step graph per step and of the two eager modes, each against the
    ground truth of the same mode; NONE on prompt positions"""
    L = q4.lib()
    table, g = tiny_guide
    prompt = PROMPTS[n_prompt]
    try:
        L.q4_set_fusion(fusion)
        truth = _truth(q4, paths["tiny"], table, prompt, TINY_STEPS)
        assert (truth[1][:n_prompt - 1] == NONE).all() and truth[1][n_prompt - 1] == 0 and (truth[1][n_prompt - 1:] >= 0).all()
        assert len(set(truth[1][n_prompt - 1:].tolist())) > 8, "the walk visits too few states to show anything"
        assert not np.array_equal(truth[3][n_prompt - 1:], ref.bits(truth[2])[n_prompt - 1:])
        t = q4.Transformer(paths["tiny"], guide=g)
        c0 = L.q4_graph_captures()
        toks = t.generate_ids(prompt, TINY_STEPS)[0].copy()
        _check_run("eight-step graphs", toks, t.guide_states(0, TINY_STEPS), truth)
        assert L.q4_graph_captures() > c0
        assert t.logits().view(np.uint16).tobytes() == truth[3][-1].tobytes(), "RunState::logits does not hold the masked logits"
        _check_run("single-step graphs", _stepwise(q4, t, prompt, TINY_STEPS), t.guide_states(0, TINY_STEPS), truth)
        t.close()
        for mode in (0, 2):
            L.q4_set_use_graphs(mode)
            truth_m = _truth(q4, paths["tiny"], table, prompt, TINY_STEPS)
            t = q4.Transformer(paths["tiny"], guide=g)
            toks = t.generate_ids(prompt, TINY_STEPS)[0].copy()
            _check_run("use_graphs %d" % mode, toks, t.guide_states(0, TINY_STEPS), truth_m)
            t.close()
            L.q4_set_use_graphs(1)
    finally:
        L.q4_set_use_graphs(1)
        L.q4_set_fusion(q4.DEFAULT_FUSION)


@pytest.mark.parametrize("name,S,steps", [("small", 40, 300), ("v32k", 3, 32), ("v40k", 3, 32)])
def test_guided_greedy_run_on_other_models(q4, paths, name, S, steps):
    """small: a span that crosses the sequence-length bins 128 and 256; v32k / v40k: the launch's register and looping paths inside a graph"""
    V = synth.geometry(name)[5]
    table = _random_table(100 + S, S, V)
    g = q4.Guide(table)
    prompt = [1, 5, 9]
    truth = _truth(q4, paths[name], table, prompt, steps)
    t = q4.Transformer(paths[name], guide=g)
    toks = t.generate_ids(prompt, steps)[0].copy()
    _check_run(name, toks, t.guide_states(0, steps), truth)
    assert t.logits().view(np.uint16).tobytes() == truth[3][-1].tobytes()
    t.close()
    g.close()


def test_a_one_state_all_live_guide_changes_nothing(q4, paths):
    L = q4.lib()
    g = q4.Guide(np.zeros((1, 512), dtype=np.uint16))
    t = q4.Transformer(paths["tiny"])
    plain = t.generate_ids([1, 20, 300], TINY_STEPS)[0].copy()
    plain_logits = t.logits()
    c1 = L.q4_graph_captures()
    t.set_guide(g)
    toks = t.generate_ids([1, 20, 300], TINY_STEPS)[0].copy()
    assert np.array_equal(toks, plain) and t.logits().tobytes() == plain_logits.tobytes()
    assert t.guide_states(0, TINY_STEPS).tolist() == [NONE, NONE] + [0] * (TINY_STEPS - 2)
    c2 = L.q4_graph_captures()
    assert c2 > c1, "the guided steps replayed the unguided graphs"
    t.set_guide(None)
    assert np.array_equal(t.generate_ids([1, 20, 300], TINY_STEPS)[0], plain)
    assert L.q4_graph_captures() == c2, "switching the guide off captured the unguided graphs again"
    t.set_guide(g)
    assert np.array_equal(t.generate_ids([1, 20, 300], TINY_STEPS)[0], plain)
    assert L.q4_graph_captures() == c2, "the same guide back on captured the guided graphs again"
    t.close()
    g.close()


SAMPLED = dict(temperature=0.8, topp=0.9, seed=4242)


def test_sampled_steps_stay_on_the_track(q4, paths, tiny_guide):
    L = q4.lib()
    table, g = tiny_guide
    prompt = PROMPTS[7]
    rings = {}
    try:
        for mode in (1, 2):                                        # eight steps per replay; eager launches of what the graphs run
            L.q4_set_use_graphs(mode)
            t = q4.Transformer(paths["tiny"], guide=g, **SAMPLED)
            toks = t.generate_ids(prompt, TINY_STEPS)[0].copy()
            states = t.guide_states(0, TINY_STEPS)
            t.close()
            assert len(toks) == TINY_STEPS + 1
            first = len(prompt) - 1
            assert (states[:first] == NONE).all()
            assert np.array_equal(states[first:], guide.walk(table, toks[first + 1:TINY_STEPS])), mode
            for p in range(first, TINY_STEPS):
                assert table[states[p], toks[p + 1]] != DEAD, "mode %d: the token of step %d is forbidden in state %d" % (mode, p, states[p])
            rings[mode] = (toks, states)
    finally:
        L.q4_set_use_graphs(1)
    assert np.array_equal(rings[1][0], rings[2][0]) and np.array_equal(rings[1][1], rings[2][1])
    t = q4.Transformer(paths["tiny"], guide=g)
    greedy = t.generate_ids(prompt, TINY_STEPS)[0].copy()
    t.close()
    assert not np.array_equal(greedy, rings[1][0]), "the sampled run is the greedy one: it shows nothing of its own"


def test_composition_with_top_k(q4, paths, tiny_guide):
    table, g = tiny_guide
    prompt = PROMPTS[7]
    truth = _truth(q4, paths["tiny"], table, prompt, TINY_STEPS)
    t = q4.Transformer(paths["tiny"], guide=g, sampling=dict(top_k=1), **SAMPLED)     # top_k = 1 counts allowed tokens: the masked argmax
    _check_run("top_k 1, sampled", t.generate_ids(prompt, TINY_STEPS)[0].copy(), t.guide_states(0, TINY_STEPS), truth)
    t.close()
    t = q4.Transformer(paths["tiny"], guide=g, sampling=dict(top_k=5))
    _check_run("top_k 5, greedy", t.generate_ids(prompt, TINY_STEPS)[0].copy(), t.guide_states(0, TINY_STEPS), truth)
    x = t.logits().astype(np.float32)
    s = int(truth[1][-1])
    finite = np.nonzero(np.isfinite(x))[0]
    assert 1 <= finite.size <= 5 and (table[s, finite] != DEAD).all()
    assert (table[s] != DEAD).sum() > 5
    t.close()


def test_records_describe_the_raw_distribution(q4, paths, tiny_guide):
    table, g = tiny_guide
    prompt, k = PROMPTS[7], 5
    truth = _truth(q4, paths["tiny"], table, prompt, TINY_STEPS)
    t = q4.Transformer(paths["tiny"], guide=g, logprobs=k)
    toks = t.generate_ids(prompt, TINY_STEPS)[0].copy()
    _check_run("with records", toks, t.guide_states(0, TINY_STEPS), truth)
    tlp, ids, top = t.logprobs(0, TINY_STEPS)
    t.close()
    off = q4.Transformer(paths["tiny"], logprobs=k)                # a guide-off model fed the same tokens
    off.reset(toks)
    for pos in range(TINY_STEPS):
        off.run_transformer_at(pos, 0)
    otlp, oids, otop = off.logprobs(0, TINY_STEPS)
    off.close()
    assert np.array_equal(ids, oids) and top.tobytes() == otop.tobytes()
    moved = 0
    for p in range(TINY_STEPS):
        x, tok = truth[2][p], int(toks[p + 1])
        assert logprobs_ref.within([tlp[p]], [logprobs_ref.logprobs(x)[tok]], logprobs_ref.bound(x, x[tok])), p
        assert logprobs_ref.within([tlp[p]], [otlp[p]], 2 * logprobs_ref.bound(x, x[tok])), p
        moved += p >= len(prompt) - 1 and tok != int(ids[p][0])
    assert moved > 8, "the guide hardly ever moved the greedy token: token_logprob shows nothing"


def test_guided_greedy_steps_are_not_screened(q4, tmp_path):
    L = q4.lib()
    path = str(tmp_path / "cls.bin")
    synth.write_model(path, "cls4096", seed=31)
    g = q4.Guide(np.zeros((1, 32000), dtype=np.uint16))
    t = q4.Transformer(path)
    plain = t.generate_ids([1, 20, 300], 24)[0].copy()
    before = t.screen_candidates()[3]
    assert before > 0, "the model does not screen at all: the checks below show nothing"
    t.set_guide(g)
    assert np.array_equal(t.generate_ids([1, 20, 300], 24)[0], plain)
    assert t.screen_candidates()[3] == before, "a guided step was screened"
    c0 = L.q4_graph_captures()
    t.set_guide(None)
    assert np.array_equal(t.generate_ids([1, 20, 300], 24)[0], plain)
    assert t.screen_candidates()[3] > before
    assert L.q4_graph_captures() == c0, "the screened graphs were captured anew"
    t.close()
    g.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the ring's rules
def test_a_second_sequence_starts_at_state_zero(q4, paths, tiny_guide):
    table, g = tiny_guide
    t = q4.Transformer(paths["tiny"], guide=g)
    a = t.generate_ids(PROMPTS[7], TINY_STEPS)[0].copy()
    sa = t.guide_states(0, TINY_STEPS)
    b = t.generate_ids(PROMPTS[7], TINY_STEPS)[0].copy()
    assert np.array_equal(a, b) and np.array_equal(sa, t.guide_states(0, TINY_STEPS))
    t.reset(PROMPTS[1])
    assert (t.guide_states(0, 64) == NONE).all()
    c = t.generate_ids(PROMPTS[1], TINY_STEPS)[0].copy()               # a shorter prompt: positions 0 .. 5 are guided now
    assert np.array_equal(t.guide_states(0, TINY_STEPS), guide.walk(table, c[1:TINY_STEPS]))
    t.close()


def test_a_forbidden_token_in_the_ring_leads_off_the_track_and_stays_there(q4, paths, tiny_guide):
    table, g = tiny_guide
    prompt, p = PROMPTS[7], 15
    t = q4.Transformer(paths["tiny"], guide=g)
    toks = t.generate_ids(prompt, 24)[0].copy()
    states = t.guide_states(0, 24)
    forbidden = int(np.nonzero(table[states[p - 1]] == DEAD)[0][5])
    _poke(t, p, forbidden)
    _set_device_pos(q4, t, p)                                         # a rewind inside the span: the step continues from state[p - 1]
    t.run_transformer_at(p, 1)
    first = t.logits()
    t.run_transformer_at(p + 1, 1)
    second = t.logits()
    after = t.guide_states(0, 24)
    ring = [t.token(i) for i in range(p + 3)]
    t.close()
    assert np.array_equal(after[:p], states[:p]) and after[p] == OFFTRACK and after[p + 1] == OFFTRACK
    off = q4.Transformer(paths["tiny"])                               # the raw logits of the same ring
    off.reset(ring)
    raw = []
    for pos in range(p + 2):
        off.run_transformer_at(pos, 0)
        raw.append(off.logits())
    off.close()
    assert first.tobytes() == raw[p].tobytes() and second.tobytes() == raw[p + 1].tobytes()
    assert ring[p + 1] == int(np.argmax(raw[p].astype(np.float32))) and ring[p + 2] == int(np.argmax(raw[p + 1].astype(np.float32)))
    # the same rewind with an allowed token continues the walk
    t = q4.Transformer(paths["tiny"], guide=g)
    t.generate_ids(prompt, 24)
    allowed = int(np.nonzero(table[states[p - 1]] != DEAD)[0][3])
    _poke(t, p, allowed)
    _set_device_pos(q4, t, p)
    t.run_transformer_at(p, 1)
    assert t.guide_states(p, 1)[0] == table[states[p - 1], allowed]
    t.close()


def test_prompt_steps_end_a_span(q4, paths, tiny_guide):
    """a chat's next turn: prompt steps behind a guided span write NONE, the next generating step starts at state 0 again"""
    table, g = tiny_guide
    t = q4.Transformer(paths["tiny"], guide=g)
    plan = [0, 0, 1, 1, 1, 1, 1, 0, 0, 1, 1, 1]                      # gen_token by position
    t.generate_ids([1], len(plan))
    assert (t.guide_states(0, len(plan)) >= 0).all()                 # every position below holds a state of an earlier span: a prompt step must clear it
    for i, tok in enumerate([1, 20, 300]):
        _poke(t, i, tok)
    _set_device_pos(q4, t, 0)                                         # (no q4_reset_sequence: it would clear the whole ring)
    for pos, gen in enumerate(plan):
        if pos in (8, 9):
            q4.synchronize()
            _poke(t, pos, 50 + pos)                                   # the next turn's prompt tokens
        t.run_transformer_at(pos, gen)
    states = t.guide_states(0, len(plan))
    ring = [t.token(i) for i in range(len(plan) + 1)]
    t.close()
    want = np.full(len(plan), NONE, dtype=np.int32)
    want[2:7] = guide.walk(table, ring[3:7])
    want[9:12] = guide.walk(table, ring[10:12])
    assert np.array_equal(states, want), (states, want)
    assert want[2] == 0 and want[9] == 0 and (want[[0, 1, 7, 8]] == NONE).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. arguments and lifetime
def test_arguments_and_lifetime(q4, paths, tiny_guide):
    L = q4.lib()
    table, shared = tiny_guide
    truth = _truth(q4, paths["tiny"], table, PROMPTS[1], TINY_STEPS)
    wrong = q4.Guide(np.zeros((1, 511), dtype=np.uint16))
    g = q4.Guide(table)
    a = q4.Transformer(paths["tiny"])
    assert L.q4_get_guide(a.h) is None
    assert L.q4_set_guide(a.h, wrong.h) == ERR_ARG                   # another vocabulary
    assert L.q4_set_guide(None, g.h) == ERR_ARG
    out = np.zeros(4, dtype=np.int32)
    assert L.q4_get_guide_states(a.h, 0, 4, out.ctypes.data) == ERR_ARG      # no guide
    assert L.q4_set_guide(a.h, None) == 0                            # off and never on
    a.set_guide(g)
    assert L.q4_get_guide(a.h) == g.h
    assert L.q4_get_guide_states(a.h, 62, 4, out.ctypes.data) == ERR_ARG and L.q4_get_guide_states(a.h, -1, 1, out.ctypes.data) == ERR_ARG
    b = q4.Transformer(paths["tiny"], guide=g)                       # one guide, two live models
    assert L.q4_guide_delete(g.h) == ERR_ARG
    for t in (a, b, a):
        _check_run("two models", t.generate_ids(PROMPTS[1], TINY_STEPS)[0].copy(), t.guide_states(0, TINY_STEPS), truth)
    a.set_guide(None)
    assert L.q4_get_guide(a.h) is None
    assert L.q4_guide_delete(g.h) == ERR_ARG                         # b still holds it
    b.close()
    g.close()                                                        # after set_guide(None) and after close() of the model
    a.set_guide(shared)                                              # another guide for a model that had one: the block is rewritten
    _check_run("another guide", a.generate_ids(PROMPTS[1], TINY_STEPS)[0].copy(), a.guide_states(0, TINY_STEPS), truth)
    a.close()
    wrong.close()
