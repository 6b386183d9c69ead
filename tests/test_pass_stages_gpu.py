"""Logit stages inside verify passes, prompt passes under the guide and Mirostat, and the guide's forced drafts (q4_set_pass_stages; DESIGN.md 3.8 "Under
the logit stages"). The yardstick is section 3.8's: BYTE equality with the run without passes -- no tolerance anywhere. Op level: row r of a row launch
against the existing one-block entry run on that row alone. End to end: tokens, K / V rows below the final position, RunState::logits, the sampler's
rng_state and the guide's state ring below the final position against the same run with speculation and prompt ingest off; every such comparison also
asserts through q4_spec_stats / q4_prompt_passes that passes ran, so a run that fell back to steps fails."""
import numpy as np
import pytest

import pass_stages_cases as cases
import spec_sampled_ref as ssref
from llama_cu_awq_amd import guide, synth

pytestmark = pytest.mark.gpu

ERR_ARG = 5
DEAD, NONE, OFFTRACK = guide.DEAD, guide.NONE, guide.OFFTRACK
SPECIALS = np.array([0x8000, 0x7C00, 0xFC00, 0x7E01, 0xFFFF, 0x7D55, 0x0000, 0xFBFF], dtype=np.uint16)   # -0, +-inf, NaNs with payloads, 0, -65504
PAD = np.array([0x7E01, 0x7C00, 0xFFFF, 0x7C00, 0x7D55, 0x7C00, 0x7E00, 0x7C00], dtype=np.uint16)       # between n and ld: NaNs and +inf


# ---- op level ---------------------------------------------------------------------------------------------------------------------------------------------
def _rows_of_logits(rng, n, n_rows):
    x = (rng.standard_normal((n_rows, n)) * 2.0).astype(np.float16).view(np.uint16).copy()
    where = rng.random((n_rows, n)) < 0.05
    x[where] = SPECIALS[rng.integers(0, len(SPECIALS), int(where.sum()))]
    return x


def _padded(x):
    return np.concatenate([x, np.tile(PAD, (x.shape[0], 1))], axis=1)


def _check_rows(q4, what, x, run_rows, run_one, p):
    """run_rows(dev rows, ld, pos_rows): the row entry over all rows; run_one(dev row, r): the one-block entry on row r alone at position p + r. Row r's
    bytes equal, the padding untouched"""
    n_rows, n = x.shape
    ld = n + 8
    rows = q4.DevBuf(_padded(x))
    pos_rows = q4.DevBuf(np.arange(p, p + n_rows, dtype=np.int32))
    run_rows(rows, ld, pos_rows)
    q4.synchronize()
    got = rows.get(np.uint16, n_rows * ld).reshape(n_rows, ld)
    assert np.array_equal(got[:, n:], np.tile(PAD, (n_rows, 1))), what + ": the padding between n and ld was written"
    changed = 0
    for r in range(n_rows):
        one = q4.DevBuf(x[r])
        run_one(one, r)
        q4.synchronize()
        want = one.get(np.uint16, n)
        bad = np.flatnonzero(got[r, :n] != want)
        assert bad.size == 0, "%s, row %d: %d entries differ, first %d: rows %04x, one block %04x (input %04x)" % (
            what, r, bad.size, bad[0], got[r, bad[0]], want[bad[0]], x[r, bad[0]])
        changed += int((want != x[r]).sum())
    return changed


OP_N = [512, 32000, 40000]      # (40000: logit_process_kernel<false>, and the guide's loop behind its register chunks)
OP_ROWS = [1, 2, 8]


@pytest.mark.parametrize("n_rows", OP_ROWS)
@pytest.mark.parametrize("n", OP_N)
def test_controls_rows(q4, n, n_rows):
    rng = np.random.default_rng(100 * n_rows + n)
    bias = {int(i): float(b) for i, b in zip(rng.choice(n, 6, replace=False), (1.5, -2.0, 30.0, -np.inf, 0.25, -0.5))}
    changed = 0
    for last_n, p in ((64, 0), (64, 5), (64, 100), (1024, 1500)):       # p = 0, inside the window, beyond it
        view = rng.integers(0, 40, p + n_rows + 3).astype(np.int32)     # few distinct tokens: counts above 1
        view[rng.integers(0, view.shape[0], 2)] = (-1, n + 5)           # entries outside the vocabulary do not count
        kw = dict(top_k=40, min_p=0.02, repeat_penalty=1.1, presence_penalty=0.3, frequency_penalty=0.1, penalty_last_n=last_n)
        dview = q4.DevBuf(view)
        x = _rows_of_logits(rng, n, n_rows)

        def one(dev, r, view=view, kw=kw, p=p):
            ring, pos = q4.DevBuf(view[:p + r + 1]), q4.DevBuf(np.array([p + r], dtype=np.int32))
            q4.process_logits(dev, n, logit_bias=bias, tokens=ring, pos=pos, **kw)
            q4.synchronize()
        changed += _check_rows(q4, "controls n %d rows %d p %d" % (n, n_rows, p), x,
                               lambda rows, ld, pos: q4.process_logits_rows(rows, n, ld, n_rows, dview, pos, logit_bias=bias, **kw), one, p)
    assert changed > 0


@pytest.mark.parametrize("n_rows", OP_ROWS)
@pytest.mark.parametrize("n", OP_N)
def test_dry_rows(q4, n, n_rows):
    rng = np.random.default_rng(200 * n_rows + n)
    changed = 0
    for last_n, p in ((64, 0), (64, 5), (64, 100), (4096, 4200)):
        view = rng.integers(3, 9, p + n_rows + 3).astype(np.int32)      # six distinct tokens: repeats of every length
        view[rng.integers(0, view.shape[0], 1)] = n + 5
        kw = dict(multiplier=0.8, base=1.75, allowed_length=2, last_n=last_n, no_repeat_ngram_size=4)
        dview = q4.DevBuf(view)
        x = _rows_of_logits(rng, n, n_rows)

        def one(dev, r, view=view, kw=kw, p=p):
            ring, pos = q4.DevBuf(view[:p + r + 1]), q4.DevBuf(np.array([p + r], dtype=np.int32))
            q4.dry_penalty(dev, n, breakers=[8], tokens=ring, pos=pos, **kw)
            q4.synchronize()
        changed += _check_rows(q4, "DRY n %d rows %d p %d" % (n, n_rows, p), x,
                               lambda rows, ld, pos: q4.dry_penalty_rows(rows, n, ld, n_rows, dview, pos, breakers=[8], **kw), one, p)
    assert changed > 0


def _guide_table(rng, n, S=24):
    t = np.full((S, n), DEAD, dtype=np.uint16)
    on = rng.random((S, n)) < 0.4
    on[np.arange(S), rng.integers(0, n, S)] = True
    t[on] = rng.integers(0, S, int(on.sum())).astype(np.uint16)
    return t


@pytest.mark.parametrize("n_rows", OP_ROWS)
@pytest.mark.parametrize("n", OP_N)
def test_guide_rows(q4, n, n_rows):
    """rows and state[p .. p + n_rows) against n_rows one-block launches at consecutive positions on ONE state ring (each reads what the one before wrote):
    a walk of allowed tokens, a forbidden token in the view (OFFTRACK from that row on, sticky), state[p - 1] NONE, OFFTRACK and garbage, p = 0"""
    rng = np.random.default_rng(300 * n_rows + n)
    table = _guide_table(rng, n)
    S = table.shape[0]
    g = q4.Guide(table)
    seen = set()
    for p, prev, forbid_at in ((0, None, None), (5, 3, None), (5, NONE, None), (5, 7, min(1, n_rows - 1)), (5, 7, n_rows - 1), (5, OFFTRACK, None),
                               (5, S + 9, None), (4200, 2, None), (4200, 11, n_rows // 2)):
        view = rng.integers(0, n, p + n_rows + 2).astype(np.int32)
        s = 0 if prev in (None, NONE) else prev
        for r in range(n_rows):                                         # an allowed walk from prev ...
            if 0 <= s < S:
                live = np.flatnonzero(table[s] != DEAD)
                dead = np.flatnonzero(table[s] == DEAD)
                if r == 0 and prev in (None, NONE):
                    s = 0                                               # (behind NONE the token is not looked at)
                elif forbid_at is not None and r == forbid_at and dead.size:
                    view[p + r] = int(rng.choice(dead))                 # ... but for one forbidden token
                    s = OFFTRACK
                else:
                    view[p + r] = int(rng.choice(live))
                    s = int(table[s, view[p + r]])
        st = rng.integers(-5, S + 5, p + n_rows + 2).astype(np.int32)
        if p > 0:
            st[p - 1] = prev
        x = _rows_of_logits(rng, n, n_rows)
        what = "guide n %d rows %d p %d prev %s forbidden at %s" % (n, n_rows, p, prev, forbid_at)
        dview, d_rows_st, d_one_st = q4.DevBuf(view), q4.DevBuf(st), q4.DevBuf(st)

        def one(dev, r):
            pos = q4.DevBuf(np.array([p + r], dtype=np.int32))
            q4.guide_mask(dev, n, g, d_one_st, dview, pos)
            q4.synchronize()
        _check_rows(q4, what, x, lambda rows, ld, pos: q4.guide_mask_rows(rows, n, ld, n_rows, g, d_rows_st, dview, pos), one, p)
        got, want = d_rows_st.get(np.int32, st.shape[0]), d_one_st.get(np.int32, st.shape[0])
        assert np.array_equal(got, want), "%s: state ring %s, one-block launches %s" % (what, got[max(p - 1, 0):p + n_rows], want[max(p - 1, 0):p + n_rows])
        assert np.array_equal(want[:p], st[:p]) and np.array_equal(want[p + n_rows:], st[p + n_rows:])
        if forbid_at is not None:
            assert (want[p + forbid_at:p + n_rows] == OFFTRACK).all(), what
        seen.update(int(v) for v in want[p:p + n_rows])
    assert OFFTRACK in seen and 0 in seen and any(v > 0 for v in seen)
    g.close()


def test_row_entries_argument_errors(q4):
    L = q4.lib()
    g = q4.Guide(np.zeros((2, 512), dtype=np.uint16))
    d, s, v, p = q4.DevBuf(nbytes=8 * 520 * 2), q4.DevBuf(nbytes=64), q4.DevBuf(nbytes=64), q4.DevBuf(np.arange(8, dtype=np.int32))
    for n_rows, ld in ((0, 520), (9, 520), (-1, 520), (2, 504), (2, 516), (2, 511)):
        assert L.q4_guide_mask_rows(d.ptr, 512, g.h, s.ptr, ld, n_rows, v.ptr, p.ptr) == ERR_ARG, (n_rows, ld)
    assert L.q4_guide_mask_rows(d.ptr, 504, g.h, s.ptr, 520, 2, v.ptr, p.ptr) == ERR_ARG              # n must be the guide's vocabulary
    assert L.q4_guide_mask_rows(d.ptr, 512, g.h, None, 520, 2, v.ptr, p.ptr) == ERR_ARG
    assert L.q4_guide_mask_rows(d.ptr, 512, g.h, s.ptr, 520, 2, None, p.ptr) == ERR_ARG
    assert L.q4_guide_mask_rows(d.ptr, 512, g.h, s.ptr, 520, 2, v.ptr, None) == ERR_ARG
    assert L.q4_guide_mask_rows(d.ptr, 512, g.h, s.ptr, 520, 8, v.ptr, p.ptr) == 0
    assert L.q4_guide_mask_rows(d.ptr, 512, g.h, s.ptr, 512, 1, v.ptr, p.ptr) == 0
    q4.synchronize()
    g.close()


def test_forced_run_is_the_restatement(q4):
    """q4_guide_forced_run against guide.forced_run from every state and NONE / OFFTRACK / S, on a from_choices and a from_regex table"""
    letters = [b""] * 3 + [bytes([0x61 + i]) for i in range(26)] + [b""] * (512 - 29)     # one token per letter: literal stretches are forced
    lit = guide.from_regex("ab(?:cde|cdf)xyz[a-c]q", letters)
    for name, table in (("choices", guide.from_choices(cases.forced_choices(8, 20), 512)), ("regex", lit)):
        g = q4.Guide(table)
        runs = 0
        for s in list(range(table.shape[0])) + [NONE, OFFTRACK, table.shape[0], 70000]:
            for room in (1, 3, 7):
                want = guide.forced_run(table, s, room)
                assert g.forced_run(s, room).tolist() == want.tolist(), (name, s, room)
                runs += want.shape[0] > 1
        assert runs > 0, name
        g.close()


# ---- end to end -------------------------------------------------------------------------------------------------------------------------------------------
N_PROMPT = 16
S_LONG = 2304
DRY = dict(multiplier=0.8, no_repeat_ngram_size=4)
CONTROLS = dict(top_k=40, repeat_penalty=1.1, penalty_last_n=64)
BIAS = {7: 1.5, 100: -3.0, 301: -np.inf}
SAMPLED = dict(temperature=0.5, topp=0.6, seed=2024)


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    d = tmp_path_factory.mktemp("pass_stages")
    out = {}
    for name in ("pass_long", "ffn_pair7b", "gqa7b_pair"):
        out[name] = str(d / (name + ".bin"))
        synth.write_model(out[name], name, seed=11)
    return out


@pytest.fixture(scope="module")
def regex_guide(q4):
    table = cases.regex_table()
    assert table.shape[0] >= 32
    g = q4.Guide(table)
    yield g
    g.close()


def _prompt(n=N_PROMPT, seed=5):
    r = np.random.default_rng(seed)
    return [1] + [int(x) for x in r.integers(3, 512, size=n - 1)]


def _kv(t, n_pos):
    snap = t.snapshot(n_pos)
    try:
        return np.frombuffer(snap.to_bytes(), dtype=np.uint8).copy()
    finally:
        snap.close()


def _stage_kw(stages, g):
    kw = {}
    if "guide" in stages:
        kw["guide"] = g
    if "dry" in stages:
        kw["dry"] = DRY
    if "controls" in stages:
        kw.update(sampling=CONTROLS, logit_bias=BIAS)
    return kw


def _state(q4, t, tokens, n_pos):
    """what every comparison compares, below position n_pos"""
    q4.check(q4.lib().q4_handoff_status(t.state))
    out = dict(tokens=np.asarray(tokens).copy(), pos=t.pos(), rows=_kv(t, n_pos), logits=t.logits().view(np.uint16).copy(), rng=ssref.sampler_struct(t.sampler).rng_state)
    if q4.lib().q4_get_guide(t.h):
        out["states"] = t.guide_states(0, n_pos).copy()
    return out


def _run(q4, path, steps, passes, prompt=None, bound=256, drafter=None, draft=7, gqa=False, **kw):
    """one generation on a fresh Transformer. passes False: the stepwise run -- speculation off, prompt ingest off, the switch off"""
    L = q4.lib()
    prompt = _prompt() if prompt is None else prompt
    L.q4_set_prompt_ingest(8 if passes else 0)
    q4.set_pass_context(bound)
    t = q4.Transformer(path, pass_stages=passes, pass_gqa=gqa, **kw)
    try:
        if passes:
            t.set_speculative(draft=draft, ngram=3, min=1, sampled=True)
        if drafter is not None:
            t.set_drafter(drafter)
        before = L.q4_prompt_passes()
        toks = t.generate_ids(prompt, steps)[0]
        out = _state(q4, t, toks, min(steps, t.pos()))
        out.update(stats=t.spec_stats(), forced=t.spec_stats_forced(), prompt_passes=L.q4_prompt_passes() - before)
    finally:
        t.close()
        L.q4_set_prompt_ingest(8)
        q4.set_pass_context(256)
    return out


def _assert_same(off, on, what):
    assert np.array_equal(off["tokens"], on["tokens"]), "%s: tokens differ, first at %d" % (what, int(np.argmax(off["tokens"][:len(on["tokens"])] != on["tokens"][:len(off["tokens"])])))
    assert off["pos"] == on["pos"], what
    assert off["rows"].shape == on["rows"].shape and np.array_equal(off["rows"], on["rows"]), "%s: K / V rows differ" % what
    assert np.array_equal(off["logits"], on["logits"]), "%s: RunState::logits differ in %d entries" % (what, int((off["logits"] != on["logits"]).sum()))
    assert off["rng"] == on["rng"], "%s: rng_state" % what
    if "states" in off or "states" in on:
        assert np.array_equal(off["states"], on["states"]), "%s: the guide's states differ, first at %d" % (what, int(np.argmax(off["states"] != on["states"])))


def test_default_off(q4, models, regex_guide):
    """the switch off and a stage on: q4_verify_covers says 0 and no pass runs, even with q4_set_speculative on; the switch itself round-trips"""
    L = q4.lib()
    R = _run(q4, models["ffn_pair7b"], 60, False, guide=regex_guide)
    for kw in (dict(guide=regex_guide), dict(dry=DRY), dict(sampling=CONTROLS), dict(logit_bias=BIAS)):
        t = q4.Transformer(models["ffn_pair7b"], **kw)
        try:
            assert not t.pass_stages()
            t.set_speculative(draft=7, ngram=3, min=1, sampled=True)
            t.set_drafter(lambda ring, room: R["tokens"][len(ring):len(ring) + room])
            if "guide" in kw:
                assert not t.verify_covers(20, 3)
            t.generate_ids(_prompt(), 60)
            assert t.spec_stats() == (0, 0, 0) and t.spec_stats_forced() == (0, 0), kw
            t.set_pass_stages(True)
            assert t.pass_stages() and L.q4_get_pass_stages(t.h) == 1
            if "guide" in kw:
                assert t.verify_covers(20, 3)
            t.set_pass_stages(False)
            assert not t.pass_stages()
        finally:
            t.close()


@pytest.mark.parametrize("top_k", [False, True])
@pytest.mark.parametrize("sampled", [False, True])
def test_forced_drafts(q4, models, sampled, top_k):
    """from_choices of 8 sequences of 20 tokens that share their first token only (tests/test_pass_stages_host.py checks on the CPU that every state behind
    a choice's second token is forced): the shared token is drafted at the first generating position, the eighteen tokens behind the choice and the EOS in
    passes of 7, 7 and 3 -- every forced draft accepted, and the bytes of the stepwise run. The run ends at the EOS with no step to spare (steps = EOS + 1)."""
    seqs = cases.forced_choices(8, 20)
    g = q4.Guide(guide.from_choices(seqs, 512))
    kw = dict(guide=g, **(SAMPLED if sampled else {}))
    if top_k:
        kw["sampling"] = dict(top_k=40)
    steps = N_PROMPT + 21
    try:
        off = _run(q4, models["ffn_pair7b"], steps, False, **kw)
        on = _run(q4, models["ffn_pair7b"], steps, True, **kw)
    finally:
        g.close()
    gen = off["tokens"][N_PROMPT:].tolist()
    assert gen[:20] in seqs and gen[20] == 2, gen
    print("forced drafts (sampled %s, top-k %s): passes %s forced %s" % (sampled, top_k, on["stats"], on["forced"]))
    _assert_same(off, on, "forced drafts")
    assert off["stats"] == (0, 0, 0) and off["forced"] == (0, 0)
    drafted, accepted = on["forced"]
    assert accepted == drafted and drafted >= 18
    assert on["stats"] == (4, drafted, accepted)                          # nothing but forced drafts: the n-gram drafter was never needed


STAGE_SETS = [("guide",), ("dry",), ("controls",), ("guide", "dry", "controls")]


@pytest.mark.parametrize("sampled", [False, True])
@pytest.mark.parametrize("stages", STAGE_SETS, ids=lambda s: "+".join(s))
def test_every_first_wrong_index(q4, models, regex_guide, stages, sampled):
    """the run's own continuation corrupted at index 0 .. 7 by call, under each stage alone and all three together, greedy and sampled: the stepwise run's
    bytes, and exactly the counters the drafter's bookkeeping predicts"""
    kw = dict(_stage_kw(stages, regex_guide), **(SAMPLED if sampled else {}))
    steps = 200
    off = _run(q4, models["pass_long"], steps, False, **kw)
    assert len(off["tokens"]) == steps + 1 and off["stats"] == (0, 0, 0)
    d = cases.FirstWrong(off["tokens"])
    on = _run(q4, models["pass_long"], steps, True, drafter=d, **kw)
    print("%s sampled %s: passes, drafted, accepted = %s" % ("+".join(stages), sampled, on["stats"]))
    _assert_same(off, on, "+".join(stages))
    assert on["stats"] == d.stats() and on["stats"][0] >= 20 and on["forced"] == (0, 0)
    assert d.seen == set(range(8))
    if "guide" in stages:
        assert (off["states"][N_PROMPT - 1:] >= 0).all() and (off["states"][:N_PROMPT - 1] == NONE).all()


@pytest.mark.parametrize("sampled", [False, True])
def test_long_run_with_the_windows_full(q4, models, regex_guide, sampled):
    """all three stages to position 1100 with q4_set_pass_context(2304): the penalties' and the ban's windows are full, passes run in the split-context bins
    and are cut at the bin ends 256, 512 and 1024"""
    kw = dict(_stage_kw(STAGE_SETS[3], regex_guide), **(SAMPLED if sampled else {}))
    kw["dry"] = dict(DRY, last_n=1024)
    steps = 1100
    off = _run(q4, models["pass_long"], steps, False, bound=S_LONG, **kw)
    assert len(off["tokens"]) == steps + 1
    d = cases.FirstWrong(off["tokens"])
    on = _run(q4, models["pass_long"], steps, True, bound=S_LONG, drafter=d, **kw)
    _assert_same(off, on, "to position 1100")
    assert on["stats"] == d.stats() and on["stats"][0] >= 150


def test_grouped_query(q4, models, regex_guide):
    kw = _stage_kw(STAGE_SETS[3], regex_guide)
    off = _run(q4, models["gqa7b_pair"], 120, False, **kw)
    d = cases.FirstWrong(off["tokens"])
    on = _run(q4, models["gqa7b_pair"], 120, True, drafter=d, gqa=True, **kw)
    _assert_same(off, on, "gqa7b_pair")
    assert on["stats"] == d.stats() and on["stats"][0] >= 10


def test_primitive_under_a_guide(q4, models, regex_guide):
    """q4_verify_tokens with a guide attached, at three positions and every first-wrong index, against stepping to where the pass ends"""
    path = models["pass_long"]
    R = _run(q4, path, 260, False, guide=regex_guide)["tokens"]
    t = q4.Transformer(path, guide=regex_guide)
    try:
        assert t.verify(R[21:24].tolist()) is None                        # the switch is off: not admitted
        t.set_pass_stages(True)
        n = 0
        for p in (N_PROMPT + 4, 100, 240):
            for k in range(8):
                want = _run(q4, path, p + k + 1, False, guide=regex_guide)
                t.generate_ids(R[:N_PROMPT], p)
                assert t.pos() == p and t.verify_covers(p, 7)
                drafts = [int(x) for x in R[p + 1:p + 8]]
                if k < 7:
                    drafts[k] = cases.wrong(drafts[k])
                emitted, acc = t.verify(drafts)
                n += 1
                assert acc == k and emitted.tolist() == R[p + 1:p + k + 2].tolist(), (p, k)
                assert t.pos() == p + k + 1 == want["pos"] and t.spec_stats() == (n, 7 * n, t.spec_stats()[2])
                got = _state(q4, t, [t.token(i) for i in range(p + k + 2)], p + k + 1)
                got["rng"] = want["rng"]                                  # (the greedy primitive draws no coin)
                _assert_same(want, got, "primitive at %d, first wrong %d" % (p, k))
    finally:
        t.close()


@pytest.mark.parametrize("stage", ["guide", "mirostat"])
def test_prompt_passes(q4, models, regex_guide, stage):
    """a 200-token prompt and six generated steps, twice on one Transformer (the second prompt meets the first run's state by position): prompt passes run,
    the state ring / mu ring are NONE over the prompt positions and the stepwise run's behind them"""
    L = q4.lib()
    kw = dict(guide=regex_guide) if stage == "guide" else dict(adaptive=dict(mirostat_tau=5.0, mirostat_eta=0.1), **SAMPLED)
    out = {}
    for passes in (False, True):
        L.q4_set_prompt_ingest(8 if passes else 0)
        t = q4.Transformer(models["ffn_pair7b"], pass_stages=passes, **kw)
        try:
            before = L.q4_prompt_passes()
            t.generate_ids(_prompt(60, seed=8), 230)
            toks = t.generate_ids(_prompt(200), 206)[0]
            s = _state(q4, t, toks, 206)
            s["prompt_passes"] = L.q4_prompt_passes() - before
            if stage == "mirostat":
                s["mu"] = t.adaptive_records(0, 206).view(np.uint32).copy()
            out[passes] = s
        finally:
            t.close()
            L.q4_set_prompt_ingest(8)
    _assert_same(out[False], out[True], "prompt passes under " + stage)
    assert out[False]["prompt_passes"] == 0 and out[True]["prompt_passes"] >= 24 + 7
    if stage == "guide":
        assert (out[True]["states"][:199] == NONE).all() and (out[True]["states"][199:] >= 0).all()
    else:
        assert np.array_equal(out[False]["mu"], out[True]["mu"]), "Mirostat's records differ"
        mu = out[True]["mu"].view(np.float32)[:, 3]
        assert np.isnan(mu[:199]).all() and not np.isnan(mu[199:]).any()


@pytest.mark.parametrize("what", ["records", "typical_p"])
def test_compositions_that_stay_on_steps(q4, models, regex_guide, what):
    """records together with a stage, or the adaptive truncation: no verify pass even with the switch on, and the stepwise run's outputs"""
    kw = dict(guide=regex_guide, logprobs=3, pass_logprobs=True) if what == "records" else dict(adaptive=dict(typical_p=0.9), sampling=CONTROLS, **SAMPLED)
    off = _run(q4, models["ffn_pair7b"], 80, False, **kw)
    on = _run(q4, models["ffn_pair7b"], 80, True, drafter=lambda ring, room: off["tokens"][len(ring):len(ring) + room], **kw)
    _assert_same(off, on, what)
    assert on["stats"] == (0, 0, 0)


def test_resume_behind_rejected_drafts_and_two_models(q4, models, regex_guide):
    """Behind a pass with rejected drafts under a guide the states above the position are not trusted: q4_common_prefix stops at the position, steps that
    go on from there rewrite them and give the stepwise run's bytes, and q4_resume_sequence (a new sequence for the guide: its ring goes to NONE) behaves
    as it does behind steps. A second model with the switch off alternates with the first and each keeps its own run."""
    path = models["pass_long"]
    off = _run(q4, path, 120, False, guide=regex_guide)
    R = off["tokens"]

    def steps_to(t, first, last):
        for _ in range(first, last):
            t.run_transformer(1)
        q4.synchronize()
        out = _state(q4, t, [t.token(i) for i in range(last + 1)], last)
        out["rng"] = off["rng"]                                           # (greedy runs; these Samplers have drawn for earlier generations too)
        return out
    a = q4.Transformer(path, guide=regex_guide, pass_stages=True)
    b = q4.Transformer(path, guide=regex_guide)
    c = q4.Transformer(path, guide=regex_guide)
    try:
        a.generate_ids(R[:N_PROMPT], 40)
        b.generate_ids(R[:N_PROMPT], 30)
        drafts = [int(x) for x in R[41:48]]
        drafts[2] = cases.wrong(drafts[2])
        emitted, acc = a.verify(drafts)
        assert acc == 2 and a.pos() == 43
        assert b.verify(drafts) is None and b.pos() == 30                 # (the other model's switch is off)
        assert a.common_prefix(R[:60]) == 43
        toks_b = b.generate_ids(R[:N_PROMPT], 120)[0]
        _assert_same(off, steps_to(a, 43, 120), "steps behind rejected drafts")
        got_b = _state(q4, b, toks_b, 120)
        got_b["rng"] = off["rng"]
        _assert_same(off, got_b, "the other model")
        assert a.spec_stats() == (1, 7, 2) and b.spec_stats() == (0, 0, 0)
        # resume at 60 behind another pass with rejected drafts, against the same on a model that only ever stepped
        for t in (a, c):
            t.generate_ids(R[:N_PROMPT], 55)
        drafts = [int(x) for x in R[56:63]]
        drafts[4] = cases.wrong(drafts[4])
        assert a.verify(drafts)[1] == 4 and a.pos() == 60 and a.common_prefix(R[:80]) == 60
        for _ in range(55, 60):
            c.run_transformer(1)
        q4.synchronize()
        assert c.pos() == 60 and c.common_prefix(R[:80]) == 60
        for t in (a, c):
            t.resume(R[:61], 60)
        _assert_same(steps_to(c, 60, 120), steps_to(a, 60, 120), "resumed behind rejected drafts")
    finally:
        a.close()
        b.close()
        c.close()
