"""Context shift on synthetic models (q4_shift_context and the loops that call it): the shifted model against the numpy restatement applied to a
snapshot of the same rows -- tokens, logits and K / V rows BIT FOR BIT --, the rotation against what RoPE means, the library's loops against the
composition by hand, and what moves with the rows: guide states, log-probability records, the prefix that may still be reused."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import context_shift_ref as ref
from conftest import GOLDEN, ROOT
from llama_cu_awq_amd import guide, synth

pytestmark = pytest.mark.gpu
ERR_ARG = 5
EXE = os.path.join(ROOT, "llama_cu_awq_amd", "bin", "llama2_q4")
TOK = os.path.join(GOLDEN, "tokenizer.bin")
SEED = 4242
SNAP_HEADER = 48             # {magic, version, kv_format, n_layers, n_kv_heads, head_size, n_pos, rope_theta, fingerprint, payload_bytes}


def prompt_of(name, length, salt=0):
    vocab = synth.geometry(name)[5]
    rng = np.random.default_rng(1000 + salt)
    p = rng.integers(3, vocab, length, dtype=np.int32)
    p[0] = 1
    return p


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("shift")
    made = {}

    def get(name, seed=SEED, seq_len=None):
        key = (name, seed, seq_len)
        if key not in made:
            cfg = list(synth.geometry(name))
            if seq_len:
                cfg[6] = seq_len
            path = str(d / ("%s_%d_%s.bin" % (name, seed, seq_len or "own")))
            synth.write_model(path, tuple(cfg), seed=seed)
            made[key] = path
        return made[key]
    return get


def shifted(tokens, keep, D):
    return np.concatenate([tokens[:keep], tokens[keep + D:]]).astype(np.int32)


def shift_blob(blob, tokens, keep, D, cos_sin):
    """the serialised snapshot of positions [0, n_pos) -> the one of [0, n_pos - D) a context shift leaves, by the restatement. tokens: the ring,
    n_pos + 1 of them"""
    kv_format, layers, heads, hs, n_pos = struct.unpack_from("<5i", blob, 8)
    kv_dim, new = heads * hs, n_pos - D
    body = np.frombuffer(blob, dtype=np.uint8, offset=SNAP_HEADER + 4 * n_pos)
    if kv_format == 0:
        rows = body.view(np.float16).reshape(2, layers, n_pos, kv_dim).copy()
        ref.shift_fp16(rows[0], rows[1], n_pos, keep, D, hs, cos_sin)
        payload = np.ascontiguousarray(rows[:, :, :new]).view(np.uint8).reshape(-1)
    else:
        nb = 2 * layers * n_pos * kv_dim
        rows = body[:nb].reshape(2, layers, n_pos, kv_dim).copy()
        exps = body[nb:].view(np.int8).reshape(2, layers, heads, n_pos).copy()
        ref.shift_fp8(rows[0], rows[1], exps[0], exps[1], n_pos, keep, D, hs, cos_sin)
        payload = np.concatenate([np.ascontiguousarray(rows[:, :, :new]).reshape(-1), np.ascontiguousarray(exps[:, :, :, :new]).view(np.uint8).reshape(-1)])
    head = bytearray(blob[:SNAP_HEADER])
    struct.pack_into("<i", head, 24, new)
    struct.pack_into("<Q", head, 40, payload.size)
    return bytes(head) + shifted(tokens, keep, D)[:new].tobytes() + payload.tobytes()


def all_rows(t, n):
    return np.stack([np.stack(t.kv_row(layer, pos)) for layer in range(t.config.n_layers) for pos in range(n)])


def shifted_pair(q4, files, name, n_pos, keep, D, kv="fp16"):
    """(A after shift_context + continuation, B after restoring the restated snapshot + the same continuation): tokens, logits, rows"""
    path = files(name)
    P = prompt_of(name, min(24, max(2, n_pos // 2)))
    a, b = q4.Transformer(path, kv=kv), q4.Transformer(path, kv=kv)
    try:
        toks = a.generate_ids(P, n_pos)[0].copy()
        assert a.pos() == n_pos and len(toks) == n_pos + 1
        snap = a.snapshot(n_pos)
        blob = snap.to_bytes()
        snap.close()
        new = n_pos - D
        snap_b = q4.Snapshot.from_bytes(shift_blob(blob, toks, keep, D, a.rope_row(D)))
        b.restore(snap_b)
        a.shift_context(keep, D)
        ring = shifted(toks, keep, D)
        assert a.pos() == new and [a.token(i) for i in range(new + 1)] == ring.tolist()
        S = min(new + 12, a.config.seq_len)
        ta = a.generate_ids_from(ring, S, new)[0].copy()
        tb = b.generate_ids_from(ring, S, new)[0].copy()
        snap_b.close()
        assert len(ta) == S + 1 and np.array_equal(ta[:new + 1], ring)
        return (ta, a.logits(), all_rows(a, S)), (tb, b.logits(), all_rows(b, S))
    finally:
        a.close()
        b.close()


def assert_same(x, y):
    assert np.array_equal(x[0], y[0])
    assert np.array_equal(x[1].view(np.uint16), y[1].view(np.uint16))
    assert np.array_equal(x[2].view(np.uint16), y[2].view(np.uint16))


# head64_long (1300, 16, 650): the position falls from a split-context bin to below 512; (600, 0, 50) stays in the split bins
CASES = [("tiny_gqa", 64, 4, 1), ("tiny_gqa", 64, 0, 30), ("tiny_gqa", 33, 1, 32), ("small", 320, 8, 100), ("small", 200, 128, 1),
         ("head64_long", 1300, 16, 650), ("head64_long", 600, 0, 50), ("head96", 300, 2, 149), ("head128_gqa", 700, 4, 300)]
CASES_FP8 = [("small", 320, 8, 100), ("head256", 600, 4, 298), ("head64_long", 1300, 16, 650)]


@pytest.mark.parametrize("name, n_pos, keep, D", CASES)
def test_shifted_model_equals_the_restatement(q4, files, name, n_pos, keep, D):
    assert_same(*shifted_pair(q4, files, name, n_pos, keep, D))


@pytest.mark.parametrize("name, n_pos, keep, D", CASES_FP8)
def test_the_same_on_an_fp8_cache(q4, files, name, n_pos, keep, D):
    assert_same(*shifted_pair(q4, files, name, n_pos, keep, D, kv="fp8"))


@pytest.mark.parametrize("graphs", [0, 2])
def test_the_same_without_captured_graphs(q4, files, graphs):
    L = q4.lib()
    L.q4_set_use_graphs(graphs)
    try:
        assert_same(*shifted_pair(q4, files, "small", 320, 8, 100))
    finally:
        L.q4_set_use_graphs(1)


def test_the_same_at_fusion_level_1(q4, files):
    L = q4.lib()
    L.q4_set_fusion(1)
    try:
        assert_same(*shifted_pair(q4, files, "small", 320, 8, 100))
    finally:
        L.q4_set_fusion(q4.DEFAULT_FUSION)


def test_the_rotation_means_what_rope_means(q4, files):
    """a second model ingests the SHIFTED tokens from position 0. Layer 0's K and V depend on the token and the position only: its V rows equal the
    shifted model's bit for bit, its K rows agree within the host test's bound (context_shift_ref.tolerance), the pair's norm taken from its row"""
    name, n_pos, keep, D = "small", 320, 8, 100
    P = prompt_of(name, 24)
    a, c = q4.Transformer(files(name)), q4.Transformer(files(name))
    toks = a.generate_ids(P, n_pos)[0].copy()
    a.shift_context(keep, D)
    new = n_pos - D
    ring = shifted(toks, keep, D)
    c.generate_ids(ring[:new], new)
    assert c.pos() == new
    hs = a.config.dim // a.config.n_heads
    worst = 0.0
    for pos in range(new):
        (ka, va), (kc, vc) = a.kv_row(0, pos), c.kv_row(0, pos)
        assert np.array_equal(va.view(np.uint16), vc.view(np.uint16)), pos
        if pos < keep:
            assert np.array_equal(ka.view(np.uint16), kc.view(np.uint16)), pos
        k64 = kc.astype(np.float64).reshape(-1, hs)
        hyp = np.hypot(k64[:, :hs // 2], k64[:, hs // 2:])
        tol = ref.tolerance(np.concatenate([hyp, hyp], axis=1))
        err = np.abs(ka.astype(np.float64).reshape(-1, hs) - k64)
        worst = max(worst, float((err / tol).max()))
        assert (err <= tol).all(), (pos, float((err / tol).max()))
    print("layer-0 K after a shift against a fresh ingest: worst %.3f of the bound" % worst)
    a.close()
    c.close()


# ---- the loops ---------------------------------------------------------------------------------------------------------------------------------------
KEEP, DISCARD, SEQ, STEPS = 4, 20, 64, 64 + 45


def by_hand(t, P, steps, keep=KEEP, discard=DISCARD):
    """generate to the wall, shift, generate from the shifted ring to the next wall, and so on: (history, shifts)"""
    seq = t.config.seq_len
    ring = t.generate_ids(P, min(steps, seq))[0].copy()
    hist, done, shifts = ring.tolist(), min(steps, seq), 0
    while done < steps:
        t.shift_context(keep, discard)
        shifts += 1
        ring = shifted(ring, keep, discard)
        at = seq - discard
        assert len(ring) == at + 1
        n = min(steps - done, discard)
        ring = t.generate_ids_from(ring, at + n, at)[0].copy()
        hist += ring[at + 1:].tolist()
        done += n
    return np.array(hist, dtype=np.int32), shifts


@pytest.mark.parametrize("sampling", [None, dict(repeat_penalty=1.3, penalty_last_n=32)], ids=["plain", "repeat_penalty"])
def test_generate_ids_equals_the_composition_by_hand(q4, files, sampling):
    """tiny_gqa, 64 positions, (keep, discard) = (4, 20), 64 + 45 steps: the wall is met at steps 64, 84 and 104. The penalty window reads the ring by
    position, so the composition holds with it"""
    path = files("tiny_gqa")
    P = prompt_of("tiny_gqa", 10)
    kw = dict(sampling=sampling) if sampling else {}
    auto, hand = q4.Transformer(path, context_shift=(KEEP, DISCARD), **kw), q4.Transformer(path, **kw)
    assert auto.context_shift() == (KEEP, DISCARD) and hand.context_shift() == (0, 0)
    got, _, timed, _ = auto.generate_ids(P, STEPS)
    want, shifts = by_hand(hand, P, STEPS)
    assert shifts >= 2 and timed == STEPS - 1 and len(got) == STEPS + 1
    assert not (got[1:] == 2).any()                       # no EOS in sight
    assert np.array_equal(got, want)
    assert auto.pos() == hand.pos() == STEPS - shifts * DISCARD
    assert np.array_equal(auto.logits().view(np.uint16), hand.logits().view(np.uint16))
    if sampling:
        plain = q4.Transformer(path, context_shift=(KEEP, DISCARD))
        assert not np.array_equal(plain.generate_ids(P, STEPS)[0], got)     # (the penalty does decide tokens here)
        plain.close()
    auto.close()
    hand.close()


def test_sampled_generation_repeats_with_its_seed(q4, files):
    path = files("tiny_gqa")
    P = prompt_of("tiny_gqa", 10)
    runs = []
    for _ in range(2):
        t = q4.Transformer(path, temperature=0.7, topp=0.9, seed=99, context_shift=(KEEP, DISCARD))
        runs.append(t.generate_ids(P, STEPS)[0].copy())
        t.close()
    assert len(runs[0]) == STEPS + 1 and np.array_equal(runs[0], runs[1])
    greedy = q4.Transformer(path, context_shift=(KEEP, DISCARD))
    assert not np.array_equal(greedy.generate_ids(P, STEPS)[0], runs[0])
    greedy.close()


def test_the_setting_changes_nothing_below_the_wall_and_off_clamps(q4, files):
    path = files("tiny_gqa")
    P = prompt_of("tiny_gqa", 10)
    on, off = q4.Transformer(path, context_shift=(KEEP, DISCARD)), q4.Transformer(path)
    for steps in (50, SEQ):
        a, b = on.generate_ids(P, steps), off.generate_ids(P, steps)
        assert np.array_equal(a[0], b[0]) and a[2] == b[2] == steps - 1
        assert np.array_equal(on.logits().view(np.uint16), off.logits().view(np.uint16))
    out = np.zeros(STEPS + 2, dtype=np.int32)
    import ctypes as C
    timed = C.c_int()
    tps = q4.lib().q4_generate_ids(off.h, off.sampler, P.ctypes.data, len(P), STEPS, out.ctypes.data, C.byref(timed), None)
    assert tps >= 0 and timed.value == SEQ - 1 and off.pos() == SEQ and not out[SEQ + 1:].any()      # steps above seq_len clamp as before
    L = q4.lib()
    assert L.q4_set_context_shift(on.h, -1, 4) == ERR_ARG and L.q4_set_context_shift(on.h, 4, -1) == ERR_ARG
    assert L.q4_set_context_shift(on.h, 40, 25) == ERR_ARG and on.context_shift() == (KEEP, DISCARD)     # keep + discard above seq_len
    on.set_context_shift(0, 0)
    assert on.context_shift() == (0, 0)
    on.close()
    off.close()


# ---- what moves with the rows ------------------------------------------------------------------------------------------------------------------------
def test_guide_states_move_and_the_automaton_continues(q4, files):
    """small with 96 positions, (keep, discard) = (8, 40): two choices of 100 tokens, longer than the 40 steps between two walls"""
    vocab = synth.geometry("small")[5]
    rng = np.random.default_rng(8)
    c1 = rng.integers(3, vocab, 100).tolist()
    c2 = c1[:5] + rng.integers(3, vocab, 95).tolist()
    table = guide.from_choices([c1, c2], vocab)
    path = files("small", seq_len=96)
    P = prompt_of("small", 12)
    keep, D, seq = 8, 40, 96
    g1, g2 = q4.Guide(table), q4.Guide(table)
    hand = q4.Transformer(path, guide=g1)
    ring = hand.generate_ids(P, seq)[0].copy()
    assert hand.pos() == seq
    pre = hand.guide_states(0, seq)
    assert (pre[:11] == q4.GUIDE_NONE).all() and pre[11] == 0 and (pre[11:] >= 0).all()
    hand.shift_context(keep, D)
    assert np.array_equal(hand.guide_states(keep, seq - D - keep), pre[keep + D:])
    assert np.array_equal(hand.guide_states(0, keep), pre[:keep])
    hist = ring.tolist()
    pos = seq - D
    while hist[-1] != 2 and len(hist) < 200:              # the automaton goes on from the moved state: step by step, nothing is reset
        hand.run_transformer_at(pos, 1)
        q4.synchronize()
        pos += 1
        hist.append(hand.token(pos))
    generated = hist[len(P):]
    assert generated[-1] == 2 and generated[:-1] in (c1, c2)
    states = guide.walk(table, generated)
    assert (states >= 0).all()                            # never off the guide, never dead
    auto = q4.Transformer(path, guide=g2, context_shift=(keep, D))
    got = auto.generate_ids(P, 190)[0]
    assert np.array_equal(got, np.array(hist, dtype=np.int32))
    assert (guide.walk(table, got[len(P):]) >= 0).all()
    for t in (hand, auto):
        t.close()
    g1.close()
    g2.close()


def test_logprob_records_move_with_the_rows(q4, files):
    t = q4.Transformer(files("small"), logprobs=3)
    P = prompt_of("small", 20)
    n_pos, keep, D = 200, 8, 50
    t.generate_ids(P, n_pos)
    pre = t.logprobs(0, n_pos)
    t.shift_context(keep, D)
    post = t.logprobs(0, n_pos - D)
    for x, y in zip(pre, post):
        assert np.array_equal(y[keep:].view(np.uint32), x[keep + D:].view(np.uint32))       # record p - D after is record p before
        assert np.array_equal(y[:keep].view(np.uint32), x[:keep].view(np.uint32))
    t.close()


def test_common_prefix_stops_at_the_kept_rows(q4, files):
    t = q4.Transformer(files("small"))
    P = prompt_of("small", 20)
    toks = t.generate_ids(P, 100)[0].copy()
    assert t.common_prefix(toks) == 100
    t.shift_context(8, 30)
    ring = shifted(toks, 8, 30)
    assert t.common_prefix(ring) == 8                     # the ring's own tokens: the rows above the kept ones are not theirs
    t.shift_context(3, 10)
    assert t.common_prefix(shifted(ring, 3, 10)) == 3     # the smallest n_keep seen
    snap = t.snapshot(40)                                 # still allowed
    snap.close()
    t.reset(P)
    again = t.generate_ids(P, 100)[0]
    assert np.array_equal(again, toks) and t.common_prefix(toks) == 100
    t.close()


def test_refusals_touch_nothing(q4, files):
    t = q4.Transformer(files("small"))
    P = prompt_of("small", 20)
    toks = t.generate_ids(P, 100)[0].copy()
    L = q4.lib()
    rows = [t.kv_row(1, p) for p in (0, 50, 99)]
    for n_pos, keep, D, n_ring in [(101, 8, 30, 102), (100, 80, 30, 101), (100, 8, 0, 101), (100, 8, 30, 100), (100, -1, 30, 101),
                                   (100, 8, 30, 128 * 1024 + 1), (321, 8, 30, 322)]:
        assert L.q4_shift_context(t.h, n_pos, keep, D, n_ring) == ERR_ARG, (n_pos, keep, D, n_ring)
    assert t.pos() == 100 and [t.token(i) for i in range(101)] == toks.tolist()
    for p, (k, v) in zip((0, 50, 99), rows):
        k2, v2 = t.kv_row(1, p)
        assert np.array_equal(k.view(np.uint16), k2.view(np.uint16)) and np.array_equal(v.view(np.uint16), v2.view(np.uint16))
    assert t.common_prefix(toks) == 100
    buf = np.zeros(64, dtype=np.float32)
    assert L.q4_get_rope_row(t.h, -1, buf.ctypes.data) == ERR_ARG and L.q4_get_rope_row(t.h, 320, buf.ctypes.data) == ERR_ARG
    assert np.array_equal(t.rope_row(0), np.stack([np.ones(32, np.float32), np.zeros(32, np.float32)], axis=1))
    t.close()


# ---- the CLI -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli_model(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("shiftcli") / "cli.bin")
    synth.write_model(p, (256, 352, 2, 4, 4, 32000, 256, 10000.0), seed=31)
    return p


def _cli(model, shift, args, stdin=""):
    env = dict(os.environ)
    env.pop("Q4_CONTEXT_SHIFT", None)
    if shift:
        env["Q4_CONTEXT_SHIFT"] = shift
    r = subprocess.run([EXE, model, "-z", TOK] + list(args), input=stdin, capture_output=True, text=True, timeout=300, errors="replace", env=env)
    return r


def _generate(model, shift, n):
    r = _cli(model, shift, ["-n", str(n), "-t", "0", "-i", "write an essay about GPUs and the memory they stream"])
    assert r.returncode == 0, r.stderr
    m = re.search(r"achieved tok/s: [0-9.infa-]+\. Tokens: (-?\d+), seconds: [0-9.e+-]+", r.stdout)
    assert m, r.stdout
    return re.sub(r"achieved tok/s.*", "", r.stdout), int(m.group(1))


def test_cli_generates_past_seq_len(cli_model):
    text, tokens = _generate(cli_model, "keep=4,discard=100", 400)
    assert tokens == 399                                   # more than 256 positions' worth of steps
    again, tokens2 = _generate(cli_model, "keep=4,discard=100", 400)
    assert again == text and tokens2 == tokens
    clamped, n_clamped = _generate(cli_model, None, 400)    # without the variable: -n 400 clamps, as before
    at_256, n_256 = _generate(cli_model, None, 256)
    assert clamped == at_256 and n_clamped == n_256 == 255
    assert text.startswith(at_256.rstrip("\n")) and len(text) > len(at_256)
    below, n_below = _generate(cli_model, "keep=4,discard=100", 200)      # the setting alone changes nothing below the wall
    plain, n_plain = _generate(cli_model, None, 200)
    assert below == plain and n_below == n_plain == 199
    bad = _cli(cli_model, "keep=4,discard=0", ["-n", "10", "-t", "0", "-i", "x"])
    assert bad.returncode != 0 and "Q4_CONTEXT_SHIFT" in bad.stderr
    bad = _cli(cli_model, "keep=200,discard=100", ["-n", "10", "-t", "0", "-i", "x"])
    assert bad.returncode != 0 and "Q4_CONTEXT_SHIFT" in bad.stderr


def test_cli_chat_ends_by_n_not_at_seq_len(cli_model):
    """the synthetic model never chooses EOS, so the first turn's answer runs until the step count ends it"""
    def chat(shift, n):
        r = _cli(cli_model, shift, ["-m", "chat", "-n", str(n), "-t", "0", "-y", "be brief", "-i", "tell me about GPUs"], stdin="and then?\n")
        assert r.returncode == 0, r.stderr
        return r.stdout
    at_wall, past = chat(None, 256), chat(None, 300)
    assert past == at_wall                                 # without the variable the chat ends at position 256
    shifted_300, shifted_340 = chat("keep=4,discard=100", 300), chat("keep=4,discard=100", 340)
    assert shifted_300.startswith(at_wall.rstrip("\n")) and len(shifted_300) > len(at_wall)
    assert shifted_340.startswith(shifted_300.rstrip("\n")) and len(shifted_340) > len(shifted_300)      # ... by -n, not at 256
    assert chat("keep=4,discard=100", 200) == chat(None, 200)
