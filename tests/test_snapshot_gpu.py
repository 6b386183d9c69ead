"""Sequence snapshots and prompt-prefix reuse on synthetic models: a resumed or restored run against the full run, BIT FOR BIT -- nothing in the decode
step changes, so tokens, logits, K / V rows, guide states and log-probability records are compared for equality, without a tolerance."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from llama_cu_awq_amd import guide, synth

pytestmark = pytest.mark.gpu
ERR_ARG = 5
EXE = os.path.join(ROOT, "llama_cu_awq_amd", "bin", "llama2_q4")
TOK = os.path.join(GOLDEN, "tokenizer.bin")

# model: (prompt length, steps). head64_long's prompt crosses the 128-position graph bin and reaches the split-context forms past 512
SHAPES = {"tiny_gqa": (20, 40), "small": (140, 160), "head64_long": (540, 560)}
SEED = 4242


class SamplerStruct(C.Structure):      # include/llama2_q4.h Sampler
    _fields_ = [("vocab_size", C.c_int), ("indices", C.c_void_p), ("scan", C.c_void_p), ("sort", C.c_void_p), ("bytes_scan", C.c_size_t),
                ("bytes_sort", C.c_size_t), ("temperature", C.c_float), ("topp", C.c_float), ("rng_state", C.c_ulonglong)]


def next_u32(q4, t):
    s = C.cast(t.sampler, C.POINTER(SamplerStruct)).contents
    state = C.c_ulonglong(s.rng_state)       # (a copy: the sampler itself stays where it is)
    return q4.lib().random_u32(C.byref(state))


def prompt_of(name, length=None, salt=0):
    vocab = synth.geometry(name)[5]
    rng = np.random.default_rng(1000 + salt)
    p = rng.integers(3, vocab, length or SHAPES[name][0], dtype=np.int32)
    p[0] = 1
    return p


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("snap")
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


def rows_of(t, last):
    """K and V at the first, a middle and the last position of every layer"""
    out = []
    for layer in range(t.config.n_layers):
        for pos in (0, last // 2, last):
            out.extend(t.kv_row(layer, pos))
    return np.stack(out)


_FULL = {}


def full_run(q4, files, name, kv="fp16"):
    """run A: a fresh model's generate_ids -- computed once per (model, format), shared, never modified"""
    key = (name, kv)
    if key not in _FULL:
        P, S = prompt_of(name), SHAPES[name][1]
        t = q4.Transformer(files(name), kv=kv)
        toks = t.generate_ids(P, S)[0].copy()
        _FULL[key] = {"P": P, "S": S, "tokens": toks, "logits": t.logits(), "rows": rows_of(t, S - 1)}
        for v in _FULL[key].values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        t.close()
    return _FULL[key]


def ingest(t, P, n):
    """positions [0, n) from P[:n], nothing else"""
    t.generate_ids(P[:n], n)
    assert t.pos() == n


def overwrite(t, name, n):
    """an unrelated sequence longer than n (a guided one may stop at its EOS before all its steps): the rows of the prefix are gone"""
    t.generate_ids(prompt_of(name, length=8, salt=77), min(n + 9, t.config.seq_len))
    assert t.pos() > n


def resumed_run(q4, files, name, n, kv="fp16", serialise=False):
    A = full_run(q4, files, name, kv)
    P, S = A["P"], A["S"]
    t = q4.Transformer(files(name), kv=kv)
    try:
        ingest(t, P, n)
        snap = t.snapshot(n)
        assert snap.n_pos == n and np.array_equal(snap.tokens, P[:n])
        if serialise:
            blob = snap.to_bytes()
            assert len(blob) == snap.info["export_bytes"] and q4.snapshot_check(blob)["n_pos"] == n
            snap.close()
            snap = q4.Snapshot.from_bytes(blob)
            assert np.array_equal(snap.tokens, P[:n]) and snap.nbytes == snap.info["device_bytes"]
        before = rows_of(t, n - 1)
        overwrite(t, name, n)
        assert not np.array_equal(rows_of(t, n - 1), before) or n == 1      # (position 0 of two sequences that both begin with BOS holds the same rows)
        t.restore(snap)
        assert np.array_equal(rows_of(t, n - 1), before)
        toks = t.generate_ids_from(P, S, n)[0]
        assert np.array_equal(toks, A["tokens"])
        assert np.array_equal(t.logits().view(np.uint16), A["logits"].view(np.uint16))
        assert np.array_equal(rows_of(t, S - 1).view(np.uint16), A["rows"].view(np.uint16))
        snap.close()
    finally:
        t.close()


CASES = [("tiny_gqa", 1), ("tiny_gqa", 19), ("small", 1), ("small", 127), ("small", 128), ("small", 129), ("small", 139),
         ("head64_long", 1), ("head64_long", 127), ("head64_long", 128), ("head64_long", 129), ("head64_long", 520), ("head64_long", 539)]


@pytest.mark.parametrize("name, n", CASES)
def test_resume_from_a_restored_snapshot_equals_the_full_run(q4, files, name, n):
    assert n <= SHAPES[name][0] - 1
    resumed_run(q4, files, name, n)


@pytest.mark.parametrize("n", [129, 520])
def test_the_same_on_an_fp8_cache(q4, files, n):
    """bytes and exponents through kv_row (the dequantised halves: byte * 2^e), and the logits"""
    resumed_run(q4, files, "head64_long", n, kv="fp8")


def test_a_serialised_snapshot_restores_the_same_rows(q4, files):
    resumed_run(q4, files, "small", 100, serialise=True)
    resumed_run(q4, files, "head64_long", 130, kv="fp8", serialise=True)


def test_start_pos_at_the_prompts_length_is_an_argument_error(q4, files):
    P = prompt_of("small")
    t = q4.Transformer(files("small"))
    ingest(t, P, 10)
    with pytest.raises(q4.Q4Error, match="start_pos"):
        t.generate_ids_from(P, 160, len(P))
    L = q4.lib()
    assert L.q4_resume_sequence(t.state, P.ctypes.data, len(P), len(P)) == ERR_ARG
    assert L.q4_resume_sequence(t.state, P.ctypes.data, len(P), -1) == ERR_ARG
    assert L.q4_resume_sequence(t.state, P.ctypes.data, 0, 0) == ERR_ARG
    assert t.pos() == 10                                                         # a refused call moves nothing
    long = prompt_of("small", length=400)
    assert L.q4_resume_sequence(t.state, long.ctypes.data, len(long), 321) == ERR_ARG      # above seq_len (320)
    t.close()


# ---- step features across a resume (model small) -----------------------------------------------------------------------------------------------------
def _feature_pair(q4, files, n, P, S, **kw):
    """(A's model after its full run, B's after restore + resume), both fresh with the same settings; B's rows come from a third model's snapshot, so
    that B's sampler stands at its seed as A's did"""
    a = q4.Transformer(files("small"), **kw)
    ta = a.generate_ids(P, S)[0].copy()
    c = q4.Transformer(files("small"), **kw)
    ingest(c, P, n)
    snap = c.snapshot(n)
    c.close()
    b = q4.Transformer(files("small"), **kw)
    b.restore(snap)
    tb = b.generate_ids_from(P, S, n)[0].copy()
    snap.close()
    return a, ta, b, tb


def test_sampled_generation_across_a_resume(q4, files):
    P = prompt_of("small", length=40)
    a, ta, b, tb = _feature_pair(q4, files, 30, P, 80, temperature=0.8, topp=0.9, seed=12345)
    assert np.array_equal(ta, tb) and len(ta) > 41         # (sampled tokens were generated)
    assert next_u32(q4, a) == next_u32(q4, b)              # a reused Sampler stands at the same state
    a.close()
    b.close()


def test_penalty_window_reaches_below_the_resumed_position(q4, files):
    P = prompt_of("small", length=40)
    P[5:35] = P[5]                                         # a token the window counts many times, all of them below start_pos
    kw = dict(sampling=dict(repeat_penalty=1.3, frequency_penalty=0.2, penalty_last_n=64))
    a, ta, b, tb = _feature_pair(q4, files, 36, P, 60, **kw)      # 20 generated tokens, a window of 64
    plain = q4.Transformer(files("small"))
    assert not np.array_equal(plain.generate_ids(P, 60)[0], ta)   # (the penalties do decide tokens here)
    assert np.array_equal(ta, tb)
    for t in (a, b, plain):
        t.close()


def test_guide_across_a_resume(q4, files):
    vocab = synth.geometry("small")[5]
    table = guide.from_choices([[11, 12, 13, 14, 15, 16, 17, 18, 19, 20], [11, 12, 21, 22, 23, 24, 25, 26, 27, 28]], vocab)
    P = prompt_of("small", length=24)
    g1, g2 = q4.Guide(table), q4.Guide(table)
    a = q4.Transformer(files("small"), guide=g1)
    ta = a.generate_ids(P, 60)[0].copy()
    n_run = len(ta) - 1
    assert ta[-1] == 2 and n_run == 24 + 10                # the choice, then EOS
    b = q4.Transformer(files("small"), guide=g2)
    ingest(b, P, 17)
    snap = b.snapshot(17)
    overwrite(b, "small", 17)
    b.restore(snap)
    tb = b.generate_ids_from(P, 60, 17)[0]
    assert np.array_equal(ta, tb)
    sa, sb = a.guide_states(17, n_run - 17), b.guide_states(17, n_run - 17)
    assert np.array_equal(sa, sb) and (sa[: 23 - 17] == q4.GUIDE_NONE).all() and sa[23 - 17] == 0
    snap.close()
    a.close()
    b.close()
    g1.close()
    g2.close()


def test_logprob_records_across_a_resume(q4, files):
    P = prompt_of("small", length=40)
    a, ta, b, tb = _feature_pair(q4, files, 29, P, 70, logprobs=5)
    assert np.array_equal(ta, tb)
    for x, y in zip(a.logprobs(29, 70 - 29), b.logprobs(29, 70 - 29)):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    a.close()
    b.close()


@pytest.mark.parametrize("mode", [0, 1])
def test_graph_forms(q4, files, mode):
    """eager steps and captured graphs; the resumed run's groups of eight start at positions that are no multiple of eight"""
    L = q4.lib()
    P = prompt_of("small", length=60)
    L.q4_set_use_graphs(mode)
    try:
        a = q4.Transformer(files("small"))
        ta = a.generate_ids(P, 150)[0].copy()
        la, ra = a.logits(), rows_of(a, 149)
        a.close()
        b = q4.Transformer(files("small"))
        ingest(b, P, 13)
        snap = b.snapshot(13)
        overwrite(b, "small", 13)
        b.restore(snap)
        tb = b.generate_ids_from(P, 150, 13)[0]
        assert np.array_equal(ta, tb)
        assert np.array_equal(la.view(np.uint16), b.logits().view(np.uint16)) and np.array_equal(ra.view(np.uint16), rows_of(b, 149).view(np.uint16))
        snap.close()
        b.close()
    finally:
        L.q4_set_use_graphs(1)


# ---- restoring elsewhere -------------------------------------------------------------------------------------------------------------------------------
def test_restore_into_a_second_live_model_of_the_same_file(q4, files):
    A = full_run(q4, files, "small")
    P, S = A["P"], A["S"]
    src, dst = q4.Transformer(files("small")), q4.Transformer(files("small"))
    ingest(src, P, 101)
    snap = src.snapshot()                                  # None: every completed position
    assert snap.n_pos == 101
    dst.restore(snap)
    assert np.array_equal(dst.generate_ids_from(P, S, 101)[0], A["tokens"])
    assert np.array_equal(dst.logits().view(np.uint16), A["logits"].view(np.uint16))
    assert np.array_equal(rows_of(dst, S - 1).view(np.uint16), A["rows"].view(np.uint16))
    assert np.array_equal(src.generate_ids(P, S, reuse=snap)[0], A["tokens"])     # restore + common prefix with the snapshot's tokens, in one call
    snap.close()
    src.close()
    dst.close()


def test_restore_into_a_model_with_another_seq_len(q4, files):
    """the same tensors from the same seed behind a header with another seq_len: the same checkpoint to a snapshot"""
    P, S = prompt_of("small"), SHAPES["small"][1]
    src, dst = q4.Transformer(files("small")), q4.Transformer(files("small", seq_len=400))
    fresh = q4.Transformer(files("small", seq_len=400))
    want = fresh.generate_ids(P, S)[0].copy()
    ingest(src, P, 90)
    snap = src.snapshot(90)
    dst.restore(snap)
    for layer in range(dst.config.n_layers):
        for pos in (0, 45, 89):
            for x, y in zip(src.kv_row(layer, pos), dst.kv_row(layer, pos)):
                assert np.array_equal(x.view(np.uint16), y.view(np.uint16))
    assert np.array_equal(dst.generate_ids_from(P, S, 90)[0], want)
    assert np.array_equal(dst.logits().view(np.uint16), fresh.logits().view(np.uint16))
    assert np.array_equal(rows_of(dst, S - 1).view(np.uint16), rows_of(fresh, S - 1).view(np.uint16))
    snap.close()
    for t in (src, dst, fresh):
        t.close()


def test_refusals(q4, files):
    P = prompt_of("head64_long")
    src = q4.Transformer(files("head64_long"))
    ingest(src, P, 100)
    snap = src.snapshot(100)
    for n in (0, -1, 101, 5000):                           # beyond the completed positions (or none)
        with pytest.raises(q4.Q4Error, match="status 5"):
            src.snapshot(n)
    other_seed = q4.Transformer(files("head64_long", seed=SEED + 1))
    fp8 = q4.Transformer(files("head64_long"), kv="fp8")
    short = q4.Transformer(files("head64_long", seq_len=64))
    for what, t in (("fingerprint", other_seed), ("fp16 into fp8", fp8), ("n_pos beyond seq_len", short)):
        k0 = t.kv_row(0, 0)[0].copy()
        with pytest.raises(q4.Q4Error, match="status 5"):
            t.restore(snap)
        assert np.array_equal(t.kv_row(0, 0)[0], k0), what
    ingest(fp8, P, 50)
    snap8 = fp8.snapshot(50)
    assert snap8.info["kv_format"] == q4.KV_FP8 and snap8.nbytes < snap.nbytes
    with pytest.raises(q4.Q4Error, match="status 5"):
        src.restore(snap8)                                 # fp8 into fp16
    small = q4.Transformer(files("small"))
    with pytest.raises(q4.Q4Error, match="status 5"):
        small.restore(snap)                                # another geometry
    for s in (snap, snap8):
        s.close()
    for t in (src, other_seed, fp8, short, small):
        t.close()


# ---- in-place reuse ------------------------------------------------------------------------------------------------------------------------------------
def test_common_prefix_and_reuse_in_place(q4, files):
    name, S = "small", 90
    P1 = prompt_of(name, length=50)
    t = q4.Transformer(files(name))
    toks1 = t.generate_ids(P1, S)[0].copy()
    nothing = P1.copy()
    nothing[0] = 7                                         # shares no token
    k = 33
    partly = np.concatenate([P1[:k], prompt_of(name, length=30, salt=5)[1:]])
    assert partly[k] != P1[k]
    assert t.common_prefix(nothing) == 0
    assert t.common_prefix(partly) == k
    assert t.common_prefix(P1) == len(P1) - 1              # capped: the last prompt token always runs
    assert t.common_prefix(toks1) == S                     # ... and by the positions completed (S of the ring's S + 1 tokens)
    assert t.common_prefix(P1[:1]) == 0
    fresh = q4.Transformer(files(name))
    want = fresh.generate_ids(partly, S)[0].copy()
    got, _, timed, _ = t.generate_ids(partly, S, reuse=True)
    assert np.array_equal(got, want) and timed == S - 1 - k
    assert np.array_equal(t.logits().view(np.uint16), fresh.logits().view(np.uint16))
    assert np.array_equal(rows_of(t, S - 1).view(np.uint16), rows_of(fresh, S - 1).view(np.uint16))
    t.reset(P1)
    assert t.common_prefix(P1) == 0                        # a reset model has completed nothing
    t.close()
    fresh.close()


def test_roll_back_reproduces_the_continuation(q4, files):
    name, S = "small", 70
    P1 = prompt_of(name, length=30)
    t = q4.Transformer(files(name))
    toks = t.generate_ids(P1, S)[0].copy()
    final = t.logits()
    for start, prompt in ((12, P1), (45, toks[:46])):      # into the prompt; into the answer (regenerate from its 16th token on)
        t.resume(prompt, start)
        assert t.pos() == start
        for pos in range(start, S):
            t.run_transformer(pos >= len(prompt) - 1)
            q4.synchronize()
        assert [t.token(i) for i in range(S + 1)] == toks.tolist()
        assert np.array_equal(t.logits().view(np.uint16), final.view(np.uint16))
    t.close()


# ---- the CLI -------------------------------------------------------------------------------------------------------------------------------------------
def _cli(model, cache, extra=()):
    env = dict(os.environ)
    env.pop("Q4_PROMPT_CACHE", None)
    if cache:
        env["Q4_PROMPT_CACHE"] = cache
    args = [EXE, model, "-n", "48", "-i", "write an essay about GPUs and the memory they stream", "-z", TOK] + list(extra)
    r = subprocess.run(args, capture_output=True, text=True, timeout=300, errors="replace", env=env)
    assert r.returncode == 0, r.stderr
    m = re.search(r"achieved tok/s: [0-9.infa-]+\. Tokens: (-?\d+), seconds: [0-9.e+-]+", r.stdout)
    assert m, r.stdout
    return re.sub(r"achieved tok/s.*", "", r.stdout), int(m.group(1)), r.stderr


@pytest.fixture(scope="module")
def cli_model(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("snapcli") / "cli.bin")
    synth.write_model(p, (256, 352, 2, 4, 4, 32000, 256, 10000.0), seed=31)
    return p


@pytest.mark.parametrize("extra", [("-t", "0"), ("-t", "0.7", "-s", "42")], ids=["greedy", "sampled"])
def test_cli_prompt_cache(cli_model, tmp_path, extra):
    cache = str(tmp_path / "prompt.q4snap")
    plain, steps_plain, _ = _cli(cli_model, None, extra)
    first, steps_first, _ = _cli(cli_model, cache, extra)
    assert os.path.exists(cache) and steps_first == steps_plain == 47
    size = os.path.getsize(cache)
    second, steps_second, _ = _cli(cli_model, cache, extra)
    assert plain == first == second
    assert 0 < steps_second < steps_plain                  # the prompt's positions but the last were not run
    assert os.path.getsize(cache) == size                  # ... and the file already covered them


def test_cli_ignores_a_file_that_fails_the_check(cli_model, tmp_path):
    cache = str(tmp_path / "junk.q4snap")
    open(cache, "wb").write(b"Q4SN" + bytes(100))
    plain, steps_plain, _ = _cli(cli_model, None, ("-t", "0"))
    out, steps, err = _cli(cli_model, cache, ("-t", "0"))
    assert out == plain and steps == steps_plain
    assert "Q4_PROMPT_CACHE" in err and "ignored" in err
    from llama_cu_awq_amd import api
    assert api.snapshot_check(open(cache, "rb").read())["n_pos"] >= 2       # replaced by a good one
