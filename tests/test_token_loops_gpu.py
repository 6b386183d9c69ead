"""The library's two generate drivers walk one token loop: what the CLI (q4_generate) prints is what generate_ids (q4_generate_ids_from) leaves in
the ring -- below the wall, across two context shifts and from a resumed start, greedy and sampled -- with the same `Tokens:` count, and the loop
leaves the sampler's xorshift stream at one draw per step (llama2_q4.cu:436-492, sampler.h:45). Written against the loops as they stood when each
driver had its own copy: every assertion here held there.

Comparisons other files already make, not repeated here: an EOS inside the PROMPT rewinds the surplus draws of its group
(test_forward_gpu::test_sampler_rng_after_an_early_stop_matches_one_draw_per_executed_step); a resumed sampled generate_ids_from equals the full
run and leaves the sampler where the full run does (test_snapshot_gpu::test_sampled_generation_across_a_resume); the CLI's text with a prompt cache
equals its text without (test_snapshot_gpu::test_cli_prompt_cache); generate_ids across the wall equals the shifts made by hand
(test_context_shift_gpu::test_generate_ids_equals_the_composition_by_hand)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from llama_cu_awq_amd import guide, synth

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "llama_cu_awq_amd", "bin", "llama2_q4")
TOK = os.path.join(GOLDEN, "tokenizer.bin")
GEOMETRY = (256, 352, 2, 4, 4, 32000, 256, 10000.0)          # test_cli_gpu.py's
TEXT = "write an essay about GPUs"
IDS = [1, 2436, 385, 3686, 388, 1048, 22796, 118]            # TEXT as the CLI encodes it
SEED = 42
MODES = {"greedy": (0.0, ["-t", "0"]), "sampled": (0.5, ["-t", "0.5", "-p", "0.6", "-s", str(SEED)])}


class SamplerStruct(C.Structure):      # include/llama2_q4.h Sampler
    _fields_ = [("vocab_size", C.c_int), ("indices", C.c_void_p), ("scan", C.c_void_p), ("sort", C.c_void_p), ("bytes_scan", C.c_size_t),
                ("bytes_sort", C.c_size_t), ("temperature", C.c_float), ("topp", C.c_float), ("rng_state", C.c_ulonglong)]


def sampler_of(t):
    return C.cast(t.sampler, C.POINTER(SamplerStruct)).contents


def advanced(state, draws):
    """sampler.h:31-37, the state after `draws` coins"""
    for _ in range(draws):
        state ^= state >> 12
        state = (state ^ (state << 25)) & 0xFFFFFFFFFFFFFFFF
        state ^= state >> 27
    return state


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("loops") / "cli.bin")
    synth.write_model(p, GEOMETRY, seed=31)
    return p


@pytest.fixture(scope="module")
def tok(q4):
    t = q4.Tokenizer(TOK, GEOMETRY[5])
    assert t.encode(TEXT) == IDS
    yield t
    t.close()


def cli(model, n, mode, env=()):
    """(stdout between the prompt's encoding and the throughput line, the line's Tokens)"""
    e = {k: v for k, v in os.environ.items() if k not in ("Q4_CONTEXT_SHIFT", "Q4_PROMPT_CACHE")}
    e.update(env)
    r = subprocess.run([EXE, model, "-n", str(n), "-i", TEXT, "-z", TOK] + MODES[mode][1], capture_output=True, timeout=300, env=e)
    assert r.returncode == 0, r.stderr
    m = re.search(rb"Encoding Prompt\.\.\. Done!\n(.*)achieved tok/s: [0-9.infa-]+\. Tokens: (-?\d+), seconds: [0-9.e+-]+\n", r.stdout, re.S)
    assert m, r.stdout
    return m.group(1), int(m.group(2))


def printed(tok, ring, steps):
    """what generate() prints for a ring: the piece of every token the loop looks at -- ring[1 .. pos], pos < steps -- behind its predecessor, through
    safe_printf's filter (tokenizer.h:81-93: a one-byte piece that is neither printable nor white space is dropped), then the two newlines that
    close the text and open the throughput line"""
    vocab, out, prev = GEOMETRY[5], b"", int(ring[0])
    for nxt in ring[1:steps]:
        nxt = int(nxt) if nxt < vocab else 0                   # llama2_q4.cu:474
        piece = tok.decode(prev, nxt)
        if len(piece) > 1 or (len(piece) == 1 and (0x20 <= piece[0] <= 0x7e or piece[0] in b"\t\n\v\f\r")):
            out += piece
        prev = nxt
    return out + b"\n\n"


def transformer(q4, model, mode, **kw):
    return q4.Transformer(model, temperature=MODES[mode][0], topp=0.6, seed=SEED, **kw)


@pytest.mark.parametrize("mode", sorted(MODES))
def test_cli_text_is_the_ids_loops_ring(q4, model, tok, mode):
    text, n_tokens = cli(model, 40, mode)
    t = transformer(q4, model, mode)
    ring, _, timed, _ = t.generate_ids(IDS, 40)
    assert len(ring) == 41 and timed == n_tokens == 39
    assert text == printed(tok, ring, 40)
    t.close()


@pytest.mark.parametrize("mode", sorted(MODES))
def test_the_same_across_the_wall(q4, model, tok, mode):
    """256 positions, (keep, discard) = (4, 64), 330 steps: the wall is met at steps 256 and 320, and the last ten steps run at positions 192 .. 201 of
    the slid rows, a group of Q4_MULTI_STEPS and two steps alone"""
    text, n_tokens = cli(model, 330, mode, {"Q4_CONTEXT_SHIFT": "keep=4,discard=64"})
    t = transformer(q4, model, mode, context_shift=(4, 64))
    ring, _, timed, _ = t.generate_ids(IDS, 330)
    assert len(ring) == 331 and timed == n_tokens == 329 and t.pos() == 330 - 2 * 64
    assert text == printed(tok, ring, 330)
    t.close()


@pytest.mark.parametrize("mode", sorted(MODES))
def test_the_same_from_a_resumed_start(q4, model, tok, mode, tmp_path):
    """The CLI's second run with one prompt cache skips the prompt's positions but the last; so does generate_ids_from at n_prompt - 1 over the rows a
    run of the same prompt left. Both burn the skipped steps' coins: sampled, the text is the full run's."""
    env = {"Q4_PROMPT_CACHE": str(tmp_path / "prompt.q4snap")}
    first, n_first = cli(model, 40, mode, env)
    second, n_second = cli(model, 40, mode, env)
    t = transformer(q4, model, mode)
    full = t.generate_ids(IDS, 40)[0].copy()
    sampler_of(t).rng_state = SEED
    ring, _, timed, _ = t.generate_ids_from(IDS, 40, len(IDS) - 1)
    assert np.array_equal(ring, full)                         # (the rows were in place)
    assert n_first == 39 and timed == n_second == 39 - (len(IDS) - 1)
    assert second == printed(tok, ring, 40) == first
    assert sampler_of(t).rng_state == advanced(SEED, 40)
    t.close()


def test_a_run_that_ends_at_steps_draws_one_coin_per_step(q4, model):
    """steps 0 .. 39 are queued, in groups of Q4_MULTI_STEPS and alone, each with one draw whether it samples or not"""
    t = transformer(q4, model, "sampled")
    ring, _, timed, _ = t.generate_ids(IDS, 40)
    assert timed == 39 and not (ring[1:] == 2).any()
    assert sampler_of(t).rng_state == advanced(SEED, 40)
    t.close()


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("n_prompt, in_group", [(8, 7), (124, 2)], ids=["group_end", "mid_group"])
def test_a_guided_stop_leaves_pos_plus_one_draws(q4, model, tok, mode, n_prompt, in_group):
    """A guide over one six-token choice forces EOS into ring[n_prompt + 6]: the loop stops at pos = n_prompt + 6 and the sampler stands at pos + 1
    draws, the reference's count (one per run_transformer call, steps 0 .. pos). Generating groups start at step n_prompt - 1, or at 128 where that
    is the next graph bin's first step: after 8 prompt tokens the stop is the last step of the group 7 .. 14 (no surplus draw to take back), after
    124 it is step 130 of the group 128 .. 135 (five of them)."""
    choice = tok.encode("yes, of course it is", 0, 0)
    assert len(choice) == 6
    prompt = np.random.default_rng(7).integers(3, GEOMETRY[5], n_prompt, dtype=np.int32)
    prompt[0] = 1
    g = q4.Guide(guide.from_choices([choice], GEOMETRY[5]))
    t = transformer(q4, model, mode, guide=g)
    ring, _, timed, _ = t.generate_ids(prompt, 200)
    pos = timed + 1
    group_start = n_prompt - 1 if n_prompt - 1 + 8 <= 128 else 128
    assert pos == n_prompt + 6 and ring[pos] == 2 and ring[n_prompt:pos].tolist() == choice
    assert (pos - group_start) % 8 == in_group
    assert sampler_of(t).rng_state == advanced(SEED, pos + 1)
    t.close()
    g.close()
