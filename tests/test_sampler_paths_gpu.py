"""topp_sample_kernel (csrc/q4_sampling.hip) on distributions with holes -- a few, a few hundred or a few thousand finite logits, -inf everywhere
else: what top-k, typical-p, top-n-sigma and a guide hand the sampler -- at sixteen vocabulary sizes (E = ceil(n / 1024) from 1 to 126, both sides of
every threshold between two forms, and Llama-3's 128256 with every finite logit at an id beyond 16 bits), token for token against the restatement (oracle/q4_oracle.c orc_sample_topp) with the same coin stream.
tests/sampler_paths_ref.py crafts the inputs and names the branch each should take (inferred from restated probabilities, not observed on the device);
tests/test_sampler_paths_host.py holds every reachable branch to at least eight of these trials. Then the same supports inside captured sampled
steps: top_k of 1 .. 3000 through the real step, every token against the restated sampler over the reference's processed logits."""
import ctypes as C

import numpy as np
import pytest

import sampler_paths_ref as ref
import teacher_forced
from llama_cu_awq_amd import synth

pytestmark = pytest.mark.gpu

SEED = 99                                                        # test_sampler_paths_host.py's: the census counts these very coins


class SamplerStruct(C.Structure):
    """Sampler of include/llama2_q4.h: the three samplers of a size (one per setting) are handed ONE coin stream through rng_state"""
    _fields_ = [("vocab_size", C.c_int), ("indices", C.c_void_p), ("tempStorage_scan", C.c_void_p), ("tempStorage_sort", C.c_void_p),
                ("temp_storage_bytes_scan", C.c_size_t), ("temp_storage_bytes_sort", C.c_size_t), ("temperature", C.c_float), ("topp", C.c_float),
                ("rng_state", C.c_ulonglong)]


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    d = tmp_path_factory.mktemp("paths")
    out = {}
    for name in ("small", "v32k"):
        out[name] = str(d / (name + ".bin"))
        synth.write_model(out[name], name, seed=5)
    # v128k's body with eight more vocabulary rows: its logits buffer and embedding table hold the largest size, 128259, and every id below it
    out["host"] = str(d / "host.bin")
    synth.write_model(out["host"], synth.GEOMETRIES["v128k"][:5] + (128264,) + synth.GEOMETRIES["v128k"][6:], seed=5)
    return out


@pytest.fixture(scope="module")
def host(q4, paths):
    """one model whose logits buffer holds every size: q4_sample reads the SAMPLER's vocab_size, and the kernel writes logits[0 .. n)"""
    t = q4.Transformer(paths["host"])
    assert t.config.vocab_size >= max(ref.SIZES)
    yield t
    t.close()


@pytest.mark.parametrize("n", ref.SIZES)
def test_sampler_matches_the_restatement_on_every_branch(q4, orc, host, n):
    L, t = q4.lib(), host
    assert n <= t.config.vocab_size
    samplers = {}
    for T, topp in ref.SETTINGS:
        samplers[(T, topp)] = L.q4_sampler_new(n, T, topp, SEED)
        assert samplers[(T, topp)]
    state = C.c_ulonglong(SEED)
    bad, labels = [], {}
    try:
        for name, x, T, topp, coin_range in ref.trials(n):
            smp = samplers[(T, topp)]
            before, coin = ref.next_coin(L.random_f32, state, coin_range)      # (an aimed trial skips to the stream's next coin inside its range)
            C.cast(smp, C.POINTER(SamplerStruct)).contents.rng_state = before
            t.reset([1])
            q4.check(L.q4_memcpy_h2d(t.state.contents.logits, x.ctypes.data, x.nbytes))
            q4.check(L.q4_sample(smp, t.state, 1))
            q4.synchronize()
            assert C.cast(smp, C.POINTER(SamplerStruct)).contents.rng_state == state.value      # the sampler drew that coin
            want = orc.lib().orc_sample_topp(orc.f16_bits(x.copy()), n, T, topp, coin)
            assert t.pos() == 1
            got = int(t.token(1))
            label = ref.classify(x, n, T, topp, coin)
            labels[label] = labels.get(label, 0) + 1
            assert want >= ref.low_id(n), name                   # (sizes beyond 16 bits of id: the restatement's token lies there)
            if got != want or not np.isfinite(np.float32(x[got])):      # (a -inf logit has probability 0: never the sample)
                bad.append("%s [%s] coin %.9g: token %d, restatement %d" % (name, label, coin, got, want))
    finally:
        q4.synchronize()
        for smp in samplers.values():                            # (before the model goes: the samplers hold device memory of their own)
            L.q4_sampler_delete(smp)
    print("n %d: %s" % (n, dict(sorted(labels.items()))))
    assert not bad, "n %d: %d of %d trials differ: %s" % (n, len(bad), sum(labels.values()), "; ".join(bad[:8]))


@pytest.mark.parametrize("n,topp,supports", ref.FALLBACK)
def test_no_prefix_reaches_the_threshold(q4, orc, host, n, topp, supports):
    """a coin of 0.9999 over equal entries whose fp16 total stays below it: the search falls back to the last entry with a probability above 0 (the
    unsorted scan, the sorted scan on chip, the passes through global memory), never to a -inf logit at n - 1"""
    L, t = q4.lib(), host
    smp = L.q4_sampler_new(n, 1.0, topp, 1)
    assert smp
    try:
        for k in supports:
            x, last = ref.fallback_case(n, k)
            state = C.c_ulonglong(ref.FALLBACK_STATE)
            C.cast(smp, C.POINTER(SamplerStruct)).contents.rng_state = state.value
            t.reset([1])
            q4.check(L.q4_memcpy_h2d(t.state.contents.logits, x.ctypes.data, x.nbytes))
            q4.check(L.q4_sample(smp, t.state, 1))
            q4.synchronize()
            coin = L.random_f32(C.byref(state))
            assert coin > 0.9999
            want = orc.lib().orc_sample_topp(orc.f16_bits(x.copy()), n, 1.0, topp, coin)
            assert int(t.token(1)) == want == last, "n %d topp %g, %d equal entries: token %d, restatement %d, the last entry %d" % (
                n, topp, k, int(t.token(1)), want, last)
    finally:
        q4.synchronize()
        L.q4_sampler_delete(smp)


PROMPT = [1, 5, 9]
SAMPLED = (0.8, 0.9)
STEP_SEED = 4242
GENERATED = 12


@pytest.mark.parametrize("name", ["small", "v32k"])
def test_captured_sampled_steps_on_top_k_supports(q4, orc, paths, name):
    """top_k = k leaves exactly k finite logits (ties at the k-th value aside) in front of the sampler inside the captured step: every generated
    token is the restated sampler's over sampling_controls_ref.process of the teacher-forced raw logits"""
    steps = len(PROMPT) - 1 + GENERATED
    ran = 0
    for k in (1, 2, 65, 1025, 1500, 3000):
        t = q4.Transformer(paths[name], temperature=SAMPLED[0], topp=SAMPLED[1], seed=STEP_SEED, sampling=dict(top_k=k))
        if k > t.config.vocab_size:
            t.close()
            continue
        toks = t.generate_ids(PROMPT, steps)[0].copy()
        t.close()
        assert len(toks) == steps + 1, "top_k %d: the run stopped at an EOS: pick another seed" % k
        raw = teacher_forced.raw_logits(q4, paths[name], toks)
        want = teacher_forced.predict(q4, orc, raw, toks, len(PROMPT), dict(top_k=k), None, "sampled", STEP_SEED, SAMPLED)
        diff = np.nonzero(want != toks)[0]
        assert diff.size == 0, "%s top_k %d: %d tokens differ, first at ring index %d: %d, reference %d" % (name, k, diff.size, diff[0], toks[diff[0]],
                                                                                                           want[diff[0]])
        ran += 1
    assert ran == (3 if name == "small" else 6)
