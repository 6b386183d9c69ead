"""The opt-in FP8 (e4m3) K / V cache on the GPU: the attention kernels of csrc/attention_kv8.h against the oracle's attention over the
round-tripped cache, the append (bytes and exponents exactly the numpy quantiser's, nothing else touched), the network at every
fusion level against a forward composed from the oracle's ops with the round trip on, the split-context forms inside the network,
and the runtime around it (alternating formats, the untouched fp16 path, unsupported head sizes, the CLI)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import kv8_ref
from conftest import GOLDEN, ROOT
from llama_cu_awq_amd import synth
from test_forward_gpu import BOUND
from test_ops_gpu import _attention_close

pytestmark = pytest.mark.gpu
GUARD_BYTE, GUARD_EXP = 0xA5, 0x5A


@pytest.fixture(autouse=True)
def _format_back_to_fp16(q4):
    yield
    assert q4.lib().q4_get_kv_format() == q4.KV_FP16, "a test left the process-wide K / V format at FP8"


def _trait_row(trait, hs, rng):
    x = rng.standard_normal(hs).astype(np.float32)
    if trait == "zero":
        x[:] = 0.0
    elif trait == "saturating":
        x[int(rng.integers(hs))] = 60000.0            # amax > 57344: saturates at 448 * 2^7
    elif trait == "subnormal":
        x = rng.integers(-1023, 1024, size=hs).astype(np.float32) * np.float32(2.0 ** -24)
    elif trait == "outlier":
        x[int(rng.integers(hs))] = -300.0 if rng.integers(2) else 300.0
    return x.astype(np.float16)


def _kernel_case(q4, orc, rng, heads, kv_mul, hs, pos, seq, split, traits=None):
    """One launch of q4_multi_head_attention_kv8 on caches whose rows below `pos` hold quantised random rows and whose other bytes hold
    guard patterns. Checks the append exactly; returns (output, reference over the round-tripped cache, reference over the fp16 cache)."""
    L = q4.lib()
    n_kv, dim = heads // kv_mul, heads * hs
    kv_dim = n_kv * hs
    bin_ = seq
    q = rng.standard_normal(dim).astype(np.float16)
    kc = rng.standard_normal((bin_, kv_dim)).astype(np.float16)
    vc = rng.standard_normal((bin_, kv_dim)).astype(np.float16)
    if traits:
        for h in range(n_kv):
            kc[pos, h * hs:(h + 1) * hs] = _trait_row(traits[h % len(traits)], hs, rng)
            vc[pos, h * hs:(h + 1) * hs] = _trait_row(traits[(h + 1) % len(traits)], hs, rng)
    kb, ke = kv8_ref.quantise(kc, hs)                   # [bin, kv_dim], [bin, n_kv]
    vb, ve = kv8_ref.quantise(vc, hs)
    k_rt, v_rt = kv8_ref.dequantise(kb, ke, hs), kv8_ref.dequantise(vb, ve, hs)
    ref, _ = orc.attention(q, k_rt.reshape(-1), v_rt.reshape(-1), heads, hs, kv_mul, pos, max_seq_len=bin_)
    ref16, _ = orc.attention(q, kc.reshape(-1), vc.reshape(-1), heads, hs, kv_mul, pos, max_seq_len=bin_)

    def device_image(b, e):
        bytes_ = np.full((bin_, kv_dim), GUARD_BYTE, dtype=np.uint8)
        exps = np.full((n_kv, bin_), GUARD_EXP, dtype=np.int8)
        bytes_[:pos] = b[:pos]
        exps[:, :pos] = e[:pos].T
        return bytes_, exps

    k_img, ke_img = device_image(kb, ke)
    v_img, ve_img = device_image(vb, ve)
    dk, dv, dke, dve = q4.DevBuf(k_img), q4.DevBuf(v_img), q4.DevBuf(ke_img), q4.DevBuf(ve_img)
    dkr, dvr = q4.DevBuf(kc[pos]), q4.DevBuf(vc[pos])
    dq, do = q4.DevBuf(q), q4.DevBuf(nbytes=dim * 2)
    dpos = q4.DevBuf(np.array([pos], dtype=np.int32))
    att = q4.DevBuf(nbytes=heads * bin_ * 8) if split else None      # (the entry's contract: 8 bytes per head and position)
    q4.check(L.q4_multi_head_attention_kv8(do.ptr, dq.ptr, dk.ptr, dv.ptr, dke.ptr, dve.ptr, dkr.ptr, dvr.ptr, att.ptr if att else None,
                                           heads, hs, kv_mul, bin_, dpos.ptr))
    q4.synchronize()
    got = do.get(np.float16, dim)
    # ---- the append: position `pos` holds exactly the numpy quantiser's bytes and exponents, every other byte is untouched
    for name, dev, img, b, dexp, eimg, e in (("K", dk, k_img, kb, dke, ke_img, ke), ("V", dv, v_img, vb, dve, ve_img, ve)):
        want = img.copy()
        want[pos] = b[pos]
        have = dev.get(np.uint8, bin_ * kv_dim).reshape(bin_, kv_dim)
        assert np.array_equal(have[pos], want[pos]), "%s bytes at the position differ from the quantiser's: %d of %d" % (name, int((have[pos] != want[pos]).sum()), kv_dim)
        assert np.array_equal(have, want), "%s bytes away from the position were written" % name
        want_e = eimg.copy()
        want_e[:, pos] = e[pos]
        have_e = dexp.get(np.int8, n_kv * bin_).reshape(n_kv, bin_)
        assert np.array_equal(have_e[:, pos], want_e[:, pos]), "%s exponents %s, the quantiser's %s" % (name, have_e[:, pos], want_e[:, pos])
        assert np.array_equal(have_e, want_e), "%s exponents away from the position were written" % name
    if split:       # the records of the split form lie in `att`: the launch did take that form
        assert att.get(np.uint8).any(), "the split-context form did not run"
    return got, ref, ref16


ONE_PASS = [(4, 1, 64, 0, 64), (8, 4, 64, 40, 128), (4, 1, 128, 127, 128), (4, 1, 128, 128, 256), (4, 2, 256, 9, 128)]
SPLIT = [(8, 1, 128, 2047, 2048), (8, 4, 64, 1000, 2048), (8, 2, 256, 1023, 1024),
         (8, 1, 128, 255, 1024), (8, 1, 128, 256, 1024), (8, 1, 128, 257, 1024),      # the current row as the last / first of a chunk
         (8, 2, 64, 255, 1024), (8, 2, 64, 256, 1024), (8, 2, 64, 257, 1024),         # ... of the 256-position chunks of a 64-wide head
         (8, 1, 128, 4000, 4096)]


def _closer_to_fp8(got, ref, ref16):
    """a kernel that read fp16 by mistake (or dropped the exponents) lands on the other reference"""
    g = got.astype(np.float64)
    d8, d16 = np.abs(g - ref.astype(np.float64)).sum(), np.abs(g - ref16.astype(np.float64)).sum()
    assert d8 < d16, (d8, d16)


@pytest.mark.parametrize("heads,kv_mul,hs,pos,seq", ONE_PASS)
def test_kernel_one_pass_and_append(q4, orc, rng, heads, kv_mul, hs, pos, seq):
    got, ref, ref16 = _kernel_case(q4, orc, rng, heads, kv_mul, hs, pos, seq, split=False)
    _attention_close(got, ref, frac_gt1=0.03)
    _closer_to_fp8(got, ref, ref16)


@pytest.mark.parametrize("heads,kv_mul,hs,pos,seq", SPLIT)
def test_kernel_split_context_and_append(q4, orc, rng, heads, kv_mul, hs, pos, seq):
    got, ref, ref16 = _kernel_case(q4, orc, rng, heads, kv_mul, hs, pos, seq, split=True)
    _attention_close(got, ref, frac_gt1=0.25)
    _closer_to_fp8(got, ref, ref16)


@pytest.mark.parametrize("heads,kv_mul,hs,pos,seq,split", [(8, 2, 64, 40, 128, False), (8, 1, 128, 77, 128, False), (4, 1, 256, 30, 128, False),
                                                            (8, 2, 64, 700, 1024, True), (8, 2, 128, 300, 1024, True)])
def test_append_of_hostile_rows(q4, orc, rng, heads, kv_mul, hs, pos, seq, split):
    """The appended row of every kv head is a zero row, a row that saturates (amax 60000 -> 448 * 2^7), a row of fp16 subnormals or a row
    with one +-300 outlier: bytes and exponents exactly the quantiser's (checked inside), the hardware convert against torch's RNE."""
    got, ref, _ = _kernel_case(q4, orc, rng, heads, kv_mul, hs, pos, seq, split, traits=["zero", "saturating", "subnormal", "outlier"])
    _attention_close(got, ref, frac_gt1=0.25 if split else 0.03)


# ---- the network -------------------------------------------------------------------------------------------------------------------
NET_POSITIONS = 40
NET_BOUND = {"tiny": BOUND["tiny"], "head64_long": 5e-3}     # head64_long: the bound test_forward_gpu applies to it (test_split_context_merge_by_the_last_block)


def _tokens(n, vocab, seed=3):
    return [1] + [int(v) for v in np.random.default_rng(seed).integers(3, vocab, size=n - 1)]


@pytest.fixture(scope="module")
def net(tmp_path_factory):
    """per geometry: the checkpoint, the forced tokens and the composed forward's logits / layer-0 rows with the round trip on (computed once)"""
    d = tmp_path_factory.mktemp("kv8")
    out = {}
    for name in ("tiny", "head64_long"):
        path = str(d / (name + ".bin"))
        synth.write_model(path, name, seed=7)
        cfg = synth.geometry(name)
        toks = _tokens(NET_POSITIONS, cfg[5])
        f = kv8_ref.Forward(path, cfg, round_trip=True)
        logits = np.stack([f.forward(t, pos) for pos, t in enumerate(toks)])
        out[name] = {"path": path, "cfg": cfg, "toks": toks, "logits": logits}
    return out


def _forced_run(q4, path, toks, kv, positions=None):
    t = q4.Transformer(path, kv=kv)
    assert t.kv_format == kv and q4.lib().q4_kv_format_of(t.state) == q4.KV_FORMATS[kv]
    t.reset(toks)
    logits, rows = [], []
    for pos in range(len(toks) if positions is None else positions):
        t.run_transformer(False)
        q4.synchronize()
        logits.append(t.logits())
    for pos in range(len(logits)):
        rows.append(np.concatenate(t.kv_row(0, pos)))
    q4.check(q4.lib().q4_handoff_status(t.state))
    t.close()
    return np.stack(logits), np.stack(rows)


@pytest.mark.parametrize("name", ["tiny", "head64_long"])
@pytest.mark.parametrize("fusion,graphs", [(5, 1), (1, 1), (0, 1), (5, 0), (1, 0), (0, 0)])
def test_network_against_the_composed_forward(q4, net, observed, name, fusion, graphs):
    L = q4.lib()
    n = net[name]
    hs = n["cfg"][0] // n["cfg"][3]
    L.q4_set_fusion(fusion)
    L.q4_set_use_graphs(graphs)
    try:
        l16, r16 = _forced_run(q4, n["path"], n["toks"], "fp16")
        l8, r8 = _forced_run(q4, n["path"], n["toks"], "fp8")
    finally:
        L.q4_set_fusion(q4.DEFAULT_FUSION)
        L.q4_set_use_graphs(1)
    # layer 0's K / V do not depend on attention: the FP8 model's rows are the round trip of the fp16 model's, bit for bit, at every position
    want = kv8_ref.round_trip(r16, hs)
    bad = np.argwhere((r8.view(np.uint16) != want.view(np.uint16)).any(axis=1)).ravel()
    assert bad.size == 0, "layer-0 K / V rows are not the round trip of the fp16 rows at positions %s" % bad[:8]
    ref = n["logits"].astype(np.float64)
    err = np.abs(l8.astype(np.float64) - ref) / np.maximum(1.0, np.abs(ref))
    worst = float(err.max())
    print("kv8 %s fusion %d graphs %d: worst logit error %.3e at position %d (bound %.1e)" % (name, fusion, graphs, worst, int(err.max(axis=1).argmax()), NET_BOUND[name]))
    observed.setdefault("kv8_network_vs_composed_forward", {})["%s_f%d_g%d" % (name, fusion, graphs)] = worst
    assert worst <= NET_BOUND[name], (worst, int(err.max(axis=1).argmax()))
    assert not np.array_equal(l8, l16)                   # (the FP8 model is not the fp16 model)


def test_split_context_bins_inside_the_network(q4, net, observed):
    """head64_long past the split threshold (bins 512 .. 1300): the same forced tokens through the captured graphs (bins, merged by each head's last
    block) and through eager launches (exact context lengths: other chunk counts), logits within the bound of
    test_split_context_merge_by_the_last_block; then the last layer's attention output of the last step, merged by the last arriver inside
    the network, against the public entry's launch over the same rows, merged by a second launch."""
    L = q4.lib()
    path, cfg = net["head64_long"]["path"], net["head64_long"]["cfg"]
    dim, heads, kv_heads, seq_len = cfg[0], cfg[3], cfg[4], cfg[6]
    hs, kv_dim, n = dim // heads, dim * kv_heads // heads, 1200
    toks = _tokens(n, cfg[5], seed=9)
    checkpoints = (300, 511, 512, 700, 1023, 1024, 1100, n - 1)
    runs = {}
    L.q4_set_fusion(1)          # (the launch sequence of an FP8 model leaves the last layer's attention output in RunState::xb at this level)
    try:
        for graphs in (1, 0):
            L.q4_set_use_graphs(graphs)
            t = q4.Transformer(path, kv="fp8")
            t.reset(toks)
            got = {}
            for pos in range(n):
                t.run_transformer(False)
                q4.synchronize()                             # (q4_run_transformer takes the position from the pinned word, as the reference's loop does: it must be current)
                if pos in checkpoints:
                    got[pos] = t.logits().astype(np.float64)
            q4.check(L.q4_handoff_status(t.state))
            runs[graphs] = got
            if graphs == 0:
                last = cfg[2] - 1
                rows = [t.kv_row(last, pos) for pos in range(n)]
                k = np.stack([r[0] for r in rows])
                v = np.stack([r[1] for r in rows])
                q = np.empty(dim, dtype=np.float16)
                xb = np.empty(dim, dtype=np.float16)
                q4.check(L.q4_memcpy_d2h(q.ctypes.data, t.state.contents.q, q.nbytes))
                q4.check(L.q4_memcpy_d2h(xb.ctypes.data, t.state.contents.xb, xb.nbytes))
            t.close()
    finally:
        L.q4_set_fusion(q4.DEFAULT_FUSION)
        L.q4_set_use_graphs(1)
    worst = 0.0
    for pos in checkpoints:
        a, b = runs[1][pos], runs[0][pos]
        worst = max(worst, float((np.abs(a - b) / np.maximum(1.0, np.abs(b))).max()))
    observed["kv8_split_graphs_vs_eager_head64_long"] = worst
    assert worst <= 5e-3, worst
    # the second-launch merge over the same state: rows below the last position from the (dequantised, idempotent) cache, the last as the staging row
    pos, bin_ = n - 1, 4096
    kb, ke = kv8_ref.quantise(k, hs)
    vb, ve = kv8_ref.quantise(v, hs)
    assert np.array_equal(kv8_ref.dequantise(kb, ke, hs), k)
    k_img, v_img = np.zeros((bin_, kv_dim), dtype=np.uint8), np.zeros((bin_, kv_dim), dtype=np.uint8)
    ke_img, ve_img = np.zeros((kv_heads, bin_), dtype=np.int8), np.zeros((kv_heads, bin_), dtype=np.int8)
    k_img[:pos], v_img[:pos], ke_img[:, :pos], ve_img[:, :pos] = kb[:pos], vb[:pos], ke[:pos].T, ve[:pos].T
    bufs = [q4.DevBuf(a) for a in (k_img, v_img, ke_img, ve_img, k[pos], v[pos], q)]
    do, dpos, att = q4.DevBuf(nbytes=dim * 2), q4.DevBuf(np.array([pos], dtype=np.int32)), q4.DevBuf(nbytes=heads * bin_ * 8)
    q4.check(L.q4_multi_head_attention_kv8(do.ptr, bufs[6].ptr, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, bufs[4].ptr, bufs[5].ptr, att.ptr,
                                           heads, hs, heads // kv_heads, bin_, dpos.ptr))
    q4.synchronize()
    second = do.get(np.float16, dim).astype(np.float64)
    assert att.get(np.uint8).any()
    d = float((np.abs(second - xb.astype(np.float64)) / np.maximum(1.0, np.abs(xb.astype(np.float64)))).max())
    observed["kv8_last_arriver_vs_second_launch_head64_long"] = d
    assert d <= 5e-3, d


# ---- the runtime -------------------------------------------------------------------------------------------------------------------
def _generate(t, prompt, steps):
    toks, _, _, _ = t.generate_ids(prompt, steps)
    return [int(v) for v in toks], t.logits().view(np.uint16).copy()


def test_formats_alternate_without_recapture(q4, net):
    L = q4.lib()
    path = net["tiny"]["path"]
    a, b = q4.Transformer(path), q4.Transformer(path, kv="fp8")
    assert L.q4_kv_format_of(a.state) == q4.KV_FP16 and L.q4_kv_format_of(b.state) == q4.KV_FP8 and L.q4_get_kv_format() == q4.KV_FP16
    first = [_generate(a, [1, 5, 9], 30), _generate(b, [1, 5, 9], 30)]
    captures = L.q4_graph_captures()
    for _ in range(2):
        for t, want in ((a, first[0]), (b, first[1])):
            toks, logits = _generate(t, [1, 5, 9], 30)
            assert toks == want[0] and np.array_equal(logits, want[1])
    assert L.q4_graph_captures() == captures, "alternating the two models captured graphs again"
    assert not np.array_equal(first[0][1], first[1][1])
    a.close()
    b.close()


@pytest.mark.parametrize("name", ["tiny", "ffn_pair7b"])
def test_fp16_models_are_untouched_by_the_setting(q4, tmp_path, name):
    """An fp16 model built after an FP8 model and q4_set_kv_format(0) computes what one built before any of it does: logits and token ring, bit for
    bit. (ffn_pair7b: the 7B-wide layers, whose FFN half runs as the pair launch with the next layer's QKV inside.) And on ffn_pair7b the FP8 model's
    pair launch (level 5, behind a separate o-proj launch) reproduces its launch sequence (level 1) bit for bit, as it does for fp16 models."""
    L = q4.lib()
    path = str(tmp_path / (name + ".bin"))
    synth.write_model(path, name, seed=11)
    steps = 140 if name == "ffn_pair7b" else 40           # (ffn_pair7b: across bins 128 and 256)
    t = q4.Transformer(path)
    before = _generate(t, [1, 17, 300, 45, 9], steps)
    t.close()
    t8 = q4.Transformer(path, kv="fp8")
    fp8 = _generate(t8, [1, 17, 300, 45, 9], steps)
    q4.check(L.q4_handoff_status(t8.state))
    t8.close()
    assert L.q4_set_kv_format(q4.KV_FP8) == 0 and L.q4_set_kv_format(q4.KV_FP16) == 0
    t = q4.Transformer(path)
    after = _generate(t, [1, 17, 300, 45, 9], steps)
    t.close()
    assert before[0] == after[0] and np.array_equal(before[1], after[1])
    assert np.isfinite(fp8[1].view(np.float16).astype(np.float32)).all() and not np.array_equal(fp8[1], before[1])
    if name == "ffn_pair7b":
        try:
            L.q4_set_fusion(1)
            t8 = q4.Transformer(path, kv="fp8")
            seq = _generate(t8, [1, 17, 300, 45, 9], steps)
            t8.close()
        finally:
            L.q4_set_fusion(q4.DEFAULT_FUSION)
        assert seq[0] == fp8[0] and np.array_equal(seq[1], fp8[1])


def test_unsupported_head_size_fails_at_build(q4):
    L = q4.lib()
    path = os.path.join(GOLDEN, "micro_model.bin")          # head size 32
    with pytest.raises(q4.Q4Error, match="FP8 KV cache: head size 32 is not supported"):
        q4.Transformer(path, kv="fp8")
    assert L.q4_get_kv_format() == q4.KV_FP16
    t = q4.Transformer(path)                                # ... and as an fp16 model it builds
    t.close()


def test_cli_honours_the_environment_variable(tmp_path):
    exe = os.path.join(ROOT, "llama_cu_awq_amd", "bin", "llama2_q4")
    tok = os.path.join(GOLDEN, "tokenizer.bin")
    path = str(tmp_path / "cli.bin")
    synth.write_model(path, (256, 352, 2, 4, 4, 32000, 256, 10000.0), seed=31)      # the model of test_cli_gpu.py
    args = [exe, path, "-n", "40", "-i", "write an essay about GPUs", "-t", "0", "-z", tok]
    env = {k: v for k, v in os.environ.items() if k != "Q4_KV_CACHE"}
    strip = lambda s: s[:s.index("achieved tok/s")]
    plain = subprocess.run(args, capture_output=True, text=True, timeout=300, errors="replace", env=env)
    fp16 = subprocess.run(args, capture_output=True, text=True, timeout=300, errors="replace", env=dict(env, Q4_KV_CACHE="fp16"))
    fp8 = subprocess.run(args, capture_output=True, text=True, timeout=300, errors="replace", env=dict(env, Q4_KV_CACHE="fp8"))
    assert plain.returncode == 0 and fp16.returncode == 0 and fp8.returncode == 0, (plain.stderr, fp8.stderr)
    assert strip(plain.stdout) == strip(fp16.stdout)        # without the variable (or with fp16) the output is what it is today
    assert "write an essay about GPUs" in fp8.stdout and "Tokens: 39" in fp8.stdout
    assert "Model params:- \ndim: 256 " in fp8.stdout and "Loading Weights... done!" in fp8.stdout
    bad = subprocess.run(args, capture_output=True, text=True, timeout=300, errors="replace", env=dict(env, Q4_KV_CACHE="int4"))
    assert bad.returncode != 0 and "Q4_KV_CACHE" in bad.stderr
