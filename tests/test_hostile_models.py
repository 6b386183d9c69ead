"""The hostile checkpoints of tests/hostile_models.py on the CPU: the default writer is unchanged, every trait is in the written file, and the
restatement (oracle/) stays a valid yardstick on them -- finite, logits O(1..100), within the unrounded double forward's bracket."""
import hashlib

import numpy as np
import pytest

import hostile_models as hm
from llama_cu_awq_amd import synth

# synth.write_model(path, name) with default arguments; the hostile traits are patched onto these bytes and must never change them
DEFAULT_SHA256 = {"tiny": "98dbd03f76aa5874e84bbf66cb1e2b9f5885de2c7c7157b4f9a405d412caf90f",
                  "micro": "b8b4b1b380e4dc45ea95ab714a0b91be0930c1d9e2a78986a15325b87d694028"}
SEQ = [1, 17, 300, 45, 9, 230, 77, 401, 12, 5, 498, 64, 33, 150]       # the fixed token sequence of the network tests


@pytest.mark.parametrize("name", sorted(DEFAULT_SHA256))
def test_default_write_model_bytes_are_pinned(tmp_path, name):
    p = str(tmp_path / (name + ".bin"))
    synth.write_model(p, name)
    assert hashlib.sha256(open(p, "rb").read()).hexdigest() == DEFAULT_SHA256[name]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("hostile")
    out = {}
    for geom in ("tiny", "small"):
        base = str(d / ("%s_default.bin" % geom))
        synth.write_model(base, geom, seed=5)
        out[geom, None] = base
        for trait in hm.TRAITS:
            p = str(d / ("%s_%s.bin" % (geom, trait)))
            hm.write_hostile_model(p, geom, trait, seed=5)
            out[geom, trait] = p
    return out


def _read(path, geom):
    return hm.Tensors(path, synth.geometry(geom), mode="r")


def _zeros_nibbles(Z, groups):
    return hm.unpack(np.asarray(Z))[:, :groups]


@pytest.mark.parametrize("trait", hm.TRAITS)
def test_traits_are_in_the_written_file(files, trait):
    geom = "small"
    dim, hidden, layers, heads, kv_heads = synth.geometry(geom)[:5]
    a, b = _read(files[geom, None], geom), _read(files[geom, trait], geom)
    on = lambda t: trait in (t, "combined")                        # noqa: E731
    assert np.array_equal(a.wcls, b.wcls)                            # no trait touches the classifier
    mch, sch = hm.massive_channels(dim), hm.sink_channels(dim)
    if on("massive"):
        assert (b.emb[:, mch] == np.array(hm.MASSIVE_VALUES, dtype=np.float16)).all()
        for layer in range(layers):
            for which in ("rms_att", "rms_ffn"):
                ra, rb = a.rms(layer, which).astype(np.float64), b.rms(layer, which).astype(np.float64)
                if trait == "massive":
                    assert np.allclose(rb[mch], ra[mch] * hm.MASSIVE_NORM_FACTOR, rtol=2e-3)
                    others = np.setdiff1d(np.arange(dim), mch)
                    assert np.array_equal(ra[others], rb[others])
                else:
                    assert (np.abs(rb[mch]) <= 8.0 * hm.MASSIVE_NORM_FACTOR * 1.01).all()
        if trait == "massive":
            assert np.array_equal(a.rms_final, b.rms_final)          # the final norm weight is left alone
    else:
        assert np.abs(b.emb.astype(np.float32)).max() < 10
    if on("peaked"):
        for layer in range(layers):
            for mat in ("q", "k"):
                Sa, Sb = a.qweight(layer, mat)[2].astype(np.float64), b.qweight(layer, mat)[2].astype(np.float64)
                if trait == "peaked":
                    assert np.allclose(Sb, Sa * hm.PEAK_SCALE, rtol=2e-3)
                nib = hm.unpack(np.asarray(b.qweight(layer, mat)[0]))[:, sch]
                assert np.isin(nib, (0, 15)).all() and (nib == nib[:, :1]).all()
        assert (b.emb[1, sch] == np.float16(hm.SINK_BOS)).all() and (b.emb[2:, sch] == np.float16(hm.SINK_SHARED)).all()
    if on("quant_edges"):
        for layer in range(layers):
            for mat in hm.MATS:
                W, Z, S, h, w = b.qweight(layer, mat)
                zn = _zeros_nibbles(Z, S.shape[1])
                assert (zn[1::8] == 0).all() and (zn[2::8] == 15).all()
                nib = hm.unpack(np.asarray(W))[3::8, :h]
                g = np.arange(h) // synth.GROUP_SIZE
                even = g % 2 == 0
                assert (nib[:, even] == zn[3::8][:, g[even]]).all()          # q == z: these groups contribute exactly zero
                if trait == "quant_edges":
                    other = np.setdiff1d(np.arange(w), np.concatenate([np.arange(1, w, 8), np.arange(2, w, 8), np.arange(3, w, 8)]))
                    s = S[other].astype(np.float64)
                    assert s.min() >= hm.QE_SCALE_LO * 0.99 and s.max() <= hm.QE_SCALE_HI * 1.01
                    assert s.max() / s.min() > 50                           # ~two decades
    if on("norm_weights"):
        vecs = [b.rms_final] + [b.rms(l, w) for l in range(layers) for w in ("rms_att", "rms_ffn")]
        for v in vecs:
            v = v.astype(np.float64)
            assert (v == 0).any() and (v < 0).any() and np.abs(v).max() <= hm.NW_HI * 1.01
        allv = np.abs(np.concatenate([v.astype(np.float64) for v in vecs]))
        assert allv[allv > 0].min() < 2e-3 and allv.max() > 4.0


def _layer0_attention(path, geom, toks):
    """Layer 0's attention probabilities of the fixed sequence in float64, straight from the file (scores [heads, T, T], probs)."""
    dim, _, _, heads, kv_heads, _, _, theta = synth.geometry(geom)
    hs, kv_mul, T = dim // heads, heads // kv_heads, len(toks)
    t = _read(path, geom)
    dense = {}
    for mat in ("q", "k"):
        W, Z, S, h, w = t.qweight(0, mat)
        dense[mat] = synth.dequant_dense(np.asarray(W).reshape(-1), np.asarray(Z).reshape(-1), np.asarray(S).reshape(-1), h, w)
    x = t.emb[toks].astype(np.float64)
    xn = x / np.sqrt((x ** 2).mean(axis=1, keepdims=True) + 1e-5) * t.rms(0, "rms_att").astype(np.float64)
    freq = theta ** (-(2.0 * np.arange(hs // 2)) / hs)

    def rope(a, nh):
        a = a.reshape(T, nh, hs)
        ang = np.arange(T)[:, None, None] * freq
        lo, hi = a[..., : hs // 2], a[..., hs // 2:]
        return np.concatenate([lo * np.cos(ang) - hi * np.sin(ang), lo * np.sin(ang) + hi * np.cos(ang)], axis=-1)
    q, k = rope(xn @ dense["q"].T, heads), rope(xn @ dense["k"].T, kv_heads)
    sc = np.einsum("thd,shd->hts", q, k[:, np.arange(heads) // kv_mul]) / np.sqrt(hs)
    sc = np.where(np.tril(np.ones((T, T), dtype=bool)), sc, -np.inf)
    p = np.exp(sc - sc.max(axis=-1, keepdims=True))
    return sc, p / p.sum(axis=-1, keepdims=True)


@pytest.mark.parametrize("geom", ["tiny", "small"])
def test_peaked_scores_and_the_sink(files, geom):
    """peaked: scores of several tens, a near-one-hot softmax, and position 0 draws far more than its uniform share."""
    sc, p = _layer0_attention(files[geom, "peaked"], geom, SEQ)
    sb, pb = _layer0_attention(files[geom, None], geom, SEQ)
    late = slice(4, None)
    assert np.abs(sb[np.isfinite(sb)]).max() < 5                     # benign: flat
    assert 20 <= np.abs(sc[np.isfinite(sc)]).max() < 2000
    assert p[:, late].max(axis=-1).mean() > 0.8                      # near-one-hot rows
    uniform = (1.0 / np.arange(1, len(SEQ) + 1))[late].mean()
    assert p[:, late, 0].mean() > 2 * uniform and pb[:, late, 0].mean() < 1.5 * uniform


@pytest.mark.parametrize("trait", hm.TRAITS)
@pytest.mark.parametrize("geom", ["tiny", "small"])
def test_the_restatement_stays_a_yardstick(orc, files, geom, trait):
    """orc.Model.forward on a hostile model: finite, logits at most O(100), and within the bound of
    tests/test_oracle.py::test_unrounded_f64_forward_brackets_the_restatement (5e-3) of the double forward."""
    m = orc.Model(files[geom, trait])
    for pos, tok in enumerate(SEQ[:8]):
        a = m.forward(tok, pos).astype(np.float64)
        b = m.forward_f64(tok, pos, cap=8)
        assert np.isfinite(a).all() and np.isfinite(b).all(), pos
        assert np.abs(a).max() <= 100.0, (pos, np.abs(a).max())
        assert np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))) < 5e-3, pos
    k, v = m.kv()
    assert np.isfinite(k[:, :8].astype(np.float32)).all() and np.isfinite(v[:, :8].astype(np.float32)).all()
    m.close()


def _attention_f64(q, kc, vc, heads, hs, kv_mul, pos):
    Q = q.reshape(heads, hs).astype(np.float64)
    K = kc.reshape(-1, heads // kv_mul, hs)[: pos + 1].astype(np.float64)[:, np.arange(heads) // kv_mul]
    V = vc.reshape(-1, heads // kv_mul, hs)[: pos + 1].astype(np.float64)[:, np.arange(heads) // kv_mul]
    sc = np.einsum("hd,thd->ht", Q, K) / np.sqrt(hs)
    p = np.exp(sc - sc.max(axis=1, keepdims=True))
    p /= p.sum(axis=1, keepdims=True)
    return np.einsum("ht,thd->hd", p, V).reshape(-1), sc


@pytest.mark.parametrize("case", ["peaked", "dominant0", "dominant_last", "flat"])
def test_restated_attention_against_fp64_on_hostile_scores(orc, rng, case):
    heads, kv_mul, hs, pos = 4, 2, 64, 300
    kv_dim = heads * hs // kv_mul
    q = rng.standard_normal(heads * hs).astype(np.float16)
    kc = (0.5 * rng.standard_normal((pos + 1) * kv_dim)).astype(np.float16)
    vc = rng.standard_normal((pos + 1) * kv_dim).astype(np.float16)
    if case == "peaked":
        q = (q.astype(np.float32) * 16).astype(np.float16)                # scores of several tens
    elif case.startswith("dominant"):
        at = 0 if case == "dominant0" else pos
        K = kc.reshape(pos + 1, -1, hs)
        K[at] = (q.reshape(heads // kv_mul, kv_mul, hs).astype(np.float32).mean(axis=1) * 4.0).astype(np.float16)   # score ~ +16
    else:
        kc[:] = kc[:kv_dim].reshape(1, -1).repeat(pos + 1, 0).reshape(-1)   # all keys equal: the mean of the V rows
    out, att = orc.attention(q, kc, vc, heads, hs, kv_mul, pos)
    ref, sc = _attention_f64(q, kc, vc, heads, hs, kv_mul, pos)
    assert np.isfinite(out.astype(np.float32)).all()
    if case == "peaked":
        assert np.abs(sc).max() > 20
    if case.startswith("dominant"):
        at = 0 if case == "dominant0" else pos
        V = vc.reshape(pos + 1, -1, hs)[at][np.arange(heads) // kv_mul].reshape(-1).astype(np.float64)
        assert np.abs(ref - V).max() < 1e-2                              # the fp64 output is (almost exactly) that V row
    if case == "flat":
        mean = vc.reshape(pos + 1, -1, hs).astype(np.float64).mean(axis=0)[np.arange(heads) // kv_mul].reshape(-1)
        assert np.abs(ref - mean).max() < 1e-12
    # fp16 scores (ulp 2^-6 at |s| ~ 30 moves a probability by ~1.5 %) and fp16 probabilities: a few 1e-2 absolute on unit-scale V
    tol = 3e-2 if case == "peaked" else 6e-3
    assert np.abs(out.astype(np.float64) - ref).max() < tol, float(np.abs(out.astype(np.float64) - ref).max())
