"""The fp16 companion kernels (rmsnorm, attention, RoPE, the fp16 classifier GEMV) on hostile inputs: massive channels up to 65504, all-zero and
fp16-denormal inputs, norm weights with zeros and negatives, near-one-hot and exactly flat softmaxes, one dominant key on both sides of a
256-position chunk boundary, V outliers at +-1000, rope_theta 5e5 / 1e6 at positions up to 16383. Each case against the restatement (oracle/)
and a plain float64 evaluation written here; the worst observed values go to parity_observed.json."""
import numpy as np
import pytest

from conftest import assert_close_f16, f16_ulp_diff
from test_ops_gpu import _attention_close

pytestmark = pytest.mark.gpu

F16_MAX = 65504.0


def _rec(observed, key, **vals):
    o = observed.setdefault("hostile_ops", {}).setdefault(key, {})
    for k, v in vals.items():
        o[k] = max(o.get(k, 0.0), float(v))


# ---- rmsnorm ------------------------------------------------------------------------------------------------------------------------------

def _rms_case(rng, case, size):
    x = rng.standard_normal(size).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(size)).astype(np.float32)
    ch = np.unique(np.array([1, size // 3, size // 2 + 1, size - 2]) % size)
    if case == "massive":                                  # a few channels at 1e2 .. 1e3 and one at the fp16 limit
        x[ch] = np.array([300.0, -1000.0, 2000.0, -F16_MAX])[: len(ch)]
        w[ch] *= 0.01
    elif case == "at_f16_max":
        x[ch[0]] = F16_MAX
    elif case == "zeros":
        x[:] = 0
    elif case == "eps_dominates":                          # mean(x^2) ~ 1e-8 << eps 1e-5
        x *= 1e-4
    elif case == "denormal":                               # fp16 subnormals (< 6.1e-5)
        x *= 1.5e-5
    elif case == "weights_zero_negative":
        w = np.exp(rng.uniform(np.log(1e-3), np.log(8.0), size)).astype(np.float32)
        w[rng.random(size) < 0.1] *= -1
        w[rng.random(size) < 0.05] = 0
        w[0] = 0
    return x.astype(np.float16), w.astype(np.float16)


@pytest.mark.parametrize("case", ["massive", "at_f16_max", "zeros", "eps_dominates", "denormal", "weights_zero_negative"])
@pytest.mark.parametrize("size", [8, 256, 4096, 5120, 8192])
def test_rmsnorm_hostile(q4, orc, rng, observed, size, case):
    x, w = _rms_case(rng, case, size)
    ref = orc.rmsnorm(x, w)
    xf = x.astype(np.float64)
    ref64 = xf / np.sqrt((xf ** 2).mean() + 1e-5) * w.astype(np.float64)
    dx, dw, do = q4.DevBuf(x), q4.DevBuf(w), q4.DevBuf(nbytes=size * 2)
    q4.rmsnorm(do, dx, dw, size)
    q4.synchronize()
    got = do.get(np.float16, size)
    q4.rmsnorm(dx, dx, dw, size)                           # in place, as the final norm
    q4.synchronize()
    got_in_place = dx.get(np.float16, size)
    assert np.array_equal(got.view(np.uint16), got_in_place.view(np.uint16)), "in place differs from out of place"
    if case == "zeros":
        assert (got.view(np.uint16) & 0x7FFF == 0).all(), "rmsnorm of an all-zero input must be exactly 0"
    assert_close_f16(got, ref, ref64, what="rmsnorm %s %d" % (case, size))
    _rec(observed, "rmsnorm_%s" % case, max_ulp=f16_ulp_diff(got, ref).max(), max_abs_err_vs_f64=np.abs(got.astype(np.float64) - ref64).max())


# ---- fp16 classifier GEMV -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["massive", "zeros", "denormal"])
@pytest.mark.parametrize("n,d", [(4096, 32000), (5120, 32008), (4096, 16376), (2048, 64)])   # strips x 3, gemv_f16_kernel
def test_matmul_f16_hostile(q4, orc, rng, observed, n, d, case):
    w = (rng.standard_normal(n * d) * 0.02).astype(np.float16)
    x = rng.standard_normal(n).astype(np.float32)
    if case == "massive":
        x[[n // 8 + 1, 3 * n // 8 + 3, 5 * n // 8 + 5, 7 * n // 8 + 7]] = (300.0, -600.0, 1000.0, -2000.0)
    elif case == "zeros":
        x[:] = 0
    elif case == "denormal":
        x *= 1.5e-5
    x = x.astype(np.float16)
    ref = orc.matmul_f16(x, w, n, d)
    ref64 = w.reshape(d, n).astype(np.float64) @ x.astype(np.float64)
    dw, dx, do = q4.DevBuf(w), q4.DevBuf(x), q4.DevBuf(nbytes=d * 2)
    q4.matmul(do, dx, dw, n, d)
    q4.synchronize()
    got = do.get(np.float16, d)
    if case == "zeros":
        assert (got.view(np.uint16) & 0x7FFF == 0).all(), "an all-zero x must give exactly 0"
    assert_close_f16(got, ref, ref64, what="fp16 gemv %s %dx%d" % (case, n, d))
    _rec(observed, "matmul_f16_%s" % case, max_ulp=f16_ulp_diff(got, ref).max())


# ---- RoPE ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("theta", [5e5, 1e6])
@pytest.mark.parametrize("pos", [8191, 8192, 16383])
@pytest.mark.parametrize("hs", [64, 128, 256])
def test_rope_long_theta(q4, orc, rng, observed, hs, pos, theta):
    heads, kv_heads = 8, 2
    q = rng.standard_normal(heads * hs).astype(np.float16)
    kv_dim = kv_heads * hs
    seq = pos + 1
    kc = np.zeros(seq * kv_dim, dtype=np.float16)
    kc[pos * kv_dim:] = rng.standard_normal(kv_dim).astype(np.float16)
    krow = kc[pos * kv_dim:]
    rq, rk = orc.rope(q, krow, heads, kv_heads, hs, pos, theta)
    dq, dk, dpos = q4.DevBuf(q), q4.DevBuf(kc), q4.DevBuf(np.array([pos], dtype=np.int32))
    q4.RoPERotation(dq, dk, heads, kv_heads, hs, dpos, 0, theta)
    q4.synchronize()
    gq, gk = dq.get(np.float16), dk.get(np.float16)[pos * kv_dim:]
    # against the restatement: absolute, not in ulps. Both compute the angle pos * theta^(-2i/hs) in fp32; one fp32 ulp of the frequency (powf here,
    # the device's pow there) moves the angle by up to pos * 2^-24 rad, 1e-3 rad at 16383, so an output that cancels to ~0.01 differs by tens of its own
    # ulps (measured worst over these 18 cases in two runs: 2.1e-3, 2.7e-3 absolute on unit-scale inputs). Bound: ~3x the first, 2.4x the second
    for got, ref, what in ((gq, rq, "rope q"), (gk, rk, "rope k")):
        err = np.abs(got.astype(np.float64) - ref.astype(np.float64)).max()
        _rec(observed, "rope_theta_vs_restatement", abs_err=err)
        assert err <= 6.5e-3, "%s: max |gpu - restatement| %g" % (what, err)
    # float64 rotation (pairs i, i + hs/2; frequency theta^(-2i/hs)). The restatement's angle pos * freq is an fp32 product (2^-24 relative of up to
    # 16383 rad: ~1e-3 rad), as the kernel's: the kernel may be at most 1.5x as far from the exact rotation as the restatement, plus 1 fp16 ulp
    freq = float(theta) ** (-(2.0 * np.arange(hs // 2)) / hs)
    ang = pos * freq

    def rot(v, nh):
        v = v.astype(np.float64).reshape(nh, hs)
        lo, hi = v[:, : hs // 2], v[:, hs // 2:]
        return np.concatenate([lo * np.cos(ang) - hi * np.sin(ang), lo * np.sin(ang) + hi * np.cos(ang)], axis=1).reshape(-1)
    for got, ref, exact in ((gq, rq, rot(q, heads)), (gk, rk, rot(krow, kv_heads))):
        eg = np.abs(got.astype(np.float64) - exact).max()
        er = np.abs(ref.astype(np.float64) - exact).max()
        assert eg <= 1.5 * er + 2.0 ** -10 * np.abs(exact).max(), (eg, er)
        _rec(observed, "rope_theta_vs_f64", gpu=eg, restatement=er)


# ---- attention ----------------------------------------------------------------------------------------------------------------------------

ATT_CASES = ["peaked", "dominant_0", "dominant_pos", "dominant_255", "dominant_256", "dominant_511", "dominant_512", "flat", "q_zero", "v_outliers"]


def _att_case(rng, case, heads, kv_mul, hs, pos, seq):
    kv_heads = heads // kv_mul
    q = rng.standard_normal(heads * hs).astype(np.float32)
    K = (0.5 * rng.standard_normal((seq, kv_heads, hs))).astype(np.float32)
    V = rng.standard_normal((seq, kv_heads, hs)).astype(np.float32)
    K[pos + 1:] = 0
    V[pos + 1:] = 0
    dominant = None
    if case == "peaked":                                   # scores ~ N(0, 30^2)
        q *= 60.0
    elif case.startswith("dominant"):                      # this key's score ~ +40, every other one ~ N(0, 0.5^2)
        dominant = pos if case == "dominant_pos" else int(case.split("_")[1])
        qm = q.reshape(kv_heads, kv_mul, hs).mean(axis=1)
        K[dominant] = qm * (40.0 * kv_mul / np.sqrt(hs))
    elif case == "flat":                                   # all keys equal: the output is the mean of the V rows
        K[: pos + 1] = K[0]
    elif case == "q_zero":
        q[:] = 0
    elif case == "v_outliers":                             # massive V channels, one sign per channel
        ch = [1, hs // 2 + 3]
        V[: pos + 1, :, ch[0]] += 1000.0
        V[: pos + 1, :, ch[1]] -= 1000.0
    return q.astype(np.float16), K.astype(np.float16), V.astype(np.float16), dominant


def _attention_f64(q, K, V, heads, kv_mul, hs, pos):
    kvh = np.arange(heads) // kv_mul
    Q = q.reshape(heads, hs).astype(np.float64)
    Kf = K[: pos + 1].astype(np.float64)[:, kvh]
    Vf = V[: pos + 1].astype(np.float64)[:, kvh]
    sc = np.einsum("hd,thd->ht", Q, Kf) / np.sqrt(hs)
    p = np.exp(sc - sc.max(axis=1, keepdims=True))
    p /= p.sum(axis=1, keepdims=True)
    return np.einsum("ht,thd->hd", p, Vf).reshape(-1), sc


def _run_attention(q4, q, K, V, heads, kv_mul, hs, pos, seq, scratch):
    dim = heads * hs
    dq, dk, dv, do = q4.DevBuf(q), q4.DevBuf(K.reshape(-1)), q4.DevBuf(V.reshape(-1)), q4.DevBuf(nbytes=dim * 2)
    dpos = q4.DevBuf(np.array([pos], dtype=np.int32))
    att = q4.DevBuf(nbytes=heads * max(seq, dim) * 2 * 2) if scratch else None
    q4.check(q4.lib().q4_multi_head_attention(do.ptr, dq.ptr, dk.ptr, dv.ptr, att.ptr if att else None, heads, hs, kv_mul, seq, dpos.ptr))
    q4.synchronize()
    return do.get(np.float16, dim)


def _check_attention(q4, orc, rng, observed, case, heads, kv_mul, hs, pos, seq, scratch, form):
    q, K, V, dominant = _att_case(rng, case, heads, kv_mul, hs, pos, seq)
    ref, _ = orc.attention(q, K.reshape(-1), V.reshape(-1), heads, hs, kv_mul, pos, max_seq_len=seq)
    ref64, sc = _attention_f64(q, K, V, heads, kv_mul, hs, pos)
    kvh = np.arange(heads) // kv_mul
    # the float64 yardstick has the property the case was built for
    if case == "peaked":
        assert np.abs(sc).max() > 50
    if dominant is not None:
        assert np.abs(ref64 - V[dominant].astype(np.float64)[kvh].reshape(-1)).max() < 1e-3
    if case in ("flat", "q_zero"):
        assert np.abs(ref64 - V[: pos + 1].astype(np.float64).mean(axis=0)[kvh].reshape(-1)).max() < 1e-9
    got = _run_attention(q4, q, K, V, heads, kv_mul, hs, pos, seq, scratch)
    assert np.isfinite(got.astype(np.float32)).all()
    _attention_close(got, ref, frac_gt1=0.25 if scratch else 0.03)
    # float64 bracket: at most 1.5x the restatement's distance from the exact softmax, plus 2 fp16 ulps of the output scale
    eg = np.abs(got.astype(np.float64) - ref64).max()
    er = np.abs(ref.astype(np.float64) - ref64).max()
    scale = max(1.0, np.abs(ref64).max())
    assert eg <= 1.5 * er + 2.0 * 2.0 ** -10 * scale, (case, eg, er)
    d = f16_ulp_diff(got, ref)
    _rec(observed, "attention_%s_%s" % (form, case), max_ulp=d.max(), frac_gt1=(d > 1).mean(), gpu_vs_f64=eg / scale, restatement_vs_f64=er / scale)


@pytest.mark.parametrize("case", ATT_CASES)
@pytest.mark.parametrize("hs,kv_mul", [(64, 1), (64, 4), (128, 1), (128, 4), (256, 1), (256, 2)])
def test_attention_one_block_hostile(q4, orc, rng, observed, hs, kv_mul, case):
    """The one-block-per-head kernel (att = None): 600 positions, a 1024-position bin."""
    _check_attention(q4, orc, rng, observed, case, 8, kv_mul, hs, 600, 1024, False, "one_block")


@pytest.mark.parametrize("case", ATT_CASES)
@pytest.mark.parametrize("hs,kv_mul", [(64, 1), (64, 4), (128, 1), (128, 4), (256, 1), (256, 2)])
def test_attention_split_context_hostile(q4, orc, rng, observed, hs, kv_mul, case):
    """Split context (one block per (head, 256 positions) + the merge, scratch = `att`): 600 positions in a 2048-position bin, three chunks."""
    _check_attention(q4, orc, rng, observed, case, 8, kv_mul, hs, 600, 2048, True, "split")


@pytest.mark.parametrize("case", ["peaked", "dominant_0", "dominant_pos", "dominant_8191", "dominant_8192", "flat", "v_outliers"])
@pytest.mark.parametrize("scratch", [False, True])
def test_attention_16k_hostile(q4, orc, rng, observed, scratch, case):
    """The 16K-context path (softmax_kernel_no_smem's restatement above 8192), grouped-query."""
    _check_attention(q4, orc, rng, observed, case, 8, 2, 128, 16000, 16384, scratch, "16k")
