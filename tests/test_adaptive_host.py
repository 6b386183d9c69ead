"""typical-p, top-n-sigma and Mirostat v2 without a GPU: the text parser, every argument check of the setter, the getter and the op-level launcher (none
of which may touch the GPU), and the numpy restatement (tests/adaptive_ref.py) on vectors worked by hand."""
import ctypes as C

import numpy as np
import pytest

import adaptive_ref as ref

ERR_ARG = 5
F = np.float32
NAN, INF = float("nan"), float("inf")


def _api():
    from llama_cu_awq_amd import api
    return api


# ---------------------------------------------------------------------------------------------------------------------------------
# the parser
def test_parser_any_order_defaults_and_errors():
    api = _api()
    L = api.lib()
    c = api.parse_adaptive("typical_p=0.9,top_n_sigma=1.5,mirostat_tau=5,mirostat_eta=0.1")
    assert c.as_dict() == dict(typical_p=F(0.9), top_n_sigma=1.5, mirostat_tau=5.0, mirostat_eta=F(0.1))
    c = api.parse_adaptive("mirostat_tau=3,typical_p=0.5")             # any subset, any order; the rest neutral
    assert c.as_dict() == dict(typical_p=0.5, top_n_sigma=0.0, mirostat_tau=3.0, mirostat_eta=F(0.1))
    assert api.parse_adaptive("").as_dict() == api.AdaptiveControls().as_dict() == {k: F(v) for k, v in ref.NEUTRAL.items()}
    assert api.parse_adaptive("typical_p=1,mirostat_eta=1").as_dict() == dict(typical_p=1.0, top_n_sigma=0.0, mirostat_tau=0.0, mirostat_eta=1.0)
    out = api.AdaptiveControls(top_n_sigma=7.0)
    for bad in ("top_k=3", "typical_p", "typical_p=", "=0.9", "typical_p=0.9x", "top_n_sigma=abc", "typical_p=0.9,", ",typical_p=0.9",
                "typical_p=0.9,,top_n_sigma=1", "typical_p=0.9,typical_p=0.9", "mirostat_tau=5,mirostat_eta=0.1,mirostat_tau=5", "typical_p=0",
                "typical_p=-0.1", "typical_p=1.5", "typical_p=nan", "top_n_sigma=-1", "top_n_sigma=inf", "top_n_sigma=nan", "mirostat_tau=-1",
                "mirostat_tau=inf", "mirostat_tau=nan", "mirostat_eta=0", "mirostat_eta=1.5", "mirostat_eta=nan", "mirostat_eta=-0.1",
                "typical_p=0.9 ", "Typical_p=0.9"):
        assert L.q4_parse_adaptive(bad.encode(), C.byref(out)) == ERR_ARG, bad
        assert out.top_n_sigma == 7.0 and out.typical_p == 1.0, "a failed parse wrote its output"
    assert L.q4_parse_adaptive(None, C.byref(out)) == ERR_ARG and L.q4_parse_adaptive(b"typical_p=0.9", None) == ERR_ARG


# ---------------------------------------------------------------------------------------------------------------------------------
# the argument checks
@pytest.fixture()
def sampler():
    """a Sampler the test builds itself: the struct of include/llama2_q4.h, zeroed (no device buffer: nothing here may touch the GPU)"""
    L = _api().lib()
    L.destroy_sampler.argtypes = [C.c_void_p]
    L.destroy_sampler.restype = None
    buf = C.create_string_buffer(64)
    yield C.cast(buf, C.c_void_p)
    L.destroy_sampler(C.cast(buf, C.c_void_p))                  # forgets the settings kept beside it


BAD = (dict(typical_p=0.0), dict(typical_p=-0.5), dict(typical_p=1.0001), dict(typical_p=NAN), dict(typical_p=INF), dict(top_n_sigma=-0.5),
       dict(top_n_sigma=NAN), dict(top_n_sigma=INF), dict(mirostat_tau=-1.0), dict(mirostat_tau=NAN), dict(mirostat_tau=INF), dict(mirostat_eta=0.0),
       dict(mirostat_eta=-0.1), dict(mirostat_eta=1.5), dict(mirostat_eta=NAN))
GOOD = (dict(typical_p=1.0), dict(typical_p=1e-6), dict(top_n_sigma=0.0), dict(top_n_sigma=100.0), dict(mirostat_tau=0.0), dict(mirostat_tau=50.0),
        dict(mirostat_eta=1.0), dict(mirostat_eta=1e-3))


def test_setter_and_getter_argument_checks(sampler):
    api = _api()
    L, AC = api.lib(), api.AdaptiveControls
    got = AC(top_n_sigma=9.0)
    assert L.q4_sampler_get_adaptive(sampler, C.byref(got)) == 0 and got.as_dict() == AC().as_dict()      # never set: neutral, off
    good = AC(typical_p=0.9, top_n_sigma=1.5, mirostat_tau=5.0, mirostat_eta=0.2)
    assert L.q4_sampler_set_adaptive(sampler, C.byref(good)) == 0
    assert L.q4_sampler_get_adaptive(sampler, C.byref(got)) == 0 and got.as_dict() == good.as_dict()
    for kw in BAD:
        assert L.q4_sampler_set_adaptive(sampler, C.byref(AC(**kw))) == ERR_ARG, kw
        assert L.q4_sampler_get_adaptive(sampler, C.byref(got)) == 0 and got.as_dict() == good.as_dict(), "a refused call changed the settings"
    for kw in GOOD:
        assert L.q4_sampler_set_adaptive(sampler, C.byref(AC(**kw))) == 0, kw
    assert L.q4_sampler_set_adaptive(None, C.byref(good)) == ERR_ARG
    assert L.q4_sampler_get_adaptive(None, C.byref(got)) == ERR_ARG and L.q4_sampler_get_adaptive(sampler, None) == ERR_ARG
    assert L.q4_sampler_set_adaptive(sampler, None) == 0                                               # NULL: off, neutral comes back
    assert L.q4_sampler_get_adaptive(sampler, C.byref(got)) == 0 and got.as_dict() == AC().as_dict()


def test_op_argument_checks_come_before_the_gpu():
    """every refusal of q4_adaptive_mask is decided on the host: the pointers here are not device pointers, so a launch would fault"""
    api = _api()
    L, AC = api.lib(), api.AdaptiveControls
    fake = C.c_void_p(0x1000)
    ok = AC(typical_p=0.9)
    assert L.q4_adaptive_mask(None, 8, C.byref(ok), 1.0, None, None, None, None, None) == ERR_ARG
    assert L.q4_adaptive_mask(fake, 0, C.byref(ok), 1.0, None, None, None, None, None) == ERR_ARG
    assert L.q4_adaptive_mask(fake, 8, None, 1.0, None, None, None, None, None) == ERR_ARG
    for kw in BAD:
        assert L.q4_adaptive_mask(fake, 8, C.byref(AC(**kw)), 1.0, None, None, None, None, None) == ERR_ARG, kw
    miro = AC(mirostat_tau=5.0)
    for t, mu, side, tok, pos in ((0.0, fake, fake, fake, fake), (-1.0, fake, fake, fake, fake), (NAN, fake, fake, fake, fake), (INF, fake, fake, fake, fake),
                                  (0.8, None, fake, fake, fake), (0.8, fake, None, fake, fake), (0.8, fake, fake, None, fake), (0.8, fake, fake, fake, None)):
        assert L.q4_adaptive_mask(fake, 8, C.byref(miro), t, mu, side, tok, pos, None) == ERR_ARG, (t, mu, side, tok, pos)
    assert L.q4_adaptive_mask(fake, 8, C.byref(AC()), 1.0, None, None, None, None, None) == 0         # everything neutral: off, no launch
    assert L.q4_get_adaptive_records(None, 0, 1, fake) == ERR_ARG


# ---------------------------------------------------------------------------------------------------------------------------------
# the restatement on vectors worked by hand
def test_two_equal_tokens_stay_under_any_typical_p():
    """0.5 / 0.5: both surprises equal the entropy (ln 2), both deviations are 0: ONE tier, which stays whole"""
    x = np.array([1.5, 1.5], dtype=np.float16)
    for tp in (1e-6, 0.25, 0.5, 0.75, 0.999):
        out, rec, _ = ref.run(x, dict(typical_p=tp))
        assert out.tobytes() == x.tobytes() and rec["kept"] == 2, tp
        assert abs(rec["H"] - np.log(2.0)) < 1e-12 and rec["d_star"] < 1e-12 and abs(rec["lse"] - (1.5 + np.log(2.0))) < 1e-12


def test_typical_p_drops_the_far_tiers_first():
    """p = (0.5, 0.25, 0.125, 0.125): surprises 1, 2, 3, 3 bits, H = 1.75 bits, deviations 0.75, 0.25, 1.25, 1.25 bits: the order is token 1, token 0,
    then the pair {2, 3} together"""
    x = np.log(np.array([0.5, 0.25, 0.125, 0.125])).astype(np.float16)
    for tp, kept in ((0.2, [1]), (0.3, [0, 1]), (0.74, [0, 1]), (0.76, [0, 1, 2, 3]), (0.99, [0, 1, 2, 3])):
        out, rec, _ = ref.run(x, dict(typical_p=tp))
        assert np.nonzero(np.isfinite(out.astype(F)))[0].tolist() == kept, (tp, out)
        assert abs(rec["H"] - 1.75 * np.log(2.0)) < 2e-3       # (the logits are rounded to half)


def test_equal_logits_have_sigma_zero_and_all_stay():
    x = np.full(37, -2.75, dtype=np.float16)
    for ns in (0.5, 1.0, 10.0):
        out, rec, extra = ref.run(x, dict(top_n_sigma=ns))
        assert extra["sigma"] == 0.0 and rec["T_s"] == -2.75 and out.tobytes() == x.tobytes() and rec["kept"] == 37


def test_top_n_sigma_by_hand():
    """(0, 0, 0, 4): mean 1, variance 3, sigma sqrt(3); T_s = 4 - n sqrt(3): n = 2 leaves the 4 alone (T_s = 0.54), n = 2.5 lets the zeros in (T_s < 0)"""
    x = np.array([0, 0, 0, 4, -np.inf, np.nan], dtype=np.float16)                 # (-inf and NaN enter no statistic and stay as they are)
    out, rec, extra = ref.run(x, dict(top_n_sigma=2.0))
    assert abs(extra["sigma"] - np.sqrt(3.0)) < 1e-12 and abs(rec["T_s"] - (4 - 2 * np.sqrt(3.0))) < 1e-12
    assert out.view(np.uint16).tolist() == [0xFC00, 0xFC00, 0xFC00, 0x4400, 0xFC00, x.view(np.uint16)[5]] and rec["kept"] == 1
    out, rec, _ = ref.run(x, dict(top_n_sigma=2.5))
    assert out.tobytes() == x.tobytes() and rec["kept"] == 4


def test_mirostat_chain_of_three_steps_by_hand():
    """p = (1/2, 1/4, 1/8, 1/8) at temperature 1, tau 1.1, eta 0.5; surprises 1, 2, 3, 3 bits.
    position 0: a span starts, mu = 2 tau = 2.2: tokens 0 and 1 stay (surprise <= 2.2); renormalised (2/3, 1/3). The sampler takes token 1:
    position 1: surprise log2(3) = 1.585, mu = 2.2 - 0.5 (1.585 - 1.1) = 1.9575: only token 0 stays (1 <= 1.9575 < 2). The sampler takes token 0:
    position 2: surprise 0, mu = 1.9575 - 0.5 (0 - 1.1) = 2.5075: tokens 0 and 1 stay again."""
    x = np.log(np.array([0.5, 0.25, 0.125, 0.125])).astype(np.float16)
    c = dict(mirostat_tau=1.1, mirostat_eta=0.5)
    ch = ref.Chain()
    out, rec, _ = ref.run(x, c, 1.0, ch, 0, None)
    assert abs(rec["mu"] - 2.2) < 1e-6 and np.isfinite(out.astype(F)).tolist() == [True, True, False, False]
    assert abs(ch.side_lse - np.log(0.75)) < 2e-3 and ch.side_pos == 0 and np.isneginf(ch.side[2:]).all()
    out, rec, _ = ref.run(x, c, 1.0, ch, 1, 1)
    assert abs(rec["mu"] - (2.2 - 0.5 * (np.log2(3.0) - 1.1))) < 3e-3 and np.isfinite(out.astype(F)).tolist() == [True, False, False, False]
    out, rec, _ = ref.run(x, c, 1.0, ch, 2, 0)
    assert abs(rec["mu"] - (2.2 - 0.5 * (np.log2(3.0) - 1.1) + 0.55)) < 3e-3 and np.isfinite(out.astype(F)).tolist() == [True, True, False, False]
    assert sorted(ch.mu) == [0, 1, 2]
    # a token the last launch masked has no surprise, a side buffer of another position is stale: mu stays
    out, rec3, _ = ref.run(x, c, 1.0, ch, 3, 3)
    assert rec3["mu"] == ch.mu[2]
    ch.side_pos = 1
    out, rec4, _ = ref.run(x, c, 1.0, ch, 4, 0)
    assert rec4["mu"] == ch.mu[3]
    # mu below the most probable token's own surprise: that token stays alone
    ch5 = ref.Chain()
    out, rec5, _ = ref.run(x, dict(mirostat_tau=0.25, mirostat_eta=0.5), 1.0, ch5, 0, None)
    assert rec5["mu"] == 0.5 and np.isfinite(out.astype(F)).tolist() == [True, False, False, False]


def test_exact_masks_follow_the_recorded_thresholds():
    """expect_from_record is float32 throughout: an entry exactly AT a threshold stays, the next half below goes"""
    x = np.array([1.0, 0.5, 0.25, -np.inf], dtype=np.float16)
    nan = {k: np.float64("nan") for k in ref.FIELDS}
    out, _, _ = ref.expect_from_record(x, dict(nan, T_s=0.5))
    assert np.isfinite(out.astype(F)).tolist() == [True, True, False, False]
    out, _, _ = ref.expect_from_record(x, dict(nan, T_m=F(0.5) / F(0.8)), temperature=0.8)
    assert np.isfinite(out.astype(F)).tolist() == [True, True, False, False]
    out, _, _ = ref.expect_from_record(x, dict(nan, T_m=5.0), temperature=0.8)     # above everything: the largest w stays
    assert np.isfinite(out.astype(F)).tolist() == [True, False, False, False]
    out, d, part = ref.expect_from_record(x, dict(nan, lse=2.0, H=1.25, d_star=0.25))   # s = 1, 1.5, 1.75; d = 0.25, 0.25, 0.5
    assert np.isfinite(out.astype(F)).tolist() == [True, True, False, False] and d[:3].tolist() == [0.25, 0.25, 0.5] and part.tolist() == [True, True, True, False]
