"""Guided decoding, host side (llama_cu_awq_amd/guide.py, the argument checks of q4_guide_new, q4_tokenizer_piece): the token automata built from
regular expressions over the committed tokenizer's pieces are sound (every walk spells a match), complete (every segmentation of a match is accepted)
and reject what does not match; from_choices accepts exactly its choices. No GPU."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

from conftest import GOLDEN
from llama_cu_awq_amd import api, guide

ERR_ARG = 5
EOS = 2
DEAD = guide.DEAD

# pattern: (longest match in bytes, matching strings, non-matching strings); all of bounded length, so every walk ends
PATTERNS = {
    r"(yes|no|maybe)": (5, [b"yes", b"no", b"maybe", b"yes", b"no", b"maybe", b"no", b"yes"],
                        [b"", b"ye", b"yesno", b"Yes", b"maybe ", b"n", b"mayb", b"noo"]),
    r"-?(0|[1-9][0-9]{0,5})(\.[0-9]{1,3})?": (11, [b"0", b"-0", b"7", b"123456", b"-999999.999", b"0.5", b"10.25", b"-3.141", b"42", b"100000.0"],
                                               [b"", b"-", b"00", b"01", b"1234567", b"1.", b"1.2345", b".5", b"--1", b"1e5", b"+1"]),
    r'\{"name": "[a-z]{1,8}", "age": [1-9][0-9]?\}': (31, [b'{"name": "a", "age": 1}', b'{"name": "bob", "age": 42}', b'{"name": "abcdefgh", "age": 99}',
                                                           b'{"name": "zz", "age": 10}', b'{"name": "alice", "age": 7}', b'{"name": "q", "age": 90}',
                                                           b'{"name": "name", "age": 31}', b'{"name": "age", "age": 5}'],
                                                      [b"", b"{}", b'{"name": "", "age": 1}', b'{"name": "Bob", "age": 1}', b'{"name": "bob", "age": 0}',
                                                       b'{"name": "bob", "age": 100}', b'{"name": "abcdefghi", "age": 1}', b'{"name":"bob","age":1}',
                                                       b'{"name": "bob", "age": 1} ', b'{"name": "bob", "age": 1']),
    r"[A-Z][a-z]{1,6}( [A-Z][a-z]{1,6}){0,2}": (23, [b"Ab", b"Alice", b"Alice Bob", b"Anna Maria Smith", b"Abcdefg", b"Abcdefg Hijklmn Opqrstu", b"Xy Zw", b"Jo Li Wu"],
                                                [b"", b"A", b"alice", b"Alice ", b"Alice  Bob", b"Alice bob", b"Abcdefgh", b"Aa Bb Cc Dd", b"ALICE", b" Alice"]),
    # a bytes pattern: the quantifier binds the LAST byte of the two-byte character, as in re.fullmatch(pattern.encode(), ...)
    # (the vocabulary spells a byte >= 0x80 only inside a whole character: the listed strings are valid UTF-8)
    '[^"\\n]{0,12}é?': (14, ["é".encode(), "abcé".encode(), "hello world é".encode(), "twelve chars".encode() + "é".encode(), b"a b\tc\xc3\xa9",
                             "ééé".encode(), b"123456789012\xc3\xa9", "{}[]()é".encode(), "ééééééé".encode()],
                        [b"", b"abc", b'a"\xc3\xa9', b"a\n\xc3\xa9", b"1234567890123\xc3\xa9", "abcée".encode(), "éééééééé".encode(), "é ".encode()]),
}


def _file_pieces():
    d = open(os.path.join(GOLDEN, "tokenizer.bin"), "rb").read()
    off, out = 4, []
    while off < len(d):
        _, n = struct.unpack_from("<fi", d, off)
        out.append(d[off + 8:off + 8 + n])
        off += 8 + n
    return out


@pytest.fixture(scope="module")
def pieces():
    tk = api.Tokenizer(os.path.join(GOLDEN, "tokenizer.bin"), 32000)
    out = tk.pieces()
    tk.close()
    return out


@pytest.fixture(scope="module")
def tables(pieces):
    return {pat: guide.from_regex(pat, pieces) for pat in PATTERNS}


def _by_bytes(pieces, text):
    """byte by byte: the single-byte pieces are ids 3 .. 130 (the file spells a byte >= 0x80 as a two-byte piece, so a non-ASCII character goes in whole,
    by its own piece)"""
    out, off = [], 0
    while off < len(text):
        b = text[off]
        if b < 0x80:
            assert pieces[b + 3] == bytes([b])
            out.append(b + 3)
            off += 1
        else:
            n = len(text[off:].decode("utf-8")[0].encode("utf-8"))
            out.append(pieces.index(text[off:off + n]))
            off += n
    return out


def _longest_first(pieces, text):
    """greedy: at every offset the longest piece (no special token, the lowest id among equals) that the rest of the text starts with"""
    ids = {}
    for i, p in enumerate(pieces):
        if i > 2 and p and p not in ids:
            ids[p] = i
    longest = max(len(p) for p in ids)
    out, off = [], 0
    while off < len(text):
        for n in range(min(longest, len(text) - off), 0, -1):
            if text[off:off + n] in ids:
                out.append(ids[text[off:off + n]])
                off += n
                break
        else:
            raise AssertionError("no piece for %r" % text[off:off + 1])
    return out


def _accepts(table, tokens):
    states = guide.walk(table, tokens)
    return states[-1] != guide.OFFTRACK and table[states[-1], EOS] != DEAD


def test_tokenizer_piece_returns_the_files_bytes(pieces):
    want = _file_pieces()
    assert len(want) == 32000 and want[3] == b"\x00"
    for i in (0, 3, 13, 31999):
        assert pieces[i] == want[i], i
    assert pieces == want
    tk = api.Tokenizer(os.path.join(GOLDEN, "tokenizer.bin"), 32000)
    p, n = C.c_void_p(), C.c_int()
    for bad in (-1, 32000):
        assert api.lib().q4_tokenizer_piece(tk.h, bad, C.byref(p), C.byref(n)) == ERR_ARG
    tk.close()


@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_tables_are_well_formed(tables, pattern):
    t = tables[pattern]
    S = t.shape[0]
    assert t.dtype == np.uint16 and t.shape[1] == 32000 and 2 <= S <= guide.MAX_STATES
    assert ((t == DEAD) | (t < S)).all()
    assert (t != DEAD).any(axis=1).all(), "a state without a live token"
    assert (t[:, [0, 1]] == DEAD).all(), "a special token is allowed"
    end = S - 1
    assert (t[end] != DEAD).sum() == 1 and t[end, EOS] == end
    assert set(np.unique(t[:, EOS]).tolist()) <= {end, DEAD}


@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_soundness_every_walk_spells_a_match(tables, pieces, pattern):
    t, longest = tables[pattern], PATTERNS[pattern][0]
    end = t.shape[0] - 1
    rng = np.random.default_rng(len(pattern))
    spelled = set()
    for _ in range(200):
        s, text = 0, b""
        for step in range(longest + 1):
            live = np.nonzero(t[s] != DEAD)[0]
            others = live[live != EOS]
            if t[s, EOS] != DEAD and (others.size == 0 or rng.random() < 0.5):
                s = int(t[s, EOS])
                break
            tok = int(rng.choice(others))
            text += pieces[tok]
            s = int(t[s, tok])
        assert s == end, "a walk of %d steps did not end: %r" % (longest + 1, text)
        assert re.fullmatch(pattern.encode(), text), "%r does not match %s" % (text, pattern)
        spelled.add(text)
    assert len(spelled) >= 3


@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_completeness_every_segmentation_of_a_match_is_accepted(tables, pieces, pattern):
    t, (longest, matching, _) = tables[pattern], PATTERNS[pattern]
    assert len(matching) >= 8
    assert max(len(m) for m in matching) == longest, "the listed matches do not reach the longest match"
    for text in matching:
        assert re.fullmatch(pattern.encode(), text), text
        a, b = _by_bytes(pieces, text), _longest_first(pieces, text)
        assert b"".join(pieces[i] for i in b) == text
        assert _accepts(t, a), "byte by byte: %r" % text
        assert _accepts(t, b), "longest piece first %s: %r" % (b, text)
    if not pattern.startswith("-?"):         # (the vocabulary spells numbers digit by digit)
        assert any(len(_longest_first(pieces, m)) < len(m) for m in matching), "no multi-byte piece was exercised"


@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_rejection(tables, pieces, pattern):
    t, (_, _, wrong) = tables[pattern], PATTERNS[pattern]
    for text in wrong:
        assert not re.fullmatch(pattern.encode(), text), text
        assert not _accepts(t, _by_bytes(pieces, text)), "byte by byte: %r" % text
        assert not _accepts(t, _longest_first(pieces, text)), "longest piece first: %r" % text
    # a special token and a token beyond the vocabulary lead off the track
    assert guide.walk(t, [1])[-1] == guide.OFFTRACK and guide.walk(t, [32000])[-1] == guide.OFFTRACK


def _language(table, limit=10):
    out = set()

    def go(s, prefix):
        assert len(prefix) <= limit
        for tok in np.nonzero(table[s] != DEAD)[0].tolist():
            if tok == EOS:
                out.add(tuple(prefix))
            else:
                go(int(table[s, tok]), prefix + [tok])

    go(0, [])
    return out


def test_from_choices_accepts_exactly_the_choices():
    choices = [[5, 6, 7], [5, 6], [5, 8], [9], [9, 9, 9], [40, 5, 6]]          # overlapping prefixes; [5, 6] and [9] are prefixes of other choices
    t = guide.from_choices(choices, 50)
    end = t.shape[0] - 1
    assert t.dtype == np.uint16 and t.shape == (12, 50)
    assert _language(t) == {tuple(c) for c in choices}
    assert (t[end] != DEAD).sum() == 1 and t[end, EOS] == end
    assert guide.walk(t, [5, 6, EOS, EOS]).tolist() == [0, int(t[0, 5]), int(t[t[0, 5], 6]), end, end]
    assert guide.walk(t, [5, 7, 6]).tolist()[2:] == [guide.OFFTRACK, guide.OFFTRACK]
    assert guide.walk(t, [EOS])[-1] == guide.OFFTRACK                          # no choice is empty
    other = guide.from_choices([[3]], 8, eos_id=7)                             # (another EOS: token 2 means nothing here)
    assert other[1, 7] == 2 and other[2, 7] == 2 and other[1, 2] == DEAD
    for bad in ([], [[]], [[5, EOS]], [[50]], [[-1]]):
        with pytest.raises(ValueError):
            guide.from_choices(bad, 50)


@pytest.mark.parametrize("pattern", [r"a*?", r"a+?", r"a??", r"a{2}?", r"a*+", r"a**", r"(?=a)b", r"(?!a)b", r"(?<=a)b", r"(?i)a", r"(?P<x>a)", r"(a)\1", r"\1",
                                     r"\b", r"\D", r"\x41", r"^a", r"a$", r"a{2,1}", r"a{1001}", r"a{,3}", r"a{x}", r"*a", r"(a", r"a)", r"[a", r"[b-a]",
                                     r"[\d-z]", r"[\w-a]", r"[a-\d]", "[é]", "a\\"])
def test_unsupported_syntax_raises(pattern):
    """the PARSER refuses it (its errors name a byte offset), whatever the vocabulary: over one that spells every byte, so that an empty language cannot
    stand in for a syntax error, from_regex fails with the same error"""
    with pytest.raises(ValueError, match=r" at byte \d+ of "):
        guide._Parser(pattern).parse()
    every_byte = [b"", b"", b""] + [bytes([b]) for b in range(256)]
    with pytest.raises(ValueError, match=r" at byte \d+ of "):
        guide.from_regex(pattern, every_byte)


@pytest.mark.parametrize("pattern", [r"[\d-]", r"[-\d]", r"[\d\-z]", r"[a-c\d]", r"[\s\w]"])
def test_class_escapes_beside_a_literal_hyphen_parse_as_in_re(pattern):
    every_byte = [b"", b"", b""] + [bytes([b]) for b in range(256)]
    t = guide.from_regex(pattern, every_byte)
    allowed = {b for b in range(256) if t[0, b + 3] != DEAD}
    assert allowed == {b for b in range(256) if re.fullmatch(pattern.encode(), bytes([b]))}


def test_empty_languages_and_too_many_states_raise(pieces):
    small = [b"<unk>", b"<s>", b"</s>", b"a", b"b", b"ab", b""]
    assert guide.from_regex(r"(a|b){1,3}", small).shape[1] == 7
    with pytest.raises(ValueError):
        guide.from_regex(r"abc", small)                      # no piece spells a 'c'
    with pytest.raises(ValueError):
        guide.from_regex(r"a", small, special_ids=(0, 1, 2, 3))  # the only piece that spells it is special
    with pytest.raises(ValueError):
        guide.from_regex(r"a{1000}b{1000}a{1000}b{1000}a{97}", small)          # 4097 states before END
    assert guide.from_regex(r"a{1000}b{1000}a{1000}b{1000}a{94}", small).shape[0] <= guide.MAX_STATES


def test_guide_new_argument_errors_never_touch_the_gpu():
    L = api.lib()
    h = C.c_void_p()
    ok = np.zeros((2, 5), dtype=np.uint16)
    new = lambda S, V, a: L.q4_guide_new(C.byref(h), S, V, a.ctypes.data)
    assert new(0, 5, ok) == ERR_ARG and new(4097, 5, ok) == ERR_ARG and new(-1, 5, ok) == ERR_ARG
    assert new(2, 0, ok) == ERR_ARG
    bad = ok.copy()
    bad[1, 3] = 2                                            # neither a state of a two-state guide nor DEAD
    assert new(2, 5, bad) == ERR_ARG
    bad = ok.copy()
    bad[1, :] = DEAD                                         # state 1 has no live entry
    assert new(2, 5, bad) == ERR_ARG
    assert L.q4_guide_new(None, 2, 5, ok.ctypes.data) == ERR_ARG and L.q4_guide_new(C.byref(h), 2, 5, None) == ERR_ARG
    assert L.q4_guide_delete(None) == ERR_ARG
    assert h.value is None
    with pytest.raises(ValueError):
        api.Guide(np.zeros(5, dtype=np.uint16))
