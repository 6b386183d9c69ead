"""Host-side compilers for guided decoding: token automata for `api.Guide` (numpy only, no GPU).

A table is a uint16 array [S, V]: table[s, i] is the state behind token i in state s, or DEAD where state s forbids the token. State 0 starts.

    from_choices(sequences, vocab_size)   "answer with one of these token sequences"
    from_regex(pattern, pieces)           a regular expression over the BYTES of the generated text, lifted to the tokenizer's pieces
    walk(table, tokens)                   the states a token sequence passes through (what the device keeps by position)
    forced_run(table, state, max_draft)   the tokens the automaton forces from a state: what the token loop drafts with q4_set_pass_stages on

Both compilers end a match with EOS: a state where the text may end allows `eos_id`, which leads to a last state END that allows only EOS.
"""
import numpy as np

DEAD = 0xFFFF            # Q4_GUIDE_DEAD
NONE, OFFTRACK = -1, -2  # Q4_GUIDE_NONE, Q4_GUIDE_OFFTRACK
MAX_STATES = 4096        # Q4_GUIDE_MAX_STATES

_MAX_REPEAT = 1000       # {m,n} beyond this is refused: the automaton is built by copying
_MAX_DFA = 20000         # byte-DFA states before trimming


def walk(table, tokens, start=0):
    """[start, s1, .., sk] for the k tokens: s_j = table[s_{j-1}, token_j]; OFFTRACK from the first forbidden (or out-of-range) token on."""
    table = np.asarray(table)
    out = np.empty(len(tokens) + 1, dtype=np.int32)
    s = int(start)
    out[0] = s
    for j, t in enumerate(tokens):
        if s != OFFTRACK:
            e = int(table[s, t]) if 0 <= s < table.shape[0] and 0 <= int(t) < table.shape[1] else DEAD
            s = e if e != DEAD else OFFTRACK
        out[j + 1] = s
    return out


def forced_run(table, state, max_draft, eos_id=2):
    """The restatement of q4_guide_forced_run: while the state has exactly ONE live token, that token, and on to the state behind it. At most max_draft
    tokens; the run ends behind an EOS, at a state with zero, two or more live tokens, and is empty for NONE, OFFTRACK or a state outside the table."""
    table = np.asarray(table)
    out = []
    s = int(state)
    while len(out) < max_draft and 0 <= s < table.shape[0]:
        live = np.flatnonzero(table[s] != DEAD)
        if live.shape[0] != 1:
            break
        t = int(live[0])
        out.append(t)
        if t == eos_id:
            break
        s = int(table[s, t])
    return np.asarray(out, dtype=np.int32)


def from_choices(sequences, vocab_size, eos_id=2):
    """A trie over token-id sequences: the accepted language is exactly the sequences, each followed by EOS (then EOS for ever)."""
    seqs = [list(map(int, s)) for s in sequences]
    if not seqs or any(len(s) == 0 for s in seqs):
        raise ValueError("from_choices: at least one choice, none of them empty")
    if not 0 <= eos_id < vocab_size:
        raise ValueError("from_choices: eos_id outside the vocabulary")
    children, terminal = [{}], [False]
    for s in seqs:
        node = 0
        for t in s:
            if not 0 <= t < vocab_size or t == eos_id:
                raise ValueError("from_choices: token %d is EOS or outside the vocabulary" % t)
            if t not in children[node]:
                children.append({})
                terminal.append(False)
                children[node][t] = len(children) - 1
            node = children[node][t]
        terminal[node] = True
    end = len(children)
    if end + 1 > MAX_STATES:
        raise ValueError("from_choices: %d states, a guide holds %d" % (end + 1, MAX_STATES))
    table = np.full((end + 1, vocab_size), DEAD, dtype=np.uint16)
    for node, ch in enumerate(children):
        for t, nxt in ch.items():
            table[node, t] = nxt
        if terminal[node]:
            table[node, eos_id] = end
    table[end, eos_id] = end
    return table


# ---- the regular-expression subset -> AST ----------------------------------------------------------------------------------------------------------
# Parsed over the pattern's UTF-8 bytes, with the meaning Python's `re` gives the same bytes pattern under fullmatch: a non-ASCII literal is its bytes
# one after another (a quantifier directly behind it binds the LAST byte -- group it, "(?:é)?", to make the character optional).
def _mask(*bytes_or_ranges):
    m = 0
    for b in bytes_or_ranges:
        if isinstance(b, tuple):
            for c in range(b[0], b[1] + 1):
                m |= 1 << c
        else:
            m |= 1 << b
    return m


_ALL = (1 << 256) - 1
_DIGIT = _mask((0x30, 0x39))
_WORD = _DIGIT | _mask((0x41, 0x5A), (0x61, 0x7A), 0x5F)
_SPACE = _mask(0x20, 0x09, 0x0A, 0x0D, 0x0C, 0x0B)
_CLASS_ESC = {ord("d"): _DIGIT, ord("w"): _WORD, ord("s"): _SPACE}
_CHAR_ESC = {ord("n"): 0x0A, ord("t"): 0x09}


class _Parser:
    def __init__(self, pattern):
        self.p = pattern.encode("utf-8") if isinstance(pattern, str) else bytes(pattern)
        self.i = 0

    def fail(self, what):
        raise ValueError("from_regex: %s at byte %d of %r" % (what, self.i, self.p))

    def peek(self):
        return self.p[self.i] if self.i < len(self.p) else None

    def parse(self):
        node = self.alt()
        if self.i != len(self.p):
            self.fail("unbalanced ')'")
        return node

    def alt(self):
        branches = [self.cat()]
        while self.peek() == ord("|"):
            self.i += 1
            branches.append(self.cat())
        return branches[0] if len(branches) == 1 else ("alt", branches)

    def cat(self):
        items = []
        while self.peek() is not None and self.peek() not in (ord("|"), ord(")")):
            items.append(self.repeat())
        return ("cat", items)

    def repeat(self):
        node = self.atom()
        c = self.peek()
        if c is None or c not in b"*+?{":
            return node
        if c == ord("*"):
            lo, hi = 0, None
            self.i += 1
        elif c == ord("+"):
            lo, hi = 1, None
            self.i += 1
        elif c == ord("?"):
            lo, hi = 0, 1
            self.i += 1
        else:
            lo, hi = self.braces()
        c = self.peek()
        if c is not None and c in b"*+?{":
            self.fail("lazy, possessive and stacked quantifiers are not supported")
        return ("rep", node, lo, hi)

    def number(self):
        j = self.i
        while self.peek() is not None and 0x30 <= self.peek() <= 0x39:
            self.i += 1
        return int(self.p[j:self.i]) if self.i > j else None

    def braces(self):
        self.i += 1
        lo = self.number()
        if lo is None:
            self.fail("'{' without a count")
        hi = lo
        if self.peek() == ord(","):
            self.i += 1
            hi = self.number()
        if self.peek() != ord("}"):
            self.fail("malformed '{m,n}'")
        self.i += 1
        if (hi is not None and hi < lo) or max(lo, hi or 0) > _MAX_REPEAT:
            self.fail("repeat counts must satisfy m <= n <= %d" % _MAX_REPEAT)
        return lo, hi

    def escape(self, in_class):
        """behind a backslash: ('set', mask) for \\d \\w \\s, else ('byte', b)"""
        c = self.peek()
        if c is None:
            self.fail("a trailing backslash")
        self.i += 1
        if c in _CLASS_ESC:
            return ("set", _CLASS_ESC[c])
        if c in _CHAR_ESC:
            return ("byte", _CHAR_ESC[c])
        if c < 0x80 and not (chr(c).isalnum() or c == ord("_")):
            return ("byte", c)
        self.i -= 1
        self.fail("unsupported escape")

    def atom(self):
        c = self.peek()
        self.i += 1
        if c == ord("("):
            if self.peek() == ord("?"):
                if self.p[self.i:self.i + 2] != b"?:":
                    self.fail("look-around, flags and named groups are not supported")
                self.i += 2
            node = self.alt()
            if self.peek() != ord(")"):
                self.fail("missing ')'")
            self.i += 1
            return node
        if c == ord("["):
            return ("set", self.char_class())
        if c == ord("."):
            return ("set", _ALL & ~(1 << 0x0A))
        if c == ord("\\"):
            kind, v = self.escape(False)
            return ("set", v if kind == "set" else 1 << v)
        if c in b"*+?{":
            self.i -= 1
            self.fail("nothing to repeat")
        if c in b"^$":
            self.i -= 1
            self.fail("anchors are not supported (the pattern is a full match)")
        return ("set", 1 << c)

    def char_class(self):
        negate = self.peek() == ord("^")
        if negate:
            self.i += 1
        m, first = 0, True
        while True:
            c = self.peek()
            if c is None:
                self.fail("missing ']'")
            if c == ord("]") and not first:
                self.i += 1
                break
            first = False
            self.i += 1
            if c >= 0x80:
                self.i -= 1
                self.fail("non-ASCII characters inside a class are not supported")
            if c == ord("\\"):
                kind, v = self.escape(True)
                if kind == "set":
                    if self.peek() == ord("-") and self.i + 1 < len(self.p) and self.p[self.i + 1] != ord("]"):
                        self.fail("a class escape cannot start a range")
                    m |= v
                    continue
                c = v
            if self.peek() == ord("-") and self.i + 1 < len(self.p) and self.p[self.i + 1] != ord("]"):
                self.i += 1
                d = self.peek()
                self.i += 1
                if d == ord("\\"):
                    kind, d = self.escape(True)
                    if kind == "set":
                        self.fail("a class escape cannot end a range")
                if d >= 0x80 or d < c:
                    self.fail("bad character range")
                m |= _mask((c, d))
            else:
                m |= 1 << c
        return (_ALL & ~m) if negate else m


# ---- AST -> NFA (Thompson) -> byte DFA (subsets) ---------------------------------------------------------------------------------------------------
class _Nfa:
    def __init__(self):
        self.eps, self.edges = [], []          # per state: epsilon targets; (mask, target) byte edges

    def state(self):
        self.eps.append([])
        self.edges.append([])
        return len(self.eps) - 1

    def build(self, node):
        """(start, end) of the fragment"""
        kind = node[0]
        if kind == "set":
            a, b = self.state(), self.state()
            self.edges[a].append((node[1], b))
            return a, b
        if kind == "cat":
            a = b = self.state()
            for item in node[1]:
                s, e = self.build(item)
                self.eps[b].append(s)
                b = e
            return a, b
        if kind == "alt":
            a, b = self.state(), self.state()
            for item in node[1]:
                s, e = self.build(item)
                self.eps[a].append(s)
                self.eps[e].append(b)
            return a, b
        _, sub, lo, hi = node
        a = b = self.state()
        for _ in range(lo):
            s, e = self.build(sub)
            self.eps[b].append(s)
            b = e
        if hi is None:                         # sub*
            s, e = self.build(sub)
            loop = self.state()
            self.eps[b].append(loop)
            self.eps[loop].append(s)
            self.eps[e].append(loop)
            return a, loop
        end = self.state()
        for _ in range(hi - lo):               # (sub(sub(...)?)?)?
            self.eps[b].append(end)
            s, e = self.build(sub)
            self.eps[b].append(s)
            b = e
        self.eps[b].append(end)
        return a, end

    def closure(self, states):
        seen, stack = set(states), list(states)
        while stack:
            for t in self.eps[stack.pop()]:
                if t not in seen:
                    seen.add(t)
                    stack.append(t)
        return frozenset(seen)


def _byte_dfa(pattern):
    """(delta int32 [Q + 1, 256] with Q the sink row, accepting bool [Q + 1]); state 0 starts; only states that can still reach acceptance are kept"""
    nfa = _Nfa()
    start, end = nfa.build(_Parser(pattern).parse())
    first = nfa.closure([start])
    index, order, rows = {first: 0}, [first], []
    # bytes that no edge of the automaton tells apart share their transitions: one subset step per class of bytes
    masks = sorted({m for edges in nfa.edges for m, _ in edges})
    classes = {}
    for b in range(256):
        classes.setdefault(tuple((m >> b) & 1 for m in masks), []).append(b)
    classes = list(classes.values())
    k = 0
    while k < len(order):
        edges = [e for s in order[k] for e in nfa.edges[s]]
        row, cache = [-1] * 256, {}
        for members in classes:
            key = tuple(t for m, t in edges if (m >> members[0]) & 1)
            if not key:
                continue
            if key not in cache:
                target = nfa.closure(key)
                if target not in index:
                    if len(order) >= _MAX_DFA:
                        raise ValueError("from_regex: the pattern needs more than %d byte states" % _MAX_DFA)
                    index[target] = len(order)
                    order.append(target)
                cache[key] = index[target]
            for b in members:
                row[b] = cache[key]
        rows.append(row)
        k += 1
    delta = np.array(rows, dtype=np.int32)
    accept = np.array([end in s for s in order], dtype=bool)
    # states from which acceptance is reachable
    src, dst = np.nonzero(delta >= 0)[0], delta[delta >= 0]
    before = {}
    for a, b in np.unique(np.stack([src, dst], axis=1), axis=0).tolist():
        before.setdefault(b, []).append(a)
    good = accept.copy()
    stack = np.nonzero(accept)[0].tolist()
    while stack:
        for a in before.get(stack.pop(), ()):
            if not good[a]:
                good[a] = True
                stack.append(a)
    if not good[0]:
        raise ValueError("from_regex: the pattern matches nothing")
    new = np.full(len(order) + 1, -1, dtype=np.int32)
    new[:-1][good] = np.arange(int(good.sum()), dtype=np.int32)
    q = int(good.sum())
    d = new[delta[good]]                       # (delta -1 indexes the last entry, -1)
    d[d < 0] = q
    d = np.vstack([d, np.full((1, 256), q, dtype=np.int32)])
    return d, np.append(accept[good], False)


def from_regex(pattern, pieces, eos_id=2, special_ids=(0, 1, 2)):
    """The token automaton of a regular expression over the bytes of the generated text (a full match; EOS ends it). pieces: the vocabulary's raw
    bytes by token id (api.Tokenizer.pieces()). Tokens in special_ids and tokens with an empty piece are never allowed, except EOS where the text may end.

    Subset: literals and backslash-escaped punctuation, \\d \\w \\s \\n \\t, '.' (any byte but newline), classes with ranges and negation, ( ), (?: ),
    |, * + ?, {m} {m,} {m,n}; non-ASCII literals as their UTF-8 bytes. Anything else -- lazy quantifiers, back-references, look-around, flags, anchors --
    raises ValueError, as do a pattern no token sequence can satisfy and one that needs more than 4095 states."""
    V = len(pieces)
    if not 0 <= eos_id < V:
        raise ValueError("from_regex: eos_id outside the vocabulary")
    delta, accept = _byte_dfa(pattern)
    Q = delta.shape[0] - 1                     # row Q is the sink
    lens = np.array([len(p) for p in pieces], dtype=np.int32)
    usable = lens > 0
    usable[[i for i in special_ids if 0 <= i < V]] = False
    L = int(lens[usable].max()) if usable.any() else 0
    padded = np.zeros((V, max(L, 1)), dtype=np.uint8)
    for i in np.nonzero(usable)[0]:
        padded[i, :lens[i]] = np.frombuffer(pieces[i], dtype=np.uint8)
    # the lift, one byte position at a time over every (state, token) pair: cur[q, i] = delta*(q, piece_i[:j])
    cur = np.repeat(np.arange(Q, dtype=np.int32)[:, None], V, axis=1)
    cur[:, ~usable] = Q
    for j in range(L):
        cols = np.nonzero(usable & (lens > j))[0]
        cur[:, cols] = delta[cur[:, cols], padded[cols, j][None, :]]
    live = cur < Q
    # states left with no live token go, to a fixpoint (an accepting state keeps EOS); then what the start state cannot reach
    keep = np.ones(Q, dtype=bool)
    while True:
        live &= np.append(keep, False)[cur]
        now = keep & (live.any(axis=1) | accept[:Q])
        if (now == keep).all():
            break
        keep = now
    if not keep[0]:
        raise ValueError("from_regex: no sequence of tokens satisfies the pattern")
    reach = np.zeros(Q, dtype=bool)
    reach[0] = True
    frontier = [0]
    while frontier:
        nxt = np.unique(cur[frontier][live[frontier]])
        frontier = [int(s) for s in nxt if not reach[s]]
        reach[frontier] = True
    keep &= reach
    n = int(keep.sum())
    if n > MAX_STATES - 1:
        raise ValueError("from_regex: %d states remain, a guide holds %d and END" % (n, MAX_STATES - 1))
    new = np.full(Q + 1, DEAD, dtype=np.int64)
    new[:Q][keep] = np.arange(n)
    table = np.full((n + 1, V), DEAD, dtype=np.uint16)
    body = new[cur[keep]]
    body[~live[keep]] = DEAD
    table[:n] = body.astype(np.uint16)
    table[:n, eos_id][accept[:Q][keep]] = n
    table[n, eos_id] = n
    return table
