"""Python restatements for verify passes under the temperature / top-p sampler ("Under the sampler"): the sampler's xorshift coin stream
(sampler.h:31-40) and its inverse -- the state from which the next coin is a chosen value --, the coin bookkeeping of the token loop around a pass, and
the accept rule on given tokens."""
import ctypes as C

MASK = (1 << 64) - 1
MUL = 0x2545F4914F6CDD1D
MUL_INV = pow(MUL, -1, 1 << 64)


class SamplerStruct(C.Structure):      # include/llama2_q4.h Sampler
    _fields_ = [("vocab_size", C.c_int), ("indices", C.c_void_p), ("scan", C.c_void_p), ("sort", C.c_void_p), ("bytes_scan", C.c_size_t),
                ("bytes_sort", C.c_size_t), ("temperature", C.c_float), ("topp", C.c_float), ("rng_state", C.c_ulonglong)]


def sampler_struct(handle):
    return C.cast(handle, C.POINTER(SamplerStruct)).contents


def next_state(state):
    """random_u32's update of the state, sampler.h:32-34"""
    state ^= state >> 12
    state ^= (state << 25) & MASK
    state ^= state >> 27
    return state


def coin_of(state):
    """(coin, next state): random_f32, sampler.h:31-40 -- the upper 24 bits of the product's upper half, over 2^24"""
    state = next_state(state)
    return (((state * MUL) & MASK) >> 40) / 16777216.0, state


def draw(state, n):
    """n coins from `state`: (coins, state behind them)"""
    coins = []
    for _ in range(n):
        c, state = coin_of(state)
        coins.append(c)
    return coins, state


def _undo_right(x, k):          # x = y ^ (y >> k)  ->  y
    y, s = x, k
    while s < 64:
        y ^= y >> s
        s *= 2
    return y


def _undo_left(x, k):           # x = y ^ (y << k)  ->  y
    y, s = x, k
    while s < 64:
        y = (y ^ (y << s)) & MASK
        s *= 2
    return y


def state_for_coin(k24, low=0x5A5A5A5A5A):
    """A state whose NEXT coin is k24 / 2^24 exactly (0 <= k24 < 2^24): the multiplication by an odd constant and the three xor-shifts are bijections
    of the 64-bit words, so the product with k24 in its top 24 bits (and any low 40 bits) has exactly one state in front of it."""
    assert 0 <= k24 < (1 << 24) and 0 < low < (1 << 40)
    after = (((k24 << 40) | low) * MUL_INV) & MASK
    state = _undo_right(_undo_left(_undo_right(after, 27), 25), 12)
    assert state != 0 and next_state(state) == after and coin_of(state)[0] == k24 / 16777216.0
    return state


def pass_coins(state, pos, n_draft, m):
    """The token loop's bookkeeping around a pass at `pos` with n_draft drafts of which m are accepted: the state is saved, n_draft + 1 coins are drawn
    for the ring entries pos .. pos + n_draft, the state is put back, and m + 1 coins are drawn -- one per position that ran. Returns (ring entries as
    {position: coin}, the state behind the pass)."""
    coins, _ = draw(state, n_draft + 1)
    _, after = draw(state, m + 1)
    return {pos + i: c for i, c in enumerate(coins)}, after


def replay_coins(seed, n_prompt, passes, groups, steps):
    """The coin each position's step samples with in a run of `steps` positions from `seed`, drawn (a) one per position, as the run without passes
    draws them, and (b) through the loop's bookkeeping with `passes` = [(pos, n_draft, accepted)] and step groups between them (groups(pos) -> steps
    queued at pos). Returns (a, b, state_a, state_b): b must equal a at every position that ran, and the states must be equal."""
    a, state_a = draw(seed, steps)
    b = {}
    state = seed
    by_pos = {p[0]: p for p in passes}
    pos = 0
    while pos < steps:
        if pos in by_pos:
            _, d, m = by_pos[pos]
            ring, state = pass_coins(state, pos, d, m)
            b.update(ring)                                   # (entries above pos + m are stale: whatever runs there next rewrites them)
            pos += m + 1
        else:
            k = 1 if pos < n_prompt - 1 else min(groups(pos), steps - pos)
            coins, state = draw(state, k)
            for i, c in enumerate(coins):
                b[pos + i] = c
            pos += k
    return a, b, state_a, state


def accept_tokens(tokens, drafts):
    """m: the number of leading drafts that equal the given token of the row in front of them"""
    m = 0
    while m < len(drafts) and int(tokens[m]) == int(drafts[m]):
        m += 1
    return m
