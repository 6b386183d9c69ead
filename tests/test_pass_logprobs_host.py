"""Log-probability records inside prompt and verify passes (q4_set_pass_logprobs, q4_logprob_topk_rows), the parts that need no GPU: the exported
symbols, the switch on handles the library did not build, and the refusals of the row form in front of any launch."""
import ctypes as C
import os
import re

from llama_cu_awq_amd import api

ERR_ARG, ERR_UNSUPPORTED_SIZE = 5, 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["q4_set_pass_logprobs", "q4_get_pass_logprobs", "q4_logprob_topk_rows"]


def test_symbols_in_header_map_and_library():
    header = open(os.path.join(ROOT, "include", "llama2_q4.h")).read()
    exports = open(os.path.join(ROOT, "llama_cu_awq_amd", "csrc", "exports.map")).read()
    patterns = re.findall(r"[\w*]+(?=;)", exports.split("global:")[1].split("local:")[0])
    L = api.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert any(re.fullmatch(p.replace("*", r"\w*"), name) for p in patterns), name
        assert hasattr(L, name) and name in api.SYMBOLS, name


def test_switch_on_null_and_foreign_handles():
    """a NULL Transformer and one the library did not build (zeroed memory of a Transformer's size and more): Q4_ERR_ARG from the setter, 0 from the getter"""
    L = api.lib()
    assert L.q4_set_pass_logprobs(None, 1) == ERR_ARG
    assert L.q4_set_pass_logprobs(None, 0) == ERR_ARG
    assert L.q4_get_pass_logprobs(None) == 0
    foreign = C.create_string_buffer(1 << 16)
    assert L.q4_set_pass_logprobs(foreign, 1) == ERR_ARG
    assert L.q4_get_pass_logprobs(foreign) == 0
    assert foreign.raw == bytes(1 << 16)                    # nothing was written through the handle


def test_row_form_refusals_need_no_launch():
    """q4_logprob_topk's argument and size errors, plus n_rows outside 1 .. 8 and an ld below n or not a multiple of 8 -- all in front of the launch, so the
    (never dereferenced) pointers may be anything non-null"""
    L = api.lib()
    p = C.c_void_p(4096)                                    # non-null, never read: every call below is refused first
    rows = lambda ld, n, n_rows, k, ids=p, top=p, logits=p, lse=p, tlp=p: L.q4_logprob_topk_rows(logits, ld, n, n_rows, k, None, lse, tlp, ids, top)
    for n_rows in (0, -1, 9, 1 << 20):
        assert rows(512, 512, n_rows, 5) == ERR_ARG, n_rows
    for ld, n in ((504, 512), (511, 512), (513, 512), (516, 513), (519, 513), (0, 8), (-8, 8), (12, 8)):
        assert rows(ld, n, 3, 1) == ERR_ARG, (ld, n)
    assert rows(520, 513, 3, 21) == ERR_ARG                 # top_k above Q4_MAX_TOP_LOGPROBS
    assert rows(8, 8, 3, 9) == ERR_ARG                      # top_k above n
    assert rows(8, 8, 3, -1) == ERR_ARG
    assert rows(8, 0, 3, 0) == ERR_ARG
    assert rows(512, 512, 3, 5, logits=None) == ERR_ARG
    assert rows(512, 512, 3, 5, lse=None) == ERR_ARG
    assert rows(512, 512, 3, 5, tlp=None) == ERR_ARG
    assert rows(512, 512, 3, 5, ids=None) == ERR_ARG
    assert rows(512, 512, 3, 5, top=None) == ERR_ARG
    # the looping path's candidate list (q4_logprob_topk's size error): about 311,000 logits at top_k 20
    assert rows(400000, 400000, 2, 20) == ERR_UNSUPPORTED_SIZE
    assert L.q4_logprob_topk(p, 400000, 20, None, p, p, p, p) == ERR_UNSUPPORTED_SIZE


def test_python_surface():
    import inspect
    sig = inspect.signature(api.Transformer.__init__)
    assert sig.parameters["pass_logprobs"].default is False
    assert callable(api.Transformer.set_pass_logprobs) and callable(api.Transformer.pass_logprobs) and callable(api.logprob_topk_rows)
