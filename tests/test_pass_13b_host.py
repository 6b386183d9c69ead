"""Prompt and verify passes for the Llama-2-13B shape (q4_set_pass_13b), the parts that need no GPU: the exported symbols, the switch on
handles the library did not build, the CLI variable's parser and the Python surface."""
import ctypes as C
import inspect
import os
import re

import pytest

from llama_cu_awq_amd import api

ERR_ARG = 5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["q4_set_pass_13b", "q4_get_pass_13b", "q4_parse_pass_13b"]


def test_symbols_in_header_map_and_library():
    header = open(os.path.join(ROOT, "include", "llama2_q4.h")).read()
    exports = open(os.path.join(ROOT, "llama_cu_awq_amd", "csrc", "exports.map")).read()
    patterns = re.findall(r"[\w*]+(?=;)", exports.split("global:")[1].split("local:")[0])
    L = api.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert any(re.fullmatch(p.replace("*", r"\w*"), name) for p in patterns), name
        assert hasattr(L, name) and name in api.SYMBOLS, name
    wrapper = open(os.path.join(ROOT, "include", "llama2_q4.hpp")).read()
    assert "q4_set_pass_13b" in wrapper and "q4_get_pass_13b" in wrapper


def test_switch_on_null_and_foreign_handles():
    """a NULL Transformer and one the library did not build (zeroed memory of a Transformer's size and more): Q4_ERR_ARG from the setter, 0 from the getter"""
    L = api.lib()
    assert L.q4_set_pass_13b(None, 1) == ERR_ARG
    assert L.q4_set_pass_13b(None, 0) == ERR_ARG
    assert L.q4_get_pass_13b(None) == 0
    foreign = C.create_string_buffer(1 << 16)
    assert L.q4_set_pass_13b(foreign, 1) == ERR_ARG
    assert L.q4_get_pass_13b(foreign) == 0
    assert foreign.raw == bytes(1 << 16)                    # nothing was written through the handle


@pytest.mark.parametrize("text,want", [(b"0", 0), (b"1", 1)])
def test_cli_text_accepted(text, want):
    on = C.c_int(-7)
    assert api.lib().q4_parse_pass_13b(text, C.byref(on)) == 0 and on.value == want


@pytest.mark.parametrize("text", [b"", b"2", b"-1", b" 1", b"1 ", b"01", b"10", b"on", b"true", b"1x", b"+1"])
def test_cli_text_rejected(text):
    """Q4_PASS_13B is "0" or "1" and nothing else; a rejected text leaves *on alone"""
    on = C.c_int(-7)
    L = api.lib()
    assert L.q4_parse_pass_13b(text, C.byref(on)) == ERR_ARG and on.value == -7
    assert L.q4_parse_pass_13b(None, C.byref(on)) == ERR_ARG and L.q4_parse_pass_13b(b"1", None) == ERR_ARG


def test_python_surface():
    sig = inspect.signature(api.Transformer.__init__)
    assert sig.parameters["pass_13b"].default is False
    assert callable(api.Transformer.set_pass_13b) and callable(api.Transformer.pass_13b)
