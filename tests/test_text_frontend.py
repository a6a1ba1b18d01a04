"""CPU: the text front-end wire format against the stored outputs of the reference's own classes and against a
committed golden id map."""
import json
import os

import pytest
import torch

from conftest import GOLDEN
from oracle.ref_harness import REF_ROOT, load_reference, reference_available
from valle_amd.text import TextTokenCollater, get_text_token_collater, read_symbol_table, write_symbol_table

SYMS = {"<eps>": 0, "a": 1, "ʃ": 2, "b": 3, "ɔː": 4, "_": 5, ",": 6, "ð": 7}
TEXTS = [["a", "ʃ", "_", "b"], ["ð"], ["ɔː", ",", "a", "a", "b", "_"]]


def test_symbol_table_roundtrip(tmp_path):
    p = str(tmp_path / "unique_text_tokens.k2symbols")
    write_symbol_table(p, SYMS)
    assert read_symbol_table(p) == SYMS
    assert open(p, encoding="utf-8").read().splitlines()[:2] == ["<eps> 0", "a 1"]


def test_collater_matches_committed_golden(tmp_path):
    p = str(tmp_path / "t.k2symbols")
    write_symbol_table(p, SYMS)
    tokens, lens = get_text_token_collater(p)(TEXTS)
    g = json.load(open(os.path.join(GOLDEN, "text_collater.json")))
    assert tokens.tolist() == g["tokens"] and lens.tolist() == g["lens"]
    assert tokens.dtype == torch.int64 and lens.dtype == torch.int32  # collation.py:100-111
    assert tokens[0, 0] == 1 and tokens[1, 2] == 2 and tokens[1, 3] == 0  # <bos>=1, <eos>=2, <pad>=0


def _reference_outputs(path):
    """What the reference's own SymbolTable.from_file and get_text_token_collater return for `path` and TEXTS: needs the
    reference tree (build container only), used to (re)write tests/golden/text_reference.json under WRITE_GOLDEN."""
    load_reference()
    import importlib
    import importlib.util

    # valle.utils imports icefall.utils (stubbed by the harness); valle.data is a stub package -> load collation.py by path
    st = importlib.import_module("valle.utils.symbol_table")
    spec = importlib.util.spec_from_file_location("ref_collation", os.path.join(REF_ROOT, "valle", "data", "collation.py"))
    col = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(col)
    rt, rl = col.get_text_token_collater(path)(TEXTS)
    return {"sym2id": dict(st.SymbolTable.from_file(path)._sym2id), "tokens": rt.tolist(), "lens": rl.tolist(),
            "tokens_dtype": str(rt.dtype), "lens_dtype": str(rl.dtype)}


def test_collater_matches_reference_classes(tmp_path):
    """Against the outputs of the reference's own classes for the same symbol table and texts, stored in
    tests/golden/text_reference.json (rewritten from the reference tree with WRITE_GOLDEN=1 where it is present)."""
    p = str(tmp_path / "t.k2symbols")
    write_symbol_table(p, SYMS)
    golden = os.path.join(GOLDEN, "text_reference.json")
    if os.environ.get("WRITE_GOLDEN") and reference_available():
        ref = _reference_outputs(p)
        with open(golden, "w", encoding="utf-8") as fh:
            json.dump(ref, fh, ensure_ascii=False)
        with open(os.path.join(GOLDEN, "text_collater.json"), "w") as fh:
            json.dump({"tokens": ref["tokens"], "lens": ref["lens"]}, fh)
    with open(golden, encoding="utf-8") as fh:
        ref = json.load(fh)
    assert ref["sym2id"] == read_symbol_table(p)
    tokens, lens = get_text_token_collater(p)(TEXTS)
    assert tokens.tolist() == ref["tokens"] and lens.tolist() == ref["lens"]
    assert str(tokens.dtype) == ref["tokens_dtype"] and str(lens.dtype) == ref["lens_dtype"]
