#!/usr/bin/env python
"""Generates tests/golden/reference_surface.json: the config / CLI surface of the reference, as data.

`python tests/golden/make_reference_surface.py <reference checkout>` `ast`-parses (imports and executes nothing of) the reference's
hparams.py:6-176,190-192 and the three argparse blocks (generate.py:51-79, synthesizer.py:371-380, train_vocoder.py:34-58) and
writes what tests/test_reference_surface.py compares this repo against: every hparam name with its default (value and Python
type), the values of the three derived hparams, every flag with its type / default / required / action, and which of the names
the post-parse rules of generate.py:45-49,72-77 mention appear in its `raise` statements.  Names and literal values only; no
source text is stored."""
import ast
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from test_reference_surface import CLI_FILES, RAISE_NAMES, _argparse_surface, _const, _parse, _raises_of   # noqa: E402


def _hparams_of(ref):
    tree = _parse(os.path.join(ref, "hparams.py"))
    values = None
    derived = {}
    for node in ast.walk(tree):
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == "HParams":
            values = {kw.arg: _const(kw.value) for kw in node.keywords}
    assert values, "tf.contrib.training.HParams(...) call not found in the reference's hparams.py"
    # hparams.py:190-192: the `else` branch of `if hparams.use_lws` (use_lws is False by default)
    for node in ast.walk(tree):
        if isinstance(node, ast.If) and isinstance(node.test, ast.Attribute) and node.test.attr == "use_lws":
            for st in node.orelse:
                if isinstance(st, ast.Assign) and isinstance(st.targets[0], ast.Attribute):
                    derived[st.targets[0].attr] = _eval_derived(st.value, values)
    return values, derived


def _eval_derived(expr, hp):
    """hparams.py:190-192 right-hand sides: arithmetic over hparams.<name> and int(...)"""
    if isinstance(expr, ast.Call) and isinstance(expr.func, ast.Name) and expr.func.id == "int":
        return int(_eval_derived(expr.args[0], hp))
    if isinstance(expr, ast.BinOp):
        a, b = _eval_derived(expr.left, hp), _eval_derived(expr.right, hp)
        return {ast.Add: a + b, ast.Sub: a - b, ast.Mult: a * b, ast.Div: a / b}[type(expr.op)]
    if isinstance(expr, ast.Attribute):
        return hp[expr.attr]
    return _const(expr)


def main(ref):
    hparams, derived = _hparams_of(ref)
    raises = _raises_of(os.path.join(ref, "generate.py"))
    out = {
        "hparams": hparams,
        "derived": derived,
        "cli": {f: _argparse_surface(os.path.join(ref, f)) for f in CLI_FILES},
        "generate_py_raises": [n for n in RAISE_NAMES if n in raises],
    }
    text = json.dumps(out, indent=1, sort_keys=True, allow_nan=False) + "\n"
    path = os.path.join(HERE, "reference_surface.json")
    with open(path, "w", encoding="utf-8") as fh:
        fh.write(text)
    print("wrote", path, "(%d hparams, %d derived, %s flags)" % (len(hparams), len(derived),
                                                                 {f: len(v) for f, v in out["cli"].items()}))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit("usage: make_reference_surface.py <reference checkout>")
    main(sys.argv[1])
