#!/usr/bin/env python3
"""What the reference's test_demo.py asks of its helper modules, parsed with ast (never imported, never copied).

  python tools/gen_golden_demo_calls.py <reference checkout>/test_demo.py

writes tests/golden/demo_calls.json -- names and call shapes only, the data tests/test_shim_and_op.py resolves in shim/:
  utils_aliases         local alias -> module of every `from utils import ...` (test_demo.py:8-10)
  summary_imports       the names imported from utils.model_summary
  attributes            every `<alias>.<name>` it touches, with each call site's positional count and keyword names
  select_model_imports  model_id -> (module, imported names) of the `from models... import ...` lines in select_model()
"""
import ast
import json
import os
import sys

GOLD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")


def extract(src):
    tree = ast.parse(src)
    aliases, from_summary = {}, []
    for node in ast.walk(tree):
        if isinstance(node, ast.ImportFrom) and node.module == "utils":
            for a in node.names:
                aliases[a.asname or a.name] = "utils." + a.name
        if isinstance(node, ast.ImportFrom) and node.module == "utils.model_summary":
            from_summary += [a.name for a in node.names]
    used = {}                                            # (alias, attr) -> list of call sites
    for node in ast.walk(tree):
        if isinstance(node, ast.Attribute) and isinstance(node.value, ast.Name) and node.value.id in aliases:
            used.setdefault((node.value.id, node.attr), [])
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and isinstance(node.func.value, ast.Name) \
                and node.func.value.id in aliases:
            used.setdefault((node.func.value.id, node.func.attr), []).append(
                {"nargs": len(node.args), "keywords": [k.arg for k in node.keywords]})
    sel = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "select_model")
    model_imports = {}
    for node in ast.walk(sel):
        if isinstance(node, ast.If) and isinstance(node.test, ast.Compare) and isinstance(node.test.left, ast.Name) \
                and node.test.left.id == "model_id" and isinstance(node.test.comparators[0], (ast.Constant, ast.UnaryOp)):
            mid = ast.literal_eval(node.test.comparators[0])
            for st in node.body:
                if isinstance(st, ast.ImportFrom):
                    model_imports[str(mid)] = [st.module, [a.name for a in st.names]]
    return {"utils_aliases": aliases, "summary_imports": from_summary,
            "attributes": [{"alias": al, "attr": at, "calls": calls} for (al, at), calls in sorted(used.items())],
            "select_model_imports": model_imports}


if __name__ == "__main__":
    out = extract(open(sys.argv[1]).read())
    with open(os.path.join(GOLD, "demo_calls.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", os.path.join(GOLD, "demo_calls.json"))
