#!/usr/bin/env python3
"""Signature fixture of tests/test_graft_signatures_vs_reference.py, produced by PARSING the reference sources (ast; nothing is
imported or executed, and no source text is kept): for every method that a product mixin's `install()` grafts and the reference
class defines, its parameter list (names, number of defaults, keyword-only names, *args / **kwargs); and every call of the
Fisher methods in the reference's tester (line, number of positional arguments, keyword names).  Run from the repo root:
    python tests/golden/make_reference_signatures.py <path of the reference checkout>
"""
import ast
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from test_graft_signatures_vs_reference import (CALLED, PKG, TARGETS, TESTER, _classes, _grafted_names,  # noqa: E402
                                                _methods, _signature)

ref = sys.argv[1]
classes = {}
for ref_file, ref_cls, our_file, mixins in TARGETS:
    ref_methods = _methods(_classes(os.path.join(ref, ref_file))[ref_cls])
    ours = _classes(os.path.join(PKG, our_file))
    grafted = [n for m in mixins for n in _grafted_names(_methods(ours[m])["install"])]
    sigs = {}
    for name in grafted:
        if name in ref_methods:
            pos, ndef, kwonly, var, kw = _signature(ref_methods[name])
            sigs[name] = dict(pos=pos, ndefaults=ndef, kwonly=kwonly, vararg=var, kwarg=kw)
    classes[ref_cls] = dict(file=ref_file, methods=sigs)

tree = ast.parse(open(os.path.join(ref, TESTER)).read())
attrs = {n.attr for n in ast.walk(tree) if isinstance(n, ast.Attribute)}
calls = [dict(name=n.func.attr, line=n.lineno, n_args=len(n.args), keywords=[k.arg for k in n.keywords])
         for n in ast.walk(tree) if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute) and n.func.attr in CALLED]
out = dict(classes=classes, call_sites=dict(file=TESTER, attributes_used=sorted(attrs & set(CALLED)),
                                            calls=sorted(calls, key=lambda c: (c["line"], c["name"]))))
with open(os.path.join(HERE, "reference_signatures.json"), "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(f"{sum(len(c['methods']) for c in classes.values())} method signatures, {len(calls)} call sites")
