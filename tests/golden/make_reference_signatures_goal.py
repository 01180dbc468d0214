#!/usr/bin/env python3
"""Signature fixture of tests/test_goal_python_cpu.py (reference_signatures_goal.json), produced by PARSING the reference sources (ast; nothing is imported
or executed, and no source text is kept): the parameter names and the defaults (literals only; anything else is recorded as the
string "<expr>") of AstarPlanner.build_object_frontiers, generate_candidate_adv_object, global_planning, global_object_planning
(planning/astar.py) and NavTester.action_planning_object_adv (tester_gaussians_navigation.py).  Run from the repo root:
    python tests/golden/make_reference_signatures_goal.py <path of the reference checkout>
"""
import ast
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TARGETS = [
    ("planning/astar.py", "AstarPlanner", ("build_object_frontiers", "generate_candidate_adv_object", "global_planning", "global_object_planning")),
    ("tester_gaussians_navigation.py", "NavTester", ("action_planning_object_adv",)),
]


def signature(fn):
    a = fn.args
    pos = [x.arg for x in a.posonlyargs + a.args]
    if pos and pos[0] in ("self", "cls"):
        pos = pos[1:]
    defaults = []
    for d in a.defaults:
        try:
            defaults.append(ast.literal_eval(d))
        except ValueError:
            defaults.append("<expr>")
    return dict(pos=pos, defaults=defaults, kwonly=[x.arg for x in a.kwonlyargs], vararg=a.vararg is not None, kwarg=a.kwarg is not None)


def main(ref):
    out = {}
    for path, cls, names in TARGETS:
        tree = ast.parse(open(os.path.join(ref, path)).read(), filename=path)
        node = next(n for n in ast.walk(tree) if isinstance(n, ast.ClassDef) and n.name == cls)
        methods = {n.name: n for n in node.body if isinstance(n, ast.FunctionDef)}
        out[cls] = dict(file=path, methods={n: signature(methods[n]) for n in names})
    with open(os.path.join(HERE, "reference_signatures_goal.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"{sum(len(c['methods']) for c in out.values())} method signatures")


if __name__ == "__main__":
    main(sys.argv[1])
