"""mimsem_amd/device.py is the only guard between a Python caller and the C ABI, which takes raw addresses and cannot check a length.
These checks read its source: no argument check of Engine may vanish under `python -O`, an address may come from the checking helpers
only, and no wrapper may hand an address to the library without having gone through them."""
import ast
import pathlib

SRC = pathlib.Path(__file__).resolve().parents[1] / "mimsem_amd" / "device.py"
ADDRESS_HELPERS = {"_ptr", "_ps", "_vec", "_blocks"}                    # the only functions that may touch .data_ptr
CHECKS = ADDRESS_HELPERS | {"_need", "_col", "_rows", "_like", "_out", "_word", "_host"}
NO_ARRAYS = {"__init__", "__del__", "use_stream", "sync", "set_profiling", "profile_read", "reset_parts", "set_pivot_fallback"}   # context calls: scalars only


def _functions(node):
    return [f for f in ast.walk(node) if isinstance(f, ast.FunctionDef)]


def _called(fn):
    """names a function calls as name(...) or self.name(...)"""
    out = set()
    for c in ast.walk(fn):
        if isinstance(c, ast.Call):
            f = c.func
            if isinstance(f, ast.Name):
                out.add(f.id)
            elif isinstance(f, ast.Attribute) and isinstance(f.value, ast.Name) and f.value.id == "self":
                out.add(f.attr)
    return out


def _library_calls(fn):
    """the self.L.mimsem_* calls of a function that pass anything besides the context"""
    return [c for c in ast.walk(fn) if isinstance(c, ast.Call) and isinstance(c.func, ast.Attribute) and c.func.attr.startswith("mimsem_")
            and isinstance(c.func.value, ast.Attribute) and c.func.value.attr == "L" and len(c.args) > 1]


def test_engine_wrappers_check_their_arguments_without_assert():
    tree = ast.parse(SRC.read_text())
    engine = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "Engine")
    assert not [n.lineno for n in ast.walk(engine) if isinstance(n, ast.Assert)], "assert in Engine: the check vanishes under python -O"

    inside = {id(n) for f in _functions(tree) if f.name in ADDRESS_HELPERS for n in ast.walk(f)}
    stray = [n.lineno for n in ast.walk(tree) if isinstance(n, ast.Attribute) and n.attr == "data_ptr" and id(n) not in inside]
    assert not stray, "data_ptr outside %s at lines %s" % (sorted(ADDRESS_HELPERS), stray)
    assert all(any(isinstance(n, ast.Attribute) and n.attr == "data_ptr" for n in ast.walk(f)) for f in _functions(tree) if f.name in ADDRESS_HELPERS)

    methods = {f.name: f for f in engine.body if isinstance(f, ast.FunctionDef)}
    checked = set(CHECKS)                                                 # closure: a method that calls a checking method checks
    grew = True
    while grew:
        grew = False
        for name, f in methods.items():
            if name not in checked and _called(f) & checked:
                checked.add(name); grew = True
    wrappers = [name for name, f in methods.items() if _library_calls(f) and name not in NO_ARRAYS]
    assert len(wrappers) > 60, len(wrappers)                             # the parse found the wrappers at all
    unchecked = [name for name in wrappers if not _called(methods[name]) & checked]
    assert not unchecked, "wrappers that reach the library without a check: %s" % unchecked
